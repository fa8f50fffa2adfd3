#!/usr/bin/env python3
"""Wall time of FusedMLP.predict against FusedMLP.test on the same inputs and S, one measurement point per process.

    python tools/predict_bench.py            # every point, each in a child process under its own time limit
    python tools/predict_bench.py --point a  # one point in this process

Points: (a) the reference's test point, 784-10-10, R = 100, S = 30, fp32 (config.lua:12,33); (b) 784-400-400-10, R = 256,
S = 30, fp32; (c) the wide bf16 net, 784-4096-4096-10, R = 4096, S = 30, predict stacked and sequential. Prints one JSON line
per point: ms per call (host clock around device-synchronised calls, median of the timed calls) and predictions per second."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = {
    "a": dict(hidden=[10], R=100, S=30, dtype="f32", forms=["auto"]),
    "b": dict(hidden=[400, 400], R=256, S=30, dtype="f32", forms=["auto"]),
    "c": dict(hidden=[4096, 4096], R=4096, S=30, dtype="bf16", forms=[True, False]),
}


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def run_point(name, reps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    p = POINTS[name]
    out = []
    for form in p["forms"]:
        opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype=p["dtype"], seed=3, input_size=784, hidden=p["hidden"],
                   n_classes=10, type="vb", testSamples=p["S"], predict_stacked=form)
        eng = FusedMLP(opt)
        eng.prepare()
        x = torch.empty(p["R"], 784, dtype=torch.float32, device="cuda")
        nn.fill_normal(x, 3, 4, 0, 0)
        t = eng.synthetic_targets(x)
        ms_test = timed(lambda: eng.test(x, t), reps, warmup)
        ms_pred = timed(lambda: eng.predict(x, targets=t), reps, warmup)
        r = eng.predict(x, targets=t)
        out.append({"point": name, "net": "784-" + "-".join(map(str, p["hidden"])) + "-10", "R": p["R"], "S": p["S"],
                    "dtype": p["dtype"], "stacked": r.stacked, "predict_ms": round(ms_pred, 4), "test_ms": round(ms_test, 4),
                    "speedup": round(ms_test / ms_pred, 2), "predictions_per_s": round(p["R"] / (ms_pred * 1e-3), 1),
                    "test_rows_per_s": round(p["R"] / (ms_test * 1e-3), 1)})
        del eng
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=sorted(POINTS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per point (child process)")
    a = ap.parse_args()
    if a.point:
        for line in run_point(a.point, a.reps, a.warmup):
            print(json.dumps(line), flush=True)
        return 0
    for name in sorted(POINTS):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--point", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(json.dumps({"point": name, "error": f"exit status {rc}"}), flush=True)
            return rc                       # nothing more on the GPU after a failed point
    return 0


if __name__ == "__main__":
    sys.exit(main())
