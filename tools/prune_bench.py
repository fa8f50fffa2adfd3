#!/usr/bin/env python3
"""Device time of signal-to-noise pruning (FusedMLP.prune: vbnn_prune_select + vbnn_prune_pack) on the wide configuration,
784-4096-4096-10 bf16 (W = 19,988,480), against the same work composed from PyTorch-ROCm device ops on the same tensors, the
host NumPy route of tests/test_train_gpu.py, and the streaming bound of this box.

    python tools/prune_bench.py [--fraction 0.9] [--reps 20] [--warmup 3] [--out profiles/prune_bench.json]
    python tools/prune_bench.py --curve        # also the accuracy / NLL curve of a briefly trained small network

HIP events on the engine's stream in one process after a warm-up, median of the timed repetitions. The parts: `key` (vbnn_snr
of every layer -- not a step of prune(), which re-forms the keys inside its sweeps; the price of one 8 B read + 4 B write
pass), `select` (three histogram passes per layer + three one-workgroup picks), `pack` (one sweep per layer + the finish),
`prune` (FusedMLP.prune end to end on the device: select + pack; its host read-back of tau and the counts is outside the
events). Bytes the design moves per weight: 8 B read by each of the three histogram passes and by the pack, 2 x 2 B written by
the pack (bf16): 36 B, against vbnn_box_calibrate's stream-copy rate."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def curve():
    """The recipe of tests/test_train_gpu.py (synthetic digits, 64-48 hidden, three epochs, LRT f32), then prune_curve."""
    import tempfile
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    with tempfile.TemporaryDirectory() as d:
        opt = train.default_opt(network_name=os.path.join(d, "exp"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                                trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32", log=False,
                                state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
        m = train.Main(opt)
        m.run(trainSet, testSet, epochs=3)
        inputs, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
        x, t = m._to_device(inputs, targets)
        return m.net.prune_curve(x, t, [0, 0.5, 0.75, 0.9, 0.95, 0.98, 0.99, 1.0], map=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fraction", type=float, default=0.9)
    ap.add_argument("--hidden", default="4096,4096")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import _Packed, _p
    hidden = [int(h) for h in a.hidden.split(",")]
    opt = dict(var_init=1e-2, B=1e6, S=1, mode="lrt", dtype=a.dtype, seed=3, input_size=784, hidden=hidden, n_classes=10, type="vb")
    eng = FusedMLP(opt)
    for li, v in enumerate(eng.vb):                      # sigma varies per weight (the inputs of tests/test_prune_gpu.py)
        z = torch.empty_like(v.lvars)
        nn.fill_normal(z, 3, L.STREAM_INIT, li, 7)
        v.lvars.copy_(math.log(1e-2) + 0.75 * z)
    eng.prepare()
    lib, ctx, nl = L.lib(), eng.ctx.h, len(eng.vb)
    W = sum(v.O * v.I for v in eng.vb)
    k = int(math.floor(a.fraction * W))
    box = L.BoxInfo()
    L.check(lib.vbnn_box_calibrate(ctx, C.byref(box)))

    # ---- the HIP path and its parts
    mu_p = [_Packed(v.O, v.I, eng.tdt, eng.device) for v in eng.vb]
    var_p = [_Packed(v.O, v.I, eng.tdt, eng.device) for v in eng.vb]
    stats = torch.zeros(nl, 4, dtype=torch.float64, device=eng.device)
    descs = eng._prune_descs(mu_p, var_p, stats, list(range(nl)))
    nb = C.c_size_t()
    L.check(lib.vbnn_prune_workspace_bytes(nl, descs, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=eng.device)
    tau = torch.zeros(1, dtype=torch.float32, device=eng.device)
    keys = [torch.empty_like(v.means) for v in eng.vb]

    def f_key():
        for v, kk in zip(eng.vb, keys):
            L.check(lib.vbnn_snr(ctx, _p(v.means), _p(v.lvars), v.O * v.I, _p(kk)))

    def f_select():
        L.check(lib.vbnn_prune_select(ctx, nl, descs, k, _p(tau), _p(ws), nb.value))

    def f_pack():
        L.check(lib.vbnn_prune_pack(ctx, eng.code, nl, descs, _p(tau), 0.0))

    def f_prune():
        f_select()
        f_pack()
    ms = {name: event_ms(fn, a.reps, a.warmup) for name, fn in (("key", f_key), ("select", f_select), ("pack", f_pack), ("prune", f_prune))}
    t0 = time.perf_counter()
    res = eng.prune(fraction=a.fraction)
    torch.cuda.synchronize()
    ms["prune_call_wall"] = (time.perf_counter() - t0) * 1e3          # with allocation of the shadows and the read-back

    # ---- the same work from PyTorch-ROCm device ops on the same tensors
    def t_key():
        return [v.means.abs() / v.lvars.exp().sqrt() for v in eng.vb]

    def t_select(ks):
        return torch.kthvalue(torch.cat([x.reshape(-1) for x in ks]), k + 1).values

    def t_pack(ks, th):
        for v, x, m, s in zip(eng.vb, ks, mu_p, var_p):
            mask = x < th
            m.t[:, :v.I] = torch.where(mask, 0.0, v.means).to(eng.tdt)
            s.t[:, :v.I] = torch.where(mask, 0.0, v.lvars.exp()).to(eng.tdt)

    def t_prune():
        ks = t_key()
        t_pack(ks, t_select(ks))
    ks0 = t_key()
    th0 = t_select(ks0)
    tms = {"key": event_ms(t_key, a.reps, a.warmup), "select": event_ms(lambda: t_select(ks0), a.reps, a.warmup),
           "pack": event_ms(lambda: t_pack(ks0, th0), a.reps, a.warmup), "prune": event_ms(t_prune, a.reps, a.warmup)}
    same_tau = bool(np.float32(th0.item()).view(np.uint32) == np.float32(res.tau[0]).view(np.uint32))

    # ---- the host NumPy route (tests/test_train_gpu.py: the parameters downloaded, the statistic in NumPy)
    t0 = time.perf_counter()
    means = torch.cat([v.means.reshape(-1) for v in eng.vb]).cpu().numpy()
    vars_ = torch.cat([v.lvars.reshape(-1) for v in eng.vb]).exp().cpu().numpy()
    snr = np.abs(means / np.sqrt(vars_))
    th_np = np.partition(snr, k)[k]
    n_np = int((snr < th_np).sum())
    numpy_ms = (time.perf_counter() - t0) * 1e3

    esize = 2 if a.dtype == "bf16" else 4
    moved = W * (4 * 8 + 2 * esize)
    bound_ms = moved / (box.hbm_TBps * 1e12) * 1e3
    out = {"net": "784-" + "-".join(map(str, hidden)) + "-10", "dtype": a.dtype, "W": W, "fraction": a.fraction, "k": k,
           "tau": res.tau[0], "n_pruned": res.n_pruned, "mean_var": res.mean_var, "mean_pruned_var": res.mean_pruned_var,
           "hip_ms": {n: round(v, 4) for n, v in ms.items()}, "torch_ms": {n: round(v, 4) for n, v in tms.items()},
           "torch_over_hip": round(tms["prune"] / ms["prune"], 3), "same_tau_as_torch_kthvalue": same_tau,
           "numpy_host_ms": round(numpy_ms, 2), "numpy_n_pruned": n_np,
           "bytes_moved": moved, "bytes_per_weight": moved // W, "streaming_bound_ms": round(bound_ms, 4),
           "fraction_of_streaming_bound": round(bound_ms / ms["prune"], 3),
           "box": {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
                   "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus}}
    if a.curve:
        out["curve_784-64-48-10_map"] = curve()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
