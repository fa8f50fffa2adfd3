#!/usr/bin/env python3
"""What the regression posterior predictive (FusedMLP.predict_regression over vbnn_predict_moments) costs.

    python tools/regress_predict_bench.py [--reps 5] [--rounds 5] [--out profiles/regress_predict_bench.json]
    python tools/regress_predict_bench.py --skip-engine | --skip-kernel

(a) predict_regression against test() on the same inputs and S = 30: BASELINE configs[4] (4096-[4096]x8-4096, bf16, 4096 rows)
and a launch-bound point (784-400-400 with D = 10, fp32, 100 rows). ms per call (HIP events around `reps` calls, median of the
rounds, the two interleaved) and the share of the call that is the moments kernel: the same vbnn_predict_moments launches the
call issues, timed as a block on the same buffers.

(b) the kernel alone: STACKED at (R 128, D 4096, S 30) and ACCUMULATE at (R 4096, D 4096; one middle draw per launch, and the
S = 8 launches of a whole prediction), with targets and a noise variance. us per launch from blocks of launches (never one
launch on its own), the bytes the form must move (y, targets, state in and out, the outputs of a finish) over the box's measured
stream-copy rate (vbnn_box_calibrate), and beside them the same quantities from PyTorch device ops on the same tensors:
torch.var_mean(draws, 0, unbiased=False), the squared-error row sums and torch.logsumexp. Before anything is timed the kernel's
outputs are asserted against float64 on the same inputs at the tolerances of tests/test_predict_regression_gpu.py.
Whatever is measured is written down, including where the kernel misses the byte-derived figure."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _block_ms(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _interleaved(fns, n, rounds):
    """median over `rounds` of ms per call, the variants alternating round by round (one warm-up round)."""
    times = {k: [] for k in fns}
    for rnd in range(rounds + 1):
        for k, fn in fns.items():
            ms = _block_ms(fn, n)
            if rnd:
                times[k].append(ms)
    return {k: statistics.median(v) for k, v in times.items()}


def _box(L, h):
    box = L.BoxInfo()
    L.check(L.lib().vbnn_box_calibrate(h, C.byref(box)))
    return box, {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
                 "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus}


ENGINE_POINTS = {
    "configs4": dict(input_size=4096, hidden=[4096] * 8, D=4096, dtype="bf16", R=4096, S=30),
    "launch_bound": dict(input_size=784, hidden=[400, 400], D=10, dtype="f32", R=100, S=30),
}


def engine_point(name, a):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import _p
    p = ENGINE_POINTS[name]
    R, D, S = p["R"], p["D"], p["S"]
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype=p["dtype"], seed=3, input_size=p["input_size"], hidden=p["hidden"],
               n_classes=D, criterion="mse", type="vb", testSamples=S)
    eng = FusedMLP(opt)
    eng.prepare()
    x = torch.empty(R, p["input_size"], dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    res = eng.predict_regression(x, targets=t, noise_var=0.1)
    err, _ = eng.test(x, t)
    lib, h = L.lib(), eng.ctx.h
    # the moments launches of one call, alone: the forms and shapes predict_regression issued (res.stacked, one chunk)
    f32 = dict(dtype=torch.float32, device="cuda")
    one_call = res.stacked and D <= L.MOMENTS_STACKED_MAX_D
    y = torch.randn((S * R) if res.stacked else R, D, **f32)
    state = None if one_call else torch.empty(R, 2 * D + 2, **f32)
    out = [torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, **f32), torch.empty(R, **f32), torch.empty(R, **f32)]
    tot = torch.zeros(4, dtype=torch.float64, device="cuda")
    m = L.MomentsArgs(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, noise_var=0.1, state=_p(state),
                      form=L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE, mean=_p(out[0]), var=_p(out[1]), ld_out=D,
                      row_var=_p(out[2]), row_sq_err=_p(out[3]), row_log_lik=_p(out[4]), totals=_p(tot))

    def moments():
        with eng._on_stream():
            if one_call:
                L.check(lib.vbnn_predict_moments(h, C.byref(m)))
                return
            for s in range(S):
                m.draw = s
                if res.stacked:
                    m.y = C.c_void_p(y.data_ptr() + 4 * s * R * D)
                L.check(lib.vbnn_predict_moments(h, C.byref(m)))
    assert res.chunks == 1
    ms = _interleaved({"predict_regression": lambda: eng.predict_regression(x, targets=t, noise_var=0.1),
                       "test": lambda: eng.test(x, t), "moments": moments}, a.reps, a.rounds)
    return {"point": name, "net": f"{p['input_size']}-" + "-".join(map(str, p["hidden"])) + f"-{D}", "dtype": p["dtype"], "R": R, "S": S,
            "stacked": res.stacked, "moments_launches_per_call": 1 if one_call else S,
            "predict_regression_ms": round(ms["predict_regression"], 4), "test_ms": round(ms["test"], 4),
            "predict_over_test": round(ms["predict_regression"] / ms["test"], 4),
            "moments_ms_per_call": round(ms["moments"], 5), "moments_share_of_call": round(ms["moments"] / ms["predict_regression"], 4),
            "mean_draw_mse": res.mean_draw_mse, "test_error": err, "mse": res.mse, "log_lik": res.log_lik, "mean_var": res.mean_var}


def _assert_against_float64(got, draws, t, tau2, S, D):
    import torch
    y = draws.double()
    mean, var, amax = y.mean(0), y.var(0, unbiased=False), y.abs().amax(0)
    assert bool(((got["mean"].double() - mean).abs() <= max(4, S) * EPS * amax).all()), "mean"
    assert bool(((got["var"].double() - var).abs() <= 8 * EPS * (var + amax * var.sqrt() + EPS * amax * amax)).all()), "var"
    e = ((t.double()[None] - y) ** 2).sum(2)
    ll = torch.logsumexp(-e / (2 * tau2), 0) - math.log(S) - 0.5 * D * math.log(2 * math.pi * tau2)
    d = (got["row_log_lik"].double() - ll).abs() / ll.abs().clamp(min=1.0)
    assert float(d.max()) <= (D + 4 * S + 16) * EPS and float(d.median()) <= 16 * EPS, ("row_log_lik", float(d.max()) / EPS)
    rel = (D + 16) * EPS
    sq = ((t.double() - got["mean"].double()) ** 2).sum(1)
    assert bool(((got["row_sq_err"].double() - sq).abs() <= rel * sq).all()), "row_sq_err"
    rv = got["var"].double().mean(1)
    assert bool(((got["row_var"].double() - rv).abs() <= rel * rv).all()), "row_var"
    assert abs(got["totals"][1] - float(e.sum())) <= rel * float(e.sum()), "sum e"


def kernel_points(a):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    box, box_d = _box(L, h)
    f32 = dict(dtype=torch.float32, device="cuda")
    tau2 = 0.1
    c = 0.5 / tau2
    rows = []
    for form, R, D, S in (("stacked", 128, 4096, 30), ("accumulate", 4096, 4096, 8)):
        g = torch.Generator(device="cuda").manual_seed(5)
        draws = torch.randn(S, R, D, generator=g, **f32)
        t = torch.randn(R, D, generator=g, **f32)
        out = {"mean": torch.empty(R, D, **f32), "var": torch.empty(R, D, **f32), "row_var": torch.empty(R, **f32),
               "row_sq_err": torch.empty(R, **f32), "row_log_lik": torch.empty(R, **f32)}
        tot = torch.zeros(4, dtype=torch.float64, device="cuda")
        state = torch.empty(R, 2 * D + 2, **f32) if form == "accumulate" else None
        m = L.MomentsArgs(y=_p(draws), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, noise_var=tau2, state=_p(state),
                          form=L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE, mean=_p(out["mean"]),
                          var=_p(out["var"]), ld_out=D, row_var=_p(out["row_var"]), row_sq_err=_p(out["row_sq_err"]),
                          row_log_lik=_p(out["row_log_lik"]), totals=_p(tot))

        def launch(s):
            m.draw = s
            m.y = C.c_void_p(draws.data_ptr() + 4 * s * R * D)
            L.check(lib.vbnn_predict_moments(h, C.byref(m)))

        def whole():
            if form == "stacked":
                launch(0)
            else:
                for s in range(S):
                    launch(s)

        def composition():                                   # three passes over the draws, PyTorch device ops
            var, mean = torch.var_mean(draws, 0, unbiased=False)
            e = ((t[None] - draws) ** 2).sum(2)
            ll = torch.logsumexp(e * (-c), 0)
            return mean, var, e, ll
        whole()
        got = dict(out, totals=tot.cpu().tolist())
        _assert_against_float64(got, draws, t, tau2, S, D)
        mean_t, var_t, _, _ = composition()
        torch_err = float((mean_t.double() - draws.double().mean(0)).abs().max())
        fns = {"kernel": whole, "torch": composition}
        if form == "accumulate":
            fns["middle_draw"] = lambda: launch(1)
        ms = _interleaved(fns, a.kernel_reps, a.rounds)
        rd = 4.0 * R * D
        if form == "stacked":
            nbytes = S * rd + rd + 2 * rd                    # y of every draw, the targets, mean and var out
        else:
            nbytes = (S - 1) * 2 * rd + S * (rd + rd + 2 * rd) + 2 * rd   # state in (not draw 0), y + t + state out per draw, the finish's outputs
        row = {"form": form, "R": R, "D": D, "S": S, "launches": 1 if form == "stacked" else S,
               "kernel_us": round(ms["kernel"] * 1e3, 2), "torch_composition_us": round(ms["torch"] * 1e3, 2),
               "kernel_over_torch": round(ms["kernel"] / ms["torch"], 4), "bytes_moved": int(nbytes),
               "byte_floor_us": round(nbytes / (box.hbm_TBps * 1e12) * 1e6, 2),
               "fraction_of_stream_copy": round(nbytes / (ms["kernel"] * 1e-3) / (box.hbm_TBps * 1e12), 4),
               "torch_bytes_at_least": int(3 * S * rd), "torch_max_mean_error_vs_float64": torch_err}
        if form == "accumulate":
            mid = 2 * rd + rd + rd + 2 * rd                  # state in, y, t, state out
            row["middle_draw_us"] = round(ms["middle_draw"] * 1e3, 2)
            row["middle_draw_bytes"] = int(mid)
            row["middle_draw_fraction_of_stream_copy"] = round(mid / (ms["middle_draw"] * 1e-3) / (box.hbm_TBps * 1e12), 4)
        rows.append(row)
        del draws, t, out, state
    return rows, box_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches (or whole predictions) per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regress_predict_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"reps": a.reps, "kernel_reps": a.kernel_reps, "rounds": a.rounds}
    if not a.skip_kernel:
        out["kernel"], out["box"] = kernel_points(a)
    if not a.skip_engine:
        out["engine"] = [engine_point(name, a) for name in ENGINE_POINTS]
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
