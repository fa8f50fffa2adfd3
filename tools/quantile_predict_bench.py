#!/usr/bin/env python3
"""What the regression predictive's quantiles cost: vbnn_predict_quantiles and FusedMLP.predict_quantiles.

    python tools/quantile_predict_bench.py [--reps 5] [--kernel-reps 10] [--rounds 5] [--out profiles/quantile_predict_bench.json]

The protocol of tools/gauss_predict_bench.py: blocks of calls between HIP events (never one launch on its own), the variants
interleaved round by round, medians of the rounds, the box's held clock and stream-copy rate (vbnn_box_calibrate) beside every
figure, and the outputs asserted against float64 on the same inputs before anything is timed.

(a) EMPIRICAL at R 4096 x D 4096 x S 30, Q 2, against torch.quantile on the same tensor (in row blocks: torch.quantile takes at
    most 2^24 elements a call), and its share of the stream-copy rate by the bytes it must move (every draw once, the Q planes
    out) -- beside the MSE ACCUMULATE moments kernel at R 4096 x D 4096 timed TWICE in the same process: that kernel's own
    spread is the allowance. HIT or MISS.
(b) GAUSS and FIXED_NOISE at R 1024 x D 1000 x S 30, Q 2, with targets, against a PyTorch bisection on torch.special.erfc in
    fp32 run until the bracket is a few floats wide (40 halvings of the same starting bracket).
(c) one predict_quantiles call against one predict_regression call on 784-400-400-(2 x 10), fp32, 100 rows, S = 30.
Whatever is measured is written down, including where a kernel misses the byte-derived figure."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_F = 4 * 4.39e-07             # the allowance of F's fp32 evaluation, as measured in tests/_quantiles_np.py
S_MIN, S_MAX = -20.0, 20.0
PROBS = (0.05, 0.95)


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


def _quant_args(L, _p, y, W, R, D, S, kind, q, t=None, pit=None, row_le=None, count=None, noise_var=0.0):
    a = L.QuantilesArgs(y=_p(y), ld_y=W, draw_stride=R * W, R=R, D=D, S=S, kind=kind, Q=len(PROBS), noise_var=noise_var,
                        s_min=S_MIN, s_max=S_MAX, q=_p(q), ld_q=D, plane_stride=R * D, target=_p(t), ld_t=D, pit=_p(pit), ld_pit=D,
                        row_le=_p(row_le), count_le=_p(count))
    for j, v in enumerate(PROBS):
        a.p[j] = v
    return a


def empirical_point(a, box):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    R, D, S, Qn = 4096, 4096, 30, len(PROBS)
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn(S, R, D, generator=g, **f32)
    q = torch.empty(Qn, R, D, **f32)
    qa = _quant_args(L, _p, y, D, R, D, S, L.QUANT_EMPIRICAL, q)
    p32 = torch.tensor(PROBS, dtype=torch.float32)
    block = max(1, (1 << 24) // (S * D))                     # rows per torch.quantile call
    qt = torch.empty(Qn, R, D, **f32)

    def kernel():
        L.check(lib.vbnn_predict_quantiles(h, C.byref(qa)))

    def torch_quantile():
        pd = p32.cuda()
        for r0 in range(0, R, block):
            qt[:, r0:r0 + block] = torch.quantile(y[:, r0:r0 + block], pd, dim=0)
    kernel()
    rows = 64                                                # against float64 on a row block: fp32 rounding of the values and of
    ref = torch.quantile(y[:, :rows].double(), p32.double().cuda(), dim=0)             # the position p (S - 1) times the gap
    spread = y[:, :rows].amax(0) - y[:, :rows].amin(0)
    tol = 4 * 2.0 ** -23 * y[:, :rows].abs().amax(0) + 2.0 ** -19 * spread
    assert bool(((q[:, :rows].double() - ref).abs() <= tol[None]).all()), "empirical quantiles"
    # the MSE ACCUMULATE moments kernel, one middle draw, twice (tools/gauss_predict_bench.py's yardstick)
    t = torch.randn(R, D, generator=g, **f32)
    st = torch.empty(R, 2 * D + 2, **f32)
    om = {k: torch.empty((R, D) if k in ("mean", "var") else (R,), **f32) for k in ("mean", "var", "row_var", "row_sq_err", "row_log_lik")}
    tot = torch.zeros(4, dtype=torch.float64, device="cuda")
    mm = L.MomentsArgs(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, noise_var=0.1, state=_p(st), form=L.MOMENTS_ACCUMULATE,
                       mean=_p(om["mean"]), var=_p(om["var"]), ld_out=D, row_var=_p(om["row_var"]), row_sq_err=_p(om["row_sq_err"]),
                       row_log_lik=_p(om["row_log_lik"]), totals=_p(tot))

    def mse_draw(s=1):
        mm.draw, mm.y = s, C.c_void_p(y.data_ptr() + 4 * s * R * D)
        L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    ms = _interleaved({"kernel": kernel, "mse_first": mse_draw, "mse_second": mse_draw}, a.kernel_reps, a.rounds)
    ms_t = _interleaved({"torch": torch_quantile}, max(1, a.kernel_reps // 5), max(1, a.rounds // 2))
    rd = 4.0 * R * D
    nbytes, bm = (S + Qn) * rd, (1 + 1 + 2 + 2) * rd
    share = lambda nb, t_ms: nb / (t_ms * 1e-3) / bw
    sk, s1, s2 = share(nbytes, ms["kernel"]), share(bm, ms["mse_first"]), share(bm, ms["mse_second"])
    allowance = abs(s1 - s2)
    return {"kind": "empirical", "R": R, "D": D, "S": S, "Q": Qn, "kernel_us": round(ms["kernel"] * 1e3, 2),
            "torch_quantile_us": round(ms_t["torch"] * 1e3, 2), "torch_quantile_calls": (R + block - 1) // block,
            "kernel_over_torch": round(ms["kernel"] / ms_t["torch"], 4), "bytes_moved": int(nbytes),
            "byte_floor_us": round(nbytes / bw * 1e6, 2), "fraction_of_stream_copy": round(sk, 4),
            "mse_accumulate_us": [round(ms["mse_first"] * 1e3, 2), round(ms["mse_second"] * 1e3, 2)],
            "mse_fraction_of_stream_copy": [round(s1, 4), round(s2, 4)], "allowance": round(allowance, 4),
            "verdict": "HIT" if sk >= min(s1, s2) - allowance else "MISS"}


def mixture_points(a, box):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    R, D, S, Qn = 1024, 1000, 30, len(PROBS)
    g = torch.Generator(device="cuda").manual_seed(7)
    out = []
    for name, kind, W, tau2 in (("gauss", L.QUANT_GAUSS, 2 * D, 0.0), ("fixed_noise", L.QUANT_FIXED_NOISE, D, 0.3)):
        y = torch.randn(S, R, W, generator=g, **f32)
        if name == "gauss":
            y[:, :, D:] = 2.0 * y[:, :, D:] - 2.0            # log variances around -2
        mu = y[:, :, :D]
        sigma = (0.5 * y[:, :, D:].clamp(S_MIN, S_MAX)).exp() if name == "gauss" else torch.full_like(mu, math.sqrt(tau2))
        pick = torch.randint(0, S, (1, R, D), generator=g, device="cuda")
        t = (mu.gather(0, pick) + sigma.gather(0, pick) * torch.randn(1, R, D, generator=g, **f32))[0].contiguous()
        q, pit = torch.empty(Qn, R, D, **f32), torch.empty(R, D, **f32)
        row_le, count = torch.empty(R, Qn, dtype=torch.int32, device="cuda"), torch.zeros(Qn, dtype=torch.int64, device="cuda")
        qa = _quant_args(L, _p, y, W, R, D, S, kind, q, t, pit, row_le, count, noise_var=tau2)
        c = 1.0 / (sigma * math.sqrt(2.0))

        def kernel():
            L.check(lib.vbnn_predict_quantiles(h, C.byref(qa)))

        def cdf(x, m=mu, cc=c):
            return 0.5 * torch.special.erfc((m - x[None]) * cc).mean(0)

        def torch_bisection():
            lo0, hi0 = (mu - 3.5 * sigma).amin(0), (mu + 3.5 * sigma).amax(0)
            res = []
            for pj in PROBS:
                lo, hi = lo0.clone(), hi0.clone()
                for _ in range(40):
                    mid = 0.5 * (lo + hi)
                    below = cdf(mid) < pj
                    lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
                res.append(hi)
            return torch.stack(res), cdf(t), torch.stack([(t <= r).sum() for r in res])
        kernel()
        # the header's criterion against float64: F(q - 2 ulp) - eps_F <= p <= F(q + 2 ulp) + eps_F, and pit = F(t) within eps_F
        mu64, c64 = mu.double(), 1.0 / (sigma.double() * math.sqrt(2.0))
        inf = torch.tensor(float("inf"), **f32)
        for j, pj in enumerate(PROBS):
            p32 = float(torch.tensor(pj, dtype=torch.float32))
            down, up = q[j], q[j]
            for _ in range(2):
                down, up = torch.nextafter(down, -inf), torch.nextafter(up, inf)
            assert bool((cdf(down.double(), mu64, c64) - EPS_F <= p32).all() and (cdf(up.double(), mu64, c64) + EPS_F >= p32).all()), name
        assert bool(((pit.double() - cdf(t.double(), mu64, c64)).abs() <= EPS_F).all()), name + " pit"
        cal = (count.cpu().double() / (R * D)).tolist()
        ms = _interleaved({"kernel": kernel}, a.kernel_reps, a.rounds)
        ms_t = _interleaved({"torch": torch_bisection}, 1, max(1, a.rounds // 2))
        nbytes = 4.0 * R * (S * W + (Qn + 2) * D)            # every draw once, the targets in, the Q planes and the PIT out
        out.append({"kind": name, "R": R, "D": D, "S": S, "Q": Qn, "kernel_us": round(ms["kernel"] * 1e3, 2),
                    "torch_bisection_us": round(ms_t["torch"] * 1e3, 2), "kernel_over_torch": round(ms["kernel"] / ms_t["torch"], 5),
                    "bytes_moved": int(nbytes), "byte_floor_us": round(nbytes / bw * 1e6, 2),
                    "kernel_over_byte_floor": round(ms["kernel"] * 1e-3 / (nbytes / bw), 2),
                    "ns_per_element_quantile": round(ms["kernel"] * 1e6 / (R * D * Qn), 3), "calibration": cal})
    return out


def engine_point(a):
    import torch
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    R, D, S = 100, 10, 30
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=784, hidden=[400, 400], n_classes=2 * D,
               criterion="gauss", type="vb", testSamples=S)
    eng = FusedMLP(opt)
    eng.prepare()
    x = torch.empty(R, 784, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    res = eng.predict_quantiles(x, PROBS, targets=t)
    ms = _interleaved({"predict_quantiles": lambda: eng.predict_quantiles(x, PROBS, targets=t),
                       "predict_regression": lambda: eng.predict_regression(x, targets=t)}, a.reps, a.rounds)
    return {"net": f"784-400-400-(2x{D})", "dtype": "f32", "R": R, "S": S, "stacked": res.moments.stacked,
            "predict_quantiles_ms": round(ms["predict_quantiles"], 4), "predict_regression_ms": round(ms["predict_regression"], 4),
            "quantiles_over_regression": round(ms["predict_quantiles"] / ms["predict_regression"], 4),
            "calibration": res.calibration, "interval_0.9": list(res.interval(0.9)[2:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=10, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_predict_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    box, box_d = _box(L, Context.get().h)
    out = {"reps": a.reps, "kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d}
    out["empirical"] = empirical_point(a, box)
    out["mixture"] = mixture_points(a, box)
    out["engine"] = engine_point(a)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
