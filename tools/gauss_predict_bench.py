#!/usr/bin/env python3
"""What the heteroscedastic Gaussian head costs: vbnn_gauss_nll_forward, vbnn_predict_gauss_moments and
FusedMLP.predict_regression / test() with criterion = "gauss".

    python tools/gauss_predict_bench.py [--reps 5] [--kernel-reps 20] [--rounds 5] [--out profiles/gauss_predict_bench.json]

The protocol of tools/regress_predict_bench.py: blocks of calls between HIP events (never one launch on its own), the variants
interleaved round by round, medians of the rounds, the box's held clock and stream-copy rate (vbnn_box_calibrate) beside every
figure, and the outputs asserted against float64 on the same inputs before anything is timed.

(a) ACCUMULATE at R 4096 x D 2048 (a y 4096 floats wide), one middle draw per launch, beside the MSE form at R 4096 x D 4096
    in the same process -- timed TWICE (its own spread is the allowance); each as a share of the stream-copy rate by the bytes
    its form must move (gauss: y 2 rd, t rd, state 3 rd in and 3 rd out, rd = 4 R D; mse: y, t, state 2 + 2).
(b) STACKED at R 128 x D 2048 x S 30 against the PyTorch composition on the same tensors (var_mean, exp, row sums, logsumexp).
(c) the criterion kernel at 4096 x 2048 against vbnn_mse_forward at 4096 x 4096 and the byte floor of each
    (gauss: 12 B read + 8 B written per target element; mse: 8 + 4 per output element).
(d) one predict_regression call and one test() on 784-400-400-(2 x 10), fp32, 100 rows, S = 30.
Whatever is measured is written down, including where a kernel misses the byte-derived figure."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
S_MIN, S_MAX = -20.0, 20.0


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


def _gauss_args(L, _p, y, t, R, D, S, form, state, out, tot):
    return L.GaussMomentsArgs(y=_p(y), ld_y=2 * D, target=_p(t), ld_t=D, R=R, D=D, S=S, form=form, s_min=S_MIN, s_max=S_MAX,
                              state=_p(state), mean=_p(out["mean"]), var=_p(out["var"]), noise_var=_p(out["noise_var"]), ld_out=D,
                              row_var=_p(out["row_var"]), row_noise_var=_p(out["row_noise_var"]), row_sq_err=_p(out["row_sq_err"]),
                              row_log_lik=_p(out["row_log_lik"]), totals=_p(tot))


def _outputs(R, D, gauss):
    import torch
    f32 = dict(dtype=torch.float32, device="cuda")
    keys = ["mean", "var", "row_var", "row_sq_err", "row_log_lik"] + (["noise_var", "row_noise_var"] if gauss else [])
    return {k: torch.empty((R, D) if k in ("mean", "var", "noise_var") else (R,), **f32) for k in keys}


def _assert_gauss_against_float64(got, draws, t, S, D):
    """The element and row bounds of tests/_gauss_np.py, in torch float64 on the device."""
    import torch
    y = draws.double()
    m, s = y[:, :, :D], y[:, :, D:].clamp(S_MIN, S_MAX)
    mean, var, amax = m.mean(0), m.var(0, unbiased=False), m.abs().amax(0)
    assert bool(((got["mean"].double() - mean).abs() <= max(4, S) * EPS * amax).all()), "mean"
    assert bool(((got["var"].double() - var).abs() <= 8 * EPS * (var + amax * var.sqrt() + EPS * amax * amax)).all()), "var"
    v = s.exp().mean(0)
    assert bool(((got["noise_var"].double() - v).abs() <= (S + 4) * EPS * v).all()), "noise_var"
    dw = (t.double()[None] - m) ** 2 * (-s).exp()
    nll, mag = 0.5 * (s + dw).sum(2), 0.5 * (s.abs() + dw).sum(2)
    ll = torch.logsumexp(-nll, 0) - math.log(S) - 0.5 * D * math.log(2 * math.pi)
    tl = (D + 32) * EPS * mag.amax(0) + (4 * S + 16) * EPS * ll.abs().clamp(min=1.0)
    assert bool(((got["row_log_lik"].double() - ll).abs() <= tl).all()), "row_log_lik"
    rel = (D + 16) * EPS
    for key, terms in (("row_var", got["var"]), ("row_noise_var", got["noise_var"])):
        rv = terms.double().mean(1)
        assert bool(((got[key].double() - rv).abs() <= rel * rv).all()), key
    assert abs(got["totals"][1] - float(nll.sum())) <= float((D + 32) * EPS * mag.sum() + S * EPS * nll.abs().sum()), "sum nll"


def moments_points(a, box):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    rows = []
    g = torch.Generator(device="cuda").manual_seed(5)
    # ---- (a) ACCUMULATE, one middle draw: gauss R 4096 x D 2048 beside mse R 4096 x D 4096 (the same y width)
    R, Dg, Dm, S = 4096, 2048, 4096, 8
    yg = torch.randn(S, R, 2 * Dg, generator=g, **f32)
    tg = torch.randn(R, Dg, generator=g, **f32)
    og, totg = _outputs(R, Dg, True), torch.zeros(5, dtype=torch.float64, device="cuda")
    stg = torch.empty(R, 3 * Dg + 2, **f32)
    mg = _gauss_args(L, _p, yg, tg, R, Dg, S, L.MOMENTS_ACCUMULATE, stg, og, totg)
    ym, tm = yg.view(S, R, Dm), torch.randn(R, Dm, generator=g, **f32)
    om, totm = _outputs(R, Dm, False), torch.zeros(4, dtype=torch.float64, device="cuda")
    stm = torch.empty(R, 2 * Dm + 2, **f32)
    mm = L.MomentsArgs(y=_p(ym), ld_y=Dm, target=_p(tm), ld_t=Dm, R=R, D=Dm, S=S, noise_var=0.1, state=_p(stm),
                       form=L.MOMENTS_ACCUMULATE, mean=_p(om["mean"]), var=_p(om["var"]), ld_out=Dm, row_var=_p(om["row_var"]),
                       row_sq_err=_p(om["row_sq_err"]), row_log_lik=_p(om["row_log_lik"]), totals=_p(totm))

    def gauss_draw(s):
        mg.draw, mg.y = s, C.c_void_p(yg.data_ptr() + 4 * s * R * 2 * Dg)
        L.check(lib.vbnn_predict_gauss_moments(h, C.byref(mg)))

    def mse_draw(s):
        mm.draw, mm.y = s, C.c_void_p(ym.data_ptr() + 4 * s * R * Dm)
        L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
    for s in range(S):
        gauss_draw(s)
        mse_draw(s)
    _assert_gauss_against_float64(dict(og, totals=totg.cpu().tolist()), yg, tg, S, Dg)
    ms = _interleaved({"gauss": lambda: gauss_draw(1), "mse_first": lambda: mse_draw(1), "mse_second": lambda: mse_draw(1)},
                      a.kernel_reps, a.rounds)
    rdg, rdm = 4.0 * R * Dg, 4.0 * R * Dm
    bg, bm = (2 + 1 + 3 + 3) * rdg, (1 + 1 + 2 + 2) * rdm
    share = lambda nbytes, t_ms: nbytes / (t_ms * 1e-3) / bw
    sg, s1, s2 = share(bg, ms["gauss"]), share(bm, ms["mse_first"]), share(bm, ms["mse_second"])
    allowance = abs(s1 - s2)
    rows.append({"form": "accumulate", "what": "one middle draw", "R": R, "gauss_D": Dg, "mse_D": Dm,
                 "gauss_us": round(ms["gauss"] * 1e3, 2), "mse_us": [round(ms["mse_first"] * 1e3, 2), round(ms["mse_second"] * 1e3, 2)],
                 "gauss_bytes": int(bg), "mse_bytes": int(bm), "gauss_fraction_of_stream_copy": round(sg, 4),
                 "mse_fraction_of_stream_copy": [round(s1, 4), round(s2, 4)], "allowance": round(allowance, 4),
                 "verdict": "HIT" if sg >= min(s1, s2) - allowance else "MISS"})
    del yg, tg, og, stg, ym, tm, om, stm
    # ---- (b) STACKED against the PyTorch composition
    R, D, S = 128, 2048, 30
    draws = torch.randn(S, R, 2 * D, generator=g, **f32)
    t = torch.randn(R, D, generator=g, **f32)
    out, tot = _outputs(R, D, True), torch.zeros(5, dtype=torch.float64, device="cuda")
    m = _gauss_args(L, _p, draws, t, R, D, S, L.MOMENTS_STACKED, None, out, tot)

    def kernel():
        L.check(lib.vbnn_predict_gauss_moments(h, C.byref(m)))

    def composition():
        mu, s = draws[:, :, :D], draws[:, :, D:].clamp(S_MIN, S_MAX)
        var, mean = torch.var_mean(mu, 0, unbiased=False)
        nv = s.exp().mean(0)
        nll = 0.5 * (s + (t[None] - mu) ** 2 * (-s).exp()).sum(2)
        ll = torch.logsumexp(-nll, 0)
        return mean, var, nv, var.mean(1), nv.mean(1), ((t - mean) ** 2).sum(1), ll
    kernel()
    _assert_gauss_against_float64(dict(out, totals=tot.cpu().tolist()), draws, t, S, D)
    ms = _interleaved({"kernel": kernel, "torch": composition}, a.kernel_reps, a.rounds)
    rd = 4.0 * R * D
    nbytes = S * 2 * rd + rd + 3 * rd                        # y of every draw, the targets, mean / var / noise_var out
    rows.append({"form": "stacked", "R": R, "D": D, "S": S, "kernel_us": round(ms["kernel"] * 1e3, 2),
                 "torch_composition_us": round(ms["torch"] * 1e3, 2), "kernel_over_torch": round(ms["kernel"] / ms["torch"], 4),
                 "bytes_moved": int(nbytes), "byte_floor_us": round(nbytes / bw * 1e6, 2),
                 "fraction_of_stream_copy": round(share(nbytes, ms["kernel"]), 4),
                 "kernel_over_byte_floor": round(ms["kernel"] * 1e-3 / (nbytes / bw), 2)})
    return rows


def criterion_point(a, box):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    N, D, Dm = 4096, 2048, 4096
    g = torch.Generator(device="cuda").manual_seed(9)
    y = torch.randn(N, 2 * D, generator=g, **f32)
    y[:, D:] *= 4.0
    t, tm = torch.randn(N, D, generator=g, **f32), torch.randn(N, Dm, generator=g, **f32)
    grad = torch.empty(N, 2 * D, **f32)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    inv_g, inv_m = 1.0 / (N * D), 1.0 / (N * Dm)

    def gauss():
        L.check(lib.vbnn_gauss_nll_forward(h, _p(y), 2 * D, _p(t), D, N, D, inv_g, S_MIN, S_MAX, _p(grad), 2 * D, 0, _p(loss)))

    def mse():
        L.check(lib.vbnn_mse_forward(h, _p(y), Dm, _p(tm), Dm, N, Dm, inv_m, _p(grad), Dm, 0, _p(loss)))
    gauss()
    m64, s64, t64 = y[:, :D].double(), y[:, D:].double().clamp(S_MIN, S_MAX), t.double()
    w, inv32 = (-s64).exp(), float(torch.tensor(inv_g, dtype=torch.float32))
    dw = (t64 - m64) ** 2 * w
    want = inv32 * float((0.5 * (s64 + dw)).sum())
    assert abs(float(loss.cpu()) - want) <= 8 * EPS * inv32 * float((0.5 * (s64.abs() + dw)).sum()), "loss"
    gm = inv32 * (m64 - t64) * w
    assert bool(((grad[:, :D].double() - gm).abs() <= 8 * EPS * gm.abs()).all()), "g_m"
    gs = torch.where((y[:, D:] < S_MIN) | (y[:, D:] > S_MAX), torch.zeros_like(dw), 0.5 * inv32 * (1 - dw))
    assert bool(((grad[:, D:].double() - gs).abs() <= 8 * EPS * 0.5 * inv32 * (1 + dw)).all()), "g_s"
    ms = _interleaved({"gauss": gauss, "mse": mse}, a.kernel_reps, a.rounds)
    bg, bm = 20.0 * N * D, 12.0 * N * Dm
    return {"N": N, "gauss_D": D, "mse_D": Dm, "gauss_us": round(ms["gauss"] * 1e3, 2), "mse_us": round(ms["mse"] * 1e3, 2),
            "gauss_bytes": int(bg), "mse_bytes": int(bm), "gauss_byte_floor_us": round(bg / bw * 1e6, 2),
            "mse_byte_floor_us": round(bm / bw * 1e6, 2),
            "gauss_fraction_of_stream_copy": round(bg / (ms["gauss"] * 1e-3) / bw, 4),
            "mse_fraction_of_stream_copy": round(bm / (ms["mse"] * 1e-3) / bw, 4)}


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
    res = eng.predict_regression(x, targets=t)
    err, _ = eng.test(x, t)
    ms = _interleaved({"predict_regression": lambda: eng.predict_regression(x, targets=t), "test": lambda: eng.test(x, t)},
                      a.reps, a.rounds)
    return {"net": f"784-400-400-(2x{D})", "dtype": "f32", "R": R, "S": S, "stacked": res.stacked,
            "predict_regression_ms": round(ms["predict_regression"], 4), "test_ms": round(ms["test"], 4),
            "predict_over_test": round(ms["predict_regression"] / ms["test"], 4),
            "mean_draw_nll": res.mean_draw_nll, "test_error": err, "log_lik": res.log_lik, "mean_var": res.mean_var,
            "mean_noise_var": res.mean_noise_var}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_predict_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    box, box_d = _box(L, Context.get().h)
    out = {"reps": a.reps, "kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d}
    out["moments"] = moments_points(a, box)
    out["criterion"] = criterion_point(a, box)
    out["engine"] = engine_point(a)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
