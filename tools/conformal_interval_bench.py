#!/usr/bin/env python3
"""What conformal intervals cost (vbnn_conformal_interval, vbnn_select_columns; csrc/conformal_interval.hip).

    python tools/conformal_interval_bench.py [--kernel-reps 10] [--rounds 5] [--out profiles/conformal_interval_bench.json]

The family's protocol (tools/calibration_bench.py): before anything is timed every output is asserted BIT FOR BIT against the
restatement of tests/_interval_np.py on the same inputs; us per launch come from blocks of launches between HIP events, the
variants interleaved, medians of the rounds; the box's held clock and stream-copy rate (vbnn_box_calibrate) are recorded, and
the MSE form's ACCUMULATE middle draw (vbnn_predict_moments at R 4096 x D 4096) is timed twice beside every point as the
yardstick: its spread between the two timings is the allowance.

Streaming points: R 4096 x D 4096 and R 65536 x D 10, the "scaled" score (mean, variance, target in), Q = 1 and Q = 3 thresholds
per output, lo / hi written; and score mode at the same shapes. Byte floor = (3 + 2 Q) planes (score mode: 4). The expectation
is the MSE kernel's share of the stream-copy rate less its spread (`meets_mse_share`). Beside them a PyTorch composition of
elementwise ops on the same tensors.
Select points: R 10^4 x D 4096, 10^5 x 10 and 10^6 x 1, Q = 1 and Q = 3 ranks; byte floor = 4 ceil(Q / U) reads of the matrix
(U = 4); beside it torch.kthvalue along dim 0 as given and on the contiguous transpose. Recorded, not judged.
A whole conformal_calibrate_intervals and conformal_intervals call at 65536 x 10 by the host clock.
Whatever is measured is written down, including where a kernel misses."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = {1: (0.9,), 3: (0.5, 0.9, 0.99)}


def _yardstick(L, h, g):
    import torch
    from vbnn_amd.nn import _p
    f32 = dict(dtype=torch.float32, device="cuda")
    Ry = Dy = 4096
    draws = torch.randn(2, Ry, Dy, generator=g, **f32)
    tt = torch.randn(Ry, Dy, generator=g, **f32)
    st2 = torch.empty(Ry, 2 * Dy + 2, **f32)
    mm = L.MomentsArgs(y=_p(draws), ld_y=Dy, target=_p(tt), ld_t=Dy, R=Ry, D=Dy, S=4, noise_var=0.1, state=_p(st2),
                       form=L.MOMENTS_ACCUMULATE, ld_out=Dy)

    def mse_draw(s=1):
        mm.draw = s
        mm.y = C.c_void_p(draws.data_ptr() + 4 * s * Ry * Dy)
        L.check(L.lib().vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    return mse_draw, 6 * 4.0 * Ry * Dy, (draws, tt, st2, mm)


def streaming_points(a, L, h, rate, mse_draw, mse_bytes):
    import numpy as np
    import torch
    from calibration_bench import _interleaved
    from tests._interval_np import W_MIN, calibrate32, interval32, score32, width32
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    f32 = dict(dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    for R, D in ((4096, 4096), (65536, 10)):
        mean = torch.randn(R, D, generator=g, **f32)
        var = torch.rand(R, D, generator=g, **f32) + 0.05
        t = mean + torch.randn(R, D, generator=g, **f32) * var.sqrt() * 1.5
        mh, vh, th = mean.cpu().numpy(), var.cpu().numpy(), t.cpu().numpy()
        w = width32(vh, None, 0.0, True, W_MIN)
        want_s = score32(mh[None], mh[None], th, w)
        score, row_score = torch.empty(1, R, D, **f32), torch.empty(1, R, **f32)
        sacc = torch.zeros(2, dtype=torch.int64, device="cuda")
        base = dict(lower=_p(mean), upper=_p(mean), ld=D, P=1, scale=_p(var), ld_s=D, scale_is_variance=1, w_min=W_MIN,
                    target=_p(t), ld_t=D, R=R, D=D)
        sm = L.ConformalIntervalArgs(Q=0, score=_p(score), row_score=_p(row_score), acc=_p(sacc), **base)
        score_fn = lambda sm=sm: L.check(lib.vbnn_conformal_interval(h, C.byref(sm)))
        score_fn()
        assert score.cpu().numpy().tobytes() == want_s["score"].tobytes() and row_score.cpu().numpy().tobytes() == want_s["row_score"].tobytes()
        for Q in (1, 3):
            qhat, _ = calibrate32(want_s["score"][0], LEVELS[Q])
            qd = torch.from_numpy(qhat).cuda()
            lo, hi = torch.empty(Q, R, D, **f32), torch.empty(Q, R, D, **f32)
            acc = torch.zeros(8 * Q + 2, dtype=torch.int64, device="cuda")
            m = L.ConformalIntervalArgs(Q=Q, qhat=_p(qd), ld_qhat=D, per_column=1, lo=_p(lo), hi=_p(hi), acc=_p(acc), **base)
            fn = lambda m=m: L.check(lib.vbnn_conformal_interval(h, C.byref(m)))
            fn()
            want = interval32(mh[None], mh[None], qhat, th, w)
            assert np.array_equal(acc.cpu().numpy().view(np.uint64), want["acc"]), (R, D, Q, "acc")
            assert lo.cpu().numpy().tobytes() == want["lo"].tobytes() and hi.cpu().numpy().tobytes() == want["hi"].tobytes(), (R, D, Q)

            def torch_interval(qd=qd):                       # PyTorch device ops on the same tensors
                ww = var.sqrt().clamp_min(W_MIN)
                s = (t - mean).abs() / ww
                qw = qd[:, None, :] * ww[None]
                return mean[None] - qw, mean[None] + qw, (s[None] <= qd[:, None, :]).sum((1, 2))

            def torch_score():
                s = (t - mean).abs() / var.sqrt().clamp_min(W_MIN)
                return s, s.max(1).values
            fns = {"mse_a": mse_draw, "interval": fn, "score": score_fn, "torch_interval": torch_interval, "torch_score": torch_score,
                   "mse_b": mse_draw}
            ms = _interleaved(fns, a.kernel_reps, a.rounds)
            mse = [mse_bytes / (ms[k] * 1e-3) / rate for k in ("mse_a", "mse_b")]
            spread = abs(mse[0] - mse[1])
            nbytes = {"interval": (3 + 2 * Q) * 4.0 * R * D, "score": 4 * 4.0 * R * D}
            share = {k: nbytes[k] / (ms[k] * 1e-3) / rate for k in nbytes}
            row = {"R": R, "D": D, "Q": Q, "bytes": {k: int(v) for k, v in nbytes.items()},
                   "byte_floor_us": {k: round(v / rate * 1e6, 2) for k, v in nbytes.items()},
                   "mse_middle_draw_us": [round(ms["mse_a"] * 1e3, 2), round(ms["mse_b"] * 1e3, 2)],
                   "mse_fraction_of_stream_copy": [round(v, 4) for v in mse], "mse_spread": round(spread, 4),
                   "interval_us": round(ms["interval"] * 1e3, 2), "score_us": round(ms["score"] * 1e3, 2),
                   "torch_interval_us": round(ms["torch_interval"] * 1e3, 2), "torch_score_us": round(ms["torch_score"] * 1e3, 2),
                   "fraction_of_stream_copy": {k: round(v, 4) for k, v in share.items()},
                   "meets_mse_share": {k: bool(v >= min(mse) - spread) for k, v in share.items()},
                   "coverage": [int(want["acc"][8 * j + 1]) / int(want["acc"][8 * j]) for j in range(Q)]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fns, lo, hi
        del mean, var, t, score
    return rows


def select_points(a, L, h, rate, mse_draw, mse_bytes):
    import numpy as np
    import torch
    from calibration_bench import _interleaved
    from tests._interval_np import conformal_rank, select_columns32
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    f32 = dict(dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(9)
    for R, D in ((10000, 4096), (100000, 10), (1000000, 1)):
        x = torch.randn(R, D, generator=g, **f32).abs()
        xt = x.t().contiguous()
        xh = x.cpu().numpy()
        for Q in (1, 3):
            ks = [conformal_rank(R, lv) for lv in LEVELS[Q]]
            tau = torch.empty(Q, D, **f32)
            cnt = torch.empty(Q, D, 2, dtype=torch.int32, device="cuda")
            nn = torch.empty(D, dtype=torch.int32, device="cuda")
            m = L.SelectColumnsArgs(x=_p(x), ld=D, R=R, D=D, Q=Q, tau=_p(tau), ld_tau=D, counts=_p(cnt), n_nan=_p(nn))
            for j, k in enumerate(ks):
                m.k[j] = k
            fn = lambda m=m: L.check(lib.vbnn_select_columns(h, C.byref(m)))
            fn()
            want = select_columns32(xh, ks)
            assert tau.cpu().numpy().tobytes() == want["tau"].tobytes(), (R, D, Q, "tau")
            assert cnt.cpu().numpy().view(np.uint32).tobytes() == want["counts"].tobytes(), (R, D, Q, "counts")
            kth = lambda: [torch.kthvalue(x, k, dim=0).values for k in ks]
            kth_t = lambda: [torch.kthvalue(xt, k, dim=1).values for k in ks]
            assert all(torch.equal(v, tau[j]) for j, v in enumerate(kth()))
            fns = {"mse_a": mse_draw, "select_columns": fn, "torch_kthvalue": kth, "torch_kthvalue_transposed": kth_t, "mse_b": mse_draw}
            ms = _interleaved(fns, max(1, a.kernel_reps // 2), a.rounds)
            nbytes = 4 * -(-Q // 4) * 4.0 * R * D
            mse = [mse_bytes / (ms[k] * 1e-3) / rate for k in ("mse_a", "mse_b")]
            row = {"R": R, "D": D, "Q": Q, "ranks": ks, "bytes_floor": int(nbytes), "byte_floor_us": round(nbytes / rate * 1e6, 2),
                   "select_columns_us": round(ms["select_columns"] * 1e3, 2), "torch_kthvalue_us": round(ms["torch_kthvalue"] * 1e3, 2),
                   "torch_kthvalue_transposed_us": round(ms["torch_kthvalue_transposed"] * 1e3, 2),
                   "fraction_of_stream_copy": round(nbytes / (ms["select_columns"] * 1e-3) / rate, 4),
                   "mse_fraction_of_stream_copy": [round(v, 4) for v in mse], "workgroups": -(-D // 16)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, xt
    return rows


def engine_calls(a):
    import torch
    from vbnn_amd.engine import FusedMLP
    R, D = 65536, 10
    eng = FusedMLP(dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=16, hidden=[32, 32],
                        n_classes=D, criterion="mse", type="vb", testSamples=4))
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(R, 16, generator=g, dtype=torch.float32, device="cuda")
    t = torch.randn(R, D, generator=g, dtype=torch.float32, device="cuda")
    res = eng.predict_regression(x, S=4, targets=t, noise_var=0.25)
    out = {"R": R, "D": D, "levels": list(LEVELS[3])}
    for scope in ("per_output", "joint"):
        cal_ms, int_ms = [], []
        for rnd in range(a.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cal = eng.conformal_calibrate_intervals(res, t, levels=LEVELS[3], scope=scope, noise_var=0.25)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r = eng.conformal_intervals(res, cal, targets=t)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rnd:
                cal_ms.append((t1 - t0) * 1e3)
                int_ms.append((t2 - t1) * 1e3)
        out[scope] = {"conformal_calibrate_intervals_ms": round(statistics.median(cal_ms), 3),
                      "conformal_intervals_ms": round(statistics.median(int_ms), 3), "coverage": r.coverage, "joint_coverage": r.joint_coverage}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=10, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformal_interval_bench.json"))
    a = ap.parse_args()
    import torch
    from calibration_bench import _box
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = _box(L, h)
    rate = box.hbm_TBps * 1e12
    mse_draw, mse_bytes, keep = _yardstick(L, h, torch.Generator(device="cuda").manual_seed(5))
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d,
           "streaming": streaming_points(a, L, h, rate, mse_draw, mse_bytes),
           "select_columns": select_points(a, L, h, rate, mse_draw, mse_bytes),
           "engine_calls_host_clock": engine_calls(a)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
