#!/usr/bin/env python3
"""What the rank metrics cost (vbnn_rank_metrics; csrc/ranking.hip).

    python tools/ranking_bench.py [--kernel-reps 10] [--rounds 5] [--out profiles/ranking_bench.json]

The family's protocol: before anything is timed the outputs are asserted BIT FOR BIT against the restatement of
tests/_ranking_np.py on the same inputs (every column, or 16 columns spread over the matrix at the 4096-column point -- recorded
as `columns_checked`); us per call come from blocks of calls between HIP events (never one call on its own), the variants
interleaved, medians of the rounds; the box's held clock and stream-copy rate (vbnn_box_calibrate) are recorded beside them, and
the MSE form's ACCUMULATE middle draw (vbnn_predict_moments at 4096 x 4096) is timed twice in the same process as the yardstick
of what a streaming kernel of this library reaches on this box.

Points, R x D: 10^4 x 10, 10^4 x 4096, 10^5 x 100, 10^6 x 1, 10^6 x 10 -- uniform scores in [0, 1), about 10 % positives that
lean towards the high scores, one threshold. Beside each point: a PyTorch composition on the same tensors (torch.sort along the
rows, cumulative sums, ties by run boundaries, AUROC and average precision in float64) and the same composition on their D x R
transposes, where the sort runs along the contiguous dimension, once with run boundaries (a cummax) and once with ties by
searchsorted (the transposition itself is not timed; `kernel_over_torch` is against the fastest of the three), all asserted to
agree with the kernel's ratios within 1e-10 + 2^-32; the byte floor of the passes the method makes -- per element the pack
reads 8 B (score, target) and writes 8 B, the histograms read 8 B, each of the four radix passes reads 8 B and writes 8 B, the
walk reads 8 B: 96 B -- over the measured stream-copy rate; and the workspace size. A whole FusedMLP.ranking call from Python at
10^4 x 10 is recorded by the host clock. Nothing is judged here: whatever is measured is written down, including where the
kernel loses."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = ((10 ** 4, 10), (10 ** 4, 4096), (10 ** 5, 100), (10 ** 6, 1), (10 ** 6, 10))
BYTES_PER_ELEMENT = 16 + 8 + 4 * 16 + 8


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


def _composition(score, pos, dim=0):
    """AUROC and average precision per column with PyTorch device ops, float64: descending sort along `dim` (0: the R x D tensors as
    they are; 1: their D x R transposes, the sort along the contiguous dimension), cumulative counts, one term per run of equal
    scores (its last element)."""
    import torch
    n = score.shape[dim]
    s, idx = torch.sort(score, dim=dim, descending=True)
    y = pos.gather(dim, idx).double()
    tp, fp = y.cumsum(dim), (1.0 - y).cumsum(dim)
    end = torch.ones_like(s, dtype=torch.bool)
    end.narrow(dim, 0, n - 1).copy_(s.narrow(dim, 1, n - 1) != s.narrow(dim, 0, n - 1))
    zero = torch.zeros_like(tp.narrow(dim, 0, 1))
    tpe = torch.where(end, tp, zero).cummax(dim).values     # (the counts never fall: the latest run end's)
    fpe = torch.where(end, fp, zero).cummax(dim).values
    tp0, fp0 = torch.cat([zero, tpe.narrow(dim, 0, n - 1)], dim), torch.cat([zero, fpe.narrow(dim, 0, n - 1)], dim)
    n_pos, n_neg = tp.narrow(dim, n - 1, 1), fp.narrow(dim, n - 1, 1)
    ap = (torch.where(end, (tp - tp0) * tp / (tp + fp), zero)).sum(dim, keepdim=True) / n_pos
    auroc = (torch.where(end, (fp - fp0) * (tp + tp0) * 0.5, zero)).sum(dim, keepdim=True) / (n_pos * n_neg)
    return auroc.reshape(-1), ap.reshape(-1)


def _composition_searchsorted(score_t, pos_t):
    """The same two ratios from the D x R transposes with ties by searchsorted: an ascending sort along the contiguous
    dimension, and per element the negatives below it, the negatives tied with it and the counts at or above it."""
    import torch
    s, idx = torch.sort(score_t, dim=1)
    y = pos_t.gather(1, idx).double()
    zero = torch.zeros_like(y[:, :1])
    cpos, cneg = torch.cat([zero, y.cumsum(1)], 1), torch.cat([zero, (1.0 - y).cumsum(1)], 1)
    lo, hi = torch.searchsorted(s, s, right=False), torch.searchsorted(s, s, right=True)
    n_pos, n_neg = cpos[:, -1:], cneg[:, -1:]
    below, tied = cneg.gather(1, lo), cneg.gather(1, hi) - cneg.gather(1, lo)
    auroc = (y * (below + 0.5 * tied)).sum(1, keepdim=True) / (n_pos * n_neg)
    tp, fp = n_pos - cpos.gather(1, lo), n_neg - cneg.gather(1, lo)
    ap = (y * tp / (tp + fp)).sum(1, keepdim=True) / n_pos
    return auroc.reshape(-1), ap.reshape(-1)


def mse_yardstick(L, h, g):
    """The MSE form's ACCUMULATE middle draw at 4096 x 4096: a closure, and its bytes."""
    import torch
    from vbnn_amd.nn import _p
    R = Cn = 4096
    f32 = dict(dtype=torch.float32, device="cuda")
    draws, tt = torch.randn(2, R, Cn, generator=g, **f32), torch.randn(R, Cn, generator=g, **f32)
    st2 = torch.empty(R, 2 * Cn + 2, **f32)
    mm = L.MomentsArgs(y=_p(draws), ld_y=Cn, target=_p(tt), ld_t=Cn, R=R, D=Cn, S=4, noise_var=0.1, state=_p(st2),
                       form=L.MOMENTS_ACCUMULATE, ld_out=Cn)

    def mse_draw(s=1):
        mm.draw = s
        mm.y = C.c_void_p(draws.data_ptr() + 4 * s * R * Cn)
        L.check(L.lib().vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    return mse_draw, 6 * 4.0 * R * Cn, (draws, tt, st2)


def points(a, L, h, rate):
    import numpy as np
    import torch
    from tests._ranking_np import derived, rank_metrics
    from vbnn_amd.nn import _p
    lib, rows, tau = L.lib(), [], (0.5,)
    g = torch.Generator(device="cuda").manual_seed(11)
    mse_draw, mse_bytes, _keep = mse_yardstick(L, h, g)
    for R, D in POINTS:
        score = torch.rand(R, D, generator=g, dtype=torch.float32, device="cuda")
        target = (torch.rand(R, D, generator=g, device="cuda") < 0.04 + 0.12 * score).float()
        pos = target > 0.5
        W = 6 + 2 * len(tau)
        out = torch.empty(D, W, dtype=torch.int64, device="cuda")
        need = C.c_size_t()
        L.check(lib.vbnn_rank_metrics_workspace_bytes(R, D, C.byref(need)))
        ws = torch.empty(need.value // 8, dtype=torch.int64, device="cuda")
        m = L.RankMetricsArgs(score=_p(score), ld=D, target=_p(target), ld_t=D, R=R, D=D, Q=len(tau), out=_p(out), workspace=_p(ws),
                              workspace_bytes=need.value)
        m.tau[0] = tau[0]

        def kernel():
            L.check(lib.vbnn_rank_metrics(h, C.byref(m)))
        kernel()
        torch.cuda.synchronize()
        got = [[v & 0xFFFFFFFFFFFFFFFF for v in row] for row in out.cpu().tolist()]
        cols = list(range(D)) if D <= 100 else list(range(0, D, D // 16))[:16]
        sc, tc = score[:, cols].cpu().numpy(), target[:, cols].cpu().numpy()
        want = rank_metrics(sc, target=tc, tau=tau)
        assert [got[j] for j in cols] == want, (R, D, "the kernel's words against the restatement")
        score_t, pos_t = score.t().contiguous(), pos.t().contiguous()          # (the transposition is not timed)
        d = [derived(w, 0) for w in got]
        err_a = err_p = 0.0
        for auroc, ap in (_composition(score, pos), _composition(score_t, pos_t, 1), _composition_searchsorted(score_t, pos_t)):
            err_a = max(err_a, float(np.nanmax(np.abs(auroc.cpu().numpy() - np.array([v["auroc"] for v in d])))))
            err_p = max(err_p, float(np.nanmax(np.abs(ap.cpu().numpy() - np.array([v["average_precision"] for v in d])))))
        assert err_a <= 1e-10 and err_p <= 1e-10 + 2.0 ** -32, (R, D, err_a, err_p)
        ms = _interleaved({"mse_a": mse_draw, "kernel": kernel, "torch": (lambda: _composition(score, pos)),
                           "torch_t": (lambda: _composition(score_t, pos_t, 1)),
                           "torch_ss": (lambda: _composition_searchsorted(score_t, pos_t)), "mse_b": mse_draw}, a.kernel_reps, a.rounds)
        ms_torch = min(ms["torch"], ms["torch_t"], ms["torch_ss"])
        floor_us = BYTES_PER_ELEMENT * R * D / rate * 1e6
        rows.append({"R": R, "D": D, "Q": len(tau), "columns_checked": len(cols), "kernel_us": round(ms["kernel"] * 1e3, 2),
                     "torch_composition_us": round(ms["torch"] * 1e3, 2), "torch_composition_transposed_us": round(ms["torch_t"] * 1e3, 2),
                     "torch_composition_searchsorted_us": round(ms["torch_ss"] * 1e3, 2),
                     "kernel_over_torch": round(ms["kernel"] / ms_torch, 4),
                     "bytes_per_element": BYTES_PER_ELEMENT, "byte_floor_us": round(floor_us, 2),
                     "kernel_over_byte_floor": round(ms["kernel"] * 1e3 / floor_us, 2), "workspace_bytes": need.value,
                     "composition_max_abs_diff": {"auroc": err_a, "average_precision": err_p},
                     "mse_middle_draw_us": [round(ms["mse_a"] * 1e3, 2), round(ms["mse_b"] * 1e3, 2)],
                     "mse_fraction_of_stream_copy": [round(mse_bytes / (ms[k] * 1e-3) / rate, 4) for k in ("mse_a", "mse_b")]})
        print(json.dumps(rows[-1]), flush=True)
        del score, target, pos, score_t, pos_t, out, ws, auroc, ap
    return rows


def whole_call(a):
    """FusedMLP.ranking from Python at 10^4 x 10, host clock around the call (it ends with the copy of the integers)."""
    import torch
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=16, hidden=[32], n_classes=10,
                        criterion="bce", type="vb", testSamples=1, fuse_kl=True, state={"learningRate": 5e-2},
                        meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2}))
    g = torch.Generator(device="cuda").manual_seed(12)
    score = torch.rand(10 ** 4, 10, generator=g, dtype=torch.float32, device="cuda")
    target = (torch.rand(10 ** 4, 10, generator=g, device="cuda") < 0.1).float()
    times = []
    for i in range(3 + 5 * a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ranking(score, target)
        if i >= 3:
            times.append((time.perf_counter() - t0) * 1e6)
    return {"R": 10 ** 4, "D": 10, "calls": len(times), "host_us_median": round(statistics.median(times), 1),
            "host_us_min": round(min(times), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=10, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranking_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = _box(L, h)
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d, "points": points(a, L, h, box.hbm_TBps * 1e12),
           "whole_call": whole_call(a)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
