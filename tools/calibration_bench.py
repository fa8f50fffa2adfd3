#!/usr/bin/env python3
"""What classifier calibration and selective prediction cost (vbnn_predict_calibration, vbnn_selective; csrc/calibration.hip).

    python tools/calibration_bench.py [--kernel-reps 20] [--rounds 5] [--out profiles/calibration_bench.json]

The family's protocol: before anything is timed the outputs are asserted BIT FOR BIT against the restatement of
tests/_calibration_np.py on the same inputs; us per launch come from blocks of launches between HIP events (never one launch on
its own), the variants interleaved, medians of the rounds; the box's held clock and stream-copy rate (vbnn_box_calibrate) are
recorded beside them.

(a) vbnn_predict_calibration at (R 4096, C 4096): 67 MB read. Beside it, in the same process, the MSE form's ACCUMULATE middle
    draw (vbnn_predict_moments at the same R x D: 6 R D floats), timed twice: the expectation is that form's share of the
    stream-copy rate, the allowance its own spread between the two timings (`meets_mse_share`). The shape is timed with uniform
    confidences AND with every row in the last bin: the two are expected to agree within that spread -- a gap would be
    contention on the last bin's words (`last_bin_gap`, `within_spread`). Then (R 65536, C 10), each beside the PyTorch
    composition on the same tensors (gather, comparison, row sums, bincounts).
(b) vbnn_selective at R = 10^4 and 10^6, Q = 1 and Q = 19, beside torch.sort + cumsum on the same tensors. Recorded, not judged.
Whatever is measured is written down, including where a kernel misses."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _probs(R, Cn, conf_lo, conf_hi, g):
    """R x C probabilities whose row r gives its class pred[r] a confidence uniform in [conf_lo, conf_hi) and shares the rest out
    by a softmax; pred, and targets that agree with pred on about that fraction of the rows."""
    import torch
    f32 = dict(dtype=torch.float32, device="cuda")
    conf = conf_lo + (conf_hi - conf_lo) * torch.rand(R, generator=g, **f32)
    probs = torch.softmax(torch.randn(R, Cn, generator=g, **f32), 1) * (1.0 - conf)[:, None]
    pred = torch.randint(0, Cn, (R,), generator=g, device="cuda")
    probs[torch.arange(R, device="cuda"), pred] = conf
    right = torch.rand(R, generator=g, **f32) < conf
    target = torch.where(right, pred, (pred + 1) % Cn)
    return probs.contiguous(), pred.to(torch.int32), target.to(torch.int32)


def rows_points(a, L, h, rate):
    import numpy as np
    import torch
    from tests._calibration_np import calibration32
    from vbnn_amd.nn import _p
    lib, M, rows = L.lib(), 15, []
    f32 = dict(dtype=torch.float32, device="cuda")
    for R, Cn in ((4096, 4096), (65536, 10)):
        g = torch.Generator(device="cuda").manual_seed(5)
        cases = {"uniform": _probs(R, Cn, 0.0, 1.0, g), "last_bin": _probs(R, Cn, 0.95, 0.999, g)}
        out = {"conf": torch.empty(R, **f32), "hit": torch.empty(R, dtype=torch.int32, device="cuda")}
        fns, accs = {}, {}
        for name, (probs, pred, target) in cases.items():
            acc = torch.zeros(3 * M + 4, dtype=torch.int64, device="cuda")
            m = L.CalibrationArgs(probs=_p(probs), ld=Cn, pred=_p(pred), target=_p(target), R=R, C=Cn, bins=M, conf=_p(out["conf"]),
                                  hit=_p(out["hit"]), acc=_p(acc))
            fns[name] = (lambda m=m: L.check(lib.vbnn_predict_calibration(h, C.byref(m))))
            fns[name]()
            want = calibration32(probs.cpu().numpy(), pred.cpu().numpy(), target.cpu().numpy(), M)
            assert np.array_equal(acc.cpu().numpy().view(np.uint64), want["acc"]), (R, Cn, name, "acc")
            assert out["conf"].cpu().numpy().tobytes() == want["conf"].tobytes() and np.array_equal(out["hit"].cpu().numpy(), want["hit"])
            accs[name] = acc
        assert int(accs["last_bin"][M - 1]) == R
        probs, pred, target = cases["uniform"]

        def composition():                                   # PyTorch device ops on the same tensors
            conf = probs.gather(1, pred.long()[:, None])[:, 0]
            hit = pred == target
            brier = (probs * probs).sum(1) - 2.0 * probs.gather(1, target.long()[:, None])[:, 0] + 1.0
            b = (conf * M).long().clamp(max=M - 1)
            return (torch.bincount(b, minlength=M), torch.bincount(b, weights=hit.float(), minlength=M),
                    torch.bincount(b, weights=conf, minlength=M), brier.sum())

        nbytes = 4.0 * R * Cn
        row = {"R": R, "C": Cn, "bins": M, "bytes_read": int(nbytes), "byte_floor_us": round(nbytes / rate * 1e6, 2)}
        if R == 4096:                                        # the MSE form's middle draw beside it, twice
            draws = torch.randn(2, R, Cn, generator=g, **f32)
            tt = torch.randn(R, Cn, generator=g, **f32)
            st2 = torch.empty(R, 2 * Cn + 2, **f32)
            mm = L.MomentsArgs(y=_p(draws), ld_y=Cn, target=_p(tt), ld_t=Cn, R=R, D=Cn, S=4, noise_var=0.1, state=_p(st2),
                               form=L.MOMENTS_ACCUMULATE, ld_out=Cn)

            def mse_draw(s=1):
                mm.draw = s
                mm.y = C.c_void_p(draws.data_ptr() + 4 * s * R * Cn)
                L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
            mse_draw(0)
            ms = _interleaved({"mse_a": mse_draw, "uniform": fns["uniform"], "last_bin": fns["last_bin"], "mse_b": mse_draw,
                               "torch": composition}, a.kernel_reps, a.rounds)
            mse_bytes = 6 * nbytes                           # state in and out (2 D each), y, t
            mse = [mse_bytes / (ms[k] * 1e-3) / rate for k in ("mse_a", "mse_b")]
            spread = abs(mse[0] - mse[1])
            share = {k: nbytes / (ms[k] * 1e-3) / rate for k in ("uniform", "last_bin")}
            row.update(mse_middle_draw_us=[round(ms["mse_a"] * 1e3, 2), round(ms["mse_b"] * 1e3, 2)], mse_middle_draw_bytes=int(mse_bytes),
                       mse_fraction_of_stream_copy=[round(v, 4) for v in mse], mse_spread=round(spread, 4),
                       meets_mse_share=bool(min(share.values()) >= min(mse) - spread),
                       last_bin_gap=round(abs(share["uniform"] - share["last_bin"]), 4),
                       within_spread=bool(abs(share["uniform"] - share["last_bin"]) <= spread))
            del draws, tt, st2
        else:
            ms = _interleaved({"uniform": fns["uniform"], "last_bin": fns["last_bin"], "torch": composition}, a.kernel_reps, a.rounds)
            share = {k: nbytes / (ms[k] * 1e-3) / rate for k in ("uniform", "last_bin")}
        row.update(uniform_us=round(ms["uniform"] * 1e3, 2), last_bin_us=round(ms["last_bin"] * 1e3, 2),
                   fraction_of_stream_copy={k: round(v, 4) for k, v in share.items()},
                   torch_composition_us=round(ms["torch"] * 1e3, 2), kernel_over_torch=round(ms["uniform"] / ms["torch"], 4))
        rows.append(row)
        del cases, fns, accs, probs, pred, target
    return rows


def selective_points(a, L, h):
    import numpy as np
    import torch
    from tests._calibration_np import selective32
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    for R in (10 ** 4, 10 ** 6):
        g = torch.Generator(device="cuda").manual_seed(7)
        score = 2.3 * torch.rand(R, generator=g, dtype=torch.float32, device="cuda")          # entropy-like
        hit = (torch.rand(R, generator=g, device="cuda") < 0.8).to(torch.int32)
        for Q in (1, 19):
            ks = [R // 2] if Q == 1 else [max(1, (j + 1) * R // 20) for j in range(19)]
            tau = torch.empty(Q, dtype=torch.float32, device="cuda")
            counts = torch.empty(Q, 4, dtype=torch.int64, device="cuda")
            m = L.SelectiveArgs(score=_p(score), hit=_p(hit), R=R, Q=Q, tau=_p(tau), counts=_p(counts))
            for j, k in enumerate(ks):
                m.k[j] = k
            kd = torch.tensor(ks, device="cuda") - 1

            def kernel():
                L.check(lib.vbnn_selective(h, C.byref(m)))

            def composition():                               # PyTorch device ops on the same tensors
                s, idx = torch.sort(score)
                ch = hit[idx].cumsum(0)
                return s[kd], ch[kd].double() / (kd + 1)
            kernel()
            wtau, wcounts = selective32(score.cpu().numpy(), hit.cpu().numpy(), ks)
            assert tau.cpu().numpy().tobytes() == wtau.tobytes() and np.array_equal(counts.cpu().numpy().view(np.uint64), wcounts), (R, Q)
            ms = _interleaved({"kernel": kernel, "torch": composition}, a.kernel_reps, a.rounds)
            rows.append({"R": R, "Q": Q, "kernel_us": round(ms["kernel"] * 1e3, 2), "torch_sort_cumsum_us": round(ms["torch"] * 1e3, 2),
                         "kernel_over_torch": round(ms["kernel"] / ms["torch"], 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = _box(L, h)
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d,
           "calibration": rows_points(a, L, h, box.hbm_TBps * 1e12), "selective": selective_points(a, L, h)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
