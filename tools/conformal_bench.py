#!/usr/bin/env python3
"""What conformal prediction sets cost (vbnn_conformal; csrc/conformal.hip).

    python tools/conformal_bench.py [--kernel-reps 10] [--rounds 5] [--out profiles/conformal_bench.json]

The family's protocol (tools/calibration_bench.py): before anything is timed every output is asserted BIT FOR BIT against the
restatement of tests/_conformal_np.py on the same inputs; us per launch come from blocks of launches between HIP events, the
variants interleaved, medians of the rounds; the box's held clock and stream-copy rate (vbnn_box_calibrate) are recorded, and
the MSE form's ACCUMULATE middle draw (vbnn_predict_moments at R 4096 x D 4096) is timed twice in the same process as the
yardstick: its spread between the two timings is the allowance.

Points: R 4096 x C 4096, R 4096 x C 1000, R 65536 x C 10, each with Q = 1 and Q = 3 thresholds (the calibration quantiles of the
same rows at 0.9 and 0.5 / 0.9 / 0.99), size + cut + covered + acc written, no member words.
LAC reads the matrix once with per-row work, as vbnn_predict_calibration does: the expectation is calibration's share of the
    stream-copy rate at the same R x C in the same run, less the yardstick's spread (`meets_calibration_share`).
APS is not byte bound (32 + log2 C masked row sums a row). It is timed against a PyTorch composition on the same tensors --
    descending torch.sort, cumsum, comparison, row sums -- and the expectation is `not slower than the composition`
    (`not_slower_than_torch`). steps_per_row is what the kernel's search takes by construction.
Whatever is measured is written down, including where a kernel misses."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = {1: (0.9,), 3: (0.5, 0.9, 0.99)}


def points(a, L, h, rate):
    import numpy as np
    import torch
    from calibration_bench import _interleaved, _probs
    from tests._conformal_np import APS, LAC, conformal32, conformal_rank
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    f32 = dict(dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    # the yardstick, once per point in the same interleaving
    Ry = Dy = 4096
    draws = torch.randn(2, Ry, Dy, generator=g, **f32)
    tt = torch.randn(Ry, Dy, generator=g, **f32)
    st2 = torch.empty(Ry, 2 * Dy + 2, **f32)
    mm = L.MomentsArgs(y=_p(draws), ld_y=Dy, target=_p(tt), ld_t=Dy, R=Ry, D=Dy, S=4, noise_var=0.1, state=_p(st2),
                       form=L.MOMENTS_ACCUMULATE, ld_out=Dy)

    def mse_draw(s=1):
        mm.draw = s
        mm.y = C.c_void_p(draws.data_ptr() + 4 * s * Ry * Dy)
        L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    mse_bytes = 6 * 4.0 * Ry * Dy
    for R, Cn in ((4096, 4096), (4096, 1000), (65536, 10)):
        probs, pred, target = _probs(R, Cn, 0.0, 1.0, g)
        ph, th = probs.cpu().numpy(), target.cpu().numpy()
        M = 15
        cacc = torch.zeros(3 * M + 4, dtype=torch.int64, device="cuda")
        cm = L.CalibrationArgs(probs=_p(probs), ld=Cn, pred=_p(pred), target=_p(target), R=R, C=Cn, bins=M, acc=_p(cacc))
        calibration = lambda cm=cm: L.check(lib.vbnn_predict_calibration(h, C.byref(cm)))
        nbytes = 4.0 * R * Cn
        for Q in (1, 3):
            fns = {"mse_a": mse_draw, "calibration": calibration}
            row = {"R": R, "C": Cn, "Q": Q, "bytes_read": int(nbytes), "byte_floor_us": round(nbytes / rate * 1e6, 2),
                   "aps_steps_per_row": 32 + int(Cn).bit_length()}
            keep = []
            for name, kind in (("lac", LAC), ("aps", APS)):
                s = conformal32(ph, th, kind)["score"]
                qhat = np.sort(s)[[conformal_rank(R, lv) - 1 for lv in LEVELS[Q]]].astype(np.float32)
                qd = torch.from_numpy(qhat).cuda()
                out = {k: torch.empty(Q, R, dtype=torch.int32, device="cuda") for k in ("size", "cut_index", "covered")}
                out["cut_prob"] = torch.empty(Q, R, **f32)
                acc = torch.zeros(8 * Q + 2, dtype=torch.int64, device="cuda")
                m = L.ConformalArgs(probs=_p(probs), ld=Cn, target=_p(target), R=R, C=Cn, kind=kind, Q=Q, qhat=_p(qd), acc=_p(acc),
                                    **{k: _p(v) for k, v in out.items()})
                fns[name] = (lambda m=m: L.check(lib.vbnn_conformal(h, C.byref(m))))
                fns[name]()
                want = conformal32(ph, th, kind, qhat)
                assert np.array_equal(acc.cpu().numpy().view(np.uint64), want["acc"]), (R, Cn, Q, name, "acc")
                for k, v in out.items():
                    assert v.cpu().numpy().tobytes() == want[k].tobytes(), (R, Cn, Q, name, k)
                row[name + "_mean_size"] = [round(float(x), 3) for x in want["size"].mean(1)]
                keep.append((m, qd, out, acc))
                if kind == APS:
                    tlong = target.long()[:, None]

                    def composition(qd=qd):                  # PyTorch device ops on the same tensors
                        sp, idx = torch.sort(probs, dim=1, descending=True, stable=True)
                        cs = sp.cumsum(1)
                        inside = cs[None, :, :] <= qd[:, None, None]
                        size = inside.sum(2)
                        rank_t = (idx == tlong).int().argmax(1)
                        covered = rank_t[None, :] < size
                        return size.sum(1), covered.sum(1), (size == 1).sum(1)
                    fns["torch_aps"] = composition
            fns["mse_b"] = mse_draw
            ms = _interleaved(fns, a.kernel_reps, a.rounds)
            mse = [mse_bytes / (ms[k] * 1e-3) / rate for k in ("mse_a", "mse_b")]
            spread = abs(mse[0] - mse[1])
            share = {k: nbytes / (ms[k] * 1e-3) / rate for k in ("lac", "calibration")}
            row.update(mse_middle_draw_us=[round(ms["mse_a"] * 1e3, 2), round(ms["mse_b"] * 1e3, 2)],
                       mse_fraction_of_stream_copy=[round(v, 4) for v in mse], mse_spread=round(spread, 4),
                       lac_us=round(ms["lac"] * 1e3, 2), calibration_us=round(ms["calibration"] * 1e3, 2),
                       fraction_of_stream_copy={k: round(v, 4) for k, v in share.items()},
                       meets_calibration_share=bool(share["lac"] >= share["calibration"] - spread),
                       aps_us=round(ms["aps"] * 1e3, 2), torch_sort_cumsum_us=round(ms["torch_aps"] * 1e3, 2),
                       aps_over_torch=round(ms["aps"] / ms["torch_aps"], 4), not_slower_than_torch=bool(ms["aps"] <= ms["torch_aps"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fns, keep
        del probs, pred, target
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=10, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformal_bench.json"))
    a = ap.parse_args()
    from calibration_bench import _box
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = _box(L, h)
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d, "points": points(a, L, h, box.hbm_TBps * 1e12)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
