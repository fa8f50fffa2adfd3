#!/usr/bin/env python3
"""What the class-probability predictive for any class count (FusedMLP.predict_classes over vbnn_predict_class_moments) costs.

    python tools/class_predict_bench.py [--reps 5] [--rounds 5] [--out profiles/class_predict_bench.json]
    python tools/class_predict_bench.py --skip-engine | --skip-kernel

(a) the kernel alone, us per launch from blocks of launches between HIP events (never one launch on its own), the variants
interleaved, medians of the rounds:
  ACCUMULATE at (R 4096, C 4096), one middle draw per launch: y in, state in, state out = 201 MB. Beside it, in the same
    process, the MSE form's middle draw (vbnn_predict_moments at the same R x D: 6 R D floats), timed twice: the expectation
    for the class form is the MSE form's share of the stream-copy rate, the allowance that form's own spread over its two
    timings. `meets_mse_share` says whether it held.
  STACKED at (R 128, C 4096, S 30) and (R 1024, C 1000, S 30), targets and K = 5: y of every draw in, probs and log_probs out.
Each point in us, as a share of the box's measured stream-copy rate (vbnn_box_calibrate) by the bytes the form must move, and
against a PyTorch composition on the same tensors (log_softmax per draw, logsumexp over the draws, the entropy sums, topk).
Before anything is timed the kernel's outputs are asserted against float64 on the same inputs at the bounds of
tests/_classes_np.py, and the order of the classes and the counts exactly.

(b) a whole predict_classes call at 784-400-400-100, fp32, 100 rows, S = 30, against test() on the same inputs, and the share
of the call that is the moments launch. Whatever is measured is written down, including where the kernel misses."""
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


def _assert_against_float64(got, draws, t, K):
    """the bounds of tests/_classes_np.py, in float64 on the device"""
    import torch
    S, R, Cn = draws.shape
    o = torch.log_softmax(draws.double(), 2)
    lp = torch.logsumexp(o, 0) - math.log(S)
    p = lp.exp()
    tl = (Cn + 4 * S + 16) * EPS * lp.abs().clamp(min=1.0)
    assert bool(((got["log_probs"].double() - lp).abs() <= tl).all()), "log_probs"
    assert bool(((got["probs"].double() - p).abs() <= (Cn + 4 * S + 20) * EPS * lp.abs().clamp(min=1.0) * p + 2.0 ** -126).all()), "probs"
    ent, H = -(p * lp).sum(1), -(o.exp() * o).sum(2)
    te = (Cn + 16) * EPS * ent.abs() + (p * (1 + lp.abs()) * tl).sum(1)
    tx = (Cn + 16) * EPS * H.mean(0).abs() + (o.exp() * (1 + o.abs()) * (Cn + 16) * EPS * o.abs().clamp(min=1.0)).sum(2).mean(0)
    assert bool(((got["entropy"].double() - ent).abs() <= te).all()), "entropy"
    assert bool(((got["expected_entropy"].double() - H.mean(0)).abs() <= tx).all()), "expected_entropy"
    assert bool(((got["mutual_info"].double() - (ent - H.mean(0))).abs() <= te + tx).all()), "mutual_info"
    order = torch.sort(-got["log_probs"], dim=1, stable=True).indices[:, :K]
    assert torch.equal(got["topk_idx"].long(), order) and torch.equal(got["pred"].long(), order[:, 0]), "the order of the classes"
    assert torch.equal(got["topk_prob"], torch.gather(got["probs"], 1, order)), "topk_prob"
    tot, tl_ = got["totals"], t.long()
    assert tot[1] == float((got["pred"].long() == tl_).sum()) and tot[3] == float((draws.argmax(2) == tl_[None]).sum()), "hits"
    assert tot[4] == float((got["topk_idx"].long() == tl_[:, None]).any(1).sum()), "top-K hits"
    want = float(-got["log_probs"].double().gather(1, tl_[:, None]).sum())
    assert abs(tot[0] - want) <= 1e-12 * abs(want), "totals[0]"


def _class_args(L, _p, draws, t, form, K, state, ld_state, out, tot):
    S, R, Cn = draws.shape
    return L.ClassMomentsArgs(y=_p(draws), ld_y=Cn, target=_p(t), R=R, C=Cn, S=S, form=form, K=K, state=_p(state), ld_state=ld_state,
                              probs=_p(out["probs"]), log_probs=_p(out["log_probs"]), ld_out=Cn, entropy=_p(out["entropy"]),
                              expected_entropy=_p(out["expected_entropy"]), mutual_info=_p(out["mutual_info"]), pred=_p(out["pred"]),
                              topk_idx=_p(out["topk_idx"]), topk_prob=_p(out["topk_prob"]), totals=_p(tot))


def kernel_points(a):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    box, box_d = _box(L, h)
    rate = box.hbm_TBps * 1e12
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    K, rows = 5, []
    for form, R, Cn, S in (("accumulate", 4096, 4096, 4), ("stacked", 128, 4096, 30), ("stacked", 1024, 1000, 30)):
        g = torch.Generator(device="cuda").manual_seed(5)
        draws = 2.0 * torch.randn(S, R, Cn, generator=g, **f32)
        t = torch.randint(0, Cn, (R,), generator=g, device="cuda").to(torch.int32)
        out = {"probs": torch.empty(R, Cn, **f32), "log_probs": torch.empty(R, Cn, **f32), "entropy": torch.empty(R, **f32),
               "expected_entropy": torch.empty(R, **f32), "mutual_info": torch.empty(R, **f32), "pred": torch.empty(R, **i32),
               "topk_idx": torch.empty(R, K, **i32), "topk_prob": torch.empty(R, K, **f32)}
        tot = torch.zeros(5, dtype=torch.float64, device="cuda")
        ld_state = (Cn + 3 + 3) // 4 * 4
        state = torch.empty(R, ld_state, **f32) if form == "accumulate" else None
        m = _class_args(L, _p, draws, t, L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE, K, state, ld_state, out, tot)

        def launch(s):
            m.draw = s
            m.y = C.c_void_p(draws.data_ptr() + 4 * s * R * Cn)
            L.check(lib.vbnn_predict_class_moments(h, C.byref(m)))

        def whole():
            if form == "stacked":
                m.y = _p(draws)
                L.check(lib.vbnn_predict_class_moments(h, C.byref(m)))
            else:
                for s in range(S):
                    launch(s)

        def composition():                                   # PyTorch device ops on the same tensors
            o = torch.log_softmax(draws, 2)
            lp = torch.logsumexp(o, 0) - math.log(S)
            p = lp.exp()
            ent = -(p * lp).sum(1)
            eH = -(o.exp() * o).sum(2).mean(0)
            top = lp.topk(K, 1)
            return lp, p, ent, eH, top

        def composition_draw():                              # ... of one middle draw: the running logsumexp of one more log_softmax
            o = torch.log_softmax(draws[1], 1)
            Lr = torch.logaddexp(out["log_probs"], o)
            return Lr, -(o.exp() * o).sum(1)
        whole()
        _assert_against_float64(dict(out, totals=tot.cpu().tolist()), draws, t, K)
        rd = 4.0 * R * Cn
        row = {"form": form, "R": R, "C": Cn, "S": S, "K": K}
        if form == "stacked":
            ms = _interleaved({"kernel": whole, "torch": composition}, a.kernel_reps, a.rounds)
            nbytes = S * rd + 2 * rd                         # y of every draw in, probs and log_probs out
            row.update(kernel_us=round(ms["kernel"] * 1e3, 2), torch_composition_us=round(ms["torch"] * 1e3, 2),
                       kernel_over_torch=round(ms["kernel"] / ms["torch"], 4), bytes_moved=int(nbytes),
                       byte_floor_us=round(nbytes / rate * 1e6, 2), fraction_of_stream_copy=round(nbytes / (ms["kernel"] * 1e-3) / rate, 4),
                       over_byte_floor=round(ms["kernel"] * 1e-3 / (nbytes / rate), 2))
        else:                                                # the MSE form's middle draw beside it, twice
            tt = torch.randn(R, Cn, generator=g, **f32)
            st2 = torch.empty(R, 2 * Cn + 2, **f32)
            mm = L.MomentsArgs(y=_p(draws), ld_y=Cn, target=_p(tt), ld_t=Cn, R=R, D=Cn, S=S, noise_var=0.1, state=_p(st2),
                               form=L.MOMENTS_ACCUMULATE, ld_out=Cn)

            def mse_draw(s=1):
                mm.draw = s
                mm.y = C.c_void_p(draws.data_ptr() + 4 * s * R * Cn)
                L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
            mse_draw(0)
            ms = _interleaved({"mse_a": mse_draw, "middle_draw": lambda: launch(1), "mse_b": mse_draw, "torch": composition_draw},
                              a.kernel_reps, a.rounds)
            mid, mse_mid = 3 * rd, 6 * rd                    # y, state in, state out; the MSE form: state in and out (2 D each), y, t
            share = mid / (ms["middle_draw"] * 1e-3) / rate
            mse = [mse_mid / (ms[k] * 1e-3) / rate for k in ("mse_a", "mse_b")]
            row.update(middle_draw_us=round(ms["middle_draw"] * 1e3, 2), middle_draw_bytes=int(mid),
                       byte_floor_us=round(mid / rate * 1e6, 2), middle_draw_fraction_of_stream_copy=round(share, 4),
                       torch_composition_us=round(ms["torch"] * 1e3, 2), kernel_over_torch=round(ms["middle_draw"] / ms["torch"], 4),
                       mse_middle_draw_us=[round(ms["mse_a"] * 1e3, 2), round(ms["mse_b"] * 1e3, 2)], mse_middle_draw_bytes=int(mse_mid),
                       mse_fraction_of_stream_copy=[round(v, 4) for v in mse], mse_spread=round(abs(mse[0] - mse[1]), 4),
                       meets_mse_share=bool(share >= min(mse) - abs(mse[0] - mse[1])))
            del tt, st2
        rows.append(row)
        del draws, t, out, state
    return rows, box_d


def engine_point(a):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import _p
    I0, hidden, Cn, R, S, K = 784, [400, 400], 100, 100, 30, 5
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=I0, hidden=hidden, n_classes=Cn, type="vb",
               testSamples=S)
    eng = FusedMLP(opt)
    eng.prepare()
    x = torch.empty(R, I0, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    res = eng.predict_classes(x, targets=t, topk=K)
    err, acc = eng.test(x, t)
    assert res.chunks == 1 and res.stacked
    lib, h = L.lib(), eng.ctx.h
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    draws = torch.randn(S, R, Cn, **f32)
    out = {"probs": torch.empty(R, Cn, **f32), "log_probs": torch.empty(R, Cn, **f32), "entropy": torch.empty(R, **f32),
           "expected_entropy": torch.empty(R, **f32), "mutual_info": torch.empty(R, **f32), "pred": torch.empty(R, **i32),
           "topk_idx": torch.empty(R, K, **i32), "topk_prob": torch.empty(R, K, **f32)}
    tot = torch.zeros(5, dtype=torch.float64, device="cuda")
    m = _class_args(L, _p, draws, t, L.MOMENTS_STACKED, K, None, 0, out, tot)

    def moments():
        with eng._on_stream():
            L.check(lib.vbnn_predict_class_moments(h, C.byref(m)))
    ms = _interleaved({"predict_classes": lambda: eng.predict_classes(x, targets=t, topk=K), "test": lambda: eng.test(x, t),
                       "moments": moments}, a.reps, a.rounds)
    return {"net": f"{I0}-" + "-".join(map(str, hidden)) + f"-{Cn}", "dtype": "f32", "R": R, "S": S, "K": K, "stacked": res.stacked,
            "predict_classes_ms": round(ms["predict_classes"], 4), "test_ms": round(ms["test"], 4),
            "predict_over_test": round(ms["predict_classes"] / ms["test"], 4), "moments_ms_per_call": round(ms["moments"], 5),
            "moments_share_of_call": round(ms["moments"] / ms["predict_classes"], 4), "mean_draw_nll": res.mean_draw_nll,
            "test_error": err, "mean_draw_accuracy": res.mean_draw_accuracy, "test_accuracy": acc, "nll": res.nll,
            "accuracy": res.accuracy, "topk_accuracy": res.topk_accuracy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_predict_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"reps": a.reps, "kernel_reps": a.kernel_reps, "rounds": a.rounds}
    if not a.skip_kernel:
        out["kernel"], out["box"] = kernel_points(a)
    if not a.skip_engine:
        out["engine"] = [engine_point(a)]
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
