#!/usr/bin/env python3
"""What the Bernoulli likelihood head costs: vbnn_bce_forward, vbnn_predict_label_moments and FusedMLP.predict_labels / test()
with criterion = "bce".

    python tools/label_predict_bench.py [--reps 5] [--kernel-reps 20] [--rounds 5] [--out profiles/label_predict_bench.json]

The protocol of tools/gauss_predict_bench.py: blocks of calls between HIP events (never one launch on its own), the variants
interleaved round by round, medians of the rounds, the box's held clock and stream-copy rate (vbnn_box_calibrate) beside every
figure, and the outputs asserted against float64 on the same inputs before anything is timed.

(a) ACCUMULATE at R 4096 x D 4096, one middle draw per launch, beside the MSE form at the same shape in the same process -- the
    MSE form timed TWICE (its own spread is the allowance); each as a share of the stream-copy rate by the bytes its form must
    move (labels: y rd, t rd, state 3 rd in and 3 rd out, rd = 4 R D; mse: y, t, state 2 + 2). "Runs at the byte rate" means:
    the label kernel's share is not below the MSE kernel's lower share minus the allowance. Otherwise the row says MISS.
(b) STACKED at R 128 x D 4096 x S 30 against the PyTorch composition on the same tensors (sigmoid, logsigmoid, means, entropies,
    row sums, logsumexp).
(c) the criterion kernel at 4096 x 4096 against vbnn_mse_forward at the same shape and the byte floor of both (8 B read + 4 B
    written per element), and the PyTorch composition (binary_cross_entropy_with_logits and its gradient formula).
(d) one predict_labels call and one test() on 784-400-400-10, fp32, 100 rows, S = 30.
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
ELEM, ROWS = ("probs", "entropy", "mutual_info"), ("row_entropy", "row_mutual_info", "row_log_lik", "row_marg_log_lik")


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


def _outputs(R, D):
    import torch
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {k: torch.empty(R, D, **f32) for k in ELEM}
    out.update({k: torch.empty(R, **f32) for k in ROWS})
    out["row_hits"] = torch.empty(R, dtype=torch.int32, device="cuda")
    return out


def _label_args(L, _p, y, t, R, D, S, form, state, out, tot):
    return L.LabelMomentsArgs(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, form=form, state=_p(state), ld_out=D, totals=_p(tot),
                              **{k: _p(v) for k, v in out.items()})


def _assert_labels_against_float64(got, draws, t, S, D):
    """The element and row bounds of tests/_labels_np.py, in torch float64 on the device."""
    import torch
    z = draws.double().clamp(-80.0, 80.0)
    lp, ln = torch.nn.functional.logsigmoid(z), torch.nn.functional.logsigmoid(-z)
    p, q = lp.exp(), ln.exp()
    pm, qm = p.mean(0), q.mean(0)
    ent = -(pm * pm.log() + qm * qm.log())
    ee = (-(p * lp + q * ln)).mean(0)
    assert bool(((got["probs"].double() - pm).abs() <= (S + 6) * EPS * pm).all()), "probs"
    ent_tol = (S + 10) * EPS * (ent + 1.0)
    assert bool(((got["entropy"].double() - ent).abs() <= ent_tol).all()), "entropy"
    mi = ent - ee
    assert bool(((got["mutual_info"].double() - mi).abs() <= ent_tol + (S + 16) * EPS * ee + EPS * mi.abs()).all()), "mutual_info"
    t64 = t.double()
    a = (t64[None] * lp + (1 - t64[None]) * ln).sum(2)
    ll = torch.logsumexp(a, 0) - math.log(S)
    tl = (D + 32) * EPS * a.abs().amax(0) + (4 * S + 16) * EPS * ll.abs().clamp(min=1.0)
    assert bool(((got["row_log_lik"].double() - ll).abs() <= tl).all()), "row_log_lik"
    marg = (t64 * pm.log() + (1 - t64) * qm.log()).sum(1)
    assert bool(((got["row_marg_log_lik"].double() - marg).abs() <= (D + 32) * EPS * marg.abs() + D * (S + 7) * EPS).all()), "row_marg"
    assert abs(got["totals"][2] + float(a.sum())) <= float((D + 32) * EPS * a.abs().sum() + S * EPS * a.abs().sum()), "sum -a_s"
    # away from a tie the hits are exact; among millions of random elements a few lie inside the bound of one: either way there
    clear = (p.sum(0) - q.sum(0)).abs() > 2 * (S + 6) * EPS * S
    hit = ((pm > qm) == (t64 > 0.5)) & clear
    lo, hi = hit.sum(1), hit.sum(1) + (~clear).sum(1)
    hits = got["row_hits"].long()
    assert bool(((hits >= lo) & (hits <= hi)).all()) and got["totals"][3] == float(hits.sum()), "hits"


def moments_points(a, box):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    rows = []
    g = torch.Generator(device="cuda").manual_seed(5)
    share = lambda nbytes, t_ms: nbytes / (t_ms * 1e-3) / bw
    # ---- (a) ACCUMULATE, one middle draw: labels beside mse, both R 4096 x D 4096
    R, D, S = 4096, 4096, 4
    y = 3.0 * torch.randn(S, R, D, generator=g, **f32)
    t = (torch.rand(R, D, generator=g, **f32) < 0.4).float()
    ol, totl = _outputs(R, D), torch.zeros(5, dtype=torch.float64, device="cuda")
    stl = torch.empty(R, 3 * D + 2, **f32)
    ml = _label_args(L, _p, y, t, R, D, S, L.MOMENTS_ACCUMULATE, stl, ol, totl)
    om = {k: torch.empty((R, D) if k in ("mean", "var") else (R,), **f32) for k in ("mean", "var", "row_var", "row_sq_err", "row_log_lik")}
    totm = torch.zeros(4, dtype=torch.float64, device="cuda")
    stm = torch.empty(R, 2 * D + 2, **f32)
    mm = L.MomentsArgs(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, noise_var=0.1, state=_p(stm),
                       form=L.MOMENTS_ACCUMULATE, mean=_p(om["mean"]), var=_p(om["var"]), ld_out=D, row_var=_p(om["row_var"]),
                       row_sq_err=_p(om["row_sq_err"]), row_log_lik=_p(om["row_log_lik"]), totals=_p(totm))

    def label_draw(s):
        ml.draw, ml.y = s, C.c_void_p(y.data_ptr() + 4 * s * R * D)
        L.check(lib.vbnn_predict_label_moments(h, C.byref(ml)))

    def mse_draw(s):
        mm.draw, mm.y = s, C.c_void_p(y.data_ptr() + 4 * s * R * D)
        L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
    for s in range(S):
        label_draw(s)
        mse_draw(s)
    _assert_labels_against_float64(dict(ol, totals=totl.cpu().tolist()), y, t, S, D)
    ms = _interleaved({"labels": lambda: label_draw(1), "mse_first": lambda: mse_draw(1), "mse_second": lambda: mse_draw(1)},
                      a.kernel_reps, a.rounds)
    rd = 4.0 * R * D
    bl, bm = (1 + 1 + 3 + 3) * rd, (1 + 1 + 2 + 2) * rd
    sl, s1, s2 = share(bl, ms["labels"]), share(bm, ms["mse_first"]), share(bm, ms["mse_second"])
    allowance = abs(s1 - s2)
    rows.append({"form": "accumulate", "what": "one middle draw", "R": R, "D": D,
                 "labels_us": round(ms["labels"] * 1e3, 2), "mse_us": [round(ms["mse_first"] * 1e3, 2), round(ms["mse_second"] * 1e3, 2)],
                 "labels_bytes": int(bl), "mse_bytes": int(bm), "labels_fraction_of_stream_copy": round(sl, 4),
                 "mse_fraction_of_stream_copy": [round(s1, 4), round(s2, 4)], "allowance": round(allowance, 4),
                 "verdict": "HIT" if sl >= min(s1, s2) - allowance else "MISS"})
    del y, t, ol, stl, om, stm
    # ---- (b) STACKED against the PyTorch composition
    R, D, S = 128, 4096, 30
    draws = 3.0 * torch.randn(S, R, D, generator=g, **f32)
    t = (torch.rand(R, D, generator=g, **f32) < 0.4).float()
    out, tot = _outputs(R, D), torch.zeros(5, dtype=torch.float64, device="cuda")
    m = _label_args(L, _p, draws, t, R, D, S, L.MOMENTS_STACKED, None, out, tot)

    def kernel():
        L.check(lib.vbnn_predict_label_moments(h, C.byref(m)))

    def composition():
        z = draws.clamp(-80.0, 80.0)
        lp, ln = torch.nn.functional.logsigmoid(z), torch.nn.functional.logsigmoid(-z)
        p, q = lp.exp(), ln.exp()
        pm, qm = p.mean(0), q.mean(0)
        log_p, log_q = pm.log(), qm.log()
        ent = -(pm * log_p + qm * log_q)
        mi = ent - (-(p * lp + q * ln)).mean(0)
        a_s = (t[None] * lp + (1 - t[None]) * ln).sum(2)
        return pm, ent, mi, ent.sum(1), mi.sum(1), torch.logsumexp(a_s, 0), (t * log_p + (1 - t) * log_q).sum(1), \
            ((pm > qm) == (t > 0.5)).sum(1)
    kernel()
    _assert_labels_against_float64(dict(out, totals=tot.cpu().tolist()), draws, t, S, D)
    ms = _interleaved({"kernel": kernel, "torch": composition}, a.kernel_reps, a.rounds)
    rd = 4.0 * R * D
    nbytes = S * rd + rd + 3 * rd                            # y of every draw, the targets, probs / entropy / mutual_info out
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
    N, D = 4096, 4096
    g = torch.Generator(device="cuda").manual_seed(9)
    y = 4.0 * torch.randn(N, D, generator=g, **f32)
    t = (torch.rand(N, D, generator=g, **f32) < 0.4).float()
    grad = torch.empty(N, D, **f32)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    corr = torch.zeros(1, dtype=torch.int32, device="cuda")
    inv = 1.0 / (N * D)

    def bce():
        L.check(lib.vbnn_bce_forward(h, _p(y), D, _p(t), D, N, D, inv, _p(grad), D, 0, _p(loss), _p(corr)))

    def mse():
        L.check(lib.vbnn_mse_forward(h, _p(y), D, _p(t), D, N, D, inv, _p(grad), D, 0, _p(loss)))

    def composition():
        l = torch.nn.functional.binary_cross_entropy_with_logits(y, t, reduction="sum") * inv
        return l, inv * (torch.sigmoid(y) - t), ((y > 0) == (t > 0.5)).sum()
    bce()
    z64, t64 = y.double(), t.double()
    inv32 = float(torch.tensor(inv, dtype=torch.float32))
    l1p = torch.log1p((-z64.abs()).exp())
    want = inv32 * float((z64.clamp(min=0) - z64 * t64 + l1p).sum())
    assert abs(float(loss.cpu()) - want) <= 10 * EPS * inv32 * float((z64.abs() * t64 + z64.clamp(min=0) + l1p).sum()), "loss"
    sig = torch.sigmoid(z64)
    assert bool(((grad.double() - inv32 * (sig - t64)).abs() <= 8 * EPS * inv32 * (sig + (sig - t64).abs()) + inv32 * 2.0 ** -126).all()), "g"
    assert int(corr.cpu()) == int(((y > 0) == (t > 0.5)).sum()), "hits"
    ms = _interleaved({"bce": bce, "mse": mse, "torch": composition}, a.kernel_reps, a.rounds)
    nbytes = 12.0 * N * D
    return {"N": N, "D": D, "bce_us": round(ms["bce"] * 1e3, 2), "mse_us": round(ms["mse"] * 1e3, 2),
            "torch_composition_us": round(ms["torch"] * 1e3, 2), "bytes": int(nbytes), "byte_floor_us": round(nbytes / bw * 1e6, 2),
            "bce_fraction_of_stream_copy": round(nbytes / (ms["bce"] * 1e-3) / bw, 4),
            "mse_fraction_of_stream_copy": round(nbytes / (ms["mse"] * 1e-3) / bw, 4)}


def engine_point(a):
    import torch
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    R, D, S = 100, 10, 30
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=784, hidden=[400, 400], n_classes=D,
               criterion="bce", type="vb", testSamples=S)
    eng = FusedMLP(opt)
    eng.prepare()
    x = torch.empty(R, 784, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    res = eng.predict_labels(x, targets=t)
    err, acc = eng.test(x, t)
    ms = _interleaved({"predict_labels": lambda: eng.predict_labels(x, targets=t), "test": lambda: eng.test(x, t)}, a.reps, a.rounds)
    return {"net": f"784-400-400-{D}", "dtype": "f32", "R": R, "S": S, "stacked": res.stacked,
            "predict_labels_ms": round(ms["predict_labels"], 4), "test_ms": round(ms["test"], 4),
            "predict_over_test": round(ms["predict_labels"] / ms["test"], 4),
            "mean_draw_bce": res.mean_draw_bce, "test_error": err, "test_label_accuracy": acc, "log_lik": res.log_lik,
            "label_accuracy": res.label_accuracy, "exact_match": res.exact_match}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_predict_bench.json"))
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
