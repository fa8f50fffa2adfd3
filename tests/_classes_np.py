"""NumPy restatements for the class-probability predictive's tests (vbnn_predict_class_moments, include/vbnn_hip.h): the float64
reference, an fp32 restatement of the online form the kernel runs (with worst-case, sequential row sums), the bounds its outputs
are held to, and check_classes, which prints err / tol ratios as tests/_regress_np.check_moments does."""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126          # the smallest normal fp32: a probability below it may come back as a denormal or as zero

# name: (R, C, S, scale, layout keywords of the GPU test's runner)
KERNEL_CASES = {
    "1x2x1": (1, 2, 1, 2.0, {}),
    "3x5x2": (3, 5, 2, 2.0, {}),
    "37x17x3": (37, 17, 3, 2.0, {}),
    "64x257x30": (64, 257, 30, 2.0, {}),
    "5x4096x4": (5, 4096, 4, 2.0, {}),
    "2x4100x3-above-the-cap": (2, 4100, 3, 2.0, {}),
    "9x20x7-nan-pads": (9, 20, 7, 2.0, dict(ld_y=24)),
    "9x20x7-y-off-by-one-float": (9, 20, 7, 2.0, dict(y_offset=1)),
    "6x1000x5-scale-40": (6, 1000, 5, 40.0, {}),
}


def case_inputs(name):
    """y (S x R x C fp32), t (R int32), K of a kernel case."""
    R, C, S, scale, _ = KERNEL_CASES[name]
    y = (np.float32(scale) * np.random.default_rng(11).standard_normal((S, R, C)).astype(np.float32)).astype(np.float32)
    t = np.random.default_rng(12).integers(0, C, R).astype(np.int32)
    return y, t, min(5, C)


def classes64(y, t=None):
    """The float64 reference on fp32 logits y (S x R x C): o (S x R x C), log_probs, probs, entropy, expected_entropy,
    mutual_info, H (S x R), and with t (R) the four sums that need no ordering."""
    y = y.astype(np.float64)
    S, R, C = y.shape
    mx = y.max(2, keepdims=True)
    o = y - (mx + np.log(np.exp(y - mx).sum(2, keepdims=True)))
    m = o.max(0)
    lp = m + np.log(np.exp(o - m).sum(0)) - np.log(S)
    p = np.exp(lp)
    H = -(np.exp(o) * o).sum(2)
    ref = dict(o=o, log_probs=lp, probs=p, entropy=-(p * lp).sum(1), H=H, expected_entropy=H.mean(0))
    ref["mutual_info"] = ref["entropy"] - ref["expected_entropy"]
    if t is not None:
        rows = np.arange(R)
        ref["nlp_t"] = -lp[rows, t]
        ref["nll_t"] = -o[:, rows, t]                    # S x R
        ref["hits"] = (y.argmax(2) == t[None]).sum()
    return ref


def _seq_sum32(terms):
    """fp32 sum over the last axis, one column after the other (the worst order a row sum can take)."""
    acc = np.zeros(terms.shape[:-1], np.float32)
    for c in range(terms.shape[-1]):
        acc = (acc + terms[..., c]).astype(np.float32)
    return acc


def classes32(y, t=None, K=0):
    """The arithmetic of include/vbnn_hip.h in plain fp32 NumPy, operation by operation, with sequential row sums: the dict
    check_classes takes (+ "rows": R x 3 = { sum H, sum -o[t], hits }, the row values of the ACCUMULATE state)."""
    f32 = np.float32
    S, R, C = y.shape
    rows = np.arange(R)
    L = sumH = nll = hits = None
    for s in range(S):
        ys = y[s]
        mx = ys.max(1)
        arg = ys.argmax(1)
        lse = (mx + np.log(_seq_sum32(np.exp((ys - mx[:, None]).astype(f32)).astype(f32))).astype(f32)).astype(f32)
        o = (ys - lse[:, None]).astype(f32)
        Hs = -_seq_sum32((np.exp(o).astype(f32) * o).astype(f32))
        if s == 0:
            L, sumH = o, Hs
        else:
            u = np.exp(-np.abs((L - o).astype(f32))).astype(f32)
            w = (f32(1) + u).astype(f32)                     # log1p(u) as the header evaluates it: log(w) u / (w - 1), u where w = 1
            with np.errstate(invalid="ignore", divide="ignore"):
                l1p = np.where(w == 1, u, ((np.log(w).astype(f32) * u).astype(f32) / (w - f32(1)).astype(f32)).astype(f32))
            L = (np.maximum(L, o) + l1p).astype(f32)
            sumH = (sumH + Hs).astype(f32)
        if t is not None:
            n, h = -o[rows, t], (arg == t).astype(f32)
            nll, hits = (n, h) if s == 0 else ((nll + n).astype(f32), (hits + h).astype(f32))
    lp = (L - np.log(f32(S)).astype(f32)).astype(f32)
    p = np.exp(lp).astype(f32)
    got = dict(log_probs=lp, probs=p, entropy=-_seq_sum32((p * lp).astype(f32)), expected_entropy=(sumH / f32(S)).astype(f32))
    got["mutual_info"] = (got["entropy"] - got["expected_entropy"]).astype(f32)
    order = np.argsort(-lp, axis=1, kind="stable")
    got["pred"] = order[:, 0].astype(np.int32)
    if K:
        got["topk_idx"] = order[:, :K].astype(np.int32)
        got["topk_prob"] = np.take_along_axis(p, order[:, :K], 1)
    if t is not None:
        in_top = (got["topk_idx"] == t[:, None]).any(1).sum() if K else 0
        got["totals"] = [float((-lp[rows, t]).astype(np.float64).sum()), float((got["pred"] == t).sum()),
                         float(nll.astype(np.float64).sum()), float(hits.astype(np.float64).sum()), float(in_top)]
        got["rows"] = np.stack([sumH, nll, hits], 1)
    return got


def logp_tol(ref, S):
    """|d log_p| <= (C + 4 S + 16) eps max(|log_p|, 1): the family's logsumexp bound with C in D's place."""
    C = ref["log_probs"].shape[1]
    return (C + 4 * S + 16) * EPS * np.maximum(np.abs(ref["log_probs"]), 1.0)


def probs_tol(ref, S):
    """relative (C + 4 S + 20) eps max(|log p|, 1); below the smallest normal fp32 the format itself gives out (TINY)."""
    C = ref["log_probs"].shape[1]
    return (C + 4 * S + 20) * EPS * np.maximum(np.abs(ref["log_probs"]), 1.0) * ref["probs"] + TINY


def entropy_tol(ref, S):
    """against the all-float64 entropy: (C + 16) eps relative + the log_probs bound carried through sum_c p log p."""
    C = ref["log_probs"].shape[1]
    p, lp = ref["probs"], ref["log_probs"]
    return (C + 16) * EPS * np.abs(ref["entropy"]) + (p * (1.0 + np.abs(lp)) * logp_tol(ref, S)).sum(1)


def expected_entropy_tol(ref):
    """(C + 16) eps relative + per draw the bound of o, (C + 16) eps max(|o|, 1), carried through sum_c exp(o) o."""
    o = ref["o"]
    C = o.shape[2]
    tol_o = (C + 16) * EPS * np.maximum(np.abs(o), 1.0)
    return (C + 16) * EPS * np.abs(ref["expected_entropy"]) + (np.exp(o) * (1.0 + np.abs(o)) * tol_o).sum(2).mean(0)


def check_classes(got, y, t=None, K=0, label=""):
    """got: dict of NumPy arrays (entropy, expected_entropy, mutual_info, pred; optionally probs, log_probs, topk_idx,
    topk_prob, and with t totals (5) and rows (R x 3, the ACCUMULATE state's row values)) against classes64(y, t). The bounds are
    the functions above; the order of the classes, the counts and the totals are exact (see the body). Returns the reference."""
    S, R, C = y.shape
    ref = classes64(y, t)
    rows = np.arange(R)
    tl, te, tx = logp_tol(ref, S), entropy_tol(ref, S), expected_entropy_tol(ref)
    msg = [f"{label} S {S} R {R} C {C} K {K}:"]
    lp = got.get("log_probs")
    if lp is not None:
        d = np.abs(lp - ref["log_probs"])
        msg.append(f"log_p err/tol {np.max(d / tl):.3f} (worst {np.max(d / np.maximum(np.abs(ref['log_probs']), 1.0)) / EPS:.1f} eps)")
        assert (d <= tl).all(), (label, "log_probs", float((d / tl).max()))
    p = got.get("probs")
    if p is not None:
        d, tp = np.abs(p - ref["probs"]), probs_tol(ref, S)
        msg.append(f"p err/tol {np.max(d / tp):.3f}")
        assert (d <= tp).all(), (label, "probs", float((d / tp).max()))
    for k, tol in (("entropy", te), ("expected_entropy", tx), ("mutual_info", te + tx)):
        d = np.abs(got[k] - ref[k])
        msg.append(f"{k} err/tol {np.max(d / tol):.3f}")
        assert (d <= tol).all(), (label, k, float((d / tol).max()))
    if p is not None and lp is not None:
        # the entropy is a sum of C terms: relative (C + 16) eps against the float64 sum of ITS terms, the returned fp32 p, log p
        terms = p.astype(np.float64) * lp.astype(np.float64)
        d, tol = np.abs(got["entropy"] + terms.sum(1)), (C + 16) * EPS * np.abs(terms).sum(1)
        msg.append(f"entropy against its own terms {np.max(d / np.maximum(tol, 1e-300)):.3f}")
        assert (d <= tol).all(), (label, "entropy of the returned terms")
    print(" ".join(msg))
    # ---- exact: the order of the classes is that of the returned log_probs, first maximum first
    idx = got.get("topk_idx")
    if lp is not None:
        order = np.argsort(-lp, axis=1, kind="stable")
        assert np.array_equal(got["pred"], order[:, 0]), (label, "pred")
        if K:
            assert np.array_equal(idx, order[:, :K]), (label, "topk_idx")
    if K:
        assert idx.shape == (R, K) and np.array_equal(got["pred"], idx[:, 0]), (label, "pred is topk_idx[:, 0]")
        if p is not None:
            want = np.take_along_axis(p, idx.astype(np.int64), 1)
            assert np.array_equal(got["topk_prob"].view(np.uint32), want.view(np.uint32)), (label, "topk_prob")
        # against float64, membership: every class above the K-th by more than the bound is in, none below it by more is
        kth = -np.sort(-ref["log_probs"], axis=1)[:, K - 1]
        bound = tl.max(1)
        inside = np.zeros((R, C), bool)
        inside[rows[:, None], idx] = True
        assert inside.sum(1).tolist() == [K] * R, (label, "topk_idx holds K different classes")
        assert inside[ref["log_probs"] > (kth + bound)[:, None]].all(), (label, "a class well above the K-th is missing")
        assert not inside[ref["log_probs"] < (kth - bound)[:, None]].any(), (label, "a class well below the K-th was returned")
    else:
        assert (got["pred"] >= 0).all() and (got["pred"] < C).all()
    if t is None or got.get("totals") is None:
        return ref
    tot = got["totals"]
    print(f"{label} totals {tot!r}")
    assert tot[1] == float((got["pred"] == t).sum()), (label, "totals[1]")
    assert tot[3] == float((y.argmax(2) == t[None]).sum()), (label, "totals[3]")
    assert tot[4] == (float((idx == t[:, None]).any(1).sum()) if K else 0.0), (label, "totals[4]")
    if lp is not None:               # the double sum of the returned fp32 rows
        want = (-lp[rows, t]).astype(np.float64).sum()
        assert abs(tot[0] - want) <= 1e-12 * abs(want), (label, "totals[0]", tot[0], want)
    assert abs(tot[0] - ref["nlp_t"].sum()) <= tl[rows, t].sum(), (label, "totals[0] against float64")
    if got.get("rows") is not None:  # ... and of the state's fp32 row values (ACCUMULATE keeps them; STACKED equals it bitwise)
        want = got["rows"][:, 1].astype(np.float64).sum()
        assert abs(tot[2] - want) <= 1e-12 * abs(want), (label, "totals[2]", tot[2], want)
        assert tot[3] == float(got["rows"][:, 2].astype(np.float64).sum())
    # a row's sum of S terms, each within the bound of o: S eps of the sum on top
    o_t = ref["nll_t"]
    tol2 = ((C + 16) * EPS * np.maximum(o_t, 1.0)).sum() + S * EPS * o_t.sum()
    assert abs(tot[2] - o_t.sum()) <= tol2, (label, "totals[2] against float64", tot[2], o_t.sum())
    return ref
