"""NumPy restatements for the Bernoulli likelihood head's tests: vbnn_bce_forward (the criterion) and vbnn_predict_label_moments
(the multi-label predictive), each twice -- a float64 reference evaluated on the fp32 inputs the kernel saw, and an fp32
restatement that follows include/vbnn_hip.h operation by operation (every intermediate rounded to fp32, the row sums formed in
the family's order: thread i of T = 64 (D <= 256) or 256 adds the columns of its quads i, i + T, ... in ascending order, then the
xor butterfly 32 .. 1 inside a wave, then the four waves in wave order) -- with the bounds the tests hold either to.

THE BOUNDS ARE DERIVED, not measured. eps = 2^-24 is the unit roundoff of fp32: one correctly rounded operation (+, -, *, /) is
off by at most eps relative; the library's expf / logf / log1pf are taken as 1-ulp functions (2 eps relative), which is what the
project's other restatements assume ("a 1-ulp expf"). Second-order terms are covered by rounding every count up.

  l1p = (logf(w) * u) / (w - 1), w = fl(1 + u), against log1p(u) of the exact u = exp(-|z|): u carries 2 eps (expf), which
    log1p passes on as at most 2 eps of itself (u / (1 + u) <= log1p(u)); w - 1 is exact; evaluating log(1 + x) / x at x = w - 1
    instead of u moves it by at most eps ((1 + u) eps of argument, the function's log-slope is at most 1/2 in magnitude); logf 2
    eps, the product and the quotient one each: 7 eps, taken as L1P_K = 8. Where w == 1 (u < eps) l1p = u is off by u / 2.
  criterion element e = (max(z, 0) - z t) + l1p: the product eps |z| t, the difference eps (max(z, 0) + |z| t), l1p 8 eps, the sum
    eps (all three): at most 9 eps (|z| t + max(z, 0) + l1p), taken as LOSS_K = 10 against inv_nd sum (|z| t + max(z, 0) + l1p);
    the sum itself is formed in double.
  sig = 1 / w or u / w: w one rounding and u's 2 eps (at most eps of 1 / w), the quotient one, u itself 2: at most 5 eps sig.
    g = inv_nd (sig - t): the difference and the product one each: 5 eps sig + 2 eps |sig - t|, taken as
    G_K = 8 against inv_nd (sig + |sig - t|). At z = 0, t = 1/2 every operation is exact: g = +0 bitwise.
    The criterion does not clamp z: past |z| ~ 87 u and u / w fall below the smallest normal fp32, TINY = 2^-126, where a
    rounding (or a flush to zero) is an absolute error of at most TINY instead of a relative one: the element bounds of the
    criterion carry + TINY (times inv_nd). The predictive's clamp at 80 keeps every value it forms normal.
  predictive, per draw: p and q as sig (5 eps each); lp = min(zc, 0) - l1p: 8 eps l1p + eps |lp| <= 9 eps |lp|, ln alike;
    h = -(p lp + q ln): per product 5 + 9 + 1, the sum 1: 16 eps h (both terms have one sign).
  P = sum_s p (S - 1 additions of positive terms), pm = P / S: (S + 5) eps pm, taken as (S + 6) eps pm; qm alike.
  log_p = logf(pm): 2 eps |log_p| + (S + 6) eps, taken as 2 eps |log_p| + (S + 7) eps.
  entropy = -(pm log_p + qm log_q): per product (S + 6) + 2 + 1 relative and (S + 7) eps pm absolute, the sum one:
    (S + 10) eps entropy + (S + 7) eps (pm + qm), taken as ENT: (S + 10) eps (entropy + 1).
  expected_entropy = (sum_s h) / S: 16 + (S - 1) + 1 = (S + 16) eps of itself.
  mutual_info = entropy - expected_entropy: the two above plus eps |mutual_info|.
  a_s = sum_d (t lp + (1 - t) ln): per element 9 + 1 and 1 + 9 + 1, the sum one: 12 eps |term| (one sign); the row sum adds at
    most D eps of the magnitudes: (D + 12) eps, taken as ROW: (D + 32) eps |a_s| -- the form of tests/_gauss_np.nll_bound.
  sum_s -a_s: an fp32 running sum of S values, each within its bound: sum_s bound_s + S eps sum_s |a_s|.
  row_log_lik = L - logf(S), L the online logsumexp: logsumexp moves by at most the largest error of its arguments; each of the
    S - 1 steps rounds |L - a|, expf (2 eps of a value <= 1), log1pf (2 eps of a value <= log 2) and the sum (eps |L|): at most
    4 eps max(|L|, 1) a step; logf(S) and the last difference: the largest bound of the a_s + (4 S + 16) eps max(|row_log_lik|, 1)
    -- tests/_gauss_np.check_gauss_moments' form.
  row_marg_log_lik = sum_d (t log_p + (1 - t) log_q): per element the logs' 2 eps |log| + (S + 7) eps weighted by t and 1 - t
    (which add to one), three roundings: 5 eps |term| + (S + 7) eps; the row sum D eps: (D + 32) eps |row| + D (S + 7) eps.
  row_entropy, row_mutual_info: (D + 16) eps of the summed magnitudes plus the elements' bounds.
  hits: P > Q is decided as in float64 wherever |P64 - Q64| > (S + 6) eps S (P is within (S + 5) eps P, Q within
    (S + 5) eps Q, and P + Q <= S (1 + 6 eps)); TIE is twice that, 2 (S + 6) eps S, so that the returned probs = P / S, itself
    within (S + 6) eps / 2 of the exact one near 1/2, lies on the same side of 1/2 as well; the tests choose inputs with no element inside it and assert so,
    then hold EVERY element's predicted label and every hit count to float64 exactly.
"""
import numpy as np

EPS = 2.0 ** -24
CLAMP = 80.0
L1P_K, LOSS_K, G_K = 8, 10, 8
TINY = 2.0 ** -126                    # the smallest normal fp32


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _expf(x):
    """A correctly rounded fp32 exp (float64 exp, rounded): a 1-ulp expf."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(x.astype(np.float64)).astype(np.float32)


def _logf(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.astype(np.float64)).astype(np.float32)


def _log1pf(x):
    return np.log1p(x.astype(np.float64)).astype(np.float32)


def _l1p32(u, w):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (_logf(w) * u) / (w - np.float32(1))
    return np.where(w == np.float32(1), u, r).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the criterion
def criterion64(z, t, inv_nd):
    """float64 on the fp32 inputs: loss = inv_nd sum e, g = inv_nd (sig - t), hits (a NaN logit is a miss), and the magnitudes
    the bounds are stated against."""
    inv_nd = float(np.float32(inv_nd))
    z, t = np.asarray(z, dtype=np.float64), np.asarray(t, dtype=np.float64)
    u = np.exp(-np.abs(z))
    l1p = np.log1p(u)
    e = np.maximum(z, 0.0) - z * t + l1p
    e = np.where(np.isnan(z), np.nan, e)
    sig = np.where(z >= 0, 1.0 / (1.0 + u), u / (1.0 + u))
    sig = np.where(np.isnan(z), np.nan, sig)
    mag = np.abs(z) * t + np.maximum(z, 0.0) + l1p
    hits = int((~np.isnan(z) & ((z > 0) == (t > 0.5))).sum())
    return dict(loss=inv_nd * e.sum(), g=inv_nd * (sig - t), hits=hits, loss_mag=inv_nd * np.nansum(mag),
                g_mag=inv_nd * (sig + np.abs(sig - t)))


def criterion32(z, t, inv_nd):
    """The header, op by op in fp32; the element sum in float64, as the kernel's double partials."""
    z, t, inv = _f32(z), _f32(t), np.float32(inv_nd)
    one = np.float32(1)
    with np.errstate(invalid="ignore"):
        u = _expf(-np.abs(z))
        w = one + u
        l1p = _l1p32(u, w)
        relu = np.where(z > 0, z, np.float32(0)).astype(np.float32)          # fmaxf(z, 0): a NaN gives 0
        e = (relu - z * t) + l1p
        sig = np.where(z >= 0, one / w, u / w).astype(np.float32)
        g = (inv * (sig - t)).astype(np.float32)
        hits = int((~np.isnan(z) & ((z > 0) == (t > np.float32(0.5)))).sum())
    return dict(loss=float(inv) * float(e.astype(np.float64).sum()), g=g, hits=hits)


def check_criterion(loss, g, hits, z, t, inv_nd, label=""):
    """loss (float or None), g (N x D fp32) and hits (int or None) of an implementation against criterion64 on the same inputs.
    Prints the share of each bound in use. Returns the reference."""
    ref = criterion64(z, t, inv_nd)
    ok = ~np.isnan(np.asarray(z, dtype=np.float64))
    inv = float(np.float32(inv_nd))
    dg = np.abs(np.asarray(g, dtype=np.float64) - ref["g"])[ok] / (G_K * EPS * ref["g_mag"][ok] + inv * TINY)
    print(f"{label}: g err/bound {dg.max() if dg.size else 0.0:.3f}")
    assert (dg <= 1.0).all(), (label, float(dg.max()))
    assert np.isnan(np.asarray(g)[~ok]).all(), label
    if hits is not None:
        assert hits == ref["hits"], (label, hits, ref["hits"])
    if loss is not None:
        if ok.all():
            dl = abs(loss - ref["loss"]) / (LOSS_K * EPS * ref["loss_mag"] + inv * TINY * ok.size)
            print(f"{label}: loss {loss!r} want {ref['loss']!r}, err/bound {dl:.3f}")
            assert dl <= 1.0, (label, loss, ref["loss"])
        else:
            assert np.isnan(loss), (label, loss)
    return ref


# ------------------------------------------------------------------------------------------------ the predictive
def _clamp(z):
    return np.where(np.isnan(z), z, np.minimum(np.maximum(z, -CLAMP), CLAMP))


def draw_terms64(y):
    """Per draw and element in float64 (y: .. fp32 logits): p, q, lp, ln."""
    zc = _clamp(np.asarray(y, dtype=np.float64))
    u = np.exp(-np.abs(zc))
    l1p = np.log1p(u)
    pos = zc >= 0
    p, q = np.where(pos, 1.0 / (1.0 + u), u / (1.0 + u)), np.where(pos, u / (1.0 + u), 1.0 / (1.0 + u))
    lp, ln = np.minimum(zc, 0.0) - l1p, np.minimum(-zc, 0.0) - l1p
    nan = np.isnan(zc)
    return tuple(np.where(nan, np.nan, v) for v in (p, q, lp, ln))


def label_moments64(y, t=None):
    """The float64 reference on fp32 inputs: y S x R x D logits, t R x D. P, Q (the sums over draws), probs, entropy,
    expected_entropy, mutual_info (exactly 0 for S = 1), pred (P > Q), row_entropy, row_mutual_info; with t: a (S x R),
    row_log_lik, row_marg_log_lik, hit (R x D), row_hits, totals."""
    S, R, D = y.shape
    p, q, lp, ln = draw_terms64(y)
    P, Q = p.sum(0), q.sum(0)
    pm, qm = P / S, Q / S
    log_p, log_q = np.log(pm), np.log(qm)
    ent = -(pm * log_p + qm * log_q)
    ee = (-(p * lp + q * ln)).sum(0) / S
    mi = np.zeros_like(ent) if S == 1 else ent - ee
    mi = np.where(np.isnan(ent), np.nan, mi)
    ref = dict(P=P, Q=Q, probs=pm, qm=qm, log_p=log_p, log_q=log_q, entropy=ent, expected_entropy=ee, mutual_info=mi, pred=P > Q,
               row_entropy=ent.sum(1), row_mutual_info=mi.sum(1))
    if t is not None:
        t = np.asarray(t, dtype=np.float64)
        a = (t[None] * lp + (1.0 - t[None]) * ln).sum(2)
        top = a.max(0)
        ref["a"] = a
        ref["row_log_lik"] = top + np.log(np.exp(a - top).sum(0)) - np.log(S)
        ref["row_marg_log_lik"] = (t * log_p + (1.0 - t) * log_q).sum(1)
        ref["hit"] = ~np.isnan(P) & (ref["pred"] == (t > 0.5))
        ref["row_hits"] = ref["hit"].sum(1)
        ref["totals"] = [ref["row_log_lik"].sum(), ref["row_marg_log_lik"].sum(), -a.sum(), float(ref["row_hits"].sum()),
                         float((ref["row_hits"] == D).sum())]
    return ref


def tie_margin(ref, S):
    """|P64 - Q64| / TIE per element: above 1 the fp32 comparison P > Q is decided as in float64."""
    return np.abs(ref["P"] - ref["Q"]) / (2 * (S + 6) * EPS * S)


def row_sum32(x):
    """The family's row sum of x (R x D fp32), in fp32, in the kernel's order. Every thread starts from +0."""
    x = _f32(x)
    R, D = x.shape
    T = 64 if D <= 256 else 256
    nq = (D + 3) // 4
    per = (nq + T - 1) // T
    pad = np.zeros((R, per * T * 4), np.float32)
    pad[:, :D] = x
    xs = pad.reshape(R, per, T, 4)
    acc = np.zeros((R, T), np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(per):
            for j in range(4):
                acc = acc + xs[:, k, :, j]
        v = acc.reshape(R, T // 64, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lanes ^ off]
        w = v[:, :, 0]
        if T == 64:
            return w[:, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def label_moments32(y, t=None):
    """The header, op by op in fp32 (both forms of the kernel run exactly this per draw). Returns the kernel's outputs: probs,
    entropy, mutual_info, row_entropy, row_mutual_info, P, Q; with t row_log_lik, row_marg_log_lik, row_hits (int32), totals."""
    y = _f32(y)
    S, R, D = y.shape
    one, zero = np.float32(1), np.float32(0)
    has_t = t is not None
    if has_t:
        t = _f32(t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            z = y[s]
            zc = np.where(np.isnan(z), z, np.minimum(np.maximum(z, np.float32(-CLAMP)), np.float32(CLAMP))).astype(np.float32)
            u = _expf(-np.abs(zc))
            w = one + u
            l1p = _l1p32(u, w)
            big, small = one / w, u / w
            pos = zc >= 0
            p, q = np.where(pos, big, small).astype(np.float32), np.where(pos, small, big).astype(np.float32)
            fmin0 = lambda v: np.where(v < 0, v, zero).astype(np.float32)        # fminf(v, 0): a NaN gives 0
            lp, ln = fmin0(zc) - l1p, fmin0(-zc) - l1p
            h = -(p * lp + q * ln)
            P, Q, Hs = (p, q, h) if s == 0 else (P + p, Q + q, Hs + h)
            if has_t:
                a = row_sum32(t * lp + (one - t) * ln)
                if s == 0:
                    nsum, L = -a, a
                else:
                    nsum = nsum + (-a)
                    L = (np.fmax(L, a) + _log1pf(_expf(-np.abs(L - a)))).astype(np.float32)     # fmaxf; a NaN passes through |L - a|
        Sf = np.float32(S)
        pm, qm = P / Sf, Q / Sf
        log_p, log_q = _logf(pm), _logf(qm)
        ent = -(pm * log_p + qm * log_q)
        ee = Hs / Sf
        mi = np.zeros_like(ent) if S == 1 else (ent - ee).astype(np.float32)
        out = dict(probs=pm, entropy=ent, mutual_info=mi, row_entropy=row_sum32(ent), row_mutual_info=row_sum32(mi), P=P, Q=Q)
        if has_t:
            out["row_log_lik"] = (L - _logf(np.full(R, S, np.float32))).astype(np.float32)
            out["row_marg_log_lik"] = row_sum32(t * log_p + (one - t) * log_q)
            hit = ~np.isnan(P) & ((P > Q) == (t > np.float32(0.5)))
            hits = row_sum32(hit.astype(np.float32))
            out["row_hits"] = hits.astype(np.int32)
            out["totals"] = [float(out["row_log_lik"].astype(np.float64).sum()), float(out["row_marg_log_lik"].astype(np.float64).sum()),
                             float(nsum.astype(np.float64).sum()), float(hits.astype(np.float64).sum()), float((hits == np.float32(D)).sum())]
    return out


def a_bound(ref, D):
    """ROW: (D + 32) eps |a_s| per draw and row."""
    return (D + 32) * EPS * np.abs(ref["a"])


def check_label_moments(got, y, t=None, label=""):
    """got: dict of NumPy arrays (probs, entropy, mutual_info, row_entropy, row_mutual_info; with t row_log_lik,
    row_marg_log_lik, row_hits, totals) against label_moments64(y, t) within the module's bounds. The inputs must be free of
    NaN and of near ties (asserted). Prints the share of each bound in use. Returns the reference."""
    S, R, D = y.shape
    ref = label_moments64(y, t)
    assert not np.isnan(ref["P"]).any()
    margin = tie_margin(ref, S)
    assert (margin > 1.0).all(), (label, "an element within the bound of a tie", float(margin.min()))
    use = {}

    def hold(name, err, tol):
        share = float(np.max(np.asarray(err) / np.maximum(np.asarray(tol), 1e-300)))
        use[name] = share
        assert share <= 1.0, (label, name, share)

    p_tol = (S + 6) * EPS * ref["probs"]
    ent_tol = (S + 10) * EPS * (ref["entropy"] + 1.0)
    ee_tol = (S + 16) * EPS * ref["expected_entropy"]
    mi_tol = ent_tol + ee_tol + EPS * np.abs(ref["mutual_info"])
    hold("probs", np.abs(got["probs"] - ref["probs"]), p_tol)
    hold("entropy", np.abs(got["entropy"] - ref["entropy"]), ent_tol)
    if S == 1:
        assert not np.ascontiguousarray(got["mutual_info"]).view(np.uint32).any(), label        # +0 bitwise
        assert not np.ascontiguousarray(got["row_mutual_info"]).view(np.uint32).any(), label
    else:
        hold("mutual_info", np.abs(got["mutual_info"] - ref["mutual_info"]), mi_tol)
        hold("row_mutual_info", np.abs(got["row_mutual_info"] - ref["row_mutual_info"]),
             (D + 16) * EPS * (np.abs(ref["mutual_info"]) + mi_tol).sum(1) + mi_tol.sum(1))
    hold("row_entropy", np.abs(got["row_entropy"] - ref["row_entropy"]), (D + 16) * EPS * ref["row_entropy"] + ent_tol.sum(1))
    # the predicted label of EVERY element, from the returned probabilities
    assert np.array_equal(got["probs"] > 0.5, ref["pred"]), label
    if t is not None:
        assert np.array_equal(got["row_hits"], ref["row_hits"]), (label, got["row_hits"], ref["row_hits"])
        ab = a_bound(ref, D)
        ll = got["row_log_lik"].astype(np.float64)
        hold("row_log_lik", np.abs(ll - ref["row_log_lik"]), ab.max(0) + (4 * S + 16) * EPS * np.maximum(np.abs(ref["row_log_lik"]), 1.0))
        marg = got["row_marg_log_lik"].astype(np.float64)
        hold("row_marg_log_lik", np.abs(marg - ref["row_marg_log_lik"]),
             (D + 32) * EPS * np.abs(ref["row_marg_log_lik"]) + D * (S + 7) * EPS)
        tot = got.get("totals")
        if tot is not None:
            assert len(tot) == 5
            assert abs(tot[0] - ll.sum()) <= 1e-12 * max(np.abs(ll).sum(), 1e-300), (label, tot[0], ll.sum())
            assert abs(tot[1] - marg.sum()) <= 1e-12 * max(np.abs(marg).sum(), 1e-300), (label, tot[1], marg.sum())
            hold("totals[2]", abs(tot[2] - ref["totals"][2]), ab.sum() + S * EPS * np.abs(ref["a"]).sum())
            assert tot[3] == ref["totals"][3] and tot[4] == ref["totals"][4], (label, tot, ref["totals"])
    print(f"{label} S {S} R {R} D {D}: share of each bound in use: " + ", ".join(f"{k} {v:.3f}" for k, v in use.items()))
    return ref
