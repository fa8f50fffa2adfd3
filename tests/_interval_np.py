"""NumPy restatement for the tests of vbnn_conformal_interval and vbnn_select_columns (include/vbnn_hip.h,
vbnn_amd/csrc/conformal_interval.hip): fp32, one rounding per operation, and integers -- what the GPU tests compare bit for bit.
score32 / interval32 restate the two modes of the first call (scores, row scores, end points, covered, row_covered, every
accumulator word); select_columns32 restates the second as a plain SORT of order words, not as a radix walk; score64 is the
float64 definition; conformal_rank the rank k = ceil((n + 1) level) in exact arithmetic.

THE DERIVED BOUND of the fp32 score against float64 on the same fp32 inputs (score_bound), eps = 2^-24, every operation
correctly rounded, no underflow assumed on the way (a relative bound; tiny = 2^-126 is added once per operation that can round
a subnormal):
  absolute / cqr: s = max(a - t, t - b): ONE rounding, of the difference that wins, so |s32 - s| <= eps |s| -- unless the two
    differences round to different winners, which happens only where they agree within eps of the larger; the bound below uses
    eps * max(|a - t|, |t - b|), which covers both.
  scaled: v = (var + noise) + add: 2 roundings of non-negative terms, relative error <= 2 eps (1 + eps);  u = sqrt(v): half of
    that plus one rounding, <= 2 eps (first order) -- we take 2.5 eps to cover the second-order terms;  w = max(u, w_min):
    exact;  m: eps as above;  s = m / w: the errors of m and w add and the division rounds once more:
    |s32 - s| <= (1 + 2.5 + 1) eps |s| (1 + 8 eps) <= 4.6 eps |s|. The test uses 4.6 eps |s| + tiny: 100 % of the derived
    bound, no slack factor, and reports the share of it that the worst element uses."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32
MAX_Q = 8
QNAN_BITS = 0x7FC00000
QNAN = np.array([QNAN_BITS], np.uint32).view(F32)[0]
W_MIN = 2.0 ** -60


def order_word(x):
    """vbnn_order_word of fp32 values: sign clear -> b ^ 0x80000000, sign set -> ~b (uint32)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u >> 31, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def unorder_word(w):
    w = np.asarray(w, np.uint32)
    return np.where(w >> 31, w ^ np.uint32(0x80000000), ~w).astype(np.uint32).view(F32)


def keys(x):
    """vbnn_selective's key: the order word, every NaN taken as the positive quiet NaN (above +inf)."""
    x = np.ascontiguousarray(x, dtype=F32)
    return order_word(np.where(np.isnan(x), QNAN, x))


def conformal_rank(n, level):
    """k = ceil((n + 1) level), the level taken as the decimal number its repr shows (0.9 is nine tenths), in exact arithmetic."""
    x = (int(n) + 1) * Fraction(repr(float(level)))
    return int(-((-x.numerator) // x.denominator))


def width32(scale, scale2=None, scale_add=0.0, is_variance=True, w_min=W_MIN):
    """w of the header: ((scale [+ scale2]) + scale_add), its root for a variance, not below w_min; a NaN stays one."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.ascontiguousarray(scale, dtype=F32)
        if scale2 is not None:
            v = (v + np.asarray(scale2, F32)).astype(F32)
        v = (v + F32(scale_add)).astype(F32)
        u = np.sqrt(v).astype(F32) if is_variance else v
        return np.where(u < F32(w_min), F32(w_min), u).astype(F32)


def _score(a, b, t, w):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d1, d2 = (a - t).astype(F32), (t - b).astype(F32)
        m = np.where(d1 > d2, d1, d2)
        m = np.where(np.isnan(d1) | np.isnan(d2), QNAN, m).astype(F32)
        s = (m / w).astype(F32) if w is not None else m
        return np.where(np.isnan(s), QNAN, s).astype(F32)


def score32(lower, upper, target, w=None, acc=None):
    """Score mode. lower, upper: P x R x D fp32 (pads cut); target: R x D; w: R x D widths (width32) or None. Returns
    dict(score: P x R x D, row_score: P x R, acc: uint64[2] = `acc` + {NaN elements, rows with a NaN})."""
    A, B = np.ascontiguousarray(lower, dtype=F32), np.ascontiguousarray(upper, dtype=F32)
    assert A.ndim == 3 and A.shape == B.shape and 1 <= A.shape[0] <= MAX_Q
    t = np.asarray(target, F32)[None]
    s = _score(A, B, t, None if w is None else np.asarray(w, F32)[None])
    nan = np.isnan(s)
    word = np.where(nan, np.uint32(0), order_word(s)).max(axis=2)            # the maximum by order word: -0 below +0
    row = np.where(nan.any(axis=2), QNAN, unorder_word(word)).astype(F32)
    words = np.zeros(2, np.uint64) if acc is None else np.asarray(acc).astype(np.uint64).copy()
    words[0] += np.uint64(nan.sum())
    words[1] += np.uint64(nan.any(axis=2).sum())
    return dict(score=s, row_score=row, acc=words)


def n_words(Q):
    return 8 * Q + 2


def interval32(lower, upper, qhat, target=None, w=None, per_column=True, acc=None):
    """Interval mode. lower, upper: P x R x D with P = 1 or Q; qhat: Q x D (per_column) or Q (one per level) fp32; target R x D or
    None; w: R x D or None. Returns dict(lo, hi: Q x R x D; covered: Q x R x D uint8 (None without target); row_covered: Q x R
    int32 (None without target); acc: uint64[8 Q + 2])."""
    A, B = np.ascontiguousarray(lower, dtype=F32), np.ascontiguousarray(upper, dtype=F32)
    P, R, D = A.shape
    qhat = np.asarray(qhat, F32)
    Q = qhat.shape[0]
    assert 1 <= Q <= MAX_Q and P in (1, Q) and A.shape == B.shape
    q = qhat.reshape(Q, 1, D) if per_column else np.broadcast_to(qhat.reshape(Q, -1)[:, :1, None], (Q, 1, 1))
    q = np.where(np.isnan(q), F32(np.inf), q).astype(F32)
    if P == 1:
        A, B = np.broadcast_to(A, (Q, R, D)), np.broadcast_to(B, (Q, R, D))
    W = None if w is None else np.asarray(w, F32)[None]
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(A) | np.isnan(B)
        if W is not None:
            nan = nan | np.isnan(W)
        if target is not None:
            s = _score(A, B, np.asarray(target, F32)[None], W)
            nan = nan | np.isnan(s)
        qw = (q * W).astype(F32) if W is not None else np.broadcast_to(q, (Q, R, D))
        lo, hi = (A - qw).astype(F32), (B + qw).astype(F32)
        empty = (lo > hi) & ~nan
        lo, hi = np.where(nan, QNAN, lo).astype(F32), np.where(nan, QNAN, hi).astype(F32)
        cov = (s <= q) & ~nan if target is not None else np.zeros((Q, R, D), bool)
    rown = nan.any(axis=2)
    words = np.zeros(n_words(Q), np.uint64) if acc is None else np.asarray(acc).astype(np.uint64).copy()
    for j in range(Q):
        add = [(~nan[j]).sum(), cov[j].sum(), (~rown[j]).sum(), (cov[j].all(axis=1) & ~rown[j]).sum(), empty[j].sum(), 0, 0, 0]
        if target is None:
            add[1] = add[3] = 0
        words[8 * j:8 * j + 8] += np.array(add, np.uint64)
    planes = range(Q) if P > 1 else range(1)
    words[8 * Q] += np.uint64(sum(int(nan[j].sum()) for j in planes))
    words[8 * Q + 1] += np.uint64(sum(int(rown[j].sum()) for j in planes))
    out = dict(lo=lo, hi=hi, acc=words, covered=None, row_covered=None, nan=nan)
    if target is not None:
        out["covered"] = np.where(nan, 255, cov).astype(np.uint8)
        out["row_covered"] = np.where(rown, -1, cov.sum(axis=2)).astype(np.int32)
    return out


def select_columns32(x, ks):
    """vbnn_select_columns by a plain sort: x R x D fp32, ks the 1-based ranks. Returns dict(tau: Q x D fp32, counts: Q x D x 2
    uint32 {keys below, keys tied}, n_nan: D uint32)."""
    x = np.ascontiguousarray(x, dtype=F32)
    R, D = x.shape
    key = keys(x)
    srt = np.sort(key, axis=0)
    Q = len(ks)
    tau = np.empty((Q, D), F32)
    counts = np.empty((Q, D, 2), np.uint32)
    for j, k in enumerate(ks):
        assert 1 <= k <= R
        kw = srt[k - 1]
        tau[j] = unorder_word(kw)
        counts[j, :, 0] = (key < kw[None]).sum(axis=0)
        counts[j, :, 1] = (key == kw[None]).sum(axis=0)
    return dict(tau=tau, counts=counts, n_nan=np.isnan(x).sum(axis=0).astype(np.uint32))


def calibrate32(score, levels, scope="per_output"):
    """The thresholds of a calibration set: score n x D (per_output: one per column) or n row scores (joint). k > n gives +inf.
    Returns (qhat: Q x D or Q x 1 fp32, k)."""
    score = np.asarray(score, F32)
    if scope == "joint":
        score = score.reshape(-1, 1)
    n, D = score.shape
    k = [conformal_rank(n, v) for v in levels]
    qhat = np.full((len(k), D), np.inf, F32)
    inside = [j for j, kj in enumerate(k) if kj <= n]
    if inside:
        qhat[inside] = select_columns32(score, [k[j] for j in inside])["tau"]
    return qhat, k


def score64(a, b, t, w64=None):
    """The float64 definition on the same fp32 inputs (w64: the float64 width, or None)."""
    a, b, t = (np.asarray(v, F32).astype(np.float64) for v in (a, b, t))
    m = np.maximum(a - t, t - b)
    return m / w64 if w64 is not None else m


def width64(scale, scale2=None, scale_add=0.0, is_variance=True, w_min=W_MIN):
    v = np.asarray(scale, F32).astype(np.float64)
    if scale2 is not None:
        v = v + np.asarray(scale2, F32).astype(np.float64)
    v = v + float(F32(scale_add))
    u = np.sqrt(v) if is_variance else v
    return np.maximum(u, float(F32(w_min)))


def score_bound(a, b, t, s64, scaled):
    a, b, t = (np.asarray(v, F32).astype(np.float64) for v in (a, b, t))
    if not scaled:
        return EPS * np.maximum(np.abs(a - t), np.abs(t - b)) + TINY
    return 4.6 * EPS * np.abs(s64) + TINY
