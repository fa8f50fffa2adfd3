"""NumPy restatement for the tests of vbnn_conformal (include/vbnn_hip.h, vbnn_amd/csrc/conformal.hip): conformal32 restates the
call in fp32 and integers -- the ranking of a row by order word and index, the masked row sum in the family's order (row_sum32:
the order of _calibration_np.row_sumsq32 without the squares), the sets, the accumulator's words -- and is what the GPU tests
compare bit for bit. brute32 scores EVERY class and compares EVERY class (C masked sums a row), the form the restatement is held
to on the CPU; scores64 is the float64 definition; conformal_rank is the rank k = ceil((n + 1) level) in exact arithmetic.

WHY THE SET IS A PREFIX OF THE RANKING (what conformal32's bisection and the kernel's both rest on). Number a row's classes by
rank: c_1 (the largest order word; among equal words the lowest index), c_2, ... The score of c_i is s_i.
  LAC: s_i = fl(1 - p[c_i]). p does not increase along the ranking (equal words: equal values; -0 and +0 give the same 1), and
    x -> fl(1 - x) is monotone non-increasing because rounding is monotone. So s_1 <= s_2 <= ...
  APS: s_i = the row sum, in ONE fixed tree of fp32 additions that depends on C alone, of the terms m_c = p[c] for c in
    {c_1 .. c_i} and +0 for the others. Going from i to i + 1 replaces one leaf +0 by p[c_{i+1}] >= 0 (for a -0 the leaf's effect
    on any node is the same as +0's, since every partial starts at +0 and +0 + -0 = +0). A rounded addition fl(a + b) is monotone
    non-decreasing in a and in b, so by induction up the tree no node decreases: s_i <= s_{i+1}, in fp32, exactly.
  Hence { j : s_j <= q } = { c_1 .. c_n } with n the largest i with s_i <= q: one boundary names the set, a bisection over i finds
  it with log2(C) masked sums, and covered = [s(t) <= q] is the member bit of t. Nothing of this needs the probabilities to sum
  to one or the fp32 sum to be accurate.

THE DERIVED BOUND of the fp32 APS score against float64 (aps_bound), eps = 2^-24, probabilities in [0, 1]: a term enters the tree
unrounded and passes at most n_add additions -- 4 per quad its thread owns (per = ceil(ceil(C / 4) / T) quads, T = 64 for C <= 256
and 256 above), 6 butterfly levels, 3 more for the four waves of a T = 256 row -- so |s32 - s| <= gamma s with gamma = n eps /
(1 - n eps), n = 4 per + 6 + 3 (all terms >= 0: the bound is relative to s itself). LAC: |fl(1 - p) - (1 - p)| <= eps |1 - p|."""
from fractions import Fraction

import numpy as np

from tests._calibration_np import threads_per_row

EPS = 2.0 ** -24
F32 = np.float32
LAC, APS = 0, 1
MAX_Q = 8
QNAN_BITS = 0x7FC00000


def order_word(x):
    """vbnn_order_word of fp32 values: sign clear -> b ^ 0x80000000, sign set -> ~b (uint32)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u >> 31, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def ranking(P):
    """order[r, i] = the class of rank i (0-based) of row r: larger order word first, ties to the lower index."""
    return np.argsort(~order_word(P), axis=1, kind="stable")


def positions(order):
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(order.shape[1]), order.shape), axis=1)
    return pos


def row_sum32(X):
    """sum_c X[r, c] in fp32 in the family's order (R x C fp32 in, R fp32 out): thread i of T adds to +0, in ascending order, the
    columns of its quads i, i + T, ...; the xor butterfly 32 .. 1 inside a wave; the waves in wave order."""
    X = np.ascontiguousarray(X, dtype=F32)
    R, C = X.shape
    T = threads_per_row(C)
    per = -(-((C + 3) // 4) // T)
    Z = np.zeros((R, per * T * 4), F32)                      # (a column past C adds +0)
    Z[:, :C] = X
    Z = Z.reshape(R, per, T, 4)
    v = np.zeros((R, T), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(per):
            for j in range(4):
                v = v + Z[:, k, :, j]
        v = v.reshape(R, T // 64, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lanes ^ off]
        w = v[:, :, 0]
        return w[:, 0] if T == 64 else ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def masked_sum32(P, mask):
    return row_sum32(np.where(mask, P, F32(0)))


def clamp_targets(target, C):
    return np.clip(np.asarray(target).astype(np.int64), 0, C - 1)


def n_words(Q):
    return 8 * Q + 2


def member_words(C):
    return (C + 31) // 32


def conformal32(probs, target, kind, qhat=(), acc=None):
    """vbnn_conformal on NumPy arrays: probs (R x C fp32; pad columns already cut), target (R int32 or None), kind LAC / APS, qhat
    (Q fp32 thresholds). Returns dict(score: R fp32 (None without target); size, cut_index, covered: Q x R int32; cut_prob: Q x R
    fp32; member: Q x R x ceil(C / 32) uint32; acc: uint64[8 Q + 2], `acc` + this call's adds; n: the prefix lengths with the NaN
    rows at 0; order: the ranking)."""
    P = np.ascontiguousarray(probs, dtype=F32)
    R, C = P.shape
    qhat = np.asarray(qhat, F32).reshape(-1)
    Q = qhat.size
    assert 0 <= Q <= MAX_Q and kind in (LAC, APS)
    rows = np.arange(R)
    nan = np.isnan(row_sum32(P))
    Pc = np.where(nan[:, None], F32(0), P)                   # (the NaN rows are overwritten below)
    order = ranking(Pc)
    pos = positions(order)
    qn = np.array([QNAN_BITS], np.uint32).view(F32)[0]
    out = dict(order=order, nan=nan)
    with np.errstate(invalid="ignore"):
        if target is not None:
            t = clamp_targets(target, C)
            if kind == LAC:
                score = (F32(1) - Pc[rows, t]).astype(F32)
            else:
                score = masked_sum32(Pc, pos <= pos[rows, t][:, None])
            out["score"] = np.where(nan, qn, score).astype(F32)
        else:
            t, score = None, None
            out["score"] = None
        size = np.zeros((Q, R), np.int32)
        for q in range(Q):
            qh = F32(np.inf) if np.isnan(qhat[q]) else qhat[q]
            if kind == LAC:
                size[q] = ((F32(1) - Pc) <= qh).sum(1)       # (a prefix: test_conformal_ref.py)
            else:
                lo, hi = np.zeros(R, np.int64), np.full(R, C + 1, np.int64)      # s_lo <= qh (the empty set always), s_hi > qh
                while (hi - lo > 1).any():
                    mid = (lo + hi) // 2
                    ok = masked_sum32(Pc, pos < mid[:, None]) <= qh
                    go = hi - lo > 1
                    lo = np.where(go & ok, mid, lo)
                    hi = np.where(go & ~ok, mid, hi)
                size[q] = lo
            size[q][nan] = 0
    member_b = pos[None, :, :] < size[:, :, None]            # Q x R x C
    nw = member_words(C)
    bits = np.zeros((Q, R, nw * 32), np.uint64)
    bits[:, :, :C] = member_b
    member = (bits.reshape(Q, R, nw, 32) << np.arange(32, dtype=np.uint64)).sum(3).astype(np.uint32)
    last = order[rows[None, :], np.maximum(size - 1, 0)]     # Q x R
    cut_index = np.where(size > 0, last, -1).astype(np.int32)
    cut_prob = np.where(size > 0, Pc[rows[None, :], last].view(np.uint32), np.uint32(QNAN_BITS)).astype(np.uint32).view(F32)
    if target is not None:
        qh_all = np.where(np.isnan(qhat), F32(np.inf), qhat).astype(F32)
        with np.errstate(invalid="ignore"):
            covered = (score[None, :] <= qh_all[:, None]).astype(np.int32)
    else:
        covered = np.zeros((Q, R), np.int32)
    words = np.zeros(n_words(Q), np.uint64) if acc is None else np.asarray(acc).astype(np.uint64).copy()
    ok = ~nan
    for q in range(Q):
        s, c = size[q][ok].astype(np.uint64), covered[q][ok] != 0
        add = [ok.sum(), c.sum(), s.sum(), (s == 0).sum(), (s == 1).sum(), ((s == 1) & c).sum(), (s == C).sum(), 0]
        if target is None:
            add[1] = add[5] = 0
        words[8 * q:8 * q + 8] += np.array(add, np.uint64)
    words[8 * Q] += np.uint64(nan.sum())
    out["n"] = size.copy()
    out["size"] = np.where(nan[None, :], -1, size).astype(np.int32)
    out["cut_index"] = np.where(nan[None, :], -1, cut_index).astype(np.int32)
    out["cut_prob"] = np.where(nan[None, :], qn, cut_prob).astype(F32)
    out["covered"] = np.where(nan[None, :], -1, covered).astype(np.int32) if target is not None else None
    out["member"] = np.where(nan[None, :, None], np.uint32(0), member).astype(np.uint32)
    out["acc"] = words
    return out


def scores_all32(P, kind):
    """s(r, j) for EVERY class j, each from its own masked sum over the classes that rank at or above j (C sums a row)."""
    P = np.ascontiguousarray(P, dtype=F32)
    R, C = P.shape
    if kind == LAC:
        return (F32(1) - P).astype(F32)
    pos = positions(ranking(P))
    S = np.empty((R, C), F32)
    for j in range(C):
        S[:, j] = masked_sum32(P, pos <= pos[:, j][:, None])
    return S


def brute32(P, kind, qhat):
    """The sets by definition: dict(member: Q x R x C bool = [s(r, j) <= qhat[q]], scores: R x C). No ranking is assumed."""
    S = scores_all32(P, kind)
    qh = np.where(np.isnan(qhat), F32(np.inf), np.asarray(qhat, F32))
    return dict(member=S[None, :, :] <= qh[:, None, None], scores=S)


def scores64(P, kind):
    """The float64 definition of every class's score on the same fp32 probabilities (the ranking is part of the definition)."""
    P64 = np.ascontiguousarray(P, dtype=F32).astype(np.float64)
    if kind == LAC:
        return 1.0 - P64
    order = ranking(P)
    cum = np.cumsum(np.take_along_axis(P64, order, 1), axis=1)
    S = np.empty_like(P64)
    np.put_along_axis(S, order, cum, axis=1)
    return S


def aps_bound(C, s64):
    T = threads_per_row(C)
    per = -(-((C + 3) // 4) // T)
    n = 4 * per + 6 + 3
    return n * EPS / (1.0 - n * EPS) * s64


def lac_bound(s64):
    return EPS * np.abs(s64)


def conformal_rank(n, level):
    """k = ceil((n + 1) level), the level taken as the decimal number its repr shows (0.9 is nine tenths), in exact arithmetic."""
    x = (n + 1) * Fraction(repr(float(level)))
    return int(-((-x.numerator) // x.denominator))


def derived(acc, Q, C=None):
    """What the host derives from the integers, float64, per threshold."""
    a = [int(v) for v in acc]
    out = []
    for q in range(Q):
        n, cov, ssum, empty, single, csingle, full = a[8 * q:8 * q + 7]
        nanv = float("nan")
        out.append(dict(n=n, coverage=cov / n if n else nanv, mean_size=ssum / n if n else nanv,
                        empty_fraction=empty / n if n else nanv, singleton_fraction=single / n if n else nanv,
                        singleton_accuracy=csingle / single if single else nanv, full_fraction=full / n if n else nanv))
    return out, a[8 * Q]


def tied_case(R, C, seed=3, levels=16):
    """Probabilities quantised to 1 / levels: large tie groups, a cut inside a group."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels + 1, (R, C)) / levels).astype(F32)
