"""NumPy restatement for the tests of vbnn_rank_metrics (include/vbnn_hip.h, vbnn_amd/csrc/ranking.hip): rank_metrics restates the
call in integers -- the order words of the fp32 scores, a stable sort per column, run arithmetic in uint64 (returned as Python
ints) -- and is what the GPU tests compare bit for bit, every word of `out`. brute is the O(R^2) definition in Python ints and
ap_fraction the exact rational average precision that tests/test_ranking_ref.py holds the restatement to; derived is the host's
float64 arithmetic (RankingResult's)."""
from fractions import Fraction

import numpy as np

F32 = np.float32
MAX_Q = 16
TWO32 = 1 << 32


def n_words(Q):
    return 6 + 2 * Q


def order32(score):
    """The order words of fp32 values: -0 as +0, then u ^ (u >> 31 ? 0xffffffff : 0x80000000). (NaNs map somewhere; the caller
    leaves them out.)"""
    u = np.ascontiguousarray(score, dtype=F32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def labels(score, target=None, target_class=None):
    """(positive, counted): R x D bool each, by the contract's two label rules."""
    s = np.asarray(score, dtype=F32)
    R, D = s.shape
    assert (target is None) != (target_class is None)
    if target is not None:
        t = np.asarray(target, dtype=F32)
        with np.errstate(invalid="ignore"):
            pos = t > F32(0.5)
        counted = ~np.isnan(s) & ~np.isnan(t)
    else:
        t = np.clip(np.asarray(target_class).astype(np.int64), 0, D - 1)
        pos = t[:, None] == np.arange(D)[None, :]
        counted = ~np.isnan(s)
    return pos, counted


def column_words(keys, pos, tauk):
    """One column's words from the order words (uint32) and labels of its counted elements; tauk: the thresholds' order words
    (None for a NaN threshold)."""
    order = np.argsort(keys, kind="stable")
    k, p = keys[order], pos[order]
    n = k.size
    n_pos, n_neg = int(p.sum()), int(n - p.sum())
    u2 = ap = 0
    if n:                                                    # per run of equal order words, in uint64: nothing passes 2^63 (header)
        assert n < 1 << 31
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]]).astype(np.uint64)
        ends = np.r_[starts[1:], np.uint64(n)]
        cp = np.r_[0, np.cumsum(p.astype(np.uint64))].astype(np.uint64)
        pb, pe = cp[starts.astype(np.int64)], cp[ends.astype(np.int64)]
        nb = starts - pb
        rp = pe - pb
        rn = (ends - starts) - rp
        u2 = int((rp * (np.uint64(2) * nb + rn)).sum(dtype=np.uint64))
        tp, fp = np.uint64(n_pos) - pb, np.uint64(n_neg) - nb                      # (tp + fp >= the run's own length)
        ap = int((rp * ((tp << np.uint64(32)) // (tp + fp))).sum(dtype=np.uint64))
    words = [n_pos, n_neg, 0, u2, ap, 0]
    for tk in tauk:
        ge = (k >= tk) if tk is not None else np.zeros(n, bool)
        words += [int((ge & p).sum()), int((ge & ~p).sum())]
    return words


def rank_metrics(score, target=None, target_class=None, tau=()):
    """vbnn_rank_metrics on NumPy arrays (pad columns already cut): score R x D fp32, target R x D fp32 or target_class R int32,
    tau the Q thresholds. Returns D lists of 6 + 2 Q Python ints."""
    s = np.ascontiguousarray(score, dtype=F32)
    R, D = s.shape
    assert len(tau) <= MAX_Q
    pos, counted = labels(s, target, target_class)
    keys = order32(s)
    tau32 = np.asarray(list(tau), dtype=F32)
    tauk = [None if np.isnan(t) else int(order32(np.array([t], F32))[0]) for t in tau32]
    out = []
    for j in range(D):
        c = counted[:, j]
        w = column_words(keys[c, j], pos[c, j], tauk)
        w[2] = int(R - c.sum())
        out.append(w)
    return out


def brute(score, pos, tau=()):
    """The definitions word for word on ONE column of counted elements (fp32 scores without NaN, bool labels), O(R^2), Python ints."""
    s = [F32(v) for v in score]
    P = [i for i in range(len(s)) if pos[i]]
    N = [i for i in range(len(s)) if not pos[i]]
    u2 = sum(2 * sum(1 for k in N if s[k] < s[i]) + sum(1 for k in N if s[k] == s[i]) for i in P)
    ap = 0
    for i in P:
        tp, fp = sum(1 for k in P if s[k] >= s[i]), sum(1 for k in N if s[k] >= s[i])
        ap += (tp * TWO32) // (tp + fp)
    words = [len(P), len(N), 0, u2, ap, 0]
    for t in tau:
        t = F32(t)
        words += [sum(1 for k in P if s[k] >= t), sum(1 for k in N if s[k] >= t)]
    return words


def ap_fraction(score, pos):
    """The exact average precision of one column: sum over the positives of TP / (TP + FP), over n_pos, as a Fraction."""
    s = np.asarray(score, dtype=F32)
    pos = np.asarray(pos, bool)
    tot = Fraction(0)
    for i in np.flatnonzero(pos):
        ge = s >= s[i]
        tot += Fraction(int((ge & pos).sum()), int(ge.sum()))
    return tot / int(pos.sum())


def derived(words, Q):
    """What the host derives from one column's integers, in float64: dict(auroc, average_precision, precision, recall, f1, tpr, fpr)."""
    n_pos, n_neg, u2, ap = words[0], words[1], words[3], words[4]
    nan = float("nan")
    d = dict(auroc=u2 / (2 * n_pos * n_neg) if n_pos and n_neg else nan,
             average_precision=ap / (TWO32 * n_pos) if n_pos else nan, precision=[], recall=[], f1=[], tpr=[], fpr=[])
    for q in range(Q):
        tp, fp = words[6 + 2 * q], words[7 + 2 * q]
        d["precision"].append(tp / (tp + fp) if tp + fp else nan)
        d["recall"].append(tp / n_pos if n_pos else nan)
        d["tpr"].append(tp / n_pos if n_pos else nan)
        d["fpr"].append(fp / n_neg if n_neg else nan)
        d["f1"].append(2 * tp / (2 * tp + fp + (n_pos - tp)) if n_pos + fp else nan)
    return d


# ------------------------------------------------------------------------------------------------ score patterns of the tests
SEVEN = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-42, 0.75, np.inf], F32)      # (1e-42 is a subnormal; -0 and +0 tie)


def scores(kind, R, D, seed=0):
    rng = np.random.default_rng([seed, R, D])
    if kind == "distinct":
        assert R * D < 1 << 24                               # (integers below 2^24 and their halves are exact: distinct)
        return (rng.permutation(R * D).reshape(R, D) - (R * D) // 2).astype(F32) * F32(0.5)
    if kind == "normal":
        return rng.standard_normal((R, D)).astype(F32)
    if kind == "seven":
        return SEVEN[rng.integers(0, 7, (R, D))]
    if kind == "equal":
        return np.full((R, D), 0.25, F32)
    if kind == "low_byte":                                   # order words that differ in their lowest byte alone
        return (np.uint32(0x3F000000) + rng.integers(0, 256, (R, D)).astype(np.uint32)).view(F32)
    if kind == "high_byte":                                  # ... in their highest byte alone (sign and bit 23 clear: no NaN)
        hi = rng.integers(0, 128, (R, D)).astype(np.uint32)
        return ((hi << np.uint32(24)) | np.uint32(0x00123456)).view(F32)
    if kind == "saturated":                                  # probabilities at exactly 1, at 1 - 2^-24 and a few below
        return np.array([1.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -30], F32)[rng.choice(4, (R, D), p=[0.6, 0.3, 0.05, 0.05])]
    raise ValueError(kind)


def targets01(R, D, seed=0, p=0.3):
    rng = np.random.default_rng([seed, R, D, 7])
    return (rng.random((R, D)) < p).astype(F32)
