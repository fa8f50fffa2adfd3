"""NumPy restatements for the tests of vbnn_predict_calibration and vbnn_selective (include/vbnn_hip.h,
vbnn_amd/csrc/calibration.hip): calibration32 / selective32 restate the two calls in fp32 and integers, operation for operation --
the row sum of squares in the family's order, the fixed-point adds in uint64, the key transform, selection by np.sort on the keys
-- and are what the GPU tests compare bit for bit. calibration64 is the float64 definition of ECE, MCE and the Brier score they
are held to on the CPU.

The DERIVED bound of the fp32 Brier score of a row against float64 (brier_bound), eps = 2^-24, for probabilities in [0, 1]:
  ss = sum_c p[c]^2: a term passes through 1 rounding (its square) and then at most n_add additions -- 4 per quad the row's thread
    owns (per = ceil(ceil(C / 4) / T) quads, T = 64 for C <= 256 and 256 above), 6 butterfly levels, 3 more for the four waves of
    a T = 256 row -- so |ss32 - ss| <= gamma ss with gamma = n eps / (1 - n eps), n = 1 + 4 per + 6 + 3 (all terms are >= 0: no
    cancellation, the bound is relative to ss itself);
  2 p[t] is exact; d = fl(ss32 - 2 p[t]) adds eps |d|; b = fl(d + 1) adds eps |b|; the final max with 0 moves b towards the true
    value (which is >= 0) or not at all. Three roundings beside the sum:
  |brier32 - brier| <= (gamma ss + eps |ss - 2 p[t]| + eps |brier|) (1 + 2^-20)     (the factor: the second-order terms).
The fixed-point conversion (uint64)(x 2^32) truncates less than 2^-32 per row (nothing for conf >= 2^-9, where x 2^32 is an
integer). tests/test_calibration_ref.py re-measures the share of the bound the restatement uses and prints it."""
import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
TWO32 = F32(4294967296.0)
MAX_BINS, MAX_Q = 64, 32
QNAN_BITS = 0x7FC00000


def softmax_case(R, C, seed=5, scale=2.0):
    """probs (R x C fp32, softmax of fp32 normals), pred (argmax), target (half the rows right)."""
    rng = np.random.default_rng(seed)
    y = (scale * rng.standard_normal((R, C))).astype(F32)
    e = np.exp(y - y.max(1, keepdims=True)).astype(F32)
    probs = (e / e.sum(1, keepdims=True, dtype=F32)).astype(F32)
    pred = probs.argmax(1).astype(np.int32)
    target = np.where(rng.random(R) < 0.5, pred, rng.integers(0, C, R)).astype(np.int32)
    return probs, pred, target


def threads_per_row(C):
    return 64 if C <= 256 else 256


def row_sumsq32(P):
    """sum_c P[r, c]^2 in fp32 in the family's order (R x C fp32 in, R fp32 out): thread i of T adds to +0, in ascending order,
    the columns of its quads i, i + T, ...; the xor butterfly 32 .. 1 inside a wave; the waves in wave order."""
    P = np.ascontiguousarray(P, dtype=F32)
    R, C = P.shape
    T = threads_per_row(C)
    per = -(-((C + 3) // 4) // T)
    X = np.zeros((R, per * T * 4), F32)                      # (a column past C adds +0: no bit of a sum of squares changes)
    X[:, :C] = P
    X = X.reshape(R, per, T, 4)
    v = np.zeros((R, T), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(per):
            for j in range(4):
                v = v + X[:, k, :, j] * X[:, k, :, j]        # fp32 product, fp32 sum
        v = v.reshape(R, T // 64, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lanes ^ off]
        w = v[:, :, 0]
        return w[:, 0] if T == 64 else ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def n_words(M):
    return 3 * M + 4


def calibration32(probs, pred, target, M, acc=None):
    """vbnn_predict_calibration on NumPy arrays: probs (R x C fp32; pad columns already cut), pred / target (R int32), M bins.
    Returns dict(conf, hit, brier, bin: the row outputs; acc: uint64[3 M + 4], `acc` + this call's adds -- a fresh zero without)."""
    assert 1 <= M <= MAX_BINS
    probs = np.ascontiguousarray(probs, dtype=F32)
    R, C = probs.shape
    rows = np.arange(R)
    p = np.clip(pred.astype(np.int64), 0, C - 1)
    t = np.clip(target.astype(np.int64), 0, C - 1)
    conf, pt = probs[rows, p], probs[rows, t]
    ss = row_sumsq32(probs)
    nan = np.isnan(conf) | np.isnan(ss)
    hit = (p == t).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        brier = np.maximum((ss - F32(2) * pt) + F32(1), F32(0)).astype(F32)
        x = np.minimum(np.maximum(conf * F32(M), F32(0)), F32(M - 1))
    b = np.where(nan, 0, np.nan_to_num(x)).astype(np.int32)
    out = np.zeros(n_words(M), np.uint64) if acc is None else acc.astype(np.uint64).copy()
    ok = ~nan
    with np.errstate(invalid="ignore", over="ignore"):
        cfix = (np.maximum(conf[ok], F32(0)) * TWO32).astype(np.uint64)
        bfix = (brier[ok] * TWO32).astype(np.uint64)
    np.add.at(out, b[ok], np.uint64(1))
    np.add.at(out, M + b[ok], hit[ok].astype(np.uint64))
    np.add.at(out, 2 * M + b[ok], cfix)
    out[3 * M] += bfix.sum(dtype=np.uint64)
    out[3 * M + 1] += np.uint64(ok.sum())
    out[3 * M + 2] += np.uint64(nan.sum())
    qn = F32(np.nan)
    return dict(conf=np.where(nan, qn, conf).astype(F32), hit=np.where(nan, -1, hit).astype(np.int32),
                brier=np.where(nan, qn, brier).astype(F32), bin=np.where(nan, -1, b).astype(np.int32), acc=out)


def derived(acc, M):
    """What the host derives from the integers, in float64 (CalibrationResult's arithmetic): dict(count, hits, confidence_sum,
    ece, mce, brier, accuracy, n, n_nan, bin_accuracy, bin_confidence)."""
    acc = [int(v) for v in acc]
    count, hits = np.array(acc[:M], np.float64), np.array(acc[M:2 * M], np.float64)
    csum = np.array([v / 4294967296.0 for v in acc[2 * M:3 * M]], np.float64)
    n, n_nan = acc[3 * M + 1], acc[3 * M + 2]
    gap = np.abs(hits - csum)
    nz = count > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        bin_acc, bin_conf = np.where(nz, hits / count, np.nan), np.where(nz, csum / count, np.nan)
        mce = float(np.max(np.where(nz, gap / count, 0.0))) if n else float("nan")
    return dict(count=count, hits=hits, confidence_sum=csum, ece=float(gap.sum() / n) if n else float("nan"), mce=mce,
                brier=acc[3 * M] / 4294967296.0 / n if n else float("nan"), accuracy=float(hits.sum() / n) if n else float("nan"),
                n=n, n_nan=n_nan, bin_accuracy=bin_acc, bin_confidence=bin_conf)


def calibration64(probs, pred, target, M):
    """The float64 definition on the same fp32 probabilities: per bin the exact (float64) sums, ECE, MCE, and per row the Brier
    score sum_c (p[c] - [c == t])^2. The bins are the contract's -- min(int(fl32(conf M)), M - 1), the fp32 product -- since the
    edges are part of the definition; rows with a NaN confidence or a NaN in the row are left out, as the call leaves them out."""
    P = probs.astype(np.float64)
    R, C = P.shape
    rows = np.arange(R)
    p = np.clip(pred.astype(np.int64), 0, C - 1)
    t = np.clip(target.astype(np.int64), 0, C - 1)
    ok = ~np.isnan(P).any(1)
    conf = P[rows, p]
    with np.errstate(invalid="ignore"):
        b = np.minimum(np.nan_to_num(probs[rows, p].astype(F32) * F32(M)).astype(np.int64), M - 1)
    onehot = np.zeros_like(P)
    onehot[rows, t] = 1.0
    brier = ((P - onehot) ** 2).sum(1)
    count, hits, csum = np.zeros(M), np.zeros(M), np.zeros(M)
    np.add.at(count, b[ok], 1.0)
    np.add.at(hits, b[ok], (p == t)[ok].astype(np.float64))
    np.add.at(csum, b[ok], conf[ok])
    n = int(ok.sum())
    gap = np.abs(hits - csum)
    return dict(count=count, hits=hits, confidence_sum=csum, ece=gap.sum() / n, mce=np.max(np.where(count > 0, gap / np.maximum(count, 1), 0.0)),
                brier_rows=brier, brier=brier[ok].sum() / n, ss=(P * P).sum(1), pt=P[rows, t], ok=ok, n=n)


def brier_bound(C, ss, pt, brier):
    """The module docstring's bound of a row's fp32 Brier score against float64 (arrays of the float64 ss, p[t], brier)."""
    T = threads_per_row(C)
    per = -(-((C + 3) // 4) // T)
    n = 1 + 4 * per + 6 + 3
    gamma = n * EPS / (1.0 - n * EPS)
    return (gamma * ss + EPS * np.abs(ss - 2.0 * pt) + EPS * np.abs(brier)) * (1.0 + 2.0 ** -20)


# ------------------------------------------------------------------------------------------------ selective prediction
def keys32(score):
    """The ordered keys of fp32 scores: u ^ (u >> 31 ? 0xffffffff : 0x80000000), every NaN first made the positive quiet NaN."""
    s = np.ascontiguousarray(score, dtype=F32)
    u = s.view(np.uint32).copy()
    u[np.isnan(s)] = QNAN_BITS
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def unkey32(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def selective32(score, hit, ks):
    """vbnn_selective on NumPy arrays: score (R fp32), hit (R int32), ks (Q ranks, 1-based). Returns (tau: Q fp32, counts: Q x 4
    uint64 = n_below, hits_below, n_tied, hits_tied)."""
    assert 1 <= len(ks) <= MAX_Q
    keys = keys32(score)
    h = np.asarray(hit) != 0
    srt = np.sort(keys)
    tau, counts = [], []
    for k in ks:
        assert 1 <= k <= keys.size
        tk = srt[k - 1]
        below, tied = keys < tk, keys == tk
        tau.append(tk)
        counts.append([below.sum(), (below & h).sum(), tied.sum(), (tied & h).sum()])
    return unkey32(np.array(tau, np.uint32)), np.array(counts, np.uint64).reshape(len(ks), 4)


def selective_accuracy(counts, ks):
    """acc@k = (hits_below + (k - n_below) hits_tied / n_tied) / k in float64: the expectation over a random tie-break."""
    return [(int(c[1]) + (k - int(c[0])) * int(c[3]) / int(c[2])) / k for c, k in zip(counts, ks)]


def ranks(coverages, R):
    """k = max(1, ceil(c R)), as FusedMLP.selective computes it."""
    import math
    return [max(1, min(R, math.ceil(c * R))) for c in coverages]
