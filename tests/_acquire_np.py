"""vbnn_top_rows (include/vbnn_hip.h) restated in NumPy -- test infrastructure, independent of the library: the order map,
vbnn_det_logf op for op, the stochastic key and the selection itself by np.lexsort on (row index, mapped key).

det_logf here IS include/vbnn_philox.h's vbnn_det_logf, one float32 operation per line (tests/test_acquire_ref.py holds it bit
for bit to the C oracle's). Its header comment states [2^-24, 1]; the stochastic key also evaluates it at E = -log u in
[2^-24, 17] and at scores over the whole positive normal range. Measured against float64 log (test_acquire_ref.py prints and
bounds it; the bound, 3 x 2^-24 + 1e-8 = 1.89e-7, is derived there from the roundings):
    u in [2^-24, 1):              1.47e-07 relative where |log x| >= 2^-6,  1.12e-09 absolute nearer 1
    E in [2^-24, 17]:             1.51e-07 relative,                         1.39e-09 absolute nearer 1
    scores over [2^-126, 2^128):  1.01e-07 relative,                         8.6e-10 absolute nearer 1
(near x = 1 the result goes to 0 and only an absolute figure means anything). The header's "~2e-8 before the final rounding"
is the series alone; the divide and the last fmaf round at full weight. The exponent never matters: e ln 2 is one fmaf away."""
import numpy as np

from tests._philox_np import philox4x32_10
from tests._update_np import fma_f32

F32 = np.float32
STREAM_ACQUIRE = 6
MAX_K = 4096
QNAN = 0x7FC00000


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def floats(b):
    return np.ascontiguousarray(np.asarray(b, np.uint32)).view(F32)


def order_map(b):
    """The monotone map of a float's bits: sign clear -> b ^ 0x80000000, sign set -> ~b."""
    b = np.asarray(b, np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def is_nan_bits(b):
    return (np.asarray(b, np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def det_logf(x):
    """vbnn_det_logf, op for op, on an array of positive normal float32."""
    b = bits(x).astype(np.int64)
    e = (b >> 23) - 127
    mb = (b & 0x007FFFFF) | 0x3F800000
    big = (mb > 0x3FB504F3).astype(np.int64)
    mb = mb - (big << 23)
    e = e + big
    m = floats(mb.astype(np.uint32))
    with np.errstate(all="ignore"):
        f = (m - F32(1.0)).astype(F32)
        den = (F32(2.0) + f).astype(F32)
        s = (f / den).astype(F32)
        z = (s * s).astype(F32)
        p = fma_f32(z, F32(0.111111111), F32(0.142857143))
        p = fma_f32(z, p, F32(0.2))
        p = fma_f32(z, p, F32(0.333333333))
        p = (z * p).astype(F32)
        s2 = (s + s).astype(F32)
        lm = fma_f32(s2, p, s2)
        return fma_f32(e.astype(F32), F32(0.693147181), lm)


def noise_words(R, seed, draw, row0):
    """x of the contract: word g & 3 of the Philox block of quad g >> 2, for g = row0 .. row0 + R - 1."""
    g = np.arange(R, dtype=np.uint64) + np.uint64(row0)
    w = philox4x32_10(g >> np.uint64(2), 0, draw, STREAM_ACQUIRE, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1)[np.arange(R), (g & np.uint64(3)).astype(np.int64)]


def race_key(score, R, beta, seed, draw, row0):
    """The stochastic key of every row (float32); a NaN score's key is whatever falls out: such a row is no candidate."""
    return race_key_of_words(noise_words(R, seed, draw, row0), score, beta)


def race_key_of_words(x, score, beta):
    """The key from the rows' Philox words x (uint32, R of them) -- steps 2 to 5 of the contract."""
    R = len(x)
    t = np.minimum((x >> np.uint32(8)).astype(np.uint32) + np.uint32(1), np.uint32(0x00FFFFFF))
    u = (t.astype(F32) * F32(2.0 ** -24)).astype(F32)
    E = (-det_logf(u)).astype(F32)
    if score is None:
        Lg = np.zeros(R, F32)
    else:
        sb = bits(score)
        normal = (sb >= np.uint32(0x00800000)) & (sb <= np.uint32(0x7F7FFFFF))
        Lg = np.full(R, -np.inf, F32)
        if normal.any():
            Lg[normal] = det_logf(floats(sb[normal]))
        Lg[sb == np.uint32(0x7F800000)] = np.inf
    with np.errstate(all="ignore"):
        return fma_f32(F32(beta), Lg, (-det_logf(E)).astype(F32))


def top_rows(score, k, largest=True, exclude=None, R=None, beta=None, seed=0, draw=0, row0=0):
    """(index int32[k], value bits uint32[k], key bits uint32[k], counts [4]) of the contract. score: float32 array or None."""
    R = len(score) if score is not None else int(R)
    sb = bits(score) if score is not None else None
    excl = np.zeros(R, bool) if exclude is None else (np.asarray(exclude) != 0)
    nan = np.zeros(R, bool) if sb is None else is_nan_bits(sb)
    cand = ~excl & ~nan
    if beta is None:
        kb = sb
    else:
        assert largest
        kb = bits(race_key(score, R, beta, seed, draw, row0))
    m = order_map(kb)
    rank = (~m if largest else m).astype(np.uint64)                   # ascending rank word: best first
    rows = np.nonzero(cand)[0]
    rows = rows[np.lexsort((rows, rank[rows]))][:k]
    n = len(rows)
    index = np.full(k, -1, np.int32)
    value = np.full(k, QNAN, np.uint32)
    key = np.full(k, QNAN, np.uint32)
    index[:n] = rows
    value[:n] = sb[rows] if sb is not None else bits(np.ones(n, F32))
    key[:n] = kb[rows]
    return index, value, key, [n, int(cand.sum()), int((nan & ~excl).sum()), int(excl.sum())]


def brute_top_rows(score, k, largest=True, exclude=None):
    """The deterministic selection by a plain Python sort on (float order, row), for the restatement to be held to: floats
    compared as numbers, the sign of a zero breaking the tie, NaN and excluded rows dropped."""
    import math
    rows = []
    for r, s in enumerate(np.asarray(score, F32).tolist()):
        if exclude is not None and exclude[r]:
            continue
        if math.isnan(s):
            continue
        zero_rank = math.copysign(1.0, s) if s == 0.0 else 0.0        # -0 below +0
        rows.append(((-s, -zero_rank) if largest else (s, zero_rank), r))
    rows.sort()
    return [r for _, r in rows[:k]]


# ------------------------------------------------------------------------------------------------ the adversarial inputs
NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA00000)


def population(name, R, seed=0):
    """The named input of R float32 scores (tests/test_acquire_ref.py and test_acquire_gpu.py share them)."""
    rs = np.random.RandomState(seed + 17)
    if name == "normal":
        return rs.randn(R).astype(F32)
    if name == "equal":
        return np.full(R, 0.75, F32)
    if name == "two_values":
        return np.where(rs.rand(R) < 0.5, F32(1.5), F32(-2.0)).astype(F32)
    if name == "small_ints":                                          # mass ties across workgroup boundaries
        return rs.randint(0, 16, R).astype(F32)
    if name == "ascending":
        return np.arange(R, dtype=np.float64).astype(F32) - F32(R // 3)
    if name == "descending":
        return (F32(R // 3) - np.arange(R, dtype=np.float64)).astype(F32)
    if name == "low_bits":                                            # differ in the last digit pass only
        return floats(np.uint32(0x3F800000) + rs.randint(0, 1 << 10, R).astype(np.uint32))
    if name == "top_bits":                                            # differ in the first digit pass only
        return floats(rs.randint(0, 1 << 11, R).astype(np.uint32) << np.uint32(21))  # (with a few NaN rows: exponent 255, a mantissa bit set)
    if name == "specials":
        pool = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                         0x3F800000, 0xBF800000, 0x00800000, 0x7F7FFFFF] + list(NAN_PATTERNS), np.uint32)
        return floats(pool[rs.randint(0, len(pool), R)])
    if name == "positive":                                            # weights for the stochastic cases
        return (rs.rand(R).astype(F32) + F32(0.01)).astype(F32)
    raise KeyError(name)


def exclusion(name, R, seed=0):
    rs = np.random.RandomState(seed + 29)
    if name == "none":
        return None
    if name == "half":
        return (rs.rand(R) < 0.5).astype(np.uint8) * np.uint8(3)      # any non-zero byte excludes
    if name == "all":
        return np.ones(R, np.uint8)
    if name == "all_but_one":
        e = np.ones(R, np.uint8)
        e[R // 2] = 0
        return e
    raise KeyError(name)
