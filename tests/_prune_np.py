"""NumPy reference of the pruning family -- prune.hip (vbnn_snr, vbnn_prune_select, vbnn_prune_pack), the compress half of
sparse.hip (vbnn_prune_compress) and units.hip (vbnn_unit_snr / _select / _index / _gather) -- restated from include/vbnn_hip.h.
NumPy only; nothing here reads GPU code or a GPU tensor. TEST INFRASTRUCTURE ONLY (tests/test_prune_ref.py holds it to brute
force on the CPU, tests/test_prune_forms_gpu.py holds the device to it).

WHAT IS BITWISE                                                         WHAT IS BOUNDED
  weight key  |m / sqrt(v)| in float32 from the device's own            against |m| exp(-l / 2) in float64: KEY_REL (below)
              v = expf(l): __fsqrt_rn and __fdiv_rn are correctly
              rounded, so NumPy's float32 sqrt and divide give the
              same bits (weight_key32)
  unit key    float32(sqrt(sum m^2) / sqrt(sum v)) in float64 from      against the float64 definition: UNIT_REL (below)
              the device's v, unless the quotient lies within
              unit_midpoint_distance of a rounding midpoint
  selection   the k-th smallest key bit pattern (np.partition)          --
  pack        mask = key < tau; shadows = where(mask, +0, prepared);    stats[1], stats[2]: the exact sum of the device's v,
              stats[0], stats[3]                                         within pack_sum_depth(...) 2^-53 relative
  compress    _sparse_np.csr_build on the same keys                     --
  unit lists  _units_np.kept                                            --

BOUNDS. u = U32 = 2^-24 (unit roundoff), ULP = 2^-23 (the largest relative size of one unit in the last place).
  KEY_REL. v = expf(l) lies within E_ULP ulp of the ROUNDED float64 exponential (what _sweeps_np.exp_ok holds every expf of the
      library to), so within E_ULP + 1 / 2 ulp of exp(l): relative e_v <= (E_ULP + 1 / 2) ULP. s = sqrt(v) halves that and rounds
      once: e_v / 2 + u. The divide rounds once more: |key - |m| exp(-l / 2)| <= (e_v / 2 + 2 u) |key| = (E_ULP / 2 + 5 / 4) ULP
      |key| -- 2.25 ULP with E_ULP = 2 -- times SLACK for the products of the terms, plus HALF_DENORMAL = 2^-150 where the quotient
      is subnormal (its rounding is then absolute). exp(l) itself must be a normal number (asserted by key_bound).
  UNIT_REL. Each term of sum v carries e_v, so the sum does (the terms are positive); its square root e_v / 2; sum m^2, both
      square roots and the quotient are double operations (2^-53 each, I additions per sum) and the result is rounded to float32
      once: e_v / 2 + u + (I + 3) 2^-52 = (E_ULP / 2 + 3 / 4) ULP + (I + 3) 2^-52, times SLACK.
  unit_midpoint_distance. The device and NumPy add the same doubles (m^2 is exact in double: 48 bits) in different orders: a
      sum of I positive terms is within (I - 1) 2^-53 relative of the exact sum in any order, so two orders differ by at most
      (I - 1) 2^-52 per sum, half of that after the square root, the two sums together (I - 1) 2^-52; the two square roots and the
      quotient round on either side: 6 x 2^-53 more. (I + 2) 2^-52 in all; the reference uses (I + 3) 2^-52 to cover the
      second-order terms. Only a float64 quotient that close to the midpoint of two neighbouring float32 values can round to
      either of them.
  pack_sum_depth. In a sum of non-negative doubles every term passes through d additions and the result is within
      d 2^-53 / (1 - d 2^-53) relative of the exact sum, d the largest such count. k_prune_pack: a thread adds
      4 ceil(quads / (256 nb)) terms one by one, quads = O ceil(I / 4), nb = the layer's workgroups; the wave's shuffle tree is 6
      additions, the four waves 3 more. k_prune_finish: a thread adds ceil(nb / 256) partials, then 6 + 3 again.
      Against sums of exp(lvars) instead of the device's v (pack_sum_rel) every term carries e_v as well.

KEY POPULATIONS (population). With lvars = 0 the key is |mean| bit for bit (expf(0) == 1, sqrt(1) == 1, m / 1 == m), so a
population is a list of 31-bit patterns; `means_of` gives every second one a sign for fabsf to clear. Each has a coverage
condition (coverage) that the tests assert on NumPy's keys and again on the keys the device returned.
  full     random 31-bit patterns: denormals, normals, NaNs with random payloads
  low10    1024 consecutive patterns that share their top 22 bits, second digit 2047 (the last bin of that digit), shuffled,
           some repeated
  lsb      two values one ulp apart, alternating
  edges    copies of 0, the smallest and largest denormal, the smallest normal, 1.0, the largest finite, inf and the NaNs
           0x7fc00000, 0x7fe00000, 0x7fffffff: first-digit bins 0, 1020 (inf) and 1023 (the last) are occupied
  but_low / but_high   all equal but one smaller / one larger

DEVICE FINDINGS (MI355X, recorded by tests/test_prune_forms_gpu.py in profiles/prune_bounds.txt): see DEVICE_FINDINGS. The first
run of test_snr found one key in seven an ulp above weight_key32: __fsqrt_rn is the hardware's approximate root in this toolchain.
vbnn_snr_key (csrc/common.h) now calls sqrtf, which hipcc rounds correctly, and the restatement holds bit for bit."""
import math

import numpy as np

from tests import _units_np as U
from tests._head_np import E_ULP, U32, ULP
from tests._sparse_np import csr_build  # noqa: F401  (the compress reference, re-exported)
from tests._update_np import bf16_bits, exp32, exp_shifted, step_ulps  # noqa: F401

F = np.float32
f8 = np.float64
SLACK = 1.0 + 2.0 ** -10
HALF_DENORMAL = 2.0 ** -150
E_V = (E_ULP + 0.5) * ULP                                                 # relative error of the device's expf
KEY_REL = (E_V / 2 + 2 * U32) * SLACK                                     # the weight key against float64 (2.25 ulp)
INF_BITS = 0x7f800000

# what the MI355X does with the inputs IEEE 754 leaves open, as tests/test_prune_forms_gpu.py::test_key_edges found it:
# the key of a denormal mean at lvar = 0 is the denormal itself (no flush), and a quiet NaN keeps its payload through the
# divide (fabsf clears the sign; a signalling NaN comes out quiet with the rest of its payload, as on the host). The selection
# tests do not depend on either: they select on the keys the device returned.
DEVICE_FINDINGS = dict(denormal_keys_kept=True, nan_payload_kept=True)

# largest fraction of KEY_REL / UNIT_REL the float32 restatement with a correctly rounded exp uses over the inputs of
# test_prune_ref.py::test_restatements_stay_inside_their_bounds (which fails when a record is below the measurement or more
# than twice above it)
BOUND_USED = {"weight_key": 0.51, "unit_key": 0.32}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ keys
def weight_key32(m, v):
    """The device's key from its own v = expf(l): one float32 sqrt, one float32 divide, fabs. Bit for bit."""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(m, F) / np.sqrt(np.asarray(v, F)))


def weight_key64(m, l):
    return np.abs(np.asarray(m, F).astype(f8)) * np.exp(-np.asarray(l, F).astype(f8) / 2)


def key_bound(m, l):
    """|device key - weight_key64| allowed, element-wise."""
    ex = np.exp(np.asarray(l, F).astype(f8))
    assert (ex >= 2.0 ** -126).all() and (ex < 2.0 ** 127).all(), "the bound is derived for a normal exp(l)"
    return KEY_REL * weight_key64(m, l) + HALF_DENORMAL


def unit_rel(I):
    return (E_V / 2 + U32 + (I + 3) * 2.0 ** -52) * SLACK


def unit_midpoint_distance(I):
    return (I + 3) * 2.0 ** -52


def unit_key_value(m, v):
    """(key as float32, the float32 neighbour on the other side of the nearest midpoint, close): the unit key from the
    device's v in float64, and where the float64 quotient lies within unit_midpoint_distance of a rounding midpoint."""
    m, v = np.asarray(m, F).astype(f8), np.asarray(v, F).astype(f8)
    I = m.shape[1]
    with np.errstate(all="ignore"):
        q = np.sqrt((m * m).sum(1)) / np.sqrt(v.sum(1))
    k = q.astype(F)
    k = np.where(np.isnan(k), U.NAN_BITS.view(F), k).astype(F)
    with np.errstate(all="ignore"):
        other = np.where(k.astype(f8) <= q, np.nextafter(k, F(np.inf)), np.nextafter(k, F(-np.inf))).astype(F)
        mid = (k.astype(f8) + other.astype(f8)) / 2
        close = np.abs(q - mid) <= unit_midpoint_distance(I) * np.abs(q)
    close &= np.isfinite(q) & (q > 0)
    return k, other, close


# ------------------------------------------------------------------------------------------------ the order statistic
def kth_bits(bits, k):
    """The k-th smallest (0-based) key bit pattern: non-negative floats order as their bits, NaNs (payloads and all) above inf."""
    b = u32(bits).ravel()
    assert 0 <= k < b.size and not (b >> 31).any()
    return np.partition(b, k)[k]


def digit_walk(bits, k, widths):
    """The radix select restated: per digit (most significant first) a histogram of the keys that match the prefix chosen so
    far, a walk to the bin that holds the remaining rank, the longer prefix and the rank inside the bin. widths = (11, 11, 10)
    for vbnn_prune_select, (8, 8, 8, 8) for units.hip's unit_kth."""
    b = u32(bits).ravel()
    assert sum(widths) == 32 and 0 <= k < b.size
    prefix, mask, rank, shift = 0, 0, int(k), 32
    for w in widths:
        shift -= w
        sel = b[(b & np.uint32(mask)) == np.uint32(prefix)]
        hist = np.bincount(((sel >> np.uint32(shift)) & np.uint32((1 << w) - 1)).astype(np.int64), minlength=1 << w)
        before = np.cumsum(hist) - hist
        j = int(np.flatnonzero((before <= rank) & (rank - before < hist))[0])      # exactly one bin
        rank -= int(before[j])
        prefix |= j << shift
        mask |= ((1 << w) - 1) << shift
    return np.uint32(prefix)


WEIGHT_DIGITS = (11, 11, 10)
UNIT_DIGITS = (8, 8, 8, 8)


# ------------------------------------------------------------------------------------------------ vbnn_prune_pack
def pack_ref(keys, tau, mu_prep, var_prep):
    """(mask O x I bool, mu_p, var_p): pruned = key < tau (false for a NaN key and under a NaN tau); a pruned weight's shadows
    are +0 (all bits clear), a kept weight's what vbnn_prep_layer stored (any dtype: bit patterns are copied)."""
    with np.errstate(invalid="ignore"):
        mask = np.asarray(keys, F) < F(tau)
    zero = np.zeros((), mu_prep.dtype)
    return mask, np.where(mask, zero, mu_prep), np.where(mask, zero, var_prep)


def prune_grid(W):
    return int(min(max((W + 4095) // 4096, 1), 1024))


def pack_sum_depth(O, I):
    quads, nb = O * ((I + 3) // 4), prune_grid(O * I)
    return 4 * -(-quads // (256 * nb)) + 9 + -(-nb // 256) + 9


def pack_sum_rel(O, I):
    """stats[1], stats[2] against a NumPy float64 sum of exp(lvars): every term within E_V of its exponential, the device's
    additions (pack_sum_depth) and 64 more for NumPy's own pairwise sum (blocks of 128 in 8 partial sums, then a tree)."""
    return (E_V + (pack_sum_depth(O, I) + 64) * 2.0 ** -53) * SLACK


def pack_stats(mask, v):
    """stats[0 .. 3] with the two sums exact (math.fsum of the device's float32 v), and the relative bound of the sums."""
    v = np.asarray(v, F).astype(f8)
    O, I = mask.shape
    d = pack_sum_depth(O, I) * 2.0 ** -53
    return [float(mask.sum()), math.fsum(v[mask].tolist()), math.fsum(v.ravel().tolist()), float(mask.size)], d / (1 - d)


# ------------------------------------------------------------------------------------------------ key populations
POPULATIONS = ("full", "low10", "lsb", "edges", "but_low", "but_high")
LOW10_BASE = 0x3f9ffc00                        # first digit 508, second digit 2047, third digit 0
EDGES = np.array([0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x7fe00000,
                  0x7fffffff], np.uint32)


def population(name, W, seed=0):
    """W key bit patterns (uint32, sign clear)."""
    rng = np.random.default_rng(1000 + seed)
    if name == "full":
        b = rng.integers(0, 1 << 31, W, dtype=np.int64)
    elif name == "low10":
        assert W >= 1024
        b = LOW10_BASE + np.concatenate([np.arange(1024), rng.integers(0, 1024, W - 1024)])
        rng.shuffle(b)
    elif name == "lsb":
        b = 0x40490fda + (np.arange(W) & 1)
    elif name == "edges":
        b = EDGES[np.arange(W) % EDGES.size].astype(np.int64)
        rng.shuffle(b)
    elif name in ("but_low", "but_high"):
        b = np.full(W, 0x3e99999a, np.int64)
        if W > 1:
            b[int(rng.integers(0, W))] += -1 if name == "but_low" else 1
    else:
        raise KeyError(name)
    return b.astype(np.uint32)


def means_of(bits):
    """float32 means whose key at lvar = 0 is `bits`: the pattern itself, every second one negative."""
    b = u32(bits).copy()
    b[1::2] |= np.uint32(1 << 31)
    return b.view(F)


def coverage(name, bits):
    """The names of the coverage conditions population `name` does NOT meet on the key patterns `bits` (empty = covered)."""
    b = u32(bits).ravel()
    d1, d3 = b >> np.uint32(21), b & np.uint32(1023)
    miss = []

    def need(cond, what):
        if not cond:
            miss.append(what)
    need(not (b >> 31).any(), "sign bits clear")
    if name == "full" and b.size >= 1000:
        need(np.unique(d1).size >= 400, "400 first-digit bins")
        need((b < 0x00800000).any(), "a denormal")
        need((b > INF_BITS).any(), "a NaN")
        need(np.unique(b[b > INF_BITS]).size >= 2, "NaN payloads differ")
    if name == "low10":
        need(np.unique(b >> np.uint32(10)).size == 1, "one 22-bit prefix")
        need(np.unique(d3).size == 1024, "every value of the last digit")
        need(((b >> np.uint32(10)) & np.uint32(2047) == 2047).all(), "second digit 2047")
    if name == "lsb" and b.size >= 2:
        v = np.unique(b)
        need(v.size == 2 and v[1] - v[0] == 1, "two values one ulp apart")
    if name == "edges" and b.size >= EDGES.size:
        for j in (0, 1020, 1023):
            need((d1 == j).any(), f"first-digit bin {j}")
        need((b == 0).any() and (b == INF_BITS).any(), "zero and inf")
        need(np.unique(b[b > INF_BITS]).size >= 2, "two NaN patterns")
    if name in ("but_low", "but_high") and b.size >= 2:
        v, c = np.unique(b, return_counts=True)
        need(v.size == 2 and c[0 if name == "but_low" else 1] == 1, "all equal but one")
    return miss


# ------------------------------------------------------------------------------------------------ unit lists
def run_length(O):
    """k_unit_index: the units one of the 16 waves owns, whole 64s."""
    return -(-(-(-O // 16)) // 64) * 64


def tie_keys(O, n_high, seed=0):
    """O two-valued keys (0.25 / 0.5), n_high of them 0.5 at random places."""
    k = np.full(O, 0.25, F)
    k[np.random.default_rng(77 + seed).permutation(O)[:n_high]] = 0.5
    return k


def gather_ref(src, rows, cols, O, I):
    """vbnn_unit_gather of one array: index words clamped to the source shape, NULL lists = every row / column."""
    r = np.arange(O) if rows is None else np.minimum(np.asarray(rows, np.uint32), np.uint32(O - 1)).astype(np.int64)
    c = np.arange(I) if cols is None else np.minimum(np.asarray(cols, np.uint32), np.uint32(I - 1)).astype(np.int64)
    src = np.asarray(src)
    return src[r] if src.ndim == 1 else src[r][:, c]
