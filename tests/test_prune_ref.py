"""CPU tests of tests/_prune_np.py, the reference tests/test_prune_forms_gpu.py holds the pruning kernels to: both digit walks
against np.partition at every k on every key population, the float32 key restatements inside their derived float64 bounds (with
the fraction of each bound they use on record), the populations' coverage conditions, and _units_np.kept against a brute-force
sort at the tie cuts the GPU file uses."""
import numpy as np
import pytest

from tests import _prune_np as P
from tests import _units_np as U

F, f8 = np.float32, np.float64
W_SMALL = 1100


def _params(W, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(W).astype(F)
    l = (F(np.log(1e-2)) + F(0.75) * rng.standard_normal(W).astype(F)).astype(F)
    return m, l


@pytest.mark.parametrize("name", P.POPULATIONS)
def test_populations_meet_their_coverage_conditions(name):
    for W in (W_SMALL, 4096 * 1025 + 3):
        b = P.population(name, W)
        assert b.dtype == np.uint32 and b.size == W and P.coverage(name, b) == [], (name, W, P.coverage(name, b))
        m = P.means_of(b)
        with np.errstate(invalid="ignore"):
            key = P.weight_key32(m, np.ones(W, F))                     # lvars = 0: the key is |mean| bit for bit
        snan = (b > P.INF_BITS) & (b & 0x00400000 == 0)                 # a signalling NaN leaves an operation quiet: bit 22 set
        assert np.array_equal(P.u32(key), np.where(snan, b | 0x00400000, b)) and (P.u32(m)[1::2] >> 31).all()
        assert snan.any() == (name == "full")
    assert P.coverage("edges", P.population("low10", W_SMALL)) != []      # (the conditions can fail)
    assert P.coverage("low10", P.population("full", W_SMALL)) != []


@pytest.mark.parametrize("name", P.POPULATIONS)
def test_digit_walks_equal_partition_at_every_k(name):
    for W in (1, 2, 3, 255, W_SMALL):
        if name == "low10" and W < 1024:
            continue
        b = P.population(name, W)
        s = np.sort(b)
        c = U.code(b.view(F))                                           # the units' order: every NaN is 0x7fc00000
        sc = np.sort(c)
        for k in range(W):
            assert P.digit_walk(b, k, P.WEIGHT_DIGITS) == s[k] == P.kth_bits(b, k), (name, W, k)
            assert P.digit_walk(c, k, P.UNIT_DIGITS) == sc[k] == P.u32(U.kth(b.view(F), k)), (name, W, k)


def test_digit_walks_on_the_large_population():
    W = 4096 * 1025 + 3
    b = P.population("full", W)
    s = np.sort(b)
    for k in (0, 1, W // 1000, W // 2, W - 2, W - 1):
        assert P.digit_walk(b, k, P.WEIGHT_DIGITS) == s[k]


def test_restatements_stay_inside_their_bounds():
    used = {}
    m, l = _params(200000, 5)
    l[:8] = [-80.0, -40.0, 0.0, 40.0, 80.0, -87.0, 87.0, 1.0]
    m[:4] = [0.0, 1e-30, -3e30, 1e-38]
    k64, bound = P.weight_key64(m, l), P.key_bound(m, l)
    worst = 0.0
    for e in range(-P.E_ULP, P.E_ULP + 1):                              # an expf anywhere in its allowance
        k32 = P.weight_key32(m, P.exp_shifted(e)(l)).astype(f8)
        fin = np.isfinite(k32)
        assert fin.sum() >= m.size - 4
        frac = (np.abs(k32 - k64)[fin] / bound[fin]).max()
        assert frac <= 1.0, (e, frac)
        worst = max(worst, frac) if e == 0 else worst
    used["weight_key"] = worst
    worst = 0.0
    for O, I in ((5, 3), (1030, 7), (4, 1025), (3, 2049), (64, 1)):
        m, l = _params(O * I, 100 + I)
        m, l = m.reshape(O, I), l.reshape(O, I)
        want = U.unit_key64(m, l)
        for e in range(-P.E_ULP, P.E_ULP + 1):
            k, other, close = P.unit_key_value(m, P.exp_shifted(e)(l))
            frac = (np.abs(k.astype(f8) - want) / (P.unit_rel(I) * want)).max()
            assert frac <= 1.0 and not close.any(), (O, I, e, frac)
            worst = max(worst, frac) if e == 0 else worst
    used["unit_key"] = worst
    print("fraction of the bounds used:", used)
    for name, frac in used.items():
        assert frac <= P.BOUND_USED[name] <= 2 * frac, (name, frac, P.BOUND_USED[name])


def test_unit_midpoint_rule_flags_a_midpoint():
    """sqrt(1 + b^2) with b^2 ~ 2^-23 is 1 + 2^-24 to about 2e-15: the midpoint of 1 and its successor. Among 100000 terms that is
    within the reordering distance; among two terms it is not."""
    b = F(2.0 ** -11.5)
    for I, want in ((100000, True), (2, False)):
        m, v = np.zeros((2, I), F), np.zeros((2, I), F)
        m[:, 0], m[0, 1], v[:, 0] = 1.0, b, 1.0
        k, other, close = P.unit_key_value(m, v)
        assert close.tolist() == [want, False] and k[1] == 1.0
        assert {float(k[0]), float(other[0])} == {1.0, float(np.nextafter(F(1), F(2)))}


def test_pack_reference():
    keys = np.array([[0.5, np.nan, 0.25], [0.25, np.inf, 0.0]], F)
    mu = np.arange(1, 7, dtype=np.uint16).reshape(2, 3)
    var = np.arange(11, 17, dtype=np.uint16).reshape(2, 3)
    for tau, pruned in ((0.0, 0), (0.25, 1), (0.5, 3), (np.inf, 4), (np.nan, 0)):
        mask, a, b = P.pack_ref(keys, tau, mu, var)
        assert mask.sum() == pruned and not mask[0, 1] and a.dtype == np.uint16
        assert np.array_equal(a[~mask], mu[~mask]) and not a[mask].any() and not b[mask].any()
    v = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]], F)
    st, rel = P.pack_stats(keys < F(0.5), v)
    assert st == [3.0, 4.0 + 8.0 + 32.0, 63.0, 6.0] and 0 < rel < 1e-13
    assert P.pack_sum_depth(1, 1) == 4 + 9 + 1 + 9 and P.prune_grid(4096 * 1025 + 3) == 1024 and P.prune_grid(1030 * 1030) == 260
    assert P.pack_sum_depth(1, 4096 * 1025 + 3) == 4 * 5 + 9 + 4 + 9


def _kept_brute(keys, tau, m):
    keys = np.asarray(keys, F)
    O = keys.size
    n0 = sum(1 for x in keys if not (x < F(tau)))
    n = min(O, m * -(-max(n0, 1) // m))
    order = sorted(range(O), key=lambda i: (-(0x7fc00000 if np.isnan(keys[i]) else int(keys[i:i + 1].view(np.uint32)[0])), i))
    return np.array(sorted(order[:n]), np.uint32)


@pytest.mark.parametrize("O", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 5000])
def test_kept_equals_brute_force_at_the_tie_cuts(O):
    per = P.run_length(O)
    assert per % 64 == 0 and 16 * per >= O and (per == 64 or 16 * (per - 64) < O)
    for t in (1, 63, 64, 65, per, per + 1):
        if t > O:
            continue
        eq = np.full(O, 0.25, F)                                          # all equal, tau = +inf: the first `multiple` units
        with np.errstate(invalid="ignore"):
            assert np.array_equal(U.kept(eq, np.inf, t), np.arange(t)) and np.array_equal(_kept_brute(eq, np.inf, t), np.arange(t))
        H = (O - t) // 2
        if H >= 1:
            two = P.tie_keys(O, H, seed=t)                                # tau = 0.5, multiple = H + t: every 0.5 and t ties
            got = U.kept(two, 0.5, H + t)
            assert got.size == H + t and np.array_equal(got, _kept_brute(two, 0.5, H + t))
            assert (two[got] == 0.25).sum() == t
    keys = P.population("full", O, seed=3).view(F).copy()
    keys[:: max(O // 7, 1)] = np.array([0x7fc00001], np.uint32).view(F)[0]
    for tau in (np.nan, 0.0, np.inf, float(np.nan_to_num(keys[O // 2], nan=1.0))):
        for m in (1, 4, 256, O + 1):
            with np.errstate(invalid="ignore"):
                assert np.array_equal(U.kept(keys, tau, m), _kept_brute(keys, tau, m)), (O, tau, m)
