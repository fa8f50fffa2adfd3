"""CPU tests of tests/_kcentre_np.py, the fp32 restatement the GPU tests hold vbnn_kcentre to, against a plain float64 greedy.

THE BOUND on a distance (random features; derived, not measured). The fp32 route rounds, per column, t = fl(a - b) =
(a - b)(1 + e1) and p = fl(t t) = (a - b)^2 (1 + e1)^2 (1 + e2) with |e| <= u = 2^-24 -- no multiply-add is fused, as the
header states -- so every term is within 3u + O(u^2) of its exact value. All terms are >= 0, so the summation's error is at
most (the number of additions a term passes through) u relative to the exact sum: L = 4 ceil(ceil(D / 4) / T) in the thread,
6 in the butterfly, 3 across the waves when T = 256. Hence |d32 - d| <= d g(L + 3), g(n) = n u / (1 - n u); the float64 reference's
own error (D 2^-53 relative, on exactly representable inputs) is five orders below. A weighted key adds one multiplication:
g(L + 4). The minimum over centres is exact, so it inherits the bound, PROVIDED both routes picked the same rows -- which holds
whenever at every step the float64 gap between the best and the second-best key exceeds the two keys' bounds together; the
tests assert that of their inputs before they compare a single pick."""
import numpy as np
import pytest

from . import _kcentre_np as K

U = 2.0 ** -24


def _levels(D):
    T = K.threads(D)
    return 4 * -(-((D + 3) // 4) // T) + 6 + (3 if T == 256 else 0)


def _g(n):
    return n * U / (1 - n * U)


def _ints(rng, R, D, amp):
    return rng.integers(-amp, amp + 1, size=(R, D)).astype(np.float32)


EXACT = [  # R, D, amp, k, weighted, n_centres, seed -- |f| <= amp: every sum is an integer below 2^24, exact in fp32
    (40, 1, 64, 40, False, 0, 1), (37, 3, 64, 10, True, 2, 2), (50, 5, 64, 50, False, 1, 3), (64, 64, 64, 20, True, 0, 4),
    (33, 255, 64, 12, False, 3, 5), (20, 257, 64, 20, True, 1, 6), (12, 1024, 64, 12, False, 0, 7), (9, 4096, 16, 9, True, 2, 8),
]


@pytest.mark.parametrize("R,D,amp,k,weighted,nc,seed", EXACT)
def test_exact_on_integer_features(R, D, amp, k, weighted, nc, seed):
    rng = np.random.default_rng(seed)
    F = _ints(rng, R, D, amp)
    F[R // 2] = F[0]                                                # duplicate rows: exact ties
    F[R - 1] = F[1]
    w = rng.integers(0, 4, size=R).astype(np.float32) if weighted else None      # zero weights among them
    ex = (rng.random(R) < 0.2).astype(np.uint8)
    cen = list(rng.integers(0, R, size=nc))
    got = K.kcentre(F, k, w, ex, cen)
    idx, key, dist, m, _ = K.greedy64(F, k, w, ex, cen)
    n = len(idx)
    assert got["counts"][0] == n == min(k, int((ex == 0).sum()))
    assert np.array_equal(got["index"][:n], idx) and np.all(got["index"][n:] == -1)
    assert np.array_equal(got["key"][:n].astype(np.float64), key) and np.array_equal(got["dist"][:n].astype(np.float64), dist)
    assert np.all(np.isnan(got["key"][n:])) and np.all(np.isnan(got["dist"][n:]))
    assert np.array_equal(got["min_dist"].astype(np.float64), m)
    assert float(m.max()) < 2.0 ** 24                               # the premise: nothing left the exact integers


def test_all_equal_rows_and_zero_weights():
    F = np.full((10, 7), 3.0, dtype=np.float32)
    got = K.kcentre(F, 4)
    assert list(got["index"]) == [0, 1, 2, 3]                       # +inf, then three exact zeros: the lower row each time
    assert np.isinf(got["key"][0]) and np.all(got["key"][1:] == 0) and np.all(got["min_dist"] == 0)
    got = K.kcentre(F, 3, weight=np.zeros(10, dtype=np.float32))
    assert list(got["index"]) == [0, 1, 2] and np.all(got["key"] == 0)
    w = np.array([0, -0.0, 1, 1, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    got = K.kcentre(F, 10, weight=w)                                # no centre yet: the key is the weight; then m w = 0 w
    assert list(got["index"][:3]) == [2, 0, 3]                      # 1 first; then keys +0 (rows 0, 3, 4..) above -0 (row 1)
    assert got["index"][9] == 1 and np.signbit(got["key"][9])


RANDOM = [(200, 50, 30, False, 11), (150, 300, 25, True, 12), (120, 1000, 20, False, 13), (60, 4096, 15, True, 14),
          (90, 8192, 10, False, 15)]


@pytest.mark.parametrize("R,D,k,weighted,seed", RANDOM)
def test_within_the_derived_bound_on_random_features(R, D, k, weighted, seed, record_property):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, D)).astype(np.float32)
    w = (rng.random(R).astype(np.float32) + np.float32(0.5)) if weighted else None
    cen = [int(rng.integers(0, R))]
    idx, key, dist, m, gaps = K.greedy64(F, k, w, None, cen)
    bound_d, bound_k = _g(_levels(D) + 3), _g(_levels(D) + 4)
    assert np.all(gaps > 2 * bound_k * np.abs(key)), "a near tie in the float64 reference: choose another seed"
    got = K.kcentre(F, k, w, None, cen)
    assert np.array_equal(got["index"], idx)
    used_d = np.max(np.abs(got["dist"].astype(np.float64) - dist) / dist)
    used_k = np.max(np.abs(got["key"].astype(np.float64) - key) / key)
    live = m > 0
    used_m = np.max(np.abs(got["min_dist"].astype(np.float64)[live] - m[live]) / m[live])
    print(f"R={R} D={D}: used {used_d / bound_d:.3f} of the distance bound {bound_d:.3e}, {used_k / bound_k:.3f} of the key bound, "
          f"{used_m / bound_d:.3f} on min_dist")
    record_property("bound_used", float(max(used_d / bound_d, used_k / bound_k, used_m / bound_d)))
    assert used_d <= bound_d and used_m <= bound_d and used_k <= bound_k
    assert np.all(got["min_dist"][idx] == 0)                        # d(r, r) is exactly +0


def test_sum_order_is_the_header_s():
    # one row whose sum depends on the order: the restated order against the same order spelled out lane by lane
    rng = np.random.default_rng(21)
    for D in (5, 256, 257, 1024, 1025, 2049):
        p = (rng.random((1, D)) * 10.0 ** rng.integers(-3, 4, size=(1, D))).astype(np.float32)
        T = 64 if D <= 1024 else 256
        acc = [np.float32(0)] * T
        for q in range((D + 3) // 4):
            for e in range(4):
                if 4 * q + e < D:
                    acc[q % T] = np.float32(acc[q % T] + p[0, 4 * q + e])
        waves = []
        for wv in range(T // 64):
            v = acc[64 * wv:64 * wv + 64]
            for off in (32, 16, 8, 4, 2, 1):
                v = [np.float32(v[i] + v[i ^ off]) for i in range(64)]
            waves.append(v[0])
        want = waves[0]
        for x in waves[1:]:
            want = np.float32(want + x)
        assert K.row_sums(p)[0] == want


def test_properties():
    rng = np.random.default_rng(31)
    F = rng.standard_normal((300, 40)).astype(np.float32)
    ex = (rng.random(300) < 0.3).astype(np.uint8)
    got = K.kcentre(F, 50, None, ex, [5])
    assert np.all(np.diff(got["dist"]) <= 0)                        # without weights the picks' distances never increase
    rest = (ex == 0)
    rest[got["index"]] = False
    assert got["min_dist"][rest].max() <= got["dist"][-1]           # nobody left is farther than the last pick was
    # a + b picks equal a picks, then resume with the picks excluded
    w = rng.random(300).astype(np.float32)
    for weight in (None, w):
        whole = K.kcentre(F, 30, weight, ex, [5, 7])
        first = K.kcentre(F, 12, weight, ex, [5, 7])
        ex2 = ex.copy()
        ex2[first["index"]] = 1
        second = K.kcentre(F, 18, weight, ex2, (), resume=True, min_dist=first["min_dist"])
        for f in ("index", "key", "dist"):
            assert np.array_equal(np.concatenate([first[f], second[f]]).view(np.uint32), whole[f].view(np.uint32)), f
        assert np.array_equal(second["min_dist"].view(np.uint32), whole["min_dist"].view(np.uint32))


def test_void_rows_change_nothing_else():
    rng = np.random.default_rng(41)
    F = rng.standard_normal((60, 33)).astype(np.float32)
    w = rng.random(60).astype(np.float32)
    base = K.kcentre(F, 60, w, None, [3])
    G = np.vstack([F, np.zeros((3, 33), dtype=np.float32)])
    G[60, 4], G[61, 0], G[62, :] = np.nan, np.inf, 3e19             # a NaN, an infinity, a norm that overflows
    w2 = np.concatenate([w, np.ones(3, dtype=np.float32)])
    got = K.kcentre(G, 63, w2, None, [3, 61, 99, -2])               # a void and two out-of-range centres: ignored
    assert got["counts"] == [60, 60, 3, 0] and got["ignored"] == 2
    assert np.array_equal(got["index"][:60], base["index"]) and np.all(got["index"][60:] == -1)
    assert np.array_equal(got["key"][:60].view(np.uint32), base["key"].view(np.uint32))
    assert np.array_equal(got["min_dist"][:60].view(np.uint32), base["min_dist"].view(np.uint32))
    assert np.all(got["min_dist"][60:].view(np.uint32) == 0x7fc00000)
    w3 = w.copy()
    w3[[7, 8]] = np.nan, -1.0                                       # a NaN or negative weight: no candidate, counted void
    got = K.kcentre(F, 60, w3, None, [3])
    assert got["counts"] == [58, 58, 2, 0] and 7 not in got["index"] and 8 not in got["index"]
    assert np.all(np.isfinite(got["min_dist"]))
