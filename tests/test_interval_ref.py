"""CPU tests of the restatement tests/_interval_np.py that the GPU tests compare the kernels with bit for bit: the fp32 scores
against the float64 definition within the bound derived there, the column select against brute-force counting, the rule that
`covered` follows the score (and the cases where a comparison with the rounded end points would say otherwise), the ranks, and
the coverage guarantee itself, measured over random splits."""
import numpy as np
import pytest

from tests._interval_np import (EPS, F32, QNAN_BITS, W_MIN, calibrate32, conformal_rank, interval32, keys, order_word, score32,
                                score64, score_bound, select_columns32, unorder_word, width32, width64)


def test_scores_are_within_the_derived_bound_of_float64():
    rng = np.random.default_rng(2)
    R, D = 400, 37
    mean = rng.standard_normal((1, R, D)).astype(F32) * 3
    t = (mean[0] + rng.standard_normal((R, D)) * rng.gamma(2.0, 1.0, (R, D))).astype(F32)
    t[::7] = mean[0, ::7]                                    # exact hits: a zero score
    half = rng.gamma(2.0, 0.4, (1, R, D)).astype(F32)
    cases = {"absolute": (mean, mean, None, None), "cqr": ((mean - half).astype(F32), (mean + half).astype(F32), None, None)}
    var, noise = rng.gamma(2.0, 0.5, (R, D)).astype(F32), rng.gamma(2.0, 0.1, (R, D)).astype(F32)
    var[::5] = 0
    cases["scaled"] = (mean, mean, width32(var, None, 0.0, True, W_MIN), width64(var, None, 0.0, True, W_MIN))
    cases["scaled + noise plane + scalar"] = (mean, mean, width32(var, noise, 0.3, True, W_MIN), width64(var, noise, 0.3, True, W_MIN))
    cases["plain width"] = (mean, mean, width32(var, noise, 0.3, False, 0.25), width64(var, noise, 0.3, False, 0.25))
    for name, (a, b, w, w64) in cases.items():
        s32 = score32(a, b, t, w)["score"][0].astype(np.float64)
        s64 = score64(a[0], b[0], t, w64)
        bound = score_bound(a[0], b[0], t, s64, w is not None)
        err = np.abs(s32 - s64)
        share = float((err / bound).max())
        print(f"{name}: worst share of the derived bound {share:.3f}")
        assert (err <= bound).all(), (name, share)
        assert share > 0.05                                  # (the bound is not vacuous: some element uses a real part of it)
    assert (score32(mean, mean, t)["score"][0][::7] == 0).all()
    # "absolute" is |t - mean| exactly
    with np.errstate(invalid="ignore"):
        assert np.array_equal(score32(mean, mean, t)["score"][0], np.abs(t - mean[0]).astype(F32))


def brute_select(col, k):
    """The k-th smallest key of one column by counting, in Python ints: the key with below < k <= below + tied."""
    ky = [int(v) for v in keys(col)]
    for v in set(ky):
        below, tied = sum(1 for u in ky if u < v), sum(1 for u in ky if u == v)
        if below < k <= below + tied:
            return v, below, tied
    raise AssertionError("no key holds the rank")


def special_columns(R, rng):
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-41, -1e-41, 1.0, -1.0], F32)
    neg_nan = np.array([0xFFFFFFFF], np.uint32).view(F32)[0]
    cols = [rng.standard_normal(R).astype(F32), (np.round(rng.standard_normal(R) * 8) / 8).astype(F32), np.full(R, 0.375, F32),
            np.full(R, np.nan, F32), rng.choice(pool, R), np.where(rng.random(R) < 0.5, neg_nan, rng.standard_normal(R)).astype(F32),
            rng.choice(np.array([-0.0, 0.0], F32), R)]
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("R", [1, 2, 3, 17, 256, 301])
def test_select_equals_brute_force(R):
    rng = np.random.default_rng(R)
    x = special_columns(R, rng)
    ranks = sorted({1, R, (R + 1) // 2, max(1, R // 3), max(1, (9 * R) // 10)}) + [(R + 1) // 2]      # (a repeat)
    got = select_columns32(x, ranks)
    for d in range(x.shape[1]):
        for j, k in enumerate(ranks):
            key, below, tied = brute_select(x[:, d], k)
            assert int(order_word(got["tau"][j, d:d + 1])[0]) == key, (d, k)
            assert got["counts"][j, d].tolist() == [below, tied], (d, k)
        assert int(got["n_nan"][d]) == int(np.isnan(x[:, d]).sum())
    assert (got["tau"][:, 2] == F32(0.375)).all() and (got["tau"][:, 3].view(np.uint32) == QNAN_BITS).all()
    # -0 ranks right below +0; the NaNs (either sign) rank last as the one quiet NaN
    z = select_columns32(x[:, 6:7], [1, R])["tau"][:, 0]
    col = x[:, 6]
    assert np.signbit(z[0]) == bool(np.signbit(col).any()) and np.signbit(z[1]) == bool(np.signbit(col).all())
    assert np.array_equal(unorder_word(order_word(x[:, 0])), x[:, 0])


def test_covered_follows_the_score_not_the_rounded_end_points():
    """Targets planted within +-3 ulps of the rounded upper end point fl(a + fl(q w)): [s <= q] and [t <= hi'] disagree on some of
    them (the division and the product round separately), and `covered` is the former -- the statistic that was calibrated."""
    rng = np.random.default_rng(0)
    R, D = 500, 8
    mean = rng.standard_normal((1, R, D)).astype(F32)
    disagreements = {}
    for name, w in (("scaled", width32(rng.gamma(2.0, 0.5, (R, D)).astype(F32))), ("absolute", None)):
        q = rng.gamma(2.0, 0.6, (1, D)).astype(F32)
        hi = interval32(mean, mean, q, None, w)["hi"][0]
        t = hi.copy()
        for _ in range(3):
            step = rng.integers(-1, 2, (R, D))
            t = np.where(step > 0, np.nextafter(t, F32(np.inf)), np.where(step < 0, np.nextafter(t, F32(-np.inf)), t)).astype(F32)
        out = interval32(mean, mean, q, t, w)
        s = score32(mean, mean, t, w)["score"][0]
        by_score = s <= q
        assert np.array_equal(out["covered"][0] == 1, by_score)
        by_end_points = (out["lo"][0] <= t) & (t <= out["hi"][0])
        disagreements[name] = int((by_score != by_end_points).sum())
        assert int(out["acc"][1]) == int(by_score.sum()) and np.array_equal(out["row_covered"][0], by_score.sum(1))
    print("elements where the two definitions differ:", disagreements)
    assert all(v >= 1 for v in disagreements.values())


def test_ranks_and_thresholds():
    assert conformal_rank(99, 0.9) == 90 and conformal_rank(199, 0.9) == 180 and conformal_rank(999, 0.9) == 900
    assert conformal_rank(5, 0.9) == 6 and conformal_rank(9, 0.9) == 9 and conformal_rank(1, 0.5) == 1
    rng = np.random.default_rng(1)
    s = rng.gamma(2.0, 1.0, (5, 3)).astype(F32)
    qhat, k = calibrate32(s, (0.5, 0.9))
    assert k == [3, 6] and np.array_equal(qhat[0], np.sort(s, axis=0)[2]) and np.isposinf(qhat[1]).all()
    qj, kj = calibrate32(s.max(axis=1), (0.5, 0.9), "joint")
    assert kj == [3, 6] and qj.shape == (2, 1) and qj[0, 0] == np.sort(s.max(axis=1))[2] and np.isposinf(qj[1, 0])
    # +inf covers every element that is not NaN; a NaN threshold is taken as +inf; a NaN score ranks last
    m = np.zeros((1, 5, 3), F32)
    t = s.copy()
    t[1, 1] = np.nan
    out = interval32(m, m, np.array([[np.inf] * 3, [np.nan] * 3], F32), t)
    assert out["acc"].tolist() == [14, 14, 4, 4, 0, 0, 0, 0] * 2 + [1, 1]
    assert out["covered"][0, 1, 1] == 255 and out["row_covered"][:, 1].tolist() == [-1, -1]
    sc = score32(m, m, t)
    assert sc["acc"].tolist() == [1, 1] and np.isnan(sc["row_score"][0, 1]) and sc["row_score"][0, 0] == np.abs(t[0]).max()
    q5, _ = calibrate32(sc["score"][0], (0.8,))              # k = 5 of 5: column 1's largest key is its NaN
    assert np.isnan(q5[0, 1]) and q5[0, 0] == np.abs(t[:, 0]).max()
    # a negative threshold shrinks a "cqr" interval; lo' > hi' is empty and counted
    a, b = np.full((1, 2, 1), -1, F32), np.full((1, 2, 1), 1, F32)
    e = interval32(a, b, np.array([[-1.5]], F32), np.array([[0.0], [5.0]], F32))
    assert e["lo"][0, 0, 0] == 0.5 and e["hi"][0, 0, 0] == -0.5 and int(e["acc"][4]) == 2 and int(e["acc"][1]) == 0


def exchangeable_set(rows, D, rng):
    """One heteroscedastic set with Student-t(3) noise and a deliberately mis-scaled width (the predictive believes a third of
    the spread where x is large and three times where it is small)."""
    x = rng.standard_normal((rows, 1))
    sigma = 0.3 + np.abs(x) * np.ones((1, D))
    mean = np.sin(x) * np.arange(1, D + 1)
    t = mean + sigma * rng.standard_t(3, (rows, D))
    believed = np.where(np.abs(x) > 1, sigma / 3, sigma * 3) ** 2
    return mean.astype(F32)[None], believed.astype(F32), t.astype(F32)


def coverage_over_splits(score, scope, n=199, m=300, T=200, D=3, level=0.9, seed=17):
    rng = np.random.default_rng(seed)
    mean, var, t = exchangeable_set(n + m, D, rng)
    w = width32(var) if score in ("scaled", "cqr") else None
    if score == "cqr":                                       # the believed 5 % and 95 % quantiles of a Gaussian of that width
        a, b, w = (mean - F32(1.645) * w).astype(F32), (mean + F32(1.645) * w).astype(F32), None
    else:
        a = b = mean
    cov = np.zeros((T, D if scope == "per_output" else 1))
    for i in range(T):
        p = rng.permutation(n + m)
        c, u = p[:n], p[n:]
        sc = score32(a[:, c], b[:, c], t[c], None if w is None else w[c])
        qhat, k = calibrate32(sc["score" if scope == "per_output" else "row_score"][0], (level,), scope)
        out = interval32(a[:, u], b[:, u], qhat if scope == "per_output" else qhat[:, 0], t[u], None if w is None else w[u],
                         scope == "per_output")
        cov[i] = (out["covered"][0] == 1).mean(axis=0) if scope == "per_output" else int(out["acc"][3]) / m
    k = conformal_rank(n, level)
    c = k / (n + 1)
    beta_var = k * (n + 1 - k) / ((n + 1) ** 2 * (n + 2))
    bound = c - 5 * np.sqrt((beta_var + c * (1 - c) / m) / T)
    return cov.mean(axis=0), bound


@pytest.mark.parametrize("scope", ["per_output", "joint"])
@pytest.mark.parametrize("score", ["scaled", "absolute", "cqr"])
def test_the_guarantee_measured(score, scope):
    """Mean coverage over T = 200 random splits of one exchangeable set is at least k / (n + 1) less 5 standard errors (the Beta(k,
    n + 1 - k) variance of a split's coverage plus the binomial c (1 - c) / m of its test rows, over T): 0.9 - 0.0097 here."""
    cov, bound = coverage_over_splits(score, scope)
    print(score, scope, "mean coverage", np.round(cov, 4), "bound", round(float(bound), 4))
    assert abs(bound - 0.8903) < 2e-4
    assert (cov >= bound).all()


def test_one_split_repairs_an_over_confident_predictive():
    """What tests/test_interval_gpu.py asserts of the engine, here of the restatement alone: one split with n = 999 and m = 1000,
    a predictive that believes a tenth of the true spread; the nominal 90 % interval covers far less than the conformal one, and
    the conformal one at least 0.9 - 5 sqrt(ab / ((a + b)^2 (a + b + 1)) + 0.09 / m) = 0.9 - 0.067 with a = 900, b = 100."""
    n, m, D = 999, 1000, 3
    rng = np.random.default_rng(11)
    mean, var, t = exchangeable_set(n + m, D, rng)
    var = (var / 100).astype(F32)
    w = width32(var)
    bound = 0.9 - 5 * np.sqrt(900 * 100 / (1000 ** 2 * 1001) + 0.09 / m)
    assert abs(bound - (0.9 - 0.067)) < 1e-3
    nominal = interval32(mean[:, n:], mean[:, n:], np.full((1, D), 1.645, F32), t[n:], w[n:])
    for scope in ("per_output", "joint"):
        sc = score32(mean[:, :n], mean[:, :n], t[:n], w[:n])
        qhat, k = calibrate32(sc["score" if scope == "per_output" else "row_score"][0], (0.9,), scope)
        assert k == [900]
        out = interval32(mean[:, n:], mean[:, n:], qhat if scope == "per_output" else qhat[:, 0], t[n:], w[n:], scope == "per_output")
        cov = int(out["acc"][1]) / int(out["acc"][0]) if scope == "per_output" else int(out["acc"][3]) / int(out["acc"][2])
        nom = int(nominal["acc"][1]) / int(nominal["acc"][0])
        print(scope, "nominal", nom, "conformal", cov, "bound", bound)
        assert nom < cov and cov >= bound
