"""CPU tests of the quantile restatement (tests/_quantiles_np.py): the fp32 EMPIRICAL form against np.quantile, and the
MEASUREMENT of EPS_F -- the error the fp32 evaluation of the mixture CDF must be allowed for the 2-ulp bracket criterion of
include/vbnn_hip.h to hold against float64 -- on every mixture input set the GPU tests use."""
import functools

import numpy as np
import pytest

from tests import _quantiles_np as Q

EPS_F = Q.EPS_F                      # 4 x the largest value measured below (see the comment beside Q.EPS_F)


def test_empirical_form_is_numpy_linear():
    rng = np.random.default_rng(5)
    for S, R, D in ((1, 3, 4), (2, 3, 5), (7, 5, 9), (30, 11, 10), (128, 4, 6)):
        y = (3.0 * rng.standard_normal((S, R, D))).astype(np.float32)
        y[:, 0, 0] = y[0, 0, 0]                                        # all draws equal: every quantile is that value
        if S > 2:
            y[1, 1, 1] = y[2, 1, 1]                                    # duplicates
        p = (0.001, 0.05, 0.25, 0.5, 0.9, 0.999)
        q, _ = Q.empirical32(y, p)
        ref = np.quantile(y.astype(np.float64), [float(np.float32(v)) for v in p], axis=0, method="linear")
        # fp32 rounding: a few ulp of the values, and the rounding of the position p (S - 1) (half an ulp of S - 1 at most)
        # times the gap between neighbours (the draws' range at most)
        scale, spread = np.abs(y).max(0), y.max(0) - y.min(0)
        tol = 4 * np.spacing(scale.astype(np.float32)) + np.spacing(np.float32(max(S - 1, 1))) * spread
        assert (np.abs(q - ref) <= tol).all()
        assert (q[:, 0, 0] == y[0, 0, 0]).all()
        assert (np.diff(q, axis=0) >= 0).all()
    # exact where S - 1 divides the position: p (S - 1) is an integer in fp32
    y = rng.standard_normal((5, 6, 7)).astype(np.float32)
    q, _ = Q.empirical32(y, (0.25, 0.5, 0.75))
    assert np.array_equal(q, np.sort(y, 0)[[1, 2, 3]])
    y = rng.standard_normal((3, 6, 7)).astype(np.float32)
    q, _ = Q.empirical32(y, (0.5,))
    assert np.array_equal(q[0], np.sort(y, 0)[1])


def test_empirical_pit_and_nan():
    rng = np.random.default_rng(6)
    y = rng.standard_normal((7, 4, 5)).astype(np.float32)
    t = rng.standard_normal((4, 5)).astype(np.float32)
    t[0, 0] = y[3, 0, 0]                                               # a target equal to a draw counts (<=)
    t[1, 1] = np.nan
    y[2, 2, 2] = np.nan
    q, pit = Q.empirical32(y, (0.1, 0.9), t)
    assert pit[0, 0] == np.float32((y[:, 0, 0] <= t[0, 0]).sum()) / np.float32(7)
    assert np.isnan(pit[1, 1]) and np.isnan(pit[2, 2]) and np.isnan(q[:, 2, 2]).all()
    assert np.isnan(q).sum() == 2 and np.isnan(pit).sum() == 2


@functools.lru_cache(maxsize=None)
def measured(name):
    """The largest eps the restatement needs on this input set: over its quantiles (the bracket criterion at the fp32 root)
    and its PIT."""
    y, t, kind, p, kw = Q.mixture_case(name)
    mu, sigma = Q.components(y, kind, **kw)
    m32, c = Q.c32(y, kind, **kw)
    worst = float(np.abs(Q.cdf32(t, m32, c).astype(np.float64) - Q.cdf64(t.astype(np.float64), mu, sigma)).max())
    prev = None
    for pj in p:
        q = Q.root32(pj, m32, c, sigma)
        worst = max(worst, float(Q.eps_needed(q, float(np.float32(pj)), mu, sigma).max()))
        assert prev is None or (q >= prev).all()
        prev = q
    return worst


@pytest.mark.parametrize("name", list(Q.MIXTURE_CASES))
def test_eps_f_is_measured_not_assumed(name):
    eps = measured(name)
    print(f"{name}: the restatement needs eps_F = {eps:.3e} (EPS_F / 4 = {EPS_F / 4:.3e})")
    assert eps <= EPS_F / 4


def test_eps_f_is_four_times_the_largest_measured():
    worst = max(measured(name) for name in Q.MIXTURE_CASES)
    print(f"largest measured eps_F = {worst:.3e}")
    assert worst <= EPS_F / 4 <= 1.05 * worst + 1e-12               # the constant follows the measurement, not the reverse


def test_float64_root_and_s1_closed_form():
    """S = 1: the root is mu + sigma Phi^-1(p); the float64 bisection finds it."""
    from statistics import NormalDist
    y, t, kind, p, kw = Q.mixture_case("gauss-37x7-S1")
    mu, sigma = Q.components(y, kind, **kw)
    for pj in p:
        ref = mu[0] + sigma[0] * NormalDist().inv_cdf(float(pj))
        got = Q.root64(float(pj), mu, sigma)
        assert np.allclose(got, ref, rtol=0, atol=1e-9 * (np.abs(ref) + sigma[0]))
