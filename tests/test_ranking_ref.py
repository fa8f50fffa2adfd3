"""CPU tests of the NumPy restatement of vbnn_rank_metrics (tests/_ranking_np.py), which the GPU tests compare bit for bit: it
is held to the brute-force O(R^2) definitions of include/vbnn_hip.h in Python ints, to the exact rational average precision (the
fixed-point value lies within 2^-32 below it), to scikit-learn where that is installed, and to the closed cases."""
from fractions import Fraction

import numpy as np
import pytest

from tests._ranking_np import (F32, SEVEN, TWO32, ap_fraction, brute, derived, labels, order32, rank_metrics, scores, targets01)

KINDS = ["distinct", "normal", "seven", "equal", "low_byte", "high_byte", "saturated"]


def sprinkle_nan(s, t, seed):
    rng = np.random.default_rng(seed)
    s, t = s.copy(), t.copy()
    s[rng.random(s.shape) < 0.05] = np.nan
    t[rng.random(t.shape) < 0.05] = np.nan
    return s, t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", [1, 2, 65, 300])
def test_restatement_equals_the_brute_force_definitions(kind, R):
    D, tau = 3, (0.5, 0.0, -0.0, 1.0, float("inf"), float("-inf"), float("nan"), 1e-42)
    s, t = sprinkle_nan(scores(kind, R, D, seed=1), targets01(R, D, seed=1), seed=R)
    got = rank_metrics(s, target=t, tau=tau)
    pos, counted = labels(s, target=t)
    for j in range(D):
        c = counted[:, j]
        want = brute(s[c, j], pos[c, j], tau)
        want[2] = int(R - c.sum())
        assert got[j] == want, (kind, R, j)
        assert got[j][0] + got[j][1] + got[j][2] == R and got[j][5] == 0


@pytest.mark.parametrize("D", [3, 17])
def test_class_targets_are_one_against_the_rest(D):
    R = 200
    s = scores("seven", R, D, seed=2)
    tc = np.random.default_rng(D).integers(-3, D + 3, R).astype(np.int32)           # out of range on both sides: clamped
    onehot = (np.clip(tc, 0, D - 1)[:, None] == np.arange(D)[None, :]).astype(F32)
    assert rank_metrics(s, target_class=tc, tau=(0.5,)) == rank_metrics(s, target=onehot, tau=(0.5,))
    pos, _ = labels(s, target_class=tc)
    for j in range(D):
        assert rank_metrics(s, target_class=tc, tau=(0.5,))[j] == brute(s[:, j], pos[:, j], (0.5,))


@pytest.mark.parametrize("kind", KINDS)
def test_fixed_point_average_precision_is_within_2_to_minus_32_below_the_exact_rational(kind):
    R, D = 257, 2
    s, t = scores(kind, R, D, seed=3), targets01(R, D, seed=3)
    for j, w in enumerate(rank_metrics(s, target=t)):
        exact = ap_fraction(s[:, j], t[:, j] > 0.5)
        gap = exact - Fraction(w[4], TWO32 * w[0])
        assert 0 <= gap < Fraction(1, TWO32), (kind, j, float(gap))


def test_against_scikit_learn():
    sk = pytest.importorskip("sklearn.metrics")
    for seed in range(30):
        for kind in ("normal", "seven", "saturated"):
            R = 50 + 13 * seed
            s, t = scores(kind, R, 1, seed=seed), targets01(R, 1, seed=seed)
            w = rank_metrics(s, target=t)[0]
            if not (w[0] and w[1]):
                continue
            d = derived(w, 0)
            y, x = (t[:, 0] > 0.5).astype(int), s[:, 0].astype(np.float64)
            x = np.clip(x, -1e300, 1e300)                    # (scikit-learn refuses infinities; the order is kept)
            assert abs(d["auroc"] - sk.roc_auc_score(y, x)) <= 1e-12, (seed, kind)
            assert abs(d["average_precision"] - sk.average_precision_score(y, x)) <= 1e-9, (seed, kind)


def test_closed_cases():
    R = 101
    t = targets01(R, 1, seed=5)
    n_pos, n_neg = int(t.sum()), int(R - t.sum())
    assert n_pos and n_neg
    # all scores equal: every pair is a tie
    w = rank_metrics(np.full((R, 1), 0.7, F32), target=t)[0]
    assert w[:3] == [n_pos, n_neg, 0] and w[3] == n_pos * n_neg and derived(w, 0)["auroc"] == 0.5
    assert w[4] == n_pos * ((n_pos * TWO32) // R)
    # perfect separation
    s = (t * F32(0.25) + F32(0.1) + np.arange(R, dtype=F32)[:, None] * F32(2.0 ** -12)).astype(F32)
    w = rank_metrics(s, target=t)[0]
    assert w[3] == 2 * n_pos * n_neg and w[4] == n_pos * TWO32
    d = derived(w, 0)
    assert d["auroc"] == 1.0 and d["average_precision"] == 1.0
    # reversed
    w = rank_metrics(-s, target=t)[0]
    assert w[3] == 0 and derived(w, 0)["auroc"] == 0.0
    # -0 and +0 tie, and are met by a threshold of either sign
    s = np.array([[-0.0], [0.0], [-0.0], [0.0]], F32)
    t4 = np.array([[1], [0], [0], [1]], F32)
    assert order32(s).min() == order32(s).max() == 0x80000000
    assert rank_metrics(s, target=t4, tau=(0.0, -0.0))[0] == [2, 2, 0, 4, 2 * (TWO32 // 2), 0, 2, 2, 2, 2]
    # the order words ascend with the values
    assert (np.diff(order32(SEVEN).astype(np.int64))[[0, 1, 3, 4, 5]] > 0).all() and order32(SEVEN)[2] == order32(SEVEN)[3]


def test_no_positives_and_no_negatives():
    s = scores("normal", 50, 2, seed=6)
    t = np.stack([np.zeros(50, F32), np.ones(50, F32)], 1)
    w0, w1 = rank_metrics(s, target=t, tau=(0.0,))
    assert w0[0] == 0 and w0[3] == 0 and w0[4] == 0 and w1[1] == 0 and w1[3] == 0
    d0, d1 = derived(w0, 1), derived(w1, 1)
    assert np.isnan(d0["auroc"]) and np.isnan(d0["average_precision"]) and np.isnan(d1["auroc"])
    assert d1["average_precision"] == 1.0 and w1[4] == sum((k * TWO32) // k for k in range(1, 51))
