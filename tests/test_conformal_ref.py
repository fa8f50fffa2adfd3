"""CPU tests of the conformal restatement (tests/_conformal_np.py), which the GPU tests compare vbnn_conformal with bit for bit:
it is held to a score-every-class, compare-every-class form; to the float64 definition within a derived bound; the prefix
property is asserted on random and on heavily tied rows; the rank k is exact; and the split-conformal guarantee itself is
measured over random calibration / test splits."""
from fractions import Fraction

import numpy as np
import pytest

from tests._calibration_np import row_sumsq32, softmax_case
from tests._conformal_np import (APS, F32, LAC, aps_bound, brute32, conformal32, conformal_rank, derived, lac_bound, masked_sum32,
                                 order_word, positions, ranking, row_sum32, scores64, scores_all32, tied_case)

KINDS = [LAC, APS]


def special_rows(C):
    P = tied_case(8, C, seed=C)
    P[0] = F32(1.0 / C)                                      # uniform
    P[1] = 0
    P[1, C // 2] = 1                                         # one-hot: the zeros tie by index
    P[2, ::2] = F32(-0.0)
    P[2, 1::3] = F32(1e-41)
    P[3] = F32(-0.0)
    P[3, C - 1] = 0.0
    return P


def own_thresholds(P, target, kind):
    s = conformal32(P, target, kind)["score"]
    return np.array([s[0], s[len(s) // 2], np.nextafter(s.min(), F32(-np.inf)), 0, -1, np.inf, np.nan, 0.5], F32)


@pytest.mark.parametrize("C", [1, 2, 3, 17, 64, 300])
def test_the_row_sum_is_the_calibration_family_s(C):
    P, _, _ = softmax_case(9, C, seed=C)
    assert row_sum32(P * P).tobytes() == row_sumsq32(P).tobytes()


def test_ranking_ties_go_to_the_lower_index_and_minus_zero_ranks_below_zero():
    P = np.array([[0.25, 0.5, 0.25, -0.0, 0.0, 0.5]], F32)
    assert ranking(P).tolist() == [[1, 5, 0, 2, 4, 3]]
    assert order_word(np.array([-0.0], F32))[0] + 1 == order_word(np.array([0.0], F32))[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1, 2, 3, 10, 17, 64])
def test_restatement_equals_score_every_class_compare_every_class(C, kind):
    for name, P in (("softmax", softmax_case(12, C, seed=C)[0]), ("tied", tied_case(12, C, seed=C)), ("special", special_rows(C))):
        target = (np.arange(P.shape[0]) * 5 % C).astype(np.int32)
        qhat = own_thresholds(P, target, kind)
        w = conformal32(P, target, kind, qhat)
        b = brute32(P, kind, qhat)
        pos = positions(w["order"])
        assert ((pos[None] < w["n"][:, :, None]) == b["member"]).all(), name
        rows = np.arange(P.shape[0])
        assert w["score"].tobytes() == b["scores"][rows, np.clip(target, 0, C - 1)].tobytes()
        assert (w["covered"] == b["member"][:, rows, np.clip(target, 0, C - 1)]).all()
        assert (w["size"] == b["member"].sum(2)).all()
        # the last admitted class is the member that ranks last
        for q in range(len(qhat)):
            for r in rows:
                m = np.flatnonzero(b["member"][q, r])
                assert w["cut_index"][q, r] == (m[np.argmax(pos[r, m])] if m.size else -1)
        bits = ((w["member"][..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(qhat), P.shape[0], -1)
        assert (bits[:, :, :C] == b["member"]).all() and (bits[:, :, C:] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [5, 64, 257, 1000])
def test_scores_never_decrease_along_the_ranking(C, kind):
    """The prefix property, on random rows and on rows of sixteenths (large tie groups)."""
    R = 6 if C > 64 else 16
    for P in (softmax_case(R, C, seed=C, scale=4.0)[0], tied_case(R, C, seed=C + 1), special_rows(C)):
        if C <= 64:
            S = scores_all32(P, kind)
        else:                                                # every rank, without C^2 work a row: a few hundred ranks
            order = ranking(P)
            picks = np.unique(np.concatenate([np.arange(0, C, max(1, C // 200)), [C - 1]]))
            pos = positions(order)
            S = np.stack([masked_sum32(P, pos <= i) if kind == APS else (F32(1) - np.take_along_axis(P, order[:, i:i + 1], 1)[:, 0])
                          for i in picks], 1)
            assert (np.diff(S, axis=1) >= 0).all()
            continue
        along = np.take_along_axis(S, ranking(P), 1)
        assert (np.diff(along, axis=1) >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [3, 10, 64, 257, 1000, 4099])
def test_restatement_against_the_float64_definition(C, kind):
    R = 8
    P, _, target = softmax_case(R, C, seed=C, scale=3.0)
    rows, t = np.arange(R), np.clip(target, 0, C - 1)
    s32 = conformal32(P, target, kind)["score"].astype(np.float64)
    s64 = scores64(P, kind)[rows, t]
    bound = aps_bound(C, s64) if kind == APS else lac_bound(s64)
    err = np.abs(s32 - s64)
    assert (err <= bound).all()
    share = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"kind {kind} C {C}: largest share of the derived bound used = {share:.3f}")
    if C <= 64:                                              # every class, not the target alone
        S32, S64 = scores_all32(P, kind).astype(np.float64), scores64(P, kind)
        assert (np.abs(S32 - S64) <= (aps_bound(C, S64) if kind == APS else lac_bound(S64))).all()


def test_rank_is_exact():
    assert conformal_rank(99, 0.9) == 90                     # (100 * 0.9 in floats is 90.00000000000001: ceil gives 91)
    assert conformal_rank(9, 0.9) == 9 and conformal_rank(10, 0.9) == 10 and conformal_rank(19, 0.95) == 19
    assert conformal_rank(1, 0.5) == 1 and conformal_rank(4, 0.99) == 5 and conformal_rank(999, 0.999) == 999
    for n in (1, 7, 99, 100, 1000, 12345):
        for lv in (0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.975, 0.99, 0.999):
            x = (n + 1) * Fraction(repr(lv))
            k = conformal_rank(n, lv)
            assert k - 1 < x <= k
    from vbnn_amd.conformal import conformal_rank as engine_rank
    assert all(engine_rank(n, lv) == conformal_rank(n, lv) for n in (1, 99, 400, 12345) for lv in (0.5, 0.9, 0.95, 0.999))


def test_acc_words_and_what_the_host_derives():
    P, _, target = softmax_case(40, 6, seed=2)
    P[7, 3] = np.nan
    qhat = np.array([0.3, 0.9, -1, np.inf], F32)
    w = conformal32(P, target, APS, qhat)
    d, n_nan = derived(w["acc"], 4)
    assert n_nan == 1 and all(x["n"] == 39 for x in d) and int(w["acc"][7]) == 0 and int(w["acc"][8 * 4 + 1]) == 0
    assert d[2]["empty_fraction"] == 1.0 and d[2]["coverage"] == 0.0 and d[3]["full_fraction"] == 1.0 and d[3]["coverage"] == 1.0
    ok = np.arange(40) != 7
    assert d[0]["mean_size"] == w["size"][0][ok].mean() and d[1]["coverage"] == (w["covered"][1][ok] == 1).mean()
    assert w["size"][0][7] == -1 and np.isnan(w["score"][7]) and (w["member"][:, 7] == 0).all()
    halves = conformal32(P[20:], target[20:], APS, qhat, acc=conformal32(P[:20], target[:20], APS, qhat)["acc"])
    assert halves["acc"].tobytes() == w["acc"].tobytes()
    blind = conformal32(P, None, APS, qhat)
    assert blind["size"].tobytes() == w["size"].tobytes() and all(int(blind["acc"][8 * q + j]) == 0 for q in range(4) for j in (1, 5))


@pytest.mark.parametrize("kind", KINDS)
def test_the_coverage_guarantee(kind):
    """Split conformal prediction over T random calibration / test splits of ONE exchangeable set: the mean coverage is at least
    k / (n + 1), here asserted as a LOWER bound with 5 standard errors of slack. Given the calibration set the coverage is
    Beta(k, n + 1 - k) distributed (variance a b / ((a + b)^2 (a + b + 1))) and the test set adds the binomial c (1 - c) / m;
    both divided by T. n, m, T and the seed are chosen so that the run takes a second."""
    n, m, T, C, level = 199, 300, 200, 10, 0.9
    rng = np.random.default_rng(17)
    P, _, _ = softmax_case(n + m, C, seed=23, scale=1.5)
    cdf = np.cumsum(P.astype(np.float64), 1)
    y = np.minimum((rng.random(n + m)[:, None] * cdf[:, -1:] > cdf).sum(1), C - 1).astype(np.int32)      # labels drawn from P
    s = conformal32(P, y, kind)["score"]                     # a row's score does not depend on the split
    k = conformal_rank(n, level)
    assert k == 180
    cov = np.empty(T)
    for i in range(T):
        perm = rng.permutation(n + m)
        qhat = np.sort(s[perm[:n]])[k - 1]
        test = perm[n:]
        w = conformal32(P[test[:8]], y[test[:8]], kind, [qhat])      # the sets' own covered flags are the comparison
        assert (w["covered"][0] == (s[test[:8]] <= qhat)).all()
        cov[i] = (s[test] <= qhat).mean()
    a, b = k, n + 1 - k
    c = k / (n + 1)
    se = np.sqrt((a * b / ((a + b) ** 2 * (a + b + 1)) + c * (1 - c) / m) / T)
    print(f"kind {kind}: mean coverage {cov.mean():.4f} against k / (n + 1) = {c:.4f}, SE {se:.4f}")
    assert cov.mean() >= c - 5 * se
