"""CPU tests of the restatements the calibration GPU tests compare against (tests/_calibration_np.py): calibration32 against the
float64 definition inside the bounds that file derives, the bin edges, the order of the selective keys, the tie rule, and the
invariances the integer accumulator is there for (halves, permutations)."""
import numpy as np
import pytest

from tests._calibration_np import (EPS, F32, brier_bound, calibration32, calibration64, derived, keys32, ranks, row_sumsq32,
                                   selective32, selective_accuracy, softmax_case, unkey32)


@pytest.mark.parametrize("C", [2, 3, 10, 17, 255, 256, 257, 1000, 4099])
def test_restatement_against_float64(C):
    R, M = 257, 15
    probs, pred, target = softmax_case(R, C, scale=2.0 if C < 1000 else 4.0)
    got, ref = calibration32(probs, pred, target, M), calibration64(probs, pred, target, M)
    d = derived(got["acc"], M)
    assert (got["conf"] >= 2.0 ** -9).all()                  # where the fixed-point conversion truncates nothing
    assert np.array_equal(d["count"], ref["count"]) and np.array_equal(d["hits"], ref["hits"]) and d["n"] == R and d["n_nan"] == 0
    # per bin: the fixed-point sum is exact here, so it differs from the float64 sum by that sum's own rounding; 2^-32 on top
    tol_bin = 2.0 ** -32 + ref["count"] * 2.0 ** -52 * np.maximum(ref["confidence_sum"], 1.0)
    err_bin = np.abs(d["confidence_sum"] - ref["confidence_sum"])
    assert (err_bin <= tol_bin).all(), (err_bin / tol_bin).max()
    assert abs(d["ece"] - ref["ece"]) <= tol_bin.sum() / R + 2.0 ** -50
    nz = ref["count"] > 0
    assert abs(d["mce"] - ref["mce"]) <= (tol_bin[nz] / ref["count"][nz]).max() + 2.0 ** -50
    # the Brier score: per row inside the derived bound, the mean inside the mean bound + the conversion's 2^-32 a row
    bound = brier_bound(C, ref["ss"], ref["pt"], ref["brier_rows"])
    err = np.abs(got["brier"].astype(np.float64) - ref["brier_rows"])
    print(f"C {C}: brier err / bound {np.max(err / bound):.3f} (worst row error {err.max() / EPS:.2f} eps); "
          f"ece {d['ece']:.6f} mce {d['mce']:.6f} brier {d['brier']:.6f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert abs(d["brier"] - ref["brier"]) <= bound.mean() + 2.0 ** -32 + 2.0 ** -50


def test_row_sum_order_depends_on_C_alone():
    """The same row gives the same bits wherever it sits, and the two thread counts meet at C = 256 / 257."""
    rng = np.random.default_rng(2)
    for C in (5, 256, 257, 1030):
        P = rng.random((7, C)).astype(F32)
        full = row_sumsq32(P)
        for r in range(7):
            assert row_sumsq32(P[r:r + 1])[0].tobytes() == full[r].tobytes()
        assert np.abs(full.astype(np.float64) - (P.astype(np.float64) ** 2).sum(1)).max() <= 20 * EPS * C


@pytest.mark.parametrize("M", [4, 8, 16])
def test_bin_edges(M):
    """conf = j / M exactly lands in bin j; conf = 1 and a hair above 1 land in the last bin."""
    conf = np.array([j / M for j in range(M)] + [1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))], F32)
    R = conf.size
    probs = np.zeros((R, 2), F32)
    probs[:, 0] = conf
    probs[:, 1] = F32(1) - conf
    zero = np.zeros(R, np.int32)
    got = calibration32(probs, zero, zero, M)
    assert got["bin"].tolist() == list(range(M)) + [M - 1, M - 1, M - 1]
    d = derived(got["acc"], M)
    assert d["count"].tolist() == [1.0] * (M - 1) + [4.0] and d["n"] == R and d["accuracy"] == 1.0
    assert int(got["acc"][2 * M + 1]) == (1 << 32) // M      # conf = 1 / M in fixed point, exactly


def test_nan_row_is_skipped_and_changes_no_other_row():
    probs, pred, target = softmax_case(9, 20)
    clean = calibration32(probs, pred, target, 15)
    bad = probs.copy()
    bad[4, 7] = np.nan
    got = calibration32(bad, pred, target, 15)
    keep = np.arange(9) != 4
    for k in ("conf", "hit", "brier", "bin"):
        assert got[k][keep].tobytes() == clean[k][keep].tobytes()
    assert np.isnan(got["conf"][4]) and np.isnan(got["brier"][4]) and got["hit"][4] == -1 and got["bin"][4] == -1
    one = calibration32(probs[4:5], pred[4:5], target[4:5], 15)["acc"]
    want = clean["acc"] - one
    want[3 * 15 + 2] += 1
    assert np.array_equal(got["acc"], want)


def test_out_of_range_classes_are_clamped():
    probs, pred, target = softmax_case(6, 5)
    wild_p, wild_t = pred.copy(), target.copy()
    wild_p[0], wild_p[1], wild_t[2], wild_t[3] = -7, 99, -1, 5
    ref_p, ref_t = np.clip(wild_p, 0, 4), np.clip(wild_t, 0, 4)
    a, b = calibration32(probs, wild_p, wild_t, 8), calibration32(probs, ref_p, ref_t, 8)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_two_halves_equal_one_call_and_rows_may_be_permuted():
    probs, pred, target = softmax_case(301, 10)
    one = calibration32(probs, pred, target, 15)["acc"]
    half = calibration32(probs[:150], pred[:150], target[:150], 15)["acc"]
    both = calibration32(probs[150:], pred[150:], target[150:], 15, acc=half)["acc"]
    assert np.array_equal(one, both)
    perm = np.random.default_rng(0).permutation(301)
    assert np.array_equal(one, calibration32(probs[perm], pred[perm], target[perm], 15)["acc"])


# ------------------------------------------------------------------------------------------------ selective
def test_key_order():
    vals = np.array([np.nan, np.inf, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf], F32)
    k = keys32(vals)
    assert (np.diff(k.astype(np.int64)) < 0).all()           # descending as listed: -inf first, -0 below +0, NaN last
    assert unkey32(k)[1:].tobytes() == vals[1:].tobytes() and unkey32(k)[:1].view(np.uint32)[0] == 0x7FC00000
    neg_nan = np.array([0xFFC00001], np.uint32).view(F32)      # every NaN is the positive quiet NaN
    assert keys32(neg_nan)[0] == keys32(np.array([np.nan], F32))[0] == 0xFFC00000
    tau, counts = selective32(vals, np.ones(9, np.int32), [1, 4, 5, 9])
    assert tau[0] == -np.inf and tau[1].tobytes() == F32(-0.0).tobytes() and tau[2].tobytes() == F32(0.0).tobytes() and np.isnan(tau[3])
    assert counts[:, 0].tolist() == [0, 3, 4, 8] and counts[:, 2].tolist() == [1, 1, 1, 1]


def test_all_equal_scores_give_the_overall_accuracy():
    rng = np.random.default_rng(1)
    hit = (rng.random(1000) < 0.7).astype(np.int32)
    hit[:100] = 1                                            # the first rows are all right: a row-order tie-break would say 100 %
    covs = [0.01, 0.1, 0.5, 0.9, 1.0]
    ks = ranks(covs, 1000)
    assert ks == [10, 100, 500, 900, 1000]
    tau, counts = selective32(np.zeros(1000, F32), hit, ks)
    acc = selective_accuracy(counts, ks)
    assert (tau == 0).all() and counts[:, 0].tolist() == [0] * 5 and counts[:, 2].tolist() == [1000] * 5
    assert all(abs(a - hit.mean()) <= 1e-15 for a in acc)


def test_selective_against_a_sort_and_under_permutation():
    rng = np.random.default_rng(3)
    R = 777
    score = rng.integers(0, 40, R).astype(F32) / F32(8) - F32(2)          # many duplicates, both signs
    hit = (rng.random(R) < 0.6).astype(np.int32)
    ks = [1, 2, 100, 388, 776, 777]
    tau, counts = selective32(score, hit, ks)
    order = np.argsort(score, kind="stable")
    for j, k in enumerate(ks):
        assert tau[j] == score[order[k - 1]]
        nb, hb, nt, ht = (int(v) for v in counts[j])
        assert nb < k <= nb + nt and nb == (score < tau[j]).sum() and nt == (score == tau[j]).sum()
        # no tie straddles the rank: the plain accuracy of the first k sorted rows
        if nb + nt == k:
            assert selective_accuracy(counts[j:j + 1], [k])[0] == pytest.approx(hit[order[:k]].mean(), abs=1e-15)
    perm = rng.permutation(R)
    tau2, counts2 = selective32(score[perm], hit[perm], ks)
    assert tau2.tobytes() == tau.tobytes() and np.array_equal(counts, counts2)
