"""CPU tests of vbnn_top_rows' restatement (tests/_acquire_np.py), which the GPU tests hold the device to: its det_logf is the
C oracle's bit for bit on the contract's range and on the ranges the stochastic key newly uses; its selection equals a plain
Python sort on the adversarial inputs; the keys do not depend on how the pool is split; and the stochastic selection has the
distribution it claims, sampling rows with probability proportional to score^beta."""
import math
import os
import re

import numpy as np
import pytest

from oracle import vbnn_oracle as vo
from tests import _acquire_np as A
from tests._philox_np import philox4x32_10

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def _restates_the_header():
    """The restatement is of include/'s contract: its stream id and cap are the header's, or it restates nothing."""
    philox = open(os.path.join(ROOT, "include", "vbnn_philox.h")).read()
    header = open(os.path.join(ROOT, "include", "vbnn_hip.h")).read()
    stream = re.search(r"^#define VBNN_STREAM_ACQUIRE\s+(\d+)u", philox, flags=re.M)
    cap = re.search(r"^#define VBNN_TOP_ROWS_MAX_K\s+(\d+)", header, flags=re.M)
    assert stream and int(stream.group(1)) == A.STREAM_ACQUIRE, "VBNN_STREAM_ACQUIRE"
    assert cap and int(cap.group(1)) == A.MAX_K, "VBNN_TOP_ROWS_MAX_K"


def _oracle_log(x):
    return np.array([vo.det_logf(float(v)) for v in x], F32)


def _ranges():
    rs = np.random.RandomState(5)
    u = ((rs.randint(0, 1 << 24, 6000).astype(np.int64) + 1).clip(max=(1 << 24) - 1).astype(F32) * F32(2.0 ** -24)).astype(F32)
    u = np.concatenate([u, np.array([2.0 ** -24, 1 - 2.0 ** -24, 0.5, 2.0 ** -23], F32)])
    E = np.concatenate([(-A.det_logf(u)).astype(F32), np.array([2.0 ** -24, 17.0, 1.0, 16.635532], F32),
                        np.exp(rs.uniform(math.log(2.0 ** -24), math.log(17.0), 4000)).astype(F32)])
    s = np.concatenate([A.floats(rs.randint(0x00800000, 0x7F800000, 8000).astype(np.uint32)),
                        A.floats(np.array([0x00800000, 0x7F7FFFFF, 0x3F800000, 0x3F7FFFFF, 0x3F800001], np.uint32))])
    return {"u in [2^-24, 1)": u, "E in [2^-24, 17]": E, "scores, normal range": s}


def test_det_logf_is_the_oracles_bit_for_bit_and_its_error_on_the_new_ranges():
    for name, x in _ranges().items():
        got, want = A.det_logf(x), _oracle_log(x)
        assert np.array_equal(A.bits(got), A.bits(want)), name
        ref = np.log(x.astype(np.float64))
        err = np.abs(got.astype(np.float64) - ref)
        away = np.abs(ref) >= 2.0 ** -6
        rel = float((err[away] / np.abs(ref[away])).max())
        near = float(err[~away].max()) if (~away).any() else 0.0
        print(f"det_logf, {name}: max relative error {rel:.3e} where |log x| >= 2^-6, max absolute error {near:.3e} nearer 1")
        # Derived, not measured: three roundings reach the result at full weight (den = 2 + f, s = f / den, the last fmaf:
        # 2^-24 each, f and s + s being exact), the polynomial's own roundings and the truncated series enter scaled by
        # z <= 0.03 (below 1e-8 together), and e ln 2 adds at most 127 x 1.9e-9 to a result of 88. The same roundings bound the
        # ABSOLUTE error near 1, at the scale of a result below 2^-6.
        bound = 3 * 2.0 ** -24 + 1e-8
        assert rel <= bound, (name, rel)
        assert near <= 2.0 ** -6 * bound, (name, near)


CASES = [(name, R) for name in ("normal", "equal", "two_values", "small_ints", "ascending", "descending", "low_bits", "top_bits",
                                "specials") for R in (1, 2, 65, 1023)]


@pytest.mark.parametrize("name,R", CASES)
def test_restated_top_rows_is_a_plain_sort(name, R):
    s = A.population(name, R)
    for ex in ("none", "half", "all", "all_but_one"):
        e = A.exclusion(ex, R)
        for k in sorted({1, 2, 7, 64, R, max(1, R - 1), R + 3}):
            for largest in (True, False):
                index, value, key, counts = A.top_rows(s, k, largest, e)
                want = A.brute_top_rows(s, k, largest, e)
                n = len(want)
                assert index[:n].tolist() == want and (index[n:] == -1).all()
                assert counts[0] == n and counts[1] + counts[2] + counts[3] == R
                assert np.array_equal(value[:n], A.bits(s)[want]) and np.array_equal(key[:n], value[:n])
                assert (value[n:] == A.QNAN).all() and (key[n:] == A.QNAN).all()


def test_keys_do_not_depend_on_how_the_pool_is_split():
    R = 1001
    s = A.population("positive", R)
    s[[3, 50]] = [0.0, np.inf]
    for row0 in (0, 7, 2 ** 31):
        whole = A.race_key(s, R, 2.0, 0x1234567890ABCDEF, 9, row0)
        for cut in (1, 2, 3, 500, 998):
            parts = np.concatenate([A.race_key(s[:cut], cut, 2.0, 0x1234567890ABCDEF, 9, row0),
                                    A.race_key(s[cut:], R - cut, 2.0, 0x1234567890ABCDEF, 9, row0 + cut)])
            assert np.array_equal(A.bits(whole), A.bits(parts))
    assert not np.array_equal(A.race_key(s, R, 2.0, 1, 9, 0), A.race_key(s, R, 2.0, 1, 10, 0))


def _keys_over_draws(score, beta, n_draws, seed):
    """race keys of R = len(score) rows for draws 0 .. n_draws - 1: n_draws x R."""
    R = len(score)
    g = np.arange(R, dtype=np.uint64)
    w = philox4x32_10((g >> np.uint64(2))[None, :], 0, np.arange(n_draws, dtype=np.uint64)[:, None], A.STREAM_ACQUIRE,
                      seed & 0xFFFFFFFF, seed >> 32)
    x = np.stack(w, axis=-1)[:, np.arange(R), (g & np.uint64(3)).astype(np.int64)]
    keys = A.race_key_of_words(x.reshape(-1), np.tile(score, n_draws), beta).reshape(n_draws, R)
    assert np.array_equal(A.bits(keys[5]), A.bits(A.race_key(score, R, beta, seed, 5, 0)))
    return keys


@pytest.mark.parametrize("beta", [1.0, 2.0])
def test_stochastic_selection_samples_in_proportion_to_score_to_the_beta(beta):
    """8 rows, 20 000 draws: the frequency of each row as THE pick (k = 1) and as the first of k = 3 lies within 5 binomial
    standard errors of score^beta / sum score^beta (derived, not measured; deterministic for the fixed seed). The first of
    k = 3 IS the top key, so its frequencies are the k = 1 ones: what the k = 3 round adds is only that the restatement's
    own selection puts that row first (checked on every 997th draw), not a second distributional fact."""
    score = np.array([0.5, 1.0, 2.0, 0.25, 3.0, 1.5, 0.75, 4.0], F32)
    n = 20000
    keys = _keys_over_draws(score, beta, n, seed=11)
    p = score.astype(np.float64) ** beta
    p /= p.sum()
    for k in (1, 3):
        first = np.empty(n, np.int64)
        for d in range(0, n, 997):                                    # the restatement's own selection on a sample of the draws
            first[d] = A.top_rows(score, k, True, None, beta=beta, seed=11, draw=d)[0][0]
            assert first[d] == np.argmax(keys[d])
        first = np.argmax(keys, axis=1)                                # (distinct keys: argmax is the top of the lexsort)
        freq = np.bincount(first, minlength=8) / n
        se = np.sqrt(p * (1 - p) / n)
        print(f"beta {beta:g}, k {k}: max |freq - p| / se = {(np.abs(freq - p) / se).max():.2f}")
        assert (np.abs(freq - p) <= 5 * se).all(), (freq, p, se)


def test_random_scores_none_is_uniform_and_special_scores_come_last():
    keys = _keys_over_draws(np.ones(8, F32), 1.0, 4000, seed=2)
    x = A.noise_words(8, 2, 7, 0)
    assert np.array_equal(A.bits(A.race_key(None, 8, 1.0, 2, 7, 0)), A.bits(A.race_key_of_words(x, np.ones(8, F32), 1.0)))
    freq = np.bincount(np.argmax(keys, axis=1), minlength=8) / 4000
    assert (np.abs(freq - 0.125) <= 5 * math.sqrt(0.125 * 0.875 / 4000)).all()
    s = A.floats(np.array([0x3F800000, 0, 0x80000000, 0xBF800000, 0x00000001, 0x7F800000, 0x7FC00000, 0x40000000], np.uint32))
    index, value, key, counts = A.top_rows(s, 8, True, None, beta=1.0, seed=3, draw=1)
    assert index[0] == 5 and set(index[1:3].tolist()) == {0, 7} and index[3:7].tolist() == [1, 2, 3, 4] and index[7] == -1
    assert counts == [7, 7, 1, 0]
    assert (A.floats(key[3:7]) == -np.inf).all() and A.floats(key[:1])[0] == np.inf
