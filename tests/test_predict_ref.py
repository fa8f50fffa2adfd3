"""CPU checks of tests/_predict_np.py, the reference the GPU tests of vbnn_head_predict compare against: the fp32 restatement of
the kernel's update stays inside the bounds on every input set of tests/test_head_predict_gpu.py (and the recorded shares are
re-measured), the float64 reference is the engine test's own definition, the tie constructions tie exactly and the underflow
sets underflow. No device, no vbnn_amd."""
import numpy as np
import pytest

from tests import _head_np as R
from tests import _predict_np as P

F = np.float32


def test_predict32_stays_inside_the_bounds_on_every_input_set():
    used = dict.fromkeys(P.BOUND_USED, 0.0)
    n_sets = 0
    for name, lg, t in P.input_sets():
        got = P.predict32(lg, t)
        _, ratios = P.check_predict(got, lg, t, label=name)
        ratios.update(P.check_states(got["states"], lg, t, label=name + " state"))
        bare = P.predict32(lg, None)                             # without targets: the same outputs, the target's sums 0
        for k in ("log_probs", "probs", "entropy", "expected_entropy", "mutual_info", "pred"):
            assert np.array_equal(bare[k], got[k]), (name, k)
        P.check_states(bare["states"], lg, None, label=name + " state, no targets")
        for k, v in ratios.items():
            used[k] = max(used[k], v)
        n_sets += 1
    print("shares of the bounds used:", {k: round(v, 3) for k, v in used.items()}, "over", n_sets, "sets")
    for k, v in used.items():
        assert v <= P.BOUND_USED[k] + 0.02, f"{k}: {v:.3f} measured, {P.BOUND_USED[k]} recorded"
        assert v >= 0.5 * P.BOUND_USED[k], f"{k}: the recorded {P.BOUND_USED[k]} is stale ({v:.3f} measured)"


def test_the_bias_sets_need_the_derived_term():
    """What the module docstring says of _classes_np's bounds: under a bias of +-30000 the rounding of lse alone is beyond them."""
    from tests import _classes_np as K
    op = P.extreme_set("bias+30000", 10)
    lg = P.stacked_logits(op)
    ref = P.predict64(lg, op["target"])
    assert P.lse_term(lg).max() > 100 * K.logp_tol(ref, 3).max()
    d = np.abs(P.predict32(lg, op["target"])["log_probs"] - ref["log_probs"])
    assert (d > K.logp_tol(ref, 3)).any() and (d <= P.logp_tol(ref, lg)).all()


def test_predict64_is_the_engine_tests_definition():
    from tests.test_predict_gpu import oracle_predictive
    rng = np.random.default_rng(3)
    for S, N, C in ((1, 5, 10), (3, 37, 10), (30, 11, 16), (4, 9, 1)):
        lg = (rng.standard_normal((S, N, C)) * 4).astype(F)
        lp, p, ent, eH = oracle_predictive([R.log_softmax(lg[s]) for s in range(S)])     # float64 log-softmax rows of the fp32 logits
        ref = P.predict64(lg)
        for k, want in (("log_probs", lp), ("probs", p), ("entropy", ent), ("expected_entropy", eH), ("mutual_info", ent - eH)):
            assert np.abs(ref[k] - want).max() <= 1e-12, (k, np.abs(ref[k] - want).max())


def test_targets_are_clamped():
    op = P.extreme_set("target_high", 10)
    lg = P.stacked_logits(op)
    assert (op["target"] >= 10).any()
    a, b = P.predict64(lg, op["target"]), P.predict64(lg, np.clip(op["target"], 0, 9))
    for k in ("nlp_t", "nll_t", "sum_hits"):
        assert np.array_equal(a[k], b[k])


def tied(op, a, b):
    lg = P.stacked_logits(op)
    got = P.predict32(lg, op["target"])
    L = got["states"][-1][:, :op["C"]]
    assert np.array_equal(L[:, a].view(np.uint32), L[:, b].view(np.uint32)), "L of the tied classes differs in bits"
    lp = got["log_probs"]
    assert np.array_equal(lp[:, a].view(np.uint32), lp[:, b].view(np.uint32))
    if a != b:
        others = np.delete(lp, [a, b], axis=1)
        assert others.size == 0 or (others.max(1) < lp[:, a]).all(), "the tied classes are the maximum of the average"
    assert (got["pred"] == min(a, b)).all()
    return lg


@pytest.mark.parametrize("kind", P.TIE_KINDS)
@pytest.mark.parametrize("C", P.EXTREME_CLASSES)
def test_every_draw_tied_is_an_exact_tie_of_the_average(kind, C):
    a, b = (min(int(k), C - 1) for k in kind.split("_")[1:])
    lg = tied(P.extreme_set(kind, C), a, b)
    assert C == 1 or len({lg[s].tobytes() for s in range(lg.shape[0])}) == lg.shape[0], "the draws are distinct"


@pytest.mark.parametrize("a,b", P.TIE_PAIRS)
def test_swapped_draws_are_an_exact_tie_of_the_average(a, b):
    op = P.swapped_tie_set(a, b)
    lg = tied(op, a, b)
    assert (lg[0, :, a] > lg[0, :, b]).all() and (lg[1, :, a] < lg[1, :, b]).all()     # no draw ties them by itself


def test_the_underflow_sets_underflow():
    """Some draw has exp(o) == 0 in fp32 where the averaged log-probability is finite: what the online logsumexp is for."""
    for op in (P.rotating_peak_set(), P.extreme_set("peak120", 10), P.extreme_set("target100", 10)):
        lg = P.stacked_logits(op)
        ref = P.predict64(lg, op["target"])
        o32 = ref["o"].astype(F)
        assert (np.exp(o32.astype(np.float64)).astype(F) == 0).any()
        assert np.isfinite(ref["log_probs"]).all()
    ref = P.predict64(P.stacked_logits(P.rotating_peak_set()))
    lp = ref["log_probs"]
    peaked = np.zeros(lp.shape, bool)
    for s in range(3):
        peaked[np.arange(19), (np.arange(19) + 3 * s) % 10] = True
    assert (np.abs(lp[peaked] + np.log(3)) <= 1e-6).all()
    assert (np.abs(lp[~peaked] + 120) <= 10).all() and (ref["probs"][~peaked] < P.TINY).all()
