"""CPU tests of the Bernoulli head's restatements (tests/_labels_np.py): the float64 reference against
torch.nn.functional.binary_cross_entropy_with_logits in float64 (loss and autograd gradient) and against a plain float64
composition of the predictive; the fp32 op-by-op restatement inside the DERIVED bounds (the share of each bound in use is
printed); the clamp floor, S = 1, and the tie rule."""
import os

import numpy as np
import pytest
import torch

from tests import _labels_np as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def the_header_states_what_the_restatement_follows():
    """The restatement follows include/vbnn_hip.h operation by operation: the lines it restates have to be there."""
    hdr = " ".join(open(os.path.join(ROOT, "include", "vbnn_hip.h")).read().split())
    for line in ("u = expf(-|z|); w = 1 + u; l1p = (logf(w) * u) / (w - 1) (u itself where w == 1)",
                 "e = (fmaxf(z, 0) - z * t) + l1p", "sig = z >= 0 ? 1 / w : u / w;",
                 "zc = min(max(z, -80), 80) (a NaN z stays NaN)", "p = zc >= 0 ? 1 / w : u / w; q = zc >= 0 ? u / w : 1 / w",
                 "lp = fminf(zc, 0) - l1p; ln = fminf(-zc, 0) - l1p", "P = P + p; Q = Q + q; Hs = Hs + -(p * lp + q * ln)",
                 "the label is predicted 1 iff P > Q (a tie predicts 0)", "stored as +0 when S = 1"):
        assert line in hdr, line
    assert f"#define VBNN_LABEL_MOMENTS_STACKED_MAX_D {4096}" in hdr


def normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def labels(shape, seed, soft=False):
    rng = np.random.default_rng(seed)
    return rng.random(shape).astype(np.float32) if soft else (rng.random(shape) < 0.4).astype(np.float32)


@pytest.mark.parametrize("N,D,scale,soft", [(1, 1, 1.0, False), (3, 5, 4.0, False), (37, 70, 12.0, True), (9, 257, 30.0, False)])
def test_criterion64_is_torch_bce_with_logits(N, D, scale, soft):
    z = (np.float32(scale) * normal((N, D), 5)).astype(np.float32)
    t = labels((N, D), 6, soft)
    inv_nd = float(np.float32(1.0 / (N * D)))
    ref = B.criterion64(z, t, inv_nd)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.tensor(t, dtype=torch.float64), reduction="sum") * inv_nd
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-13 * ref["loss_mag"]
    assert (np.abs(ref["g"] - zt.grad.numpy()) <= 1e-13 * ref["g_mag"]).all()
    assert ref["hits"] == int(((z > 0) == (t > 0.5)).sum())


@pytest.mark.parametrize("N,D,scale,soft", [(1, 1, 1.0, False), (3, 5, 4.0, True), (37, 70, 12.0, False), (9, 257, 30.0, True)])
def test_criterion32_is_inside_the_derived_bounds(N, D, scale, soft):
    z = (np.float32(scale) * normal((N, D), 7)).astype(np.float32)
    z.flat[:6] = np.array([80.0, -80.0, 100.0, -100.0, 1e4, -1e4], np.float32)[:z.size]
    t = labels((N, D), 8, soft)
    inv_nd = float(np.float32(1.0 / (N * D)))
    got = B.criterion32(z, t, inv_nd)
    assert np.isfinite(got["loss"]) and np.isfinite(got["g"]).all()
    B.check_criterion(got["loss"], got["g"], got["hits"], z, t, inv_nd, label=f"criterion32 {N}x{D} x{scale:g}")


def test_criterion32_exact_cases_and_nan():
    z = np.zeros((2, 3), np.float32)
    t = np.full((2, 3), 0.5, np.float32)
    got = B.criterion32(z, t, 1.0 / 6)
    assert not got["g"].view(np.uint32).any()                       # sig = t = 1/2: g = +0 bitwise
    assert got["hits"] == 6                                         # (0 > 0) == (0.5 > 0.5)
    z[1, 2] = np.nan
    bad = B.criterion32(z, t, 1.0 / 6)
    assert np.isnan(bad["loss"]) and np.isnan(bad["g"][1, 2]) and bad["hits"] == 5
    assert not bad["g"].view(np.uint32)[[0, 0, 0, 1, 1], [0, 1, 2, 0, 1]].any()
    B.check_criterion(bad["loss"], bad["g"], bad["hits"], z, t, 1.0 / 6, label="nan")


def _torch_predictive(y, t):
    """A plain float64 composition: sigmoid, logsigmoid, means and entropies by torch."""
    z = torch.tensor(y, dtype=torch.float64).clamp(-80.0, 80.0)
    S = z.shape[0]
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    lp, ln = torch.nn.functional.logsigmoid(z), torch.nn.functional.logsigmoid(-z)
    pm, qm = p.mean(0), q.mean(0)
    ent = -(pm * pm.log() + qm * qm.log())
    ee = (-(p * lp + q * ln)).mean(0)
    tt = torch.tensor(t, dtype=torch.float64)
    a = (tt * lp + (1 - tt) * ln).sum(2)
    return dict(probs=pm, entropy=ent, mutual_info=ent - ee, row_log_lik=torch.logsumexp(a, 0) - np.log(S),
                row_marg_log_lik=(tt * pm.log() + (1 - tt) * qm.log()).sum(1), a=a)


SHAPES = [(1, 1, 1), (2, 3, 5), (3, 5, 63), (7, 3, 257), (2, 2, 1027)]


@pytest.mark.parametrize("S,R,D", SHAPES)
def test_label_moments64_is_the_plain_composition(S, R, D):
    y = (np.float32(3.0) * normal((S, R, D), 11)).astype(np.float32)
    t = labels((R, D), 12)
    ref, tp = B.label_moments64(y, t), _torch_predictive(y, t)
    for k in ("probs", "entropy", "row_log_lik", "row_marg_log_lik", "a"):
        want = tp[k].numpy()
        assert (np.abs(ref[k] - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)).all(), k
    if S > 1:
        assert (np.abs(ref["mutual_info"] - tp["mutual_info"].numpy()) <= 1e-12).all()
        assert (ref["mutual_info"] >= -1e-12).all()                  # Jensen: the entropy of the mean is not below the mean entropy
    assert ref["totals"][2] == -ref["a"].sum() and ref["totals"][3] == ref["hit"].sum()


@pytest.mark.parametrize("S,R,D", SHAPES + [(30, 2, 260)])
def test_label_moments32_is_inside_the_derived_bounds(S, R, D):
    y = (np.float32(3.0) * normal((S, R, D), 13)).astype(np.float32)
    y.flat[:6] = np.array([80.0, -80.0, 100.0, -100.0, 1e4, -1e4], np.float32)[:y.size]
    t = labels((R, D), 14)
    got = B.label_moments32(y, t)
    B.check_label_moments(got, y, t, label="label_moments32")
    bare = B.label_moments32(y, None)
    assert set(bare) == {"probs", "entropy", "mutual_info", "row_entropy", "row_mutual_info", "P", "Q"}
    for k in bare:
        assert np.array_equal(bare[k], got[k]), k


def test_the_clamp_floors_every_probability():
    """Logits far outside the clamp: p and q of every draw are at least e^-80, every log of an average is finite, and the values
    are those of logits of exactly +-80."""
    y = np.array([[[1e4, -1e4, 100.0, -100.0, 80.0, -80.0]]] * 3, np.float32)
    t = np.array([[0, 1, 1, 0, 1, 0]], np.float32)
    got = B.label_moments32(y, t)
    floor = float(np.exp(-80.0))
    assert (got["probs"] >= 0.99 * floor).all() and (got["probs"] <= 1.0).all()
    for k in ("entropy", "mutual_info", "row_log_lik", "row_marg_log_lik", "row_entropy"):
        assert np.isfinite(got[k]).all(), k
    same = B.label_moments32(np.sign(y) * np.float32(80.0), t)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(same[k])), k
    ref = B.label_moments64(y, t)
    assert np.isfinite(ref["log_p"]).all() and np.isfinite(ref["log_q"]).all()
    assert abs(ref["row_marg_log_lik"][0] - (-80.0 * 2)) < 1e-6       # the first two labels contradict a saturated logit: -80 each


def test_one_draw_has_exactly_no_mutual_information():
    y = normal((1, 4, 9), 15)
    got = B.label_moments32(y, labels((4, 9), 16))
    assert not got["mutual_info"].view(np.uint32).any() and not got["row_mutual_info"].view(np.uint32).any()
    assert (B.label_moments64(y)["mutual_info"] == 0).all()


def test_a_tie_predicts_zero():
    """P == Q bitwise (z = 0 in every draw; z = +a and -a in two draws): the label is predicted 0, a hit only for t <= 1/2."""
    y = np.array([[[0.0, 0.0, 1.5, 1.5]], [[0.0, 0.0, -1.5, -1.5]]], np.float32)
    t = np.array([[0, 1, 0, 1]], np.float32)
    got = B.label_moments32(y, t)
    assert np.array_equal(got["P"], got["Q"])
    assert got["row_hits"][0] == 2 and got["totals"][3] == 2.0 and got["totals"][4] == 0.0
    ref = B.label_moments64(y, t)
    assert not ref["pred"].any() and ref["row_hits"][0] == 2
    assert (B.tie_margin(ref, 2) == 0).all()
