"""CPU checks of tests/_head_np.py, the float64 reference the GPU tests of the classifier head compare against: it is held to the
oracle (the C restatement of the reference's modules) at the shapes of tests/test_head_gpu.py that the oracle can run -- targets
in range, dense operands --, its tie rule is checked on constructed ties, and the derived bound of the row arithmetic
(_head_np's module docstring) is re-measured on every input set the GPU tests use. No device, no vbnn_amd."""
import numpy as np
import pytest

from oracle import vbnn_oracle as vo
from tests import _head_np as R

F = np.float32
SHAPES = [(1, 1, 1), (17, 70, 10), (37, 70, 12), (65, 64, 16), (64, 72, 13), (33, 130, 1), (47, 31, 7)]


def _u(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("N,H,C", SHAPES)
def test_reference_matches_the_oracle_exactly_on_integer_operands(N, H, C):
    """Integer operands: every sum is exact in float32, so the oracle's float32 modules and the float64 reference agree bit
    for bit wherever no exp is on the way."""
    o = R.int_operands(N, H, C, 40 + N)
    inv = F(1.0) / F(N)
    fw = R.head_forward(o["h"], o["w3"], o["bias"], o["target"], inv)
    lg = vo.linear_forward(o["h"], o["w3"], o["bias"])
    assert (_u(lg) == _u(fw["logits"])).all()
    bw = R.head_backward(o["h"], o["w3"], o["g"], "f32", relu_mask=1, r=o["r"])
    gx = vo.linear_grad_input(o["g"], o["w3"])
    want = vo.relu_backward(o["h"], gx)
    assert (_u(want) == _u(bw["g_prev"])).all()
    assert (_u(want * o["r"]) == _u(bw["gv_prev"])).all()
    nomask = R.head_backward(o["h"], o["w3"], o["g"], "f32", relu_mask=0)
    assert (_u(gx) == _u(nomask["g_prev"])).all()
    base = dict(gradWeight=np.full((C, H), 3, F), gradBias=np.full(C, -2, F))
    gw, gb = base["gradWeight"].copy(), base["gradBias"].copy()
    vo.acc_grad_parameters(o["h"], o["g"], None, 1.0, gw, gb, None)
    acc = R.head_backward(o["h"], o["w3"], o["g"], "f32", base=base)
    assert (_u(gw) == _u(acc["gradWeight"])).all() and (_u(gb) == _u(acc["gradBias"])).all()
    assert (_u(gb - base["gradBias"]) == _u(R.acc_grad_bias(o["g"], 1.0)[0])).all()
    assert (_u(want.sum(axis=0)) == _u(bw["gradBias_prev"])).all()
    # the criterion: the oracle's float32 modules inside the derived bound of the reference, the loss and the hits as they are
    out = vo.logsoftmax_forward(lg)
    b_out, b_g, b_loss = R.row_bounds(lg, o["target"], inv)
    assert (np.abs(out - fw["out"]) <= b_out).all()
    g = vo.logsoftmax_backward(out, vo.nll_backward(o["target"], N, C))
    assert (_u(vo.nll_backward(o["target"], N, C)) == _u(R.nll_backward(o["target"], N, C, inv))).all()
    assert (np.abs(g - fw["g_logits"]) <= b_g + 4 * R.ULP * np.abs(fw["g_logits"])).all()      # + the oracle's own expf(out) sum form
    assert abs(vo.nll_forward(out, o["target"]) - fw["loss"]) <= b_loss + 2 * R.U32 * abs(fw["loss"])   # its 1 / N is a double's
    loss, hits = R.nll_forward(out, o["target"], inv)
    assert abs(vo.nll_forward(out, o["target"]) - loss) <= 2 * R.U32 * abs(loss) + 1e-12
    assert vo.get_accuracy(out, o["target"]) == 100.0 * hits / N
    assert vo.get_accuracy(lg, o["target"]) == 100.0 * fw["hits"] / N
    gx2 = vo.logsoftmax_backward(out, o["g"])
    want2 = R.logsoftmax_backward(out, o["g"])
    s = np.abs(o["g"].astype(np.float64).sum(axis=1, keepdims=True))
    assert (np.abs(gx2 - want2) <= 4 * R.ULP * (np.abs(o["g"]) + np.exp(out.astype(np.float64)) * s) + 1e-30).all()


@pytest.mark.parametrize("N,H,C", [(37, 70, 10), (65, 64, 16)])
def test_reference_matches_the_oracle_on_real_operands(N, H, C):
    """Random real operands, with the element-wise bounds the GPU tests use for the same sums."""
    o = R.real_operands(N, H, C, 9, "f32")
    fw = R.head_forward(o["h"], o["w3"], o["bias"], o["target"], F(1.0 / N))
    lg = vo.linear_forward(o["h"], o["w3"], o["bias"])
    assert (np.abs(lg - fw["logits"]) <= 4e-6 * (np.abs(o["h"]) @ np.abs(o["w3"]).T + np.abs(o["bias"])) + 1e-6).all()
    bw = R.head_backward(o["h"], o["w3"], o["g"], "f32", relu_mask=1, r=o["r"])
    gx = vo.relu_backward(o["h"], vo.linear_grad_input(o["g"], o["w3"]))
    assert (np.abs(gx - bw["g_prev"]) <= 2e-6 * bw["g_prev_abs"]).all()
    gw, gb = np.zeros((C, H), F), np.zeros(C, F)
    vo.acc_grad_parameters(o["h"], o["g"], None, 1.0, gw, gb, None)
    assert (np.abs(gw - bw["gradWeight"]) <= 2e-6 * bw["gradWeight_abs"]).all()
    assert (np.abs(gb - bw["gradBias"]) <= 2e-6 * bw["gradBias_abs"]).all()


def test_relu_reference_is_the_oracle_bit_for_bit():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(1000).astype(F)
    x[:6] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45]
    g = rng.standard_normal(1000).astype(F)
    assert (_u(vo.relu_forward(x)) == _u(R.relu_forward(x))).all()
    assert (_u(vo.relu_backward(x, g)) == _u(R.relu_backward(x, g))).all()
    assert _u(R.relu_forward(x))[1] == 0 and _u(R.relu_forward(x))[2] == 0          # -0.0 and a NaN give +0


def test_first_maximum_wins_on_constructed_ties():
    lg = np.array([[5, 5, 1, 0], [0, 5, 1, 5], [2, 2, 2, 2], [1, 0, 3, 3]], F)
    assert list(R.first_max(lg)) == [0, 1, 0, 2]
    for t, hits in (([0, 1, 0, 2], 4), ([1, 3, 3, 3], 0)):
        t = np.array(t, np.int32)
        assert R.criterion(lg, t, F(0.25))["hits"] == hits
        assert vo.get_accuracy(lg, t) == 25.0 * hits
    for kind in ("all_equal", "tie_3_4", "tie_7_8", "tie_0_15"):
        lg, bias, target = R.extreme_logits(kind, 16, 16)
        a = 0 if kind == "all_equal" else int(kind.split("_")[1])
        assert (R.first_max(lg + bias) == a).all()
        assert R.criterion(lg + bias, target, F(1 / 16))["hits"] == int((np.clip(target, 0, 15) == a).sum())
        assert vo.get_accuracy(lg + bias, target) == 100.0 * int((target == a).sum()) / 16
    nan = np.array([[np.nan, 1, 2], [0, 1, 2]], F)
    assert list(R.first_max(nan)) == [-1, 2] and R.criterion(nan, np.array([0, 2], np.int32), F(0.5))["hits"] == 1


def test_targets_are_clamped_for_loss_gradient_and_hits():
    lg = np.array([[3, 0, 0], [0, 0, 3]], F)
    a = R.criterion(lg, np.array([-4, 9], np.int32), F(0.5))
    b = R.criterion(lg, np.array([0, 2], np.int32), F(0.5))
    assert a["loss"] == b["loss"] and a["hits"] == b["hits"] == 2 and (a["g_logits"] == b["g_logits"]).all()
    assert (R.nll_backward(np.array([-4, 9], np.int32), 2, 3, F(0.5)) == R.nll_backward(np.array([0, 2], np.int32), 2, 3, F(0.5))).all()


def test_slot_sum_is_in_order_float32():
    s = np.zeros((3, 1, 16), F)
    s[:, 0, 0] = [2.0 ** 24, 1.0, -2.0 ** 24]                    # in order: (2^24 + 1) rounds to 2^24, then 0; any other order: 1
    assert R.slot_logits(s, None)[0, 0] == 0.0
    assert R.slot_logits(s, np.array([0.5], F))[0, 0] == 0.5


def test_row_arithmetic_stays_inside_the_derived_bound():
    """The float32 restatement of the row arithmetic on every input set of the GPU tests, extremes included: inside the derived
    bound, and using no more of it than _head_np.ROW_BOUND_USED records (the device is held to the bound itself)."""
    used = {"out": 0.0, "g_logits": 0.0, "loss": 0.0}
    n_sets = 0
    for name, lg, target, inv_n, rpd in R.row_sets():
        ref = R.criterion(lg, target, inv_n, rpd)
        b_out, b_g, b_loss = R.row_bounds(lg, target, inv_n, rpd)
        o, g, loss = R.row_arith_f32(lg, target, inv_n, rpd)
        f = {"out": float((np.abs(o - ref["out"]) / b_out).max()), "g_logits": float((np.abs(g - ref["g_logits"]) / b_g).max()),
             "loss": abs(loss - ref["loss"]) / b_loss}
        for k in used:
            assert f[k] <= 1.0, f"{name}: {k} uses {f[k]:.3f} of its bound"
            used[k] = max(used[k], f[k])
        n_sets += 1
    print("fractions of the row-arithmetic bound used:", {k: round(v, 3) for k, v in used.items()}, "over", n_sets, "sets")
    for k in used:
        assert used[k] <= R.ROW_BOUND_USED[k] + 0.02, f"{k}: {used[k]:.3f} measured, {R.ROW_BOUND_USED[k]} recorded"
        assert used[k] >= 0.5 * R.ROW_BOUND_USED[k], f"{k}: the recorded {R.ROW_BOUND_USED[k]} is stale ({used[k]:.3f} measured)"
