"""NumPy restatements for the tests of the posterior-predictive head (vbnn_head_predict, include/vbnn_hip.h): the float64
reference predict64, an fp32 restatement of the kernel's update (predict32), the bounds the outputs and the ACCUMULATE state are
held to, the input sets the CPU and the GPU tests share, and check_predict / check_states, which print err / tol ratios as
tests/_classes_np.check_classes does. NumPy only; nothing here reads GPU code or a GPU tensor. tests/test_predict_ref.py holds it
on the CPU, tests/test_head_predict_gpu.py holds k_head_predict to it through the C ABI.

The definitions are those of tests/_classes_np.classes64 (vbnn_predict_class_moments states the same predictive for any class
count); targets are clamped to [0, C - 1] with tests/_head_np.clamp_targets, as the header says.

The bounds -- _classes_np's, plus one derived term
--------------------------------------------------
_classes_np.logp_tol / probs_tol / entropy_tol / expected_entropy_tol are written for this sequence of operations (per draw a
log-softmax, the online logsumexp per class, fp32 row sums of exp(o) o, the finish L - log S). Two differences of this kernel
are inside them as they stand: the row sums run over lane groups of four classes and two shuffle steps instead of one column
after the other -- C - 1 additions of relative eps in any order, which the (C + 16) eps terms hold --, and log1p is the
library's log1pf (1 ulp by the HIP math API table) where _classes_np allows its own form 3 ulp.
One term is missing. _classes_np bounds a draw's o[c] = y[c] - lse by (C + 16) eps max(|o[c]|, 1): relative to o, with no
term for the MAGNITUDE of the logits. The kernel forms lse = mx + logf(se) and rounds it to fp32 once: an error of up to
u |lse| (u = 2^-24), the `u |lse|` of _head_np's B_lse, common to every class of the row in that draw. At the logits of
_classes_np's own cases it is small beside (C + 16) eps; under a bias of +-30000 (an input set here) |lse| ~ 30005, and
u |lse| = 1.8e-3 where (C + 16) eps max(|o|, 1) ~ 1e-5. So, with d_s = u |lse_s| of draw s of the row (lse_term):
  * o_s[c] carries d_s on top of its _classes_np bound;
  * L[c] = logsumexp_s o_s[c] has partial derivatives (the draws' weights) that are positive and sum to 1, so shifts of at most
    d_s move it by at most max_s d_s: logp_tol gains max_s d_s, and so does each state row's L after its draws;
  * p = exp(log p) moves by p expm1(max_s d_s): probs_tol gains that;
  * the entropy -sum_c p log p moves by sum_c p (1 + |log p|) times the shift of log p, the form entropy_tol already carries
    logp_tol through: it gains sum_c p (1 + |log p|) max_s d_s;
  * H(p_s) = -sum_c exp(o) o likewise gains sum_c exp(o_s) (1 + |o_s|) d_s per draw; expected_entropy_tol gains their mean,
    the state's sum H their sum;
  * -o_s[t] gains d_s per draw: the state's sum -o[t] and totals[2] gain sum_s d_s.
Nothing else is added and no constant is chosen: predict32 is measured against these bounds on every input set below
(BOUND_USED), the device's own ratios are printed by the GPU tests."""
import numpy as np

from tests import _classes_np as K
from tests import _head_np as R

F = np.float32
EPS = K.EPS
U32 = R.U32
TINY = K.TINY
# the largest share of each bound that predict32 uses over every input set below (input_sets: extremes, underflow, ties and the
# 8209-row set included), measured 2026-10-21 by test_predict_ref.py::test_predict32_stays_inside_the_bounds_on_every_input_set
BOUND_USED = {"log_probs": 0.533, "probs": 0.533, "entropy": 0.520, "expected_entropy": 0.556, "mutual_info": 0.056,
              "state_L": 0.544, "state_sum_H": 0.556, "state_sum_nll": 0.544, "totals0": 0.091, "totals2": 0.070}


# ------------------------------------------------------------------------------------------------ the float64 reference
def predict64(lg, t=None):
    """The float64 definition of the header's section on the predictive head, on exact fp32 logits lg (S x R x C, bias included):
    _classes_np.classes64 on the clamped targets, plus what the ACCUMULATE state holds after each draw -- L (S x R x C: the
    logsumexp of the draws so far), sum_H, and with t sum_nll and sum_hits (S x R each; first maximum wins)."""
    lg = np.asarray(lg, F)
    S, N, C = lg.shape
    tc = None if t is None else R.clamp_targets(t, C, N)
    ref = K.classes64(lg, tc)
    ref["t"] = tc
    ref["L"] = np.logaddexp.accumulate(ref["o"], axis=0)
    ref["sum_H"] = np.cumsum(ref["H"], axis=0)
    if tc is not None:
        ref["hit"] = lg.argmax(2) == tc[None]
        ref["sum_nll"] = np.cumsum(ref["nll_t"], axis=0)
        ref["sum_hits"] = np.cumsum(ref["hit"], axis=0)
    return ref


# ------------------------------------------------------------------------------------------------ the kernel's update in fp32
def _f64(x):
    return np.asarray(x, F).astype(np.float64)


def _exp32(x):
    return np.exp(_f64(x)).astype(F)


def _log32(x):
    return np.log(_f64(x)).astype(F)


def _log1p32(x):
    return np.log1p(_f64(x)).astype(F)


def _lanes(groups):
    """The two shuffle steps over a row's four lane groups (groups without a class hold 0, and adding 0 is exact)."""
    while len(groups) > 1:
        groups = [(groups[i] + groups[i + 1]).astype(F) if i + 1 < len(groups) else groups[i] for i in range(0, len(groups), 2)]
    return groups[0]


def _lane_sum(e):
    """The fp32 row sum of e (N x C) in _head_np.row_arith_f32's order: lane groups of four classes in order, then the shuffles."""
    N, C = e.shape
    groups = []
    for q in range(0, C, 4):
        s = np.zeros(N, F)
        for c in range(q, min(q + 4, C)):
            s = (s + e[:, c]).astype(F)
        groups.append(s)
    return _lanes(groups)


def _lane_entropy(o):
    """-sum_c exp(o) o in the same order, each term folded in by one fused multiply-add (the product of two fp32 values is
    exact in float64)."""
    N, C = o.shape
    groups = []
    for q in range(0, C, 4):
        e = np.zeros(N, F)
        for c in range(q, min(q + 4, C)):
            e = (_f64(_exp32(o[:, c])) * _f64(o[:, c]) + _f64(e)).astype(F)
        groups.append(e)
    return -_lanes(groups)


def predict32(lg, t=None):
    """The kernel's update, one fp32 NumPy operation per statement (exp, log and log1p rounded from float64), only to MEASURE
    how much of each bound such arithmetic uses. Returns the outputs, totals (with t), rows (N x 3, the state's row values) and
    states: the state rows, N x (C + 3), after every draw."""
    lg = np.asarray(lg, F)
    S, N, C = lg.shape
    rows = np.arange(N)
    tc = None if t is None else R.clamp_targets(t, C, N)
    L = sH = None
    sNll, sHit = np.zeros(N, F), np.zeros(N, F)
    states = []
    for s in range(S):
        y = lg[s]
        mx = y.max(axis=1)
        arg = y.argmax(axis=1)
        se = _lane_sum(_exp32((y - mx[:, None]).astype(F)))
        lse = (mx + _log32(se)).astype(F)
        o = (y - lse[:, None]).astype(F)
        ent = _lane_entropy(o)
        nll = np.zeros(N, F) if tc is None else -o[rows, tc]
        hit = np.zeros(N, F) if tc is None else (arg == tc).astype(F)
        if s == 0:
            L, sH, sNll, sHit = o, ent, nll, hit
        else:
            m = np.maximum(L, o)
            L = (m + _log1p32(_exp32((np.minimum(L, o) - m).astype(F)))).astype(F)
            sH, sNll, sHit = (sH + ent).astype(F), (sNll + nll).astype(F), (sHit + hit).astype(F)
        states.append(np.concatenate([L, sH[:, None], sNll[:, None], sHit[:, None]], axis=1))
    logS = _log32(F(S))
    lp = (L - logS).astype(F)
    p = _exp32(lp)
    got = dict(log_probs=lp, probs=p, entropy=_lane_entropy(lp), expected_entropy=(sH / F(S)).astype(F), states=states)
    got["mutual_info"] = (got["entropy"] - got["expected_entropy"]).astype(F)
    got["pred"] = lp.argmax(axis=1).astype(np.int32)
    if tc is not None:
        got["totals"] = [float((-lp[rows, tc]).astype(np.float64).sum()), float((got["pred"] == tc).sum()),
                         float(sNll.astype(np.float64).sum()), float(sHit.astype(np.float64).sum())]
        got["rows"] = np.stack([sH, sNll, sHit], axis=1)
    return got


# ------------------------------------------------------------------------------------------------ the bounds
def lse_term(lg):
    """d_s = u |lse_s| (S x R) of the module docstring."""
    y = np.asarray(lg, F).astype(np.float64)
    mx = y.max(2)
    return U32 * np.abs(mx + np.log(np.exp(y - mx[:, :, None]).sum(2)))


def logp_tol(ref, lg):
    return K.logp_tol(ref, lg.shape[0]) + lse_term(lg).max(0)[:, None]


def probs_tol(ref, lg):
    return K.probs_tol(ref, lg.shape[0]) + ref["probs"] * np.expm1(lse_term(lg).max(0))[:, None]


def entropy_tol(ref, lg):
    p, lp = ref["probs"], ref["log_probs"]
    return K.entropy_tol(ref, lg.shape[0]) + (p * (1.0 + np.abs(lp))).sum(1) * lse_term(lg).max(0)


def _draw_entropy_shift(ref, lg):
    o = ref["o"]
    return (np.exp(o) * (1.0 + np.abs(o))).sum(2) * lse_term(lg)             # S x R


def expected_entropy_tol(ref, lg):
    return K.expected_entropy_tol(ref) + _draw_entropy_shift(ref, lg).mean(0)


def sum_nll_tol(ref, lg):
    """Per row, the bound of sum_s -o_s[t] (_classes_np.check_classes' bound of totals[2], row by row) + sum_s d_s."""
    S, N, C = lg.shape
    o_t = ref["nll_t"]
    return ((C + 16) * EPS * np.maximum(o_t, 1.0)).sum(0) + S * EPS * o_t.sum(0) + lse_term(lg).sum(0)


def check_predict(got, lg, t=None, label=""):
    """got: dict of NumPy arrays (any of probs, log_probs, entropy, expected_entropy, mutual_info, pred; with t totals (4) and
    optionally rows, N x 3) against predict64(lg, t) on the exact fp32 logits lg. Bounded by the functions above; the order of
    the classes, the counts and the totals exactly, as _classes_np.check_classes has them. Returns (reference, err / tol ratios)."""
    lg = np.asarray(lg, F)
    S, N, C = lg.shape
    ref = predict64(lg, t)
    rows = np.arange(N)
    tl = logp_tol(ref, lg)
    tols = dict(log_probs=tl, probs=probs_tol(ref, lg), entropy=entropy_tol(ref, lg), expected_entropy=expected_entropy_tol(ref, lg))
    tols["mutual_info"] = tols["entropy"] + tols["expected_entropy"]
    ratios = {}
    for k, tol in tols.items():
        if got.get(k) is not None:
            d = np.abs(got[k].astype(np.float64) - ref[k])
            ratios[k] = float((d / tol).max())
            assert (d <= tol).all(), (label, k, ratios[k])
    lp, p = got.get("log_probs"), got.get("probs")
    if p is not None and lp is not None and got.get("entropy") is not None:
        # the entropy is a sum of C terms: relative (C + 16) eps against the float64 sum of ITS terms, the returned fp32 p, log p
        terms = p.astype(np.float64) * lp.astype(np.float64)
        d, tol = np.abs(got["entropy"] + terms.sum(1)), (C + 16) * EPS * np.abs(terms).sum(1)
        assert (d <= tol).all(), (label, "entropy of the returned terms")
    if got.get("pred") is not None:
        assert (got["pred"] >= 0).all() and (got["pred"] < C).all(), (label, "pred outside [0, C)")
        if lp is not None:
            assert np.array_equal(got["pred"], lp.argmax(1)), (label, "pred is the first maximum of the returned log_probs")
    tot = got.get("totals")
    if t is not None and tot is not None:
        tc = ref["t"]
        assert tot[3] == float(ref["hit"].sum()), (label, "totals[3]", tot[3], float(ref["hit"].sum()))
        if got.get("pred") is not None:
            assert tot[1] == float((got["pred"] == tc).sum()), (label, "totals[1]")
        if lp is not None:               # the double sum of the returned fp32 rows
            want = (-lp[rows, tc]).astype(np.float64).sum()
            assert abs(tot[0] - want) <= 1e-12 * abs(want), (label, "totals[0]", tot[0], want)
        b0, b2 = tl[rows, tc].sum(), sum_nll_tol(ref, lg).sum()
        ratios["totals0"] = float(abs(tot[0] - ref["nlp_t"].sum()) / b0)
        ratios["totals2"] = float(abs(tot[2] - ref["nll_t"].sum()) / b2)
        assert ratios["totals0"] <= 1.0 and ratios["totals2"] <= 1.0, (label, "totals against float64", tot, ratios)
        if got.get("rows") is not None:  # ... and of the state's fp32 row values
            want = got["rows"][:, 1].astype(np.float64).sum()
            assert abs(tot[2] - want) <= 1e-12 * abs(want), (label, "totals[2]", tot[2], want)
            assert tot[3] == float(got["rows"][:, 2].astype(np.float64).sum()), (label, "totals[3] against the state")
    print(f"{label} S {S} R {N} C {C}: err/tol " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return ref, ratios


def check_states(states, lg, t=None, label=""):
    """The state rows (N x (C + 3)) after each draw against predict64 of the draws so far: L and sum H and sum -o[t] inside the
    bounds of those draws (L = log p + log(s + 1) with |L| <= |log p|, so log p's bound holds L; a sum of s + 1 entropies takes
    s + 1 times the bound of their mean), the hits exactly. Returns the err / tol ratios."""
    lg = np.asarray(lg, F)
    S, N, C = lg.shape
    ratios = {"state_L": 0.0, "state_sum_H": 0.0, "state_sum_nll": 0.0}
    for s, st in enumerate(states):
        part = lg[:s + 1]
        ref = predict64(part, t)
        checks = [("state_L", st[:, :C], ref["L"][s], logp_tol(ref, part)),
                  ("state_sum_H", st[:, C], ref["sum_H"][s], (s + 1) * expected_entropy_tol(ref, part))]
        if t is not None:
            checks.append(("state_sum_nll", st[:, C + 1], ref["sum_nll"][s], sum_nll_tol(ref, part)))
            assert np.array_equal(st[:, C + 2], ref["sum_hits"][s].astype(F)), (label, "hits after draw", s)
        else:
            assert (st[:, C + 1:] == 0).all(), (label, "without targets the target's sums stay 0")
        for k, got, want, tol in checks:
            d = np.abs(got.astype(np.float64) - want)
            assert (d <= tol).all(), (label, k, "after draw", s, float((d / tol).max()))
            ratios[k] = max(ratios[k], float((d / tol).max()))
    if t is None:
        del ratios["state_sum_nll"]
    print(f"{label} S {S} R {N} C {C}: err/tol " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return ratios


# ------------------------------------------------------------------------------------------------ input sets (shared by the CPU and the GPU tests)
def stacked_logits(op):
    """The exact fp32 logits (S x R x C, bias included) of an operand set whose sums are exact (integer operands)."""
    lg = op["h"].astype(np.float64) @ op["w3"].astype(np.float64).T + (0 if op["bias"] is None else op["bias"])
    return lg.astype(F).reshape(op["S"], op["R"], op["C"])


def _set(h, w3, bias, target, S, N, C):
    return dict(h=h, w3=w3, bias=bias, target=target, S=S, R=N, C=C, H=h.shape[1])


def class_count_set(C, N=17, S=3, H=70):
    o = R.int_operands(S * N, H, C, 300 + C)
    return _set(o["h"], o["w3"], o["bias"], o["target"][:N], S, N, C)


def from_logits(lg, bias, target):
    """Integer logits lg (S x R x C, without the bias) as operands: _head_np.logit_operands on the stacked rows."""
    S, N, C = lg.shape
    h, w3 = R.logit_operands(lg.reshape(S * N, C))
    return _set(h, w3, bias, target, S, N, C)


def extreme_set(kind, C, N=19, S=3):
    """One of _head_np.EXTREME_KINDS per draw (draw s from seed 11 + s; bias and targets are draw 0's)."""
    draws = [R.extreme_logits(kind, N, C, seed=11 + s) for s in range(S)]
    return from_logits(np.stack([d[0] for d in draws]), draws[0][1], draws[0][2])


def rotating_peak_set(N=19, C=10, S=3):
    """Each draw peaks 120 above the rest at a different class of the row: (r + 3 s) mod C."""
    rng = np.random.default_rng(23)
    lg = rng.integers(-3, 4, (S, N, C)).astype(F)
    for s in range(S):
        lg[s, np.arange(N), (np.arange(N) + 3 * s) % C] += 120
    return from_logits(lg, np.zeros(C, F), rng.integers(0, C, N).astype(np.int32))


def swapped_tie_set(a, b, N=19, C=16):
    """Two draws with classes a and b swapped (5 and 3; every other class 200 below, where its exp is 0 in fp32 and in the sum):
    the two draws' lse have equal bits, so the averaged probabilities of a and b tie exactly."""
    rng = np.random.default_rng(29)
    lg = np.repeat((rng.integers(-3, 4, (1, N, C)) - 200).astype(F), 2, axis=0)
    lg[0, :, a], lg[0, :, b] = 5, 3
    lg[1, :, a], lg[1, :, b] = 3, 5
    target = np.array([(a, b, (a + 1) % C, 0)[n % 4] for n in range(N)], np.int32)
    return from_logits(lg, np.zeros(C, F), target)


def real_set(S, N, H, C, seed, dtype, scale=1.0):
    """Random real operands, distinct per draw; scale (a power of two) widens the logits' spread exactly."""
    o = R.real_operands(S * N, H, C, seed, dtype)
    return _set(o["h"], (o["w3"] * F(scale)).astype(F), o["bias"], o["target"][:N], S, N, C)


def identical_draws_set(S=5, N=37, H=70, C=10, dtype="f32"):
    o = real_set(1, N, H, C, 41, dtype)
    return dict(o, h=np.tile(o["h"], (S, 1)), S=S)


def many_workgroups_set():
    """16 x 512 + 17 rows: 514 workgroups, so the totals finish (512 threads) goes round a second time."""
    N = 16 * 512 + 17
    o = R.int_operands(N, 32, 10, 77)
    return _set(o["h"], o["w3"], o["bias"], o["target"], 1, N, 10)


TIE_KINDS = ("tie_3_4", "tie_7_8", "tie_0_15")
TIE_PAIRS = ((3, 4), (7, 8), (0, 15))
EXTREME_CLASSES = (1, 10, 16)
FORM_S = (1, 2, 3, 7)
FORM_R = (1, 16, 17, 47)


def input_sets():
    """(name, exact fp32 logits S x R x C with the bias, targets) of every set the GPU tests hold to the bounds. For the real
    operand sets the logits are rounded from float64: the CPU's stand-in for the device's own logits, which the GPU tests use."""
    rounded_logits = stacked_logits
    for C in range(1, 17):
        op = class_count_set(C)
        yield f"int C{C}", stacked_logits(op), op["target"]
    for kind in R.EXTREME_KINDS:
        for C in EXTREME_CLASSES:
            op = extreme_set(kind, C)
            yield f"{kind} C{C}", stacked_logits(op), op["target"]
    op = rotating_peak_set()
    yield "rotating peaks", stacked_logits(op), op["target"]
    for a, b in TIE_PAIRS:
        op = swapped_tie_set(a, b)
        yield f"swapped tie {a} {b}", stacked_logits(op), op["target"]
    for S in FORM_S:
        for N in FORM_R:
            op = real_set(S, N, 70, 10, 50 + S, "f32")
            yield f"real S{S} R{N}", rounded_logits(op), op["target"]
    op = real_set(3, 37, 70, 10, 43, "f32", scale=8.0)
    yield "real spread x8", rounded_logits(op), op["target"]
    op = identical_draws_set()
    yield "identical draws", rounded_logits(op), op["target"]
    op = many_workgroups_set()
    yield "514 workgroups", stacked_logits(op), op["target"]
