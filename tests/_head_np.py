"""NumPy float64 reference of the classification loss path: the classifier head (final Linear + LogSoftMax + ClassNLL, forward,
from slots, backward), the fused and the separate criterion, ReLU and the bias-gradient column sum. NumPy only; no code is shared
with vbnn_amd/ and nothing here reads GPU code or a GPU tensor. tests/test_head_ref.py holds it to the oracle,
tests/test_head_gpu.py holds every form of head.hip and the small kernels of elementwise.hip to it.

Operands arrive as float32 arrays whose values the operand type holds exactly (bf16 operands widened exactly: round them with
bf16_round first); every product and sum below is float64.

The bound for the row arithmetic (row_bounds) -- derived, not chosen
--------------------------------------------------------------------
The four kernels that hold the row arithmetic (head_rows_from_logits, k_head_step_f32, k_logsoftmax_nll, k_nll_forward's
input) compute, per row of C float32 logits lg[c], in float32:
    mx = max lg;  d[c] = lg[c] - mx;  e[c] = expf(d[c]);  se = sum_c e[c];  lse = mx + logf(se);  o[c] = lg[c] - lse;
    p[c] = expf(o[c]);  g[c] = (p[c] - [c == t]) * inv_n
With u = 2^-24 (half an ulp, relative: every float32 add, subtract or multiply errs by at most u times its result) and
ulp = 2^-23, against the exact values of the same float32 logits:
  * expf and logf are within 1 ulp (HIP math API accuracy table); one more ulp is allowed for the reference's own rounding: the
    E_ULP = 2 convention of test_update_gpu.py. So e[c] errs by E_ULP ulp relative -- plus, where the true value is below
    the smallest normal float32 TINY = 2^-126, an absolute TINY: whether expf returns a subnormal is not part of the contract.
  * d[c] errs by u |d[c]|, which moves e[c] by the relative u |d[c]|; e |d| <= 1/e for d <= 0 and se >= 1 (the maximum's own
    term is exactly 1), so all C - 1 such terms together move se by at most (C - 1) u / e, relative.
  * the sum of C positive terms is C - 1 additions of at most u each, relative to se, in any order (the kernels' orders differ:
    lane groups of four, then two shuffles; k_logsoftmax_nll sums in double, which is inside this too).
  * so se errs relatively, and log(se) absolutely, by  E_ULP ulp + (C - 1) u (1 + 1/e) + C TINY;  logf adds E_ULP ulp of
    |log se| (0 <= log se <= log C).
  * lse = mx + logf(se) adds u |lse|  (|lse| <= |mx| + log C);  o = lg - lse adds u |o|.
  per row:      B_lse      = E_ULP ulp (1 + log se) + (C - 1) u (1 + 1/e) + C TINY + u |lse|
  per element:  B_out[c]   = B_lse + u |o[c]|                (|o[c]| <= mx - min lg + log C: a per-row bound with the row's spread)
  * p = expf(o) errs by p (exp(B_out) - 1) from its argument and E_ULP ulp of p from expf (absolute TINY when p < TINY); the
    subtraction and the product by inv_n cost u each of |p - [c == t]|:
  per element:  B_g[c]     = inv_n (p (expm1(B_out[c]) + E_ULP ulp) + 2 u |p - [c == t]|) + TINY inv_n
  the loss (a double sum of double products of o[t] and inv_n):  B_loss = inv_n sum_n B_out[n][t_n] + 1e-12 sum_n |o[t_n]| inv_n.
The logits themselves are exact in every case that uses these bounds (integer operands), or the bound is applied to the
device's own logits. row_arith_f32 restates the arithmetic above in float32 NumPy (exp and log rounded from float64) only to
MEASURE how much of the bound such arithmetic uses: test_head_ref.py re-measures it on every input set of the GPU tests."""
import math

import numpy as np

from tests._update_np import bf16_bits, bf16_round, bf16_to_f32  # noqa: F401  (formats only)

F = np.float32
U32 = 2.0 ** -24
ULP = 2.0 ** -23
TINY = 2.0 ** -126
E_ULP = 2
# largest fraction of B_out / B_g / B_loss that row_arith_f32 uses over every input set of tests/test_head_gpu.py (extremes
# included), measured 2026-10-19 by test_head_ref.py::test_row_arithmetic_stays_inside_the_derived_bound
ROW_BOUND_USED = {"out": 0.812, "g_logits": 0.743, "loss": 0.120}


def round_t(x, dtype):
    """float -> the operand type's value (float32 array): bf16 round-to-nearest-even, or the float32 itself."""
    x = np.asarray(x, F)
    return bf16_round(x) if dtype == "bf16" else x


def clamp_targets(target, C, N, rows_per_draw=0):
    t = np.asarray(target, np.int64)
    t = t[np.arange(N) % rows_per_draw] if rows_per_draw > 0 else t[:N]
    return np.clip(t, 0, C - 1)


# ------------------------------------------------------------------------------------------------ the criterion rows
def log_softmax(lg):
    lg = np.asarray(lg, np.float64)
    with np.errstate(invalid="ignore"):
        mx = lg.max(axis=1, keepdims=True)
        se = np.exp(lg - mx).sum(axis=1, keepdims=True)
        return lg - (mx + np.log(se))


def first_max(lg):
    """Arg-max with the first maximum winning (Tensor:max); -1 for a row holding a NaN (never a hit)."""
    lg = np.asarray(lg, np.float64)
    arg = np.argmax(np.where(np.isnan(lg), -np.inf, lg), axis=1)
    return np.where(np.isnan(lg).any(axis=1), -1, arg)


def criterion(lg, target, inv_n, rows_per_draw=0, base=None):
    """out, g_logits, loss, hits of N x C logits. base = (loss, hits) to accumulate onto."""
    lg = np.asarray(lg, np.float64)
    N, C = lg.shape
    t = clamp_targets(target, C, N, rows_per_draw)
    inv = float(F(inv_n))
    out = log_softmax(lg)
    onehot = np.zeros((N, C))
    onehot[np.arange(N), t] = 1.0
    with np.errstate(invalid="ignore"):
        g = (np.exp(out) - onehot) * inv
    loss = float(-(out[np.arange(N), t] * inv).sum())
    hits = int((first_max(lg) == t).sum())
    if base is not None:
        loss, hits = loss + base[0], hits + base[1]
    return dict(logits=lg, out=out, g_logits=g, loss=loss, hits=hits, t=t)


def head_forward(h, w3, bias, target, inv_n, rows_per_draw=0, base=None):
    lg = np.asarray(h, np.float64) @ np.asarray(w3, np.float64).T + 0.0
    if bias is not None:
        lg = lg + np.asarray(bias, np.float64)
    return criterion(lg, target, inv_n, rows_per_draw, base)


def slot_logits(slots, bias):
    """Bit-exact: the slots added in float32, slot by slot in order from 0, then the bias (include/vbnn_hip.h fixes the order).
    slots is n_slots x N x 16; returns N x 16 float32 (the caller cuts the first C classes)."""
    s = np.zeros(slots.shape[1:], F)
    for k in range(slots.shape[0]):
        s = (s + slots[k].astype(F)).astype(F)
    if bias is not None:
        b = np.zeros(16, F)
        b[:len(bias)] = bias
        s = (s + b).astype(F)
    return s


def nll_forward(out, target, inv_n):
    out = np.asarray(out, np.float64)
    N, C = out.shape
    t = clamp_targets(target, C, N)
    return float(-(out[np.arange(N), t] * float(F(inv_n))).sum()), int((first_max(out) == t).sum())


def nll_backward(target, N, C, inv_n):
    g = np.zeros((N, C), F)
    g[np.arange(N), clamp_targets(target, C, N)] = -F(inv_n)
    return g


def logsoftmax_backward(out, g):
    out, g = np.asarray(out, np.float64), np.asarray(g, np.float64)
    return g - np.exp(out) * g.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------ the head's backward
def head_backward(h, w3, g, dtype, relu_mask=1, r=None, g_prev_stored=None, base=None):
    """Everything vbnn_head_backward produces. h, w3, r: values of the operand type; g: float32 d(loss)/d(logits).
    g_prev_stored: the g_prev the sums of gradBias_prev run over (default: this function's own, rounded to the type).
    base: dict of gradWeight / gradBias / gradBias_prev to accumulate onto. The `_abs` entries are the sums of the absolute
    terms of the same sums (what the rounding bounds scale with)."""
    h64, w64 = np.asarray(h, np.float64), np.asarray(w3, np.float64)
    gr = round_t(g, dtype).astype(np.float64)
    gx = gr @ w64 + 0.0                                  # (+ 0.0: a sum of -0 products is +0 on the device, which starts from +0)
    gx_abs = np.abs(gr) @ np.abs(w64)
    keep = (h64 > 0) if relu_mask else np.ones_like(h64, bool)
    gp = np.where(keep, gx, 0.0)
    res = dict(g_prev=gp, g_prev_abs=np.where(keep, gx_abs, 0.0))
    if r is not None:
        r64 = np.asarray(r, np.float64)
        res["gv_prev"] = gp * r64
        res["gv_prev_abs"] = res["g_prev_abs"] * np.abs(r64)
    stored = round_t(gp, dtype).astype(np.float64) if g_prev_stored is None else np.asarray(g_prev_stored, np.float64)
    res["gradWeight"], res["gradWeight_abs"] = gr.T @ h64 + 0.0, np.abs(gr).T @ np.abs(h64)
    g64 = np.asarray(g, np.float64)
    res["gradBias"], res["gradBias_abs"] = g64.sum(axis=0) + 0.0, np.abs(g64).sum(axis=0)
    res["gradBias_prev"], res["gradBias_prev_abs"] = stored.sum(axis=0) + 0.0, np.abs(stored).sum(axis=0)
    if base is not None:
        for k in ("gradWeight", "gradBias", "gradBias_prev"):
            if base.get(k) is not None:
                res[k] = res[k] + np.asarray(base[k], np.float64)
    return res


# ------------------------------------------------------------------------------------------------ the small pieces
def relu_forward(x):
    x = np.asarray(x, F)
    return np.where(x > 0, x, F(0))                      # a NaN and -0.0 give +0: x > 0 ? x : 0


def relu_backward(x, g):
    return np.where(np.asarray(x, F) > 0, np.asarray(g, F), F(0))


def acc_grad_bias(g, scale, base=None):
    """(sum, sum of absolute terms) of gradBias = base + scale * column sums of g."""
    g = np.asarray(g, np.float64)
    s, a = float(F(scale)) * g.sum(axis=0), abs(float(F(scale))) * np.abs(g).sum(axis=0)
    return (s if base is None else s + np.asarray(base, np.float64)), a


# ------------------------------------------------------------------------------------------------ the derived bound
def row_bounds(lg, target, inv_n, rows_per_draw=0):
    """B_out (N x C), B_g (N x C), B_loss of the module docstring for exact float32 logits lg. Rows holding a NaN get NaN."""
    lg = np.asarray(lg, np.float64)
    N, C = lg.shape
    t = clamp_targets(target, C, N, rows_per_draw)
    inv = float(F(inv_n))
    with np.errstate(invalid="ignore"):
        mx = lg.max(axis=1)
        se = np.exp(lg - mx[:, None]).sum(axis=1)
        lse = mx + np.log(se)
        out = lg - lse[:, None]
        b_lse = E_ULP * ULP * (1.0 + np.log(se)) + (C - 1) * U32 * (1.0 + 1.0 / math.e) + C * TINY + U32 * np.abs(lse)
        b_out = b_lse[:, None] + U32 * np.abs(out)
        p = np.exp(out)
        onehot = np.zeros((N, C))
        onehot[np.arange(N), t] = 1.0
        b_g = inv * (p * (np.expm1(b_out) + E_ULP * ULP) + 2 * U32 * np.abs(p - onehot)) + TINY * inv
        ot = out[np.arange(N), t]
        b_loss = float(np.nansum(inv * b_out[np.arange(N), t] + 1e-12 * np.abs(ot) * inv))
    return b_out, b_g, b_loss


def _exp32(x):
    return np.exp(np.asarray(x, F).astype(np.float64)).astype(F)


def row_arith_f32(lg, target, inv_n, rows_per_draw=0):
    """The row arithmetic as the kernels write it, one float32 NumPy operation per statement (exp and log rounded from
    float64): lane groups of four classes summed in order, then the two shuffle steps. Only to measure the bound."""
    lg = np.asarray(lg, F)
    N, C = lg.shape
    t = clamp_targets(target, C, N, rows_per_draw)
    inv = F(inv_n)
    mx = lg.max(axis=1, keepdims=True)
    e = _exp32(lg - mx)
    groups = []
    for q in range(0, C, 4):
        s = np.zeros(N, F)
        for c in range(q, min(q + 4, C)):
            s = (s + e[:, c]).astype(F)
        groups.append(s)
    while len(groups) > 1:                               # xor 16, then xor 32 (more groups: the same pairing carried on)
        groups = [(groups[i] + groups[i + 1]).astype(F) if i + 1 < len(groups) else groups[i] for i in range(0, len(groups), 2)]
    se = groups[0]
    lse = (mx[:, 0] + np.log(se.astype(np.float64)).astype(F)).astype(F)
    o = (lg - lse[:, None]).astype(F)
    onehot = np.zeros((N, C), F)
    onehot[np.arange(N), t] = 1
    g = ((_exp32(o) - onehot).astype(F) * inv).astype(F)
    loss = float(-(o[np.arange(N), t].astype(np.float64) * float(inv)).sum())
    return o, g, loss


# ------------------------------------------------------------------------------------------------ input sets (shared by the CPU and the GPU tests)
def int_operands(N, H, C, seed, r_kind="T"):
    """Integer-valued operands on which every sum of the head is exact: h in 0..3, w3 and g in -3..3, r in +-0.5, +-1, +-2, a small
    integer bias; |gx| <= 16 x 9 = 144 is exact in bf16."""
    rng = np.random.default_rng(seed)
    return dict(h=rng.integers(0, 4, (N, H)).astype(F), w3=rng.integers(-3, 4, (C, H)).astype(F),
                g=rng.integers(-3, 4, (N, C)).astype(F), bias=rng.integers(-4, 5, C).astype(F),
                r=rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], F), (N, H)), target=rng.integers(0, C, N).astype(np.int32))


def real_operands(N, H, C, seed, dtype):
    rng = np.random.default_rng(seed)
    rt = lambda a: round_t(a.astype(F), dtype)
    return dict(h=rt(np.maximum(rng.standard_normal((N, H)), -0.3)), w3=rt(rng.standard_normal((C, H)) * 0.2),
                g=(rng.standard_normal((N, C)) / N).astype(F), bias=(rng.standard_normal(C) * 0.5).astype(F),
                r=rt(rng.standard_normal((N, H))), target=rng.integers(0, C, N).astype(np.int32))


def logit_operands(lg):
    """h (N x 32), w3 (C x 32) with h w3^T = lg for integer logits |lg| <= 256 (exact in bf16): w3 is the identity on the
    first C hidden units."""
    N, C = lg.shape
    h, w3 = np.zeros((N, 32), F), np.zeros((C, 32), F)
    h[:, :C] = lg
    w3[np.arange(C), np.arange(C)] = 1
    return h, w3


EXTREME_KINDS = ("peak120", "target100", "bias+30000", "bias-30000", "all_equal", "tie_3_4", "tie_7_8", "tie_0_15",
                 "target_low", "target_high")


def extreme_logits(kind, N, C, seed=11):
    """(integer logits without the bias, bias, targets) of one of the log-softmax edge cases."""
    rng = np.random.default_rng(seed)
    lg = rng.integers(-3, 4, (N, C)).astype(F)
    bias = np.zeros(C, F)
    target = rng.integers(0, C, N).astype(np.int32)
    rows = np.arange(N)
    if kind == "peak120":
        lg[rows, rows % C] += 120
    elif kind == "target100":
        peak = (target + 1 + rows % max(C - 1, 1)) % C
        lg[rows, peak] += 100                             # the target class ~100 below the maximum (C = 1: the maximum itself)
    elif kind.startswith("bias"):
        bias[:] = 30000.0 if kind[4] == "+" else -30000.0
    elif kind == "all_equal":
        lg[:] = 2
    elif kind.startswith("tie_"):
        a, b = (min(int(k), C - 1) for k in kind.split("_")[1:])
        lg[:, a] = 5
        lg[:, b] = 5                                      # a true tie of the maximum; the target on it (a, b) and off it, by row
        target = np.array([(a, b, (a + 1) % C, 0)[n % 4] for n in range(N)], np.int32)
    elif kind == "target_low":
        target[::2] = -1
    elif kind == "target_high":
        target[::2] = C
        target[1::4] = C + 7
    return lg, bias, target


FWD_SHAPES = ([(N, 70, 10, 0) for N in (1, 16, 17, 47)] + [(17, H, 10, 0) for H in (1, 2, 31, 33, 130)] +
              [(17, 70, C, 0) for C in range(1, 17)] + [(33, 70, 10, 11)])          # (N, H, C, rows_per_draw)
NLL_CLASSES = (1, 10, 16, 17, 64, 65, 1030)                                         # vbnn_logsoftmax_nll's class counts


def row_sets():
    """Every set of exact float32 logits the GPU tests put through the row arithmetic: (name, logits with the bias, targets,
    inv_n, rows_per_draw)."""
    for i, (N, H, C, rpd) in enumerate(FWD_SHAPES):
        o = int_operands(N, H, C, 100 + i)
        lg = (o["h"].astype(np.float64) @ o["w3"].astype(np.float64).T + o["bias"]).astype(F)
        yield f"int N{N} H{H} C{C} rpd{rpd}", lg, o["target"][:rpd or N], F(1.0 / (rpd or N)), rpd
    for H in (3456, 6912):
        o = int_operands(17, H, 10, 7)
        yield f"int H{H}", (o["h"].astype(np.float64) @ o["w3"].astype(np.float64).T + o["bias"]).astype(F), o["target"], F(1 / 17), 0
    for kind in EXTREME_KINDS:
        for C in NLL_CLASSES:
            lg, bias, target = extreme_logits(kind, 19, C)
            yield f"{kind} C{C}", (lg + bias).astype(F), target, F(1.0 / 19), 0
    for C in (10, 16):
        o = real_operands(37, 70, C, 3, "f32")
        yield f"real C{C}", (o["h"] @ o["w3"].T * 20 + o["bias"]).astype(F), o["target"], F(1.0 / 37), 0
