"""NumPy reference of the first half of elementwise.hip: the noise fill, the weight draw, the operand packers and the prior / KL
sweeps (vbnn_fill_normal, vbnn_wn_sample, vbnn_pack, vbnn_pack_input, vbnn_compute_prior, vbnn_prep_layer, vbnn_prepare,
vbnn_calc_lc, vbnn_compute_mugrads, vbnn_compute_vargrads), restated from include/vbnn_hip.h and VBLinear.lua as the header cites
it. NumPy and the CPU oracle's Philox normals only; nothing here reads GPU code or a GPU tensor. TEST INFRASTRUCTURE ONLY.

Every entry has a float64 definition (`*_f64`: inputs widened, nothing rounded) and a float32 restatement (`*_f32`: one NumPy
float32 operation per statement of the stated order -- the kernels are built with -ffp-contract=off, and hipcc's fp32 divide and
sqrtf are correctly rounded). Only expf, logf and the double sums are not reproducible bit for bit.

WHAT IS BITWISE (device == `*_f32`, bit for bit)                       WHAT IS BOUNDED
  fill_normal   z scale (one multiply); pads untouched                 the hardware form: HW_ABS |scale| + u |z scale|
  wn_sample     e; w = means + fl(sd e) with stdv given                 lvars only: sd = sqrt32(exp(l)): envelope (below)
  pack          COPY, SQUARE, MUL, RELU, RELU_SQUARE, both dtypes;      EXP: f32 within E_ULP ulp of exp64; bf16 by the
                SQUARE forms square the value ROUNDED to T;             interval rule on exp64 (1 +- E_ULP ULP)
                dstT == dst transposed
  pack_input    x_s = T(x[n % rpd]), x2_s = T(fl(T(x)^2)),              --
                both transposes == the row-major outputs transposed
  prior         mu_s = T(means); mu_sqe = fl(m m);                      vars / var_s: E_ULP ulp of exp64 (bf16: interval);
                stdv = sqrt32(the device's own vars);                   stats[0], stats[1]: below; stats[2] = stats[0] / W to
                transposes == row-major shadows; stats[3] == W          double rounding
  calc_lc       the sum is the float64 sum of the device's own          per element: lc_bound (derived below), absolute;
                elements to 1e-10 sum |lc|                              the sum against the definition: the summed bounds
  mugrads       lcg = m / den, gradWeight / S                           --
  vargrads      lcg, gradSum with vars + stdv given                     lvars only: envelope

ENVELOPE (the update test's rule). Where a float32 result depends on expf, it must lie between the smallest and the largest of
the restatement's results with exp moved by -E_ULP .. +E_ULP ulp, element-wise, widened by one ulp either way. E_ULP = 2: the
1 ulp of expf in the HIP math API's accuracy table plus 1 ulp for the float32 rounding of the float64 reference.

RELU FUNCTIONS OF pack (fmaxf(a, 0)). A NaN gives +0 (fmaxf drops a NaN), so RELU_SQUARE of a NaN is +0 as well. For -0.0 IEEE 754
leaves the sign of maxNum(-0, +0) open; gfx950's maximum orders -0 below +0 and k_pack writes +0, as k_relu_fwd (x > 0 ? x : 0)
does, so the reference is where(a > 0, a, +0) and is compared bit for bit like everything else.

BOUNDS. u = U32 = 2^-24 (unit roundoff), ULP = 2^-23, TINY = 2^-126 (absolute error of an operation that underflows).
  stats[0] = sum fl(v + fl(m m)), v = expf(l): per term |v - exp(l)| <= E_ULP ULP exp(l); the square u m^2 + TINY; the add
      u (v + m^2). Summed, times SLACK, plus 1e-10 of the sum for the reordered double accumulation:      prior_sum_bound
  stats[1] = sum l: the terms are exact; 1e-10 sum |l| (relative to the magnitudes: the sum itself cancels).
  calc_lc, per element (lc_bound). Kernel:  s = sqrtf(v); g = logf(s); first = -g + lvh, lvh = (float) log(sqrt(var_hat));
      d = v - vh, vh = (float) var_hat; n = q + d; second = n / (2 vh); t = first + second; lc = t invB, invB = 1 / B.
      Inputs: v is exact when given; = expf(l) otherwise: relative e_v = E_ULP ULP. q is exact when given; fl(m m) otherwise:
      e_q = u q + TINY.
        s       sqrt halves v's error, one rounding: relative e_v / 2 + u
        g       |g - log sqrt v| <= E_ULP ULP |log sqrt v| + (e_v / 2 + u)     (logf: 1 ulp documented + 1; d log s = ds / s)
        lvh     u |lvh|
        first   e_first = E_ULP ULP A + e_v / 2 + u + u |lvh| + u (A + |lvh|),   A = |log sqrt v|
        d       e_d = e_v v + u vh + u (|v - var_hat| + e_v v + u vh)            (vh against the double var_hat: u vh)
        n       e_n = e_q + e_d + u (|q + v - var_hat| + e_q + e_d)
        second  e_second = e_n / (2 var_hat) + 2 u |second|                       (vh in the denominator: u; the divide: u)
        t       e_t = e_first + e_second + u (|first + second| + e_first + e_second)
        lc      e_lc = e_t / B + 2 u |lc| + TINY                                  (invB: u; the product: u)
      times SLACK. Absolute: it stays meaningful where first + second cancels (v = var_hat, mu = 0: a fresh layer)."""
import numpy as np

from tests._gemm_np import interval_ok
from tests._head_np import E_ULP, TINY, U32, ULP
from tests._update_np import bf16_bits, bf16_round, bf16_to_f32, exp32, exp_shifted, step_ulps

F = np.float32
f8 = np.float64
SLACK = 1.0 + 2.0 ** -10
HW_ABS = 2e-6            # the header's bound of the hardware-transcendental normals against the contract's
COPY, EXP, SQUARE, MUL, RELU, RELU_SQUARE = range(6)
SQUARE_FORMS = (SQUARE, RELU_SQUARE)
RELU_FORMS = (RELU, RELU_SQUARE)

# largest fraction of each derived bound that the float32 restatement (correctly rounded exp / log) uses over every input set
# of tests/test_sweeps_gpu.py, measured 2026-10-20 by test_sweeps_ref.py::test_restatement_stays_inside_the_derived_bounds
# and ::test_prior_restatement_against_the_oracle_and_the_definition (which fail when a record is below the measurement or more
# than twice above it): 0.4671, 0.0693, 0.4170, below 1e-3
BOUND_USED = {"lc_elem": 0.47, "lc_sum": 0.07, "stats0": 0.42, "stats1": 0.001}


def round_t(x, dtype):
    x = np.asarray(x, F)
    return bf16_round(x) if dtype == "bf16" else x


def stored(x, dtype):
    """What a T store of the float32 x holds: the float32 itself, or the bf16 bit pattern (uint16)."""
    x = np.asarray(x, F)
    return bf16_bits(x) if dtype == "bf16" else x


def values(a):
    return bf16_to_f32(a) if a.dtype == np.uint16 else a


def envelope(run):
    """[min, max], one ulp wider either way, of run(exp) over exp = exp32 moved by -E_ULP .. +E_ULP ulp. The two ends alone
    are the envelope only where the result is monotone in exp(l); the roundings behind a cancellation are not, and an expf
    within E_ULP ulp IS one of these 2 E_ULP + 1 floats, so all of them are run."""
    outs = [run(exp_shifted(k)) for k in range(-E_ULP, E_ULP + 1)]
    a = np.nextafter(np.minimum.reduce(outs), F(-np.inf))
    b = np.nextafter(np.maximum.reduce(outs), F(np.inf))
    return a, b


def exp_ok(got, l, dtype):
    """element-wise: `got` (float32 values, or bf16 values as float32) is expf(l) within E_ULP ulp of exp64, or its bf16 store."""
    l = np.asarray(l, F)
    ex = np.exp(l.astype(f8))
    if dtype == "bf16":
        return interval_ok(np.asarray(got, f8), ex, E_ULP * ULP * ex)
    r = exp32(l)
    return (step_ulps(r, -E_ULP) <= got) & (got <= step_ulps(r, +E_ULP))


def exp_ulps(got, l):
    """|got - exp64(l)| in ulp of the rounded exp64."""
    ex = np.exp(np.asarray(l, F).astype(f8))
    return np.abs(np.asarray(got, f8) - ex) / np.spacing(ex.astype(F)).astype(f8)


# ------------------------------------------------------------------------------------------------ input sets
MU_SPECIAL = np.array([0.0, 1e-20, -1e-20, 3.0, -3.0], F)
PARAM_SETS = ("trained", "wide", "fresh")


def param_set(kind, W, seed=0):
    """(means, lvars), flat float32. trained: lvars ~ log 1e-3 +- 0.5; wide: lvars uniform over [-20, 5]; fresh: v = var_hat
    exactly and mu = 0. The first two carry mu in {0, +-1e-20, +-3} at scattered places (where W leaves room)."""
    r = np.random.RandomState(1000 + seed + W % 997)
    if kind == "fresh":
        return np.zeros(W, F), np.full(W, F(np.log(1e-3)), F)
    means = (0.05 * r.standard_normal(W)).astype(F)
    lvars = (np.log(1e-3) + 0.5 * r.standard_normal(W)).astype(F) if kind == "trained" else r.uniform(-20.0, 5.0, W).astype(F)
    if W >= 5:
        at = (np.arange(5) * max(1, W // 5) + (W // 7)) % W
        means[at] = MU_SPECIAL
        means[W - 1] = MU_SPECIAL[3]
    return means, lvars


def input_set(N, I, seed=0):
    """A minibatch: normals; a zero row; -0.0; values bf16 rounds up into the next binade (0.99999994 -> 1, 1.9999999 -> 2)."""
    r = np.random.RandomState(2000 + seed + N * 131 + I)
    x = r.standard_normal((N, I)).astype(F)
    flat = x.reshape(-1)
    up = np.array([0x3F7FFFFF, 0x3FFFFFFF, 0xBFFFFF00, 0x3EFFFFC0], np.uint32).view(F)
    if N * I >= 16:
        flat[1::max(2, (N * I) // 9)] = F(-0.0)
        flat[2::max(3, (N * I) // 7)] = np.resize(up, flat[2::max(3, (N * I) // 7)].shape)
    if N >= 3:
        x[N // 2] = 0.0
    return x


def pack_set(rows, cols, seed=0):
    """(src, src2): 3 x normals; from two rows on, row 1 starts with NaN, +inf, -inf, -0.0, +0.0 (as far as the columns go)."""
    r = np.random.RandomState(3000 + seed + rows * 131 + cols)
    a = (3.0 * r.standard_normal((rows, cols))).astype(F)
    b = r.standard_normal((rows, cols)).astype(F)
    if rows >= 2:
        sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F)[:cols]
        a[1, :sp.size] = sp
    return a, b


# ------------------------------------------------------------------------------------------------ fill_normal
def _normals(rows, cols, seed, stream, layer, draw, row0):
    from oracle import vbnn_oracle as vo          # the contract's Philox + Box-Muller, pinned by the known-answer vectors
    return vo.fill_normal(rows, cols, seed, stream, layer, draw, row0)


def fill_normal_f32(rows, cols, seed, stream, layer, draw, row0=0, scale=1.0):
    return _normals(rows, cols, seed, stream, layer, draw, row0) * F(scale)


def fill_normal_f64(rows, cols, seed, stream, layer, draw, row0=0, scale=1.0):
    return _normals(rows, cols, seed, stream, layer, draw, row0).astype(f8) * float(F(scale))


def fill_normal_hw_bound(z64_scaled, scale):
    return (HW_ABS * abs(float(F(scale))) + U32 * np.abs(z64_scaled)) * SLACK


# ------------------------------------------------------------------------------------------------ wn_sample
STREAM_EPS = 1


def wn_eps(O, I, seed, layer, draw):
    return _normals(O, I, seed, STREAM_EPS, layer, draw, 0)


def wn_sample_f32(means, stdv, lvars, e, exp=exp32):
    """w = means + fl(sd e); sd = stdv when given, sqrt32(exp(lvars)) otherwise."""
    sd = np.asarray(stdv, F) if stdv is not None else np.sqrt(exp(np.asarray(lvars, F)))
    tmp = sd * np.asarray(e, F)
    return np.asarray(means, F) + tmp


def wn_sample_f64(means, stdv, lvars, e):
    sd = np.asarray(stdv, F).astype(f8) if stdv is not None else np.exp(0.5 * np.asarray(lvars, F).astype(f8))
    return np.asarray(means, F).astype(f8) + sd * np.asarray(e, F).astype(f8)


# ------------------------------------------------------------------------------------------------ pack
def relu32(a):
    """fmaxf(a, 0) as gfx950 answers it: a itself where a > 0, +0 otherwise (NaN and -0.0 included)."""
    a = np.asarray(a, F)
    return np.where(a > 0, a, F(0.0)).astype(F)


def pack_f32(func, a, b, dtype):
    """The float32 value k_pack forms before the store to T (EXP: the float32-rounded exp64, a stand-in the tests bound)."""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        if func in SQUARE_FORMS:
            h = relu32(a) if func == RELU_SQUARE else a
            hr = round_t(h, dtype)
            return hr * hr
        if func == EXP:
            return exp32(a)
        if func == MUL:
            return a * np.asarray(b, F)
        if func == RELU:
            return relu32(a)
        return a


def pack_f64(func, a, b, dtype):
    a8 = np.asarray(a, F).astype(f8)
    with np.errstate(all="ignore"):
        if func in SQUARE_FORMS:
            hr = round_t(relu32(a) if func == RELU_SQUARE else a, dtype).astype(f8)
            return hr * hr
        if func == EXP:
            return np.exp(a8)
        if func == MUL:
            return a8 * np.asarray(b, F).astype(f8)
        if func == RELU:
            return relu32(a).astype(f8)
        return a8


# ------------------------------------------------------------------------------------------------ pack_input
def pack_input_f32(x, N, rpd, dtype):
    """(x_s, x2_s) as stored (float32, or bf16 bits): x_s = T(x[n % rpd]), x2_s = T(fl(T(x)^2))."""
    x = np.asarray(x, F)
    rows = x[np.arange(N) % rpd] if rpd > 0 else x[:N]
    xr = round_t(rows, dtype)
    return stored(rows, dtype), stored(xr * xr, dtype)


def pack_input_f64(x, N, rpd, dtype):
    x = np.asarray(x, F)
    rows = x[np.arange(N) % rpd] if rpd > 0 else x[:N]
    xr = round_t(rows, dtype).astype(f8)
    return rows.astype(f8), xr * xr


# ------------------------------------------------------------------------------------------------ compute_prior / prep_layer
def _double_sum(a):
    return float(np.sum(np.asarray(a).astype(f8)))


def finish_stats(s0, s1, W):
    """prior_finish: var_hat is (1 / W) x the sum, formed in double."""
    return np.array([s0, s1, (1.0 / float(W)) * s0, float(W)])


def prior_f32(means, lvars, exp=exp32):
    """vars, stdv, mu_sqe (float32) and the four statistics as the sweeps form them: sums of fl(v + fl(m m)) and of l in double."""
    m, l = np.asarray(means, F), np.asarray(lvars, F)
    v = exp(l)
    sd = np.sqrt(v)
    q = m * m
    return dict(vars=v, stdv=sd, mu_sqe=q, stats=finish_stats(_double_sum(v + q), _double_sum(l), m.size))


def prior_f64(means, lvars):
    m, l = np.asarray(means, F).astype(f8), np.asarray(lvars, F).astype(f8)
    v = np.exp(l)
    return dict(vars=v, stdv=np.sqrt(v), mu_sqe=m * m, stats=finish_stats(float(np.sum(v + m * m)), float(np.sum(l)), m.size))


def prior_sum_bound(means, lvars):
    """Bound of |stats[0] - sum(exp64(l) + m^2)| (module docstring)."""
    m, l = np.asarray(means, F).astype(f8), np.asarray(lvars, F).astype(f8)
    v, q = np.exp(l), m * m
    per = E_ULP * ULP * v + U32 * q + TINY + U32 * (v + q)
    return float(np.sum(per)) * SLACK + 1e-10 * float(np.sum(v + q))


def lsum_bound(lvars):
    return 1e-10 * float(np.sum(np.abs(np.asarray(lvars, F).astype(f8))))


# ------------------------------------------------------------------------------------------------ calc_lc
def calc_lc_f32(means, lvars, vars_, mu_sqe, var_hat, B, exp=exp32):
    """k_lc_partial in float32; logf as the float32 rounding of the float64 log. Returns (elements, their float64 sum)."""
    var_hat = float(var_hat)
    lvh = F(np.log(np.sqrt(var_hat)))
    vh = F(var_hat)
    invB = F(1.0) / F(B)
    v = np.asarray(vars_, F) if vars_ is not None else exp(np.asarray(lvars, F))
    q = np.asarray(mu_sqe, F) if mu_sqe is not None else np.asarray(means, F) * np.asarray(means, F)
    s = np.sqrt(v)
    g = np.log(s.astype(f8)).astype(F)
    first = -g + lvh
    second = (q + (v - vh)) / (F(2.0) * vh)
    lc = (first + second) * invB
    return lc, _double_sum(lc)


def _lc_terms(means, lvars, vars_, mu_sqe, var_hat, B):
    var_hat, Bf = float(var_hat), float(F(B))
    v = np.asarray(vars_, F).astype(f8) if vars_ is not None else np.exp(np.asarray(lvars, F).astype(f8))
    q = np.asarray(mu_sqe, F).astype(f8) if mu_sqe is not None else np.asarray(means, F).astype(f8) ** 2
    first = -np.log(np.sqrt(v)) + np.log(np.sqrt(var_hat))
    second = (q + v - var_hat) / (2.0 * var_hat)
    return v, q, first, second, var_hat, Bf


def calc_lc_f64(means, lvars, vars_, mu_sqe, var_hat, B):
    v, q, first, second, var_hat, Bf = _lc_terms(means, lvars, vars_, mu_sqe, var_hat, B)
    lc = (first + second) / Bf
    return lc, float(np.sum(lc))


def lc_bound(means, lvars, vars_, mu_sqe, var_hat, B):
    """The per-element absolute bound of the module docstring."""
    v, q, first, second, var_hat, Bf = _lc_terms(means, lvars, vars_, mu_sqe, var_hat, B)
    e_v = 0.0 if vars_ is not None else E_ULP * ULP
    e_q = np.zeros_like(q) if mu_sqe is not None else U32 * q + TINY
    A, lvh = np.abs(np.log(np.sqrt(v))), abs(np.log(np.sqrt(var_hat)))
    e_first = E_ULP * ULP * A + 0.5 * e_v + U32 + U32 * lvh + U32 * (A + lvh)
    e_d = e_v * v + U32 * var_hat + U32 * (np.abs(v - var_hat) + e_v * v + U32 * var_hat)
    e_n = e_q + e_d + U32 * (np.abs(q + v - var_hat) + e_q + e_d)
    e_second = e_n / (2.0 * var_hat) + 2.0 * U32 * np.abs(second)
    e_t = e_first + e_second + U32 * (np.abs(first + second) + e_first + e_second)
    return (e_t / Bf + 2.0 * U32 * np.abs((first + second) / Bf) + TINY) * SLACK


# ------------------------------------------------------------------------------------------------ KL gradients
def mugrads_f32(means, var_hat, B, S, gradWeight):
    """(lcg, gradWeight / S): den = (float)((double) B x stats[2])."""
    den = F(float(F(B)) * float(var_hat))
    return np.asarray(means, F) / den, None if gradWeight is None else np.asarray(gradWeight, F) / F(S)


def mugrads_f64(means, var_hat, B, S, gradWeight):
    return (np.asarray(means, F).astype(f8) / (float(F(B)) * float(var_hat)),
            None if gradWeight is None else np.asarray(gradWeight, F).astype(f8) / float(F(S)))


def vargrads_f32(lvars, vars_, stdv, var_hat, B, S, gradSum, exp=exp32):
    """(lcg, gradSum'): inv_vh = (float)(1.0 / stats[2]); a = -(1 / v) + inv_vh; lcg = (a / (2 B)) v; gs = (gs / (2 S)) sd."""
    inv_vh = F(1.0 / float(var_hat))
    v = np.asarray(vars_, F) if vars_ is not None else exp(np.asarray(lvars, F))
    sd = np.asarray(stdv, F) if stdv is not None else np.sqrt(v)
    a = -(F(1.0) / v) + inv_vh
    lcg = (a / (F(2.0) * F(B))) * v
    return lcg, None if gradSum is None else (np.asarray(gradSum, F) / (F(2.0) * F(S))) * sd


def vargrads_f64(lvars, vars_, stdv, var_hat, B, S, gradSum):
    v = np.asarray(vars_, F).astype(f8) if vars_ is not None else np.exp(np.asarray(lvars, F).astype(f8))
    sd = np.asarray(stdv, F).astype(f8) if stdv is not None else np.sqrt(v)
    lcg = (-(1.0 / v) + 1.0 / float(var_hat)) / (2.0 * float(F(B))) * v
    return lcg, None if gradSum is None else np.asarray(gradSum, F).astype(f8) / (2.0 * float(F(S))) * sd


def telling_var_hat(var_hat):
    """The nearest double at or above var_hat for which (float)(1.0 / vh) and 1.0f / (float) vh differ: a statistic on which a
    kernel that formed inv_vh the second way would be seen."""
    f = F(var_hat)
    for _ in range(1000):
        vh = float(f) * (1.0 + 0.2 * ULP)         # 0.2 .. 0.4 ulp above a float32: (float) vh is that float, 1 / vh is not 1 / it
        if F(vh) == f and F(1.0 / vh) != F(1.0) / F(vh):
            return vh
        f = np.nextafter(f, F(np.inf))
    raise AssertionError("no distinguishing var_hat found")
