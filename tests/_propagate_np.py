"""NumPy restatement of the sampling-free predictive (include/vbnn_hip.h: moment propagation; vbnn_amd/csrc/propagate.hip) for the
tests. NumPy only; nothing here reads GPU code or a GPU tensor.
  (a) float64 moment propagation of a whole network from the operands as the engine holds them (operands()), with the rounding
      points of the engine's dtype and an error bound that the RESTATEMENT computes, never the engine: the project's GEMM bound
      (4e-6 sum |a| |b| per product, tests/test_parity_gpu.py) carried through the layers, 4 EPS_RELU per ReLU stage.
  (b) relu_moments32: vbnn_relu_moments' op sequence in np.float32, one NumPy operation per statement of the header; expf and
      erfcf are the float64 functions rounded to fp32 (correctly rounded, where the device's are a few ulp).
  (c) the LRT sampler of a one-VB-layer network in NumPy (sample_one_layer) and the moment band the statistical tests share.
erfc comes from tests/_quantiles_np.py (torch on the CPU, float64)."""
import numpy as np

from tests._quantiles_np import erfc64
from tests._update_np import bf16_round

F, D = np.float32, np.float64
GEMM_EPS = 4e-6                        # the parity tests' bound per fp32-accumulated product: |d| <= 4e-6 sum |a| |b|

# The largest scale-relative error of relu_moments32 against relu_moments64 that tests/test_propagate_ref.py measures on its grid
# and its 1e5 random (m, v): |da| / scale, |dq| / scale^2, |dc| / scale^2 with scale = max(s, |m|). The device tests allow
# 4 x this; measured 3.61e-07 on the random pairs, 1.20e-07 on the grid (the device's erfcf / expf are a few ulp where the restatement's are correctly rounded: the margin EPS_F took).
EPS_RELU = 3.7e-07

ALPHAS = (-12.0, -6.0, -2.0, -0.5, 0.0, 0.5, 2.0, 6.0, 12.0)
SCALES = (1e-4, 1.0, 30.0)


# ------------------------------------------------------------------------------------------------ the ReLU of a Gaussian
def relu_moments64(m, v):
    """E[h], E[h^2], Var[h] of h = max(0, y), y ~ N(m, v), float64; v = 0: the point mass at m."""
    m, v = np.asarray(m, D), np.asarray(v, D)
    pos = v > 0
    s = np.sqrt(np.where(pos, v, 1.0))
    al = m / s
    Phi = 0.5 * erfc64(-al * np.sqrt(0.5))
    phi = np.exp(-0.5 * al * al) / np.sqrt(2.0 * np.pi)
    a = np.maximum(m * Phi + s * phi, 0.0)
    q = np.maximum((m * m + v) * Phi + m * s * phi, 0.0)
    r = np.maximum(m, 0.0)
    a, q = np.where(pos, a, r), np.where(pos, q, r * r)
    return a, q, np.where(pos, np.maximum(q - a * a, 0.0), 0.0)


def _exp32(x):
    return np.exp(x.astype(D)).astype(F)


def _erfc32(x):
    return erfc64(x.astype(D)).astype(F)


def relu_moments32(m, v1, v2=None):
    """vbnn_relu_moments in np.float32, statement for statement (fp32 a, q, c BEFORE the rounding to the operand type)."""
    m, v = np.asarray(m, F), np.asarray(v1, F)
    if v2 is not None:
        v = v + np.asarray(v2, F)
    with np.errstate(all="ignore"):
        s = np.sqrt(v)
        al = m / s
        phi = F(0.3989423) * _exp32(F(-0.5) * (al * al))
        Phi = F(0.5) * _erfc32(-(al * F(0.70710677)))
        a = np.maximum(m * Phi + s * phi, F(0))
        q = np.maximum((m * m + v) * Phi + (m * s) * phi, F(0))
        c = np.maximum(q - a * a, F(0))
    pos = v > 0
    r = np.maximum(m, F(0))
    return np.where(pos, a, r).astype(F), np.where(pos, q, r * r).astype(F), np.where(pos, c, F(0)).astype(F)


def relu_scale(m, v):
    """The scale of the scale-relative error: max(s, |m|) in float64."""
    return np.maximum(np.sqrt(np.asarray(v, D)), np.abs(np.asarray(m, D)))


def scale_relative_error(got, m, v):
    """max over elements of |da| / scale, |dq| / scale^2, |dc| / scale^2 of `got` = (a, q, c) against float64 on the same fp32
    inputs (elements of scale 0 must be exact)."""
    want = relu_moments64(m, v)
    sc = relu_scale(m, v)
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        d = np.abs(np.asarray(g, D) - w)
        assert (d[sc == 0] == 0).all()
        worst = max(worst, float((d[sc > 0] / sc[sc > 0] ** (1 if k == 0 else 2)).max(initial=0.0)))
    return worst


def grid32():
    """The issue's grid as fp32 (m, v): alpha x s, plus v = 0 at every m of the grid."""
    ms, vs = [], []
    for s in SCALES:
        for al in ALPHAS:
            ms.append(al * s); vs.append(s * s)
    for m in list(ms):
        ms.append(m); vs.append(0.0)
    return np.array(ms, F), np.array(vs, F)


def random32(n=100000, seed=5):
    """n random fp32 (m, v): |m| over five decades either sign, v over twelve."""
    g = np.random.default_rng(seed)
    m = g.standard_normal(n) * 10.0 ** g.uniform(-3, 2, n)
    v = 10.0 ** g.uniform(-8, 4, n)
    return m.astype(F), v.astype(F)


# ------------------------------------------------------------------------------------------------ the whole network
def rounder(dtype):
    """float64 -> the engine's operand type -> float64."""
    if dtype == "bf16":
        return lambda a: bf16_round(np.asarray(a, D).astype(F)).astype(D)
    return lambda a: np.asarray(a, D).astype(F).astype(D)


def _round_with_bound(rnd, a, e):
    """a rounded to the operand type, and the bound of |rounded device value - rounded a| given |device value - a| <= e before
    the rounding: rounding is monotone, so the device's lands in [rnd(a - e), rnd(a + e)] -- exactly rnd(a) where no rounding
    boundary lies within e."""
    r = rnd(a)
    return r, np.maximum(np.abs(rnd(a + e) - r), np.abs(r - rnd(a - e)))


def operands(means, lvars, dtype, mask=None):
    """One VB layer's operands as the engine holds them, float64: mu = T(means), var = T(expf(lvars)) with the bound var_err of
    what an expf two ulp off would change, mu2 = T(mu . mu in fp32); mask (bool, True = pruned): +0 in all of them."""
    rnd = rounder(dtype)
    mu = rnd(np.asarray(means, F))
    v32 = np.exp(np.asarray(lvars, F).astype(D)).astype(F).astype(D)
    var, var_err = _round_with_bound(rnd, v32, v32 * 2.0 ** -22)
    if mask is not None:
        mu, var, var_err = np.where(mask, 0.0, mu), np.where(mask, 0.0, var), np.where(mask, 0.0, var_err)
    mu2 = rnd((mu.astype(F) * mu.astype(F)).astype(D))
    return dict(mu=mu, var=var, var_err=var_err, mu2=mu2)


def final_operands(w3, dtype):
    rnd = rounder(dtype)
    w = rnd(np.asarray(w3, F))
    return w, rnd((w.astype(F) * w.astype(F)).astype(D))


def layer64(mom, err, op, b, first, rnd, eps_relu=EPS_RELU):
    """One hidden layer in float64 from its input moments mom = (a, q, c) as the operands hold them and the bounds err = (ea, eq,
    ec) of what the engine's may differ by: the three products, the ReLU moments, the rounding to the operand type. `first`: the
    input is deterministic (no c product). Returns ((a, q, c), (ea, eq, ec)) of the layer's output."""
    (a, q, c), (ea, eq, ec) = mom, err
    mu, var, mu2, b = op["mu"], op["var"], op["mu2"], np.asarray(b, D)
    amu = np.abs(mu)
    m = a @ mu.T + b
    em = GEMM_EPS * ((np.abs(a) + ea) @ amu.T + np.abs(b)) + ea @ amu.T
    v = q @ var.T
    ev = GEMM_EPS * ((q + eq) @ var.T) + eq @ var.T + (q + eq) @ op["var_err"].T
    if not first:
        v2 = c @ mu2.T
        ev = ev + GEMM_EPS * ((c + ec) @ mu2.T) + ec @ mu2.T + 2.0 ** -23 * (v + v2)
        v = v + v2
    s = np.sqrt(v)
    ds = np.maximum(np.sqrt(v + ev) - s, s - np.sqrt(np.maximum(v - ev, 0.0)))
    a, q, c = relu_moments64(m, v)
    # the stage's sensitivities: |da/dm| <= 1, |da/ds| <= phi(0); dq/dm = 2 a, dq/ds = 2 s Phi; |dc/dm| <= 2 a, |dc/ds| <= 2 s
    sc = np.maximum(s, np.abs(m)) + ds + em
    ea = em + 0.39894228 * ds + 4 * eps_relu * sc
    e2 = 2.0 * (a + ea) * em + 2.0 * (s + ds) * ds + 4 * eps_relu * sc * sc
    a, ea = _round_with_bound(rnd, a, ea)
    q, eq = _round_with_bound(rnd, q, e2)
    c, ec = _round_with_bound(rnd, c, e2)
    return (a, q, c), (ea, eq, ec)


def final64(a, c, ea, ec, w3, w3sq, b3):
    """The final Linear from the last layer's a and c: (mean, var, mean_err, var_err)."""
    b3 = np.asarray(b3, D)
    mean = a @ w3.T + b3
    mean_err = GEMM_EPS * ((np.abs(a) + ea) @ np.abs(w3).T + np.abs(b3)) + ea @ np.abs(w3).T
    var = c @ w3sq.T
    var_err = GEMM_EPS * ((c + ec) @ w3sq.T) + ec @ w3sq.T
    return mean, var, mean_err, var_err


def propagate64(x, layers, biases, w3, w3sq, b3, dtype="f32", eps_relu=EPS_RELU):
    """Moment propagation in float64 with the engine's rounding points (a, q, c and the packed input to the operand type;
    products exact). layers: operands() per VB layer; biases: their fp32 biases; w3, w3sq: final_operands(); b3: the final bias.
    Returns (mean, var, mean_err, var_err): the R x W outputs and, per output, the bound of what an engine that keeps the GEMM
    bound per product and 4 eps_relu (scale-relative) per ReLU stage may differ by."""
    rnd = rounder(dtype)
    a = rnd(np.asarray(x, F))
    mom = (a, rnd((a.astype(F) * a.astype(F)).astype(D)), np.zeros_like(a))
    err = (np.zeros_like(a),) * 3
    for li, (op, b) in enumerate(zip(layers, biases)):
        mom, err = layer64(mom, err, op, b, li == 0, rnd, eps_relu)
    return final64(mom[0], mom[2], err[0], err[2], w3, w3sq, b3)


def propagate_network(x, params, w3, b3, dtype="f32", masks=None, eps_relu=EPS_RELU):
    """propagate64 from fp32 parameters: params = [(means, lvars, bias)] per VB layer, masks[li] (True = pruned) or None."""
    layers = [operands(mu, lv, dtype, None if masks is None else masks[li]) for li, (mu, lv, _) in enumerate(params)]
    w, wsq = final_operands(w3, dtype)
    return propagate64(x, layers, [p[2] for p in params], w, wsq, b3, dtype, eps_relu)


# ------------------------------------------------------------------------------------------------ one VB layer: the sampler
def sample_one_layer(x, means, lvars, bias, w3, b3, n, seed):
    """n draws of the engine's LRT sampler for a network with ONE VB layer, float64: y = m + sqrt(v) z per unit, h = max(0, y),
    out = h w3^T + b3. Returns n x R x W."""
    x, mu, var = np.asarray(x, D), np.asarray(means, D), np.exp(np.asarray(lvars, D))
    m, v = x @ mu.T + np.asarray(bias, D), (x * x) @ var.T
    z = np.random.default_rng(seed).standard_normal((n,) + m.shape)
    h = np.maximum(m + np.sqrt(v) * z, 0.0)
    return h @ np.asarray(w3, D).T + np.asarray(b3, D)


def moment_band(draws, sigmas=5.0):
    """From n x ... draws: (sample mean, its band, population variance, its band) -- `sigmas` standard errors of the mean and
    sigmas sqrt((m4 - var^2) / n) of the variance, m4 the sample's fourth central moment."""
    n = draws.shape[0]
    mean = draws.mean(0)
    d = draws - mean
    var = (d * d).mean(0)
    m4 = (d ** 4).mean(0)
    return mean, sigmas * np.sqrt(var / n), var, sigmas * np.sqrt(np.maximum(m4 - var * var, 0.0) / n)
