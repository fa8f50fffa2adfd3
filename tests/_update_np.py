"""NumPy restatement of the parameter update: optim.hip's k_adam / k_sgd and elementwise.hip's k_vb_update / k_update_finish,
statement for statement, plus a float64 form of the same quantities. NumPy only; nothing here reads GPU code or a GPU tensor.

Every float32 statement is one NumPy float32 operation (one rounding, as the kernels are built with -ffp-contract=off and
hipcc's fp32 divide and sqrtf are correctly rounded). An explicit fmaf is one rounding of the exact a b + c (fma_f32). The
hyper-parameters reach the kernels as floats: they are rounded to float32 first and widened for the double expressions of the
step size, as the host code does. Only exp() is not reproducible bit for bit; it can be swapped (`exp=`) for a rounded-down or
rounded-up form, which is how the tests bound what depends on it."""
import math

import numpy as np

F = np.float32
FIELDS = ("means", "lvars", "m_mu", "v_mu", "m_lv", "v_lv")


# ------------------------------------------------------------------------------------------------ formats
def bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even by integer arithmetic on the float32 bits; a NaN stays
    a (quiet) NaN with its sign."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x))


def step_ulps(x, k):
    """Positive finite float32 values moved by k units in the last place (k may be negative)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) + int(k)
    assert (b > 0).all() and (b < 0x7F800000).all()
    return b.astype(np.int32).view(np.float32)


def exp32(l):
    """The float32 rounding of the float64 exponential: within half an ulp (and the libm's error, ~2^-53) of the true value."""
    return np.exp(np.asarray(l, np.float32).astype(np.float64)).astype(np.float32)


def exp_shifted(k):
    """exp32 moved by k ulp: the lower / upper end of an expf allowance of |k| ulp."""
    return lambda l: step_ulps(exp32(l), k)


def fma_f32(a, b, c):
    """fmaf(a, b, c): ONE rounding of the exact a b + c. The product of two float32 is exact in float64; the sum is rounded
    to odd in float64 (TwoSum gives its error exactly), which a final rounding to float32 cannot see (53 >= 2 x 24 + 2)."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


# ------------------------------------------------------------------------------------------------ Adam / SGD
def adam_cfg(lr, t, beta1=0.9, beta2=0.999, eps=1e-8, lambda_=1.0):
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, lambda_=lambda_, t=int(t))


def adam_consts(cfg):
    """(b1_t, b2, eps, step) as floats, and the same four in double: the host expressions of vbnn_adam_step / vbnn_update on the
    float32-rounded hyper-parameters widened to double."""
    lr, b1, b2, eps, lam = (float(F(cfg[k])) for k in ("lr", "beta1", "beta2", "eps", "lambda_"))
    t = int(cfg["t"])
    b1t = b1 * math.pow(lam, float(t - 1))
    bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
    step = lr * math.sqrt(bc2) / bc1
    return (F(b1t), F(b2), F(eps), F(step)), (b1t, b2, eps, step)


def adam_f32(x, g1, g2, m, v, cfg):
    """k_adam's statements in float32. Returns new x, m, v and the applied update."""
    (b1, b2, eps, step), _ = adam_consts(cfg)
    x, g1, m, v = (np.asarray(a, np.float32) for a in (x, g1, m, v))
    g = g1 if g2 is None else g1 + np.asarray(g2, np.float32)
    one = F(1.0)
    m2 = b1 * m + (one - b1) * g
    v2 = b2 * v + (one - b2) * g * g
    up = step * m2 / (np.sqrt(v2) + eps)
    return x - up, m2, v2, up


def adam_f64(x, g1, g2, m, v, cfg):
    """The same step in float64 (inputs widened, hyper-parameters the float32-rounded ones, the step size left in double)."""
    _, (b1, b2, eps, step) = adam_consts(cfg)
    x, g1, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (x, g1, m, v))
    g = g1 if g2 is None else g1 + np.asarray(g2, np.float32).astype(np.float64)
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    up = step * m2 / (np.sqrt(v2) + eps)
    return x - up, m2, v2, up


def adam_bound(x64, g, m, v2_64, cfg):
    """|x'_32 - x'_64| <= 2^-24 |x'| + 8 2^-24 step (|b1 m| + |(1 - b1) g|) / (sqrt(v') + eps): the final rounding, and the
    eight roundings ahead of it (g, two products and the sum of m', the product, the root, the sum and the quotient of the
    update; what v' carries is halved by the root) applied to the update's magnitude with |m'| replaced by the sum of the
    magnitudes of its two terms, so that cancellation in m' does not shrink the bound."""
    _, (b1, b2, eps, step) = adam_consts(cfg)
    g, m = np.asarray(g, np.float64), np.asarray(m, np.float64)
    u = 2.0 ** -24
    return u * np.abs(x64) + 8 * u * step * (np.abs(b1 * m) + np.abs((1.0 - b1) * g)) / (np.sqrt(v2_64) + eps)


def sgd_f32(x, g, lr):
    """k_sgd and the bias step of k_update_finish: x = fmaf(-lr, g, x)."""
    return fma_f32(-F(lr), g, x)


def adam_norms(up, x_new):
    """{ |update|, |x_new| } as k_adam / k_norm_finish form them: float64 sums of the float32 values' squares."""
    s = lambda a: math.sqrt(float(np.sum(np.asarray(a, np.float32).astype(np.float64) ** 2)))
    return s(up), s(x_new)


# ------------------------------------------------------------------------------------------------ the update sweep
def prior_terms(m, v):
    """exp(lvars) + means^2 as the sweeps form it: float32(v + float32(m m))."""
    m, v = np.asarray(m, np.float32), np.asarray(v, np.float32)
    return v + m * m


def prior_stats(means, lvars, keep=None, exp=exp32):
    """The four statistics a vbnn_prepare leaves (the input of an update): sums over the kept weights, var_hat, the count."""
    k = np.ones(means.shape, bool) if keep is None else keep
    s0 = float(np.sum(prior_terms(means[k], exp(lvars[k])).astype(np.float64)))
    s1 = float(np.sum(lvars[k].astype(np.float64)))
    return _stats(s0, s1, float(k.sum()), means.size, keep is not None)


def _stats(s0, s1, n, W, masked):
    if masked:                                                       # masked_stats (elementwise.hip)
        if n == 0.0:
            return np.zeros(4)
        return np.array([s0, s1, (1.0 / W) * s0 if n == W else s0 / n, n])
    return np.array([s0, s1, (1.0 / n) * s0, n])


def finish(tot, W, var_hat_old, n_total=None, masked=False):
    """k_update_finish on the 16 totals: the four statistics and the 14 logged series. W is the kept count of a masked layer."""
    W = float(W)
    nl, nm = math.sqrt(tot[5]), math.sqrt(tot[3])
    mean = tot[11] / W
    std = math.sqrt(max(0.0, (tot[3] - W * mean * mean) / (W - 1.0))) if W > 1.0 else 0.0
    log14 = np.array([math.sqrt(tot[8]) / nl, math.sqrt(tot[9]) / nl, math.sqrt(tot[6]) / nm, math.sqrt(tot[7]) / nm,
                      tot[12], tot[13], tot[10] / W, var_hat_old, mean, std, tot[14], tot[15],
                      math.sqrt(tot[2]) / nm, math.sqrt(tot[4]) / nl])
    return _stats(tot[0], tot[1], W, W if n_total is None else n_total, masked), log14


def _totals(t, um, m, ul, l, mlc, mle, vlc, vle, v):
    d = lambda a: np.asarray(a).astype(np.float64)
    sq = lambda a: float(np.sum(d(a) * d(a)))
    return np.array([float(np.sum(d(t))), float(np.sum(d(l))), sq(um), sq(m), sq(ul), sq(l), sq(mlc), sq(mle), sq(vlc), sq(vle),
                     float(np.sum(d(v))), float(np.sum(d(m))), float(np.min(v)), float(np.max(v)), float(np.min(m)), float(np.max(m))])


def _update_layer(state, cfg_mu, cfg_lv, B, kl_add, mask, exp, wide):
    keep = np.ones(state["means"].shape, bool) if mask is None else (np.asarray(mask) == 0)
    T = np.float64 if wide else np.float32
    c_mu, c_lv = (adam_consts(c)[1 if wide else 0] for c in (cfg_mu, cfg_lv))
    one, two = T(1.0), T(2.0)
    Bt, kl = T(F(B)), T(F(kl_add))
    sel = lambda k: np.asarray(state[k], np.float32)[keep].astype(T)
    m, l, gm, gl, mm, vm, ml, vl = (sel(k) for k in ("means", "lvars", "g_mu", "g_lv", "m_mu", "v_mu", "m_lv", "v_lv"))
    ex = (lambda a: np.exp(a)) if wide else exp
    var_hat_old = float(state["stats"][2])
    var_hat = T(F(var_hat_old))                                      # const float var_hat = (float)a.stats[2]
    k_mu, k_lv, inv_vh = one / (Bt * var_hat), one / (two * Bt), one / var_hat
    mlc = k_mu * m
    e0 = ex(l)
    vlc = k_lv * (e0 * inv_vh - one if wide else fma_f32(e0, inv_vh, F(-1.0)))
    if float(kl) != 0.0:                                             # the KL part joins the likelihood gradients here
        if wide or float(kl) == 1.0:                                 # fmaf(1, a, b) is the plain sum
            gm, gl = kl * mlc + gm, kl * vlc + gl
        else:
            gm, gl = fma_f32(kl, mlc, gm), fma_f32(kl, vlc, gl)
    mle, vle = gm - mlc, gl - vlc

    def adam(x, g, m1, v1, c):
        b1, b2, eps, step = (T(q) for q in c)
        m2 = b1 * m1 + (one - b1) * g
        v2 = b2 * v1 + (one - b2) * g * g
        up = step * m2 / (np.sqrt(v2) + eps)
        return x - up, m2, v2, up

    m_n, mm, vm, um = adam(m, gm, mm, vm, c_mu)
    l_n, ml, vl, ul = adam(l, gl, ml, vl, c_lv)
    v_n = ex(l_n)
    terms = v_n + m_n * m_n                                          # float32(v + float32(m m))
    out = {}
    for k, new in (("means", m_n), ("lvars", l_n), ("m_mu", mm), ("v_mu", vm), ("m_lv", ml), ("v_lv", vl)):
        full = np.asarray(state[k], np.float32).astype(T).copy()    # a pruned weight is frozen: parameters and moments keep their bits
        full[keep] = new
        out[k] = full
    for k, new in (("mu_s", m_n), ("var_s", v_n), ("terms", terms), ("um", um), ("ul", ul), ("g_mu_total", gm), ("g_lv_total", gl)):
        full = np.zeros(keep.shape, T)                               # a pruned weight's shadows receive +0; it enters no sum
        full[keep] = new
        out[k] = full
    out["keep"] = keep
    n_kept = int(keep.sum())
    if n_kept == 0:
        out["tot"], out["stats"], out["log14"] = None, np.zeros(4), None
        return out
    out["tot"] = _totals(terms, um, m_n, ul, l_n, mlc, mle, vlc, vle, v_n)
    out["stats"], out["log14"] = finish(out["tot"], n_kept, var_hat_old, keep.size, mask is not None)
    return out


def update_layer_f32(state, cfg_mu, cfg_lv, B, kl_add, mask=None, exp=exp32):
    """elem4 of k_vb_update op for op in float32 on a dict of O x I float32 arrays (means, lvars, g_mu, g_lv, m_mu, v_mu,
    m_lv, v_lv) and `stats` (the four PRE-update statistics). Returns the new parameters and moments, both shadows as
    float32, the per-weight prior terms, the applied updates, the 16 totals in float64 and, from those, the four statistics
    and the 14 series exactly as k_update_finish forms them. mask (non-zero = pruned) freezes weights: their shadows are +0,
    they enter no sum, and the kept count stands in for W."""
    return _update_layer(state, cfg_mu, cfg_lv, B, kl_add, mask, exp, False)


def update_layer_f64(state, cfg_mu, cfg_lv, B, kl_add, mask=None):
    """The same quantities in float64, from the same float32 inputs and float32-rounded hyper-parameters (var_hat too enters
    as the kernel's float); no intermediate is rounded to float32."""
    return _update_layer(state, cfg_mu, cfg_lv, B, kl_add, mask, None, True)


# series whose terms hold no exp(): |KL part of the means' gradient|, |its likelihood part|, the old var_hat, mean / std / min /
# max of the new means, the means' norm ratio -- and, when the sweep does not add the KL gradient itself, the lvars' norm ratio
def series_without_exp(kl_add):
    return (2, 3, 7, 8, 9, 10, 11, 12) + ((13,) if float(kl_add) == 0.0 else ())


def make_state(O, I, seed=5, zero_moments=False):
    """One layer's inputs at the scales of the fine-tuning tests' State: non-zero Adam moments, a few exact-zero gradients
    and (zero_moments, for t = 1) a few weights whose moments are still zero."""
    r = np.random.RandomState(seed)
    n = lambda *s: r.standard_normal(s).astype(np.float32)
    st = dict(means=F(0.1) * n(O, I), lvars=F(np.log(1e-2)) + F(0.6) * n(O, I), g_mu=F(1e-2) * n(O, I), g_lv=F(1e-2) * n(O, I),
              m_mu=F(1e-3) * n(O, I), m_lv=F(1e-3) * n(O, I), v_mu=F(1e-5) * np.abs(n(O, I)) + F(1e-7),
              v_lv=F(1e-5) * np.abs(n(O, I)) + F(1e-7), bias=F(0.1) * n(O), g_bias=F(1e-2) * n(O))
    W = O * I
    flat = lambda k: st[k].reshape(-1)
    if W < 16:                                                       # too few weights to give some away
        st["stats"] = prior_stats(st["means"], st["lvars"])
        return st
    for k, stride, off in (("g_mu", 7, 0), ("g_lv", 11, 1)):         # exact-zero gradients, the first and the last weight among them
        flat(k)[off::W // stride] = 0.0
        flat(k)[W - 1] = 0.0
    if zero_moments:
        for k in ("m_mu", "v_mu", "m_lv", "v_lv"):
            flat(k)[::W // 5] = 0.0                          # (weight 0: zero gradient of the means AND zero moments)
            flat(k)[W // 2] = 0.0
    st["stats"] = prior_stats(st["means"], st["lvars"])
    return st


# The relative distance of each of the 14 series between update_layer_f32 and update_layer_f64, measured on the CPU (worst over
# the layers 1x1, 5x7, 70x50, 128x192, kl_add 0 and 1, (t, lambda) = (1, 1) and (1000, 0.999); rounded up to two digits;
# test_update_ref.py re-measures it and fails if the record is below the measurement or more than twice above it):
#   1.96e-07 5.24e-07 4.93e-08 5.57e-08 2.57e-07 1.69e-07 1.69e-07 0 4.68e-07 6.65e-09 4.31e-08 4.31e-08 1.55e-07 1.35e-07
# A series whose terms hold the device's expf is allowed SERIES_TOL = 4 x this against the restatement; the others 1e-10.
SERIES_DIST = np.array([2.0e-07, 5.3e-07, 5.0e-08, 5.6e-08, 2.6e-07, 1.7e-07, 1.7e-07, 0.0, 4.7e-07, 6.7e-09, 4.4e-08, 4.4e-08,
                        1.6e-07, 1.4e-07])
SERIES_TOL = 4.0 * SERIES_DIST
