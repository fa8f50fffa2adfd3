"""NumPy restatement of vbnn_predict_quantiles (include/vbnn_hip.h) for the tests:
  * the EMPIRICAL kind in np.float32, operation for operation (bitwise what the kernel gives);
  * the mixture kinds' CDF and root in float64 (bisection to convergence) -- what the kernel is held against;
  * an fp32 restatement of the mixture CDF as the kernel evaluates it -- z = (mu - x) c in fp32, erfc in double rounded to fp32,
    a sequential fp32 sum over s, one correctly rounded division by 2 S -- and its root (adjacent floats lo < q with
    F32(lo) < p <= F32(q)): what tests/test_quantiles_ref.py measures EPS_F with;
  * the mixture input sets the CPU and the GPU tests share.
erfc comes from torch (CPU, float64)."""
import math

import numpy as np
import torch

EMPIRICAL, FIXED_NOISE, GAUSS = 0, 1, 2
f32 = np.float32

# The allowance for the fp32 evaluation of F: 4 x the largest value tests/test_quantiles_ref.py measures on the restatement over
# every mixture input set below (the factor: the device's erfcf / expf are a few ulp where the restatement's are correctly
# rounded). Measured: 4.39e-07 (fixed-5x33-S128; the S = 30 sets stay below 3.5e-07, the S = 1 sets below 4.1e-08).
EPS_F = 4 * 4.39e-07


def erfc64(z):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))).numpy()


# ---------------------------------------------------------------------------------------------------------------- EMPIRICAL
def empirical32(y, p, t=None):
    """y: S x R x D fp32; p: Q floats. Returns (q: Q x R x D fp32, pit: R x D fp32 or None)."""
    S = y.shape[0]
    bad = np.isnan(y).any(0)
    a = np.sort(np.where(np.isnan(y), f32(0), y), axis=0)
    q = np.empty((len(p),) + y.shape[1:], f32)
    for j, pj in enumerate(p):
        if S == 1:
            q[j] = a[0]
            continue
        pos = f32(pj) * f32(S - 1)
        k = min(int(pos), S - 2)
        frac = f32(pos - f32(k))
        lo, hi = a[k], a[k + 1]
        q[j] = np.minimum((lo + (frac * (hi - lo)).astype(f32)).astype(f32), hi)
    q[:, bad] = np.nan
    pit = None
    if t is not None:
        with np.errstate(invalid="ignore"):
            pit = ((y <= t[None]).sum(0).astype(f32) / f32(S)).astype(f32)
        pit[bad | np.isnan(t)] = np.nan
    return q, pit


# ---------------------------------------------------------------------------------------------------------------- mixtures
def components(y, kind, noise_var=None, s_min=None, s_max=None):
    """(mu, sigma) in float64, S x R x D each, of the fp32 inputs: the exact components the kernel is held against."""
    if kind == FIXED_NOISE:
        mu = y.astype(np.float64)
        return mu, np.full_like(mu, math.sqrt(float(f32(noise_var))))
    D = y.shape[2] // 2
    sc = np.clip(y[..., D:], f32(s_min), f32(s_max)).astype(np.float64)
    return y[..., :D].astype(np.float64), np.exp(0.5 * sc)


def cdf64(x, mu, sigma):
    """F(x) = 1/S sum_s Phi((x - mu_s) / sigma_s) in float64; x: R x D."""
    return 0.5 * erfc64((mu - x[None]) / (sigma * math.sqrt(2.0))).mean(0)


def root64(p, mu, sigma):
    lo, hi = (mu - 9 * sigma).min(0), (mu + 9 * sigma).max(0)
    for _ in range(120):
        mid = 0.5 * (lo + hi)
        below = cdf64(mid, mu, sigma) < p
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def c32(y, kind, noise_var=None, s_min=None, s_max=None):
    """(mu, c = 1 / (sigma sqrt 2)) in fp32 as the kernel forms them."""
    if kind == FIXED_NOISE:
        return y, np.full_like(y, f32(1.0 / math.sqrt(2.0 * float(f32(noise_var)))))
    D = y.shape[2] // 2
    sc = np.clip(y[..., D:], f32(s_min), f32(s_max))
    e = np.exp((f32(-0.5) * sc).astype(np.float64)).astype(f32)
    return y[..., :D], (e * f32(0.70710678)).astype(f32)


def cdf32(x, mu, c):
    """The kernel's evaluation of F at x (R x D fp32), with a correctly rounded erfc."""
    S = mu.shape[0]
    acc = np.zeros(x.shape, f32)
    for s in range(S):
        z = ((mu[s] - x).astype(f32) * c[s]).astype(f32)
        acc = (acc + erfc64(z).astype(f32)).astype(f32)
    return (acc / f32(2 * S)).astype(f32)


def key(x):
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)


def unkey(k):
    b = np.where(k & 0x80000000, k & 0x7FFFFFFF, (~k) & 0xFFFFFFFF).astype(np.uint32)
    return b.view(f32)


def root32(p, mu, c, sigma):
    """The upper of the two adjacent floats around the root of cdf32 (bisection on the ordered bit patterns)."""
    lo = key((mu.astype(np.float64) - 3.5 * sigma).min(0).astype(f32))
    hi = key((mu.astype(np.float64) + 3.5 * sigma).max(0).astype(f32))
    for _ in range(34):
        mid = np.where(hi - lo > 1, lo + (hi - lo) // 2, hi)
        below = cdf32(unkey(mid), mu, c) < f32(p)
        lo, hi = np.where((hi - lo > 1) & below, mid, lo), np.where((hi - lo > 1) & ~below, mid, hi)
    assert (hi - lo <= 1).all()
    return unkey(hi)


def step(x, n):
    """x moved n floats up (n > 0) or down."""
    x = np.ascontiguousarray(x, f32)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf))
    return x


def eps_needed(q, p, mu, sigma):
    """Per element, the smallest eps with F(q - 2 ulp) - eps <= p <= F(q + 2 ulp) + eps for the float64 F: how much error the
    evaluation of F must be allowed for the exact root to lie within 2 fp32 ulps of q."""
    below = cdf64(step(q, -2).astype(np.float64), mu, sigma) - p
    above = p - cdf64(step(q, 2).astype(np.float64), mu, sigma)
    return np.maximum(0.0, np.maximum(below, above))


# ---------------------------------------------------------------------------------------------------------------- input sets
P3 = (0.05, 0.5, 0.95)
P2 = (0.001, 0.999)
P8 = (0.001, 0.025, 0.1, 0.3, 0.5, 0.9, 0.975, 0.999)

# name: (kind, R, D, S, p, mean offset, (s_min, s_max) of the clamp, (low, high) of the s drawn)
MIXTURE_CASES = {
    "fixed-8x12-S30": (FIXED_NOISE, 8, 12, 30, P3, 0.0, None, None),
    "fixed-37x7-S1": (FIXED_NOISE, 37, 7, 1, P2, 100.0, None, None),
    "fixed-5x33-S128": (FIXED_NOISE, 5, 33, 128, P8, 0.0, None, None),
    "gauss-8x12-S30": (GAUSS, 8, 12, 30, P3, 0.0, (-20.0, 20.0), (-20.0, 3.0)),
    "gauss-8x13-S30": (GAUSS, 8, 13, 30, P3, 100.0, (-6.0, 2.0), (-12.0, 4.0)),      # clamped on both sides
    "gauss-37x7-S1": (GAUSS, 37, 7, 1, P2, 100.0, (-12.0, 3.0), (-14.0, 4.0)),
    "gauss-5x33-S128": (GAUSS, 5, 33, 128, P8, 0.0, (-20.0, 20.0), (-20.0, 3.0)),
    "fixed-calibration": (FIXED_NOISE, 200, 200, 30, P3, 0.0, None, None),
    "gauss-calibration": (GAUSS, 200, 200, 30, P3, 0.0, (-20.0, 20.0), (-6.0, 1.0)),
}
NOISE_VAR = 0.3


def mixture_case(name):
    """(y: S x R x W fp32, t: R x D fp32 drawn from the mixture itself, kind, p, kwargs of the kind). Every component keeps
    sigma >= 32 ulp(|mu|), so the 2-ulp criterion tests the solver and not the grid."""
    kind, R, D, S, p, offset, clamp, srange = MIXTURE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    centre = rng.standard_normal((1, R, D))
    m = (offset + centre + 0.7 * rng.standard_normal((S, R, D))).astype(f32)
    if kind == GAUSS:
        s = rng.uniform(srange[0], srange[1], (S, R, D)).astype(f32)
        y = np.concatenate([m, s], 2)
        kw = dict(s_min=clamp[0], s_max=clamp[1])
    else:
        y, kw = m, dict(noise_var=NOISE_VAR)
    mu, sigma = components(y, kind, **kw)
    assert (sigma >= 32 * np.spacing(np.abs(mu).astype(f32))).all()
    pick = rng.integers(0, S, (R, D))
    rr, dd = np.meshgrid(np.arange(R), np.arange(D), indexing="ij")
    t = (mu[pick, rr, dd] + sigma[pick, rr, dd] * rng.standard_normal((R, D))).astype(f32)
    return y, t, kind, p, kw
