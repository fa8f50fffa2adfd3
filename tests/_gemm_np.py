"""A float64 NumPy reference of the three GEMM families of the layer (vbnn_forward, vbnn_grad_input, vbnn_acc_grad_parameters),
restated from the contract in include/vbnn_hip.h and from VBLinear.lua as that header cites it -- not from the kernels' epilogues.
TEST INFRASTRUCTURE ONLY. The module also holds the per-element bounds the GPU tests use and the interval rule for bf16 stores.

Operations (all in float64 on the values the caller hands over; nothing here rounds):

  forward          m = x w^T (+ b),  v = (x.x) (sigma^2)^T,  y = m + sqrt(v) z,  r = z / (2 sqrt v) and 0 where v == 0,
                   h = relu?(y); h2 is the square of the STORED h, so it is formed by the caller from what the kernel stored.
  noise            z[n][o] is lane o & 3 of the contract's normals at (seed, ZETA, layer, draw, row, o >> 2) with
                   (draw, row) = (draw + draw_dev, row0 + n), or under rows_per_draw = rpd > 0
                   (draw + draw_dev + n // rpd, row0 + n % rpd): `zeta` below assembles it from a fill(rows, cols, draw, row0).
  grad_input       gx = g w  (WN)  or  g mu + 2 x . (gv sigma^2)  (LRT);  g_prev = gx . [x > 0];  gv_prev = g_prev . r_prev
                   from the UNROUNDED g_prev.
  acc_grad         gradWeight (+)= scale g^T x;  gradBias (+)= scale sum_n g;
                   gradSum (+)= (g^T x) . e (WN)  or  2 (gv^T x.x) . stdv (LRT), stdv = exp(lvars / 2);
                   grad_mu = scale (g^T x) / S + kl_scale means / (B var_hat)               (VBLinear.lua:90-93)
                   grad_lv = (gv^T x.x) vars / S + kl_scale (vars / var_hat - 1) / (2 B)    (VBLinear.lua:95-98, LRT units)
                          or (g^T x) . e . stdv / (2 S) + the same KL term                   (WN)
                   with accumulate = 1: the likelihood part is ADDED to the old value and the KL term is left out (it counts on
                   the first draw only). means / vars are the fp32 parameters or, when given, the bf16 shadows (stdv, of gradSum
                   and of the weight-noise likelihood part, stays exp(lvars / 2) of the fp32 parameter). part = 1 / 2
                   writes only what depends on the first / second GEMM.

BOUNDS. u = 2^-24 is the unit roundoff of fp32; an fp32 operation on exact inputs is within u of its result, relatively. Every
bound is a sum over the operations BETWEEN the exact accumulators and the stored value, counted as the contract states them;
SLACK = 1 + 2^-18 covers the second-order terms. None is fitted to a kernel.

  LRT forward, the accumulators m, v exact (the integer tier). The epilogue is: mb = m + b (exact there: a dyadic bias);
  rs = rsq(v), stated at 1 ulp = 2u; sd = v rs (one multiply, u); y = fma(sd, z, mb) (u).
      |y - y_ref| <= u (3 |sqrt(v) z| + |y_ref|)                                           bound_y
  r = (0.5 z) rs: the halving is exact, rs carries 2u, one multiply u:
      |r - r_ref| <= 3 u |r_ref|                                                           bound_r
  Where the first GEMM is accumulated ON TOP of b + sqrt(v) z (the two-pass kernel's fold) the sum m is no longer exact: the
  accumulation-order bound of the real tier, ACC_REL times (|b + sqrt(v) z| + |x| |w|^T), is added by the caller (accum_bound).

  accGradParameters, guarded epilogue, fp32 parameters: var = expf(lvars) (1 ulp = 2u), stdv = sqrtf(var) (correctly rounded:
  u on top of half of var's 2u).
      gradSum  = fma(2 a2, stdv, old):            u (2 |2 a2 stdv| + |gradSum|)            bound_grad_sum
  The fused total gradients: invS = 1 / S (u; exact for a power of two, counted anyway), var_hat = (float) stats[2] (u),
  k_mu = kl / (B var_hat) (product u, divide u, var_hat u: 3u), k_lv = kl / (2 B) (u), inv_vh = 1 / var_hat (2u).
      lm = (scale a1) invS: two multiplies and invS: 3u.    grad_mu = fma(k_mu, mu, lm) (u):
                                                  u (3 |lm| + 3 |k_mu mu| + |grad_mu|)     bound_grad_mu
      ll = (a2 var) invS: 3u and var's 2u (0 from a shadow).  t = fma(var, inv_vh, -1): u (4 |var / var_hat| + |t|).
      grad_lv = fma(k_lv, t, ll):                 u (5 |ll| + |k_lv| (4 |var / var_hat| + 2 |t|) + |grad_lv|)   bound_grad_lv
  With accumulate = 1 the KL terms vanish and one add joins: u (3 |lm| + |result|), u (5 |ll| + |result|).
  WN: e is the contract's bit-exact normal, gradSum = old + a1 e: u (|a1 e| + |gradSum|) whether the compiler fuses the pair or
  not; grad_lv's likelihood part a1 e stdv (0.5 invS) is four multiplies on stdv's 2u: 6u.

  Real tier (bf16-rounded normal operands): the accumulation-order bound the project already uses, per element from |A| |B|:
  ACC_REL = 4e-6 (tests/test_parity_gpu.py's gemm_tol(absprod, 4e-6)), plus ACC_ABS = 1e-12.

BF16 STORES. A stored value is right when it is the bf16 rounding (nearest, ties to even) of SOME value in [ref - e, ref + e]:
rounding is monotone, so that is bf16(ref - e) <= stored <= bf16(ref + e) (interval_ok). No operand seed has to avoid rounding
midpoints. far_side counts the accepted elements that are not bf16(ref) itself."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -18
ACC_REL, ACC_ABS = 4e-6, 1e-12
f8 = np.float64


# ---------------------------------------------------------------- bf16 rounding and the interval rule
def bf16_rne(a):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64; no double rounding through fp32.
    (Normal range only: the tests' values are far from bf16's subnormals and from its overflow.)"""
    a = np.asarray(a, f8)
    _, e = np.frexp(a)                                  # |a| = f 2^e, f in [0.5, 1)
    ulp = np.ldexp(1.0, e - 8)
    return np.where(a == 0, a, np.round(a / ulp) * ulp)  # np.round: half to even


def interval_ok(stored, ref, e):
    """element-wise: `stored` (float64 view of bf16 values) is the bf16 rounding of some value in [ref - e, ref + e]"""
    stored, ref, e = np.asarray(stored, f8), np.asarray(ref, f8), np.asarray(e, f8)
    return (stored >= bf16_rne(ref - e)) & (stored <= bf16_rne(ref + e))


def far_side(stored, ref):
    """how many stored values are not bf16(ref) itself (they landed on the far side of a rounding midpoint)"""
    return int((np.asarray(stored, f8) != bf16_rne(ref)).sum())


# ---------------------------------------------------------------- noise addressing
def noise_address(N, draw, row0, rows_per_draw=0, draw_dev=0):
    """(draw, row) of the normals of operand rows 0 .. N - 1"""
    n = np.arange(N, dtype=np.int64)
    if rows_per_draw > 0:
        return draw + draw_dev + n // rows_per_draw, row0 + n % rows_per_draw
    return np.full(N, draw + draw_dev, np.int64), row0 + n


def zeta(fill, N, O, draw, row0, rows_per_draw=0, draw_dev=0):
    """N x O normals of a forward: fill(rows, cols, draw, row0) -> rows x cols of the contract's normals for ONE draw"""
    d, r = noise_address(N, draw, row0, rows_per_draw, draw_dev)
    out = np.empty((N, O), f8)
    for dd in np.unique(d):
        sel = np.nonzero(d == dd)[0]                    # consecutive rows r[sel[0]] .. of draw dd
        assert (np.diff(r[sel]) == 1).all()
        out[sel] = fill(len(sel), O, int(dd), int(r[sel[0]]))
    return out


# ---------------------------------------------------------------- the three families
def forward(x, w, bias=None, w2=None, x2=None, z=None, relu=False):
    """dict(m, v, y, r, h): m includes the bias; v, r are None for the single GEMM (WN / MAP)"""
    x, w = np.asarray(x, f8), np.asarray(w, f8)
    m = x @ w.T + (0.0 if bias is None else np.asarray(bias, f8))
    if w2 is None:
        v = r = None
        y = m
    else:
        x2 = x * x if x2 is None else np.asarray(x2, f8)
        v = x2 @ np.asarray(w2, f8).T
        sd = np.sqrt(v)
        z = np.asarray(z, f8)
        y = m + sd * z
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(v > 0, z / (2.0 * sd), 0.0)
    return dict(m=m, v=v, y=y, r=r, h=np.maximum(y, 0.0) if relu else y)


def head_logits(h_stored, w3):
    """the head's slots summed: the STORED h times the final weight"""
    return np.asarray(h_stored, f8) @ np.asarray(w3, f8).T


def grad_input(g, w, gv=None, w2=None, x=None, relu_mask=False, r_prev=None):
    """dict(gx, g_prev, gv_prev): w, w2 are O x I (mu, sigma^2); g, gv N x O; x, r_prev N x I"""
    g, w = np.asarray(g, f8), np.asarray(w, f8)
    gx = g @ w
    if gv is not None:
        gx = gx + 2.0 * np.asarray(x, f8) * (np.asarray(gv, f8) @ np.asarray(w2, f8))
    g_prev = np.where(np.asarray(x, f8) > 0, gx, 0.0) if relu_mask else gx
    gv_prev = g_prev * (0.0 if r_prev is None else np.asarray(r_prev, f8))
    return dict(gx=gx, g_prev=g_prev, gv_prev=gv_prev)


def acc_grad(x, g, gv=None, x2=None, scale=1.0, lvars=None, e=None, means=None, var_hat=None, B=1.0, S=1.0, kl_scale=0.0,
             mu_s=None, var_s=None, old=None, part=0):
    """dict(a1, a2, gradWeight, gradBias, gradSum, grad_mu, grad_lv) of one call; `old` (dict of the same names) = accumulate 1.
    LRT when gv is given (a2 = gv^T x.x), WN otherwise (needs e for gradSum / grad_lv). Outputs a part does not write are None."""
    x, g = np.asarray(x, f8), np.asarray(g, f8)
    a1 = g.T @ x
    lrt = gv is not None
    a2 = np.asarray(gv, f8).T @ (x * x if x2 is None else np.asarray(x2, f8)) if lrt else None
    acc = old is not None
    prev = (lambda k: np.asarray(old[k], f8)) if acc else (lambda k: 0.0)
    out = dict(a1=a1, a2=a2, gradWeight=None, gradBias=None, gradSum=None, grad_mu=None, grad_lv=None)
    var = None
    if var_s is not None:
        var = np.asarray(var_s, f8)
    elif lvars is not None:
        var = np.exp(np.asarray(lvars, f8))
    if part != 2:
        out["gradWeight"] = prev("gradWeight") + scale * a1
        out["gradBias"] = prev("gradBias") + scale * g.sum(axis=0)
    if part != 1 and (lrt or e is not None) and lvars is not None:
        stdv = np.exp(np.asarray(lvars, f8) / 2.0)
        out["gradSum"] = prev("gradSum") + (2.0 * a2 * stdv if lrt else a1 * np.asarray(e, f8))
    if var_hat is not None:
        mu = np.asarray(mu_s if mu_s is not None else means, f8)
        if part != 2:
            out["grad_mu"] = scale * a1 / S + (prev("grad_mu") if acc else kl_scale * mu / (B * var_hat))
        if part != 1:
            # (weight noise: stdv is exp(lvars / 2) of the fp32 parameter even when the shadows are given, as gradSum's is)
            lik = a2 * var / S if lrt else a1 * np.asarray(e, f8) * np.exp(np.asarray(lvars, f8) / 2.0) / (2.0 * S)
            out["grad_lv"] = lik + (prev("grad_lv") if acc else kl_scale * (var / var_hat - 1.0) / (2.0 * B))
    return out


# ---------------------------------------------------------------- bounds
def bound_y(fw):
    """LRT forward, exact accumulators: see the module docstring"""
    sdz = np.abs(fw["y"] - fw["m"])
    return U * SLACK * (3.0 * sdz + np.abs(fw["y"]))


def bound_r(fw):
    return 3.0 * U * SLACK * np.abs(fw["r"])


def accum_bound(absprod):
    """accumulation-order bound of a sum whose terms' absolute values add up to absprod"""
    return ACC_REL * np.asarray(absprod, f8) + ACC_ABS


def bound_grad_sum(a2, lvars, result):
    return U * SLACK * (2.0 * np.abs(2.0 * a2 * np.exp(np.asarray(lvars, f8) / 2.0)) + np.abs(result))


def bound_grad_sum_wn(a1, e, result):
    return U * SLACK * (np.abs(a1 * e) + np.abs(result))


def bound_grad_mu(a1, mu, scale, S, B, var_hat, kl_scale, result, accumulate=False):
    lm = np.abs(scale * a1 / S)
    kl = 0.0 if accumulate else np.abs(kl_scale * np.asarray(mu, f8) / (B * var_hat))
    return U * SLACK * (3.0 * lm + 3.0 * kl + np.abs(result))


def bound_grad_lv(a2, var, S, B, var_hat, kl_scale, result, accumulate=False, var_exact=False):
    ll = np.abs(a2 * var / S)
    t = var / var_hat - 1.0
    kl = 0.0 if accumulate else np.abs(kl_scale / (2.0 * B)) * (4.0 * np.abs(var / var_hat) + 2.0 * np.abs(t))
    return U * SLACK * ((3.0 if var_exact else 5.0) * ll + kl + np.abs(result))


def bound_grad_lv_wn(a1, e, lvars, var, S, B, var_hat, kl_scale, result, accumulate=False):
    ll = np.abs(a1 * e * np.exp(np.asarray(lvars, f8) / 2.0) / (2.0 * S))
    t = var / var_hat - 1.0
    kl = 0.0 if accumulate else np.abs(kl_scale / (2.0 * B)) * (4.0 * np.abs(var / var_hat) + 2.0 * np.abs(t))
    return U * SLACK * (6.0 * ll + kl + np.abs(result))


# ---------------------------------------------------------------- fp32 restatements, op by op (tests/test_gemm_ref.py)
f4 = np.float32


def _fma32(a, b, c):
    """fmaf: the product of two fp32 values is exact in float64; the sum is rounded once to float64 and once to fp32"""
    return (np.asarray(a, f8) * np.asarray(b, f8) + np.asarray(c, f8)).astype(f4)


def _rsq32(v):
    """a correctly rounded reciprocal square root (the contract allows 1 ulp)"""
    with np.errstate(divide="ignore"):
        return (1.0 / np.sqrt(np.asarray(v, f8))).astype(f4)


def forward_f32(m, v, bias, z):
    """the LRT epilogue in fp32 on exact accumulators: mb = m + b, rs = rsq(v), sd = v rs, y = fma(sd, z, mb), r = (0.5 z) rs"""
    m, v, z = np.asarray(m, f4), np.asarray(v, f4), np.asarray(z, f4)
    mb = (m + np.asarray(bias, f4)).astype(f4)
    rs = _rsq32(v)
    with np.errstate(invalid="ignore"):
        sd = np.where(v > 0, (v * rs).astype(f4), f4(0))
    y = _fma32(sd, z, mb)
    r = np.where(v > 0, ((f4(0.5) * z).astype(f4) * rs).astype(f4), f4(0))
    return y, r


def acc_grad_f32(a1, a2, lvars, means, var_hat, scale, B, S, kl_scale, old=None):
    """the guarded LRT accGradParameters epilogue in fp32: gradSum, grad_mu, grad_lv from exact accumulators"""
    a1, a2 = np.asarray(a1, f4), np.asarray(a2, f4)
    var = np.exp(np.asarray(lvars, f8)).astype(f4)                       # a correctly rounded expf
    sd = np.sqrt(var.astype(f8)).astype(f4)
    vh, S4, B4, kl4, sc = f4(var_hat), f4(S), f4(B), f4(kl_scale), f4(scale)
    invS = f4(f4(1) / S4)
    k_mu = f4(kl4 / f4(B4 * vh))
    k_lv = f4(kl4 / f4(f4(2) * B4))
    inv_vh = f4(f4(1) / vh)
    o = (lambda k: np.asarray(old[k], f4)) if old is not None else (lambda k: f4(0))
    grad_sum = _fma32((f4(2) * a2).astype(f4), sd, o("gradSum"))
    lm = ((sc * a1).astype(f4) * invS).astype(f4)
    ll = ((a2 * var).astype(f4) * invS).astype(f4)
    if old is not None:
        return grad_sum, (lm + o("grad_mu")).astype(f4), (ll + o("grad_lv")).astype(f4)
    return grad_sum, _fma32(k_mu, np.asarray(means, f4), lm), _fma32(k_lv, _fma32(var, inv_vh, f4(-1)), ll)
