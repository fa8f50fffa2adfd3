"""CPU tests of the restatement the sampling-free predictive is held against (tests/_propagate_np.py): the float64 moments of a
rectified Gaussian against quadrature, the fp32 restatement's error against float64 (EPS_RELU), and the one-VB-layer case against
the LRT sampler itself -- the reference alone stays inside the band the GPU test uses."""
import numpy as np

from tests import _propagate_np as P


def _quadrature(m, s):
    """E[h], E[h^2] of h = max(0, m + s z) by Gauss-Legendre (16 points per panel of width 1/4) over z in [max(-m/s, -40), 40]:
    the integrand is smooth there (the kink of the ReLU is the interval's end)."""
    lo = max(-m / s, -40.0)
    if lo >= 40.0:
        return 0.0, 0.0
    t, w = np.polynomial.legendre.leggauss(16)
    edges = np.arange(lo, 40.0 + 0.25, 0.25)
    z = (edges[:-1, None] + 0.125 * (t[None, :] + 1.0)).ravel()
    wz = np.tile(0.125 * w, len(edges) - 1)
    y = m + s * z
    pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    return float((wz * y * pdf).sum()), float((wz * y * y * pdf).sum())


def test_float64_formulas_match_quadrature_on_the_grid():
    worst = 0.0
    for s in P.SCALES:
        for al in P.ALPHAS:
            m, v = al * s, s * s
            a, q, c = (float(np.ravel(t)[0]) for t in P.relu_moments64(m, v))
            qa, qq = _quadrature(m, s)
            sc = max(s, abs(m))
            errs = (abs(a - qa) / sc, abs(q - qq) / sc ** 2, abs(c - max(qq - qa * qa, 0.0)) / sc ** 2)
            worst = max(worst, *errs)
            assert max(errs) <= 1e-12, (al, s, errs)
            assert a >= 0 and q >= 0 and c >= 0
    print(f"float64 formulas against quadrature: largest scale-relative error {worst:.3e}")
    m = np.array([-3.0, -0.0, 0.0, 2.5])
    a, q, c = P.relu_moments64(m, np.zeros(4))
    assert np.array_equal(a, np.maximum(m, 0)) and np.array_equal(q, a * a) and not c.any()


def test_fp32_restatement_error_is_eps_relu():
    """Measured: the largest scale-relative error of relu_moments32 against float64 is 3.61e-07 over the 1e5 random pairs and
    1.20e-07 over the grid: EPS_RELU = 3.7e-07 in tests/_propagate_np.py and DESIGN.md section 5c. The device tests allow
    4 EPS_RELU."""
    mg, vg = P.grid32()
    mr, vr = P.random32()
    eg = P.scale_relative_error(P.relu_moments32(mg, vg), mg, vg)
    er = P.scale_relative_error(P.relu_moments32(mr, vr), mr, vr)
    print(f"eps_relu: grid {eg:.3e}, 1e5 random pairs {er:.3e}")
    worst = max(eg, er)
    assert worst <= P.EPS_RELU <= 1.25 * worst, (eg, er, P.EPS_RELU)
    for a, q, c in (P.relu_moments32(mg, vg), P.relu_moments32(mr, vr)):
        assert np.isfinite(a).all() and np.isfinite(q).all() and np.isfinite(c).all() and (c >= 0).all() and (a >= 0).all()
    # two variance parts are summed first, in fp32
    a2 = P.relu_moments32(mr, vr * np.float32(0.25), vr * np.float32(0.75))
    a1 = P.relu_moments32(mr, vr * np.float32(0.25) + vr * np.float32(0.75))
    assert all(np.array_equal(x, y) for x, y in zip(a1, a2))
    # a huge |alpha| neither overflows nor divides by zero
    a, q, c = P.relu_moments32(np.array([1e15, -1e15], np.float32), np.array([1e-30, 1e-30], np.float32))
    assert a[0] == np.float32(1e15) and a[1] == 0 and np.isfinite(q).all() and q[1] == 0 and c[1] == 0


def test_one_layer_network_is_exact_for_the_sampler():
    """12-9-2, random parameters: the propagated mean within 5 standard errors of 20 000 draws of the LRT sampler, the variance
    within 5 sqrt((m4 - var^2) / n) -- for every output of every row."""
    g = np.random.default_rng(17)
    R, I, H, W = 4, 12, 9, 2
    x = g.standard_normal((R, I))
    means, lvars, bias = g.standard_normal((H, I)) * 0.4, np.log(g.uniform(0.01, 0.2, (H, I))), g.standard_normal(H) * 0.3
    w3, b3 = g.standard_normal((W, H)) * 0.5, g.standard_normal(W) * 0.1
    mean, var, _, _ = P.propagate_network(x, [(means, lvars, bias)], w3, b3, "f32")
    draws = P.sample_one_layer(x.astype(np.float32), means.astype(np.float32), lvars.astype(np.float32), bias.astype(np.float32),
                               w3.astype(np.float32), b3.astype(np.float32), 20000, seed=23)
    sm, bm, sv, bv = P.moment_band(draws)
    print(f"one layer: max |d mean| / band {np.max(np.abs(mean - sm) / bm):.2f}, max |d var| / band {np.max(np.abs(var - sv) / bv):.2f}")
    assert (np.abs(mean - sm) <= bm).all() and (np.abs(var - sv) <= bv).all()
    assert (var > 0).all()


def test_error_bound_and_rounding_points_of_the_network_restatement():
    """The bound the GPU tests use is the restatement's own: zero GEMM / ReLU allowances give a zero bound in fp32 arithmetic of
    exact operands, the bf16 form rounds where the engine rounds, and a pruned weight leaves the network."""
    g = np.random.default_rng(3)
    x = g.standard_normal((5, 20)).astype(np.float32)
    params = [((g.standard_normal((24, 20)) * 0.3).astype(np.float32), np.log(g.uniform(0.001, 0.05, (24, 20))).astype(np.float32),
               (g.standard_normal(24) * 0.1).astype(np.float32)),
              ((g.standard_normal((17, 24)) * 0.3).astype(np.float32), np.log(g.uniform(0.001, 0.05, (17, 24))).astype(np.float32),
               (g.standard_normal(17) * 0.1).astype(np.float32))]
    w3, b3 = (g.standard_normal((3, 17)) * 0.4).astype(np.float32), (g.standard_normal(3) * 0.1).astype(np.float32)
    mean, var, em, ev = P.propagate_network(x, params, w3, b3, "f32")
    assert (em > 0).all() and (ev > 0).all() and (em < 1e-3 * (np.abs(mean) + 1)).all() and (ev < 1e-2 * (var + 1e-3)).all()
    mb, vb, _, _ = P.propagate_network(x, params, w3, b3, "bf16")
    assert 0 < np.abs(mb - mean).max() < 0.1 and (vb >= 0).all()
    masks = [g.uniform(size=p[0].shape) < 0.5 for p in params]
    zeroed = [(np.where(k, 0, mu).astype(np.float32), np.where(k, -np.inf, lv).astype(np.float32), b) for k, (mu, lv, b) in zip(masks, params)]
    m1, v1, _, _ = P.propagate_network(x, params, w3, b3, "f32", masks=masks)
    m2, v2, _, _ = P.propagate_network(x, zeroed, w3, b3, "f32")
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.abs(m1 - mean).max() > 0
