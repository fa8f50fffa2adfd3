"""CPU tests of tests/_gemm_np.py, the float64 reference the GPU tests of the GEMM forms compare against: (a) it agrees with the
oracle (OracleVBLinear, oracle/ref_numpy.lrt_forward and emulate_lrt_step) in both modes, with stacked draws; (b) an fp32
restatement of each epilogue, op by op with a correctly rounded reciprocal square root and expf, uses less than the whole of each
derived bound -- the fraction is printed; (c) the interval rule for bf16 stores accepts exactly the roundings of an interval."""
import numpy as np
import pytest

from tests import _gemm_np as G

SEED = 3
f8 = np.float64


@pytest.fixture(scope="module")
def vo():
    from oracle import vbnn_oracle
    vbnn_oracle.build()
    return vbnn_oracle


def _opt(mode):
    return dict(var_init=1e-2, mu_init=1, B=1e3, S=2, mode=mode, seed=SEED)


def _tol(absprod):           # the oracle sums in fp32: its own accumulation error
    return 4e-6 * absprod + 1e-7


@pytest.mark.parametrize("N,I,O", [(1, 1, 1), (5, 7, 3), (33, 70, 50)])
@pytest.mark.parametrize("mode", ["wn", "lrt"])
def test_reference_agrees_with_the_oracle_layer(vo, mode, N, I, O):
    """forward, gradInput and accGradParameters of one layer over two draws (the second accumulates), and the two draws stacked
    as rows under rows_per_draw"""
    om = vo.OracleVBLinear(I, O, _opt(mode), layer_id=2)
    rng = np.random.default_rng(N + I)
    om.lvars[:] = rng.normal(np.log(1e-2), 0.3, (O, I)).astype(np.float32)
    om.bias[:] = rng.normal(0, 1, O).astype(np.float32)
    om.compute_prior()
    x = rng.normal(0, 1, (N, I)).astype(np.float32)
    g = rng.normal(0, 1, (N, O)).astype(np.float32)
    fill = lambda rows, cols, draw, row0: vo.fill_normal(rows, cols, SEED, vo.STREAM_ZETA, 2, draw, row0)
    om.row0 = 11
    old, ys = None, []
    for _ in range(2):
        om.sample()
        y = om.updateOutput(x).astype(f8)
        ys.append(y)
        gx = om.backward(x, g, 0.5).astype(f8)
        if mode == "lrt":
            z = G.zeta(fill, N, O, om.draw, om.row0)
            fw = G.forward(x, om.means, om.bias, np.exp(om.lvars.astype(f8)), None, z)
            assert (np.abs(fw["y"] - y) <= _tol(np.abs(x) @ np.abs(om.means).T + np.abs(fw["y"] - fw["m"]) + 1)).all()
            assert (np.abs(fw["r"] - om.r) <= 1e-5 * np.abs(fw["r"]) + 1e-9).all()
            assert (np.abs(fw["v"] - om.v) <= _tol(fw["v"])).all()
            gv = g.astype(f8) * om.r
            dx = G.grad_input(g, om.means, gv, np.exp(om.lvars.astype(f8)), x)
            dw = G.acc_grad(x, g, gv, None, 0.5, om.lvars, old=old)
            absgx = np.abs(g) @ np.abs(om.means) + 2 * np.abs(x) * (np.abs(gv) @ np.exp(om.lvars.astype(f8)))
        else:
            fw = G.forward(x, om.weight, om.bias)
            assert (np.abs(fw["y"] - y) <= _tol(np.abs(x) @ np.abs(om.weight).T + 1)).all()
            dx = G.grad_input(g, om.weight)
            dw = G.acc_grad(x, g, None, None, 0.5, om.lvars, e=om.e, old=old)
            absgx = np.abs(g) @ np.abs(om.weight)
        assert (np.abs(dx["gx"] - gx) <= _tol(absgx)).all()
        absw = np.abs(g).T @ np.abs(x) * om.draw
        assert (np.abs(dw["gradWeight"] - om.gradWeight) <= _tol(absw)).all()
        assert (np.abs(dw["gradBias"] - om.gradBias) <= _tol(np.abs(g).sum(0) * om.draw)).all()
        assert np.abs(dw["gradSum"] - om.gradSum).max() <= 2e-5 * np.abs(dw["gradSum"]).max() + 1e-7
        old = dw
    if mode == "lrt":
        # the two draws as 2 N stacked rows: row n is minibatch row n % N of draw (first + n // N)
        z = G.zeta(fill, 2 * N, O, om.draw - 1, om.row0, rows_per_draw=N)
        fw = G.forward(np.vstack([x, x]), om.means, om.bias, np.exp(om.lvars.astype(f8)), None, z)
        assert np.abs(fw["y"] - np.vstack(ys)).max() <= 1e-4 * np.abs(fw["y"]).max()
        d, r = G.noise_address(5, 7, 100, rows_per_draw=2, draw_dev=3)
        assert d.tolist() == [10, 10, 11, 11, 12] and r.tolist() == [100, 101, 100, 101, 100]


def test_reference_agrees_with_the_blas_twin_and_the_emulated_step(vo):
    """oracle/ref_numpy: lrt_forward, and the total gradients of emulate_lrt_step (kl_scale, S, B, the shadows) for a two-layer
    net whose head this test restates"""
    from oracle import ref_numpy as R
    rng = np.random.default_rng(5)
    N, sizes, C, B, S = 9, [6, 8, 5], 4, 50.0, 2.0
    layers = [dict(means=rng.normal(0, 1, (o, i)).astype(np.float32), lvars=rng.normal(-3, 0.3, (o, i)).astype(np.float32),
                   bias=rng.normal(0, 1, o).astype(np.float32)) for i, o in zip(sizes[:-1], sizes[1:])]
    w3, b3 = rng.normal(0, 1, (C, sizes[-1])).astype(np.float32), np.zeros(C, np.float32)
    x, t = rng.normal(0, 1, (N, sizes[0])).astype(np.float32), rng.integers(0, C, N)
    zs = [rng.normal(0, 1, (N, o)) for o in sizes[1:]]
    for rnd, shadows in ((lambda a: a, False), (R.bf16_round, True)):
        loss, res, gw3, gb3 = R.emulate_lrt_step(layers, w3, b3, x, t, zs, rnd=rnd, S=S, B=B, kl_shadows=shadows, kl_scale=0.7)
        xs, x2s, rs = [rnd(x)], [rnd(rnd(x) * rnd(x))], []
        for lay, z in zip(layers, zs):
            fw = G.forward(xs[-1], rnd(lay["means"]), lay["bias"], rnd(np.exp(lay["lvars"])), x2s[-1], z, relu=True)
            y2, _ = R.lrt_forward(xs[-1], lay["means"], lay["lvars"], lay["bias"], z, rnd=rnd)
            assert np.abs(fw["y"] - y2).max() <= 1e-12 * np.abs(y2).max()
            h = rnd(fw["h"].astype(np.float32))
            rs.append(rnd(fw["r"].astype(np.float32)))
            xs.append(h); x2s.append(rnd(h * h))
        logits = (xs[-1].astype(f8) @ rnd(w3).astype(f8).T + b3).astype(np.float32)
        out = R.log_softmax(logits)
        onehot = np.zeros_like(out); onehot[np.arange(N), t] = 1.0
        g3 = rnd(((np.exp(out) - onehot) * np.float32(1.0 / N)).astype(np.float32)).astype(f8)
        gx = g3 @ rnd(w3).astype(f8)
        for k in (1, 0):
            lay = layers[k]
            gp = np.where(xs[k + 1] > 0, gx, 0.0).astype(np.float32)
            g, gv = rnd(gp), rnd(gp * rs[k])
            var32 = np.exp(lay["lvars"])
            vh = float(np.sum(var32.astype(f8) + lay["means"].astype(f8) ** 2) / var32.size)
            dw = G.acc_grad(xs[k], g, gv, x2s[k], 1.0, lay["lvars"], means=lay["means"], var_hat=vh, B=B, S=S, kl_scale=0.7,
                            mu_s=rnd(lay["means"]) if shadows else None, var_s=rnd(var32) if shadows else None)
            for name in ("gradWeight", "gradSum", "gradBias", "grad_mu", "grad_lv"):
                assert np.abs(dw[name] - res[k][name]).max() <= 1e-6 * np.abs(res[k][name]).max() + 1e-15, (k, name)
            if k:
                gx = G.grad_input(g, rnd(lay["means"]), gv, rnd(var32), xs[k])["gx"]


def test_parts_and_accumulate():
    rng = np.random.default_rng(2)
    x, g, gv = rng.normal(0, 1, (7, 5)), rng.normal(0, 1, (7, 3)), rng.normal(0, 1, (7, 3))
    lv, mu = rng.normal(-2, 0.2, (3, 5)), rng.normal(0, 1, (3, 5))
    kw = dict(scale=0.5, lvars=lv, means=mu, var_hat=0.3, B=10.0, S=2.0, kl_scale=1.0)
    full, p1, p2 = (G.acc_grad(x, g, gv, part=p, **kw) for p in (0, 1, 2))
    for k in ("gradWeight", "gradBias", "grad_mu"):
        assert np.array_equal(full[k], p1[k]) and p2[k] is None
    for k in ("gradSum", "grad_lv"):
        assert np.array_equal(full[k], p2[k]) and p1[k] is None
    again = G.acc_grad(x, g, gv, old=full, **kw)
    lik = G.acc_grad(x, g, gv, **dict(kw, kl_scale=0.0))
    for k in ("gradWeight", "gradBias", "gradSum", "grad_mu", "grad_lv"):           # accumulate adds the likelihood part only
        assert np.allclose(again[k], full[k] + lik[k], rtol=1e-14, atol=0)


def test_interval_rule():
    """bf16_rne is round-to-nearest-even at 8 significant bits; interval_ok accepts exactly the roundings of the interval"""
    from oracle.ref_numpy import bf16_round
    rng = np.random.default_rng(0)
    a = rng.normal(0, 100, 20000).astype(np.float32)
    assert np.array_equal(G.bf16_rne(a.astype(f8)), bf16_round(a).astype(f8))
    assert G.bf16_rne(1.00390625) == 1.0 and G.bf16_rne(1.01171875) == 1.015625 and G.bf16_rne(-257.0) == -256.0      # ties to even
    mid = 1.00390625                                            # midpoint of 1 and 1 + 2^-7
    assert G.interval_ok(1.0, mid, 1e-9) and G.interval_ok(1.0078125, mid, 1e-9)
    assert not G.interval_ok(1.0078125, mid - 1e-6, 1e-9) and not G.interval_ok(1.015625, mid, 1e-9)
    assert G.far_side(np.array([1.0078125, 1.0]), np.array([mid, 1.0])) == 1


def _frac(err, bound):
    """largest err / bound; where the bound is 0 (an exact zero) the error must be 0 too"""
    assert (err[bound == 0] == 0).all()
    return (err[bound > 0] / bound[bound > 0]).max()


def test_fp32_restatement_stays_inside_the_derived_bounds():
    """What fraction of each derived bound does fp32 arithmetic alone use, with correctly rounded rsq / expf? Below 1, printed."""
    rng = np.random.default_rng(7)
    N, I, O = 64, 48, 40
    mu = rng.integers(-3, 4, (O, I)); var = rng.integers(0, 3, (O, I)); x = rng.integers(-3, 4, (N, I)); x[5] = 0
    bias = rng.integers(-8, 9, O) * 0.25
    z = rng.normal(0, 1, (N, O)).astype(np.float32)
    fw = G.forward(x, mu, bias, var, None, z)
    y, r = G.forward_f32(x @ mu.T, (x * x) @ var.T, bias, z)
    fy = (np.abs(y - fw["y"])[fw["v"] > 0] / G.bound_y(fw)[fw["v"] > 0]).max()
    fr = (np.abs(r - fw["r"])[fw["v"] > 0] / G.bound_r(fw)[fw["v"] > 0]).max()
    assert (r[5] == 0).all() and np.array_equal(y[5], bias.astype(np.float32))
    g = rng.integers(-3, 4, (N, O)); gv = rng.integers(-4, 5, (N, O)) * 0.25
    lv = rng.normal(np.log(1e-2), 0.5, (O, I)).astype(np.float32)
    means = rng.normal(0, 1, (O, I)).astype(np.float32)
    vh = float(np.mean(np.exp(lv.astype(f8)) + means.astype(f8) ** 2))
    kw = dict(scale=0.5, lvars=lv, means=means, var_hat=vh, B=100.0, S=3.0, kl_scale=1.0)
    first = G.acc_grad(x, g, gv, **kw)
    fracs = {"y": fy, "r": fr}
    for tag, old in (("first", None), ("accumulate", first)):
        ref = G.acc_grad(x, g, gv, old=old, **kw)
        old32 = None if old is None else {k: np.asarray(v, np.float32) for k, v in old.items() if v is not None}
        ref32 = ref if old is None else G.acc_grad(x, g, gv, old=old32, **kw)       # the old values as fp32 stores them
        gs, gm, gl = G.acc_grad_f32(ref["a1"], ref["a2"], lv, means, vh, 0.5, 100.0, 3.0, 1.0, old=old32)
        var64 = np.exp(lv.astype(f8))
        fracs[f"gradSum/{tag}"] = _frac(np.abs(gs - ref32["gradSum"]), G.bound_grad_sum(ref["a2"], lv, ref32["gradSum"]))
        fracs[f"grad_mu/{tag}"] = _frac(np.abs(gm - ref32["grad_mu"]),
                                        G.bound_grad_mu(ref["a1"], means, 0.5, 3.0, 100.0, vh, 1.0, ref32["grad_mu"], old is not None))
        fracs[f"grad_lv/{tag}"] = _frac(np.abs(gl - ref32["grad_lv"]),
                                        G.bound_grad_lv(ref["a2"], var64, 3.0, 100.0, vh, 1.0, ref32["grad_lv"], old is not None))
    print("fraction of each derived bound used by an fp32 restatement: " + ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
    assert all(0 < v < 1 for v in fracs.values()), fracs
