"""GPU tests of the sampling-free predictive: the three kernels of vbnn_amd/csrc/propagate.hip called directly against the NumPy
restatement (tests/_propagate_np.py), and FusedMLP.predict_analytic over them -- against the float64 propagation with the
restatement's own error bound (f32 and bf16), against the Monte-Carlo predictive where propagation is exact (one VB layer), and
its contract: counters, chunking, row0, views, versions, refusals, nothing else written."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _propagate_np as P
from tests._update_np import bf16_round

pytestmark = pytest.mark.gpu

SEED = 3
EPS = 4 * P.EPS_RELU                   # the device's allowance per ReLU stage (scale-relative)
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _lib():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    return L, L.lib(), Context.get().h


def _call(name, ctx, *args):
    """One checked call of an entry point, on the default context or on a context handle of the caller's: that one's stream is its
    own, so the uploads are awaited before the call and vbnn_sync after."""
    L, lib, own = _lib()
    if ctx is not None:
        torch.cuda.synchronize()
    L.check(getattr(lib, name)(ctx or own, *args))
    if ctx is not None:
        L.check(lib.vbnn_sync(ctx))


def _placed(a2d, ld, offset, dtype=torch.float32, fill=float("nan")):
    """a2d (rows x cols) on the device with row pitch ld, `fill` in every pad, starting `offset` ELEMENTS past a 16-byte boundary.
    Returns (the owning tensor, the view of the rows x ld block, the data pointer of element [0, 0])."""
    rows, cols = a2d.shape
    buf = torch.full((rows * ld + offset + 8,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + rows * ld].view(rows, ld)
    view[:, :cols] = dev(a2d).to(dtype)
    return buf, view, buf.data_ptr() + offset * buf.element_size()


# ------------------------------------------------------------------------------------------------ vbnn_relu_moments
def relu_inputs(N, O, seed=7):
    """m over three decades either sign, two positive variance parts; row 0 (and every fifth element) has v = 0."""
    g = np.random.default_rng(seed + 131 * N + O)
    m = (g.standard_normal((N, O)) * 10.0 ** g.uniform(-1, 1.5, (N, O))).astype(np.float32)
    v1 = (10.0 ** g.uniform(-4, 2, (N, O))).astype(np.float32)
    v2 = (10.0 ** g.uniform(-4, 2, (N, O))).astype(np.float32)
    zero = np.zeros((N, O), bool)
    zero[0] = True
    zero.ravel()[::5] = True
    v1[zero] = 0.0
    v2[zero] = 0.0
    return m, v1, v2


def run_relu(m, v1, v2, dtype, ld_in, ld_out, in_off=0, out_off=0, want="aqc", ctx=None):
    """vbnn_relu_moments; returns {name: N x ld_out float array of the WHOLE packed block (pads included)}."""
    L = _lib()[0]
    N, O = m.shape
    keep = [_placed(t, ld_in, in_off) for t in ((m, v1) if v2 is None else (m, v1, v2))]
    outs = {k: _placed(np.zeros((N, O), np.float32), ld_out, out_off, TDT[dtype], fill=0.0) for k in want}
    a = L.ReluMomentsArgs(m=keep[0][2], ld_m=ld_in, v1=keep[1][2], v2=keep[2][2] if v2 is not None else None, ld_v=ld_in, N=N, O=O,
                          ld_out=ld_out, **{k: outs[k][2] for k in want})
    _call("vbnn_relu_moments", ctx, L.F32 if dtype == "f32" else L.BF16, C.byref(a))
    got = {k: host(outs[k][1]) for k in want}
    for k in want:                                             # nothing outside the block either
        assert not host(outs[k][0][:out_off]).any() and not host(outs[k][0][out_off + N * ld_out:]).any(), k
    return got


def check_relu(got, m, v1, v2, dtype):
    """Every output within e = 4 EPS_RELU (scale-relative) of the fp32 restatement w. bf16: the kernel's fp32 value lies within e
    of w and rounding is monotone, so its bf16 lies in [bf16(w - e), bf16(w + e)]: exactly bf16(w) where no rounding boundary is
    within e of w, a neighbour (one bf16 ulp) where one is, and more than that only where e itself exceeds an ulp of the tiny
    value (c in the cancellation regime, the lower tail). Pads zero, c >= 0."""
    N, O = m.shape
    want = dict(zip("aqc", P.relu_moments32(m, v1, v2)))
    v = v1 if v2 is None else v1 + v2
    sc = P.relu_scale(m, v)
    worst = 0.0
    for k, g in got.items():
        assert not g[:, O:].any(), f"{k}: pads written"
        g = g[:, :O].astype(np.float64)
        assert np.isfinite(g).all() and (g >= 0).all(), k
        w = want[k].astype(np.float64)
        e = EPS * sc ** (1 if k == "a" else 2)
        if dtype == "bf16":
            rnd = P.rounder("bf16")
            w, lo, hi = rnd(w), rnd(np.maximum(w - e, 0.0)), rnd(w + e)
            tol = np.maximum(hi - w, w - lo)
        else:
            tol = e
        d = np.abs(g - w)
        assert (d <= tol).all(), (k, float((d - tol).max()))
        worst = max(worst, float((d / np.where(tol > 0, tol, 1.0)).max()))
        assert (g[v == 0] == w[v == 0]).all(), f"{k}: the v = 0 elements are exact"
    return worst


SHAPES = [(1, 1), (3, 5), (7, 64), (5, 67), (33, 130)]
PATHS = {
    "vector": lambda O: dict(ld_in=(O + 3) // 4 * 4 + 4, ld_out=(O + 63) // 64 * 64 + 64),
    "odd-ld": lambda O: dict(ld_in=O + 3 - (O % 2), ld_out=(O + 63) // 64 * 64 + 64),  # an odd input pitch: 4-byte loads
    "off-16": lambda O: dict(ld_in=(O + 3) // 4 * 4 + 4, ld_out=(O + 63) // 64 * 64 + 64, in_off=1, out_off=1),   # 4-byte loads and stores
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N,O", SHAPES)
def test_relu_moments_match_the_restatement(N, O, dtype, path):
    m, v1, v2 = relu_inputs(N, O)
    kw = PATHS[path](O)
    assert kw["ld_in"] > O and kw["ld_out"] > O
    for parts in ((v1, None), (v1, v2)):
        got = run_relu(m, parts[0], parts[1], dtype, **kw)
        worst = check_relu(got, m, parts[0], parts[1], dtype)
        again = run_relu(m, parts[0], parts[1], dtype, **kw)
        assert all(same_bits(got[k], again[k]) for k in got), "two launches differ"
    print(f"relu_moments {N}x{O} {dtype} {path}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_relu_moments_outputs_are_optional_and_the_grid_holds(dtype):
    m, v1, v2 = relu_inputs(5, 67)
    full = run_relu(m, v1, v2, dtype, 72, 128)
    for want in ("qc", "ac", "aq", "a", "c"):
        part = run_relu(m, v1, v2, dtype, 72, 128, want=want)
        assert set(part) == set(want) and all(same_bits(part[k], full[k]) for k in want), want
    mg, vg = P.grid32()                                        # the issue's grid, v = 0 included, as one row
    got = run_relu(mg[None, :], vg[None, :], None, dtype, len(mg) + 3, 64)
    check_relu(got, mg[None, :], vg[None, :], None, dtype)


def test_relu_moments_refuses_bad_arguments():
    L, lib, ctx = _lib()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    o = torch.zeros(64, dtype=torch.float32, device="cuda")
    p, po = C.c_void_p(t.data_ptr()), C.c_void_p(o.data_ptr())
    ok = dict(m=p, ld_m=8, v1=C.c_void_p(t.data_ptr() + 128), v2=None, ld_v=8, N=2, O=8, a=po, q=None, c=None, ld_out=8)
    for bad in (dict(m=None), dict(v1=None), dict(N=0), dict(O=0), dict(ld_m=7), dict(ld_v=7), dict(ld_out=7),
                dict(m=C.c_void_p(t.data_ptr() + 2)),
                dict(a=p), dict(a=C.c_void_p(t.data_ptr() + 28)), dict(q=C.c_void_p(o.data_ptr() + 16))):      # overlaps
        for dt in (L.F32, L.BF16):
            assert lib.vbnn_relu_moments(ctx, dt, C.byref(L.ReluMomentsArgs(**dict(ok, **bad)))) == 1, bad
    assert lib.vbnn_relu_moments(ctx, L.F32, C.byref(L.ReluMomentsArgs(**dict(ok, a=C.c_void_p(o.data_ptr() + 2))))) == 1    # fp32 off its element
    assert lib.vbnn_relu_moments(ctx, L.BF16, C.byref(L.ReluMomentsArgs(**dict(ok, a=C.c_void_p(o.data_ptr() + 1))))) == 1   # an odd bf16 pointer
    assert lib.vbnn_relu_moments(ctx, 7, C.byref(L.ReluMomentsArgs(**ok))) == 4
    assert lib.vbnn_relu_moments(ctx, L.F32, None) == 1
    assert lib.vbnn_relu_moments(ctx, L.F32, C.byref(L.ReluMomentsArgs(**ok))) == 0          # (the accepted call the refused ones vary)
    torch.cuda.synchronize()
    assert not o.any()                                          # a refused call wrote nothing; the accepted one wrote relu(0) = 0


# ------------------------------------------------------------------------------------------------ vbnn_square_shadow
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (7, 64), (5, 67), (33, 130)])
def test_square_shadow_is_bitwise_the_restatement(rows, cols, dtype, off):
    check_square_shadow(rows, cols, dtype, off)


def check_square_shadow(rows, cols, dtype, off, ctx=None):
    """The whole check of one shape; returns the destination block as the device left it."""
    L, lib, own = _lib()
    g = np.random.default_rng(rows * 1000 + cols)
    src = (g.standard_normal((rows, cols)) * 10.0 ** g.uniform(-3, 2, (rows, cols))).astype(np.float32)
    src[0, 0] = 0.0
    if dtype == "bf16":
        src = bf16_round(src)
    ld = (cols + 63) // 64 * 64 + (1 if off else 0)            # (off: an odd pitch off the 16-byte boundary -- element by element)
    sbuf, sview, sptr = _placed(src, ld, off, TDT[dtype])
    dbuf, dview, dptr = _placed(np.full((rows, cols), 5.0, np.float32), ld + 64, off, TDT[dtype], fill=7.0)
    _call("vbnn_square_shadow", ctx, L.F32 if dtype == "f32" else L.BF16, sptr, ld, rows, cols, dptr, ld + 64)
    want = src * src
    if dtype == "bf16":
        want = bf16_round(want)
    got = host(dview)
    assert same_bits(got[:, :cols].astype(np.float32), want.astype(np.float32))
    assert (got[:, cols:] == 7.0).all() and (host(dbuf[:off]) == 7.0).all() and (host(dbuf[off + rows * (ld + 64):]) == 7.0).all()
    assert lib.vbnn_square_shadow(ctx or own, L.F32 if dtype == "f32" else L.BF16, sptr, cols - 1, rows, cols, dptr, ld + 64) == 1   # ld_src < cols
    torch.cuda.synchronize()
    return got


# ------------------------------------------------------------------------------------------------ vbnn_logit_draws
def device_normals(R, Cn, layer, draw, row0, seed=SEED):
    L, lib, ctx = _lib()
    z = torch.empty(R, Cn, dtype=torch.float32, device="cuda")
    L.check(lib.vbnn_fill_normal(ctx, C.c_void_p(z.data_ptr()), R, Cn, Cn, seed, L.STREAM_ZETA, layer, draw, row0, 1.0))
    return host(z)


def restated_draws(m, v, S, layer, draw, row0, seed=SEED):
    """m + sqrt(v) z in np.float32, one multiply and one add, z = vbnn_fill_normal of the same address."""
    R, Cn = m.shape
    return np.stack([m + np.sqrt(v) * device_normals(R, Cn, layer, draw + s, row0, seed) for s in range(S)]).astype(np.float32)


def run_draws(m, v, S, layer, draw, row0, ld_y=None, stride=None, off=0, ctx=None):
    L = _lib()[0]
    R, Cn = m.shape
    ld_y = ld_y or Cn
    stride = stride or R * ld_y
    md, vd = dev(m), dev(v)
    buf = torch.full((S * stride + off + 8,), 9.0, dtype=torch.float32, device="cuda")
    a = L.LogitDrawsArgs(m=C.c_void_p(md.data_ptr()), ld_m=Cn, v=C.c_void_p(vd.data_ptr()), ld_v=Cn, R=R, C=Cn, S=S, seed=SEED,
                         layer=layer, draw=draw, row0=row0, y=C.c_void_p(buf.data_ptr() + 4 * off), ld_y=ld_y, draw_stride=stride)
    _call("vbnn_logit_draws", ctx, C.byref(a))
    full = host(buf)
    y = np.stack([full[off + s * stride:off + s * stride + R * ld_y].reshape(R, ld_y) for s in range(S)])
    touched = np.zeros(full.shape, bool)
    for s in range(S):
        for r in range(R):
            b = off + s * stride + r * ld_y
            touched[b:b + Cn] = True
    assert (full[~touched] == 9.0).all(), "a pad or a gap was written"
    return y[:, :, :Cn]


@pytest.mark.parametrize("R,Cn", [(1, 1), (5, 3), (7, 12), (4, 130)])
def test_logit_draws_are_the_contracts_normals_scaled_and_shifted(R, Cn):
    g = np.random.default_rng(R * 100 + Cn)
    m = g.standard_normal((R, Cn)).astype(np.float32)
    v = (10.0 ** g.uniform(-3, 1, (R, Cn))).astype(np.float32)
    S, layer, draw, row0 = 3, 2, 5, 11
    want = restated_draws(m, v, S, layer, draw, row0)
    y = run_draws(m, v, S, layer, draw, row0)
    assert same_bits(y, want)
    assert same_bits(run_draws(m, v, S, layer, draw, row0, ld_y=Cn + 3, stride=R * (Cn + 3) + 5, off=1), want)    # 4-byte stores, gaps
    assert same_bits(run_draws(m, v, S, layer, draw, row0, ld_y=(Cn + 3) // 4 * 4 + 4), want)                     # padded rows, 16-byte stores
    y0 = run_draws(m, np.zeros_like(v), S, layer, draw, row0)
    assert all(np.array_equal(y0[s], m) for s in range(S)), "v = 0 returns m in every draw"
    if R >= 4:                                                 # row0 and draw offsets: a sub-block of rows is the same rows of the whole
        sub = run_draws(m[2:4], v[2:4], 2, layer, draw + 1, row0 + 2)
        assert same_bits(sub, y[1:3, 2:4])
    other = run_draws(m, v, 1, layer + 1, draw, row0)
    assert not np.array_equal(other[0], y[0]), "the layer id addresses the stream"


# ------------------------------------------------------------------------------------------------ engine level
def opt_for(mode="lrt", dtype="f32", **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=20, hidden=[24, 17],
             n_classes=3, criterion="mse", type="vb", testSamples=2)
    o.update(kw)
    return o


def randomise(eng, lo=0.001, hi=0.05, seed=11):
    """Random log variances, biases and final bias (the means and the final weight keep their He draw); prepare()."""
    g = np.random.default_rng(seed)
    for v in eng.vb:
        v.lvars.copy_(dev(np.log(g.uniform(lo, hi, (v.O, v.I))).astype(np.float32)))
        v.bias.copy_(dev((g.standard_normal(v.O) * 0.1).astype(np.float32)))
    eng.bias3.copy_(dev((g.standard_normal(eng.n_classes) * 0.1).astype(np.float32)))
    eng.prepare()
    return eng


def params(eng):
    return [(host(v.means), host(v.lvars), host(v.bias)) for v in eng.vb], host(eng.weight3), host(eng.bias3)


def inputs(R, I0, seed=21):
    return np.random.default_rng(seed).standard_normal((R, I0)).astype(np.float32)


def check_engine(eng, mean, var, x, label, masks=None):
    """|mean - restated| and |var - restated| within the restatement's own bound, per output."""
    ps, w3, b3 = params(eng)
    wm, wv, em, ev = P.propagate_network(x, ps, w3, b3, eng.dtype, masks=masks)
    dm, dv = np.abs(host(mean) - wm), np.abs(host(var) - wv)
    print(f"{label}: |d mean| / bound up to {np.max(dm / em):.3f} (bound {em.max():.2e}), |d var| / bound up to "
          f"{np.max(dv / ev):.3f} (bound {ev.max():.2e}, var up to {wv.max():.2e})")
    assert (dm <= em).all() and (dv <= ev).all(), label
    assert (host(var) >= 0).all()
    return wm, wv, em, ev


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_mse_mean_and_variance_match_float64_propagation(dtype, mode):
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for(mode, dtype)))
    x = inputs(5, 20)
    t = inputs(5, 3, seed=22)
    res = eng.predict_analytic(dev(x), targets=dev(t), noise_var=0.3)
    wm, wv, _, _ = check_engine(eng, res.mean, res.var, x, f"mse {dtype} {mode}")
    assert eng.draw == 0 and res.draws is None and res.S == 0 and tuple(res.mean.shape) == tuple(res.var.shape) == (5, 3)
    mean, var = host(res.mean).astype(np.float64), host(res.var).astype(np.float64)
    d2 = (t - mean) ** 2
    assert np.allclose(host(res.row_var), var.mean(1), rtol=1e-5, atol=0)
    assert np.allclose(host(res.row_sq_err), d2.sum(1), rtol=1e-5, atol=0)
    ll = (-0.5 * (np.log(2 * np.pi * (var + 0.3)) + d2 / (var + 0.3))).sum(1)      # ONE Gaussian per output
    assert np.allclose(host(res.row_log_lik), ll, rtol=1e-5, atol=1e-5)
    assert abs(res.mse - d2.mean()) <= 1e-5 * d2.mean() and abs(res.mean_var - var.mean()) <= 1e-5 * var.mean()
    assert abs(res.log_lik - ll.mean()) <= 1e-5 * abs(ll.mean()) and abs(res.mean_draw_mse - (res.mse + res.mean_var)) <= 1e-12
    again = eng.predict_analytic(dev(x), targets=dev(t), noise_var=0.3)
    assert torch.equal(again.mean, res.mean) and torch.equal(again.var, res.var) and again.totals == res.totals
    bare = eng.predict_analytic(dev(x))
    assert torch.equal(bare.mean, res.mean) and bare.row_sq_err is None and bare.row_log_lik is None and bare.mse is None


def test_one_layer_agrees_with_the_monte_carlo_predictive():
    """16-12-2, one VB layer, fp32, LRT, R = 4: propagation is exact for the engine's sampler, so the analytic mean lies within 5
    standard errors and the variance within 5 sqrt((m4 - var^2) / n) of the pooled 1024 draws -- all 8 outputs."""
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for(input_size=16, hidden=[12], n_classes=2)), lo=0.01, hi=0.2)
    x = dev(inputs(4, 16))
    ana = eng.predict_analytic(x)
    assert eng.draw == 0
    draws = torch.cat([eng.predict_regression(x, S=128, keep_draws=True).draws for _ in range(8)])
    assert tuple(draws.shape) == (1024, 4, 2) and eng.draw == 1024
    sm, bm, sv, bv = P.moment_band(host(draws).astype(np.float64))
    dm, dv = np.abs(host(ana.mean) - sm), np.abs(host(ana.var) - sv)
    print(f"one VB layer against 1024 draws: |d mean| / band up to {np.max(dm / bm):.2f}, |d var| / band up to {np.max(dv / bv):.2f}")
    assert (dm <= bm).all() and (dv <= bv).all()


NLL = dict(input_size=20, hidden=[16], criterion="nll")


@pytest.mark.parametrize("Cn", [12, 3])
def test_nll_without_logit_variance_is_the_map_prediction(Cn):
    """lvars = -80: the logit variance is ~1e-35, every draw IS the logit mean, and the probabilities are predict_classes(map=True)'s
    within the GEMM bound: each side's logits within e of the exact ones (e the restatement's bound), a log-probability within
    twice a logit's error, plus the fp32 evaluation of the log-softmax itself (a few ulp of values up to ~max |logit|)."""
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for(n_classes=Cn, **NLL))
    for v in eng.vb:
        v.lvars.fill_(-80.0)
    eng.prepare()
    x = inputs(5, 20)
    res = eng.predict_analytic(dev(x), S=4)
    ref = eng.predict_classes(dev(x), map=True)
    assert eng.draw == 4
    ps, w3, b3 = params(eng)
    wm, wv, em, _ = P.propagate_network(x, ps, w3, b3, "f32")
    assert wv.max() < 1e-30
    lm = host(res.logit_mean)
    assert (np.abs(lm - wm) <= em).all() and all(np.array_equal(host(res.draws[s]), lm) for s in range(4))
    tol = 4 * em.max(1, keepdims=True) + 2e-6 * (1 + np.abs(wm).max())
    assert (np.abs(host(res.log_probs) - host(ref.log_probs)) <= tol).all()
    assert (np.abs(host(res.probs) - host(ref.probs)) <= tol).all()
    assert float(res.mutual_info.abs().max()) <= 1e-6


@pytest.mark.parametrize("Cn", [12, 3])
def test_nll_draws_fields_and_counters(Cn):
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for(n_classes=Cn, device_draw=True, **NLL)), lo=0.01, hi=0.1)
    twin = randomise(FusedMLP(opt_for(n_classes=Cn, **NLL)), lo=0.01, hi=0.1)
    R, S, K = 5, 6, 2
    x = inputs(R, 20)
    t = dev((np.arange(R) % Cn).astype(np.int32))
    eng.sample(3)                                              # the counters do not start at zero
    d0 = eng.draw + 1
    res = eng.predict_analytic(dev(x), targets=t, S=S, topk=K)
    assert eng.draw == 3 + S and int(eng._draw_dev.cpu()[0]) == 3 + S
    # the logit moments against float64, and the draws bitwise from the device's own mean and variance
    check_engine(eng, res.logit_mean, res.logit_var, x, f"nll C={Cn}")
    lm, lv = host(res.logit_mean), host(res.logit_var)
    assert (lv > 0).all() and same_bits(host(res.draws), restated_draws(lm, lv, S, len(eng.vb), d0, eng.rank * R, eng.seed))
    # the finish is vbnn_predict_class_moments on those draws: predict_classes' fields, shapes and meanings
    ref = twin.predict_classes(dev(x), targets=t, S=S, topk=K)
    for k in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "pred", "topk_idx", "topk_prob"):
        a, b = getattr(res, k), getattr(ref, k)
        assert a.shape == b.shape and a.dtype == b.dtype, k
    for k in ("nll", "accuracy", "mean_draw_nll", "mean_draw_accuracy", "topk_accuracy"):
        assert isinstance(getattr(res, k), float) and np.isfinite(getattr(res, k)), k
    assert len(res.totals) == len(ref.totals) == 5 and res.S == S
    lp = host(res.log_probs).astype(np.float64)
    d = host(res.draws).astype(np.float64)
    o = d - np.log(np.exp(d - d.max(2, keepdims=True)).sum(2, keepdims=True)) - d.max(2, keepdims=True)
    want = np.log(np.exp(o).mean(0))
    assert np.abs(lp - want).max() <= 1e-5 and np.array_equal(host(res.pred), want.argmax(1))
    assert np.array_equal(host(res.topk_idx)[:, 0], host(res.pred))
    slim = eng.predict_analytic(dev(x), S=S, keep_probs=False)
    assert slim.probs is None and slim.log_probs is None and slim.draws is None and slim.nll is None and eng.draw == 3 + 2 * S
    eng.draw = twin.draw = 3                                   # the same draws again: without keep_probs they live in the chunk's own buffer
    eng._draw_dev.fill_(3)
    for e in (eng, twin):
        again = e.predict_analytic(dev(x), targets=t, S=S, topk=K, keep_probs=False)
        for k in ("entropy", "expected_entropy", "mutual_info", "pred", "topk_idx", "topk_prob"):
            assert torch.equal(getattr(again, k), getattr(res, k)), k
        assert again.totals == res.totals and torch.equal(again.logit_mean, res.logit_mean)
    # row0 shifts the draws as in predict; chunks read their own rows' noise
    eng.draw = twin.draw = 0
    shifted = twin.predict_analytic(dev(x), S=S, row0=7)
    assert same_bits(host(shifted.draws), restated_draws(host(shifted.logit_mean), host(shifted.logit_var), S, len(twin.vb), 1, 7, twin.seed))
    small = randomise(FusedMLP(opt_for(n_classes=Cn, predict_rows=2, **NLL)), lo=0.01, hi=0.1)
    chunked = small.predict_analytic(dev(x), targets=t, S=S, topk=K, row0=7)
    twin.draw = 0
    whole = twin.predict_analytic(dev(x), targets=t, S=S, topk=K, row0=7)
    assert (chunked.chunks, whole.chunks) == (3, 1) and torch.equal(chunked.draws, shifted.draws)
    for k in ("log_probs", "entropy", "expected_entropy", "mutual_info", "pred", "topk_idx", "topk_prob"):
        assert torch.equal(getattr(chunked, k), getattr(whole, k)), k
    assert chunked.totals == whole.totals
    # the regression criterion consumes nothing
    reg = FusedMLP(opt_for(device_draw=True))
    reg.predict_analytic(dev(x))
    assert reg.draw == 0 and int(reg._draw_dev.cpu()[0]) == 0


def test_chunked_equals_unchunked_bitwise():
    from vbnn_amd.engine import FusedMLP
    x, t = inputs(5, 20), inputs(5, 3, seed=22)
    base, small = randomise(FusedMLP(opt_for())), randomise(FusedMLP(opt_for(predict_rows=2)))
    r0 = base.predict_analytic(dev(x), targets=dev(t), noise_var=0.5)
    r1 = small.predict_analytic(dev(x), targets=dev(t), noise_var=0.5)
    assert (r0.chunks, r1.chunks) == (1, 3)
    for k in ("mean", "var", "row_var", "row_sq_err", "row_log_lik"):
        assert torch.equal(getattr(r0, k), getattr(r1, k)), k
    assert r0.totals == r1.totals
    fresh = FusedMLP(opt_for())                                # never prepared: predict_analytic prepares, as predict
    fresh.predict_analytic(dev(x))
    assert fresh._shadows_ready


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_views_held_masks_and_compact_networks(dtype):
    """A dense pruned view, the same mask held, and a compact network each agree with the restatement run on their effective
    parameters (a pruned weight: no mean, no variance)."""
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for("lrt", dtype)))
    x = inputs(5, 20)
    plain = eng.predict_analytic(dev(x))
    r = eng.prune(fraction=0.5)
    masks = [host(r.mask(li)) for li in range(len(eng.vb))]
    with eng.pruned(r):
        view = eng.predict_analytic(dev(x))
    check_engine(eng, view.mean, view.var, x, f"pruned view {dtype}", masks=masks)
    assert not torch.equal(view.mean, plain.mean)
    back = eng.predict_analytic(dev(x))                        # the view is gone: the mu^2 operand follows it
    assert torch.equal(back.mean, plain.mean) and torch.equal(back.var, plain.var)
    with pytest.raises(ValueError, match="compressed pruned view"):
        with eng.pruned(r.compress()):
            eng.predict_analytic(dev(x))
    eng.hold_pruned(r)
    held = eng.predict_analytic(dev(x))
    assert torch.equal(held.mean, view.mean) and torch.equal(held.var, view.var)
    assert all(np.array_equal(host(eng.held_mask(li)), masks[li]) for li in range(len(eng.vb)))
    with pytest.raises(RuntimeError, match="older parameters"):                     # a stale view
        with eng.pruned(r):
            eng.predict_analytic(dev(x))
    other = randomise(FusedMLP(opt_for("lrt", dtype)))
    c = other.compact(other.prune_units(fraction=0.5))
    assert c.sizes != other.sizes
    small = c.predict_analytic(dev(x))
    check_engine(c, small.mean, small.var, x, f"compact {c.sizes} {dtype}")


def test_an_update_is_followed_by_the_new_operands():
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for()))
    x, t = inputs(5, 20), inputs(5, 3, seed=22)
    before = eng.predict_analytic(dev(x))
    ops = eng._ana_ops
    assert eng.predict_analytic(dev(x)) is not None and eng._ana_ops is ops and ops.key[0] == eng._pver
    eng.resetGradients(); eng.sample(); eng.run(dev(x), dev(t)); eng.finish()
    eng.update(dict(eng.opt, state={"learningRate": 0.05}, meanState={"learningRate": 0.05}, varState={"learningRate": 0.05}))
    after = eng.predict_analytic(dev(x))
    assert eng._ana_ops.key[0] == eng._pver and not torch.equal(after.mean, before.mean)
    check_engine(eng, after.mean, after.var, x, "after an update")
    for v, mu2 in zip(eng.vb, eng._ana_ops.mu2):
        assert same_bits(host(mu2.t)[:, :v.I], host(v.means) * host(v.means))


def test_a_graph_replay_invalidates_the_squared_operands():
    """A captured step that holds update() changes the operand shadows at every replay without a new parameter version;
    _StepGraph.launch marks predict_analytic's squares stale. Here the shadows are changed in place, as a replay would, and the
    mark is set as launch() sets it."""
    import inspect
    from vbnn_amd import engine
    eng = randomise(engine.FusedMLP(opt_for()))
    x = inputs(5, 20)
    eng.predict_analytic(dev(x))
    ver = eng._pver
    for v in eng.vb:                                           # what a replayed update does: new shadows, the version as it was
        v.means.mul_(1.5)
        v.mu_s.t[:, :v.I].copy_(v.means)
    assert eng._pver == ver and "_ana_ops_stale = True" in inspect.getsource(engine._StepGraph.launch)
    eng._ana_ops_stale = True
    after = eng.predict_analytic(dev(x))
    assert not eng._ana_ops_stale
    check_engine(eng, after.mean, after.var, x, "after a replayed update")


def test_refusals():
    from vbnn_amd.engine import FusedMLP
    x = dev(inputs(5, 20))
    g = FusedMLP(opt_for(criterion="gauss", n_classes=4))
    with pytest.raises(ValueError, match="criterion = 'gauss' is not supported"):
        g.predict_analytic(x)
    eng = FusedMLP(opt_for())
    with pytest.raises(ValueError, match=r"inputs of shape \(5, 19\)"):
        eng.predict_analytic(dev(inputs(5, 19)))
    with pytest.raises(ValueError, match=r"targets of shape \(5, 2\)"):
        eng.predict_analytic(x, targets=dev(inputs(5, 2)))
    with pytest.raises(ValueError, match="topk belongs to the class predictive"):
        eng.predict_analytic(x, topk=1)
    for kw in (dict(S=4), dict(row0=0)):
        with pytest.raises(ValueError, match="S and row0 address the class predictive"):
            eng.predict_analytic(x, **kw)
    with pytest.raises(ValueError, match=r"inputs of shape \(0, 20\)"):
        eng.predict_analytic(x[:0])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_var"):
            eng.predict_analytic(x, noise_var=bad)
    nll = FusedMLP(opt_for(n_classes=12, **NLL))
    with pytest.raises(ValueError, match="noise_var belongs to the regression predictive"):
        nll.predict_analytic(x, noise_var=0.5)
    with pytest.raises(ValueError, match="topk = 9"):
        nll.predict_analytic(x, topk=9)
    with pytest.raises(ValueError, match="S = 0 draws"):
        nll.predict_analytic(x, S=0)
    with pytest.raises(ValueError, match=r"targets of shape \(4,\)"):
        nll.predict_analytic(x, targets=torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        nll.predict_analytic(x, map=True)
    assert nll.draw == 0 and eng.draw == 0 and g.draw == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nothing_else_is_written(dtype):
    """No parameter, operand shadow, gradient, training buffer or buffer of predict changes across a call (vbnn_digest before and
    after)."""
    from vbnn_amd import checkpoint
    from vbnn_amd.engine import FusedMLP
    eng = randomise(FusedMLP(opt_for("lrt", dtype)))
    x, t = dev(inputs(5, 20)), dev(inputs(5, 3, seed=22))
    eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
    eng.predict_regression(x, S=2)
    watched = [eng.grads, eng.weight3, eng.bias3, eng.w3_s.t, eng.w3T_s.t, eng.h_s.t, eng.logits, eng.g_logits]
    for v in eng.vb:
        watched += [v.means, v.lvars, v.bias, v.stats, v.mu_s.t, v.var_s.t, v.x_s.t, v.g_s.t, v.gv_s.t, v.r]
        watched += [p.t for p in (v.x2_s, v.muT_s, v.varT_s) if p is not None]
    for b in eng._pred_bufs:
        watched += [p.t for p in (b.x, b.x2) if p is not None]
    watched += [eng._pred_bufs.y_reg] if eng._pred_bufs.y_reg is not None else []
    watched = [w for w in watched if w.numel() * w.element_size() % 4 == 0]
    before = checkpoint.digests(watched, eng.ctx)
    draw = eng.draw
    eng.predict_analytic(x, targets=t, noise_var=0.3)
    assert checkpoint.digests(watched, eng.ctx) == before and eng.draw == draw


def test_trainer_logs_the_same_series(tmp_path):
    """opt.predictive = "analytic": the dev pass calls predict_analytic and records the series names of the sampled predictive."""
    from vbnn_amd import train

    class Data:
        def __init__(self, n, I0, Cn):
            g = np.random.default_rng(5)
            self.x, self.t = g.standard_normal((n, I0)).astype(np.float32), (np.arange(n) % Cn).astype(np.int32)

        def create_minibatch(self, start, bs, n, geometry):
            return self.x[start:start + bs], self.t[start:start + bs]

    opt = train.default_opt(input_size=20, hidden=[16], n_classes=3, batchSize=10, testBatchSize=10, trainSize=20, testSize=20, S=1,
                            testSamples=3, log=False, network_name=str(tmp_path / "exp"), geometry=None)
    recs = {}
    for kind in ("analytic", True):
        m = train.Main(dict(opt, predictive=kind))
        m.test(Data(20, 20, 3))
        recs[kind] = m.predictive
    assert set(recs["analytic"]) == set(recs[True]) == {"devacc_pred", "devnll_pred", "dev_mi"}
    assert all(np.isfinite(v) for v in recs["analytic"].values())

    class Regression(Data):
        def __init__(self, n, I0, D):
            Data.__init__(self, n, I0, D)
            self.t = np.random.default_rng(6).standard_normal((n, D)).astype(np.float32)

    ropt = dict(opt, criterion="mse", noise_var=0.3)
    recs = {}
    for kind in ("analytic", True):
        m = train.Main(dict(ropt, predictive=kind))
        m.test(Regression(20, 20, 3))
        recs[kind] = m.predictive
    assert set(recs["analytic"]) == set(recs[True]) == {"dev_epi_var", "devll_pred"}
    assert all(np.isfinite(v) for v in recs["analytic"].values()) and recs["analytic"]["dev_epi_var"] > 0
    with pytest.raises(ValueError, match="quantile_probs needs the sampled predictive"):
        train.Main(dict(ropt, predictive="analytic", quantile_probs=[0.1, 0.9])).test(Regression(20, 20, 3))
