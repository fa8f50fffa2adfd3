"""GPU tests of the regression posterior predictive: vbnn_predict_moments (include/vbnn_hip.h) called directly on uploaded
outputs against float64 NumPy on the same fp32 inputs, its bitwise invariants (the two forms, layouts, S = 1, NaN containment),
its argument checks; and FusedMLP.predict_regression over it against a float64 restatement of the forward, against the
kernel-level reference on its own returned draws (f32 and bf16), against test(), and its chunking / view / refusal contract."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests._regress_np import EPS, check_moments, forward_draw, moments64, mean_tol, var_tol

pytestmark = pytest.mark.gpu

SEED = 3
ROW_KEYS = ("mean", "var", "row_var", "row_sq_err", "row_log_lik")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ kernel level
def _padded(a2d, ld, offset=0):
    """a2d (rows x D) on the device with row pitch ld, NaN in every pad column, starting `offset` floats past a 16-byte boundary.
    Returns (the owning tensor, the data pointer of element [0, 0])."""
    rows, D = a2d.shape
    buf = torch.full((rows * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + rows * ld].view(rows, ld)[:, :D] = dev(a2d)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * offset


def run_moments(y, t, form, noise_var=0.0, ld_y=None, ld_t=None, y_offset=0, want=ROW_KEYS, totals=True, ctx=None):
    """vbnn_predict_moments on y (S x R x D fp32 NumPy) and t (R x D or None): STACKED in one call, ACCUMULATE in S calls over a
    state that starts as NaN (draw 0 must not read it). Returns the outputs as NumPy arrays (+ "totals": 4 floats). ctx: a context handle of the
    caller's (its stream is its own: the uploads are awaited before the calls and vbnn_sync after) in place of the default one."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, own, ctx = L.lib(), ctx is not None, ctx or Context.get().h
    S, R, D = y.shape
    ld_y, ld_t = ld_y or D, ld_t or D
    ybuf, yptr = _padded(y.reshape(S * R, D), ld_y, y_offset)
    tbuf, tptr = _padded(t, ld_t) if t is not None else (None, None)
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {k: torch.full((R, D) if k in ("mean", "var") else (R,), float("nan"), **f32) for k in want
           if t is not None or k in ("mean", "var", "row_var")}
    if not noise_var:
        out.pop("row_log_lik", None)
    tot = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda") if (totals and t is not None) else None
    state = torch.full((R, 2 * D + 2), float("nan"), **f32) if form == L.MOMENTS_ACCUMULATE else None
    a = L.MomentsArgs(y=yptr, ld_y=ld_y, target=tptr, ld_t=ld_t, R=R, D=D, S=S, form=form, noise_var=noise_var, state=_p(state),
                      mean=_p(out.get("mean")), var=_p(out.get("var")), ld_out=D, row_var=_p(out.get("row_var")),
                      row_sq_err=_p(out.get("row_sq_err")), row_log_lik=_p(out.get("row_log_lik")), totals=_p(tot))
    if own:
        torch.cuda.synchronize()
    if form == L.MOMENTS_STACKED:
        L.check(lib.vbnn_predict_moments(ctx, C.byref(a)))
    else:
        for s in range(S):
            a.y, a.draw = yptr + 4 * s * R * ld_y, s
            L.check(lib.vbnn_predict_moments(ctx, C.byref(a)))
    if own:
        L.check(lib.vbnn_sync(ctx))
    got = {k: host(v) for k, v in out.items()}
    if tot is not None:
        got["totals"] = host(tot).tolist()
    del ybuf, tbuf
    return got


def assert_same_outputs(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if k == "totals":
            assert same_bits(np.array(a[k]), np.array(b[k])), (what, k, a[k], b[k])
        else:
            assert same_bits(a[k], b[k]), (what, k)


def normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


CASES = {
    # name: (R, D, S, noise_var, kwargs of run_moments, shifted data)
    "1x1x1": (1, 1, 1, 0.5, {}, False),
    "3x5x2": (3, 5, 2, 0.5, {}, False),
    "37x70x3": (37, 70, 3, 1.0, {}, False),
    "64x257x30": (64, 257, 30, 0.01, {}, False),
    "3x1029x3-partial-quad-in-the-second-slot": (3, 1029, 3, 0.5, {}, False),
    "5x4096x4": (5, 4096, 4, 0.25, {}, False),
    "2x4100x3-above-the-cap": (2, 4100, 3, 0.25, {}, False),
    "9x8x7-nan-pads": (9, 8, 7, 0.5, dict(ld_y=24, ld_t=16), False),
    "9x8x7-y-off-by-one-float": (9, 8, 7, 0.5, dict(y_offset=1), False),
    "37x70x30-shifted": (37, 70, 30, 0.5, {}, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_float64_and_the_forms_agree_bitwise(name):
    from vbnn_amd import _lib as L
    R, D, S, tau2, kw, shifted = CASES[name]
    z = normal((S, R, D), 11)
    y = (np.float32(1000.0) + np.float32(1e-3) * z).astype(np.float32) if shifted else z
    t = normal((R, D), 12)
    acc = run_moments(y, t, L.MOMENTS_ACCUMULATE, tau2, **kw)
    check_moments(acc, y, t, tau2, label=name + " accumulate")
    if D > L.MOMENTS_STACKED_MAX_D:
        with pytest.raises(L.VbnnError, match="STACKED"):
            run_moments(y, t, L.MOMENTS_STACKED, tau2, **kw)
        return
    stk = run_moments(y, t, L.MOMENTS_STACKED, tau2, **kw)
    check_moments(stk, y, t, tau2, label=name + " stacked")
    assert_same_outputs(stk, acc, name)
    if kw:      # the layout changes the access path, never the values: pads are not read, a row sum's order depends on D alone
        assert_same_outputs(stk, run_moments(y, t, L.MOMENTS_STACKED, tau2), name + " against the dense aligned layout")
    # without targets / without a noise variance: the remaining outputs are the same bits
    bare = run_moments(y, None, L.MOMENTS_STACKED, 0.0, **kw)
    assert set(bare) == {"mean", "var", "row_var"}
    for k in bare:
        assert same_bits(bare[k], stk[k]), k
    no_ll = run_moments(y, t, L.MOMENTS_ACCUMULATE, 0.0, **kw)
    assert "row_log_lik" not in no_ll and no_ll["totals"][2] == 0.0
    for k in ("mean", "var", "row_var", "row_sq_err"):
        assert same_bits(no_ll[k], stk[k]), k
    assert [no_ll["totals"][k] for k in (0, 1, 3)] == [stk["totals"][k] for k in (0, 1, 3)]


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_one_draw_and_equal_draws_have_exactly_no_variance(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, D in ((37, 70), (3, 1028)):
        y, t = normal((1, R, D), 5), normal((R, D), 6)
        got = run_moments(y, t, f, 0.5)
        assert same_bits(got["mean"], y[0])
        assert same_bits(got["var"], np.zeros((R, D), np.float32)) and same_bits(got["row_var"], np.zeros(R, np.float32))
        assert got["totals"][3] == 0.0 and got["totals"][0] == got["totals"][1]        # S = 1: the mean's error is the draw's
        y5 = np.repeat(y, 5, axis=0)
        got = run_moments(y5, t, f, 0.5)
        assert same_bits(got["mean"], y[0]) and same_bits(got["var"], np.zeros((R, D), np.float32))
        check_moments(got, y5, t, 0.5, label=f"equal draws {form}")


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_a_nan_stays_in_its_element_its_row_and_the_totals(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, D, S, (s, r, d) in ((37, 70, 3, (1, 5, 11)), (6, 1028, 4, (3, 2, 1027))):
        y, t = normal((S, R, D), 7), normal((R, D), 8)
        clean = run_moments(y, t, f, 0.5)
        bad = y.copy()
        bad[s, r, d] = np.nan
        got = run_moments(bad, t, f, 0.5)
        assert np.isnan(got["mean"][r, d]) and np.isnan(got["var"][r, d])
        for k in ("row_var", "row_sq_err", "row_log_lik"):
            assert np.isnan(got[k][r]), k
        assert all(math.isnan(v) for v in got["totals"]), got["totals"]
        keep = np.ones(R, bool)
        keep[r] = False
        for k in ROW_KEYS:
            assert same_bits(got[k][keep], clean[k][keep]), k
        elems = np.ones(D, bool)
        elems[d] = False
        assert same_bits(got["mean"][r, elems], clean["mean"][r, elems]) and same_bits(got["var"][r, elems], clean["var"][r, elems])


def test_argument_errors():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    R, D, S = 4, 8, 3
    f32 = dict(dtype=torch.float32, device="cuda")
    y, t, state = torch.zeros(S * R, D, **f32), torch.zeros(R, D, **f32), torch.zeros(R, 2 * D + 2, **f32)
    rows, tot = torch.zeros(R, **f32), torch.zeros(4, dtype=torch.float64, device="cuda")

    def args(**kw):
        base = dict(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, form=L.MOMENTS_STACKED, noise_var=0.5, ld_out=D)
        base.update(kw)
        return L.MomentsArgs(**base)

    def refused(a):
        st = lib.vbnn_predict_moments(ctx, C.byref(a) if a is not None else None)
        assert st != 0
        with pytest.raises(L.VbnnError, match="invalid argument"):
            L.check(st)

    L.check(lib.vbnn_predict_moments(ctx, C.byref(args(row_log_lik=_p(rows), totals=_p(tot)))))       # the base call is fine
    refused(None)
    refused(args(y=None))
    for k in ("R", "D", "S"):
        refused(args(**{k: 0}))
    refused(args(form=L.MOMENTS_ACCUMULATE, draw=0))                                  # no state
    refused(args(form=L.MOMENTS_ACCUMULATE, state=_p(state), draw=-1))
    refused(args(form=L.MOMENTS_ACCUMULATE, state=_p(state), draw=S))
    refused(args(D=L.MOMENTS_STACKED_MAX_D + 1, ld_y=L.MOMENTS_STACKED_MAX_D + 1, ld_t=L.MOMENTS_STACKED_MAX_D + 1))
    for k in ("row_sq_err", "row_log_lik"):
        refused(args(target=None, **{k: _p(rows)}))
    refused(args(target=None, totals=_p(tot)))
    refused(args(noise_var=0.0, row_log_lik=_p(rows)))
    for bad in (-1.0, float("inf"), float("nan")):
        refused(args(noise_var=bad))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine level
def opt_for(mode, dtype="f32", **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=70, hidden=[50, 34],
             n_classes=12, criterion="mse", type="vb", testSamples=2)
    o.update(kw)
    return o


def data(oracle, R, I0, D):
    return oracle.fill_normal(R, I0, SEED, 4, 0, 0), normal((R, D), 21)


def params64(eng):
    ps = [(host(v.means).astype(np.float64), host(v.lvars).astype(np.float64), host(v.bias).astype(np.float64)) for v in eng.vb]
    return ps, host(eng.weight3).astype(np.float64), host(eng.bias3).astype(np.float64)


def result_arrays(res):
    got = {k: host(getattr(res, k)) for k in ROW_KEYS if getattr(res, k) is not None}
    if res.totals is not None:
        got["totals"] = res.totals
    return got


def restated_draws(oracle, eng, x, d0, S):
    ps, w3, b3 = params64(eng)
    ys, es = zip(*[forward_draw(oracle, ps, w3, b3, eng.mode, SEED, x, d0 + s) for s in range(S)])
    return np.stack(ys), np.max(np.stack(es), 0)


def check_against_restatement(oracle, eng, res, x, d0, S, label):
    """|mean - ref| <= e + kernel tolerance, |var - ref| <= 4 e sqrt(var) + 4 e^2 + kernel tolerance, e the per-row GEMM bound."""
    y64, e = restated_draws(oracle, eng, x, d0, S)
    ref = moments64(y64)
    e = e[:, None]
    got = result_arrays(res)
    check_moments(got, y64, extra_mean=e, extra_var=4 * e * np.sqrt(ref["var"]) + 4 * e * e, label=label, rows=False)
    dm = np.abs(got["mean"] - ref["mean"])
    print(f"{label}: GEMM bound up to {e.max():.3e}; median |d mean| {np.median(dm):.3e}, median |d var| "
          f"{np.median(np.abs(got['var'] - ref['var'])):.3e}")
    return ref, e


@pytest.mark.parametrize("hidden,I0,D,R,S", [([50, 34], 70, 12, 37, 3), ([400, 400], 784, 24, 100, 30)])
def test_lrt_f32_matches_float64_restatement(oracle, hidden, I0, D, R, S):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("lrt", input_size=I0, hidden=hidden, n_classes=D))
    eng.prepare()
    x, t = data(oracle, R, I0, D)
    d0 = eng.draw + 1
    res = eng.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    assert eng.draw == d0 - 1 + S and res.S == S and tuple(res.mean.shape) == (R, D) and res.draws is None
    check_against_restatement(oracle, eng, res, x, d0, S, f"lrt {hidden}")
    assert res.mse == res.totals[0] / (R * D) and res.mean_draw_mse == res.totals[1] / (R * S * D)
    assert res.log_lik == res.totals[2] / R and res.mean_var == res.totals[3] / (R * D)
    assert abs(res.mean_var - float(res.var.double().mean())) <= (D + 16) * EPS * res.mean_var


def test_wn_f32_matches_float64_restatement(oracle):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("wn"))
    eng.prepare()
    x, t = data(oracle, 37, 70, 12)
    res = eng.predict_regression(dev(x), S=3, targets=dev(t))
    assert eng.draw == 3 and not res.stacked and res.row_log_lik is None and res.log_lik is None
    check_against_restatement(oracle, eng, res, x, 1, 3, "wn")


@pytest.mark.parametrize("dtype,kw", [("f32", {}), ("bf16", {}), ("f32", dict(predict_stacked=False)),
                                      ("bf16", dict(predict_rows=4 * 200))],
                         ids=["f32", "bf16", "f32-sequential", "bf16-three-chunks"])
def test_returned_draws_hold_every_output(oracle, dtype, kw):
    """keep_draws: mean, var, the row values and the totals against the kernel-level reference computed from res.draws -- the
    engine's plumbing (buffers, chunk offsets, the draws the final Linear wrote) for f32 and bf16 without a rounding emulation."""
    from vbnn_amd.engine import FusedMLP
    I0, hidden, D, R, S = 256, [512, 256], 64, 512, 4
    eng = FusedMLP(opt_for("lrt", dtype, input_size=I0, hidden=hidden, n_classes=D, **kw))
    x, t = data(oracle, R, I0, D)
    res = eng.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.3, keep_draws=True)
    assert tuple(res.draws.shape) == (S, R, D) and eng.draw == S
    if "predict_rows" in kw:
        assert res.chunks == 3 and res.stacked
    if "predict_stacked" in kw:
        assert not res.stacked
    draws = host(res.draws)
    assert np.isfinite(draws).all() and float(draws.var(0).min()) > 0          # S different draws of every output
    check_moments(result_arrays(res), draws, t, 0.3, label=f"keep_draws {dtype} {kw}")
    # the same call without keep_draws: the same bits
    twin = FusedMLP(opt_for("lrt", dtype, input_size=I0, hidden=hidden, n_classes=D, **kw))
    res2 = twin.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.3)
    for k in ROW_KEYS:
        assert torch.equal(getattr(res, k), getattr(res2, k)), k
    assert res.totals == res2.totals


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_mean_draw_mse_reproduces_test(oracle, mode):
    from vbnn_amd.engine import FusedMLP
    S, R, I0, D = 5, 100, 784, 24
    opt = opt_for(mode, input_size=I0, hidden=[400, 400], n_classes=D, testSamples=S)
    a, b = FusedMLP(opt), FusedMLP(opt)
    x, t = data(oracle, R, I0, D)
    a.prepare(); b.prepare()
    err, _ = a.test(dev(x), dev(t))
    res = b.predict_regression(dev(x), targets=dev(t))
    assert a.draw == b.draw == S and res.S == S
    print(f"{mode}: test() {err!r}, mean_draw_mse {res.mean_draw_mse!r}, mse of the mean {res.mse!r}")
    assert abs(res.mean_draw_mse - err) <= 1e-5 * abs(err)
    assert res.mse <= res.mean_draw_mse * (1 + 1e-6)                           # Jensen: the mean's error is no larger


@pytest.mark.parametrize("mode,dtype", [("lrt", "f32"), ("wn", "f32"), ("lrt", "bf16")])
def test_map_has_no_spread(oracle, mode, dtype):
    from vbnn_amd.engine import FusedMLP
    R, I0, D = 45, 70, 12
    eng = FusedMLP(opt_for(mode, dtype, hidden=[64, 34]))
    eng.prepare()
    x, t = data(oracle, R, I0, D)
    res = eng.predict_regression(dev(x), targets=dev(t), noise_var=0.5, map=True)
    assert res.S == 1 and eng.draw == 0
    assert bool((res.var == 0).all()) and bool((res.row_var == 0).all()) and res.mean_var == 0.0
    assert res.mse == res.mean_draw_mse
    eng.clamp_to_map()
    eng.resetGradients()
    eng.run(dev(x), dev(t), backward=False)
    d = host((res.mean - eng.logits[:R]).abs())
    if dtype == "f32":      # two fp32 passes over the means, each within the GEMM bound of the float64 one
        ps, w3, b3 = params64(eng)
        y64, e = forward_draw(oracle, ps, w3, b3, mode, SEED, x, None)
        assert (d <= 2 * e[:, None]).all(), float(d.max())
        assert (np.abs(host(res.mean) - y64) <= e[:, None]).all()
    else:                   # two bf16 forwards on different kernels: a few bf16 roundings (2^-8) of the outputs' scale
        assert float(d.max()) <= 3e-2 * max(1.0, float(eng.logits[:R].abs().max()))
    assert eng.draw == 0


def test_chunking_second_call_and_fresh_engine(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, D, S = 100, 784, 24, 6
    x, t = data(oracle, R, I0, D)
    kw = dict(input_size=I0, hidden=[400, 400], n_classes=D)
    base, small = FusedMLP(opt_for("lrt", **kw)), FusedMLP(opt_for("lrt", predict_rows=S * 40, **kw))
    base.prepare(); small.prepare()
    r0 = base.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    r1 = small.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    assert r0.chunks == 1 and r1.chunks == 3
    for k in ROW_KEYS:
        assert torch.equal(getattr(r0, k), getattr(r1, k)), k
    for a, b in zip(r0.totals, r1.totals):
        assert abs(a - b) <= 1e-12 * abs(a), (r0.totals, r1.totals)
    fresh = FusedMLP(opt_for("lrt", **kw))                     # never prepared: the shadows test() would have prepared
    r2 = fresh.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    assert torch.equal(r2.mean, r0.mean) and r2.totals == r0.totals
    r3 = base.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5, row0=0)
    assert base.draw == 2 * S and not torch.equal(r3.mean, r0.mean)
    shifted = fresh.predict_regression(dev(x), S=S, row0=1000)                      # other rows of the noise: other draws
    assert fresh.draw == 2 * S and not torch.equal(shifted.mean, r3.mean) and shifted.totals is None and shifted.row_sq_err is None


def test_stacked_and_sequential_agree_within_the_gemm_bound(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, D, S = 100, 784, 24, 5
    x, t = data(oracle, R, I0, D)
    out = []
    for stacked in (True, False):
        eng = FusedMLP(opt_for("lrt", input_size=I0, hidden=[400, 400], n_classes=D, predict_stacked=stacked))
        res = eng.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
        assert res.stacked == stacked
        out.append(res)
    y64, e = restated_draws(oracle, eng, x, 1, S)
    ref = moments64(y64)
    e = e[:, None]
    a, b = out
    dm, dv = host((a.mean - b.mean).abs()), host((a.var - b.var).abs())
    print(f"stacked - sequential: max |d mean| {dm.max():.3e}, max |d var| {dv.max():.3e}")
    assert (dm <= 2 * (e + mean_tol(ref, S))).all()
    assert (dv <= 2 * (4 * e * np.sqrt(ref["var"]) + 4 * e * e + var_tol(ref))).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pruned_view_is_the_hand_pruned_network(oracle, dtype):
    """Under eng.pruned(eng.prune(0.5)): bitwise the result of an engine whose pruned weights were set by hand to what
    vbnn_prune_pack writes for them (mean +0, variance exp(-inf) = +0); and the compressed view of the same pruning agrees with
    the dense one as the sparse tests require of predict (f32: twice the float64 bound)."""
    from vbnn_amd.engine import FusedMLP
    R, I0, D, S = 64, 784, 24, 3
    kw = dict(input_size=I0, hidden=[400, 400], n_classes=D)
    x, t = data(oracle, R, I0, D)
    eng, other = FusedMLP(opt_for("lrt", dtype, **kw)), FusedMLP(opt_for("lrt", dtype, **kw))
    eng.prepare()
    r = eng.prune(fraction=0.5)
    for li, (v, w) in enumerate(zip(eng.vb, other.vb)):
        m = r.mask(li)
        w.means.copy_(torch.where(m, torch.zeros_like(v.means), v.means))
        w.lvars.copy_(torch.where(m, torch.full_like(v.lvars, float("-inf")), v.lvars))
    other.prepare()
    with eng.pruned(r):
        a = eng.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    b = other.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    plain = FusedMLP(opt_for("lrt", dtype, **kw)).predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
    assert eng.draw == other.draw == S
    for k in ROW_KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.totals == b.totals and not torch.equal(a.mean, plain.mean)
    if dtype == "f32":
        eng.draw = 0
        with eng.pruned(r.compress()):
            c = eng.predict_regression(dev(x), S=S, targets=dev(t), noise_var=0.5)
        y64, e = restated_draws(oracle, other, x, 1, S)
        ref = moments64(y64)
        assert (host((a.mean - c.mean).abs()) <= 2 * (e[:, None] + mean_tol(ref, S))).all()
    with pytest.raises(RuntimeError, match="older parameters"):
        eng.prepare()
        with eng.pruned(r):
            eng.predict_regression(dev(x), S=S)
    assert eng.draw == S


def test_refusals_leave_the_counter_alone(oracle):
    from vbnn_amd.engine import FusedMLP
    x, t = data(oracle, 8, 70, 12)
    nll = FusedMLP(opt_for("lrt", criterion="nll", n_classes=10))
    with pytest.raises(ValueError, match="MSE criterion"):
        nll.predict_regression(dev(x), S=2)
    assert nll.draw == 0
    eng = FusedMLP(opt_for("lrt"))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_var"):
            eng.predict_regression(dev(x), S=2, targets=dev(t), noise_var=bad)
    with pytest.raises(ValueError, match="at least one"):
        eng.predict_regression(dev(x), S=0)
    with pytest.raises(ValueError, match="NLL criterion"):
        eng.predict(dev(x), S=2)                                                   # predict keeps refusing the MSE criterion
    assert eng.draw == 0
    res = eng.predict_regression(dev(x), S=2)
    assert eng.draw == 2 and res.totals is None and res.row_sq_err is None and res.row_log_lik is None
