"""GPU tests of vbnn_predict_quantiles (include/vbnn_hip.h) and FusedMLP.predict_quantiles: the kernel called through ctypes on
uploaded draws -- EMPIRICAL bit for bit the fp32 restatement, the mixture kinds by the 2-ulp bracket criterion with the measured
EPS_F against float64 (tests/_quantiles_np.py, tests/test_quantiles_ref.py) -- calibration by construction, NaN containment,
the adding counts, the argument checks; then the engine and the trainer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _quantiles_np as Q

pytestmark = pytest.mark.gpu

SEED = 3
EPS_F = Q.EPS_F
SENTINEL = -7.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def run_quantiles(y, p, kind, t=None, ld_y=None, y_offset=0, gap=0, ld_q=None, ld_t=None, rows=None, count=None, raw=None,
                  noise_var=0.0, s_min=0.0, s_max=0.0, ctx=None):
    """vbnn_predict_quantiles on y (S x R x W fp32 NumPy; W = D, GAUSS: 2 D) and t (R x D or None). The draws sit on the device
    with row pitch ld_y and `gap` floats between draws, NaN in every pad, the gaps and around, starting y_offset floats past a
    16-byte boundary. rows = (r0, r1): the call works that row range of the same buffer (draw_stride stays the whole draw's).
    count: the int64 device tensor the call adds to (a zeroed one by default). raw: argument overrides (the error tests). ctx: a context handle of the
    caller's (its stream is its own: the uploads are awaited before the call and vbnn_sync after) in place of the default one.
    Returns (status, dict of NumPy outputs + the pads of q)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, own, ctx = L.lib(), ctx is not None, ctx or Context.get().h
    S, R, W = y.shape
    D = W // 2 if kind == Q.GAUSS else W
    ld_y, ld_q, ld_t = ld_y or W, ld_q or D, ld_t or D
    stride = R * ld_y + gap
    ybuf = torch.full((S * stride + y_offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    for s in range(S):
        ybuf[y_offset + s * stride:y_offset + s * stride + R * ld_y].view(R, ld_y)[:, :W] = dev(y[s])
    assert ybuf.data_ptr() % 16 == 0
    r0, r1 = rows or (0, R)
    n, Qn = r1 - r0, len(p)
    plane = R * ld_q + 3
    qbuf = torch.full((Qn * plane,), SENTINEL, dtype=torch.float32, device="cuda")
    pit = torch.full((R, D), SENTINEL, dtype=torch.float32, device="cuda")
    row_le = torch.full((R, Qn), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(Qn, dtype=torch.int64, device="cuda") if count is None else count
    a = L.QuantilesArgs(y=C.c_void_p(ybuf.data_ptr() + 4 * (y_offset + r0 * ld_y)), ld_y=ld_y, draw_stride=stride, R=n, D=D, S=S,
                        kind=kind, Q=Qn, noise_var=noise_var, s_min=s_min, s_max=s_max,
                        q=C.c_void_p(qbuf.data_ptr() + 4 * r0 * ld_q), ld_q=ld_q, plane_stride=plane)
    for j, v in enumerate(p):
        a.p[j] = v
    tbuf = None
    if t is not None:
        tbuf = torch.full((R, ld_t), float("nan"), dtype=torch.float32, device="cuda")
        tbuf[:, :D] = dev(t)
        a.target, a.ld_t = C.c_void_p(tbuf.data_ptr() + 4 * r0 * ld_t), ld_t
        a.pit, a.ld_pit = C.c_void_p(pit.data_ptr() + 4 * r0 * D), D
        a.row_le, a.count_le = C.c_void_p(row_le.data_ptr() + 4 * r0 * Qn), _p(count)
    for k, v in (raw or {}).items():
        setattr(a, k, v)
    if own:
        torch.cuda.synchronize()
    status = lib.vbnn_predict_quantiles(ctx, C.byref(a))
    if own:
        L.check(lib.vbnn_sync(ctx))
    qh = host(qbuf).reshape(Qn, plane)
    planes = qh[:, :R * ld_q].reshape(Qn, R, ld_q)
    out = dict(q=np.ascontiguousarray(planes[:, :, :D]), q_pads=np.concatenate([planes[:, :, D:].ravel(), qh[:, R * ld_q:].ravel()]),
               pit=host(pit), row_le=host(row_le), count_le=host(count))
    del ybuf, tbuf
    return status, out


def ok(status):
    from vbnn_amd import _lib as L
    L.check(status)


def counts_of(q, t):
    """(row_le: R x Q, count_le: Q) of the quantiles q (Q x R x D) and the targets."""
    with np.errstate(invalid="ignore"):
        le = t[None] <= q
    return le.sum(2).T.astype(np.int32), le.sum((1, 2)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ EMPIRICAL: bit for bit
P8 = (0.001, 0.025, 0.1, 0.3, 0.5, 0.9, 0.975, 0.999)
EMP_CASES = {
    # name: (R, D, S, p, layouts)
    "1x1-S1": (1, 1, 1, (0.5,), [{}]),
    "3x5-S2": (3, 5, 2, (0.05, 0.95), [{}, dict(ld_y=8, y_offset=1)]),
    "37x10-S30": (37, 10, 30, (0.05, 0.5, 0.95), [{}, dict(gap=5, ld_q=12), dict(ld_y=12, gap=8, ld_t=11)]),
    "5x260-S7": (5, 260, 7, P8, [{}, dict(ld_y=264, gap=8), dict(y_offset=3)]),        # 16-byte loads, with pads, then 4-byte
    "130x64-S128": (130, 64, 128, (0.025, 0.975), [{}, dict(y_offset=1, ld_q=65)]),
}


def empirical_data(R, D, S, seed):
    y = (2.0 * normal((S, R, D), seed)).astype(np.float32)
    t = normal((R, D), seed + 1)
    y[:, 0, 0] = y[0, 0, 0]                                            # all draws equal: every quantile is that value
    if S > 1:
        y[1, R - 1, D - 1] = y[0, R - 1, D - 1]                        # duplicate draws
    t[0, 0] = y[0, 0, 0]                                               # targets equal to a draw: the <= side
    t[R - 1, D - 1] = y[S - 1, R - 1, D - 1]
    if R > 2:
        t[1, 0] = y[S // 2, 1, 0]
    return y, t


@pytest.mark.parametrize("name", list(EMP_CASES))
def test_empirical_is_the_restatement_bit_for_bit(name):
    R, D, S, p, layouts = EMP_CASES[name]
    y, t = empirical_data(R, D, S, 100 + R)
    p32 = [float(np.float32(v)) for v in p]
    q_ref, pit_ref = Q.empirical32(y, p32, t)
    row_ref, count_ref = counts_of(q_ref, t)
    assert (q_ref[:, 0, 0] == y[0, 0, 0]).all()
    for kw in layouts:
        st, got = run_quantiles(y, p32, Q.EMPIRICAL, t, **kw)
        ok(st)
        assert same_bits(got["q"], q_ref), (name, kw, float(np.abs(got["q"] - q_ref).max()))
        assert same_bits(got["pit"], pit_ref), (name, kw)
        assert np.array_equal(got["row_le"], row_ref) and np.array_equal(got["count_le"], count_ref), (name, kw)
        assert (got["q_pads"] == SENTINEL).all()                       # pads of q are not written
        assert (np.diff(got["q"], axis=0) >= 0).all()
    st, got = run_quantiles(y, p32, Q.EMPIRICAL)                       # without targets: the same quantiles, nothing else
    ok(st)
    assert same_bits(got["q"], q_ref) and (got["pit"] == SENTINEL).all() and (got["row_le"] == -7).all() and not got["count_le"].any()


# ------------------------------------------------------------------------------------------------ the mixture kinds
KERNEL_MIX = [n for n in Q.MIXTURE_CASES if "calibration" not in n]
MIX_LAYOUTS = {"fixed-8x12-S30": dict(ld_y=16, gap=4), "gauss-8x13-S30": dict(ld_y=29, gap=3, y_offset=2), "gauss-5x33-S128": dict(y_offset=1)}


def check_mixture(name, got, y, t, kind, p, kw):
    mu, sigma = Q.components(y, kind, **kw)
    q = got["q"]
    worst = 0.0
    for j, pj in enumerate(p):
        need = Q.eps_needed(q[j], float(np.float32(pj)), mu, sigma)
        worst = max(worst, float(need.max()))
    dpit = float(np.abs(got["pit"].astype(np.float64) - Q.cdf64(t.astype(np.float64), mu, sigma)).max())
    print(f"{name}: the 2-ulp bracket needs eps_F = {worst:.3e}, |pit - F(t)| up to {dpit:.3e} (EPS_F = {EPS_F:.3e})")
    assert np.isfinite(q).all()
    assert worst <= EPS_F and dpit <= EPS_F
    assert (np.diff(q, axis=0) >= 0).all()
    row, count = counts_of(q, t)                                       # exact, from the kernel's own q
    assert np.array_equal(got["row_le"], row) and np.array_equal(got["count_le"], count)


@pytest.mark.parametrize("name", KERNEL_MIX)
def test_mixture_quantiles_meet_the_bracket_criterion(name):
    y, t, kind, p, kw = Q.mixture_case(name)
    if kind == Q.GAUSS and "8x13" in name:                            # s clamped on both sides
        D = y.shape[2] // 2
        assert (y[..., D:] < kw["s_min"]).any() and (y[..., D:] > kw["s_max"]).any()
    st, got = run_quantiles(y, p, kind, t, **kw)
    ok(st)
    check_mixture(name, got, y, t, kind, p, kw)
    if name in MIX_LAYOUTS:                                            # the layout changes the access path, never a bit
        st, got2 = run_quantiles(y, p, kind, t, **MIX_LAYOUTS[name], **kw)
        ok(st)
        for k in ("q", "pit", "row_le", "count_le"):
            assert same_bits(got[k], got2[k]), (name, k)
    if y.shape[0] == 1:                                                # S = 1: q = mu + sigma Phi^-1(p) (the criterion above
        from statistics import NormalDist                              # held it against float64; this names the closed form)
        mu, sigma = Q.components(y, kind, **kw)
        for j, pj in enumerate(p):
            ref = mu[0] + sigma[0] * NormalDist().inv_cdf(float(np.float32(pj)))
            # the density at the root is phi(z) / sigma: an error eps_F of F moves the root by eps_F sigma / phi(z)
            z = NormalDist().inv_cdf(float(np.float32(pj)))
            tol = EPS_F * sigma[0] / NormalDist().pdf(z) + 2 * np.spacing(np.abs(ref).astype(np.float32))
            assert (np.abs(got["q"][j] - ref) <= tol).all()


# ------------------------------------------------------------------------------------------------ calibration by construction
@pytest.mark.parametrize("name", ["empirical", "fixed-calibration", "gauss-calibration"])
def test_calibration_by_construction(name):
    """40,000 targets drawn on the host from the predictive itself: the fraction at or below q_j is p_j up to the binomial's
    spread (5 standard deviations)."""
    if name == "empirical":
        rng = np.random.default_rng(77)
        S, R, D, p, kind, kw = 30, 200, 200, Q.P3, Q.EMPIRICAL, {}
        y = rng.standard_normal((S, R, D)).astype(np.float32)
        a = np.sort(y.astype(np.float64), 0)
        pos = rng.uniform(0, 1, (R, D)) * (S - 1)                      # the linear-interpolated law of the S draws, inverted
        k = np.minimum(pos.astype(np.int64), S - 2)
        lo, hi = np.take_along_axis(a, k[None], 0)[0], np.take_along_axis(a, k[None] + 1, 0)[0]
        t = (lo + (pos - k) * (hi - lo)).astype(np.float32)
    else:
        y, t, kind, p, kw = Q.mixture_case(name)
    assert t.size == 40000
    st, got = run_quantiles(y, p, kind, t, **kw)
    ok(st)
    cal = got["count_le"] / t.size
    for pj, cj in zip(p, cal):
        bound = 5 * math.sqrt(pj * (1 - pj) / t.size)
        print(f"{name}: p = {pj:g}: calibration {cj:.5f} (bound +-{bound:.5f})")
        assert abs(cj - pj) <= bound
    row, count = counts_of(got["q"], t)
    assert np.array_equal(got["row_le"], row) and np.array_equal(got["count_le"], count)
    if kind != Q.EMPIRICAL:
        check_mixture(name, got, y, t, kind, p, kw)
        assert abs(float(got["pit"].mean()) - 0.5) <= 5 * math.sqrt(1 / 12 / t.size)      # the PIT of a calibrated law is uniform


# ------------------------------------------------------------------------------------------------ NaN containment, adding counts
@pytest.mark.parametrize("kind", [Q.EMPIRICAL, Q.FIXED_NOISE, Q.GAUSS])
def test_a_nan_stays_in_its_element(kind):
    R, D, S, p = 9, 12, 30, Q.P3
    if kind == Q.EMPIRICAL:
        y, t = empirical_data(R, D, S, 5)
        kw = {}
    else:
        y, t, _, _, kw = Q.mixture_case("gauss-8x12-S30" if kind == Q.GAUSS else "fixed-8x12-S30")
        R = 8
    st, clean = run_quantiles(y, p, kind, t, **kw)
    ok(st)
    bad_y, bad_t = y.copy(), t.copy()
    bad_y[7, 2, 3] = np.nan                                            # a NaN draw (GAUSS: a NaN mean)
    hit = [(2, 3), (4, 5)]
    if kind == Q.GAUSS:
        bad_y[11, 6, D + 1] = np.nan                                   # a NaN s
        hit.append((6, 1))
    bad_t[4, 5] = np.nan                                               # a NaN target
    st, got = run_quantiles(bad_y, p, kind, bad_t, **kw)
    ok(st)
    keep = np.ones((R, D), bool)
    for r, d in hit:
        keep[r, d] = False
    assert np.isnan(got["q"][:, 2, 3]).all() and np.isnan(got["pit"][2, 3]) and np.isnan(got["pit"][4, 5])
    assert same_bits(got["q"][:, 4, 5], clean["q"][:, 4, 5])           # a NaN target leaves its quantiles alone
    if kind == Q.GAUSS:
        assert np.isnan(got["q"][:, 6, 1]).all() and np.isnan(got["pit"][6, 1])
    assert same_bits(got["q"][:, keep], clean["q"][:, keep]) and same_bits(got["pit"][keep], clean["pit"][keep])
    row, count = counts_of(np.where(keep[None], clean["q"], np.nan), t)                   # the counts skip them
    assert np.array_equal(got["row_le"], row) and np.array_equal(got["count_le"], count)


@pytest.mark.parametrize("kind", [Q.EMPIRICAL, Q.GAUSS])
def test_count_le_adds_over_row_ranges(kind):
    if kind == Q.EMPIRICAL:
        y, t = empirical_data(37, 10, 30, 9)
        p, kw = Q.P3, {}
    else:
        y, t, _, p, kw = Q.mixture_case("gauss-8x13-S30")
    R = y.shape[1]
    st, whole = run_quantiles(y, p, kind, t, **kw)
    ok(st)
    count = torch.zeros(len(p), dtype=torch.int64, device="cuda")
    h = R // 2 + 1
    st, a = run_quantiles(y, p, kind, t, rows=(0, h), count=count, **kw)
    ok(st)
    st, b = run_quantiles(y, p, kind, t, rows=(h, R), count=count, **kw)
    ok(st)
    assert np.array_equal(host(count), whole["count_le"])
    assert same_bits(a["q"][:, :h], whole["q"][:, :h]) and same_bits(b["q"][:, h:], whole["q"][:, h:])
    assert (a["q"][:, h:] == SENTINEL).all() and (b["q"][:, :h] == SENTINEL).all()         # each call wrote its rows only
    assert np.array_equal(a["row_le"][:h], whole["row_le"][:h]) and np.array_equal(b["row_le"][h:], whole["row_le"][h:])
    assert same_bits(a["pit"][:h], whole["pit"][:h]) and same_bits(b["pit"][h:], whole["pit"][h:])


def test_argument_errors():
    from vbnn_amd import _lib as L
    R, D, S = 4, 8, 5
    y, t = normal((S, R, D), 1), normal((R, D), 2)
    yg = normal((S, R, 2 * D), 3)

    def refused(kind=Q.EMPIRICAL, p=(0.1, 0.9), with_t=True, yy=None, **kw):
        raw = kw.pop("raw", None)
        st, got = run_quantiles(y if yy is None else yy, p, kind, t if with_t else None, raw=raw, **kw)
        assert st != 0
        with pytest.raises(L.VbnnError, match="invalid argument"):
            L.check(st)
        assert (got["q"] == SENTINEL).all() and (got["pit"] == SENTINEL).all() and (got["row_le"] == -7).all()
        assert not got["count_le"].any()                               # nothing was launched: the outputs are untouched

    ok(run_quantiles(y, (0.1, 0.9), Q.EMPIRICAL, t)[0])
    refused(raw=dict(S=0))
    refused(raw=dict(S=129))
    refused(raw=dict(Q=0))
    refused(raw=dict(Q=9))
    refused(p=(0.9, 0.1))                                              # not ascending
    refused(p=(0.5, 0.5))
    refused(p=(0.0005, 0.5))                                           # out of range
    refused(p=(0.5, 0.9995))
    refused(p=(float("nan"), 0.5))
    refused(kind=Q.FIXED_NOISE, noise_var=0.0)
    refused(kind=Q.FIXED_NOISE, noise_var=-1.0)
    refused(kind=Q.FIXED_NOISE, noise_var=float("nan"))
    refused(raw=dict(draw_stride=R * D - 1))
    refused(raw=dict(ld_y=D - 1))
    refused(kind=Q.GAUSS, yy=yg, s_min=-1.0, s_max=1.0, raw=dict(ld_y=2 * D - 1))
    refused(kind=Q.GAUSS, yy=yg, s_min=1.0, s_max=0.5)
    refused(raw=dict(kind=3))
    refused(raw=dict(y=None))
    refused(raw=dict(R=0))
    refused(raw=dict(D=0))
    pit = torch.zeros(R, D, dtype=torch.float32, device="cuda")
    rows = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for k, v in (("pit", pit), ("row_le", rows), ("count_le", cnt)):   # each needs a target
        refused(with_t=False, raw={k: C.c_void_p(v.data_ptr())})
    assert not host(pit).any() and not host(rows).any() and not host(cnt).any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine level
def opt_for(mode, dtype="f32", **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=70, hidden=[50, 34],
             n_classes=12, criterion="mse", type="vb", testSamples=2)
    o.update(kw)
    return o


KINDS = {"empirical": dict(criterion="mse"), "fixed_noise": dict(criterion="mse"), "gauss": dict(criterion="gauss")}
KIND_CODE = {"empirical": Q.EMPIRICAL, "fixed_noise": Q.FIXED_NOISE, "gauss": Q.GAUSS}
PROBS = (0.05, 0.5, 0.95)


def call_kw(kind):
    return dict(noise_var=0.3) if kind == "fixed_noise" else {}


def data(oracle, R, kind):
    return oracle.fill_normal(R, 70, SEED, 4, 0, 0), normal((R, 6 if kind == "gauss" else 12), 21)


def kernel_on_draws(res, t, eng):
    kind = KIND_CODE[res.kind]
    kw = dict(noise_var=0.3) if res.kind == "fixed_noise" else {}
    if res.kind == "gauss":
        kw = dict(s_min=eng.logvar_clamp[0], s_max=eng.logvar_clamp[1])
    st, got = run_quantiles(host(res.draws), res.probs, kind, t, **kw)
    ok(st)
    return got


MOMENT_KEYS = ("mean", "var", "row_var", "row_sq_err", "row_log_lik", "noise_var", "row_noise_var")


def same_moments(a, b):
    for k in MOMENT_KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        assert x is None or torch.equal(x, y), k
    assert a.totals == b.totals and (a.mse, a.log_lik, a.mean_var, a.mean_draw_mse) == (b.mse, b.log_lik, b.mean_var, b.mean_draw_mse)


@pytest.mark.parametrize("mode,dtype,kind", [("lrt", "f32", "empirical"), ("lrt", "bf16", "gauss"), ("wn", "f32", "fixed_noise"),
                                             ("wn", "bf16", "empirical"), ("lrt", "f32", "gauss"), ("lrt", "bf16", "fixed_noise")])
def test_engine_quantiles_are_the_kernel_on_the_draws(oracle, mode, dtype, kind):
    from vbnn_amd.engine import FusedMLP
    R, S = 37, 5
    x, t = data(oracle, R, kind)
    eng, twin = FusedMLP(opt_for(mode, dtype, **KINDS[kind])), FusedMLP(opt_for(mode, dtype, **KINDS[kind]))
    res = eng.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t), keep_draws=True, **call_kw(kind))
    assert eng.draw == S and res.S == S and res.kind == kind and tuple(res.quantiles.shape) == (3, R, t.shape[1])
    assert res.probs == [float(np.float32(v)) for v in PROBS]
    got = kernel_on_draws(res, t, eng)
    assert same_bits(host(res.quantiles), got["q"]) and same_bits(host(res.pit), got["pit"])
    assert np.array_equal(host(res.row_le), got["row_le"]) and res.count_le == got["count_le"].tolist()
    assert res.calibration == [c / t.size for c in res.count_le]
    ref = twin.predict_regression(dev(x), S=S, targets=dev(t), **call_kw(kind))    # the same seed and counter
    same_moments(res.moments, ref)
    assert twin.draw == S and res.moments.draws is not None
    # interval(0.9): the 0.05 and 0.95 planes, the coverage their calibrations give
    lo, hi, cov, width = res.interval(0.9)
    assert torch.equal(lo, res.quantiles[0]) and torch.equal(hi, res.quantiles[2])
    assert cov == res.calibration[2] - res.calibration[0]
    assert abs(width - float((res.quantiles[2] - res.quantiles[0]).double().mean())) <= 1e-12 and width > 0
    with pytest.raises(ValueError, match="not among probs"):
        res.interval(0.5)
    # a second call goes on with the next draws; without targets and keep_draws the optional parts are None
    nxt = eng.predict_quantiles(dev(x), PROBS, S=S, **call_kw(kind))
    assert eng.draw == 2 * S and nxt.pit is None and nxt.row_le is None and nxt.calibration is None and nxt.draws is None
    assert nxt.moments.draws is None and not torch.equal(nxt.quantiles, res.quantiles)
    assert nxt.interval(0.9)[2] is None


@pytest.mark.parametrize("kind", ["empirical", "gauss"])
def test_chunks_and_routes(oracle, kind):
    """A multi-chunk call equals the one-chunk call bitwise; the sequential route (predict_stacked=False) gives the kernel's
    result on ITS draws and predict_regression's moments. Its forwards run on other kernels, so its draws differ from the
    stacked route's within the GEMM bound (tests/test_predict_regression_gpu.py) and bitwise equality of the two routes'
    quantiles is not reachable in general: a deliberate deviation from "stacked equals predict_stacked=False". Where the two
    routes' draws do have the same bits the outputs must too; and in every case
    the quantiles differ by no more than the draws do -- empirical: an order statistic, and an interpolation between two, moves
    by at most the largest move of a draw; gauss: the bound derived in the body from the moves of the means and the sigmas."""
    from vbnn_amd.engine import FusedMLP
    R, S = 37, 5
    x, t = data(oracle, R, kind)
    base = FusedMLP(opt_for("lrt", **KINDS[kind]))
    small = FusedMLP(opt_for("lrt", predict_rows=S * 10, **KINDS[kind]))
    seq, seq_twin = (FusedMLP(opt_for("lrt", predict_stacked=False, **KINDS[kind])) for _ in range(2))
    r0 = base.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t), keep_draws=True)
    r1 = small.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t), keep_draws=True)
    assert r0.moments.chunks == 1 and r1.moments.chunks == 4 and r0.moments.stacked and r1.moments.stacked
    assert torch.equal(r0.draws, r1.draws) and torch.equal(r0.quantiles, r1.quantiles) and torch.equal(r0.pit, r1.pit)
    assert torch.equal(r0.row_le, r1.row_le) and r0.count_le == r1.count_le
    r2 = seq.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t), keep_draws=True)
    assert not r2.moments.stacked and seq.draw == S
    got = kernel_on_draws(r2, t, seq)
    assert same_bits(host(r2.quantiles), got["q"]) and same_bits(host(r2.pit), got["pit"])
    same_moments(r2.moments, seq_twin.predict_regression(dev(x), S=S, targets=dev(t)))
    if torch.equal(r0.draws, r2.draws):        # (this small fp32 network: both routes' forwards give the same bits) -- then so
        assert torch.equal(r0.quantiles, r2.quantiles) and torch.equal(r0.pit, r2.pit)       # does everything made from them
        assert torch.equal(r0.row_le, r2.row_le) and r0.count_le == r2.count_le
    if kind == "empirical":
        moved = (r0.draws - r2.draws).abs().amax(0)
        slack = 4 * torch.from_numpy(np.spacing(host(r0.draws.abs().amax(0)))).cuda()
        assert bool(((r0.quantiles - r2.quantiles).abs() <= moved[None] + slack[None]).all())
    else:
        # gauss: if every mean moves by at most delta and every sigma by a factor within [1 / rho, rho], then at
        # x = q + delta + (rho - 1) max_s |q - m_s| every component's CDF is at least what it was at q, so the mixture's is at
        # least p: the quantile moves by no more than that (either way round). On top, each route's q is its own root only up
        # to the kernel's allowance: eps_F over the mixture's density there, and 2 ulps.
        ya, yb = host(r0.draws).astype(np.float64), host(r2.draws).astype(np.float64)
        D = ya.shape[2] // 2
        lo_c, hi_c = base.logvar_clamp
        sa, sb = np.clip(ya[..., D:], lo_c, hi_c), np.clip(yb[..., D:], lo_c, hi_c)
        delta = np.abs(ya[..., :D] - yb[..., :D]).max(0)
        rho = np.exp(0.5 * np.abs(sa - sb).max(0))
        qa, qb = host(r0.quantiles).astype(np.float64), host(r2.quantiles).astype(np.float64)
        worst = 0.0
        for j in range(len(PROBS)):
            reach = np.maximum(np.abs(qa[j][None] - ya[..., :D]), np.abs(qb[j][None] - yb[..., :D])).max(0)
            own = 0.0
            for q, y, sc in ((qa[j], ya, sa), (qb[j], yb, sb)):
                sig = np.exp(0.5 * sc)
                dens = (np.exp(-0.5 * ((q[None] - y[..., :D]) / sig) ** 2) / (sig * math.sqrt(2 * math.pi))).mean(0)
                own = own + EPS_F / dens + 2 * np.spacing(np.abs(q).astype(np.float32))
            bound = delta + (rho - 1.0) * reach + own
            worst = max(worst, float((np.abs(qa[j] - qb[j]) / bound).max()))
            assert (np.abs(qa[j] - qb[j]) <= bound).all()
        print(f"gauss, stacked against sequential: |dq| reaches {worst:.3f} of its bound; the draws moved by up to {delta.max():.3e}")


def test_pruned_view_is_the_hand_pruned_network(oracle):
    from vbnn_amd.engine import FusedMLP
    R, S = 37, 3
    x, t = data(oracle, R, "empirical")
    eng, other = FusedMLP(opt_for("lrt")), FusedMLP(opt_for("lrt"))
    eng.prepare()
    r = eng.prune(fraction=0.5)
    for li, (v, w) in enumerate(zip(eng.vb, other.vb)):
        m = r.mask(li)
        w.means.copy_(torch.where(m, torch.zeros_like(v.means), v.means))
        w.lvars.copy_(torch.where(m, torch.full_like(v.lvars, float("-inf")), v.lvars))
    other.prepare()
    with eng.pruned(r):
        a = eng.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t))
    b = other.predict_quantiles(dev(x), PROBS, S=S, targets=dev(t))
    plain = FusedMLP(opt_for("lrt")).predict_quantiles(dev(x), PROBS, S=S, targets=dev(t))
    assert eng.draw == other.draw == S
    assert torch.equal(a.quantiles, b.quantiles) and torch.equal(a.pit, b.pit) and a.count_le == b.count_le
    same_moments(a.moments, b.moments)
    assert not torch.equal(a.quantiles, plain.quantiles)


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_map_gives_the_one_draw_quantiles(oracle, mode):
    from vbnn_amd.engine import FusedMLP
    x, t = data(oracle, 20, "empirical")
    eng = FusedMLP(opt_for(mode))
    res = eng.predict_quantiles(dev(x), PROBS, targets=dev(t), map=True, keep_draws=True)
    assert res.S == 1 and eng.draw == 0 and tuple(res.draws.shape) == (1, 20, 12)
    for j in range(3):                                                 # S = 1: every quantile is the one draw
        assert torch.equal(res.quantiles[j], res.draws[0])
    assert torch.equal(res.quantiles[0], res.moments.mean) and bool((res.moments.var == 0).all())
    assert set(np.unique(host(res.pit))) <= {0.0, 1.0}


def test_refusals_leave_the_counter_alone(oracle):
    from vbnn_amd.engine import FusedMLP
    x, t = data(oracle, 8, "empirical")
    nll = FusedMLP(opt_for("lrt", criterion="nll", n_classes=10))
    with pytest.raises(ValueError, match="MSE criterion"):
        nll.predict_quantiles(dev(x), PROBS, S=2)
    assert nll.draw == 0
    gauss = FusedMLP(opt_for("lrt", criterion="gauss"))
    with pytest.raises(ValueError, match="noise_var must be None"):
        gauss.predict_quantiles(dev(x), PROBS, S=2, noise_var=0.5)
    assert gauss.draw == 0
    eng = FusedMLP(opt_for("lrt"))
    with pytest.raises(ValueError, match="at most 128"):
        eng.predict_quantiles(dev(x), PROBS, S=129)
    with pytest.raises(ValueError, match="at least one"):
        eng.predict_quantiles(dev(x), PROBS, S=0)
    for bad in ((), tuple(np.linspace(0.1, 0.9, 9)), (0.9, 0.1), (0.5, 0.5), (0.0, 0.5), (0.5, 1.0), (float("nan"),)):
        with pytest.raises(ValueError, match="probabilities|probs"):
            eng.predict_quantiles(dev(x), bad, S=2)
    with pytest.raises(ValueError, match="noise_var"):
        eng.predict_quantiles(dev(x), PROBS, S=2, noise_var=-1.0)
    assert eng.draw == 0
    res = eng.predict_quantiles(dev(x), PROBS, S=2)
    assert eng.draw == 2 and res.pit is None


def test_trainer_logs_the_calibration(tmp_path):
    """Main.test with opt.predictive and opt.quantile_probs: dev_cal@<p> beside the existing series, which keep their values
    (the same draws); none without the option."""
    from vbnn_amd.data import Dataset
    from vbnn_amd.train import Main, default_opt
    n, I0, D = 64, 16, 3
    ds = Dataset(inputs=normal((n, 4, 4), 41), targets=normal((n, D), 42))
    base = dict(hidden=[24], input_size=I0, geometry=(4, 4), testBatchSize=32, testSize=n, batchSize=32, trainSize=n, testSamples=3,
                S=1, log=False, predictive=True, var_init=1e-2)
    for crit, extra in (("gauss", {}), ("mse", {}), ("mse", dict(noise_var=0.5))):
        kw = dict(criterion=crit, n_classes=2 * D if crit == "gauss" else D, **base, **extra)
        plain, cal = Main(default_opt(**kw)), Main(default_opt(quantile_probs=[0.05, 0.95], **kw))
        plain.test(ds)
        cal.test(ds)
        assert not any(k.startswith("dev_cal@") for k in plain.predictive)
        assert set(cal.predictive) == set(plain.predictive) | {"dev_cal@0.05", "dev_cal@0.95"}
        for k, v in plain.predictive.items():                          # the existing series: unchanged
            assert cal.predictive[k] == v, k
        assert 0.0 <= cal.predictive["dev_cal@0.05"] <= cal.predictive["dev_cal@0.95"] <= 1.0
        assert cal.net.draw == plain.net.draw                          # no second set of draws
    # through run(): the series reach the log, beside the existing ones
    import os
    from vbnn_amd.logger import read_data
    for name, extra in (("cal", dict(quantile_probs=[0.05, 0.95])), ("plain", {})):
        d = str(tmp_path / name)
        m = Main(default_opt(criterion="mse", n_classes=D, network_name=d, **{**base, "log": True}, **extra))
        rec = m.run(ds, ds, epochs=1)[-1]
        m.log.close()
        for series in ("dev_cal@0.05", "dev_cal@0.95"):
            assert (series in rec) == (name == "cal")
            assert os.path.exists(os.path.join(d, series)) == (name == "cal")
            if name == "cal":
                assert read_data(os.path.join(d, series)) == [pytest.approx(rec[series], rel=1e-6)]
        assert os.path.exists(os.path.join(d, "dev_epi_var"))
