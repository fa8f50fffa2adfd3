"""GPU tests of the Bernoulli likelihood head: vbnn_bce_forward / _backward and vbnn_predict_label_moments
(include/vbnn_hip.h) called directly on uploaded logits against float64 NumPy on the same fp32 inputs (tests/_labels_np.py, whose
docstring derives every bound), their bitwise invariants (the two forms, layouts, S = 1, the integer hit counts, NaN
containment) and argument checks; criterion = "bce" through FusedMLP.run / test / predict_labels, the checkpoint round trip,
the refusals, and one short descent on data.synthetic_multilabel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _labels_np as B
from tests._labels_np import EPS

pytestmark = pytest.mark.gpu

SEED = 3
DS = (1, 3, 4, 5, 63, 64, 65, 256, 257, 260, 1027)
RS = (1, 3, 5)
SS = (1, 2, 3, 7)
EXTREMES = np.array([80.0, -80.0, 100.0, -100.0, 1e4, -1e4], np.float32)
ELEM_KEYS = ("probs", "entropy", "mutual_info")
ROW_KEYS = ("row_entropy", "row_mutual_info", "row_log_lik", "row_marg_log_lik", "row_hits")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def labels(shape, seed, soft=False):
    rng = np.random.default_rng(seed)
    return rng.random(shape).astype(np.float32) if soft else (rng.random(shape) < 0.4).astype(np.float32)


def _padded(a2d, ld, offset=0, fill=float("nan")):
    """a2d (rows x W) on the device with row pitch ld, `fill` in every pad column, starting `offset` floats past a 16-byte
    boundary. Returns (the owning tensor, the data pointer of element [0, 0])."""
    rows, W = a2d.shape
    buf = torch.full((rows * ld + offset + 4,), fill, dtype=torch.float32, device="cuda")
    buf[offset:offset + rows * ld].view(rows, ld)[:, :W] = dev(a2d)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * offset


def layouts(D):
    """The dense aligned layout, odd leading dimensions with NaN pads (the scalar path), and bases 4 bytes off."""
    odd = D + 1 if D % 2 == 0 else D + 2
    return {"dense": {}, "odd-ld": dict(ld_y=odd, ld_t=odd + 2, ld_o=odd), "off-by-one-float": dict(y_offset=1, t_offset=1)}


# ------------------------------------------------------------------------------------------------ the criterion kernel
def run_criterion(z, t, inv_nd, ld_y=None, ld_t=None, ld_o=None, y_offset=0, t_offset=0, accumulate=0, loss0=0.0, hits0=0, backward=False,
                  count=True):
    """vbnn_bce_forward (or _backward) on z (N x D fp32 NumPy) and t (N x D). Returns (loss or None, g as N x D NumPy, the pad
    columns of g, the hit counter or None)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    N, D = z.shape
    ld_y, ld_t, ld_g = ld_y or D, ld_t or D, ld_o or D
    ybuf, yptr = _padded(z, ld_y, y_offset)
    tbuf, tptr = _padded(t, ld_t, t_offset)
    g = torch.full((N, ld_g), -7.0, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), loss0, dtype=torch.float64, device="cuda")
    corr = torch.full((1,), hits0, dtype=torch.int32, device="cuda")
    if backward:
        L.check(lib.vbnn_bce_backward(ctx, yptr, ld_y, tptr, ld_t, N, D, inv_nd, _p(g), ld_g))
    else:
        L.check(lib.vbnn_bce_forward(ctx, yptr, ld_y, tptr, ld_t, N, D, inv_nd, _p(g), ld_g, accumulate, _p(loss), _p(corr) if count else None))
    gh = host(g)
    del ybuf, tbuf
    return (None if backward else float(host(loss)[0])), np.ascontiguousarray(gh[:, :D]), gh[:, D:], \
        (int(host(corr)[0]) if (count and not backward) else None)


def criterion_data(N, D, scale, soft, seed=31):
    z = (np.float32(scale) * normal((N, D), seed)).astype(np.float32)
    k = min(z.size, EXTREMES.size)
    z.flat[:k] = EXTREMES[:k]                                           # the clamp-free criterion's stability: +-80, +-100, +-1e4
    return z, labels((N, D), seed + 1, soft)


@pytest.mark.parametrize("D", DS)
def test_criterion_matches_float64(D):
    for N in RS + ((64,) if D == 257 else ()):                          # (64 x 257: more than one workgroup)
        inv_nd = float(np.float32(1.0 / (N * D)))
        for scale, soft in ((1.0, False), (4.0, True), (30.0, False)):
            z, t = criterion_data(N, D, scale, soft, seed=31 + int(scale))
            base = None
            for name, kw in layouts(D).items():
                loss, g, pads, hits = run_criterion(z, t, inv_nd, **kw)
                assert math.isfinite(loss) and np.isfinite(g).all()
                B.check_criterion(loss, g, hits, z, t, inv_nd, label=f"{N}x{D} x{scale:g} {name}")    # (hits: exact)
                assert (pads == -7.0).all()                             # g's pad columns are not written
                if base is None:
                    base = (loss, g, hits)
                else:                                                   # the layout changes the access path, never the values
                    assert loss == base[0] and same_bits(g, base[1]) and hits == base[2], name
            loss, g, hits = base
            # accumulate = 1 adds to the loss and the hits add to the counter; the backward entry gives the same g bits
            loss2, g2, _, hits2 = run_criterion(z, t, inv_nd, accumulate=1, loss0=2.5, hits0=11)
            assert loss2 == 2.5 + loss and same_bits(g2, g) and hits2 == 11 + hits
            _, g3, _, _ = run_criterion(z, t, inv_nd, backward=True)
            assert same_bits(g3, g)
            loss4, g4, _, _ = run_criterion(z, t, inv_nd, count=False)  # the counter is optional
            assert loss4 == loss and same_bits(g4, g)


def test_criterion_exact_cases():
    """No expf result on the way: z = 0 with t = 1/2 gives sig = t and g = +0 bitwise; (z > 0) == (t > 0.5) counted exactly."""
    N, D = 5, 65
    z, t = np.zeros((N, D), np.float32), np.full((N, D), 0.5, np.float32)
    loss, g, _, hits = run_criterion(z, t, 1.0 / (N * D))
    assert not g.view(np.uint32).any() and hits == N * D
    assert abs(loss - math.log(2.0)) <= 10 * EPS * math.log(2.0)
    t[:, ::2] = 1.0                                                     # z = 0 predicts 0: every label 1 is a miss
    _, _, _, hits = run_criterion(z, t, 1.0 / (N * D))
    assert hits == N * (D // 2)


def test_criterion_nan_stays_in_its_element_and_is_a_miss():
    N, D = 37, 70
    z, t = criterion_data(N, D, 1.0, False)
    inv_nd = float(np.float32(1.0 / (N * D)))
    loss, g, _, hits = run_criterion(z, t, inv_nd)
    for r, d in ((5, 11), (36, 69)):
        bad = z.copy()
        bad[r, d] = np.nan
        loss_b, g_b, _, hits_b = run_criterion(bad, t, inv_nd)
        assert math.isnan(loss_b) and math.isfinite(loss) and np.isnan(g_b[r, d])
        keep = np.ones((N, D), bool)
        keep[r, d] = False
        assert same_bits(g_b[keep], g[keep])
        assert hits_b == hits - int((z[r, d] > 0) == (t[r, d] > 0.5))   # whatever the label says, a NaN logit is a miss


def test_criterion_argument_errors():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    N, D = 4, 8
    f32 = dict(dtype=torch.float32, device="cuda")
    y, t, g = torch.zeros(N, D, **f32), torch.zeros(N, D, **f32), torch.zeros(N, D, **f32)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")

    def fwd(**kw):
        a = dict(y=_p(y), ld_y=D, t=_p(t), ld_t=D, N=N, D=D, inv=0.1, g=_p(g), ld_g=D, acc=0, loss=_p(loss), corr=None)
        a.update(kw)
        return lib.vbnn_bce_forward(ctx, a["y"], a["ld_y"], a["t"], a["ld_t"], a["N"], a["D"], a["inv"], a["g"], a["ld_g"], a["acc"],
                                    a["loss"], a["corr"])

    def bwd(**kw):
        a = dict(y=_p(y), ld_y=D, t=_p(t), ld_t=D, N=N, D=D, inv=0.1, g=_p(g), ld_g=D)
        a.update(kw)
        return lib.vbnn_bce_backward(ctx, a["y"], a["ld_y"], a["t"], a["ld_t"], a["N"], a["D"], a["inv"], a["g"], a["ld_g"])

    def refused(st):
        assert st != 0
        with pytest.raises(L.VbnnError, match="invalid argument"):
            L.check(st)

    L.check(fwd())
    L.check(fwd(g=None))                                                # g is optional in the forward
    L.check(bwd())
    for k in ("y", "t", "loss"):
        refused(fwd(**{k: None}))
    for k in ("y", "t", "g"):
        refused(bwd(**{k: None}))
    for call in (fwd, bwd):
        refused(call(ld_y=D - 1))
        refused(call(ld_g=D - 1))
        refused(call(ld_t=D - 1))
        refused(call(N=0))
        refused(call(D=0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the moments kernel
def run_lmoments(y, t, form, ld_y=None, ld_t=None, ld_o=None, y_offset=0, t_offset=0, totals=True, ctx=None):
    """vbnn_predict_label_moments on y (S x R x D fp32 NumPy) and t (R x D or None): STACKED in one call, ACCUMULATE in S calls
    over a state that starts as NaN (draw 0 must not read it). Returns the outputs as NumPy arrays (+ "totals": 5 floats,
    "pads": the spare columns of the three R x ld_o outputs). ctx: a context handle of the
    caller's (its stream is its own: the uploads are awaited before the calls and vbnn_sync after) in place of the default one."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, own, ctx = L.lib(), ctx is not None, ctx or Context.get().h
    S, R, D = y.shape
    ld_y, ld_t, ld_o = ld_y or D, ld_t or D, ld_o or D
    ybuf, yptr = _padded(y.reshape(S * R, D), ld_y, y_offset)
    tbuf, tptr = _padded(t, ld_t, t_offset) if t is not None else (None, None)
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {k: torch.full((R, ld_o), -7.0, **f32) for k in ELEM_KEYS}
    out.update({k: torch.full((R,), float("nan"), **f32) for k in ROW_KEYS[:2 if t is None else 4]})
    if t is not None:
        out["row_hits"] = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    tot = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda") if (totals and t is not None) else None
    state = torch.full((R, 3 * D + 2), float("nan"), **f32) if form == L.MOMENTS_ACCUMULATE else None
    a = L.LabelMomentsArgs(y=yptr, ld_y=ld_y, target=tptr, ld_t=ld_t, R=R, D=D, S=S, form=form, state=_p(state), ld_out=ld_o,
                           totals=_p(tot), **{k: _p(v) for k, v in out.items()})
    if own:
        torch.cuda.synchronize()
    if form == L.MOMENTS_STACKED:
        L.check(lib.vbnn_predict_label_moments(ctx, C.byref(a)))
    else:
        for s in range(S):
            a.y, a.draw = yptr + 4 * s * R * ld_y, s
            L.check(lib.vbnn_predict_label_moments(ctx, C.byref(a)))
    if own:
        L.check(lib.vbnn_sync(ctx))
    got = {k: host(v) for k, v in out.items()}
    got["pads"] = np.stack([got[k][:, D:] for k in ELEM_KEYS])
    for k in ELEM_KEYS:
        got[k] = np.ascontiguousarray(got[k][:, :D])
    if tot is not None:
        got["totals"] = host(tot).tolist()
    del ybuf, tbuf
    return got


def assert_same_outputs(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if k == "pads":
            continue
        if k == "totals":
            assert same_bits(np.array(a[k]), np.array(b[k])), (what, k, a[k], b[k])
        else:
            assert same_bits(a[k], b[k]), (what, k)


def moments_data(R, D, S, soft=False, scale=3.0):
    y = (np.float32(scale) * normal((S, R, D), 11)).astype(np.float32)
    k = min(R * D, EXTREMES.size)
    y.reshape(S, R * D)[:, :k] = EXTREMES[:k]                            # the same saturated logit in every draw: the clamp
    return y, labels((R, D), 12, soft)


def _cap():
    from vbnn_amd import _lib as L
    return L.LABEL_MOMENTS_STACKED_MAX_D


def _check_forms_and_layouts(R, D, S, soft=False):
    from vbnn_amd import _lib as L
    y, t = moments_data(R, D, S, soft)
    name = f"{R}x{D}x{S}"
    acc = run_lmoments(y, t, L.MOMENTS_ACCUMULATE)
    B.check_label_moments(acc, y, t, label=name + " accumulate")       # (asserts on the CPU side that no element is near a tie)
    assert acc["pads"].size == 0
    if D > _cap():
        with pytest.raises(L.VbnnError, match="STACKED"):
            run_lmoments(y, t, L.MOMENTS_STACKED)
        return
    stk = run_lmoments(y, t, L.MOMENTS_STACKED)
    B.check_label_moments(stk, y, t, label=name + " stacked")
    assert_same_outputs(stk, acc, name)
    for lname, kw in layouts(D).items():
        if not kw:
            continue
        for form in (L.MOMENTS_STACKED, L.MOMENTS_ACCUMULATE):          # pads are not read, a row sum's order depends on D alone
            other = run_lmoments(y, t, form, **kw)
            assert_same_outputs(other, stk, f"{name} {lname} form {form}")
            assert (other["pads"] == -7.0).all(), (name, lname)        # the spare columns of padded outputs are untouched
    # without targets: the remaining outputs are the same bits
    for form in (L.MOMENTS_STACKED, L.MOMENTS_ACCUMULATE):
        bare = run_lmoments(y, None, form)
        assert set(bare) == set(ELEM_KEYS) | {"row_entropy", "row_mutual_info", "pads"}
        for k in bare:
            assert same_bits(bare[k], stk[k]), k


@pytest.mark.parametrize("D", DS)
def test_moments_match_float64_and_the_forms_agree_bitwise(D):
    for R in RS:
        for S in SS:
            _check_forms_and_layouts(R, D, S, soft=(R == 3))


@pytest.mark.parametrize("D", ["cap+4", 1024, 2052, "cap"])
def test_moments_at_the_register_tiles_and_above_the_cap(D):
    """The STACKED form's three register tiles of a workgroup per row meet at D = 1024 / 1028 and 2048 / 2052 and end at the cap;
    above it ACCUMULATE alone runs and STACKED is refused."""
    D = {"cap": _cap(), "cap+4": _cap() + 4}.get(D, D)
    _check_forms_and_layouts(2, D, 2)


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_one_draw_has_exactly_no_mutual_information(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, D in ((5, 65), (3, 1027)):
        y, t = moments_data(R, D, 1)
        got = run_lmoments(y, t, f)
        assert not got["mutual_info"].view(np.uint32).any() and not got["row_mutual_info"].view(np.uint32).any()   # +0 bitwise
        B.check_label_moments(got, y, t, label=f"S = 1 {form}")


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_ties_predict_zero_and_the_counts_are_exact(form):
    """P == Q bitwise (z = 0 in every draw; +a and -a in two draws): the label is predicted 0. The hit counts hold no expf."""
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    R, D = 3, 260
    a = np.abs(normal((R, D), 5)) + np.float32(0.5)
    a[:, ::3] = 0.0
    y = np.stack([a, -a]).astype(np.float32)
    t = labels((R, D), 6)
    t[1] = 0.0                                                          # a row whose every label is 0: an exact match
    got = run_lmoments(y, t, f)
    want = (t <= 0.5).sum(1)
    assert np.array_equal(got["row_hits"], want.astype(np.int32))
    assert got["totals"][3] == float(want.sum()) and got["totals"][4] == float((want == D).sum()) and got["totals"][4] >= 1.0
    assert same_bits(got["probs"][:, ::3], np.full((R, D), 0.5, np.float32)[:, ::3])        # z = 0: 1/2 + 1/2, halved
    assert (np.abs(got["probs"] - 0.5) <= 4 * EPS).all()


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_a_nan_stays_in_its_element_and_its_row_and_is_a_miss(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, D, S, (s, r, d) in ((5, 65, 3, (1, 2, 11)), (3, 1027, 2, (1, 2, 1026))):
        y, t = moments_data(R, D, S)
        clean = run_lmoments(y, t, f)
        ref = B.label_moments64(y, t)
        bad = y.copy()
        bad[s, r, d] = np.nan
        got = run_lmoments(bad, t, f)
        for k in ELEM_KEYS:
            assert np.isnan(got[k][r, d]), k
        for k in ROW_KEYS[:4]:
            assert np.isnan(got[k][r]), k
        miss = int(ref["hit"][r, d])
        assert got["row_hits"][r] == clean["row_hits"][r] - miss
        assert all(math.isnan(got["totals"][k]) for k in (0, 1, 2)), got["totals"]
        assert got["totals"][3] == clean["totals"][3] - miss
        assert got["totals"][4] == clean["totals"][4] - float(clean["row_hits"][r] == D)
        keep = np.ones(R, bool)
        keep[r] = False
        for k in ELEM_KEYS + ROW_KEYS:
            assert same_bits(got[k][keep], clean[k][keep]), k
        elems = np.ones(D, bool)
        elems[d] = False
        for k in ELEM_KEYS:
            assert same_bits(got[k][r, elems], clean[k][r, elems]), k


def test_moments_argument_errors():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    R, D, S = 4, 8, 3
    f32 = dict(dtype=torch.float32, device="cuda")
    y, t, state = torch.zeros(S * R, D, **f32), torch.zeros(R, D, **f32), torch.zeros(R, 3 * D + 2, **f32)
    rows, tot = torch.zeros(R, **f32), torch.zeros(5, dtype=torch.float64, device="cuda")
    hits = torch.zeros(R, dtype=torch.int32, device="cuda")

    def args(**kw):
        base = dict(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=S, form=L.MOMENTS_STACKED, ld_out=D)
        base.update(kw)
        return L.LabelMomentsArgs(**base)

    def refused(a):
        st = lib.vbnn_predict_label_moments(ctx, C.byref(a) if a is not None else None)
        assert st != 0
        with pytest.raises(L.VbnnError, match="invalid argument"):
            L.check(st)

    L.check(lib.vbnn_predict_label_moments(ctx, C.byref(args(row_log_lik=_p(rows), row_hits=_p(hits), totals=_p(tot)))))   # fine
    refused(None)
    refused(args(y=None))
    for k in ("R", "D", "S"):
        refused(args(**{k: 0}))
    refused(args(ld_y=D - 1))
    refused(args(ld_t=D - 1))
    refused(args(probs=_p(t), ld_out=D - 1))
    refused(args(form=2))
    refused(args(form=L.MOMENTS_ACCUMULATE, draw=0))                                  # no state
    refused(args(form=L.MOMENTS_ACCUMULATE, state=_p(state), draw=-1))
    refused(args(form=L.MOMENTS_ACCUMULATE, state=_p(state), draw=S))
    cap = L.LABEL_MOMENTS_STACKED_MAX_D
    refused(args(D=cap + 1, ld_y=cap + 1, ld_t=cap + 1))
    for k in ("row_log_lik", "row_marg_log_lik"):
        refused(args(target=None, **{k: _p(rows)}))
    refused(args(target=None, row_hits=_p(hits)))
    refused(args(target=None, totals=_p(tot)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine level
I0, HIDDEN = 16, [32, 32]
LR = dict(state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})


def opt_for(mode="lrt", dtype="f32", D=5, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=I0, hidden=list(HIDDEN),
             n_classes=D, criterion="bce", type="vb", testSamples=3, fuse_kl=True, **LR)
    o.update(kw)
    return o


def data(R, D, seed=21):
    return normal((R, I0), seed), labels((R, D), seed + 1)


def result_arrays(res):
    got = {k: host(getattr(res, k)) for k in ELEM_KEYS + ROW_KEYS if getattr(res, k) is not None}
    if res.totals is not None:
        got["totals"] = res.totals
    return got


def check_against_own_draws(res, t, label):
    """Every output of a LabelPredictResult recomputed from res.draws by the float64 reference, within the kernel's bounds."""
    draws = host(res.draws)
    assert np.isfinite(draws).all()
    ref = B.check_label_moments(result_arrays(res), draws, t, label=label)
    S, R, D = draws.shape
    assert res.log_lik == res.totals[0] / R and res.marg_log_lik == res.totals[1] / R
    assert res.mean_draw_bce == res.totals[2] / (R * S * D)
    assert res.label_accuracy == 100.0 * ref["totals"][3] / (R * D) and res.exact_match == 100.0 * ref["totals"][4] / R
    return draws


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [1, 5])
def test_one_run_holds_loss_hits_and_gradients(D, dtype):
    """run(): loss, g_logits and the label hits against the float64 criterion evaluated on the engine's own logits; gradBias3 is
    the column sums of g_logits."""
    from vbnn_amd.engine import FusedMLP
    N = 37
    eng = FusedMLP(opt_for("lrt", dtype, D))
    x, t = data(N, D)
    eng.prepare()
    eng.resetGradients()
    eng.sample()
    eng.run(dev(x), dev(t))
    eng.finish()
    loss, correct = eng.loss_and_accuracy()
    logits, g = host(eng.logits[:N]), host(eng.g_logits[:N])
    assert logits.shape == (N, D)
    inv_nd = float(np.float32(1.0 / N / D))
    B.check_criterion(loss, g, correct, logits, t, inv_nd, label=f"run() D {D} {dtype}")
    gb, g64 = host(eng.gradBias3).astype(np.float64), g.astype(np.float64)
    assert (np.abs(gb - g64.sum(0)) <= (N + 16) * EPS * np.abs(g64).sum(0)).all()
    assert np.isfinite(host(eng.gradWeight3)).all() and float(eng.gradWeight3.abs().max()) > 0
    for v in eng.vb:
        assert np.isfinite(host(v.gradWeight)).all() and float(v.gradWeight.abs().max()) > 0


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_mean_draw_bce_reproduces_test(mode):
    """predict_labels consumes test()'s draws: mean_draw_bce is test()'s loss, the mean per-draw label accuracy its accuracy.
    WN is sequential, hence the ACCUMULATE form."""
    from vbnn_amd.engine import FusedMLP
    S, R, D = 4, 37, 5
    opt = opt_for(mode, testSamples=S)
    a, b = FusedMLP(opt), FusedMLP(opt)                     # two engines at the same draw counter
    x, t = data(R, D)
    a.prepare(); b.prepare()
    err, acc = a.test(dev(x), dev(t))
    res = b.predict_labels(dev(x), targets=dev(t), keep_draws=True)
    assert a.draw == b.draw == S and res.S == S and res.stacked == (mode == "lrt")
    draws = check_against_own_draws(res, t, f"{mode} against test()")
    ref = B.criterion64(draws.reshape(S * R, D), np.tile(t, (S, 1)), 1.0)
    scale = ref["loss_mag"] / (R * S * D)
    print(f"{mode}: test() {err!r} / {acc!r}, mean_draw_bce {res.mean_draw_bce!r}, sum |terms| / (R S D) {scale!r}")
    assert abs(res.mean_draw_bce - err) <= 1e-6 * scale
    assert abs(acc - 100.0 * ref["hits"] / (R * S * D)) <= 1e-9


@pytest.mark.parametrize("dtype,kw", [("f32", {}), ("bf16", {}), ("f32", dict(predict_stacked=False))],
                         ids=["f32", "bf16", "f32-sequential"])
@pytest.mark.parametrize("D", [1, 5])
def test_returned_draws_hold_every_output(D, dtype, kw):
    from vbnn_amd.engine import FusedMLP
    R, S = 37, 4
    eng = FusedMLP(opt_for("lrt", dtype, D, **kw))
    x, t = data(R, D)
    res = eng.predict_labels(dev(x), S=S, targets=dev(t), keep_draws=True)
    assert tuple(res.draws.shape) == (S, R, D) and eng.draw == S                    # the draw counter advances by S
    assert res.stacked == ("predict_stacked" not in kw)
    draws = check_against_own_draws(res, t, f"keep_draws D {D} {dtype} {kw}")
    assert float(draws.var(0).min()) > 0                                            # S different draws of every logit
    assert float(res.mutual_info.min()) > -1e-5 and float(res.mutual_info.max()) > 0
    twin = FusedMLP(opt_for("lrt", dtype, D, **kw))                                 # without keep_draws: the same bits
    res2 = twin.predict_labels(dev(x), S=S, targets=dev(t))
    for k in ELEM_KEYS + ROW_KEYS:
        assert torch.equal(getattr(res, k), getattr(res2, k)), k
    assert res.totals == res2.totals and res2.draws is None


def test_chunking_map_and_a_call_without_targets():
    from vbnn_amd.engine import FusedMLP
    R, D, S = 37, 5, 6
    x, t = data(R, D)
    base, small = FusedMLP(opt_for()), FusedMLP(opt_for(predict_rows=S * 13))
    base.prepare(); small.prepare()
    r0 = base.predict_labels(dev(x), S=S, targets=dev(t))
    r1 = small.predict_labels(dev(x), S=S, targets=dev(t))
    assert r0.chunks == 1 and r1.chunks == 3 and base.draw == small.draw == S
    for k in ELEM_KEYS + ROW_KEYS:                                                  # chunked against unchunked, bit for bit
        assert torch.equal(getattr(r0, k), getattr(r1, k)), k
    assert r0.totals[3:] == r1.totals[3:]
    for a, b in zip(r0.totals[:3], r1.totals[:3]):
        assert abs(a - b) <= 1e-12 * abs(a), (r0.totals, r1.totals)
    m = base.predict_labels(dev(x), targets=dev(t), map=True, keep_draws=True)      # one pass on the means: no draw consumed
    assert m.S == 1 and base.draw == S and tuple(m.draws.shape) == (1, R, D)
    assert not host(m.mutual_info).view(np.uint32).any() and not host(m.row_mutual_info).view(np.uint32).any()
    check_against_own_draws(m, t, "map")
    bare = base.predict_labels(dev(x), S=2, row0=1000)
    assert base.draw == S + 2 and bare.totals is None and bare.row_log_lik is None and bare.row_hits is None
    assert bare.label_accuracy is None and tuple(bare.probs.shape) == (R, D) and tuple(bare.row_entropy.shape) == (R,)


def test_pruned_compact_and_held_networks_are_consistent_with_their_own_draws():
    from vbnn_amd.engine import FusedMLP
    R, D, S = 37, 5, 3
    x, t = data(R, D)
    eng = FusedMLP(opt_for())
    eng.prepare()
    plain = eng.predict_labels(dev(x), S=S, targets=dev(t))
    r = eng.prune(fraction=0.5)
    with eng.pruned(r):                                                             # a pruned view
        a = eng.predict_labels(dev(x), S=S, targets=dev(t), keep_draws=True)
    check_against_own_draws(a, t, "pruned view")
    assert not torch.equal(a.probs, plain.probs) and eng.draw == 2 * S
    with eng.pruned(r.compress()):                                                  # the compressed view: the sparse forward
        s = eng.predict_labels(dev(x), S=S, targets=dev(t), keep_draws=True)
    check_against_own_draws(s, t, "compressed view")
    c = eng.compact(eng.prune_units(fraction=0.25))                                 # a compact network
    assert c.criterion == "bce" and c.sizes[1:] != eng.sizes[1:]
    b = c.predict_labels(dev(x), S=S, targets=dev(t), keep_draws=True)
    check_against_own_draws(b, t, "compact network")
    eng.hold_pruned(eng.prune(fraction=0.5))                                        # a held mask
    h = eng.predict_labels(dev(x), S=S, targets=dev(t), keep_draws=True)
    check_against_own_draws(h, t, "held mask")


def _train(e, opt, some):
    for x, t in some:
        e.resetGradients()
        for _ in range(int(opt["S"])):
            e.sample()
            e.run(x, t)
        e.update(opt)


def test_state_dict_round_trip_continues_bit_for_bit():
    from vbnn_amd.engine import FusedMLP
    D, N = 5, 32
    opt = opt_for(S=2, B=1e3)
    batches = [(dev(normal((N, I0), 50 + b)), dev(labels((N, D), 60 + b))) for b in range(4)]
    A = FusedMLP(opt)
    A.prepare()
    _train(A, opt, batches[:2])
    state = A.state_dict()
    assert state["arch"]["criterion"] == "bce"
    Bn = FusedMLP(opt_for(S=2, B=1e3, seed=11))
    Bn.load_state_dict(state)
    from vbnn_amd.checkpoint import CheckpointError
    with pytest.raises(CheckpointError, match="criterion"):
        FusedMLP(opt_for(S=2, B=1e3, criterion="mse")).load_state_dict(state)
    _train(A, opt, batches[2:])
    _train(Bn, opt, batches[2:])
    assert A.draw == Bn.draw == 8
    for v, w in zip(A.vb, Bn.vb):
        for k in ("means", "lvars", "bias"):
            assert torch.equal(getattr(v, k), getattr(w, k)), k
    assert torch.equal(A.weight3, Bn.weight3) and torch.equal(A.bias3, Bn.bias3)
    ra, rb = A.predict_labels(batches[0][0], targets=batches[0][1]), Bn.predict_labels(batches[0][0], targets=batches[0][1])
    assert torch.equal(ra.probs, rb.probs) and ra.totals == rb.totals


def test_refusals_name_the_remedy_and_leave_the_counter_alone():
    from vbnn_amd.engine import FusedMLP
    R, D = 8, 5
    x, t = data(R, D)
    eng = FusedMLP(opt_for())
    for call in (lambda: eng.predict(dev(x), S=2), lambda: eng.predict_classes(dev(x), S=2),
                 lambda: eng.predict_regression(dev(x), S=2), lambda: eng.predict_quantiles(dev(x), [0.1, 0.9], S=2),
                 lambda: eng.predict_analytic(dev(x)), lambda: eng.calibration(None, None)):
        with pytest.raises(ValueError, match="use predict_labels"):
            call()
    with pytest.raises(ValueError, match="targets of shape"):
        eng.predict_labels(dev(x), S=2, targets=dev(labels((R, D + 1), 5)))
    with pytest.raises(ValueError, match="at least one"):
        eng.predict_labels(dev(x), S=0)
    assert eng.draw == 0
    for crit, nc, remedy in (("nll", 10, "predict or predict_classes"), ("mse", 5, "predict_regression"), ("gauss", 10, "predict_regression")):
        other = FusedMLP(opt_for(criterion=crit, n_classes=nc))
        with pytest.raises(ValueError, match=f"Bernoulli criterion.*{remedy}"):
            other.predict_labels(dev(x), S=2)
        assert other.draw == 0
    big = FusedMLP(opt_for(S=2 ** 29))                                              # 8 rows x 5 labels x 2^29 draws: past the int32 counter
    with pytest.raises(ValueError, match="2\\^31"):
        big.run(dev(x), dev(t))
    assert tuple(eng.synthetic_targets(dev(x)).shape) == (R, D)
    st = host(eng.synthetic_targets(dev(x)))
    assert set(np.unique(st)) <= {0.0, 1.0}


def test_trainer_logs_the_label_predictive():
    from vbnn_amd.data import synthetic_multilabel
    from vbnn_amd.train import Main, default_opt
    n, D = 64, 3
    train, test = synthetic_multilabel(n, n, D, seed=5, noise=0.3)
    assert train["inputs"].shape == (n, 1, 16) and test["targets"].shape == (n, D) and set(np.unique(train["targets"])) <= {0.0, 1.0}
    m = Main(default_opt(criterion="bce", n_classes=D, hidden=[24], input_size=16, geometry=(1, 16), testBatchSize=32, testSize=n,
                         batchSize=32, trainSize=n, testSamples=3, S=2, log=False, predictive=True, var_init=1e-2))
    acc, err = m.test(test)
    assert set(m.predictive) == {"devll_pred", "dev_label_acc", "dev_exact_match", "dev_label_mi"}, m.predictive
    assert all(math.isfinite(v) for v in m.predictive.values()) and math.isfinite(err)
    assert 0.0 <= acc <= 100.0 and 0.0 <= m.predictive["dev_exact_match"] <= m.predictive["dev_label_acc"] <= 100.0
    assert m.predictive["dev_label_mi"] > 0 and m.predictive["devll_pred"] < 0
    acc, err = m.train(train)                                           # R x D fp32 labels reach the step; accuracy per label
    assert math.isfinite(err) and 0.0 <= acc <= 100.0


# ------------------------------------------------------------------------------------------------ descent
STEPS = 400


def test_descent_learns_the_labels():
    """16-[32, 32]-4 on data.synthetic_multilabel (512 training rows, 512 held out, noise 0.3): after STEPS steps of the VB engine
    (one LRT draw per step on the whole training set) the MAP loss on the training set is below the initial one, and the
    held-out label accuracy of predict_labels (8 draws) is above the majority-label rate computed from the held-out labels
    themselves (predicting, per label, its more frequent value). The conditions are the two comparisons, not a magnitude."""
    from vbnn_amd.data import synthetic_multilabel
    from vbnn_amd.engine import FusedMLP
    D, n = 4, 512
    train, test = synthetic_multilabel(n, n, D, seed=7, noise=0.3)
    xd, td = dev(train["inputs"].reshape(n, -1)), dev(train["targets"])
    xt, tt = dev(test["inputs"].reshape(n, -1)), dev(test["targets"])
    opt = dict(var_init=1e-4, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=SEED, input_size=16, hidden=[32, 32], n_classes=D,
               criterion="bce", type="vb", testSamples=8, fuse_kl=True,
               state={"learningRate": 5e-2}, meanState={"learningRate": 3e-3}, varState={"learningRate": 1e-3})
    eng = FusedMLP(opt)
    eng.prepare()
    loss0 = eng.predict_labels(xd, targets=td, map=True).mean_draw_bce
    for _ in range(STEPS):
        eng.resetGradients()
        eng.sample()
        eng.run(xd, td)
        eng.update()
    loss1 = eng.predict_labels(xd, targets=td, map=True).mean_draw_bce
    res = eng.predict_labels(xt, targets=tt)
    freq = test["targets"].mean(0)
    majority = 100.0 * float(np.maximum(freq, 1.0 - freq).mean())
    print(f"descent: loss {loss0:.4f} -> {loss1:.4f}; held-out label accuracy {res.label_accuracy:.2f}% (majority-label rate "
          f"{majority:.2f}%), exact match {res.exact_match:.2f}%, log_lik {res.log_lik:.4f}, mean label MI {float(res.mutual_info.mean()):.5f}")
    assert math.isfinite(loss1) and loss1 < loss0
    assert res.label_accuracy > majority
