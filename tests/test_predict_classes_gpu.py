"""GPU tests of the class-probability predictive for any class count: vbnn_predict_class_moments (include/vbnn_hip.h) called
directly on uploaded logits against float64 NumPy on the same fp32 inputs (tests/_classes_np.py), its bitwise invariants (the
two forms, layouts, skipped outputs, S = 1, NaN containment), its argument checks; and FusedMLP.predict_classes over it against
the kernel-level reference on its own returned draws (f32 and bf16), a float64 restatement of the forward, predict() at 10
classes, test() at 20, and its chunking / view / refusal contract; train.py's predictive series at 20 classes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests._classes_np import EPS, KERNEL_CASES, case_inputs, check_classes, classes64, entropy_tol, expected_entropy_tol, logp_tol
from tests._regress_np import STREAM_ZETA, forward_draw

pytestmark = pytest.mark.gpu

SEED = 3
F32_KEYS = ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "topk_prob")
ALL_KEYS = F32_KEYS + ("pred", "topk_idx")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ kernel level
def _padded(a2d, ld, offset=0):
    """a2d (rows x C) on the device with row pitch ld, NaN in every pad column, starting `offset` floats past a 16-byte boundary.
    Returns (the owning tensor, the data pointer of element [0, 0])."""
    rows, Cn = a2d.shape
    buf = torch.full((rows * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + rows * ld].view(rows, ld)[:, :Cn] = dev(a2d)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * offset


def run_classes(y, t, form, K=0, ld_y=None, y_offset=0, probs=True, ld_state=None, n_calls=None, ctx=None):
    """vbnn_predict_class_moments on y (S x R x C fp32 NumPy) and t (R int32 or None): STACKED in one call, ACCUMULATE in S calls
    over a state that starts as NaN (draw 0 must not read it). Returns the outputs as NumPy arrays (+ "totals": 5 floats, and for
    ACCUMULATE "rows": the state's three row values, "L": its R x C running logsumexp; n_calls: only that many draws are run). ctx: a context handle of the
    caller's (its stream is its own: the uploads are awaited before the calls and vbnn_sync after) in place of the default one."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, own, ctx = L.lib(), ctx is not None, ctx or Context.get().h
    S, R, Cn = y.shape
    ld_y = ld_y or Cn
    ybuf, yptr = _padded(y.reshape(S * R, Cn), ld_y, y_offset)
    tdev = dev(t) if t is not None else None
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {k: torch.full((R,), float("nan"), **f32) for k in ("entropy", "expected_entropy", "mutual_info")}
    out["pred"] = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    if probs:
        out["probs"], out["log_probs"] = torch.full((R, Cn), float("nan"), **f32), torch.full((R, Cn), float("nan"), **f32)
    if K:
        out["topk_idx"] = torch.full((R, K), -1, dtype=torch.int32, device="cuda")
        out["topk_prob"] = torch.full((R, K), float("nan"), **f32)
    tot = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda") if t is not None else None
    ld_state = ld_state or (Cn + 3 + 3) // 4 * 4
    state = torch.full((R, ld_state), float("nan"), **f32) if form == L.MOMENTS_ACCUMULATE else None
    a = L.ClassMomentsArgs(y=yptr, ld_y=ld_y, target=_p(tdev), R=R, C=Cn, S=S, form=form, K=K, state=_p(state), ld_state=ld_state,
                           probs=_p(out.get("probs")), log_probs=_p(out.get("log_probs")), ld_out=Cn, entropy=_p(out["entropy"]),
                           expected_entropy=_p(out["expected_entropy"]), mutual_info=_p(out["mutual_info"]), pred=_p(out["pred"]),
                           topk_idx=_p(out.get("topk_idx")), topk_prob=_p(out.get("topk_prob")), totals=_p(tot))
    if own:
        torch.cuda.synchronize()
    if form == L.MOMENTS_STACKED:
        L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a)))
    else:
        for s in range(S if n_calls is None else n_calls):
            a.y, a.draw = yptr + 4 * s * R * ld_y, s
            L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a)))
    if own:
        L.check(lib.vbnn_sync(ctx))
    got = {k: host(v) for k, v in out.items()}
    if tot is not None:
        got["totals"] = host(tot).tolist()
        if state is not None:
            got["rows"] = host(state)[:, Cn:Cn + 3].copy()
    if state is not None:
        got["L"] = host(state)[:, :Cn].copy()
    del ybuf
    return got


def assert_same_outputs(a, b, what, keys=None):
    keys = (set(a) & set(b) if keys is None else set(keys)) - {"rows", "L"}
    for k in keys:
        if k == "totals":
            assert same_bits(np.array(a[k]), np.array(b[k])), (what, k, a[k], b[k])
        else:
            assert same_bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_matches_float64_and_the_forms_agree_bitwise(name):
    from vbnn_amd import _lib as L
    R, Cn, S, scale, kw = KERNEL_CASES[name]
    y, t, K = case_inputs(name)
    acc = run_classes(y, t, L.MOMENTS_ACCUMULATE, K, **kw)
    check_classes(acc, y, t, K, label=name + " accumulate")
    if scale == 40.0:       # what the case is there for: probabilities underflow to 0 while log p stays finite far below log(TINY),
        # and every draw's winner holds ~1/S of the mass, so the leading classes are near-ties that only the exact checks order
        assert (acc["probs"] == 0).any() and np.isfinite(acc["log_probs"]).all() and acc["log_probs"].min() < -150
        top = -np.sort(-classes64(y)["log_probs"], axis=1)[:, :K]
        print(f"{name}: float64 log p of the top class per row {top[:, 0].tolist()}, top-1 minus top-{K} at most {(top[:, 0] - top[:, -1]).max():.3e}")
        assert (np.abs(top[:, 0] + math.log(S)) <= 1e-6).all()
    # an odd row pitch of the state: the scalar path, the same bits
    odd = run_classes(y, t, L.MOMENTS_ACCUMULATE, K, ld_state=Cn + 3 + (Cn % 2 == 0), **kw)
    assert_same_outputs(odd, acc, name + " odd ld_state", set(acc))
    if Cn > L.CLASS_MOMENTS_STACKED_MAX_C:
        with pytest.raises(L.VbnnError, match="STACKED"):
            run_classes(y, t, L.MOMENTS_STACKED, K, **kw)
        full, form = acc, L.MOMENTS_ACCUMULATE
    else:
        full, form = run_classes(y, t, L.MOMENTS_STACKED, K, **kw), L.MOMENTS_STACKED
        check_classes(dict(full, rows=acc["rows"]), y, t, K, label=name + " stacked")
        assert_same_outputs(full, acc, name + " stacked against accumulate", set(full))
    if kw:      # the layout changes the access path, never the values: pads are not read, a row sum's order depends on C alone
        assert_same_outputs(full, run_classes(y, t, form, K), name + " against the dense aligned layout", set(full) - {"rows"})
    # without targets, and with probs / log_probs skipped: the remaining outputs are the same bits
    bare = run_classes(y, None, form, K, **kw)
    assert "totals" not in bare
    assert_same_outputs(bare, full, name + " without targets", set(bare))
    slim = run_classes(y, t, form, K, probs=False, **kw)
    assert "probs" not in slim and "log_probs" not in slim
    assert_same_outputs(slim, full, name + " without probs", set(slim) - {"rows"})
    check_classes(slim, y, t, K, label=name + " without probs")
    # K = 0: pred and everything else unchanged
    k0 = run_classes(y, t, form, 0, **kw)
    assert "topk_idx" not in k0 and k0["totals"][4] == 0.0
    assert_same_outputs(k0, full, name + " K = 0", set(k0) - {"totals", "rows"})
    assert k0["totals"][:4] == full["totals"][:4]


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_one_draw_is_its_log_softmax_and_equal_draws_carry_no_information(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, Cn in ((37, 17), (3, 1028)):
        y = (np.float32(2) * np.random.default_rng(5).standard_normal((1, R, Cn)).astype(np.float32)).astype(np.float32)
        t = np.random.default_rng(6).integers(0, Cn, R).astype(np.int32)
        got = run_classes(y, t, f, 3)
        check_classes(got, y, t, 3, label=f"S = 1 {form}")
        assert (got["mutual_info"] == 0).all()
        assert same_bits(got["expected_entropy"], got["entropy"])
        assert got["totals"][0] == got["totals"][2] and got["totals"][1] == got["totals"][3]
        # log_probs is the draw's o, bit for bit: o is what draw 0 of a longer prediction leaves in the ACCUMULATE state
        y5 = np.repeat(y, 5, axis=0)
        o = run_classes(y5, t, L.MOMENTS_ACCUMULATE, 3, n_calls=1)["L"]
        assert same_bits(got["log_probs"], o)
        o64 = classes64(y)["o"][0]
        assert (np.abs(o - o64) <= (Cn + 16) * EPS * np.maximum(np.abs(o64), 1.0)).all()
        got5 = run_classes(y5, t, f, 3)
        ref = check_classes(got5, y5, t, 3, label=f"equal draws {form}")
        tol = entropy_tol(ref, 5) + expected_entropy_tol(ref)
        assert (np.abs(got5["mutual_info"]) <= tol).all(), float((np.abs(got5["mutual_info"]) / tol).max())
        # ... and one draw through the other form's route to o: S = 1 in STACKED and ACCUMULATE are the same bits
        other = run_classes(y, t, L.MOMENTS_ACCUMULATE if form == "stacked" else L.MOMENTS_STACKED, 3)
        assert_same_outputs(got, other, "S = 1, the other form")


@pytest.mark.parametrize("form", ["stacked", "accumulate"])
def test_a_nan_stays_in_its_row_and_the_totals(form):
    from vbnn_amd import _lib as L
    f = L.MOMENTS_STACKED if form == "stacked" else L.MOMENTS_ACCUMULATE
    for R, Cn, S, (s, r, c) in ((37, 17, 3, (1, 5, 11)), (6, 1028, 4, (3, 2, 1027))):
        y = (np.float32(2) * np.random.default_rng(7).standard_normal((S, R, Cn)).astype(np.float32)).astype(np.float32)
        t = np.random.default_rng(8).integers(0, Cn, R).astype(np.int32)
        clean = run_classes(y, t, f, 4)
        bad = y.copy()
        bad[s, r, c] = np.nan
        got = run_classes(bad, t, f, 4)
        for k in F32_KEYS:
            assert np.isnan(got[k][r]).all(), k
        assert math.isnan(got["totals"][0]) and math.isnan(got["totals"][2]), got["totals"]
        for k in ("pred", "topk_idx"):
            assert (got[k][r] >= 0).all() and (got[k][r] < Cn).all(), k
        keep = np.ones(R, bool)
        keep[r] = False
        for k in ALL_KEYS:
            assert same_bits(got[k][keep], clean[k][keep]), k


def test_argument_errors():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    R, Cn, S = 4, 8, 3
    f32 = dict(dtype=torch.float32, device="cuda")
    y, state = torch.zeros(S * R, Cn, **f32), torch.zeros(R, Cn + 4, **f32)
    t = torch.zeros(R, dtype=torch.int32, device="cuda")
    tot, big = torch.zeros(5, dtype=torch.float64, device="cuda"), torch.zeros(R, 8, **f32)
    idx = torch.zeros(R, 8, dtype=torch.int32, device="cuda")

    def args(**kw):
        base = dict(y=_p(y), ld_y=Cn, target=_p(t), R=R, C=Cn, S=S, form=L.MOMENTS_STACKED, K=2, ld_out=Cn)
        base.update(kw)
        return L.ClassMomentsArgs(**base)

    def refused(a, match="invalid argument", ctx=ctx):
        st = lib.vbnn_predict_class_moments(ctx, C.byref(a) if a is not None else None)
        assert st != 0
        with pytest.raises(L.VbnnError, match=match):
            L.check(st)

    acc = dict(form=L.MOMENTS_ACCUMULATE, state=_p(state), ld_state=Cn + 4)
    L.check(lib.vbnn_predict_class_moments(ctx, C.byref(args(totals=_p(tot), topk_idx=_p(idx), topk_prob=_p(big)))))   # the base call is fine
    L.check(lib.vbnn_predict_class_moments(ctx, C.byref(args(draw=0, **acc))))
    refused(None)
    refused(args(), ctx=None)
    refused(args(y=None))
    for k in ("R", "C", "S"):
        refused(args(**{k: 0}))
    refused(args(ld_y=Cn - 1))
    for K in (-1, 9):
        refused(args(K=K))
    refused(args(C=4, ld_y=4, K=5))                                                   # K above C
    refused(args(form=L.MOMENTS_ACCUMULATE, draw=0))                                  # no state
    refused(args(draw=0, **dict(acc, ld_state=Cn + 2)))
    refused(args(draw=-1, **acc))
    refused(args(draw=S, **acc))
    refused(args(C=L.CLASS_MOMENTS_STACKED_MAX_C + 1, ld_y=L.CLASS_MOMENTS_STACKED_MAX_C + 1), match="STACKED")
    refused(args(target=None, totals=_p(tot)))
    refused(args(K=0, topk_idx=_p(idx)))
    refused(args(K=0, topk_prob=_p(big)))
    refused(args(probs=_p(big), ld_out=Cn - 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine level
def opt_for(mode, dtype="f32", **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=70, hidden=[50, 34],
             n_classes=20, type="vb", testSamples=3)
    o.update(kw)
    return o


def data(oracle, R, I0, Cn):
    return oracle.fill_normal(R, I0, SEED, 4, 0, 0), (np.arange(R) * 7 % Cn).astype(np.int32)


def params64(eng):
    ps = [(host(v.means).astype(np.float64), host(v.lvars).astype(np.float64), host(v.bias).astype(np.float64)) for v in eng.vb]
    return ps, host(eng.weight3).astype(np.float64), host(eng.bias3).astype(np.float64)


def result_arrays(res):
    got = {k: host(getattr(res, k)) for k in ALL_KEYS if getattr(res, k) is not None}
    if res.totals is not None:
        got["totals"] = res.totals
    return got


def assert_same_results(a, b, what, skip=()):
    for k in ALL_KEYS:
        if k in skip:
            continue
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert torch.equal(x, y) and same_bits(host(x), host(y)), (what, k)


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_f32_returned_draws_hold_every_output_and_match_float64(oracle, mode):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 37, 70, 20, 3, 5
    eng = FusedMLP(opt_for(mode))
    eng.prepare()
    x, t = data(oracle, R, I0, Cn)
    d0 = eng.draw + 1
    res = eng.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
    assert eng.draw == d0 - 1 + S and res.S == S and tuple(res.draws.shape) == (S, R, Cn)
    assert res.stacked == (mode == "lrt") and tuple(res.topk_idx.shape) == (R, K)
    draws = host(res.draws)
    check_classes(result_arrays(res), draws, t, K, label=f"engine {mode}")
    ps, w3, b3 = params64(eng)
    for s in range(S):                         # the draws themselves: the float64 forward, within its per-row GEMM bound
        y64, e = forward_draw(oracle, ps, w3, b3, mode, SEED, x, d0 + s)
        d = np.abs(draws[s] - y64)
        print(f"{mode} draw {s}: max |d logit| / bound {float((d / e[:, None]).max()):.3f}")
        assert (d <= e[:, None]).all()
    tot = res.totals
    assert (res.nll, res.accuracy) == (tot[0] / R, 100.0 * tot[1] / R)
    assert (res.mean_draw_nll, res.mean_draw_accuracy, res.topk_accuracy) == (tot[2] / (R * S), 100.0 * tot[3] / (R * S), 100.0 * tot[4] / R)
    assert res.topk_accuracy >= res.accuracy
    # the same call without keep_draws, on a twin: the same bits
    twin = FusedMLP(opt_for(mode))
    res2 = twin.predict_classes(dev(x), S=S, targets=dev(t), topk=K)
    assert res2.draws is None and res2.totals == res.totals
    assert_same_results(res, res2, "keep_draws")


def test_bf16_returned_draws_hold_every_output(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 37, 70, 20, 3, 5
    eng = FusedMLP(opt_for("lrt", "bf16"))
    x, t = data(oracle, R, I0, Cn)
    res = eng.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
    draws = host(res.draws)
    assert np.isfinite(draws).all() and float(draws.var(0).min()) > 0 and eng.draw == S
    check_classes(result_arrays(res), draws, t, K, label="engine bf16")


def test_ten_classes_agree_with_predict(oracle):
    """predict() forms the logits inside its head from h; predict_classes reads the final Linear's f32 outputs: two fp32 GEMMs
    over the same h, each within 4e-6 sum |h| |w3| of the exact logit, a log-probability within twice a logit's error."""
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S = 37, 70, 10, 3
    kw = dict(hidden=[32], n_classes=Cn)
    a, b = FusedMLP(opt_for("lrt", **kw)), FusedMLP(opt_for("lrt", **kw))
    x, t = data(oracle, R, I0, Cn)
    ra = a.predict(dev(x), S=S, targets=dev(t))
    rb = b.predict_classes(dev(x), S=S, targets=dev(t), keep_draws=True)
    assert a.draw == b.draw == S
    if a.device_draw:
        assert a._draw_dev.cpu().tolist() == b._draw_dev.cpu().tolist()
    ps, w3, b3 = params64(b)
    e = np.zeros(R)
    for s in range(S):                          # 4e-6 sum |h| |w3| per row, h from the float64 forward of the same draw
        h = x.astype(np.float64)
        for li, (mu, lv, bb) in enumerate(ps):
            z = oracle.fill_normal(R, mu.shape[0], SEED, STREAM_ZETA, li, 1 + s, 0).astype(np.float64)
            h = np.maximum(h @ mu.T + bb + np.sqrt((h * h) @ np.exp(lv).T) * z, 0.0)
        e = np.maximum(e, 4e-6 * (np.abs(h) @ np.abs(w3).T).max(1))
    gemm = 2 * 2 * e                            # twice the bound (two GEMMs), a log-probability twice a logit
    ref = classes64(host(rb.draws), t)
    tl = logp_tol(ref, S)
    d = np.abs(host(ra.log_probs) - host(rb.log_probs))
    print(f"predict against predict_classes: max |d log p| {d.max():.3e}, bound {float((gemm[:, None] + 2 * tl).min()):.3e}")
    assert (d <= gemm[:, None] + 2 * tl).all()
    lgC = 1 + math.log(Cn)
    te, tx = entropy_tol(ref, S) + gemm * lgC, expected_entropy_tol(ref) + gemm * lgC
    assert (np.abs(host(ra.entropy) - host(rb.entropy)) <= 2 * te).all()
    assert (np.abs(host(ra.mutual_info) - host(rb.mutual_info)) <= 2 * (te + tx)).all()


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_mean_draw_metrics_reproduce_test_at_twenty_classes(oracle, mode):
    from vbnn_amd.engine import FusedMLP
    S, R, I0, Cn = 5, 100, 70, 20
    opt = opt_for(mode, testSamples=S)
    a, b = FusedMLP(opt), FusedMLP(opt)
    x, t = data(oracle, R, I0, Cn)
    a.prepare(); b.prepare()
    err, acc = a.test(dev(x), dev(t))
    res = b.predict_classes(dev(x), targets=dev(t), keep_draws=True)
    assert a.draw == b.draw == S and res.S == S
    srt = np.sort(host(res.draws), axis=2)
    close = int(((srt[:, :, -1] - srt[:, :, -2]) < 1e-4 * np.abs(srt).max()).sum())
    print(f"{mode}: test() {err!r} {acc!r}, mean_draw_nll {res.mean_draw_nll!r}, mean_draw_accuracy {res.mean_draw_accuracy!r}; "
          f"{close} of {R * S} (row, draw) pairs with a top-2 gap under 1e-4 max|logit|")
    assert close <= 0.02 * R * S
    assert abs(res.mean_draw_nll - err) <= 3e-5 * abs(err) + 1e-6
    assert abs(res.mean_draw_accuracy - acc) <= 100.0 / R * close + 1e-9


def test_chunking_gives_the_same_bits_per_row(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 37, 70, 20, 3, 4
    x, t = data(oracle, R, I0, Cn)
    base, small = FusedMLP(opt_for("lrt")), FusedMLP(opt_for("lrt", predict_rows=S * 16))
    r0 = base.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
    r1 = small.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
    assert r0.chunks == 1 and r1.chunks == 3 and r0.stacked and r1.stacked
    assert torch.equal(r0.draws, r1.draws)
    assert_same_results(r0, r1, "chunks")
    assert [r0.totals[k] for k in (1, 3, 4)] == [r1.totals[k] for k in (1, 3, 4)]
    for k in (0, 2):
        assert abs(r0.totals[k] - r1.totals[k]) <= 1e-12 * abs(r0.totals[k])
    r2 = base.predict_classes(dev(x), S=S, targets=dev(t), row0=0)            # a second call: the next draws
    assert base.draw == 2 * S and not torch.equal(r2.log_probs, r0.log_probs) and r2.topk_idx is None and r2.topk_accuracy is None
    nt = small.predict_classes(dev(x), S=S, row0=0)
    assert nt.totals is None and nt.nll is None and torch.equal(nt.log_probs, r2.log_probs)


def test_stacked_and_sequential(oracle):
    """The sequential pass runs every draw through the forward on its own, the stacked pass all S in one launch per layer.
    On this network (fp32, 70-50-34) both take the same fp32 GEMM kernel with the same K order per output element, and the
    noise is addressed by (draw, row), so the logits -- and with them every output of the moments kernel, whose two forms are
    bitwise equal given equal logits -- are the same bits: that is what held on an MI355X. Should the returned draws ever
    differ (another kernel choice for the stacked row count), the outputs are held to the GEMM bound instead, and the test
    prints which of the two it was."""
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 37, 70, 20, 3, 4
    x, t = data(oracle, R, I0, Cn)
    out = []
    for stacked in (True, False):
        eng = FusedMLP(opt_for("lrt", predict_stacked=stacked))
        res = eng.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
        assert res.stacked == stacked and eng.draw == S
        out.append(res)
    a, b = out
    if torch.equal(a.draws, b.draws):
        print("stacked and sequential: the same logits bit for bit; every output must be too")
        assert_same_results(a, b, "stacked against sequential")
        assert a.totals == b.totals
        return
    ps, w3, b3 = params64(eng)
    e = np.max(np.stack([forward_draw(oracle, ps, w3, b3, "lrt", SEED, x, 1 + s)[1] for s in range(S)]), 0)
    ref = classes64(host(a.draws))
    d = np.abs(host(a.log_probs) - host(b.log_probs))
    print(f"stacked and sequential: logits differ (max {float((a.draws - b.draws).abs().max()):.3e}); max |d log p| {d.max():.3e}")
    assert (np.abs(host(a.draws) - host(b.draws)) <= 2 * e[None, :, None]).all()
    assert (d <= 2 * (2 * e[:, None] + logp_tol(ref, S))).all()


def test_a_head_above_the_cap_accumulates_from_a_stacked_forward(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 3, 70, 4100, 3, 8
    eng = FusedMLP(opt_for("lrt", hidden=[32], n_classes=Cn))
    x, t = data(oracle, R, I0, Cn)
    res = eng.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_draws=True)
    assert res.stacked and eng.draw == S and tuple(res.probs.shape) == (R, Cn)
    check_classes(result_arrays(res), host(res.draws), t, K, label="4100 classes")


def test_keep_probs_false_returns_the_same_bits_elsewhere(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S, K = 37, 70, 20, 3, 5
    x, t = data(oracle, R, I0, Cn)
    a, b = FusedMLP(opt_for("lrt")), FusedMLP(opt_for("lrt"))
    ra = a.predict_classes(dev(x), S=S, targets=dev(t), topk=K)
    rb = b.predict_classes(dev(x), S=S, targets=dev(t), topk=K, keep_probs=False)
    assert rb.probs is None and rb.log_probs is None and ra.totals == rb.totals
    assert_same_results(ra, rb, "keep_probs", skip=("probs", "log_probs"))


def test_views_compact_held_mask_and_map_all_run(oracle):
    from vbnn_amd.engine import FusedMLP
    R, I0, Cn, S = 37, 70, 20, 3
    x, t = data(oracle, R, I0, Cn)
    xd, td = dev(x), dev(t)
    eng = FusedMLP(opt_for("lrt"))
    eng.prepare()
    plain = eng.predict_classes(xd, S=S, targets=td, topk=3)
    r = eng.prune(fraction=0.5)
    eng.draw = 0
    with eng.pruned(r):
        view = eng.predict_classes(xd, S=S, targets=td, topk=3)
    eng.draw = 0
    with eng.pruned(r.compress()):
        comp = eng.predict_classes(xd, S=S, targets=td, topk=3)
    assert eng.draw == S and not torch.equal(view.log_probs, plain.log_probs)
    for res in (view, comp):
        lp = res.log_probs.double()
        assert bool(torch.isfinite(lp).all()) and float((lp.exp().sum(1) - 1).abs().max()) <= 1e-5 and math.isfinite(res.nll)
    with pytest.raises(RuntimeError, match="older parameters"):                   # a stale view
        eng.prepare()
        with eng.pruned(r):
            eng.predict_classes(xd, S=S)
    assert eng.draw == S
    c = eng.compact(eng.prune_units(fraction=0.5, multiple=2))
    small = c.predict_classes(xd, S=S, targets=td, topk=3)
    assert tuple(small.log_probs.shape) == (R, Cn) and math.isfinite(small.nll) and 0 <= small.topk_accuracy <= 100
    held_eng = FusedMLP(opt_for("lrt"))
    held_eng.prepare()
    pr = held_eng.prune(fraction=0.5)
    with held_eng.pruned(pr):
        want = held_eng.predict_classes(xd, targets=td, map=True)
    held_eng.hold_pruned(pr)
    held = held_eng.predict_classes(xd, targets=td, map=True)
    assert held_eng.draw == 0 and held.S == 1 and torch.equal(held.log_probs, want.log_probs) and held.nll == want.nll
    assert bool((held.mutual_info == 0).all()) and torch.equal(held.entropy, held.expected_entropy)
    assert held.mean_draw_nll == held.nll


def test_refusals_leave_the_counter_alone(oracle):
    from vbnn_amd.engine import FusedMLP
    x, t = data(oracle, 8, 70, 20)
    for crit, n in (("mse", 12), ("gauss", 12)):
        reg = FusedMLP(opt_for("lrt", criterion=crit, n_classes=n))
        with pytest.raises(ValueError, match="predict_regression"):
            reg.predict_classes(dev(x), S=2)
        assert reg.draw == 0
    eng = FusedMLP(opt_for("lrt"))
    with pytest.raises(ValueError, match="topk"):
        eng.predict_classes(dev(x), S=2, topk=9)
    with pytest.raises(ValueError, match="topk"):
        eng.predict_classes(dev(x), S=2, topk=-1)
    with pytest.raises(ValueError, match="topk"):
        FusedMLP(opt_for("lrt", n_classes=4)).predict_classes(dev(x), S=2, topk=5)
    with pytest.raises(ValueError, match="at least one"):
        eng.predict_classes(dev(x), S=0)
    with pytest.raises(ValueError, match="16 classes"):
        eng.predict(dev(x), S=2)                                                   # predict keeps its limit
    assert eng.draw == 0


def test_training_is_undisturbed(oracle):
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", "bf16", input_size=256, hidden=[512, 256], n_classes=20, testSamples=4)
    x, t = data(oracle, 128, 256, 20)
    x, t = dev(x), dev(t)
    runs = []
    for use_predict in (True, False):
        eng = FusedMLP(opt)
        eng.prepare(); eng.resetGradients(); eng.sample(); eng.run(x, t)
        N0, args0 = eng._N, dict(eng._argcache)
        if use_predict:
            eng.predict_classes(x, targets=t, topk=5)
        else:
            eng.sample(4)
        assert eng._N == N0 and eng._argcache.keys() == args0.keys()
        eng.resetGradients(); eng.sample(); eng.run(x, t)
        loss, corr = eng.loss_and_accuracy()
        runs.append((eng.grads.clone(), loss, corr, eng.draw))
    (ga, la, ca, da), (gb, lb, cb, db) = runs
    assert torch.equal(ga, gb) and la == lb and ca == cb and da == db


def test_trainer_logs_the_predictive_series_at_twenty_classes(tmp_path):
    from vbnn_amd import data as D, train
    trainSet, testSet = D.synthetic_digits(400, 200, classes=20, seed=3, noise=2.0)
    opt = train.default_opt(network_name=str(tmp_path / "exp20"), hidden=[64, 48], n_classes=20, batchSize=100, testBatchSize=100,
                            trainSize=400, testSize=200, S=2, testSamples=3, mode="lrt", dtype="f32", predictive=True,
                            state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
    m = train.Main(opt)
    hist = m.run(trainSet, testSet, epochs=1)
    rec = hist[-1]
    for k in ("devacc_pred", "devnll_pred", "dev_mi"):
        assert k in rec and math.isfinite(rec[k]), (k, rec)
    assert 0.0 <= rec["devacc_pred"] <= 100.0 and rec["devnll_pred"] > 0.0
