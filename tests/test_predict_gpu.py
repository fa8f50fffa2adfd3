"""GPU tests of the posterior-predictive path: FusedMLP.predict over vbnn_head_predict (include/vbnn_hip.h) -- the S-draw
model average p(y | x, D) ~ 1/S sum_s softmax(f_s(x)), its entropy and the mutual information, against a float64
restatement of the forward (the oracle's noise contract), against test()'s per-draw metrics, and its bitwise invariances."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 3
STREAM_EPS, STREAM_ZETA = 1, 2


def opt_for(mode, dtype="f32", **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=784, hidden=[400, 400],
             n_classes=10, type="vb", testSamples=2)
    o.update(kw)
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def inputs(oracle, R, I0):
    x = oracle.fill_normal(R, I0, SEED, 4, 0, 0)
    t = (np.arange(R) * 7 % 10).astype(np.int32)
    return x, t


def params(eng):
    ps = [(host(v.means).astype(np.float64), host(v.lvars).astype(np.float64), host(v.bias).astype(np.float64)) for v in eng.vb]
    return ps, host(eng.weight3).astype(np.float64), host(eng.bias3).astype(np.float64)


def oracle_draw(oracle, eng, x, draw, row0=0):
    """One draw's log-softmax rows in float64 (LRT: the oracle's z per layer; WN: OracleVBLinear.sample's weights), and the
    GEMM bound of the parity tests (|d| <= 4e-6 sum |a b| per fp32 GEMM) carried to the logits: per row, the largest error of a
    logit that fp32 accumulation can explain."""
    ps, w3, b3 = params(eng)
    h, err = x.astype(np.float64), np.zeros((x.shape[0], 1))
    for li, (mu, lv, b) in enumerate(ps):
        O = mu.shape[0]
        if eng.mode == "lrt":
            z = oracle.fill_normal(h.shape[0], O, SEED, STREAM_ZETA, li, draw, row0).astype(np.float64)
            var = np.exp(lv)
            m, v = h @ mu.T + b, (h * h) @ var.T
            y = m + np.sqrt(v) * z
            absprod = np.abs(h) @ np.abs(mu).T + np.sqrt(v) * np.abs(z)
            prop = (err * (np.abs(mu).sum(1)[None, :] + 2 * np.sqrt(var.max()) * np.abs(z) * np.sqrt(np.abs(h).sum(1, keepdims=True))))
            w = None
        else:
            e = oracle.fill_normal(O, mu.shape[1], SEED, STREAM_EPS, li, draw).astype(np.float64)
            w = mu + np.sqrt(np.exp(lv)) * e
            y = h @ w.T + b
            absprod = np.abs(h) @ np.abs(w).T
            prop = err * np.abs(w).sum(1)[None, :]
        err = 4e-6 * absprod + prop + 1e-6 * np.abs(y)
        h = np.maximum(y, 0.0)
        err = err.max(1, keepdims=True)
    lg = h @ w3.T + b3
    lerr = 4e-6 * (np.abs(h) @ np.abs(w3).T).max(1, keepdims=True) + err * np.abs(w3).sum(1).max()
    mx = lg.max(1, keepdims=True)
    o = lg - mx - np.log(np.exp(lg - mx).sum(1, keepdims=True))
    return o, lerr[:, 0]


def oracle_predictive(o_draws):
    o = np.stack(o_draws)                                        # S x R x C
    m = o.max(0)
    lp = m + np.log(np.exp(o - m).mean(0))
    p = np.exp(lp)
    ent = -(p * lp).sum(1)
    eH = (-(np.exp(o) * o).sum(2)).mean(0)
    return lp, p, ent, eH


def check_against_oracle(oracle, eng, res, x, t, S, d0):
    o_draws, errs = zip(*[oracle_draw(oracle, eng, x, d0 + s) for s in range(S)])
    lp, p, ent, eH = oracle_predictive(o_draws)
    # tolerance: 1e-5 absolute, or what the GEMM bound implies where it is looser -- a logit error e moves every log-softmax
    # value by at most 2e, a probability by at most 2e p <= 2e, an entropy by at most 2e (1 + log C)
    e = float(np.max(errs))
    tol_p = max(1e-5, 2 * e)
    tol_h = max(1e-5, 2 * e * (1 + math.log(eng.n_classes)))
    dp = np.abs(host(res.probs) - p)
    assert dp.max() <= tol_p, (dp.max(), tol_p)
    assert np.median(dp) <= 1e-5, np.median(dp)                 # (the bound is a worst case; the typical row is far inside it)
    # the entropies: the same worst case, and the typical row at the 1e-5 figure (the worst case is loose at 784-400-400:
    # the GEMM bound carried through two hidden layers by sum |w| allows ~0.1 on a logit; the medians hold the arithmetic)
    for got, want in ((res.entropy, ent), (res.expected_entropy, eH), (res.mutual_info, ent - eH)):
        d = np.abs(host(got) - want)
        assert d.max() <= 2 * tol_h and np.median(d) <= 2e-5, (d.max(), np.median(d), tol_h)
    srt = np.sort(lp, 1)
    clear = (srt[:, -1] - srt[:, -2]) > 2 * tol_p
    assert np.array_equal(host(res.pred)[clear], lp.argmax(1)[clear])
    R = x.shape[0]
    o = np.stack(o_draws)
    rows = np.arange(R)
    want = [-lp[rows, t].sum() / R, 100.0 * (lp.argmax(1) == t).sum() / R,
            -o[:, rows, t].sum() / (R * S), 100.0 * (o.argmax(2) == t[None, :]).sum() / (R * S)]
    got = [res.nll, res.accuracy, res.mean_draw_nll, res.mean_draw_accuracy]
    assert abs(got[0] - want[0]) <= 3e-5 * abs(want[0]) + tol_p and abs(got[2] - want[2]) <= 3e-5 * abs(want[2]) + tol_p
    # accuracies: rows whose top two are closer than the tolerance may go either way
    assert abs(got[1] - want[1]) <= 100.0 * (~clear).sum() / R + 1e-9
    assert abs(got[3] - want[3]) <= 100.0 / R + 100.0 * (~clear).sum() / R + 1e-9


@pytest.mark.parametrize("hidden,I0,R,S", [([50, 34], 70, 37, 3), ([400, 400], 784, 100, 30)])
def test_lrt_f32_matches_float64_oracle(oracle, hidden, I0, R, S):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("lrt", input_size=I0, hidden=hidden))
    eng.prepare()
    x, t = inputs(oracle, R, I0)
    d0 = eng.draw + 1
    res = eng.predict(dev(x), S=S, targets=dev(t))
    assert eng.draw == d0 - 1 + S
    check_against_oracle(oracle, eng, res, x, t, S, d0)


def test_wn_f32_matches_float64_oracle(oracle):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("wn", input_size=70, hidden=[50, 34]))
    eng.prepare()
    x, t = inputs(oracle, 37, 70)
    res = eng.predict(dev(x), S=3, targets=dev(t))
    assert eng.draw == 3 and not res.stacked
    check_against_oracle(oracle, eng, res, x, t, 3, 1)


@pytest.mark.parametrize("mode,dtype", [("lrt", "f32"), ("wn", "f32"), ("lrt", "bf16")])
def test_map_has_no_epistemic_part(oracle, mode, dtype):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for(mode, dtype, input_size=70, hidden=[64, 34]))
    eng.prepare()
    x, t = inputs(oracle, 45, 70)
    res = eng.predict(dev(x), targets=dev(t), map=True)
    assert res.S == 1 and eng.draw == 0
    assert torch.equal(res.expected_entropy, res.entropy)
    assert bool((res.mutual_info == 0).all())
    # S = 1: the average IS the one draw's log-softmax; against the training path's MAP pass
    eng.clamp_to_map()
    eng.resetGradients()
    eng.run(dev(x), dev(t), backward=False)
    tol = 1e-5 if dtype == "f32" else 3e-2
    assert float((res.log_probs - eng.out[:45]).abs().max()) <= tol
    assert res.mean_draw_nll == res.nll and abs(res.accuracy - res.mean_draw_accuracy) <= 100.0 / 45


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_mean_draw_metrics_reproduce_test(oracle, mode):
    """The last two totals are mlp:test's numbers: the same draws, the same per-draw criterion and accuracy."""
    from vbnn_amd.engine import FusedMLP
    S, R = 5, 100
    opt = opt_for(mode, testSamples=S)
    a, b = FusedMLP(opt), FusedMLP(opt)
    x, t = inputs(oracle, R, 784)
    a.prepare(); b.prepare()
    err, acc = a.test(dev(x), dev(t))
    res = b.predict(dev(x), targets=dev(t))
    assert a.draw == b.draw == S
    assert abs(res.mean_draw_nll - err) <= 3e-5 * abs(err)
    assert abs(res.mean_draw_accuracy - acc) <= 100.0 / R + 1e-9


@pytest.mark.parametrize("dtype,hidden,I0,N,S", [("f32", [50, 34], 70, 1, 30), ("f32", [400, 400], 784, 100, 5),
                                                 ("bf16", [512, 256], 256, 128, 4)])
def test_stacked_equals_sequential(oracle, dtype, hidden, I0, N, S):
    from vbnn_amd.engine import FusedMLP
    x, t = inputs(oracle, N, I0)
    out = []
    for stacked in (True, False):
        eng = FusedMLP(opt_for("lrt", dtype, input_size=I0, hidden=hidden, predict_stacked=stacked))
        eng.prepare()
        res = eng.predict(dev(x), S=S, targets=dev(t))
        assert res.stacked == stacked
        out.append(res)
    a, b = out
    for k in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "pred"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert (a.nll, a.accuracy, a.mean_draw_nll, a.mean_draw_accuracy) == (b.nll, b.accuracy, b.mean_draw_nll, b.mean_draw_accuracy)


def test_chunking_seeds_and_second_call(oracle):
    from vbnn_amd.engine import FusedMLP
    x, t = inputs(oracle, 100, 784)
    S = 6
    base = FusedMLP(opt_for("lrt"))
    small = FusedMLP(opt_for("lrt", predict_rows=S * 16))
    twin = FusedMLP(opt_for("lrt"))
    for e in (base, small, twin):
        e.prepare()
    r0 = base.predict(dev(x), S=S, targets=dev(t))
    r1 = small.predict(dev(x), S=S, targets=dev(t))
    r2 = twin.predict(dev(x), S=S, targets=dev(t))
    assert r1.chunks == 7 and r0.chunks == 1
    for k in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "pred"):
        assert torch.equal(getattr(r0, k), getattr(r1, k)), k
        assert torch.equal(getattr(r0, k), getattr(r2, k)), k
    assert r0.accuracy == r1.accuracy and r0.mean_draw_accuracy == r1.mean_draw_accuracy
    assert abs(r0.nll - r1.nll) <= 1e-12 * abs(r0.nll) and abs(r0.mean_draw_nll - r1.mean_draw_nll) <= 1e-12 * abs(r0.mean_draw_nll)
    assert (r0.nll, r0.mean_draw_nll) == (r2.nll, r2.mean_draw_nll)
    fresh = FusedMLP(opt_for("lrt"))                           # never prepared: predict prepares the shadows, as test() does
    r4 = fresh.predict(dev(x), S=S, targets=dev(t))
    assert torch.equal(r4.probs, r0.probs) and r4.nll == r0.nll
    r3 = base.predict(dev(x), S=S, targets=dev(t))
    assert base.draw == 2 * S
    assert not torch.equal(r3.probs, r0.probs)


@pytest.mark.parametrize("stacked", [True, False])
def test_wide_bf16_properties(oracle, nnmod_bf16, stacked):
    from vbnn_amd.engine import FusedMLP
    S, R = 8, 4096
    opt = opt_for("lrt", "bf16", hidden=[4096, 4096], predict_stacked=stacked)
    eng, ref = FusedMLP(opt), FusedMLP(opt)
    x = torch.empty(R, 784, dtype=torch.float32, device="cuda")
    nnmod_bf16.fill_normal(x, SEED, 4, 0, 0)
    t = eng.synthetic_targets(x)
    eng.prepare(); ref.prepare()
    res = eng.predict(x, S=S, targets=t)
    assert res.stacked == stacked
    lp, p = res.log_probs.double(), res.probs.double()
    assert bool(torch.isfinite(lp).all() and torch.isfinite(p).all() and torch.isfinite(res.mutual_info).all())
    assert float((p.sum(1) - 1).abs().max()) <= 1e-5
    assert float(res.mutual_info.min()) >= -1e-6
    assert float(res.entropy.max()) <= math.log(10) + 1e-6
    # the same draws through the training path's forward (run(backward=False)), averaged in float64
    o = []
    for _ in range(S):
        ref.sample()
        ref.resetGradients()
        ref.run(x, t, backward=False)
        o.append(ref.out[:R].double().clone())
    o = torch.stack(o)
    m = o.max(0).values
    want = m + torch.log(torch.exp(o - m).mean(0))
    rows = torch.arange(R, device="cuda")
    tl = t.long()
    # Jensen: -log p[t] <= mean_s -log p_s[t]
    assert bool((-lp[rows, tl] <= -o[:, rows, tl].mean(0) + 1e-5).all())
    # tolerance: the two paths run different bf16 GEMM kernels (stacked rows never take the two-pass 256 x 256 kernel; the training
    # forward stores r and carries the head's logits in its tiles), so an activation may differ by one bf16 rounding (2^-8
    # relative) in each of the two hidden layers: a logit by at most 2 x 2^-8 x sum_i |w3_ci h_i| (+ the next layer's share of
    # the first layer's rounding, bounded the same way), a log-probability by twice that.
    h = ref.h_s.t[:R, :4096].double().abs()
    w3 = ref.weight3.double().abs()
    tol = 2 * 2 * (2 ** -8) * float((h @ w3.T).max())
    dev_ = (lp - want).abs().max(1).values
    assert float(dev_.max()) <= tol, (float(dev_.max()), tol)
    # ... a worst case (every rounding the same way). Row by row, the roundings of h are independent and each within 2^-8 of the
    # value: a logit's difference is a sum of independent terms of standard deviation at most 2^-8 |w3_ci h_i| / sqrt(3), so six
    # of its standard deviations (x 2 for the log-softmax) bound the typical row -- a wrong draw or noise row misses it by far
    sd = (2 ** -8) * torch.sqrt(((h * h) @ (w3 * w3).T).max(1).values / 3)
    assert float((dev_ <= 2 * 6 * sd).double().mean()) >= 0.99, float((dev_ / sd).median())


@pytest.fixture(scope="module")
def nnmod_bf16():
    from vbnn_amd import nn
    return nn


def test_training_is_undisturbed(oracle):
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", "bf16", input_size=256, hidden=[512, 256], testSamples=4)
    x, t = inputs(oracle, 128, 256)
    x, t = dev(x), dev(t)
    runs = []
    for use_predict in (True, False):
        eng = FusedMLP(opt)
        eng.prepare(); eng.resetGradients(); eng.sample(); eng.run(x, t)
        N0, args0 = eng._N, dict(eng._argcache)
        if use_predict:
            eng.predict(x, targets=t)
        else:
            eng.sample(4)
        assert eng._N == N0 and eng._argcache.keys() == args0.keys()
        eng.resetGradients(); eng.sample(); eng.run(x, t)
        loss, corr = eng.loss_and_accuracy()
        runs.append((eng.grads.clone(), loss, corr, eng.draw))
    (ga, la, ca, da), (gb, lb, cb, db) = runs
    assert torch.equal(ga, gb) and la == lb and ca == cb and da == db


@pytest.mark.parametrize("stacked", [True, False])
def test_a_nan_activation_row_is_nan_in_the_result_and_counted_by_calibration(oracle, stacked):
    """The head's NaN contract (include/vbnn_hip.h) seen from the engine: one NaN in the head's input, in row 5 of the middle
    draw of three. The NaN is written into the head's operand after the draw's forward -- an input NaN never gets there: the
    ReLU between the layers is fmaxf(y, 0), Threshold's x > 0 ? x : 0, which gives 0 for a NaN. That row's probs are NaN, every
    other row is bitwise the clean call's, and calibration() skips and counts exactly that row."""
    from vbnn_amd.engine import FusedMLP
    R, S, row = 37, 3, 5
    x, t = inputs(oracle, R, 70)
    x, t = dev(x), dev(t)
    clean_eng, eng = (FusedMLP(opt_for("lrt", input_size=70, hidden=[50, 34], predict_stacked=stacked)) for _ in range(2))
    clean_eng.prepare(); eng.prepare()
    clean = clean_eng.predict(x, S=S, targets=t)
    forward = eng._draw_forward

    def poisoned(p, xc, rows, c0, s=None):
        forward(p, xc, rows, c0, s)
        h = p.bufs[len(eng.vb)].x.t                              # the head's operand: draw s of row r at s rows + r when stacked
        if s is None:
            h[1 * rows + row, 3] = float("nan")
        elif s == 1:
            h[row, 3] = float("nan")
    eng._draw_forward = poisoned
    res = eng.predict(x, S=S, targets=t)
    assert res.stacked == stacked == clean.stacked
    others = torch.arange(R, device="cuda") != row
    for k in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info"):
        got, want = getattr(res, k), getattr(clean, k)
        assert bool(torch.isnan(got[row]).all()), (k, got[row])
        assert torch.equal(got[others], want[others]), k
    assert 0 <= int(res.pred[row]) < 10 and torch.equal(res.pred[others], clean.pred[others])
    assert math.isnan(res.nll) and math.isnan(res.mean_draw_nll)
    hit = int(clean.pred[row]) == int(t[row])
    assert abs(res.accuracy - (clean.accuracy - 100.0 * hit / R)) <= 1e-9
    cal, cal_clean = eng.calibration(res, t), clean_eng.calibration(clean, t)
    assert (cal.n_nan, cal.n) == (1, R - 1) and (cal_clean.n_nan, cal_clean.n) == (0, R)


def test_errors():
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP
    import ctypes as C
    x = torch.zeros(4, 70, device="cuda")
    with pytest.raises(ValueError):
        FusedMLP(opt_for("lrt", input_size=70, hidden=[32], n_classes=20)).predict(x, S=2)
    with pytest.raises(ValueError):
        FusedMLP(opt_for("lrt", input_size=70, hidden=[32], criterion="mse")).predict(x, S=2)
    eng = FusedMLP(opt_for("lrt", input_size=70, hidden=[32]))
    with pytest.raises(ValueError):
        eng.predict(x, S=0)
    lib = L.lib()
    with pytest.raises(L.VbnnError):
        L.check(lib.vbnn_head_predict(eng.ctx.h, L.F32, None))
    a = L.PredictArgs(h=None, ld_h=64, w3=eng.w3_s.ptr, ld_w=eng.w3_s.ld, R=4, H=32, C=10, S=1)
    with pytest.raises(L.VbnnError):
        L.check(lib.vbnn_head_predict(eng.ctx.h, L.F32, C.byref(a)))
    a = L.PredictArgs(h=eng.w3_s.ptr, ld_h=eng.w3_s.ld, w3=eng.w3_s.ptr, ld_w=eng.w3_s.ld, R=4, H=32, C=10, S=3,
                      form=L.PREDICT_ACCUMULATE, first=1, final=0, state=None)
    with pytest.raises(L.VbnnError):                           # the accumulating form needs its state
        L.check(lib.vbnn_head_predict(eng.ctx.h, L.F32, C.byref(a)))
    assert eng.draw == 0


@pytest.mark.parametrize("dtype,I0,hidden,R,S", [("f32", 784, [400, 400], 100, 30), ("bf16", 256, [512, 256], 512, 4)])
def test_c_host_predict_is_bitwise_the_engines(tmp_path, dtype, I0, hidden, R, S):
    """tools/c_host.c --predict (the Lua host's executable stand-in, issuing lua/FusedMLP.lua:predict's calls in its order) after
    one training step, against engine.predict after the same step: every output and total bit for bit, the same draw counter."""
    from tests import _children
    from tests.test_c_host import build
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    exe = build(tmp_path)
    out = str(tmp_path / "predict.bin")
    cmd = [exe, "--dtype", dtype, "--input", str(I0), "--hidden", ",".join(str(h) for h in hidden), "--classes", "10",
           "--batch", str(R), "--S", "1", "--steps", "1", "--predict", str(S), "--out", out]
    res = _children.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    off = 24 + 4 * n

    def take(dt, count):
        nonlocal off
        a = np.frombuffer(raw[off:off + np.dtype(dt).itemsize * count], dt)
        off += np.dtype(dt).itemsize * count
        return a
    Rf, Cf = (int(v) for v in take(np.int64, 2))
    S_, stacked, chunks, draw = (int(v) for v in take(np.int32, 4))
    probs, log_probs = take(np.float32, Rf * Cf), take(np.float32, Rf * Cf)
    ent, eH, mi = take(np.float32, Rf), take(np.float32, Rf), take(np.float32, Rf)
    pred, totals = take(np.int32, Rf), take(np.float64, 4)
    assert off == len(raw) and (Rf, Cf, S_) == (R, 10, S)

    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype=dtype, seed=3, input_size=I0, hidden=hidden, n_classes=10,
               fuse_kl=True)
    eng = FusedMLP(opt)
    x = torch.empty(R, I0, dtype=torch.float32, device="cuda")
    fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(R, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    eng.prepare(); eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
    r = eng.predict(x, S=S, targets=t)
    assert (stacked, chunks, draw) == (int(r.stacked), r.chunks, eng.draw)
    for got, want in ((probs, r.probs), (log_probs, r.log_probs), (ent, r.entropy), (eH, r.expected_entropy), (mi, r.mutual_info)):
        assert np.array_equal(got.view(np.uint32), host(want).reshape(-1).view(np.uint32))
    assert np.array_equal(pred, host(r.pred))
    assert np.array_equal(totals.view(np.uint64), np.array(r.totals, np.float64).view(np.uint64)), (totals, r.totals)
