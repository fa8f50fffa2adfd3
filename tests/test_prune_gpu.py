"""GPU tests of signal-to-noise pruning (mainviz.lua:20-27 on the device): vbnn_snr / vbnn_prune_select / vbnn_prune_pack
(include/vbnn_hip.h), FusedMLP.prune / use_pruned / prune_curve and the C host's --prune, against a float64 restatement of the
key and of the order statistic, against NumPy's exact selection on the library's own keys, and -- for the pruned predictive --
bitwise against a second engine whose fp32 parameters were pruned by hand."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _prune_np as PN

pytestmark = pytest.mark.gpu

SEED = 3
STREAM_INIT = 3
NETS = {"mnist": (784, [400, 400]), "odd": (70, [50, 34])}
QS = (0.0, 0.1, 0.5, 0.9, 0.98)


def opt_for(net="mnist", mode="lrt", dtype="f32", **kw):
    I0, hidden = NETS[net]
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, input_size=I0, hidden=list(hidden),
             n_classes=10, type="vb", testSamples=2)
    o.update(kw)
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def make(oracle, net="mnist", mode="lrt", dtype="f32", **kw):
    """The issue's inputs: means as init_parameters leaves them, lvars = log(1e-2) + 0.75 N(0, 1) (stream INIT, draw 7), prepared."""
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for(net, mode, dtype, **kw))
    for li, v in enumerate(eng.vb):
        z = oracle.fill_normal(v.O, v.I, SEED, STREAM_INIT, li, 7)
        v.lvars.copy_(dev((np.float32(math.log(1e-2)) + np.float32(0.75) * z).astype(np.float32)))
    eng.prepare()
    return eng


def inputs(oracle, R, I0):
    x = oracle.fill_normal(R, I0, SEED, 4, 0, 0)
    t = (np.arange(R) * 7 % 10).astype(np.int32)
    return x, t


def snr64(eng, li):
    v = eng.vb[li]
    return np.abs(host(v.means).astype(np.float64)) * np.exp(-host(v.lvars).astype(np.float64) / 2)


def keys32(eng, li):
    return host(eng.snr(li))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def select_raw(eng, lis, k):
    """vbnn_prune_select on layers `lis`: (status, tau as a float32 scalar)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    lib = L.lib()
    d = (L.PruneDesc * len(lis))()
    for j, li in enumerate(lis):
        v = eng.vb[li]
        d[j] = L.PruneDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I)
    nb = C.c_size_t()
    L.check(lib.vbnn_prune_workspace_bytes(len(lis), d, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    tau = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    st = lib.vbnn_prune_select(eng.ctx.h, len(lis), d, int(k), _p(tau), _p(ws), nb.value)
    return st, host(tau)[0]


def scopes(eng):
    n = len(eng.vb)
    return [list(range(n))] + [[li] for li in range(n)]


# ---- 1. the key
@pytest.mark.parametrize("net", list(NETS))
def test_key_matches_float64(oracle, net):
    eng = make(oracle, net)
    for li in range(len(eng.vb)):
        got, want = keys32(eng, li).astype(np.float64), snr64(eng, li)
        rel = np.abs(got - want) / want
        print(f"{net} layer {li}: key max rel err {np.nanmax(rel):.3e}, range {want.min():.3e} .. {want.max():.3e}")
        bound = PN.key_bound(host(eng.vb[li].means), host(eng.vb[li].lvars))      # derived in tests/_prune_np.py: 2.25 ulp
        print(f"{net} layer {li}: fraction of the bound used {np.max(np.abs(got - want) / bound):.3f}")
        assert np.all(np.abs(got - want) <= bound)


# ---- 2. selection is exact on its own keys
@pytest.mark.parametrize("net", list(NETS))
def test_selection_is_exact_on_its_own_keys(oracle, net):
    eng = make(oracle, net)
    for lis in scopes(eng):
        keys = np.concatenate([keys32(eng, li).ravel() for li in lis])
        W = keys.size
        for k in [int(math.floor(q * W)) for q in QS] + [W - 1]:
            st, tau = select_raw(eng, lis, k)
            want = np.partition(keys, k)[k]
            assert st == 0 and same_bits(np.float32(tau), np.float32(want)), (net, lis, k, tau, want)
        st, _ = select_raw(eng, lis, W)
        assert st != 0                                             # k = W: an error status, not a clamp


def _prune_counts(eng, q):
    r = eng.prune(fraction=q)
    keys = np.concatenate([keys32(eng, li).ravel() for li in range(len(eng.vb))])
    k = int(math.floor(q * keys.size))
    return r, keys, k


@pytest.mark.parametrize("case", ["equal", "ties", "zeros", "nan"])
def test_selection_on_adversarial_keys(oracle, case):
    eng = make(oracle, "odd")
    W = sum(v.O * v.I for v in eng.vb)
    if case == "equal":
        for v in eng.vb:
            v.means.fill_(0.25); v.lvars.fill_(math.log(1e-2))
    elif case == "ties":                                           # means quantised to 16 levels, constant lvars: heavy ties
        for v in eng.vb:
            v.means.copy_(torch.round(v.means * 8).clamp_(-8, 7) / 8); v.lvars.fill_(math.log(1e-2))
    elif case == "zeros":
        eng.vb[0].means[:20].zero_()
    else:
        eng.vb[1].means[3, 5] = float("nan")
    eng.prepare()
    ks = sorted({0, 1, W // 10, W // 2, int(0.9 * W), W - 2, W - 1})
    lis = list(range(len(eng.vb)))
    keys = np.concatenate([keys32(eng, li).ravel() for li in lis])
    bits = keys.view(np.uint32)                                    # non-negative floats and the NaNs above them order as their bits
    for k in ks:
        st, tau = select_raw(eng, lis, k)
        want = np.partition(bits, k)[k]
        assert st == 0 and np.float32(tau).view(np.uint32) == want, (case, k, tau, want)
    if case == "nan":
        clean = np.sort(keys[~np.isnan(keys)])
        for k in (0, W // 2, W - 2):                               # tau unaffected for k < W - 1
            assert same_bits(np.float32(select_raw(eng, lis, k)[1]), clean[k])
    for q in (0.1, 0.5, 0.9, 1.0):
        r, keys, k = _prune_counts(eng, q)
        tau = np.float32(r.tau[0])
        n = int((keys < tau).sum())
        assert r.n_pruned == n and n <= k, (case, q, r.n_pruned, n, k)
        if case == "nan":
            assert not host(r.mask(1))[3, 5]                       # a NaN key is never pruned, not even at tau = +inf
        if case == "equal" and q < 1.0:
            assert r.n_pruned == 0


# ---- 3. the mask against float64
def _boundary(s64, tau64):
    return np.abs(s64 - tau64) <= 3e-5 * tau64


@pytest.mark.parametrize("net", list(NETS))
def test_mask_matches_float64(oracle, net):
    eng = make(oracle, net)
    n = len(eng.vb)
    s64 = [snr64(eng, li) for li in range(n)]
    flat = np.concatenate([s.ravel() for s in s64])
    for scope in ("global", "layer"):
        for q in QS:
            r = eng.prune(fraction=q, scope=scope)
            for li in range(n):
                pool = flat if scope == "global" else s64[li].ravel()
                tau64 = np.partition(pool, int(math.floor(q * pool.size)))[int(math.floor(q * pool.size))]
                edge = _boundary(s64[li], tau64)
                nb = int(_boundary(pool, tau64).sum())
                print(f"{net} {scope} q {q} layer {li}: tau {r.tau[li]:.9g} (float64 {tau64:.9g}), boundary set {nb}")
                assert nb <= 32                                   # the test's own condition
                m = host(r.mask(li))
                assert np.array_equal(m[~edge], (s64[li] < tau64)[~edge]), (net, scope, q, li)
    r = eng.prune(threshold=0.005)
    nb = int(_boundary(flat, 0.005).sum())
    print(f"{net} threshold 0.005: {r.n_pruned} pruned, float64 {(flat < 0.005).sum()}, boundary set {nb}")
    assert nb <= 32 and abs(r.n_pruned - {"mnist": 3695, "odd": 9}[net]) <= nb
    for li in range(n):
        edge = _boundary(s64[li], 0.005)
        assert np.array_equal(host(r.mask(li))[~edge], (s64[li] < 0.005)[~edge])


# ---- 4. shadows, statistics, reproducibility
@pytest.mark.parametrize("net,dtype", [("mnist", "f32"), ("mnist", "bf16"), ("odd", "f32"), ("odd", "bf16")])
def test_shadows_stats_and_reproducibility(oracle, net, dtype):
    eng = make(oracle, net, dtype=dtype)
    for q in (0.5, 0.98):
        r, r2 = eng.prune(fraction=q), eng.prune(fraction=q)
        assert same_bits(np.float32(r.tau), np.float32(r2.tau)) and r.stats == r2.stats
        npruned = 0
        for li, v in enumerate(eng.vb):
            m = host(r.mask(li))
            assert same_bits(m, host(r2.mask(li)))
            keys = keys32(eng, li)
            assert np.array_equal(m, keys < np.float32(r.tau[li]))
            for got, got2, ref in ((r.mu_p[li], r2.mu_p[li], v.mu_s), (r.var_p[li], r2.var_p[li], v.var_s)):
                g, g2, s = (host(t.t.view(torch.int16 if dtype == "bf16" else torch.int32)) for t in (got, got2, ref))
                assert np.array_equal(g, g2)
                assert np.array_equal(g[:, :v.I][~m], s[:, :v.I][~m])           # kept: bitwise the prepared shadows
                assert not g[:, :v.I][m].any() and not g[:, v.I:].any()          # pruned entries and pads: +0
            st = r.stats[li]
            var64 = np.exp(host(v.lvars).astype(np.float64))
            assert st[0] == m.sum() and st[3] == v.O * v.I
            rel = PN.pack_sum_rel(v.O, v.I)                                     # expf's allowance and the additions: _prune_np.py
            assert abs(st[1] - var64[m].sum()) <= rel * var64[m].sum() and abs(st[2] - var64.sum()) <= rel * var64.sum()
            assert r.layers[li]["n_pruned"] == int(m.sum())
            npruned += int(m.sum())
        assert r.n_pruned == npruned and r.W == sum(v.O * v.I for v in eng.vb)
        assert r.fraction_pruned == npruned / r.W


# ---- 5. pruned predict is predict on a pruned network
def _hand_pruned(oracle, eng, r, net, mode, dtype, **kw):
    """A second engine with eng's parameters, pruned BY HAND in fp32 (means = 0, lvars = -inf where the mask says so)."""
    other = make(oracle, net, mode, dtype, **kw)
    for li, (v, w) in enumerate(zip(eng.vb, other.vb)):
        m = r.mask(li)
        w.means.copy_(torch.where(m, torch.zeros_like(v.means), v.means))
        w.lvars.copy_(torch.where(m, torch.full_like(v.lvars, float("-inf")), v.lvars))
        w.bias.copy_(v.bias)
    other.prepare()
    other.draw = eng.draw
    return other


def _same_result(a, b):
    for name in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "pred"):
        assert same_bits(host(getattr(a, name)), host(getattr(b, name))), name
    assert np.array_equal(np.array(a.totals).view(np.uint64), np.array(b.totals).view(np.uint64)), (a.totals, b.totals)


@pytest.mark.parametrize("mode,dtype,kw,pk", [
    ("lrt", "f32", {}, dict(S=3)),
    ("lrt", "bf16", dict(predict_stacked=False), dict(S=3)),
    ("lrt", "bf16", dict(predict_stacked=True), dict(S=3)),
    ("lrt", "f32", {}, dict(map=True)),
    ("wn", "f32", {}, dict(map=True)),
    ("wn", "bf16", {}, dict(map=True)),
])
@pytest.mark.parametrize("q", [0.5, 0.98])
def test_pruned_predict_is_predict_on_a_pruned_network(oracle, mode, dtype, kw, pk, q):
    eng = make(oracle, "mnist", mode, dtype, **kw)
    x, t = inputs(oracle, 64, 784)
    r = eng.prune(fraction=q)
    other = _hand_pruned(oracle, eng, r, "mnist", mode, dtype, **kw)
    with eng.pruned(r):
        a = eng.predict(dev(x), targets=dev(t), **pk)
    b = other.predict(dev(x), targets=dev(t), **pk)
    assert a.stacked == b.stacked and eng.draw == other.draw
    _same_result(a, b)
    print(f"{mode} {dtype} {kw} {pk} q {q}: nll {a.nll:.6f} accuracy {a.accuracy:.2f}")


def test_pruned_predictive_matches_float64(oracle):
    from tests.test_predict_gpu import check_against_oracle
    eng = make(oracle, "mnist")
    x, t = inputs(oracle, 64, 784)
    r = eng.prune(fraction=0.9)
    other = _hand_pruned(oracle, eng, r, "mnist", "lrt", "f32")     # (its fp32 parameters ARE the masked ones: exp(-inf) = 0)
    d0 = eng.draw + 1
    with eng.pruned(r):
        res = eng.predict(dev(x), S=4, targets=dev(t))
    check_against_oracle(oracle, other, res, x, t, 4, d0)


# ---- 6. the ends of the range
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nothing_pruned_is_the_unpruned_predict(oracle, dtype):
    eng, other = make(oracle, "mnist", dtype=dtype), make(oracle, "mnist", dtype=dtype)
    x, t = inputs(oracle, 64, 784)
    for kw in (dict(fraction=0.0), dict(threshold=0.0)):
        r = eng.prune(**kw)
        assert r.n_pruned == 0 and r.fraction_pruned == 0.0
        with eng.pruned(r):
            a = eng.predict(dev(x), S=3, targets=dev(t))
        _same_result(a, other.predict(dev(x), S=3, targets=dev(t)))


def test_everything_pruned_leaves_the_biases(oracle):
    eng = make(oracle, "mnist")
    for li, v in enumerate(eng.vb):                               # VB biases: a non-zero fill with both signs
        v.bias.copy_(dev(oracle.fill_normal(1, v.O, SEED, STREAM_INIT, li, 9)[0]))
    eng.bias3.copy_(dev(oracle.fill_normal(1, 10, SEED, STREAM_INIT, 5, 9)[0]))
    r = eng.prune(fraction=1.0)
    assert r.n_pruned == r.W and all(math.isinf(tau) for tau in r.tau)
    b_last = host(eng.vb[-1].bias).astype(np.float64)
    lg = host(eng.weight3).astype(np.float64) @ np.maximum(b_last, 0.0) + host(eng.bias3).astype(np.float64)
    p = np.exp(lg - lg.max()); p /= p.sum()
    H = -(p * np.log(p)).sum()
    x, t = inputs(oracle, 37, 784)
    for S in (1, 3, 8):
        with eng.pruned(r):
            res = eng.predict(dev(x), S=S, targets=dev(t))
        assert np.abs(host(res.probs) - p[None, :]).max() <= 1e-5
        assert np.abs(host(res.entropy) - H).max() <= 1e-5 and np.abs(host(res.expected_entropy) - H).max() <= 1e-5
        assert np.abs(host(res.mutual_info)).max() <= 1e-5


# ---- 7. guards, and the training step is undisturbed
def test_guards(oracle):
    eng = make(oracle, "odd", fuse_kl=True, state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-4),
               varState=dict(learningRate=5e-2))
    x, t = inputs(oracle, 37, 70)
    xd, td = dev(x), dev(t)
    with pytest.raises(ValueError):
        eng.prune()
    with pytest.raises(ValueError):
        eng.prune(fraction=0.5, threshold=0.005)
    with pytest.raises(ValueError):
        eng.prune(fraction=1.5)
    base = eng.predict(xd, S=2, targets=td)
    r = eng.prune(fraction=0.5)
    eng.use_pruned(r)
    pruned = eng.predict(xd, S=2, targets=td)
    assert not same_bits(host(pruned.probs), host(base.probs))
    eng.use_pruned(None)
    eng.draw -= 4
    _same_result(eng.predict(xd, S=2, targets=td), base)            # use_pruned(None): bitwise the unpruned predict
    eng.use_pruned(r)
    eng.resetGradients(); eng.sample(); eng.run(xd, td); eng.finish()
    eng.predict(xd, S=2, targets=td)                                # training steps do not invalidate a view ...
    eng.update(eng.opt)
    with pytest.raises(RuntimeError):                               # ... an update does
        eng.predict(xd, S=2, targets=td)
    with pytest.raises(RuntimeError):
        r.mask(0)
    eng.use_pruned(None)
    eng.predict(xd, S=2, targets=td)
    wn = make(oracle, "odd", "wn")
    rw = wn.prune(fraction=0.5)
    with wn.pruned(rw):
        with pytest.raises(ValueError, match="pruned view"):
            wn.predict(xd, S=3)
        wn.predict(xd, map=True)
    with pytest.raises(ValueError):
        wn.use_pruned(r)                                            # another engine's result


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_is_undisturbed(oracle, dtype):
    a, b = make(oracle, "mnist", dtype=dtype), make(oracle, "mnist", dtype=dtype)
    x, t = inputs(oracle, 64, 784)
    xd, td = dev(x), dev(t)
    r = a.prune(fraction=0.9)
    with a.pruned(r):
        a.predict(xd, S=2, targets=td)
    b.predict(xd, S=2, targets=td)                                  # (the same draws consumed)
    a.use_pruned(r)                                                 # run() does not look at the view
    for e in (a, b):
        e.resetGradients(); e.sample(); e.run(xd, td); e.finish()
    assert a.loss_and_accuracy() == b.loss_and_accuracy()
    assert same_bits(host(a.grads), host(b.grads)) and np.abs(host(a.grads)).max() > 0


# ---- 8. the C host
@pytest.mark.parametrize("dtype,I0,hidden,R,S", [("f32", 784, [400, 400], 100, 4), ("bf16", 256, [512, 256], 512, 4)])
def test_c_host_prune_is_bitwise_the_engines(tmp_path, dtype, I0, hidden, R, S):
    """tools/c_host.c --prune 0.9 --predict 4 after one training step against engine.prune + predict after the same step."""
    from tests import _children
    from tests.test_c_host import build
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    exe = build(tmp_path)
    out = str(tmp_path / "prune.bin")
    cmd = [exe, "--dtype", dtype, "--input", str(I0), "--hidden", ",".join(str(h) for h in hidden), "--classes", "10",
           "--batch", str(R), "--S", "1", "--steps", "1", "--predict", str(S), "--prune", "0.9", "--out", out]
    res = _children.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    print(res.stdout.strip())
    raw = open(out, "rb").read()
    off = 24 + 4 * int(np.frombuffer(raw[:8], np.int64)[0])

    def take(dt, count):
        nonlocal off
        a = np.frombuffer(raw[off:off + np.dtype(dt).itemsize * count], dt)
        off += np.dtype(dt).itemsize * count
        return a

    def block():
        Rf, Cf = (int(v) for v in take(np.int64, 2))
        head = [int(v) for v in take(np.int32, 4)]
        fields = [take(np.float32, Rf * Cf), take(np.float32, Rf * Cf), take(np.float32, Rf), take(np.float32, Rf),
                  take(np.float32, Rf), take(np.int32, Rf), take(np.float64, 4)]
        return head, fields
    block()                                                        # the unpruned predictive (tests/test_predict_gpu.py)
    nl = int(take(np.int32, 1)[0])
    tau = take(np.float32, 1)[0]
    stats = take(np.float64, 4 * nl).reshape(nl, 4)
    head, fields = block()
    assert off == len(raw) and nl == len(hidden)

    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype=dtype, seed=3, input_size=I0, hidden=hidden, n_classes=10,
               fuse_kl=True)
    eng = FusedMLP(opt)
    x = torch.empty(R, I0, dtype=torch.float32, device="cuda")
    fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(R, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    eng.prepare(); eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
    eng.predict(x, S=S, targets=t)
    r = eng.prune(fraction=0.9)
    with eng.pruned(r):
        p = eng.predict(x, S=S, targets=t)
    assert same_bits(np.float32(tau), np.float32(r.tau[0])) and np.array_equal(stats, np.array(r.stats)), (tau, r.tau, stats, r.stats)
    assert head == [S, int(p.stacked), p.chunks, eng.draw]
    for got, want in zip(fields[:5], (p.probs, p.log_probs, p.entropy, p.expected_entropy, p.mutual_info)):
        assert np.array_equal(got.view(np.uint32), host(want).reshape(-1).view(np.uint32))
    assert np.array_equal(fields[5], host(p.pred))
    assert np.array_equal(fields[6].view(np.uint64), np.array(p.totals, np.float64).view(np.uint64))


# ---- 9. end to end
def test_prune_curve_after_training(tmp_path):
    """tests/test_train_gpu.py's recipe (synthetic digits, 64-48 hidden, three epochs, LRT f32), then the pruning curve of the
    MAP prediction over the test set. Gated: the ends and monotonicity. The accuracies in between are printed, not gated --
    nobody has measured how prunable three epochs on synthetic digits leave this network."""
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    opt = train.default_opt(network_name=str(tmp_path / "exp_prune"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                            trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32",
                            state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2},
                            prune_report=0.005, prune_eval=[0.5, 0.9])
    m = train.Main(opt)
    hist = m.run(trainSet, testSet, epochs=3)
    assert hist[-1]["devacc"] > 90.0
    assert 0 <= hist[-1]["pruned count"] < 784 * 64 + 64 * 48 and "devacc_pruned@0.5" in hist[-1] and "devacc_pruned@0.9" in hist[-1]
    inputs_, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
    x, t = m._to_device(inputs_, targets)
    net = m.net
    base = net.predict(x, targets=t, map=True)
    rows = net.prune_curve(x, t, [0, 0.5, 0.9, 0.98, 1.0], map=True)
    for row in rows:
        print("prune_curve", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in row.items()})
    assert rows[0]["n_pruned"] == 0 and rows[0]["accuracy"] == base.accuracy
    assert rows[-1]["accuracy"] < 40.0 and rows[-1]["n_pruned"] == 784 * 64 + 64 * 48
    assert all(a["n_pruned"] <= b["n_pruned"] and a["tau"][0] <= b["tau"][0] for a, b in zip(rows, rows[1:]))
    assert net._pruned is None
