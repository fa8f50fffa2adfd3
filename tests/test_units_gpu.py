"""GPU tests of structured (unit-level) signal-to-noise pruning: vbnn_unit_snr / vbnn_unit_select / vbnn_unit_index /
vbnn_unit_gather (include/vbnn_hip.h), FusedMLP.unit_snr / prune_units / compact / prune_units_curve and the C host's
--prune-units, against the float64 / NumPy restatement of tests/_units_np.py, against NumPy's exact selection on the library's
own keys, and -- for the compact engine -- bitwise against torch indexing, against the source engine and against an engine
built directly at the compact widths."""
import math

import numpy as np
import pytest
import torch

from tests import _prune_np as PN
from tests import _units_np as U
from tests.test_prune_gpu import NETS, QS, SEED, STREAM_INIT, dev, host, inputs, make, same_bits

pytestmark = pytest.mark.gpu

LRS = dict(fuse_kl=True, state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-4), varState=dict(learningRate=5e-2))


def unit_keys(eng):
    return [host(eng.unit_snr(li)) for li in range(len(eng.vb))]


def key64(eng, li):
    v = eng.vb[li]
    return U.unit_key64(host(v.means), host(v.lvars))


def select_raw(eng, lis, k):
    """vbnn_unit_snr + vbnn_unit_select on layers `lis`: (status, tau as a float32 scalar)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    lib = L.lib()
    keys = [torch.empty(eng.vb[li].O, dtype=torch.float32, device="cuda") for li in lis]
    d = (L.UnitDesc * len(lis))()
    for j, li in enumerate(lis):
        v = eng.vb[li]
        d[j] = L.UnitDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, key=_p(keys[j]), keep=None, n_keep=None)
    L.check(lib.vbnn_unit_snr(eng.ctx.h, len(lis), d))
    tau = torch.full((len(lis) + 1,), -1.0, dtype=torch.float32, device="cuda")
    st = lib.vbnn_unit_select(eng.ctx.h, len(lis), d, int(k), _p(tau))
    tau = host(tau)
    assert tau[-1] == -1.0 and (st != 0 or all(same_bits(tau[j], tau[0]) for j in range(len(lis))))     # one copy per listed layer
    return st, tau[0]


def scopes(eng):
    n = len(eng.vb)
    return [list(range(n))] + [[li] for li in range(n)]


def _same_result(a, b):
    for name in ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info", "pred"):
        assert same_bits(host(getattr(a, name)), host(getattr(b, name))), name
    assert np.array_equal(np.array(a.totals).view(np.uint64), np.array(b.totals).view(np.uint64)), (a.totals, b.totals)


# ---- 1. the key
@pytest.mark.parametrize("net", list(NETS))
def test_unit_key_matches_float64(oracle, net):
    from vbnn_amd import nn
    eng = make(oracle, net)
    for li, v in enumerate(eng.vb):
        got32 = host(eng.unit_snr(li))
        got, want = got32.astype(np.float64), key64(eng, li)
        rel = np.abs(got - want) / want
        print(f"{net} layer {li}: unit key max rel err {rel.max():.3e}, range {want.min():.3e} .. {want.max():.3e}")
        assert got32.shape == (v.O,) and np.all(np.abs(got - want) <= PN.unit_rel(v.I) * want)      # derived in _prune_np.py
        assert same_bits(got32, host(eng.unit_snr(li)))                                 # two runs: the same bits
        mod = nn.VBLinear(v.I, v.O, dict(eng.opt))
        mod.means.copy_(v.means); mod.lvars.copy_(v.lvars)
        assert same_bits(got32, host(mod.unit_snr()))
    # one input per unit: the weight key of mainviz.lua:20, |mu| / sigma
    mod = nn.VBLinear(1, 300, dict(eng.opt))
    mod.means.copy_(dev(oracle.fill_normal(300, 1, SEED, STREAM_INIT, 0, 11)))
    mod.lvars.copy_(dev((np.float32(math.log(1e-2)) + np.float32(0.75) * oracle.fill_normal(300, 1, SEED, STREAM_INIT, 0, 12)).astype(np.float32)))
    w, u = host(mod.snr()).ravel().astype(np.float64), host(mod.unit_snr()).astype(np.float64)
    assert np.all(np.abs(u - w) <= 1e-6 * w)


def test_unit_key_of_few_long_rows(oracle):
    """The workgroup-per-row form (O < 1024, I > 1024): row lengths that take scalar loads, and one that takes 16-byte loads."""
    from vbnn_amd.engine import FusedMLP
    from tests.test_prune_gpu import opt_for
    for I0 in (1030, 2049, 2048):
        eng = FusedMLP(opt_for("odd", input_size=I0))
        v = eng.vb[0]
        v.lvars.copy_(dev((np.float32(math.log(1e-2)) + np.float32(0.75) * oracle.fill_normal(v.O, v.I, SEED, STREAM_INIT, 0, 7)).astype(np.float32)))
        got32 = host(eng.unit_snr(0))
        got, want = got32.astype(np.float64), key64(eng, 0)
        assert np.all(np.abs(got - want) <= PN.unit_rel(v.I) * want) and same_bits(got32, host(eng.unit_snr(0)))


# ---- 2. selection is exact on the library's own keys
@pytest.mark.parametrize("net", list(NETS))
def test_unit_selection_is_exact_on_its_own_keys(oracle, net):
    eng = make(oracle, net)
    keys = unit_keys(eng)
    for lis in scopes(eng):
        pool = np.concatenate([keys[li] for li in lis])
        n = pool.size
        for k in [int(math.floor(q * n)) for q in QS] + [n - 1]:
            st, tau = select_raw(eng, lis, k)
            want = np.partition(pool, k)[k]
            assert st == 0 and same_bits(np.float32(tau), np.float32(want)), (net, lis, k, tau, want)
            assert same_bits(np.float32(tau), np.float32(select_raw(eng, lis, k)[1]))
        assert select_raw(eng, lis, n)[0] != 0 and select_raw(eng, lis, -1)[0] != 0     # an error status, not a clamp


# ---- 3. the kept lists are the NumPy rule's
def _adversarial(eng, case):
    if case == "equal":                                                # sigma = 1, every weight 1/4: every key exactly 1/4
        for v in eng.vb:
            v.means.fill_(0.25); v.lvars.zero_()
    elif case == "two":                                                # two key values, interleaved: every cut falls inside a tie
        for v in eng.vb:
            o = torch.arange(v.O, device="cuda")
            v.means.copy_(torch.where((o * 7 % 3 == 0)[:, None], 0.5, 0.25).expand(v.O, v.I)); v.lvars.zero_()
    elif case == "zero":
        eng.vb[0].means[:20].zero_()
    else:
        eng.vb[1].means[3, 5] = float("nan")
    eng.prepare()


@pytest.mark.parametrize("case", ["equal", "two", "zero", "nan"])
@pytest.mark.parametrize("net", list(NETS))
def test_kept_lists_are_the_numpy_rule(oracle, net, case):
    eng = make(oracle, net)
    _adversarial(eng, case)
    keys = unit_keys(eng)
    if case in ("equal", "two"):
        assert all(set(k.tolist()) <= {0.25, 0.5} for k in keys)
    if case == "zero":
        assert not keys[0][:20].any() and keys[0][20:].all()
    if case == "nan":
        assert np.isnan(keys[1][3]) and np.isnan(keys[1]).sum() == 1
    for m in (1, 4, 256):
        for scope in ("global", "layer"):
            for q in QS + (1.0,):
                r = eng.prune_units(fraction=q, scope=scope, multiple=m)
                tau, keep = U.prune_units(keys, fraction=q, scope=scope, multiple=m)
                tag = (net, case, m, scope, q)
                assert same_bits(np.float32(r.tau), np.float32(tau)), (tag, r.tau, tau)
                for li, v in enumerate(eng.vb):
                    got = host(r.keep[li])
                    assert got.dtype == np.int32 and np.array_equal(got.astype(np.uint32), keep[li]), (tag, li)
                    assert r.hidden[li] == keep[li].size and r.layers[li] == dict(
                        n_units=v.O, n_pruned=v.O - keep[li].size, fraction_pruned=(v.O - keep[li].size) / v.O)
                    if m == 1 and scope == "global" and q < 1.0:
                        with np.errstate(invalid="ignore"):
                            want = np.flatnonzero(~(keys[li] < tau[li]))
                        if want.size:                                                   # m = 1, n0 >= 1: exactly {!(key < tau)}
                            assert np.array_equal(got, want)
                    if case == "equal":
                        assert np.array_equal(got, np.arange(v.O if q < 1.0 else min(m, v.O))), (tag, li)
                    if case == "nan" and li == 1:
                        assert 3 in got                                                 # a NaN key is never pruned
                sizes = [eng.sizes[0]] + [k.size for k in keep]
                assert r.n_weights == U.n_weights(sizes, 10) and r.n_weights_before == U.n_weights(eng.sizes, 10)
                assert r.n_pruned == sum(eng.sizes[1:]) - sum(sizes[1:]) and r.version == eng._pver
    r = eng.prune_units(threshold=float(np.median(np.concatenate(keys)[~np.isnan(np.concatenate(keys))])), multiple=4)
    tau, keep = U.prune_units(keys, threshold=r.tau[0], multiple=4)
    assert all(np.array_equal(host(r.keep[li]).astype(np.uint32), keep[li]) for li in range(len(keys)))
    r2 = eng.prune_units(threshold=r.tau[0], multiple=4)
    assert all(same_bits(host(a), host(b)) for a, b in zip(r.keep, r2.keep))            # two runs: the same words


# ---- 4. compaction is a bit copy
def _check_compact(eng, r, c):
    cols = None
    assert c.sizes == [eng.sizes[0]] + r.hidden and len(c.vb) == len(eng.vb)
    for v, w, rows in zip(eng.vb, c.vb, r.keep):
        rows = rows.long()
        for name in ("means", "lvars"):
            src = getattr(v, name)[rows]
            src = src if cols is None else src[:, cols]
            assert same_bits(host(getattr(w, name)), host(src)), name
        assert same_bits(host(w.bias), host(v.bias[rows]))
        cols = rows
    assert same_bits(host(c.weight3), host(eng.weight3[:, cols])) and same_bits(host(c.bias3), host(eng.bias3))


@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("net,dtype", [("mnist", "f32"), ("mnist", "bf16"), ("odd", "f32"), ("odd", "bf16")])
def test_compaction_is_a_bit_copy(oracle, net, dtype, m):
    eng = make(oracle, net, dtype=dtype)
    for li, v in enumerate(eng.vb):
        v.bias.copy_(dev(oracle.fill_normal(1, v.O, SEED, STREAM_INIT, li, 9)[0]))
    eng.bias3.copy_(dev(oracle.fill_normal(1, 10, SEED, STREAM_INIT, 5, 9)[0]))
    eng.prepare()
    for kw in (dict(fraction=0.5), dict(fraction=0.9, scope="layer"), dict(fraction=1.0)):
        r = eng.prune_units(multiple=m, **kw)
        c = eng.compact(r)
        assert c is not eng and c.dtype == eng.dtype and c.world == 1 and c.draw == eng.draw and c.seed == eng.seed
        _check_compact(eng, r, c)
        assert 0 < r.n_weights < r.n_weights_before == sum(v.O * v.I for v in eng.vb) + 10 * eng.sizes[-1]
        assert r.n_weights == sum(w.O * w.I for w in c.vb) + 10 * c.sizes[-1]


# ---- 5. nothing pruned: the compact engine is the engine
@pytest.mark.parametrize("dtype,kw", [("f32", {}), ("bf16", dict(predict_stacked=True)), ("bf16", dict(predict_stacked=False))])
def test_nothing_pruned_is_the_same_engine(oracle, dtype, kw):
    eng = make(oracle, "mnist", dtype=dtype, **kw)
    x, t = inputs(oracle, 64, 784)
    eng.predict(dev(x), S=2)                                          # (a draw counter that is not zero)
    r = eng.prune_units(fraction=0)
    assert r.n_pruned == 0 and r.hidden == [400, 400] and r.n_weights == r.n_weights_before
    c = eng.compact(r)
    a = c.predict(dev(x), S=3, targets=dev(t))
    b = eng.predict(dev(x), S=3, targets=dev(t))
    assert a.stacked == b.stacked and c.draw == eng.draw == 5
    _same_result(a, b)


# ---- 6. the compact network computes the function of the network with those units removed
def test_compact_network_is_the_function(oracle):
    from tests.test_predict_gpu import check_against_oracle, oracle_draw
    eng = make(oracle, "mnist")
    dead = [[0, 7, 13, 399], [1, 2, 200]]
    for li, v in enumerate(eng.vb):
        for o in dead[li]:
            v.means[o].zero_(); v.bias[o] = 0.0
            if li + 1 < len(eng.vb):
                eng.vb[li + 1].means[:, o].zero_()
            else:
                eng.weight3[:, o].zero_()
    eng.prepare()
    x, t = inputs(oracle, 100, 784)
    r = eng.prune_units(threshold=1e-30)
    for li, v in enumerate(eng.vb):
        assert host(r.keep[li]).tolist() == [o for o in range(v.O) if o not in dead[li]]
    c = eng.compact(r)
    assert c.sizes == [784, 396, 397]
    big = eng.predict(dev(x), targets=dev(t), map=True)
    small = c.predict(dev(x), targets=dev(t), map=True)
    _, errs = oracle_draw(oracle, eng, x, eng.draw + 1)
    e = float(np.max(errs))
    tol = 2 * max(1e-5, 2 * e)
    dp = np.abs(host(small.probs).astype(np.float64) - host(big.probs).astype(np.float64))
    srt = np.sort(host(big.probs).astype(np.float64), 1)
    clear = (srt[:, -1] - srt[:, -2]) > tol
    print(f"compact vs big MAP predict: max |dprobs| {dp.max():.3e}, GEMM bound e {e:.3e}, tolerance {tol:.3e}, {clear.sum()} clear rows")
    assert dp.max() <= tol
    assert np.median(dp) <= 1e-5                                      # (the typical row, as check_against_oracle holds it)
    assert np.array_equal(host(small.pred)[clear], host(big.pred)[clear])
    d0 = c.draw + 1                                                   # an ordinary engine: its own float64 restatement
    res = c.predict(dev(x), S=30, targets=dev(t))
    check_against_oracle(oracle, c, res, x, t, 30, d0)


# ---- 7. guards, and the source engine's training step is undisturbed
def test_unit_guards(oracle):
    eng = make(oracle, "odd", **LRS)
    x, t = inputs(oracle, 37, 70)
    xd, td = dev(x), dev(t)
    for kw in (dict(), dict(fraction=0.5, threshold=0.1), dict(fraction=0.5, scope="unit"), dict(fraction=0.5, multiple=0),
               dict(fraction=1.5), dict(fraction=0.5, multiple=1.5)):
        with pytest.raises(ValueError):
            eng.prune_units(**kw)
    r = eng.prune_units(fraction=0.5)
    other = make(oracle, "odd")
    with pytest.raises(ValueError):
        other.compact(r)                                              # another engine's result
    with pytest.raises(ValueError):
        eng.compact(eng.prune(fraction=0.5))                          # not a unit pruning
    eng.compact(r)
    eng.resetGradients(); eng.sample(); eng.run(xd, td); eng.finish()
    eng.compact(r)                                                    # a training step does not invalidate a result ...
    eng.update(eng.opt)
    with pytest.raises(RuntimeError):                                 # ... an update does
        eng.compact(r)
    c = eng.compact(eng.prune_units(fraction=0.5))
    c.predict(xd, S=2, targets=td)
    rc = c.prune(fraction=0.5)                                        # the compact engine is an ordinary engine
    with c.pruned(rc.compress()):
        c.predict(xd, S=2, targets=td)
    assert c.test(xd, td) is not None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_source_training_step_is_undisturbed(oracle, dtype):
    a, b = make(oracle, "mnist", dtype=dtype), make(oracle, "mnist", dtype=dtype)
    x, t = inputs(oracle, 64, 784)
    xd, td = dev(x), dev(t)
    for e in (a, b):
        e.resetGradients(); e.sample()
    c = a.compact(a.prune_units(fraction=0.75, multiple=4))           # between sample() and run()
    c.predict(xd, S=2, targets=td)
    for e in (a, b):
        e.run(xd, td); e.finish()
    assert a.draw == b.draw == 1
    assert a.loss_and_accuracy() == b.loss_and_accuracy()
    assert same_bits(host(a.grads), host(b.grads)) and np.abs(host(a.grads)).max() > 0


# ---- 8. the compact engine trains
@pytest.mark.parametrize("net,dtype", [("mnist", "f32"), ("mnist", "bf16"), ("odd", "f32")])
def test_compact_engine_trains(oracle, net, dtype):
    from vbnn_amd.engine import FusedMLP
    eng = make(oracle, net, dtype=dtype, **LRS)
    x, t = inputs(oracle, 64, NETS[net][0])
    xd, td = dev(x), dev(t)
    eng.predict(xd, S=2)
    r = eng.prune_units(fraction=0.5, multiple=4)
    c = eng.compact(r)
    direct = FusedMLP(dict(eng.opt, hidden=list(r.hidden)))
    for w, d in zip(c.vb, direct.vb):
        d.means.copy_(w.means); d.lvars.copy_(w.lvars); d.bias.copy_(w.bias)
    direct.weight3.copy_(c.weight3); direct.bias3.copy_(c.bias3)
    direct.prepare()
    direct.draw = c.draw
    for e in (c, direct):
        e.resetGradients(); e.sample(); e.run(xd, td); e.finish()
    assert c.loss_and_accuracy() == direct.loss_and_accuracy() and c.draw == direct.draw == 3
    assert same_bits(host(c.grads), host(direct.grads)) and np.abs(host(c.grads)).max() > 0
    for e in (c, direct):
        e.update(e.opt)
    for w, d in zip(c.vb, direct.vb):
        assert same_bits(host(w.means), host(d.means)) and same_bits(host(w.lvars), host(d.lvars)) and same_bits(host(w.bias), host(d.bias))
    assert same_bits(host(c.weight3), host(direct.weight3)) and same_bits(host(c.bias3), host(direct.bias3))
    assert not same_bits(host(c.vb[0].means), host(eng.vb[0].means[r.keep[0].long()]))  # (the step moved the parameters)


# ---- 9. the C host
@pytest.mark.parametrize("dtype,I0,hidden,R,S", [("f32", 784, [400, 400], 100, 4), ("bf16", 256, [512, 256], 512, 4)])
def test_c_host_prune_units_is_bitwise_the_engines(tmp_path, dtype, I0, hidden, R, S):
    """tools/c_host.c --prune-units 0.5 --predict 4 after one training step against engine.prune_units + compact + predict after
    the same step: tau, the kept lists, the compact parameters and the compact network's predictive outputs."""
    from tests import _children
    from tests.test_c_host import build
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    exe = build(tmp_path)
    out = str(tmp_path / "units.bin")
    cmd = [exe, "--dtype", dtype, "--input", str(I0), "--hidden", ",".join(str(h) for h in hidden), "--classes", "10",
           "--batch", str(R), "--S", "1", "--steps", "1", "--predict", str(S), "--prune-units", "0.5", "--out", out]
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
    block()                                                           # the unpruned predictive (tests/test_predict_gpu.py)
    nl = int(take(np.int32, 1)[0])
    tau = take(np.float32, 1)[0]
    counts = [int(v) for v in take(np.int32, nl)]
    keep = [take(np.int32, n) for n in counts]
    sizes = [I0] + counts
    params = [(take(np.float32, sizes[li + 1] * sizes[li]), take(np.float32, sizes[li + 1] * sizes[li]), take(np.float32, sizes[li + 1]))
              for li in range(nl)]
    w3, b3 = take(np.float32, 10 * sizes[-1]), take(np.float32, 10)
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
    r = eng.prune_units(fraction=0.5)
    c = eng.compact(r)
    p = c.predict(x, S=S, targets=t)
    assert same_bits(np.float32(tau), np.float32(r.tau[0])) and counts == r.hidden, (tau, r.tau, counts, r.hidden)
    for li, w in enumerate(c.vb):
        assert np.array_equal(keep[li], host(r.keep[li]))
        for got, want in zip(params[li], (w.means, w.lvars, w.bias)):
            assert same_bits(got, host(want).reshape(-1))
    assert same_bits(w3, host(c.weight3).reshape(-1)) and same_bits(b3, host(c.bias3))
    assert head == [S, int(p.stacked), p.chunks, c.draw]
    for got, want in zip(fields[:5], (p.probs, p.log_probs, p.entropy, p.expected_entropy, p.mutual_info)):
        assert np.array_equal(got.view(np.uint32), host(want).reshape(-1).view(np.uint32))
    assert np.array_equal(fields[5], host(p.pred))
    assert np.array_equal(fields[6].view(np.uint64), np.array(p.totals, np.float64).view(np.uint64))


# ---- 10. end to end
def test_prune_units_curve_after_training(tmp_path):
    """tests/test_train_gpu.py's recipe (synthetic digits, 64-48 hidden, three epochs, LRT f32), then the unit-pruning curve over
    the test set. Gated: fraction 0 is the unpruned predict, the weight count does not grow with the fraction, every number is
    finite. The accuracies in between are printed, not gated."""
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    opt = train.default_opt(network_name=str(tmp_path / "exp_units"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                            trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32",
                            state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
    m = train.Main(opt)
    hist = m.run(trainSet, testSet, epochs=3)
    assert hist[-1]["devacc"] > 90.0
    inputs_, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
    x, t = m._to_device(inputs_, targets)
    net = m.net
    fractions = [0, 0.25, 0.5, 0.75, 0.9, 1.0]
    for kw in (dict(map=True), dict(S=4), dict(S=4, scope="layer", multiple=8)):
        d0 = net.draw
        rows = net.prune_units_curve(x, t, fractions, **kw)
        assert net.draw == d0                                         # the source engine's counter does not move
        for row in rows:
            print("prune_units_curve", kw, {k: (round(v, 6) if isinstance(v, float) else v) for k, v in row.items()})
        base = net.predict(x, targets=t, **{k: v for k, v in kw.items() if k in ("map", "S")})
        net.draw = d0
        r0 = rows[0]
        assert r0["hidden"] == [64, 48] and r0["n_weights"] == 784 * 64 + 64 * 48 + 48 * 10
        assert (r0["nll"], r0["accuracy"], r0["mean_draw_nll"], r0["mean_draw_accuracy"]) == \
            (base.nll, base.accuracy, base.mean_draw_nll, base.mean_draw_accuracy)
        assert r0["mutual_info"] == float(base.mutual_info.mean().item())
        assert [row["fraction"] for row in rows] == [float(q) for q in fractions]
        assert all(a["n_weights"] >= b["n_weights"] for a, b in zip(rows, rows[1:]))
        assert rows[-1]["hidden"] == ([1, 1] if kw.get("multiple", 1) == 1 else [8, 8])
        for row in rows:
            assert set(row) == {"fraction", "tau", "hidden", "n_weights", "nll", "accuracy", "mean_draw_nll", "mean_draw_accuracy",
                                "mutual_info"}
            assert all(math.isfinite(row[k]) for k in ("nll", "accuracy", "mean_draw_nll", "mean_draw_accuracy", "mutual_info"))
            assert all(not math.isnan(v) for v in row["tau"])
