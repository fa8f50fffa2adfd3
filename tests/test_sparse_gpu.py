"""GPU tests of the compressed pruned form (vbnn_prune_compress, vbnn_forward_sparse: include/vbnn_hip.h, csrc/sparse.hip),
PruneResult.compress / SparsePruneResult, predict() under a compressed view and the C host's --sparse: bit for bit against the
dense pruned shadows and the dense forward where the arithmetic is exact, against a float64 restatement (tests/_sparse_np.py)
at the fp32 accumulation bound of tests/test_parity_gpu.py elsewhere."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _sparse_np as S
from tests.test_prune_gpu import NETS, SEED, dev, host, inputs, keys32, make, same_bits

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": 0, "bf16": 1}


def bits(t):
    """A device tensor's bits as a NumPy integer array (bf16 -> uint16, f32 -> uint32, int16 / int32 -> unsigned)."""
    t = t.contiguous()
    if t.element_size() == 2:
        return host(t.view(torch.int16)).view(np.uint16)
    return host(t.view(torch.int32)).view(np.uint32)


def csr_of(sp, li):
    n = sp.nnz[li]
    return dict(row_ptr=bits(sp.row_ptr[li]), cols=bits(sp.cols[li])[:n].astype(np.int64), mu_v=bits(sp.mu_v[li])[:n],
                var_v=bits(sp.var_v[li])[:n], nnz=n)


# ---- 1. the compressed form is the dense pruned shadows
def check_compressed(eng, r):
    sp, sp2 = r.compress(), r.compress()
    from vbnn_amd.engine import SparsePruneResult
    assert isinstance(sp, SparsePruneResult) and sp.version == r.version and sp.tau == r.tau and sp.n_pruned == r.n_pruned
    assert sp.dense_nbytes == sum(2 * t.t.numel() * t.t.element_size() for t in r.mu_p)
    for li, v in enumerate(eng.vb):
        mu_d, var_d = sp.to_dense(li)
        assert np.array_equal(bits(mu_d), bits(r.mu_p[li].t)), ("mu_p", li)
        assert np.array_equal(bits(var_d), bits(r.var_p[li].t)), ("var_p", li)
        csr = csr_of(sp, li)
        S.csr_check(csr, v.O, v.I)
        assert int(csr["row_ptr"][-1]) == sp.nnz[li] == v.O * v.I - r.layers[li]["n_pruned"]
        for name in ("row_ptr", "cols", "mu_v", "var_v"):           # two runs: the same bytes, slack included
            assert np.array_equal(bits(getattr(sp, name)[li]), bits(getattr(sp2, name)[li])), (name, li)
        # the NumPy build on the library's own keys and the prepared shadows' bits
        want = S.csr_build(keys32(eng, li), np.float32(r.tau[li]), bits(v.mu_s.t)[:, :v.I], bits(v.var_s.t)[:, :v.I])
        assert np.array_equal(csr["row_ptr"], want["row_ptr"]) and np.array_equal(csr["cols"], want["cols"])
        assert np.array_equal(csr["mu_v"], want["mu_v"]) and np.array_equal(csr["var_v"], want["var_v"])
        assert np.array_equal(host(sp.mask(li)), host(r.mask(li)))
    return sp


@pytest.mark.parametrize("net,dtype", [("mnist", "f32"), ("mnist", "bf16"), ("odd", "f32"), ("odd", "bf16")])
def test_compressed_form_is_the_dense_pruned_shadows(oracle, net, dtype):
    eng = make(oracle, net, dtype=dtype)
    W = sum(v.O * v.I for v in eng.vb)
    for scope in ("global", "layer"):
        for kw in (dict(fraction=0.0), dict(fraction=0.5), dict(fraction=0.98), dict(fraction=1.0), dict(threshold=0.005)):
            r = eng.prune(scope=scope, **kw)
            sp = check_compressed(eng, r)
            print(f"{net} {dtype} {scope} {kw}: nnz {sp.nnz}, {sp.nbytes} B against {sp.dense_nbytes} B dense")
            assert sum(sp.nnz) == W - r.n_pruned
            if kw.get("fraction") == 1.0:
                assert sp.nnz == [0] * len(eng.vb)
            if kw.get("fraction") == 0.0:
                assert sum(sp.nnz) == W


@pytest.mark.parametrize("case", ["equal", "ties", "zeros", "nan"])
def test_compress_on_adversarial_keys(oracle, case):
    """The cases of test_selection_on_adversarial_keys (tests/test_prune_gpu.py)."""
    eng = make(oracle, "odd")
    if case == "equal":
        for v in eng.vb:
            v.means.fill_(0.25); v.lvars.fill_(math.log(1e-2))
    elif case == "ties":
        for v in eng.vb:
            v.means.copy_(torch.round(v.means * 8).clamp_(-8, 7) / 8); v.lvars.fill_(math.log(1e-2))
    elif case == "zeros":
        eng.vb[0].means[:20].zero_()
    else:
        eng.vb[1].means[3, 5] = float("nan")
    eng.prepare()
    W = sum(v.O * v.I for v in eng.vb)
    for q in (0.1, 0.5, 0.9, 1.0):
        r = eng.prune(fraction=q)
        sp = check_compressed(eng, r)
        assert sum(sp.nnz) == W - r.n_pruned
        if case == "equal" and q < 1.0:
            assert sum(sp.nnz) == W                                 # every key ties at tau: nothing is below it
        if case == "nan":                                           # a NaN key is an entry, even at tau = +inf
            csr = csr_of(sp, 1)
            assert 5 in csr["cols"][csr["row_ptr"][3]:csr["row_ptr"][4]].tolist()
            if q == 1.0:
                assert sp.nnz == [0, 1]
    if case == "zeros":                                             # kept weights whose value is zero are still entries
        r = eng.prune(threshold=0.0)
        sp = check_compressed(eng, r)
        assert sum(sp.nnz) == W and int((bits(sp.mu_v[0]) == 0).sum()) >= 20 * eng.vb[0].I


# ---- raw calls of the two forwards on operands of the test's own
def _ctx():
    from vbnn_amd.nn import Context
    return Context.get(torch.device("cuda", 0))


def _packed(a, dtype):
    """A rows x cols array as a packed operand (zero pads)."""
    from vbnn_amd.nn import _Packed
    p = _Packed(a.shape[0], a.shape[1], TDT[dtype], torch.device("cuda", 0))
    p.t[:, :a.shape[1]] = dev(np.asarray(a, np.float32)).to(TDT[dtype])
    return p


def _outputs(N, O, dtype):
    from vbnn_amd.nn import _Packed
    d = torch.device("cuda", 0)
    return dict(y=torch.zeros(N, O, dtype=torch.float32, device=d), h=_Packed(N, O, TDT[dtype], d), h2=_Packed(N, O, TDT[dtype], d),
                hT=_Packed(O, N, TDT[dtype], d), h2T=_Packed(O, N, TDT[dtype], d))


def run_dense(dtype, mu, var, x, x2, bias, N, I, O, layer, draw, row0, rpd):
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    o = _outputs(N, O, dtype)
    a = L.FwdArgs(w=mu.ptr, w2=var.ptr if var is not None else None, x=x.ptr, x2=x2.ptr if (x2 is not None and var is not None) else None,
                  ld_w=mu.ld, ld_x=x.ld, N=N, I=I, O=O, bias=_p(bias), seed=SEED, layer=layer, draw=draw, draw_dev=None, row0=row0,
                  y=_p(o["y"]), ld_y=O, r=None, ld_r=0, r_packed=1, relu=1, h=o["h"].ptr, h2=o["h2"].ptr, ld_h=o["h"].ld,
                  hT=o["hT"].ptr, h2T=o["h2T"].ptr, ld_hT=o["hT"].ld, rows_per_draw=rpd)
    L.check(L.lib().vbnn_forward(_ctx().h, CODE[dtype], C.byref(a)))
    return o


def upload_csr(csr, dtype, I, idx_bytes=None):
    ib = idx_bytes or (2 if I <= 65536 else 4)
    n = max(csr["nnz"], 1)
    cols = np.zeros(n, np.uint16 if ib == 2 else np.uint32)
    cols[:csr["nnz"]] = csr["cols"]
    vals = []
    for k in ("mu_v", "var_v"):
        v = np.zeros(n, np.float32)
        v[:csr["nnz"]] = csr[k]
        vals.append(dev(v).to(TDT[dtype]))
    return dict(row_ptr=dev(csr["row_ptr"].view(np.int32)), cols=dev(cols.view(np.int16 if ib == 2 else np.int32)), mu_v=vals[0],
                var_v=vals[1], idx_bytes=ib)


def run_sparse(dtype, sp, xT, x2T, bias, N, I, O, layer, draw, row0, rpd, lrt=True):
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    o = _outputs(N, O, dtype)
    a = L.SparseFwdArgs(row_ptr=_p(sp["row_ptr"]), cols=_p(sp["cols"]), mu_v=_p(sp["mu_v"]), var_v=_p(sp["var_v"]) if lrt else None,
                        idx_bytes=sp["idx_bytes"], xT=xT.ptr, x2T=x2T.ptr if x2T is not None else None, ld_xT=xT.ld, N=N, I=I, O=O,
                        bias=_p(bias), seed=SEED, layer=layer, draw=draw, row0=row0, y=_p(o["y"]), ld_y=O, relu=1, h=o["h"].ptr,
                        h2=o["h2"].ptr, ld_h=o["h"].ld, hT=o["hT"].ptr, h2T=o["h2T"].ptr, ld_hT=o["hT"].ld, rows_per_draw=rpd)
    st = L.lib().vbnn_forward_sparse(_ctx().h, CODE[dtype], C.byref(a))
    L.check(st)
    return o


def _same_outputs(a, b, what):
    assert same_bits(host(a["y"]), host(b["y"])), (what, "y", float((a["y"] - b["y"]).abs().max()))
    for k in ("h", "h2", "hT", "h2T"):
        assert np.array_equal(bits(a[k].t), bits(b[k].t)), (what, k)


# ---- 2. exact on exact operands
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("I,O,N,rpd,row0", [(784, 400, 30, 0, 0), (784, 400, 30, 10, 5), (400, 400, 100, 0, 0), (400, 400, 100, 25, 7),
                                            (67, 33, 5, 0, 0), (67, 33, 5, 1, 3), (4096, 4096, 30, 0, 0), (4096, 4096, 30, 1, 11),
                                            (4096, 4096, 200, 0, 0)])
def test_exact_operands_are_bitwise_the_dense_forward(dtype, I, O, N, rpd, row0):
    """Small-integer means and inputs, power-of-two variances: every fp32 partial sum of either kernel is exact, so the sparse
    forward's y, h, h2, hT, h2T must be the dense forward's on the same pruned shadows bit for bit, noise included."""
    rng = np.random.default_rng(I * 7 + O * 3 + N)
    kept = rng.random((O, I)) < 0.1
    kept[::7] = False                                               # rows without entries
    kept[1, :] = True                                               # a full row
    mu = rng.integers(-3, 4, (O, I)).astype(np.float32) * kept      # (a kept weight may be zero)
    var = (2.0 ** rng.integers(-4, 1, (O, I))).astype(np.float32) * kept
    x = rng.integers(-3, 4, (N, I)).astype(np.float32)
    x[N // 2] = 0.0                                                 # an all-zero input row: v = 0, no noise
    bias = dev(rng.integers(-2, 3, O).astype(np.float32))
    csr = S.csr_build(kept.astype(np.float32), 0.5, mu, var)
    sp = upload_csr(csr, dtype, I)
    layer, draw = 1, 3
    dense = run_dense(dtype, _packed(mu, dtype), _packed(var, dtype), _packed(x, dtype), _packed(x * x, dtype), bias, N, I, O, layer,
                      draw, row0, rpd)
    xT, x2T = _packed(x.T, dtype), _packed((x * x).T, dtype)
    _same_outputs(run_sparse(dtype, sp, xT, None, bias, N, I, O, layer, draw, row0, rpd), dense, "squares in registers")
    _same_outputs(run_sparse(dtype, sp, xT, x2T, bias, N, I, O, layer, draw, row0, rpd), dense, "x2T given")
    assert float(dense["y"].abs().max()) > 0 and not bool(torch.equal(dense["y"][0], dense["y"][N - 1]))
    if rpd == 0:                                                    # MAP form: the means alone
        dm = run_dense(dtype, _packed(mu, dtype), None, _packed(x, dtype), None, bias, N, I, O, layer, draw, row0, 0)
        _same_outputs(run_sparse(dtype, sp, xT, None, bias, N, I, O, layer, draw, row0, 0, lrt=False), dm, "MAP")
    if I <= 784:                                                    # 32-bit column indices compute the same
        sp4 = upload_csr(csr, dtype, I, idx_bytes=4)
        _same_outputs(run_sparse(dtype, sp4, xT, None, bias, N, I, O, layer, draw, row0, rpd), dense, "uint32 columns")


# ---- 3. random operands against float64
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("I,O,N,rpd,row0", [(784, 400, 30, 10, 5), (400, 400, 100, 0, 0), (67, 33, 5, 0, 2), (4096, 4096, 30, 1, 0),
                                            (4096, 4096, 200, 0, 0)])
def test_random_operands_match_float64(oracle, dtype, I, O, N, rpd, row0):
    """Float64 from the operand bits the kernel reads and the z it draws; per element |err| <= 4e-6 sum |a b| + 1e-6 |want| for
    fp32 y (tests/test_parity_gpu.py's bound), + 2^-8 |want| for packed bf16 outputs (one rounding to the operand type)."""
    from vbnn_amd.nn import fill_normal
    rng = np.random.default_rng(I + O + N)
    tdt = TDT[dtype]

    def rounded(a):
        return host(dev(a.astype(np.float32)).to(tdt).float())
    kept = rng.random((O, I)) < 0.1
    kept[::5] = False
    mu = rounded(rng.normal(size=(O, I))) * kept
    var = rounded(np.exp(math.log(1e-2) + 0.75 * rng.normal(size=(O, I)))) * kept
    x = rounded(rng.normal(size=(N, I)))
    x2 = rounded(x * x)                                             # the packer's square: T(x . x) of the rounded x
    b = rng.normal(size=O).astype(np.float32)
    csr = S.csr_build(kept.astype(np.float32), 0.5, mu, var)
    sp = upload_csr(csr, dtype, I)
    layer, draw = 2, 4
    z = np.empty((N, O), np.float64)
    zt = torch.empty(rpd if rpd else N, O, dtype=torch.float32, device="cuda")
    for k in range(N // rpd if rpd else 1):                         # stacked: draw k's rows are minibatch rows row0 ..
        if dtype == "bf16":
            fill_normal(zt, SEED, 2, layer, draw + k, row0, hw=True)    # the form a bf16 forward draws
            zk = host(zt)
        else:
            zk = oracle.fill_normal(zt.shape[0], O, SEED, 2, layer, draw + k, row0)
        z[k * zt.shape[0]:(k + 1) * zt.shape[0]] = zk
    got = run_sparse(dtype, sp, _packed(x.T, dtype), None, dev(b), N, I, O, layer, draw, row0, rpd)
    want, want_h, absprod = S.forward64(csr, O, x, x2, b, z)
    tol = 4e-6 * absprod + 1e-6 * np.abs(want)
    err = np.abs(host(got["y"]).astype(np.float64) - want)
    print(f"{dtype} {I}x{O} N {N}: y max err {err.max():.3e}, max err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all(), f"y: {(err > tol).sum()} off, max {err.max():.3e}"
    tol_h = tol + (2.0 ** -8 * np.abs(want_h) if dtype == "bf16" else 0.0)
    for k, w in (("h", want_h), ("hT", want_h.T)):
        g = host(got[k].t.float()).astype(np.float64)[:w.shape[0], :w.shape[1]]
        e = np.abs(g - w)
        t = tol_h if k == "h" else tol_h.T
        assert (e <= t).all(), f"{k}: {(e > t).sum()} off, max {e.max():.3e}"
    # the squares are squares of what was stored
    hh = host(got["h"].t.float()).astype(np.float32)[:N, :O]
    assert np.array_equal(bits(got["h2"].t)[:N, :O], bits(dev(hh * hh).to(tdt)))
    assert np.array_equal(bits(got["h2T"].t)[:O, :N], bits(got["h2"].t)[:N, :O].T)
    again = run_sparse(dtype, sp, _packed(x.T, dtype), None, dev(b), N, I, O, layer, draw, row0, rpd)
    _same_outputs(again, got, "two runs")


# ---- 4. end to end
def _hand_pruned(oracle, eng, r, dtype, **kw):
    from tests.test_prune_gpu import _hand_pruned as hp
    return hp(oracle, eng, r, "mnist", "lrt", dtype, **kw)


@pytest.mark.parametrize("kw,pk,q", [
    (dict(predict_stacked=True), dict(S=4), 0.9),
    (dict(predict_stacked=False), dict(S=4), 0.9),
    (dict(predict_rows=4 * 16), dict(S=4), 0.9),                    # chunked: 7 chunks of 16 rows
    (dict(), dict(S=3), 0.0),                                       # nothing pruned
    (dict(), dict(S=3), 0.5),
    (dict(), dict(S=3), 0.98),
])
def test_predict_under_the_sparse_view_f32(oracle, kw, pk, q):
    """predict under the compressed view and under the dense view of the same pruning, from the same draw counter: both within
    the float64 oracle's propagated bound (tests/test_predict_gpu.py: oracle_draw / check_against_oracle), hence within twice
    it of each other; the counters advance identically."""
    from tests.test_predict_gpu import check_against_oracle, oracle_draw
    eng = make(oracle, "mnist", **kw)
    R = 100
    x, t = inputs(oracle, R, 784)
    r = eng.prune(fraction=q)
    sp = r.compress()
    other = _hand_pruned(oracle, eng, r, "f32", **kw)               # fp32 parameters masked by hand: what the oracle reads
    d0 = eng.draw
    with eng.pruned(r):
        a = eng.predict(dev(x), targets=dev(t), **pk)
    d1, eng.draw = eng.draw, d0
    with eng.pruned(sp):
        b = eng.predict(dev(x), targets=dev(t), **pk)
    assert eng.draw == d1 == d0 + pk["S"] and (a.stacked, a.chunks, a.S) == (b.stacked, b.chunks, b.S)
    if "predict_rows" in kw:
        assert b.chunks == 7
    check_against_oracle(oracle, other, b, x, t, pk["S"], d0 + 1)
    e = max(float(np.max(oracle_draw(oracle, other, x, d0 + 1 + s)[1])) for s in range(pk["S"]))
    tol_p, tol_h = max(1e-5, 2 * e), max(1e-5, 2 * e * (1 + math.log(10)))
    assert float((a.probs - b.probs).abs().max()) <= 2 * tol_p
    for k in ("entropy", "expected_entropy", "mutual_info"):
        assert float((getattr(a, k) - getattr(b, k)).abs().max()) <= 4 * tol_h, k
    assert abs(a.nll - b.nll) <= 3e-5 * abs(a.nll) + 2 * tol_p and abs(a.mean_draw_nll - b.mean_draw_nll) <= 3e-5 * abs(a.mean_draw_nll) + 2 * tol_p
    print(f"{kw} {pk} q {q}: nll dense {a.nll:.6f} sparse {b.nll:.6f}, max |dp| {float((a.probs - b.probs).abs().max()):.3e}, tol {tol_p:.3e}")


def test_map_predict_under_the_sparse_view(oracle):
    from tests.test_predict_gpu import check_against_oracle
    for mode in ("lrt", "wn"):
        eng = make(oracle, "mnist", mode)
        x, t = inputs(oracle, 64, 784)
        r = eng.prune(fraction=0.9)
        with eng.pruned(r):
            a = eng.predict(dev(x), targets=dev(t), map=True)
        with eng.pruned(r.compress()):
            b = eng.predict(dev(x), targets=dev(t), map=True)
        assert eng.draw == 0 and b.S == 1
        assert float((a.probs - b.probs).abs().max()) <= 2e-5 and bool((b.mutual_info == 0).all())
        if mode == "lrt":
            from tests.test_prune_gpu import _hand_pruned as hp
            other = hp(oracle, eng, r, "mnist", "lrt", "f32", quicktest=True)
            # (quicktest: the oracle's draw is not used by a MAP pass; compare the log-softmax of the means' forward)
            h = x.astype(np.float64)
            for v in other.vb:
                h = np.maximum(h @ host(v.means).astype(np.float64).T + host(v.bias).astype(np.float64), 0.0)
            lg = h @ host(other.weight3).astype(np.float64).T + host(other.bias3).astype(np.float64)
            lp = lg - lg.max(1, keepdims=True)
            lp = lp - np.log(np.exp(lp).sum(1, keepdims=True))
            assert np.abs(host(b.probs) - np.exp(lp)).max() <= 2e-5
        with eng.pruned(r.compress()):
            if mode == "wn":
                with pytest.raises(ValueError, match="pruned view"):
                    eng.predict(dev(x), S=3)                        # weight-noise draws stay refused under any pruned view


@pytest.mark.parametrize("stacked", [True, False])
def test_predict_under_the_sparse_view_bf16(oracle, stacked):
    """bf16: the two views run different kernels, so an activation may differ by one bf16 rounding (2^-8 relative) in each of
    the two hidden layers -- a logit by at most 2 x 2^-8 x sum_i |w3_ci h_i|, a log-probability by twice that (the tolerance
    test_wide_bf16_properties of tests/test_predict_gpu.py derives for two dense kernels)."""
    eng = make(oracle, "mnist", dtype="bf16", predict_stacked=stacked)
    R, Sn = 64, 4
    x, t = inputs(oracle, R, 784)
    r = eng.prune(fraction=0.9)
    d0 = eng.draw
    with eng.pruned(r):
        a = eng.predict(dev(x), S=Sn, targets=dev(t))
    hbuf = eng._pred_bufs[len(eng.vb)].x.t[:, :400].double().abs().clone()
    eng.draw = d0
    with eng.pruned(r.compress()):
        b = eng.predict(dev(x), S=Sn, targets=dev(t))
    assert eng.draw == d0 + Sn and a.stacked == b.stacked == stacked
    tol = 2 * 2 * (2 ** -8) * float((hbuf @ eng.weight3.double().abs().T).max())
    d = float((a.log_probs.double() - b.log_probs.double()).abs().max())
    print(f"bf16 stacked {stacked}: max |d log p| {d:.3e}, tol {tol:.3e}; nll dense {a.nll:.6f} sparse {b.nll:.6f}")
    assert d <= tol and abs(a.nll - b.nll) <= tol
    assert float((b.probs.double().sum(1) - 1).abs().max()) <= 1e-5 and float(b.mutual_info.min()) >= -1e-6
    # ... a worst case (every rounding the same way). Row by row the roundings of h are independent and each within 2^-8 of the
    # value: a logit's difference is a sum of independent terms of standard deviation at most 2^-8 |w3_ci h_i| / sqrt(3), so six
    # of its standard deviations (x 2 for the log-softmax) bound the typical row -- a wrong draw or noise row misses it by far
    # (the second tier of test_wide_bf16_properties). The average over draws moves by at most the largest draw's difference:
    # stacked, the buffer holds every draw's h (row s R + r) and the row's bound is the largest over its draws; sequential, it
    # holds the last draw's.
    w3 = eng.weight3.double()
    sd = (2 ** -8) * torch.sqrt(((hbuf * hbuf) @ (w3 * w3).T).max(1).values / 3)
    sd = sd.reshape(-1, R).max(0).values
    drow = (a.log_probs.double() - b.log_probs.double()).abs().max(1).values
    assert float((drow <= 2 * 6 * sd).double().mean()) >= 0.99, float((drow / sd).median())
    # a log-probability difference e moves an entropy by at most e (1 + log C); the mutual information is a difference of two
    lim = (2 * 6 * sd) * (1 + math.log(10))
    for k, f in (("entropy", 1), ("expected_entropy", 1), ("mutual_info", 2)):
        dk = (getattr(a, k).double() - getattr(b, k).double()).abs()
        assert float(dk.max()) <= f * tol * (1 + math.log(10)), k
        assert float((dk <= f * lim).double().mean()) >= 0.99, (k, float(dk.max()))
    assert abs(a.mean_draw_nll - b.mean_draw_nll) <= tol and abs(a.accuracy - b.accuracy) <= 100.0 * float((drow > 0).sum()) / R + 1e-9


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_draw_counters_advance_identically(oracle, dtype):
    """opt.device_draw: the host's draw counter and the device-resident one advance by S under either view, by nothing for a
    MAP pass, and stay equal to each other."""
    eng = make(oracle, "odd", dtype=dtype, device_draw=True)
    x, t = inputs(oracle, 37, 70)
    xd, td = dev(x), dev(t)
    r = eng.prune(fraction=0.5)
    sp = r.compress()

    def counters():
        return eng.draw, int(host(eng._draw_dev)[0])
    eng.sample()                                                    # (both counters off zero)
    assert counters() == (1, 1)
    seen = {}
    for name, view in (("dense", r), ("sparse", sp)):
        h0, d0 = counters()
        with eng.pruned(view):
            eng.predict(xd, S=3, targets=td)
            h1, d1 = counters()
            eng.predict(xd, targets=td, map=True)
            h2, d2 = counters()
            eng.predict(xd, S=1)
        h3, d3 = counters()
        seen[name] = (h1 - h0, d1 - d0, h2 - h1, d2 - d1, h3 - h2, d3 - d2)
        assert (h1, h2, h3) == (d1, d2, d3)
    assert seen["dense"] == seen["sparse"] == (3, 3, 0, 0, 1, 1), seen
    assert counters() == (9, 9)
    # and from the same counter the two views draw the same noise: equal at fp32 up to the accumulation order
    eng.draw, c0 = 20, 20
    eng._draw_dev.fill_(20)
    with eng.pruned(r):
        a = eng.predict(xd, S=3, targets=td)
    eng.draw = c0
    eng._draw_dev.fill_(c0)
    with eng.pruned(sp):
        b = eng.predict(xd, S=3, targets=td)
    assert counters() == (23, 23)
    if dtype == "f32":                                              # (bf16: test_predict_under_the_sparse_view_bf16 holds the values)
        assert float((a.probs - b.probs).abs().max()) <= 2e-5


# ---- the device-chained, all-layers form of the library call: select -> compress through tau_dev, no host read in between
@pytest.mark.parametrize("net,dtype", [("mnist", "f32"), ("mnist", "bf16"), ("odd", "f32"), ("odd", "bf16")])
@pytest.mark.parametrize("q", [0.5, 0.98])
def test_compress_chained_behind_select_all_layers_in_one_call(oracle, net, dtype, q):
    """vbnn_prune_select then ONE vbnn_prune_compress for all layers with tau_dev (tau_host a decoy that would keep nothing
    the same), queued back to back: the same bytes as the engine's per-layer host-tau compress, and to_dense the dense shadows."""
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import SparsePruneResult
    from vbnn_amd.nn import _p
    eng = make(oracle, net, dtype=dtype)
    r = eng.prune(fraction=q)
    ref = r.compress()
    nl = len(eng.vb)
    lib, ctx = L.lib(), eng.ctx.h
    pd = (L.PruneDesc * nl)()
    sd = (L.SparseDesc * nl)()
    W = sum(v.O * v.I for v in eng.vb)
    slack = 7                                                       # capacity above the count: the slack is not written
    rp = [torch.full((v.O + 1,), -1, dtype=torch.int32, device="cuda") for v in eng.vb]
    cols = [torch.full((n + slack,), -1, dtype=torch.int16, device="cuda") for n in ref.nnz]
    mu_v = [torch.full((n + slack,), 7.0, dtype=TDT[dtype], device="cuda") for n in ref.nnz]
    var_v = [torch.full((n + slack,), 7.0, dtype=TDT[dtype], device="cuda") for n in ref.nnz]
    nnz_dev = torch.full((nl,), -1, dtype=torch.int32, device="cuda")
    for li, v in enumerate(eng.vb):
        pd[li] = L.PruneDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I)
        sd[li] = L.SparseDesc(row_ptr=_p(rp[li]), cols=_p(cols[li]), mu_v=_p(mu_v[li]), var_v=_p(var_v[li]), O=v.O, I=v.I,
                              nnz_cap=ref.nnz[li] + slack, nnz_dev=C.c_void_p(nnz_dev.data_ptr() + 4 * li), idx_bytes=2)
    nb = C.c_size_t()
    L.check(lib.vbnn_prune_workspace_bytes(nl, pd, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    tau = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    with eng._on_stream():
        L.check(lib.vbnn_prune_select(ctx, nl, pd, int(math.floor(q * W)), _p(tau), _p(ws), nb.value))
        L.check(lib.vbnn_prune_compress(ctx, CODE[dtype], nl, pd, sd, _p(tau), float("inf")))     # tau_host = +inf would keep nothing
    assert same_bits(np.float32(host(tau)[0]), np.float32(r.tau[0]))
    assert (host(nnz_dev).view(np.uint32)).tolist() == ref.nnz
    for li, v in enumerate(eng.vb):
        n = ref.nnz[li]
        assert np.array_equal(bits(rp[li]), bits(ref.row_ptr[li])), li
        for got, want in ((cols[li], ref.cols[li]), (mu_v[li], ref.mu_v[li]), (var_v[li], ref.var_v[li])):
            assert np.array_equal(bits(got)[:n], bits(want)[:n]), li
        assert bool((cols[li][n:] == -1).all()) and bool((mu_v[li][n:] == 7.0).all()) and bool((var_v[li][n:] == 7.0).all())
    raw = SparsePruneResult(r, rp, cols, mu_v, var_v, ref.nnz, [2] * nl, ref.dense_nbytes)
    for li in range(nl):
        mu_d, var_d = raw.to_dense(li)
        assert np.array_equal(bits(mu_d), bits(r.mu_p[li].t)) and np.array_equal(bits(var_d), bits(r.var_p[li].t)), li


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_everything_pruned_is_bitwise_the_dense_view(oracle, dtype):
    from tests.test_prune_gpu import _same_result
    eng = make(oracle, "mnist", dtype=dtype)
    for li, v in enumerate(eng.vb):
        v.bias.copy_(dev(oracle.fill_normal(1, v.O, SEED, 3, li, 9)[0]))
    eng.bias3.copy_(dev(oracle.fill_normal(1, 10, SEED, 3, 5, 9)[0]))
    r = eng.prune(fraction=1.0)
    sp = r.compress()
    assert sp.nnz == [0, 0] and sp.nbytes < 8192
    x, t = inputs(oracle, 37, 784)
    for Sn in (1, 3):
        d0 = eng.draw
        with eng.pruned(r):
            a = eng.predict(dev(x), S=Sn, targets=dev(t))
        eng.draw = d0
        with eng.pruned(sp):
            b = eng.predict(dev(x), S=Sn, targets=dev(t))
        _same_result(a, b)


# ---- 5. guards
def test_guards(oracle):
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    eng = make(oracle, "odd", fuse_kl=True, state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-4),
               varState=dict(learningRate=5e-2))
    x, t = inputs(oracle, 37, 70)
    xd, td = dev(x), dev(t)
    r = eng.prune(fraction=0.5)
    sp = r.compress()
    other = make(oracle, "odd")
    with pytest.raises(ValueError):
        other.use_pruned(sp)                                        # another engine's result
    with pytest.raises(ValueError):
        other._compress(r)
    eng.use_pruned(sp)
    eng.predict(xd, S=2, targets=td)
    eng.resetGradients(); eng.sample(); eng.run(xd, td); eng.finish()
    eng.predict(xd, S=2, targets=td)                                # training steps do not invalidate a view ...
    eng.update(eng.opt)
    with pytest.raises(RuntimeError):                               # ... an update does
        eng.predict(xd, S=2, targets=td)
    with pytest.raises(RuntimeError):
        r.compress()                                                # a stale dense result cannot be compressed either
    eng.use_pruned(None)
    eng.predict(xd, S=2, targets=td)
    wn = make(oracle, "odd", "wn")
    with wn.pruned(wn.prune(fraction=0.5).compress()):
        with pytest.raises(ValueError, match="pruned view"):
            wn.predict(xd, S=3)
        wn.predict(xd, map=True)
    # the index width: 16-bit columns with I > 65536 are refused by both entry points, 32-bit columns are taken
    O, I = 2, 70000
    means = torch.ones(O, I, dtype=torch.float32, device="cuda")
    means[:, ::2] = 0.0
    lvars = torch.zeros(O, I, dtype=torch.float32, device="cuda")
    rp = torch.zeros(O + 1, dtype=torch.int32, device="cuda")
    cols = torch.zeros(O * I, dtype=torch.int32, device="cuda")
    mu_v, var_v = torch.zeros(O * I, device="cuda"), torch.zeros(O * I, device="cuda")
    nnz = torch.zeros(1, dtype=torch.int32, device="cuda")
    pd = (L.PruneDesc * 1)(L.PruneDesc(means=_p(means), lvars=_p(lvars), O=O, I=I))

    def sdesc(ib):
        return (L.SparseDesc * 1)(L.SparseDesc(row_ptr=_p(rp), cols=_p(cols), mu_v=_p(mu_v), var_v=_p(var_v), O=O, I=I, nnz_cap=O * I,
                                               nnz_dev=_p(nnz), idx_bytes=ib))
    ctx = _ctx().h
    assert L.lib().vbnn_prune_compress(ctx, 0, 1, pd, sdesc(2), None, 0.5) == 1          # VBNN_ERR_INVALID
    assert b"idx_bytes" in L.lib().vbnn_last_error()
    L.check(L.lib().vbnn_prune_compress(ctx, 0, 1, pd, sdesc(4), None, 0.5))
    assert host(nnz)[0] == O * I // 2 and host(rp).tolist() == [0, I // 2, O * I // 2]
    assert np.array_equal(host(cols)[:I // 2], np.arange(1, I, 2))
    N = 3
    xT = torch.ones(I, 64, dtype=torch.float32, device="cuda")
    y = torch.zeros(N, O, dtype=torch.float32, device="cuda")

    def fargs(ib):
        return L.SparseFwdArgs(row_ptr=_p(rp), cols=_p(cols), mu_v=_p(mu_v), var_v=None, idx_bytes=ib, xT=_p(xT), ld_xT=64, N=N, I=I, O=O,
                               y=_p(y), ld_y=O)
    assert L.lib().vbnn_forward_sparse(ctx, 0, C.byref(fargs(2))) == 1
    L.check(L.lib().vbnn_forward_sparse(ctx, 0, C.byref(fargs(4))))
    assert np.array_equal(host(y), np.full((N, O), I // 2, np.float32))
    # a capacity below the count: nothing is written past it, the count is still reported
    cols.fill_(-1)
    L.check(L.lib().vbnn_prune_compress(ctx, 0, 1, pd, (L.SparseDesc * 1)(L.SparseDesc(
        row_ptr=_p(rp), cols=_p(cols), mu_v=_p(mu_v), var_v=_p(var_v), O=O, I=I, nnz_cap=100, nnz_dev=_p(nnz), idx_bytes=4)), None, 0.5))
    assert host(nnz)[0] == O * I // 2 and bool((cols[100:] == -1).all()) and bool((cols[:100] >= 0).all())


# ---- 6. nothing else moved
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_is_undisturbed(oracle, dtype):
    a, b = make(oracle, "mnist", dtype=dtype), make(oracle, "mnist", dtype=dtype)
    x, t = inputs(oracle, 64, 784)
    xd, td = dev(x), dev(t)
    sp = a.prune(fraction=0.9).compress()
    with a.pruned(sp):
        a.predict(xd, S=2, targets=td)
    b.predict(xd, S=2, targets=td)                                  # (the same draws consumed)
    a.use_pruned(sp)                                                # run() does not look at the view
    for e in (a, b):
        e.resetGradients(); e.sample(); e.run(xd, td); e.finish()
    assert a.loss_and_accuracy() == b.loss_and_accuracy()
    assert same_bits(host(a.grads), host(b.grads)) and np.abs(host(a.grads)).max() > 0
    for va, vb_ in zip(a.vb, b.vb):
        assert same_bits(host(va.means), host(vb_.means)) and same_bits(host(va.lvars), host(vb_.lvars))
        assert np.array_equal(bits(va.mu_s.t), bits(vb_.mu_s.t)) and np.array_equal(bits(va.var_s.t), bits(vb_.var_s.t))


# ---- 7. the C host
@pytest.mark.parametrize("dtype,I0,hidden,R,S", [("f32", 784, [400, 400], 100, 4), ("bf16", 256, [512, 256], 512, 4)])
def test_c_host_sparse_is_bitwise_the_engines(tmp_path, dtype, I0, hidden, R, S):
    """tools/c_host.c --prune 0.9 --sparse --predict 4 after one training step against engine.prune(...).compress() + predict."""
    from tests import _children
    from tests.test_c_host import build
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    exe = build(tmp_path)
    out = str(tmp_path / "sparse.bin")
    cmd = [exe, "--dtype", dtype, "--input", str(I0), "--hidden", ",".join(str(h) for h in hidden), "--classes", "10",
           "--batch", str(R), "--S", "1", "--steps", "1", "--predict", str(S), "--prune", "0.9", "--sparse", "--out", out]
    res = _children.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    print(res.stdout.strip())
    assert "compressed view" in res.stdout
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
    block()                                                        # the unpruned predictive
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
    with eng.pruned(r.compress()):
        p = eng.predict(x, S=S, targets=t)
    assert same_bits(np.float32(tau), np.float32(r.tau[0])) and np.array_equal(stats, np.array(r.stats)), (tau, r.tau, stats, r.stats)
    assert head == [S, int(p.stacked), p.chunks, eng.draw]
    for got, want in zip(fields[:5], (p.probs, p.log_probs, p.entropy, p.expected_entropy, p.mutual_info)):
        assert np.array_equal(got.view(np.uint32), host(want).reshape(-1).view(np.uint32))
    assert np.array_equal(fields[5], host(p.pred))
    assert np.array_equal(fields[6].view(np.uint64), np.array(p.totals, np.float64).view(np.uint64))


def test_prune_curve_sparse(oracle):
    eng = make(oracle, "odd")
    x, t = inputs(oracle, 37, 70)
    rows = eng.prune_curve_sparse(dev(x), dev(t), [0.0, 0.5, 1.0], S=2)
    W = sum(v.O * v.I for v in eng.vb)
    assert [row["nnz"] for row in rows] == [W - row["n_pruned"] for row in rows] and rows[0]["nnz"] == W and rows[-1]["nnz"] == 0
    assert all(row["nbytes"] > 0 and row["dense_nbytes"] == rows[0]["dense_nbytes"] for row in rows) and eng._pruned is None
    assert rows[-1]["nbytes"] < rows[1]["nbytes"] < rows[0]["nbytes"] and eng.draw == 6
