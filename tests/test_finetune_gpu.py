"""Training under a held pruning mask on the GPU: vbnn_prepare_masked / vbnn_update_masked / vbnn_calc_lc_masked through the
C ABI on three shapes (ragged tiles with the scalar path, whole vector tiles, the flat form), in f32 and bf16, under four
masks; then FusedMLP.hold_pruned / release_pruned, the C host's --hold, and what fine-tuning buys on the accuracy recipe.

Every comparison of a kept weight is BITWISE against vbnn_update / vbnn_prepare on copies of the same inputs: the masked sweeps
are template instantiations of those kernels, not copies. The float64 sums (stats[0], stats[1], the KL sum) are compared to
1e-10 relative: they are double-accumulated over at most 2^17 terms, so the reordering error is bounded by n 2^-53 ~ 1.5e-11."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(70, 50, True), (128, 192, True), (256, 512, False)]      # O, I, transposed shadows
DTYPES = ["f32", "bf16"]
MASKS = ["half", "ninety", "rowcol", "groups"]
B_KL = 50.0                                                          # a small B: the KL part of the gradients matters
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, lambda_=1.0)
FIELDS = ("means", "lvars", "m_mu", "v_mu", "m_lv", "v_lv")


def _mods():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, nn


def _mask(kind, O, I, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "zero":
        m = torch.zeros(O, I, dtype=torch.uint8)
    elif kind == "half":
        m = (torch.rand(O, I, generator=g) < 0.5).to(torch.uint8)
    elif kind == "ninety":
        m = (torch.rand(O, I, generator=g) < 0.9).to(torch.uint8)
    elif kind == "rowcol":                                           # one whole row and one whole column
        m = torch.zeros(O, I, dtype=torch.uint8)
        m[O // 3, :] = 1
        m[:, I // 2 + 1] = 1
    elif kind == "groups":                                           # 1, 2, 3 weights of a group of four, and the last (ragged) column
        m = torch.zeros(O, I, dtype=torch.uint8)
        for r in range(O):
            for g4 in range(I // 4):
                n = (r + g4) % 4                                     # 0 .. 3 pruned in this group, at rotating places
                for j in range(n):
                    m[r, 4 * g4 + (r + j) % 4] = 1
        m[:, I - 1] = 1
    else:
        raise ValueError(kind)
    return m.cuda()


class State:
    """One layer's tensors for direct ABI calls: parameters, gradients, non-zero Adam moments, bias, shadows, statistics."""

    def __init__(self, O, I, transposed, dtype, seed=5):
        L, nn = _mods()
        self.O, self.I, self.transposed, self.dtype = O, I, transposed, dtype
        self.code, self.tdt = nn._DT[dtype]
        g = torch.Generator(device="cuda").manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)
        self.means = 0.1 * r(O, I)
        self.lvars = float(np.log(1e-2)) + 0.6 * r(O, I)
        self.g_mu, self.g_lv = 1e-2 * r(O, I), 1e-2 * r(O, I)
        self.m_mu, self.m_lv = 1e-3 * r(O, I), 1e-3 * r(O, I)       # non-zero moments: a stray write to a frozen weight shows
        self.v_mu, self.v_lv = 1e-5 * r(O, I).abs() + 1e-7, 1e-5 * r(O, I).abs() + 1e-7
        self.bias, self.g_bias = 0.1 * r(O), 1e-2 * r(O)
        self.stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.log14 = torch.full((14,), -7.0, dtype=torch.float64, device="cuda")
        self.new_shadows()

    def new_shadows(self):
        L, nn = _mods()
        self.mu_s, self.var_s = nn._Packed(self.O, self.I, self.tdt, "cuda"), nn._Packed(self.O, self.I, self.tdt, "cuda")
        self.muT_s = nn._Packed(self.I, self.O, self.tdt, "cuda") if self.transposed else None
        self.varT_s = nn._Packed(self.I, self.O, self.tdt, "cuda") if self.transposed else None
        for p, (rows, cols) in ((self.mu_s, (self.O, self.I)), (self.var_s, (self.O, self.I)), (self.muT_s, (self.I, self.O)),
                                (self.varT_s, (self.I, self.O))):
            if p is not None:
                p.t[:rows, :cols] = 7.0                              # a sentinel: +0 has to be WRITTEN

    def clone(self):
        c = State.__new__(State)
        c.__dict__.update(self.__dict__)
        for k in FIELDS + ("g_mu", "g_lv", "bias", "g_bias", "stats", "log14"):
            setattr(c, k, getattr(self, k).clone())
        c.new_shadows()
        for k in ("mu_s", "var_s", "muT_s", "varT_s"):
            if getattr(self, k) is not None:
                getattr(c, k).t.copy_(getattr(self, k).t)
        return c

    def shadows(self):
        """The data regions of the shadows, the transposed ones turned back to O x I."""
        out = [self.mu_s.t[:, :self.I], self.var_s.t[:, :self.I]]
        if self.transposed:
            out += [self.muT_s.t[:, :self.O].t(), self.varT_s.t[:, :self.O].t()]
        return out

    def _masks(self, mask):
        if isinstance(mask, str):                                    # "nulls": an array whose only entry is NULL
            return (C.c_void_p * 1)()
        return None if mask is None else (C.c_void_p * 1)(mask.data_ptr())

    def prepare(self, mask=None, entry="masked"):
        L, nn = _mods()
        p = nn._p
        d = (L.PrepDesc * 1)(L.PrepDesc(means=p(self.means), lvars=p(self.lvars), O=self.O, I=self.I, mu_s=self.mu_s.ptr,
                                        var_s=self.var_s.ptr, ld_w=self.mu_s.ld, muT_s=self.muT_s.ptr if self.transposed else None,
                                        varT_s=self.varT_s.ptr if self.transposed else None,
                                        ld_wT=self.muT_s.ld if self.transposed else 0, stats=p(self.stats)))
        h = nn.Context.get().h
        if entry == "masked":
            L.check(L.lib().vbnn_prepare_masked(h, self.code, 1, d, self._masks(mask), None))
        else:
            assert mask is None
            L.check(L.lib().vbnn_prepare(h, self.code, 1, d, None))

    def update(self, t, mask=None, entry="masked", kl_add=1.0):
        L, nn = _mods()
        p = nn._p
        cfg = lambda lr: L.AdamCfg(lr=lr, t=t, **ADAM)
        d = (L.UpdateDesc * 1)(L.UpdateDesc(
            means=p(self.means), lvars=p(self.lvars), O=self.O, I=self.I, mu_s=self.mu_s.ptr, var_s=self.var_s.ptr, ld_w=self.mu_s.ld,
            muT_s=self.muT_s.ptr if self.transposed else None, varT_s=self.varT_s.ptr if self.transposed else None,
            ld_wT=self.muT_s.ld if self.transposed else 0, stats=p(self.stats), grad_mu=p(self.g_mu), grad_lv=p(self.g_lv),
            m_mu=p(self.m_mu), v_mu=p(self.v_mu), m_lv=p(self.m_lv), v_lv=p(self.v_lv), mu=cfg(1e-3), lv=cfg(5e-2),
            bias=p(self.bias), grad_bias=p(self.g_bias), lr_bias=1e-2, B=B_KL, log14=p(self.log14), kl_add=kl_add))
        h = nn.Context.get().h
        if entry == "masked":
            L.check(L.lib().vbnn_update_masked(h, self.code, 1, d, self._masks(mask), None))
        else:
            assert mask is None
            L.check(L.lib().vbnn_update(h, self.code, 1, d, None))


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b, where=None):
    a, b = _bits(a), _bits(b)
    return bool(torch.equal(a, b)) if where is None else bool(torch.equal(a[where], b[where]))


def _fp32_terms(means, lvars):
    """exp(lvars) + means^2 as the sweeps form it: the device's fp32 expf (read back from an f32 vbnn_prepare of the same
    parameters), the square and the sum rounded separately in fp32."""
    O, I = means.shape
    s = State(O, I, False, "f32")
    s.means, s.lvars = means.clone(), lvars.clone()
    s.prepare(None, entry="plain")
    v = s.var_s.t[:, :I].cpu().numpy()
    m = means.cpu().numpy()
    return (v + (m * m).astype(np.float32)).astype(np.float32), v


def _check_stats(stats, means, lvars, keep):
    st = stats.cpu().numpy()
    terms, _ = _fp32_terms(means, lvars)
    k = keep.cpu().numpy()
    n = int(k.sum())
    s0, s1 = terms[k].astype(np.float64).sum(), lvars.cpu().numpy()[k].astype(np.float64).sum()
    print(f"stats {st.tolist()} | numpy sums {s0!r} {s1!r} n_kept {n}")
    assert st[3] == n
    assert abs(st[0] - s0) <= 1e-10 * abs(s0) and abs(st[1] - s1) <= 1e-10 * abs(s1), (st, s0, s1)
    assert st[2] == st[0] / st[3]                                    # exactly: the prior variance of the network that exists


# ------------------------------------------------------------------------------------------------ 1. all-zero mask
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("O,I,transposed", SHAPES)
def test_all_zero_mask_is_the_unmasked_call_bitwise(O, I, transposed, dtype):
    a = State(O, I, transposed, dtype)
    b = a.clone()
    zero = _mask("zero", O, I)
    a.prepare(None, entry="plain")
    b.prepare(zero)
    torch.cuda.synchronize()
    for x, y in zip(a.shadows(), b.shadows()):
        assert _same(x, y)
    assert _same(a.stats, b.stats)
    for t in (1, 2):                                                 # two consecutive steps: the Adam state is carried
        a.update(t, None, entry="plain")
        b.update(t, zero)
        torch.cuda.synchronize()
        for k in FIELDS + ("bias", "stats", "log14"):
            assert _same(getattr(a, k), getattr(b, k)), (t, k)
        for x, y in zip(a.shadows(), b.shadows()):
            assert _same(x, y), t
        assert float(a.log14[0]) != -7.0
    # masks == NULL and an array of NULLs are the unmasked call as well
    c, d, e = a.clone(), a.clone(), a.clone()
    c.update(3, None, entry="plain")
    d.update(3, None, entry="masked")
    e.update(3, "nulls", entry="masked")
    torch.cuda.synchronize()
    for k in FIELDS + ("stats", "log14"):
        assert _same(getattr(c, k), getattr(d, k)) and _same(getattr(c, k), getattr(e, k)), k


# ------------------------------------------------------------------------------------------------ 2 - 4. kept, pruned, statistics
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("O,I,transposed", SHAPES)
def test_masked_sweeps_keep_prune_and_count(O, I, transposed, dtype, kind):
    mask = _mask(kind, O, I)
    pruned, keep = mask.bool(), ~mask.bool()
    assert 0 < int(pruned.sum()) < O * I
    a = State(O, I, transposed, dtype)
    orig = a.clone()

    # ---- vbnn_prepare_masked: kept shadows are vbnn_prepare's, pruned ones +0, the statistics are the kept weights'
    u = a.clone()
    u.prepare(None, entry="plain")
    a.prepare(mask)
    torch.cuda.synchronize()
    for x, y in zip(a.shadows(), u.shadows()):
        assert _same(x, y, keep)
        assert not bool(_bits(x)[pruned].any())                # the bit pattern of +0, both orientations
    _check_stats(a.stats, a.means, a.lvars, keep)
    for k in FIELDS:
        assert _same(getattr(a, k), getattr(orig, k)), k             # a prepare writes no parameter

    # ---- vbnn_update_masked against vbnn_update on copies, with the masked statistics and kl_add = 1
    b = a.clone()
    before = a.clone()
    a.update(1, mask)
    b.update(1, None, entry="plain")
    torch.cuda.synchronize()
    for k in FIELDS:                                                 # 2. kept weights: bit for bit, no tolerance
        assert _same(getattr(a, k), getattr(b, k), keep), k
        assert not _same(getattr(a, k), getattr(before, k), keep), k             # (and they did move)
        assert _same(getattr(a, k), getattr(before, k), pruned), k               # 3. pruned weights: frozen, moments included
    for x, y in zip(a.shadows(), b.shadows()):
        assert _same(x, y, keep)
        assert not bool(_bits(x)[pruned].any())
    assert _same(a.bias, b.bias)                                     # the bias step is untouched
    _check_stats(a.stats, a.means, a.lvars, keep)                    # 4. statistics of the NEW parameters

    # the 14 logged series over the kept weights (tolerances of test_update_leaves_what_prepare_would_and_logs_the_14_series)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    k_ = keep.cpu().numpy()
    mu0, lv0, gmu, glv = f64(before.means)[k_], f64(before.lvars)[k_], f64(before.g_mu)[k_], f64(before.g_lv)[k_]
    mu1, lv1 = f64(a.means)[k_], f64(a.lvars)[k_]
    vh = float(before.stats[2])
    mlc, vlc = mu0 / (B_KL * vh), (np.exp(lv0) / vh - 1.0) / (2 * B_KL)
    nl, nm, var1 = np.linalg.norm(lv1), np.linalg.norm(mu1), np.exp(lv1)
    want = [np.linalg.norm(vlc) / nl, np.linalg.norm(glv) / nl, np.linalg.norm(mlc) / nm, np.linalg.norm(gmu) / nm,
            var1.min(), var1.max(), var1.mean(), vh, mu1.mean(), mu1.std(ddof=1), mu1.min(), mu1.max(),
            np.linalg.norm(mu1 - mu0) / nm, np.linalg.norm(lv1 - lv0) / nl]
    np.testing.assert_allclose(f64(a.log14), want, rtol=2e-4, atol=1e-12)

    # vbnn_update_masked leaves what vbnn_prepare_masked would on the new parameters, bitwise
    p = a.clone()
    p.new_shadows()
    p.stats.zero_()
    p.prepare(mask)
    torch.cuda.synchronize()
    for x, y in zip(a.shadows(), p.shadows()):
        assert _same(x, y)
    assert _same(a.stats, p.stats), (a.stats.tolist(), p.stats.tolist())


def test_a_layer_without_a_kept_weight_gets_zero_statistics():
    a = State(70, 50, True, "f32")
    ones = torch.ones(70, 50, dtype=torch.uint8, device="cuda")
    a.stats.fill_(3.0)
    before = a.clone()
    a.prepare(ones)
    torch.cuda.synchronize()
    assert a.stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert all(not bool(_bits(x).any()) for x in a.shadows())
    a.stats.fill_(3.0)
    a.update(1, ones)
    torch.cuda.synchronize()
    assert a.stats.tolist() == [0.0, 0.0, 0.0, 0.0] and float(a.log14[0]) == -7.0       # nothing else is written
    for k in FIELDS:
        assert _same(getattr(a, k), getattr(before, k)), k


# ------------------------------------------------------------------------------------------------ 5. vbnn_calc_lc_masked
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("O,I,transposed", SHAPES)
def test_calc_lc_masked(O, I, transposed, kind):
    L, nn = _mods()
    p, h = nn._p, nn.Context.get().h
    mask = _mask(kind, O, I)
    pruned, keep = mask.bool(), ~mask.bool()
    a = State(O, I, transposed, "f32")
    a.prepare(mask)
    got, ref = torch.full((O, I), 5.0, device="cuda"), torch.full((O, I), 5.0, device="cuda")
    s_got, s_ref = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    L.check(L.lib().vbnn_calc_lc_masked(h, p(a.means), p(a.lvars), p(mask), p(a.stats), B_KL, p(got), p(s_got), O * I))
    L.check(L.lib().vbnn_calc_lc(h, p(a.means), p(a.lvars), None, None, p(a.stats), B_KL, p(ref), p(s_ref), O * I))
    torch.cuda.synchronize()
    assert _same(got, ref, keep)                                     # the same stats: the kept elements are vbnn_calc_lc's
    assert not bool(_bits(got)[pruned].any())
    want = float(ref[keep].double().sum())
    print(f"lc sum {float(s_got)!r}, float64 sum of the kept elements {want!r}")
    assert abs(float(s_got) - want) <= 1e-10 * abs(want)
    # mask == NULL: vbnn_calc_lc
    L.check(L.lib().vbnn_calc_lc_masked(h, p(a.means), p(a.lvars), None, p(a.stats), B_KL, p(got), p(s_got), O * I))
    torch.cuda.synchronize()
    assert _same(got, ref) and _same(s_got, s_ref)


# ------------------------------------------------------------------------------------------------ 6 - 7. the engine
STATES = dict(state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-4), varState=dict(learningRate=5e-2))


def _engine(dtype, **kw):
    from vbnn_amd.engine import FusedMLP
    opt = dict(var_init=1e-3, mu_init=1, B=1e4, S=1, mode="lrt", dtype=dtype, seed=3, input_size=256, hidden=[512, 256],
               n_classes=10, fuse_kl=True, kl_in_update=True, type="vb", **STATES)
    opt.update(kw)
    eng = FusedMLP(opt)
    for li, v in enumerate(eng.vb):                                  # sigma varies per weight: the keys are not the |means| alone
        v.lvars.add_(0.7 * torch.sin(torch.arange(v.lvars.numel(), device="cuda", dtype=torch.float32)).view_as(v.lvars))
    return opt, eng


def _batch(N=512, I0=256):
    L, nn = _mods()
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    return x, t


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_step_computes_the_pruned_network(dtype):
    x, t = _batch()
    opt, A = _engine(dtype)
    _, Bn = _engine(dtype)
    A.prepare()
    res = A.prune(fraction=0.7)
    with A.pruned(res):
        view = A.predict(x, targets=t, map=True)                     # the pruned network through the PruneResult view
        view_probs = view.probs.clone()
    masks = [res.mask(li) for li in range(len(A.vb))]
    counts = A.hold_pruned(res)
    assert counts == [int(m.sum()) for m in masks] and A.held == counts
    assert abs(sum(counts) / sum(v.O * v.I for v in A.vb) - 0.7) < 1e-3
    for v, w, m in zip(A.vb, Bn.vb, masks):                          # B: no mask, the pruned weights hand-set to nothing
        w.means[m] = 0.0
        w.lvars[m] = -200.0                                          # expf underflows to +0: B's shadows are A's
    Bn.prepare()
    torch.cuda.synchronize()
    for v, w in zip(A.vb, Bn.vb):
        assert _same(v.mu_s.t, w.mu_s.t) and _same(v.var_s.t, w.var_s.t)
    for e in (A, Bn):
        e.resetGradients(); e.sample(); e.run(x, t); e.finish()
    la, lb = A.loss_and_accuracy(), Bn.loss_and_accuracy()
    assert la == lb, (la, lb)
    for v, w, m in zip(A.vb, Bn.vb, masks):                          # kl_in_update: the arena holds the likelihood gradients
        assert _same(v.gradWeight, w.gradWeight, ~m) and _same(v.gradSum, w.gradSum, ~m)
        assert float(v.gradWeight[~m].abs().max()) > 0
    held = A.predict(x, targets=t, map=True)
    assert _same(held.probs, view_probs) and held.nll == view.nll


def test_engine_holds_grows_and_releases():
    from vbnn_amd.engine import FusedMLP
    x, t = _batch()
    opt, A = _engine("bf16")
    A.prepare()
    assert A.held is None
    counts = A.hold_pruned(A.prune(fraction=0.5))
    masks = [A.held_mask(li).clone() for li in range(len(A.vb))]
    frozen = [(v.means[m].clone(), v.lvars[m].clone()) for v, m in zip(A.vb, masks)]
    moving = [v.means[~m].clone() for v, m in zip(A.vb, masks)]
    lc0 = A.calc_lc()
    for _ in range(3):
        A.resetGradients(); A.sample(); A.run(x, t); A.update(opt)
        assert A.held == counts
    torch.cuda.synchronize()
    for v, m, (mu, lv), mv in zip(A.vb, masks, frozen, moving):
        assert _same(v.means[m], mu) and _same(v.lvars[m], lv)       # the held positions keep their parameter bits
        assert not _same(v.means[~m], mv)
        assert not bool(_bits(v.mu_s.t[:, :v.I])[m].any()) and not bool(_bits(v.var_s.t[:, :v.I])[m].any())
        assert float(v.stats[3]) == float((~m).sum())
    assert np.isfinite(lc0) and np.isfinite(A.calc_lc())
    # a second hold with a larger fraction: a superset (the masks are ORed)
    ptrs = [m.data_ptr() for m in A._held]
    counts2 = A.hold_pruned(A.prune(fraction=0.8))
    assert ptrs == [m.data_ptr() for m in A._held]                   # updated in place: a captured update's addresses stay valid
    for li, m in enumerate(masks):
        m2 = A.held_mask(li)
        assert bool((m2 | m).equal(m2)) and counts2[li] >= counts[li] and counts2[li] == int(m2.sum())
    assert sum(counts2) >= int(0.8 * sum(v.O * v.I for v in A.vb)) - 1
    # release: bitwise what an unheld engine's prepare() writes from the same parameters
    _, Cn = _engine("bf16")
    for v, w in zip(A.vb, Cn.vb):
        w.means.copy_(v.means); w.lvars.copy_(v.lvars); w.bias.copy_(v.bias)
    Cn.weight3.copy_(A.weight3); Cn.bias3.copy_(A.bias3)
    Cn.prepare()
    A.release_pruned()
    torch.cuda.synchronize()
    assert A.held is None
    for v, w in zip(A.vb, Cn.vb):
        assert _same(v.mu_s.t, w.mu_s.t) and _same(v.var_s.t, w.var_s.t) and _same(v.stats, w.stats)
        if v.muT_s is not None and getattr(v, "use_muT", True):
            assert _same(v.muT_s.t, w.muT_s.t) and _same(v.varT_s.t, w.varT_s.t)


def test_engine_refusals():
    from vbnn_amd.engine import FusedMLP
    opt, A = _engine("bf16")
    A.prepare()
    res = A.prune(fraction=0.5)
    with pytest.raises(RuntimeError, match="without a kept weight"):
        A.hold_pruned(A.prune(fraction=1.0, scope="layer"))
    assert A.held is None
    units = A.prune_units(fraction=0.25)
    A.hold_pruned(res)
    with pytest.raises(RuntimeError, match="parameters changed"):
        A.hold_pruned(res)                                           # the hold is a parameter-version change
    for what, call in (("prune_units", lambda: A.prune_units(fraction=0.5)), ("compact", lambda: A.compact(units)),
                       ("compress", lambda: A.prune(fraction=0.6).compress())):
        with pytest.raises(RuntimeError, match="mask is held"):
            call()
    with pytest.raises(ValueError):
        A.hold_pruned(None)
    # weight-noise mode and the sharded update
    _, Wn = _engine("f32", mode="wn", kl_in_update=False)
    Wn.prepare()
    with pytest.raises(RuntimeError, match="weight-noise"):
        Wn.hold_pruned(Wn.prune(fraction=0.5))
    _, Nk = _engine("f32", fuse_kl=False, kl_in_update=False)      # its parameters are stepped by the module-level update
    Nk.prepare()
    with pytest.raises(RuntimeError, match="fuse_kl"):
        Nk.hold_pruned(Nk.prune(fraction=0.5))
    sh_opt = dict(opt, exchange_mode="sharded")
    Sh = FusedMLP(sh_opt, force_reduce=True)
    Sh.prepare()
    with pytest.raises(RuntimeError, match="sharded"):
        Sh.hold_pruned(Sh.prune(fraction=0.5))


# ------------------------------------------------------------------------------------------------ 8. the C host
@pytest.mark.parametrize("dtype,I0,hidden,N", [("bf16", 256, [512, 256], 512), ("f32", 70, [50, 34], 37)])
def test_c_host_hold_means_are_bitwise_the_engines(tmp_path, dtype, I0, hidden, N):
    from tests import _children
    from tests.test_c_host import _read_arena, build
    from vbnn_amd.engine import FusedMLP
    L, nn = _mods()
    exe = build(tmp_path)
    out = str(tmp_path / "arena.bin")
    cmd = [exe, "--dtype", dtype, "--input", str(I0), "--hidden", ",".join(str(h) for h in hidden), "--classes", "10",
           "--batch", str(N), "--S", "1", "--steps", "2", "--update", "--hold", "0.5", "--out", out]
    res = _children.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    print(res.stdout.strip())
    assert "holding" in res.stdout
    n, loss_c, correct_c, flags, arena_c, rest = _read_arena(out)
    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype=dtype, seed=3, input_size=I0, hidden=hidden,
               n_classes=10, fuse_kl=True, **STATES)
    eng = FusedMLP(opt)
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    eng.prepare()
    eng.hold_pruned(eng.prune(fraction=0.5))
    start = [v.means.clone() for v in eng.vb]
    for step in range(2):
        eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
        if step == 0:
            eng.update(opt)
    loss_p, correct_p = eng.loss_and_accuracy()
    assert loss_c == loss_p and correct_c == correct_p, (loss_c, loss_p)
    assert _same(torch.from_numpy(arena_c.copy()), eng.grads.cpu())
    mu_p = np.concatenate([v.means.cpu().numpy().ravel() for v in eng.vb])
    assert np.array_equal(rest.view(np.uint32), mu_p.view(np.uint32)), "means after the masked update differ"
    for v, m0, li in zip(eng.vb, start, range(len(eng.vb))):
        m = eng.held_mask(li)
        assert _same(v.means[m], m0[m]) and not _same(v.means[~m], m0[~m])


# ------------------------------------------------------------------------------------------------ 9. recovery
def test_fine_tuning_under_the_held_mask_recovers_nll(tmp_path):
    """The README's accuracy recipe (784-64-48-10 f32, synthetic digits, 3 epochs). The first fraction of (0.95, 0.98, 0.99,
    0.995) whose pruned MAP accuracy is at least 10 points below the unpruned one is held for two epochs: the test-set NLL of
    the MAP prediction must then be strictly lower than right after pruning, the held count unchanged. (Seen on an MI355X:
    0.95 costs 5.8 points, 0.98 is chosen at 43.6 % against 100 %; NLL 2.0715 -> 1.5703 after the two epochs.)"""
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    opt = train.default_opt(network_name=str(tmp_path / "exp"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                            trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32", log=False,
                            state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
    m = train.Main(opt)
    m.run(trainSet, testSet, epochs=3)
    inputs, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
    x, t = m._to_device(inputs, targets)
    net = m.net
    base = net.predict(x, targets=t, map=True)
    chosen = None
    for q in (0.95, 0.98, 0.99, 0.995):
        res = net.prune(fraction=q)
        with net.pruned(res):
            p = net.predict(x, targets=t, map=True)
        print(f"pruned {q}: MAP accuracy {p.accuracy:.2f} % (unpruned {base.accuracy:.2f} %), NLL {p.nll:.4f} (unpruned {base.nll:.4f})")
        if p.accuracy <= base.accuracy - 10.0:
            chosen = (q, res, p)
            break
    assert chosen is not None, "no fraction costs 10 points of accuracy: nothing to recover"
    q, res, p = chosen
    counts = net.hold_pruned(res)
    held0 = net.predict(x, targets=t, map=True)
    assert held0.nll == p.nll                                        # the held network IS the pruned view
    for _ in range(2):
        m.train(trainSet)
    after = net.predict(x, targets=t, map=True)
    print(f"held {q} ({sum(counts)} weights): NLL {p.nll:.4f} -> {after.nll:.4f}, MAP accuracy {p.accuracy:.2f} -> {after.accuracy:.2f} %")
    assert net.held == counts
    assert after.nll < p.nll, (after.nll, p.nll)
