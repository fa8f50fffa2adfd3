"""The kernels that write parameters -- k_vb_update / k_update_finish (vbnn_update, vbnn_update_masked), k_adam / k_sgd
(vbnn_adam_step, vbnn_sgd_step) -- and the three device-side helpers of the sharded update (vbnn_transpose_packed,
vbnn_cast_grads, vbnn_stats_combine), through the C ABI, against the NumPy restatement of tests/_update_np.py (itself held to the
oracle and to a float64 form by test_update_ref.py).

What is compared how:
  bit for bit    everything without expf on its way: new means, m_mu, v_mu always; lvars, m_lv, v_lv when the gradients come in
                 as totals (kl_add = 0); mu_s (the independent bf16 rounding of the new means); both transposes against the
                 row-major shadows; the pad elements of all four shadows (a sentinel); the bias; the gradients (unchanged);
                 k_adam's x, m, v; k_sgd; the casts; the transposes; the combined statistics.
  E ulp          var_s against exp64 of the kernel's own new lvars, E = 2: the 1 ulp of expf in the HIP math API's accuracy
                 table plus 1 ulp for the reference's own rounding to float32. With kl_add = 1 the KL part of the lvars'
                 gradient holds expf as well: lvars, m_lv, v_lv must lie in the element-wise envelope of the restatement run
                 with exp moved down and up by E ulp, widened by one ulp.
  1e-10          double-accumulated sums (stats[0], stats[1], the norms, the series without expf in their terms): the project's
                 bound for a reordered double sum.
  4 x SERIES_DIST  the series with expf in their terms, against the restatement: four times the CPU-measured distance between
                 the float32 and the float64 restatement (tests/_update_np.py, re-measured by test_update_ref.py).
The largest shape (2112 x 4032, the tile loop and the capped FLAT grid) runs once per form: f32, t = 1, total gradients."""
import ctypes as C

import numpy as np
import pytest

from tests import _update_np as U

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_ULP = 2                # expf: 1 ulp (HIP math API accuracy table) + 1 ulp for the float32 rounding of the float64 reference
B_KL = 50.0
LR_MU, LR_LV, LR_BIAS = 1e-3, 5e-2, 1e-2
SENT = 7.0
STEPS = [(1, 1.0), (2, 1.0), (1000, 0.999)]
#         O, I, transposed shadows                    which path of k_vb_update / k_update_finish
SHAPES = [(1, 1, True), (5, 7, True), (70, 50, True),  # tile form, scalar loads, ragged tiles, transposes
          (128, 192, True),                            # tile form, vector loads, whole tiles, vector transposed stores
          (66, 68, True),                              # ld_wT & 3 decided by the padded pitch, ragged both ways
          (3, 8, False),                               # tile form without transposes (nb 1024 > O I)
          (96, 100, False),                            # FLAT; rows no multiple of 64 columns; 9600 % 1024 != 0: ragged last stride
          (256, 512, False),                           # FLAT, several whole strides
          (1280, 1280, True), (1536, 1536, False)]     # 400 / 576 partial rows: both arms of the finish kernel's two-in-flight walk
BIG = [(2112, 4032, True), (2112, 4032, False)]        # 2079 tiles > the 2048 cap: the tile loop; FLAT with the capped grid


def _mods():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, nn


def _ctx():
    L, nn = _mods()
    return L, L.lib(), nn.Context.get().h


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u(a):
    """The bit patterns of a float32 / float64 / bf16-as-uint16 NumPy array."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host(t):
    """A device tensor on the host; a bf16 tensor as its uint16 bit patterns."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.contiguous().cpu().numpy()


def _bitwise(name, got, want, show=None):
    bad = np.argwhere(_u(got) != _u(want))
    if bad.size:
        i = tuple(int(q) for q in bad[0])
        ctx = "" if show is None else " | inputs " + ", ".join(f"{k}={show[k][i]!r}" for k in show)
        raise AssertionError(f"{name}: {len(bad)} of {np.asarray(got).size} differ; first at {i}: got {got[i]!r} want {want[i]!r}{ctx}")


def _rel(name, got, want, tol):
    assert abs(got - want) <= tol * abs(want), f"{name}: got {got!r} want {want!r} relative {abs(got - want) / max(abs(want), 1e-300):.3e} > {tol:.1e}"


def _cfgs(t, lam):
    return U.adam_cfg(LR_MU, t, lambda_=lam), U.adam_cfg(LR_LV, t, lambda_=lam)


class Layer:
    """One layer's device tensors for direct ABI calls, made from a host state of _update_np.make_state. All four shadows,
    pads included, start as a sentinel; every pitch has at least one pad element."""

    def __init__(self, st, transposed, dtype):
        L, nn = _mods()
        self.O, self.I = st["means"].shape
        self.transposed, self.dtype = transposed, dtype
        self.code, self.tdt = nn._DT[dtype]
        self.t = {k: _dev(st[k]) for k in U.FIELDS + ("g_mu", "g_lv", "bias", "g_bias", "stats")}
        self.t["log14"] = torch.full((14,), -7.0, dtype=torch.float64, device="cuda")
        self.ld_w, self.ld_wT = L.pad_ld(self.I + 1), L.pad_ld(self.O + 1)
        full = lambda r, c: torch.full((r, c), SENT, dtype=self.tdt, device="cuda")
        self.t["mu_s"], self.t["var_s"] = full(self.O, self.ld_w), full(self.O, self.ld_w)
        if transposed:
            self.t["muT_s"], self.t["varT_s"] = full(self.I, self.ld_wT), full(self.I, self.ld_wT)

    def desc(self, t, lam, kl_add, rows=None, stats=None, bias=True, log14=True, transposed=None):
        L, _ = _mods()
        r0, nr = (0, self.O) if rows is None else rows
        s = lambda k: _p(self.t[k][r0:r0 + nr])
        tr = self.transposed if transposed is None else transposed
        cfg = lambda lr: L.AdamCfg(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, lambda_=lam, t=t)
        return L.UpdateDesc(
            means=s("means"), lvars=s("lvars"), O=nr, I=self.I, mu_s=s("mu_s"), var_s=s("var_s"), ld_w=self.ld_w,
            muT_s=_p(self.t["muT_s"]) if tr else None, varT_s=_p(self.t["varT_s"]) if tr else None, ld_wT=self.ld_wT if tr else 0,
            stats=_p(self.t["stats"] if stats is None else stats), grad_mu=s("g_mu"), grad_lv=s("g_lv"), m_mu=s("m_mu"),
            v_mu=s("v_mu"), m_lv=s("m_lv"), v_lv=s("v_lv"), mu=cfg(LR_MU), lv=cfg(LR_LV),
            bias=s("bias") if bias else None, grad_bias=s("g_bias") if bias else None, lr_bias=LR_BIAS, B=B_KL,
            log14=_p(self.t["log14"]) if log14 else None, kl_add=kl_add)

    def update(self, t, lam, kl_add, mask=None, **kw):
        L, lib, h = _ctx()
        d = (L.UpdateDesc * 1)(self.desc(t, lam, kl_add, **kw))
        if mask is None:
            L.check(lib.vbnn_update(h, self.code, 1, d, None))
        else:
            L.check(lib.vbnn_update_masked(h, self.code, 1, d, (C.c_void_p * 1)(mask.data_ptr()), None))
        torch.cuda.synchronize()

    def host(self):
        return {k: _host(v) for k, v in self.t.items()}


_F32_SENT = np.array([SENT], np.float32).view(np.uint32)[0]
_BF16_SENT = U.bf16_bits(np.array([SENT], np.float32))[0]


def _values(a):
    return U.bf16_to_f32(a) if a.dtype == np.uint16 else a


def device_exp(lvars):
    """The device's own float32 expf of `lvars`: var_s of an f32 vbnn_prepare (how a bf16 run's float32 variances are seen)."""
    L, lib, h = _ctx()
    lv = _dev(np.ascontiguousarray(lvars, np.float32).reshape(1, -1))
    n = lv.shape[1]
    mu = torch.zeros_like(lv)
    mu_s, var_s = torch.empty(1, n, device="cuda"), torch.empty(1, n, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    d = (L.PrepDesc * 1)(L.PrepDesc(means=_p(mu), lvars=_p(lv), O=1, I=n, mu_s=_p(mu_s), var_s=_p(var_s), ld_w=n, muT_s=None,
                                    varT_s=None, ld_wT=0, stats=_p(stats)))
    L.check(lib.vbnn_prepare(h, L.F32, 1, d, None))
    torch.cuda.synchronize()
    return var_s.cpu().numpy().reshape(np.shape(lvars))


def verify(pre, got, t, lam, kl_add, dtype, transposed, mask=None, bias=True, log14=True, tamper=None):
    """One layer after one vbnn_update against the restatement run on `pre` (the host copy of what the call was given)."""
    cm, cl = _cfgs(t, lam)
    O, I = pre["means"].shape
    ref = U.update_layer_f32(pre, cm, cl, B_KL, kl_add, mask)
    if tamper is not None:
        tamper(ref)
    keep = ref["keep"]
    show = {k: pre[k] for k in U.FIELDS + ("g_mu", "g_lv")}
    # ---- parameters and moments
    exact = U.FIELDS if kl_add == 0.0 else ("means", "m_mu", "v_mu")
    for k in exact:
        _bitwise(k, got[k], ref[k], show)
    if kl_add != 0.0:                                                # expf in the lvars' gradient: the envelope of E ulp, one ulp wider
        lo = U.update_layer_f32(pre, cm, cl, B_KL, kl_add, mask, exp=U.exp_shifted(-E_ULP))
        hi = U.update_layer_f32(pre, cm, cl, B_KL, kl_add, mask, exp=U.exp_shifted(+E_ULP))
        for k in ("lvars", "m_lv", "v_lv"):
            a = np.nextafter(np.minimum(lo[k], hi[k]), np.float32(-np.inf))
            b = np.nextafter(np.maximum(lo[k], hi[k]), np.float32(np.inf))
            out = np.argwhere(~((a <= got[k]) & (got[k] <= b)))
            assert out.size == 0, f"{k}: {len(out)} outside the expf envelope; first {tuple(out[0])}: {got[k][tuple(out[0])]!r} not in [{a[tuple(out[0])]!r}, {b[tuple(out[0])]!r}]"
            _bitwise(k + " (pruned: frozen)", got[k][~keep], pre[k][~keep])
    for k in ("g_mu", "g_lv"):
        _bitwise(k + " (unchanged)", got[k], pre[k])
    # ---- shadows: data, transposes, pads
    mu_s, var_s = got["mu_s"][:, :I], got["var_s"][:, :I]
    _bitwise("mu_s", mu_s, U.bf16_bits(ref["mu_s"]) if dtype == "bf16" else ref["mu_s"], show)
    r = U.exp32(got["lvars"])                                        # exp64 of the kernel's OWN new lvars, rounded
    vlo, vhi = U.step_ulps(r, -E_ULP), U.step_ulps(r, +E_ULP)
    if dtype == "bf16":
        vlo, vhi = U.bf16_round(vlo), U.bf16_round(vhi)
    vs = _values(var_s)
    out = np.argwhere(keep & ~((vlo <= vs) & (vs <= vhi)))
    assert out.size == 0, f"var_s: {len(out)} outside {E_ULP} ulp of exp; first {tuple(out[0])}: {vs[tuple(out[0])]!r} not in [{vlo[tuple(out[0])]!r}, {vhi[tuple(out[0])]!r}]"
    assert not _u(var_s)[~keep].any(), "var_s of a pruned weight is not +0"
    sent = _BF16_SENT if dtype == "bf16" else _F32_SENT
    for k in ("mu_s", "var_s"):
        assert (_u(got[k])[:, I:] == sent).all(), f"{k}: a pad element was written"
    if transposed:
        _bitwise("muT_s", got["muT_s"][:, :O], np.ascontiguousarray(mu_s.T))
        _bitwise("varT_s", got["varT_s"][:, :O], np.ascontiguousarray(var_s.T))
        for k in ("muT_s", "varT_s"):
            assert (_u(got[k])[:, O:] == sent).all(), f"{k}: a pad element was written"
    # ---- bias
    _bitwise("bias", got["bias"], U.sgd_f32(pre["bias"], pre["g_bias"], LR_BIAS) if bias else pre["bias"])
    # ---- statistics: the kernel's own float32 variances in the reference terms
    v32 = vs if dtype == "f32" else device_exp(got["lvars"])
    terms = U.prior_terms(got["means"], v32)
    n = int(keep.sum())
    s0, s1 = float(terms[keep].astype(np.float64).sum()), float(got["lvars"][keep].astype(np.float64).sum())
    st = got["stats"]
    print(f"stats {st.tolist()} | float64 sums {s0!r} {s1!r} n {n}")
    _rel("stats[0]", st[0], s0, 1e-10)
    _rel("stats[1]", st[1], s1, 1e-10)
    assert st[3] == n
    want2 = (1.0 / n) * st[0] if n == O * I else st[0] / n
    assert abs(st[2] - want2) <= np.spacing(want2), (st[2], want2)
    # ---- the 14 series
    if not log14:
        assert (got["log14"] == -7.0).all()
        return ref
    plain = U.series_without_exp(kl_add)
    for k in range(14):
        tol = 1e-10 if k in plain else float(U.SERIES_TOL[k])
        print(f"series {k:2d}: {got['log14'][k]!r} | restatement {ref['log14'][k]!r} | allowed {tol:.1e} relative")
    for k in range(14):
        _rel(f"series {k}", got["log14"][k], ref["log14"][k], 1e-10 if k in plain else float(U.SERIES_TOL[k]))
    return ref


# ------------------------------------------------------------------------------------------------ the device's expf
def test_device_expf_is_within_the_documented_ulp():
    """Measured once: f32 vbnn_prepare over lvars covering [-20, 5] against float64 exp, in ulp of the float32 result. The
    allowance E_ULP is NOT taken from this figure: it is the documented 1 ulp + 1. (Seen on an MI355X: see LAB_NOTES.md.)"""
    r = np.random.RandomState(1)
    l = np.concatenate([np.linspace(-20.0, 5.0, 1 << 18), r.uniform(-20.0, 5.0, 1 << 18)]).astype(np.float32)
    got = device_exp(l).astype(np.float64)
    exact = np.exp(l.astype(np.float64))
    ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)
    err = np.abs(got - exact) / ulp
    i = int(np.argmax(err))
    print(f"device expf over [-20, 5], {l.size} arguments: worst error {err[i]:.4f} ulp at l = {l[i]!r}; mean {err.mean():.4f} ulp; "
          f"{int((got.astype(np.float32) != exact.astype(np.float32)).sum())} results differ from the rounded float64 exp")
    assert err[i] <= E_ULP - 1


# ------------------------------------------------------------------------------------------------ vbnn_update, one layer
CASES = [(s, dt, kl, st) for s in SHAPES for kl in (0.0, 1.0) for st in STEPS for dt in ("f32", "bf16")] + \
        [(s, "f32", 0.0, STEPS[0]) for s in BIG]


def _id(c):
    (O, I, tr), dt, kl, (t, lam) = c
    return f"{O}x{I}{'T' if tr else 'F'}-{dt}-kl{int(kl)}-t{t}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_update_matches_the_restatement(case):
    (O, I, transposed), dtype, kl_add, (t, lam) = case
    pre = U.make_state(O, I, zero_moments=(t <= 2))
    if t == 2:                                                       # t = 2 carries what t = 1 left: moments, parameters, statistics
        first = Layer(pre, transposed, dtype)                        # (that step has its own case; here it only makes the state)
        first.update(1, 1.0, kl_add)
        got = first.host()
        pre = dict(pre, **{k: got[k] for k in U.FIELDS + ("bias", "stats")})
    lay = Layer(pre, transposed, dtype)
    lay.update(t, lam, kl_add)
    verify(pre, lay.host(), t, lam, kl_add, dtype, transposed)


def test_a_wrong_expectation_for_one_flat_element_fails():
    """The comparison bites: one element of the FLAT form's ragged last stride expected one ulp off, and verify() refuses."""
    O, I = 96, 100
    pre = U.make_state(O, I)
    lay = Layer(pre, False, "f32")
    lay.update(2, 1.0, 0.0)
    got = lay.host()
    verify(pre, got, 2, 1.0, 0.0, "f32", False)

    def tamper(ref):
        ref["means"][O - 1, I - 1] = np.nextafter(ref["means"][O - 1, I - 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"means: 1 of 9600 differ; first at \(95, 99\)"):
        verify(pre, got, 2, 1.0, 0.0, "f32", False, tamper=tamper)


# ------------------------------------------------------------------------------------------------ several layers and `extra`
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_layers_and_the_final_weight_in_one_call(dtype):
    L, lib, h = _ctx()
    _, nn = _mods()
    forms = [(70, 50, True), (128, 192, True), (256, 512, False)]   # scalar tiles, vector tiles, FLAT
    opts = [dict(bias=True, log14=True), dict(bias=False, log14=True), dict(bias=True, log14=False)]
    t, lam, kl_add = 2, 1.0, 1.0
    pres = [U.make_state(O, I, seed=20 + i) for i, (O, I, _) in enumerate(forms)]
    lays = [Layer(p, tr, dtype) for p, (_, _, tr) in zip(pres, forms)]
    rows, cols = 10, 300                                             # 3000 elements: three packing blocks share the bias steps
    w3 = (0.1 * np.random.RandomState(30).standard_normal((rows, cols + 4))).astype(np.float32)
    code, tdt = nn._DT[dtype]
    src = _dev(w3)
    dst = torch.full((rows, L.pad_ld(cols + 1)), SENT, dtype=tdt, device="cuda")
    dstT = torch.full((cols, L.pad_ld(rows + 1)), SENT, dtype=tdt, device="cuda")
    extra = L.PackDesc(src=_p(src), rows=rows, cols=cols, ld_src=cols + 4, dst=_p(dst), ld_dst=dst.shape[1], dstT=_p(dstT),
                       ld_dstT=dstT.shape[1])
    d = (L.UpdateDesc * 3)(*[lay.desc(t, lam, kl_add, **o) for lay, o in zip(lays, opts)])
    L.check(lib.vbnn_update(h, code, 3, d, C.byref(extra)))
    torch.cuda.synchronize()
    for lay, pre, (_, _, tr), o in zip(lays, pres, forms, opts):
        verify(pre, lay.host(), t, lam, kl_add, dtype, tr, **o)
    want = U.bf16_bits(w3[:, :cols]) if dtype == "bf16" else w3[:, :cols]
    sent = _BF16_SENT if dtype == "bf16" else _F32_SENT
    a, b = _host(dst), _host(dstT)
    _bitwise("packed final weight", a[:, :cols], want)
    _bitwise("packed final weight, transposed", b[:, :rows], np.ascontiguousarray(want.T))
    assert (_u(a)[:, cols:] == sent).all() and (_u(b)[:, rows:] == sent).all()
    _bitwise("source of the pack", _host(src), w3)


# ------------------------------------------------------------------------------------------------ a row slice
@pytest.mark.parametrize("kl_add", [0.0, 1.0])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("O,I,r0,nr", [(70, 50, 35, 18), (70, 50, 0, 35), (256, 512, 64, 64), (256, 512, 192, 64)])
def test_a_row_slice_by_offset_pointers(O, I, r0, nr, dtype, kl_add):
    """As the sharded update calls it: rows [r0, r0 + nr) by offset pointers, no transposed shadows, no bias, no series, and
    the WHOLE layer's var_hat in `stats` on entry."""
    t, lam = 2, 1.0
    pre = U.make_state(O, I)
    lay = Layer(pre, False, dtype)
    stats = _dev(pre["stats"].copy())
    lay.update(t, lam, kl_add, rows=(r0, nr), stats=stats, bias=False, log14=False)
    got = lay.host()
    got["stats"] = _host(stats)
    rows = slice(r0, r0 + nr)
    cut = lambda d: {k: (v[rows] if k in U.FIELDS + ("g_mu", "g_lv", "mu_s", "var_s") else v) for k, v in d.items()}
    ref = verify(cut(pre), cut(got), t, lam, kl_add, dtype, False, bias=False, log14=False)
    whole = U.update_layer_f32(pre, *_cfgs(t, lam), B_KL, kl_add)   # the same rows of the whole-layer reference
    outside = np.ones(O, bool)
    outside[rows] = False
    sent = _BF16_SENT if dtype == "bf16" else _F32_SENT
    for k in U.FIELDS:
        _bitwise(k + " (slice of the whole layer's reference)", ref[k], whole[k][rows])
        _bitwise(k + " (rows outside the slice)", got[k][outside], pre[k][outside])
    for k in ("mu_s", "var_s"):
        assert (_u(got[k])[outside] == sent).all(), k
    assert got["stats"][3] == nr * I and got["stats"][0] != pre["stats"][0]


# ------------------------------------------------------------------------------------------------ under a held mask
def _mask(kind, O, I):
    if kind == "half":
        return (np.random.RandomState(11).rand(O, I) < 0.5).astype(np.uint8)
    m = np.zeros((O, I), np.uint8)                                   # "groups": 0 .. 3 weights of a group of four, at rotating places
    r, g4 = np.meshgrid(np.arange(O), np.arange(I // 4), indexing="ij")
    for j in range(3):
        on = ((r + g4) % 4) > j
        m[r[on], 4 * g4[on] + (r[on] + j) % 4] = 1
    m[:, I - 1] = 1                                                  # and the last (ragged) column
    return m


@pytest.mark.parametrize("kl_add", [0.0, 1.0])
@pytest.mark.parametrize("kind", ["half", "groups"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("O,I,transposed", [(70, 50, True), (256, 512, False)])
def test_masked_update_matches_the_masked_restatement(O, I, transposed, dtype, kind, kl_add):
    """vbnn_update_masked against update_layer_f32(mask=...): kept weights, frozen weights (parameters AND moments keep their
    bits), +0 shadows, the kept-count statistics and the series of the kept weights."""
    mask = _mask(kind, O, I)
    assert 0 < mask.sum() < O * I
    pre = U.make_state(O, I)
    pre["stats"] = U.prior_stats(pre["means"], pre["lvars"], keep=mask == 0)
    t, lam = 2, 1.0
    lay = Layer(pre, transposed, dtype)
    lay.update(t, lam, kl_add, mask=_dev(mask))
    got = lay.host()
    ref = verify(pre, got, t, lam, kl_add, dtype, transposed, mask=mask)
    pruned = mask != 0
    for k in U.FIELDS:
        _bitwise(k + " (pruned: frozen)", got[k][pruned], pre[k][pruned])
        assert (_u(got[k])[~pruned] != _u(pre[k])[~pruned]).any(), k
    assert not _u(got["mu_s"][:, :I])[pruned].any() and not _u(got["var_s"][:, :I])[pruned].any()
    assert got["stats"][3] == (~pruned).sum() == ref["stats"][3]


# ------------------------------------------------------------------------------------------------ vbnn_adam_step / vbnn_sgd_step
ADAM_N = [1, 3, 4, 5, 1023, 1024, 1025, 4194311]                    # the last: above the 2048-block cap, a tail of three


def _adam_inputs(n, seed=3):
    r = np.random.RandomState(seed)
    f = lambda s: (s * r.standard_normal(n)).astype(np.float32)
    x, g, g2, m = f(0.1), f(1e-2), f(1e-3), f(1e-3)
    v = (1e-5 * np.abs(r.standard_normal(n)) + 1e-7).astype(np.float32)
    if n >= 64:
        g[::17], g2[::17] = 0.0, 0.0                                 # exact-zero gradients
        g[5::19], g[6::19] = 1e-25, -1e-25                           # gradients whose square underflows
        g2[5::19], g2[6::19] = 0.0, 0.0
        m[::23], v[::23] = 0.0, 0.0                                  # zero moments
    return x, g, g2, m, v


def _adam_case(n, grad2, norms, t, lam, offset=0):
    L, lib, h = _ctx()
    x, g, g2, m, v = _adam_inputs(n)
    buf = torch.zeros(n + 4, device="cuda")                          # offset 1: x starts one float past a 16-byte boundary
    dx = buf[offset:offset + n]
    dx.copy_(_dev(x))
    dg, dg2, dm, dv = _dev(g), _dev(g2), _dev(m), _dev(v)
    nd = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    cfg = U.adam_cfg(LR_MU, t, lambda_=lam)
    L.check(lib.vbnn_adam_step(h, _p(dx), _p(dg), _p(dg2) if grad2 else None, _p(dm), _p(dv), n, LR_MU, 0.9, 0.999, 1e-8, lam, t,
                               _p(nd) if norms else None))
    torch.cuda.synchronize()
    x2, m2, v2, up = U.adam_f32(x, g, g2 if grad2 else None, m, v, cfg)
    show = dict(x=x, g=g, g2=g2, m=m, v=v)
    _bitwise("x", _host(dx), x2, show)
    _bitwise("m", _host(dm), m2, show)
    _bitwise("v", _host(dv), v2, show)
    _bitwise("grad (unchanged)", _host(dg), g)
    hb = _host(buf)
    assert not hb[:offset].any() and not hb[offset + n:].any()       # nothing written outside x
    if norms:
        want = U.adam_norms(up, x2)
        got = _host(nd)
        _rel("|update|", got[0], want[0], 1e-10)
        _rel("|x|", got[1], want[1], 1e-10)
    else:
        assert (_host(nd) == -7.0).all()


@pytest.mark.parametrize("norms", [False, True])
@pytest.mark.parametrize("grad2", [False, True])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step_is_the_restatement_bit_for_bit(n, grad2, norms):
    for t, lam in (STEPS if n <= 1025 else STEPS[2:]):
        _adam_case(n, grad2, norms, t, lam)


def test_adam_step_on_a_view_offset_by_one_float():
    """x one float past a 16-byte boundary: the documented scalar path of k_adam."""
    for n in (5, 1025):
        for grad2 in (False, True):
            _adam_case(n, grad2, True, 1000, 0.999, offset=1)


@pytest.mark.parametrize("n", ADAM_N)
def test_sgd_step_is_the_restatement_bit_for_bit(n):
    L, lib, h = _ctx()
    x, g, _, _, _ = _adam_inputs(n, seed=4)
    dx, dg = _dev(x), _dev(g)
    L.check(lib.vbnn_sgd_step(h, _p(dx), _p(dg), n, LR_BIAS))
    torch.cuda.synchronize()
    _bitwise("x", _host(dx), U.sgd_f32(x, g, LR_BIAS), dict(x=x, g=g))
    _bitwise("grad (unchanged)", _host(dg), g)


# ------------------------------------------------------------------------------------------------ the sharded update's helpers
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (64, 64), (65, 63), (130, 200)])
def test_transpose_packed(rows, cols, dtype):
    L, lib, h = _ctx()
    _, nn = _mods()
    code, tdt = nn._DT[dtype]
    ld_src, ld_dst = L.pad_ld(cols + 1), L.pad_ld(rows + 1)
    src = torch.from_numpy(np.random.RandomState(rows).standard_normal((rows, ld_src)).astype(np.float32)).cuda().to(tdt)
    dst = torch.full((cols, ld_dst), SENT, dtype=tdt, device="cuda")
    L.check(lib.vbnn_transpose_packed(h, code, _p(src), ld_src, rows, cols, _p(dst), ld_dst))
    torch.cuda.synchronize()
    a, b = _host(src), _host(dst)
    _bitwise("transpose", b[:, :rows], np.ascontiguousarray(a[:, :cols].T))
    assert (_u(b)[:, rows:] == (_BF16_SENT if dtype == "bf16" else _F32_SENT)).all()


CAST_N = [1, 7, 8, 9, 2047, 2048, 2049]
_SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF,
                     0x00008000, 0x3F808000, 0x3F818000, 0xBF808000, 0x3F808001, 0x3F807FFF, 0x7F7F8000, 0x7FA00001],
                    np.uint32)   # +-0, +-inf, NaNs, the largest finite, denormals, exact ties (to even: down, up), around a tie, a tie into inf


def _cast_input(n):
    r = np.random.RandomState(n)
    x = _u(r.standard_normal(n).astype(np.float32) * np.float32(10.0) ** r.randint(-30, 30, n).astype(np.float32)).copy()
    k = np.roll(_SPECIAL, n)[:n]                                     # (rolled: the small sizes see different ones)
    x[:k.size] = k
    return x.view(np.float32)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", CAST_N)
def test_cast_grads_both_ways(n, offset):
    """offset 1: source and destination views start one element in (no 16-byte alignment: the scalar path)."""
    L, lib, h = _ctx()
    x = _cast_input(n)
    src = torch.zeros(n + 8, device="cuda")
    src[offset:offset + n].copy_(_dev(x))
    half = torch.full((n + 8,), SENT, dtype=torch.bfloat16, device="cuda")
    L.check(lib.vbnn_cast_grads(h, 1, _p(src[offset:]), _p(half[offset:]), n))
    torch.cuda.synchronize()
    hb = _host(half)
    got, want = hb[offset:offset + n], U.bf16_bits(x)
    nan = np.isnan(x)
    _bitwise("to bf16", got[~nan], want[~nan], dict(x=x[~nan]))
    assert np.isnan(U.bf16_to_f32(got[nan])).all(), "a NaN did not stay a NaN"
    assert (hb[:offset] == _BF16_SENT).all() and (hb[offset + n:] == _BF16_SENT).all()
    # back: widening is exact
    wide = torch.full((n + 8,), SENT, device="cuda")
    L.check(lib.vbnn_cast_grads(h, 0, _p(half[offset:]), _p(wide[offset:]), n))
    torch.cuda.synchronize()
    hw = _host(wide)
    back = hw[offset:offset + n]
    gn = np.isnan(U.bf16_to_f32(got))
    _bitwise("to f32", back[~gn], U.bf16_to_f32(got)[~gn])
    assert np.isnan(back[gn]).all()
    assert (_u(hw[:offset]) == _F32_SENT).all() and (_u(hw[offset + n:]) == _F32_SENT).all()
    # bf16 -> f32 -> bf16 is the identity
    again = torch.full((n + 8,), SENT, dtype=torch.bfloat16, device="cuda")
    L.check(lib.vbnn_cast_grads(h, 1, _p(wide[offset:]), _p(again[offset:]), n))
    torch.cuda.synchronize()
    ha = _host(again)[offset:offset + n]
    _bitwise("round trip", ha[~gn], got[~gn])
    assert np.isnan(U.bf16_to_f32(ha[gn])).all()


@pytest.mark.parametrize("n_layers", [1, 8])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_stats_combine(world, n_layers):
    L, lib, h = _ctx()
    r = np.random.RandomState(world * 10 + n_layers)
    parts = np.empty((world, n_layers, 4))
    parts[..., 0] = r.uniform(1.0, 3.0, (world, n_layers)) * 1e3
    parts[..., 1] = -r.uniform(1.0, 3.0, (world, n_layers)) * 1e4
    parts[..., 2] = 123.0                                            # the slices' own var_hat: not read
    parts[..., 3] = r.randint(1, 5000, (world, n_layers))
    dparts = _dev(parts)
    stats = [torch.full((4,), -7.0, dtype=torch.float64, device="cuda") for _ in range(n_layers)]
    ptrs = (C.c_void_p * n_layers)(*[s.data_ptr() for s in stats])
    L.check(lib.vbnn_stats_combine(h, n_layers, world, _p(dparts), ptrs))
    torch.cuda.synchronize()
    for l in range(n_layers):
        s0 = s1 = w = 0.0
        for k in range(world):                                       # sums in rank order
            s0, s1, w = s0 + parts[k, l, 0], s1 + parts[k, l, 1], w + parts[k, l, 3]
        _bitwise(f"layer {l}", _host(stats[l]), np.array([s0, s1, (1.0 / w) * s0, w]))
    _bitwise("parts (unchanged)", _host(dparts), parts)
