"""The first half of elementwise.hip through the C ABI -- vbnn_fill_normal / _hw, vbnn_wn_sample, vbnn_pack, vbnn_pack_input,
vbnn_compute_prior, vbnn_prep_layer, vbnn_prepare, vbnn_calc_lc, vbnn_compute_mugrads, vbnn_compute_vargrads -- against the NumPy
reference of tests/_sweeps_np.py (itself held to the oracle and to its float64 definitions by test_sweeps_ref.py). That module's
docstring says which outputs are compared bit for bit and derives every bound used here; none is fitted to the device.

Common rules: every output buffer starts as a sentinel and has one row (or a few elements) behind its last; every packed pitch
is pad_ld(cols + 1), so a whole pad block exists; pads and what lies behind the last row must still hold the sentinel afterwards;
every element is compared. Packed outputs keep the header's convention (pitches multiples of VBNN_KPAD, bases as allocated); odd
pitches and pointers offset by one float go ONLY to the arguments whose alignment the kernels test and fall back on.

Each test prints the largest fraction of a bound the device used; the module writes them, with its wall time, to
sweeps_bounds.txt in the results directory of the tools/ scripts (OUT_DIR, by default bench_out/; committed from an MI355X as
profiles/sweeps_bounds.txt)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests import _sweeps_np as R
from tests._sweeps_np import F, f8

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT = 7.0
SEED = 20240229
_F32_SENT = np.array([SENT], np.float32).view(np.uint32)[0]
_BF16_SENT = R.bf16_bits(np.array([SENT], np.float32))[0]
USED = {}


# ------------------------------------------------------------------------------------------------ plumbing
def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, L.lib(), nn.Context.get().h


def _dt(dtype):
    from vbnn_amd import nn
    return nn._DT[dtype]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.contiguous().cpu().numpy()


def _sent(a):
    return _BF16_SENT if a.dtype == np.uint16 else _F32_SENT


def _use(name, frac):
    frac = float(frac)
    USED[name] = max(USED.get(name, 0.0), frac)
    print(f"bound used: {name} {frac:.4f}")


SEEN = []


@pytest.fixture(autouse=True)
def _count(request):
    SEEN.append(request.node.name)


@pytest.fixture(scope="module", autouse=True)
def _record_bounds():
    t0 = time.time()
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.abspath(os.environ.get("OUT_DIR") or os.path.join(root, "bench_out"))     # as tools/collect_traffic.py
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "sweeps_bounds.txt"), "w") as f:
        f.write(f"tests/test_sweeps_gpu.py on one MI355X: {len(SEEN)} tests, {time.time() - t0:.1f} s wall for the file.\n"
                "Per bounded output, the largest fraction of its bound the device used (1 = the bound; bounds derived in\n"
                "tests/_sweeps_np.py; *_ulp: of the E_ULP = 2 ulp allowed to expf; *_1e-10: of the reordered double sum's 1e-10).\n"
                "Outputs not listed were compared bit for bit.\n"
                f"CPU, tests/test_sweeps_ref.py: fraction of each bound the fp32 restatement (correctly rounded exp / log) uses: {R.BOUND_USED}\n")
        for k in sorted(USED):
            f.write(f"  {k:36s} {USED[k]:.4f}\n")


def _same(name, got, want):
    """Every element, bit for bit; a NaN must be a NaN (its payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    g, w = R.values(got), R.values(want)
    ok = np.where(np.isnan(w), np.isnan(g), _u(got) == _u(want))
    bad = np.argwhere(~ok)
    if bad.size:
        i = tuple(int(q) for q in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} differ; first at {i}: got {g[i]!r} ({_u(got)[i]:#x}) want {w[i]!r} ({_u(want)[i]:#x})")


def _inside(name, got, lo, hi):
    out = np.argwhere(~((lo <= got) & (got <= hi)))
    assert out.size == 0, f"{name}: {len(out)} of {got.size} outside; first {tuple(out[0])}: {got[tuple(out[0])]!r} not in [{lo[tuple(out[0])]!r}, {hi[tuple(out[0])]!r}]"


def _all_ok(name, ok, got):
    out = np.argwhere(~ok)
    assert out.size == 0, f"{name}: {len(out)} of {ok.size} outside the bound; first {tuple(out[0])}: {got[tuple(out[0])]!r}"


class Mat:
    """rows x ld of T (+ one row behind), all sentinel: a packed output."""

    def __init__(self, rows, cols, ld, dtype):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.t = torch.full((rows + 1, ld), SENT, dtype=_dt(dtype)[1], device="cuda")

    @property
    def p(self):
        return _p(self.t)

    def data(self, name):
        """The rows x cols block as stored, after checking that pads and the row behind still hold the sentinel."""
        h = _host(self.t)
        assert (_u(h)[:self.rows, self.cols:] == _sent(h)).all(), f"{name}: a pad element was written"
        assert (_u(h)[self.rows:] == _sent(h)).all(), f"{name}: written behind the last row"
        return np.ascontiguousarray(h[:self.rows, :self.cols])


class Vec:
    """n floats at `offset` floats into a sentinel buffer with 8 spare elements: a flat float32 output (or, filled, an input)."""

    def __init__(self, n, offset=0, fill=None):
        self.n, self.off = n, offset
        self.buf = torch.full((n + 8,), SENT, dtype=torch.float32, device="cuda")
        self.v = self.buf[offset:offset + n]
        if fill is not None:
            self.v.copy_(_dev(np.ascontiguousarray(fill, np.float32).reshape(-1)))

    @property
    def p(self):
        return _p(self.v)

    def data(self, name):
        h = _host(self.buf)
        assert (_u(h[:self.off]) == _F32_SENT).all() and (_u(h[self.off + self.n:]) == _F32_SENT).all(), f"{name}: written outside"
        return h[self.off:self.off + self.n].copy()


def _stats_buf():
    return torch.full((5,), -7.0, dtype=torch.float64, device="cuda")


def _stats(t, name="stats"):
    h = _host(t)
    assert h[4] == -7.0, f"{name}: written behind the fourth statistic"
    return h[:4]


def _r4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ fill_normal
FILL = [(1, 1, "odd", 0), (3, 7, "odd", 0), (33, 130, "odd", 0),                 # ld = cols + 3: scalar stores
        (1, 1, "even", 1), (3, 7, "even", 1), (33, 130, "even", 1),              # pointer one float past 16 bytes: scalar stores
        (5, 64, 68, 0)]                                                          # vector stores, a pad of four


def _fill_case(rows, cols, ld, off, scale, hw, row0, stream=2, layer=2, draw=7):
    L, lib, h = _ctx()
    ld = cols + 3 if ld == "odd" else (_r4(cols) + 4 if ld == "even" else ld)
    n = (rows + 1) * ld
    out = Vec(n, off)
    fn = lib.vbnn_fill_normal_hw if hw else lib.vbnn_fill_normal
    L.check(fn(h, out.p, rows, cols, ld, SEED, stream, layer, draw, row0, scale))
    torch.cuda.synchronize()
    a = out.data("fill_normal").reshape(rows + 1, ld)
    assert (_u(a)[:rows, cols:] == _F32_SENT).all() and (_u(a)[rows:] == _F32_SENT).all(), "a pad element was written"
    got = np.ascontiguousarray(a[:rows, :cols])
    if not hw:
        _same("fill_normal", got, R.fill_normal_f32(rows, cols, SEED, stream, layer, draw, row0, scale))
        return
    z = R.fill_normal_f64(rows, cols, SEED, stream, layer, draw, row0, scale)
    frac = np.abs(got.astype(f8) - z) / R.fill_normal_hw_bound(z, scale)
    _use("fill_normal_hw", frac.max())
    _all_ok("fill_normal_hw", frac <= 1.0, got)


@pytest.mark.parametrize("hw", [False, True], ids=["contract", "hw"])
@pytest.mark.parametrize("scale", [1.0, 0.05])
@pytest.mark.parametrize("rows,cols,ld,off", FILL)
def test_fill_normal(rows, cols, ld, off, scale, hw):
    _fill_case(rows, cols, ld, off, scale, hw, 1000)


def test_fill_normal_beyond_one_grid_stride():
    """2100 x 1000: 525 000 quads against 2048 x 256 threads."""
    _fill_case(2100, 1000, 1000, 0, 0.05, False, 0)


@pytest.mark.parametrize("hw", [False, True], ids=["contract", "hw"])
def test_fill_normal_row_counter_wraps_at_2_32(hw):
    """row0 = 2^32 - 16: the counter's row word is (uint32)(row0 + r), rows 16.. wrap to 0.."""
    _fill_case(33, 130, "odd", 0, 1.0, hw, (1 << 32) - 16)


# ------------------------------------------------------------------------------------------------ wn_sample
def _wn_case(O, I, route, e_given, off, kind="trained", layer=3, draw=11):
    L, lib, h = _ctx()
    W = O * I
    means, lvars = R.param_set(kind, W)
    stdv = np.sqrt(R.exp32(lvars)) if route == "stdv" else None
    dm, dl = Vec(W, off, means), Vec(W, off, lvars)
    ds = Vec(W, off, stdv) if stdv is not None else None
    w, e = Vec(W, off), (Vec(W, off) if e_given else None)
    L.check(lib.vbnn_wn_sample(h, dm.p, ds.p if ds else None, dl.p if route == "lvars" else None, w.p, e.p if e else None, O, I,
                               SEED, layer, draw))
    torch.cuda.synchronize()
    eps = R.wn_eps(O, I, SEED, layer, draw).reshape(-1)
    got = w.data("weight")
    if e:
        _same("e_out", e.data("e_out"), eps)
    if route == "stdv":
        _same("weight", got, R.wn_sample_f32(means, stdv, None, eps))
    else:
        lo, hi = R.envelope(lambda exp: R.wn_sample_f32(means, None, lvars, eps, exp=exp))
        _inside("weight (lvars route)", got, lo, hi)
    _same("means (unchanged)", dm.data("means"), means)


@pytest.mark.parametrize("e_given", [False, True], ids=["noe", "e"])
@pytest.mark.parametrize("route", ["stdv", "lvars"])
@pytest.mark.parametrize("O,I", [(1, 1), (5, 7), (48, 64), (3, 130)])
def test_wn_sample(O, I, route, e_given):
    for kind in R.PARAM_SETS:
        _wn_case(O, I, route, e_given, 0, kind)


@pytest.mark.parametrize("route", ["stdv", "lvars"])
def test_wn_sample_pointers_offset_by_one_float(route):
    _wn_case(48, 64, route, True, 1)


def test_wn_sample_beyond_one_grid_stride():
    """520 x 4100: 533 000 quads against 2048 x 256 threads; the route the engine takes (lvars only, no e_out)."""
    _wn_case(520, 4100, "lvars", False, 0)
    _wn_case(520, 4100, "stdv", True, 0)


# ------------------------------------------------------------------------------------------------ pack
FUNCS = {"copy": R.COPY, "exp": R.EXP, "square": R.SQUARE, "mul": R.MUL, "relu": R.RELU, "relu_square": R.RELU_SQUARE}


def _check_packed(name, got, func, a, b, dtype):
    """got: rows x cols as stored."""
    if func == R.EXP:
        fin = np.isfinite(a)
        gv = R.values(got)
        ok = np.ones(a.shape, bool)
        ok[fin] = R.exp_ok(gv[fin], a[fin], dtype)
        _all_ok(name + " (exp)", ok, gv)
        if dtype == "f32":
            _use("pack_exp_f32_ulp", R.exp_ulps(gv[fin], a[fin]).max() / R.E_ULP)
        if (~fin).any():
            _same(name + " (exp of nan / inf)", got[~fin], R.stored(R.pack_f32(func, a[~fin], None, dtype), dtype))
        return
    _same(name, got, R.stored(R.pack_f32(func, a, b, dtype), dtype))


def _pack_case(rows, cols, fname, dtype, outs, ld_src=None):
    L, lib, h = _ctx()
    func = FUNCS[fname]
    ld_src = cols + 3 if ld_src is None else ld_src
    a, b = R.pack_set(rows, cols)
    sa, sb = np.full((rows, ld_src), 1e30, F), np.full((rows, ld_src), 1e30, F)
    sa[:, :cols], sb[:, :cols] = a, b
    da, db = _dev(sa), _dev(sb)
    dst = Mat(rows, cols, L.pad_ld(cols + 1), dtype) if "d" in outs else None
    dstT = Mat(cols, rows, L.pad_ld(rows + 1), dtype) if "t" in outs else None
    L.check(lib.vbnn_pack(h, _dt(dtype)[0], func, _p(da), _p(db) if func == R.MUL else None, ld_src, rows, cols,
                          dst.p if dst else None, dst.ld if dst else 0, dstT.p if dstT else None, dstT.ld if dstT else 0))
    torch.cuda.synchronize()
    g = dst.data("dst") if dst else None
    gT = dstT.data("dstT") if dstT else None
    if dst:
        _check_packed(f"pack {fname} {dtype} dst", g, func, a, b, dtype)
    if dstT:
        _check_packed(f"pack {fname} {dtype} dstT", np.ascontiguousarray(gT.T), func, a, b, dtype)
    if dst and dstT:
        _same("dstT against dst", gT, np.ascontiguousarray(g.T))
    _same("src (unchanged)", _host(da), sa)
    return g, gT


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fname", list(FUNCS))
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (64, 64), (65, 63), (130, 70)])
def test_pack(rows, cols, fname, dtype):
    for outs in (("dt", "d", "t") if (rows, cols) == (65, 63) else ("dt",)):
        _pack_case(rows, cols, fname, dtype, outs)


def test_pack_relu_of_negative_zero_and_nan():
    """What k_pack's fmaxf leaves for -0.0 and a NaN (the header states it): +0 for both, bit for bit; printed as well."""
    g, _ = _pack_case(5, 7, "relu", "f32", "d")
    print(f"PACK_RELU: nan -> {g[1, 0]!r}, +inf -> {g[1, 1]!r}, -inf -> {g[1, 2]!r} ({_u(g)[1, 2]:#x}), -0.0 -> bits {_u(g)[1, 3]:#x}, +0.0 -> bits {_u(g)[1, 4]:#x}")
    assert g[1, 1] == np.inf and not _u(g)[1, [0, 2, 3, 4]].any()


def test_pack_above_the_tile_cap():
    """1 x 262 208: 4097 tiles against the 4096-block cap (the grid loop), both outputs."""
    _pack_case(1, 262208, "square", "f32", "dt", ld_src=262208)


# ------------------------------------------------------------------------------------------------ pack_input
OUTS = [(1, 1, 1), (0, 1, 1), (0, 1, 0), (0, 0, 0)]          # (x2_s, xT_s, x2T_s) given; x_s always


def _pack_input_case(N, I, dtype, outs, rpd, src_form="aligned", ldT_extra=0):
    L, lib, h = _ctx()
    x = R.input_set(N, I)
    ld_src, off = {"aligned": (_r4(I), 0), "odd": (I + 1, 0), "offset": (_r4(I), 1)}[src_form]
    # the source is allocated with all N rows; under rows_per_draw only the first rpd are the minibatch and the rest hold a
    # poison value: a kernel that read row n instead of row n % rpd would be seen (and would still read inside the buffer)
    s = np.full((N, ld_src), 1e30, F)
    keep = min(rpd, N) if rpd > 0 else N
    s[:keep, :I] = x[:keep]
    src = Vec(N * ld_src, off, s)
    ld_x, ld_xT = L.pad_ld(I + 1), L.pad_ld(N + 1) + ldT_extra
    want2, wantT, want2T = outs
    xs = Mat(N, I, ld_x, dtype)
    x2 = Mat(N, I, ld_x, dtype) if want2 else None
    xT = Mat(I, N, ld_xT, dtype) if wantT else None
    x2T = Mat(I, N, ld_xT, dtype) if want2T else None
    L.check(lib.vbnn_pack_input(h, _dt(dtype)[0], src.p, ld_src, N, I, xs.p, x2.p if x2 else None, ld_x, xT.p if xT else None,
                                x2T.p if x2T else None, ld_xT if xT else 0, rpd))
    torch.cuda.synchronize()
    ref_x, ref_x2 = R.pack_input_f32(s[:, :I], N, rpd, dtype)
    tag = f"pack_input {N}x{I} {dtype} outs{outs} rpd{rpd} {src_form} ldT+{ldT_extra}"
    _same(tag + " x_s", xs.data("x_s"), ref_x)
    if x2:
        _same(tag + " x2_s", x2.data("x2_s"), ref_x2)
    if xT:
        _same(tag + " xT_s", xT.data("xT_s"), np.ascontiguousarray(ref_x.T))
    if x2T:
        _same(tag + " x2T_s", x2T.data("x2T_s"), np.ascontiguousarray(ref_x2.T))
    _same(tag + " src (unchanged)", src.data("src").reshape(N, ld_src), s)


def _rpds(N):
    return [0] + ([N // 2] if N % 2 == 0 else []) + ([7] if N % 7 != 0 else [])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N,I", [(1, 1), (3, 7), (37, 70), (64, 64), (100, 130)])
def test_pack_input(N, I, dtype):
    for outs in OUTS:
        for rpd in _rpds(N):
            _pack_input_case(N, I, dtype, outs, rpd)
    for src_form in ("odd", "offset"):                               # scalar loads
        for ldT_extra in (0, 2):                                     # ld_xT & 3 != 0: scalar transposed stores
            for rpd in (0, 7):
                _pack_input_case(N, I, dtype, OUTS[0], rpd, src_form, ldT_extra)
    _pack_input_case(N, I, dtype, OUTS[0], 0, "aligned", 2)


def test_pack_input_above_the_tile_cap():
    """1 x 262 208: 4097 tiles against the 4096-block cap."""
    _pack_input_case(1, 262208, "bf16", OUTS[0], 0)


# ------------------------------------------------------------------------------------------------ compute_prior
def _check_stats(tag, st, means, lvars, W, v32=None):
    """The four statistics against the definition (derived bounds) and, given the device's own float32 variances, the double
    sum of its own terms (1e-10: the reduction alone)."""
    ref = R.prior_f64(means, lvars)["stats"]
    print(f"{tag}: stats {st.tolist()} | definition {ref.tolist()}")
    b0, b1 = R.prior_sum_bound(means, lvars), R.lsum_bound(lvars)
    _use("stats0_vs_definition", abs(st[0] - ref[0]) / b0)
    assert abs(st[0] - ref[0]) <= b0, f"{tag} stats[0]: {st[0]!r} against {ref[0]!r}: off by {abs(st[0] - ref[0]):.3e} > {b0:.3e}"
    if b1 > 0:
        _use("stats1_vs_definition", abs(st[1] - ref[1]) / b1)
    assert abs(st[1] - ref[1]) <= b1, f"{tag} stats[1]: {st[1]!r} against {ref[1]!r}: off by {abs(st[1] - ref[1]):.3e} > {b1:.3e}"
    if v32 is not None:
        s0 = float(np.sum((np.asarray(v32, F) + np.asarray(means, F) * np.asarray(means, F)).astype(f8)))
        _use("stats0_vs_own_terms_1e-10", abs(st[0] - s0) / (1e-10 * s0))
        assert abs(st[0] - s0) <= 1e-10 * s0, f"{tag} stats[0]: {st[0]!r} against the sum of the device's own terms {s0!r}"
    want2 = (1.0 / W) * st[0]
    assert abs(st[2] - want2) <= np.spacing(want2), f"{tag} stats[2]: {st[2]!r} want {want2!r}"
    assert st[3] == W, f"{tag} stats[3]: {st[3]!r} want {W}"


def _prior_case(W, caches, off, kind):
    L, lib, h = _ctx()
    means, lvars = R.param_set(kind, W)
    dm, dl = Vec(W, off, means), Vec(W, off, lvars)
    out = {k: (Vec(W, off) if k in caches else None) for k in ("vars", "stdv", "mu_sqe")}
    st = _stats_buf()
    L.check(lib.vbnn_compute_prior(h, dm.p, dl.p, W, *[out[k].p if out[k] else None for k in ("vars", "stdv", "mu_sqe")], _p(st)))
    torch.cuda.synchronize()
    tag = f"compute_prior W{W} {kind} caches{caches} off{off}"
    got = {k: v.data(k) for k, v in out.items() if v}
    ref = R.prior_f32(means, lvars)
    if "vars" in got:
        _all_ok(tag + " vars", R.exp_ok(got["vars"], lvars, "f32"), got["vars"])
        _use("prior_vars_ulp", R.exp_ulps(got["vars"], lvars).max() / R.E_ULP)
    if "stdv" in got:
        if "vars" in got:
            _same(tag + " stdv", got["stdv"], np.sqrt(got["vars"]))
        else:                                                        # no device vars to root: sqrt32 of the expf allowance's ends
            _inside(tag + " stdv", got["stdv"], np.sqrt(R.exp_shifted(-R.E_ULP)(lvars)), np.sqrt(R.exp_shifted(+R.E_ULP)(lvars)))
    if "mu_sqe" in got:
        _same(tag + " mu_sqe", got["mu_sqe"], ref["mu_sqe"])
    _same(tag + " means (unchanged)", dm.data("means"), means)
    _same(tag + " lvars (unchanged)", dl.data("lvars"), lvars)
    _check_stats(tag, _stats(st), means, lvars, W, got.get("vars"))


CACHES = [("vars", "stdv", "mu_sqe"), (), ("vars",), ("stdv",), ("mu_sqe",)]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("W", [1, 2, 3, 5, 1023, 1025, 4096])
def test_compute_prior(W, off):
    for kind in R.PARAM_SETS:
        for caches in CACHES:
            _prior_case(W, caches, off, kind)


def test_compute_prior_beyond_one_grid_stride():
    """W = 2 200 003: more than 2048 x 256 quads, and a tail of three."""
    _prior_case(2200003, CACHES[0], 0, "trained")
    _prior_case(2200003, (), 0, "wide")


# ------------------------------------------------------------------------------------------------ prep_layer / prepare
from tests.test_update_gpu import SHAPES  # noqa: E402  (the tile form, FLAT, ragged, both transposed settings)


class PrepLayer:
    def __init__(self, O, I, transposed, dtype, kind, off=0, seed=0):
        L, _, _ = _ctx()
        self.O, self.I, self.transposed, self.dtype = O, I, transposed, dtype
        m, l = R.param_set(kind, O * I, seed)
        self.means, self.lvars = m.reshape(O, I), l.reshape(O, I)
        self.dm, self.dl = Vec(O * I, off, m), Vec(O * I, 0, l)
        self.reset()

    def reset(self):
        L, _, _ = _ctx()
        O, I = self.O, self.I
        self.mu, self.var = Mat(O, I, L.pad_ld(I + 1), self.dtype), Mat(O, I, L.pad_ld(I + 1), self.dtype)
        self.muT = Mat(I, O, L.pad_ld(O + 1), self.dtype) if self.transposed else None
        self.varT = Mat(I, O, L.pad_ld(O + 1), self.dtype) if self.transposed else None
        self.st = _stats_buf()

    def args(self):
        return (self.dm.p, self.dl.p, self.O, self.I, self.mu.p, self.var.p, self.mu.ld, self.muT.p if self.muT else None,
                self.varT.p if self.varT else None, self.muT.ld if self.muT else 0, _p(self.st))

    def desc(self):
        L, _, _ = _ctx()
        a = self.args()
        return L.PrepDesc(means=a[0], lvars=a[1], O=a[2], I=a[3], mu_s=a[4], var_s=a[5], ld_w=a[6], muT_s=a[7], varT_s=a[8],
                          ld_wT=a[9], stats=a[10])

    def verify(self, tag):
        O, I, dtype = self.O, self.I, self.dtype
        mu, var = self.mu.data("mu_s"), self.var.data("var_s")
        _same(tag + " mu_s", mu, R.stored(self.means, dtype))
        vv = R.values(var)
        _all_ok(tag + " var_s", R.exp_ok(vv, self.lvars, dtype), vv)
        if dtype == "f32":
            _use("prep_var_s_ulp", R.exp_ulps(vv, self.lvars).max() / R.E_ULP)
        if self.transposed:
            _same(tag + " muT_s", self.muT.data("muT_s"), np.ascontiguousarray(mu.T))
            _same(tag + " varT_s", self.varT.data("varT_s"), np.ascontiguousarray(var.T))
        _same(tag + " means (unchanged)", self.dm.data("means").reshape(O, I), self.means)
        st = _stats(self.st)
        _check_stats(tag, st, self.means, self.lvars, O * I, vv if dtype == "f32" else None)
        return mu, var, st


def _prep_both_entries(O, I, transposed, dtype, kind, off=0):
    """vbnn_prep_layer, then one-layer vbnn_prepare on fresh outputs: each against the reference, and the same bits."""
    L, lib, h = _ctx()
    lay = PrepLayer(O, I, transposed, dtype, kind, off)
    tag = f"{O}x{I}{'T' if transposed else 'F'} {dtype} {kind}"
    L.check(lib.vbnn_prep_layer(h, _dt(dtype)[0], *lay.args()))
    torch.cuda.synchronize()
    a = lay.verify("prep_layer " + tag)
    lay.reset()
    L.check(lib.vbnn_prepare(h, _dt(dtype)[0], 1, (L.PrepDesc * 1)(lay.desc()), None))
    torch.cuda.synchronize()
    b = lay.verify("prepare " + tag)
    for name, x, y in zip(("mu_s", "var_s", "stats"), a, b):
        _same(f"prepare against prep_layer {tag} {name}", y, x)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("O,I,transposed", SHAPES, ids=[f"{o}x{i}{'T' if t else 'F'}" for o, i, t in SHAPES])
def test_prep_layer_and_prepare(O, I, transposed, dtype):
    kinds = R.PARAM_SETS if O * I <= 30000 else (R.PARAM_SETS[(O + I) % 3],)      # the large layers take one set each
    for kind in kinds:
        _prep_both_entries(O, I, transposed, dtype, kind)


def test_prep_layer_tile_loop_above_the_block_cap():
    """(2, 131 073) with transposes: 2049 tiles against the 2048-block cap on 262 k elements, scalar loads (odd I)."""
    _prep_both_entries(2, 131073, True, "f32", "trained")


def test_prep_layer_flat_form_on_the_capped_grid():
    """(17, 131 072) without transposes: FLAT, 2048 blocks x 1024 elements per stride, a ragged second stride."""
    _prep_both_entries(17, 131072, False, "f32", "wide")
    _prep_both_entries(17, 131072, False, "bf16", "trained")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prep_layer_means_offset_by_one_float(dtype):
    """(128, 192) without transposes would take the FLAT form; means one float past 16 bytes refuses it (scalar loads)."""
    _prep_both_entries(128, 192, False, dtype, "trained", off=1)
    _prep_both_entries(128, 192, True, dtype, "wide", off=1)


EIGHT = [(1, 1, True), (5, 7, True), (70, 50, True), (128, 192, True), (96, 100, False), (256, 512, False),
         (2, 131073, True), (17, 131072, False)]                     # the last two at the 2048-block cap


@pytest.mark.parametrize("extra_outs", ["dt", "d", "t"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prepare_eight_layers_and_the_extra_matrix(dtype, extra_outs):
    """One vbnn_prepare: eight layers of different shapes and forms, every layer's four statistics its own, plus the extra
    matrix, 100 x 10 so that ld_dst (64) != ld_dstT (128)."""
    L, lib, h = _ctx()
    lays = [PrepLayer(O, I, tr, dtype, R.PARAM_SETS[i % 3], seed=i) for i, (O, I, tr) in enumerate(EIGHT)]
    rows, cols, ld_src = 100, 10, 13
    w = np.full((rows, ld_src), 1e30, F)
    w[:, :cols] = R.pack_set(rows, cols)[0]
    src = _dev(w)
    dst = Mat(rows, cols, L.pad_ld(cols + 1), dtype) if "d" in extra_outs else None
    dstT = Mat(cols, rows, L.pad_ld(rows + 1), dtype) if "t" in extra_outs else None
    assert L.pad_ld(cols + 1) < L.pad_ld(rows + 1)
    extra = L.PackDesc(src=_p(src), rows=rows, cols=cols, ld_src=ld_src, dst=dst.p if dst else None, ld_dst=dst.ld if dst else 0,
                       dstT=dstT.p if dstT else None, ld_dstT=dstT.ld if dstT else 0)
    L.check(lib.vbnn_prepare(h, _dt(dtype)[0], 8, (L.PrepDesc * 8)(*[lay.desc() for lay in lays]), C.byref(extra)))
    torch.cuda.synchronize()
    seen = []
    for lay, (O, I, tr) in zip(lays, EIGHT):
        seen.append(lay.verify(f"prepare[8] {O}x{I} {dtype}")[2])
    assert len({s.tobytes() for s in seen}) == 8, "two layers share their statistics"
    want = R.stored(w[:, :cols], dtype)
    if dst:
        _same("extra dst", dst.data("extra dst"), want)
    if dstT:
        _same("extra dstT", dstT.data("extra dstT"), np.ascontiguousarray(want.T))
    _same("extra src (unchanged)", _host(src), w)


# ------------------------------------------------------------------------------------------------ calc_lc
def _lc_case(W, route, kind, B, check_null=True):
    L, lib, h = _ctx()
    means, lvars = R.param_set(kind, W)
    var_hat = R.prior_f64(means, lvars)["stats"][2]
    st = _dev(np.array([0.0, 0.0, var_hat, float(W)]))
    vars_ = R.exp32(lvars) if route == "cached" else None
    mu_sqe = means * means if route == "cached" else None
    ins = [Vec(W, 0, a) if a is not None else None for a in
           ((means, lvars, None, None) if route == "derived" else (None, None, vars_, mu_sqe))]
    sums = []
    for elem in ((True, False) if check_null else (True,)):
        lc = Vec(W) if elem else None
        s = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
        L.check(lib.vbnn_calc_lc(h, *[v.p if v else None for v in ins], _p(st), B, lc.p if lc else None, _p(s), W))
        torch.cuda.synchronize()
        hs = _host(s)
        assert hs[1] == -7.0
        sums.append(hs[0])
        if elem:
            got = lc.data("lc_elem")
    tag = f"calc_lc W{W} {route} {kind} B{B:g}"
    a = (means, lvars, vars_, mu_sqe, var_hat, B)
    want, want_sum = R.calc_lc_f64(*a)
    bound = R.lc_bound(*a)
    err = np.abs(got.astype(f8) - want)
    _use(f"lc_elem_{route}", (err / bound).max())
    i = int(np.argmax(err / bound))
    print(f"{tag}: worst element {i}: got {got[i]!r} definition {want[i]!r} bound {bound[i]:.3e}; sum {sums[0]!r} definition {want_sum!r}")
    _all_ok(tag + " lc_elem", err <= bound, got)
    own = float(np.sum(got.astype(f8)))
    mag = float(np.sum(np.abs(got.astype(f8))))
    if mag > 0:
        _use("lc_sum_vs_own_elements_1e-10", abs(sums[0] - own) / (1e-10 * mag))
    assert abs(sums[0] - own) <= 1e-10 * mag, f"{tag}: sum {sums[0]!r} against the float64 sum of the device's own elements {own!r}"
    sb = float(np.sum(bound)) + 1e-10 * float(np.sum(np.abs(want)))
    _use(f"lc_sum_{route}", abs(sums[0] - want_sum) / sb)
    assert abs(sums[0] - want_sum) <= sb, f"{tag}: sum {sums[0]!r} against the definition {want_sum!r}: off by more than {sb:.3e}"
    if check_null:
        assert _u(np.array(sums[1])) == _u(np.array(sums[0])), f"{tag}: the sum without lc_elem {sums[1]!r} is not the sum with it {sums[0]!r}"


@pytest.mark.parametrize("route", ["cached", "derived"])
@pytest.mark.parametrize("W", [1, 5, 1023, 1025, 70000])
def test_calc_lc(W, route):
    for kind in R.PARAM_SETS:
        for B in (1e6, 50.0):
            _lc_case(W, route, kind, B)


def test_calc_lc_beyond_one_grid_stride():
    """W = 2 200 003: 2048 blocks x 256 threads x more than four elements each."""
    _lc_case(2200003, "derived", "trained", 1e6)


# ------------------------------------------------------------------------------------------------ KL gradients
def _grads_inputs(W, kind):
    means, lvars = R.param_set(kind, W)
    var_hat = R.telling_var_hat(R.prior_f64(means, lvars)["stats"][2])
    r = np.random.RandomState(W)
    return means, lvars, var_hat, r.standard_normal(W).astype(F)


@pytest.mark.parametrize("S", [1.0, 30.0])
@pytest.mark.parametrize("B", [1.0, 1e6])
@pytest.mark.parametrize("W", [1, 5, 1025])
def test_compute_mugrads(W, B, S):
    L, lib, h = _ctx()
    for kind in R.PARAM_SETS:
        means, _, var_hat, g = _grads_inputs(W, kind)
        st = _dev(np.array([0.0, 0.0, var_hat, float(W)]))
        want_lcg, want_g = R.mugrads_f32(means, var_hat, B, S, g)
        for outs in ("gl", "g", "l"):
            dm = Vec(W, 0, means)
            dg = Vec(W, 0, g) if "g" in outs else None
            dl = Vec(W) if "l" in outs else None
            L.check(lib.vbnn_compute_mugrads(h, dm.p, _p(st), B, S, dg.p if dg else None, dl.p if dl else None, W))
            torch.cuda.synchronize()
            tag = f"mugrads W{W} {kind} B{B:g} S{S:g} {outs}"
            if dg:
                _same(tag + " gradWeight (in place)", dg.data("gradWeight"), want_g)
            if dl:
                _same(tag + " lcg", dl.data("lcg"), want_lcg)
            _same(tag + " means (unchanged)", dm.data("means"), means)


@pytest.mark.parametrize("route", ["given", "lvars"])
@pytest.mark.parametrize("S", [1.0, 30.0])
@pytest.mark.parametrize("B", [1.0, 1e6])
@pytest.mark.parametrize("W", [1, 5, 1025])
def test_compute_vargrads(W, B, S, route):
    L, lib, h = _ctx()
    for kind in R.PARAM_SETS:
        _, lvars, var_hat, g = _grads_inputs(W, kind)
        st = _dev(np.array([0.0, 0.0, var_hat, float(W)]))
        vars_ = R.exp32(lvars) if route == "given" else None
        stdv = np.sqrt(vars_) if route == "given" else None
        for outs in ("gl", "g", "l"):
            dlv = Vec(W, 0, lvars) if route == "lvars" else None
            dv, dsd = (Vec(W, 0, vars_), Vec(W, 0, stdv)) if route == "given" else (None, None)
            dg = Vec(W, 0, g) if "g" in outs else None
            dl = Vec(W) if "l" in outs else None
            L.check(lib.vbnn_compute_vargrads(h, dlv.p if dlv else None, dv.p if dv else None, dsd.p if dsd else None, _p(st), B, S,
                                              dg.p if dg else None, dl.p if dl else None, W))
            torch.cuda.synchronize()
            tag = f"vargrads W{W} {kind} B{B:g} S{S:g} {route} {outs}"
            if route == "given":
                want_lcg, want_g = R.vargrads_f32(None, vars_, stdv, var_hat, B, S, g)
                if dg:
                    _same(tag + " gradSum (in place)", dg.data("gradSum"), want_g)
                if dl:
                    _same(tag + " lcg", dl.data("lcg"), want_lcg)
            else:
                if dg:
                    _inside(tag + " gradSum (in place)", dg.data("gradSum"),
                            *R.envelope(lambda exp: R.vargrads_f32(lvars, None, None, var_hat, B, S, g, exp=exp)[1]))
                if dl:
                    _inside(tag + " lcg", dl.data("lcg"),
                            *R.envelope(lambda exp: R.vargrads_f32(lvars, None, None, var_hat, B, S, g, exp=exp)[0]))
