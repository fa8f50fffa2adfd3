"""The pruning family through the C ABI -- vbnn_snr, vbnn_prune_select, vbnn_prune_pack (prune.hip), vbnn_prune_compress
(sparse.hip) and vbnn_unit_snr / _select / _index / _gather (units.hip) -- against the NumPy reference of tests/_prune_np.py
(itself held to brute force by test_prune_ref.py). That module's docstring says what is compared bit for bit and derives every
bound used here; none is fitted to the device.

Common rules. Every buffer a launch may write is a run of bytes inside an allocation filled with the byte 0xA5: 256 guard bytes
in front (plus the misalignment under test), the payload, some spare elements (a row behind a matrix, the entries behind
nnz_cap, the list words behind n_keep) and 256 guard bytes behind. An output is compared WHOLE against an expectation that
starts as the sentinel too: pads, spare elements and guards must still hold it. Every launch runs twice on fresh buffers and
the two runs must leave the same bytes. Inputs a broken clamp could over-read carry spare rows as well, so that a defect shows
as a wrong value. Misaligned pointers go only to the arguments whose alignment the kernels test and fall back on.

The module writes the fractions of the bounds the device used, what it did with denormals and NaN payloads, and the duration of
each test to prune_bounds.txt in the results directory of the tools/ scripts (OUT_DIR, by default bench_out/; committed from an
MI355X as profiles/prune_bounds.txt)."""
import ctypes as C
import itertools
import os
import time

import numpy as np
import pytest

from tests import _prune_np as P
from tests import _units_np as U
from tests._sparse_np import csr_to_dense

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F, f8, u8, u16, u32 = np.float32, np.float64, np.uint8, np.uint16, np.uint32
SB = 0xA5
GUARD = 256
W_BIG = 4096 * 1025 + 3
USED, FOUND, TIMES = {}, {}, []


# ------------------------------------------------------------------------------------------------ plumbing
def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, L.lib(), nn.Context.get().h


def _np_dt(dtype):
    return F if dtype == "f32" else u16


def _code(dtype):
    from vbnn_amd import _lib as L
    return L.F32 if dtype == "f32" else L.BF16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: u8, 2: u16, 4: u32, 8: np.uint64}[a.dtype.itemsize])


def _sentinel(n, dt):
    return np.full(n * np.dtype(dt).itemsize, SB, u8).view(dt)


def _use(name, frac):
    frac = float(frac)
    USED[name] = max(USED.get(name, 0.0), frac)
    print(f"bound used: {name} {frac:.4f}")


@pytest.fixture(autouse=True)
def _time_each(request):
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    TIMES.append((request.node.name, time.time() - t0))


@pytest.fixture(scope="module", autouse=True)
def _record():
    t0 = time.time()
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.abspath(os.environ.get("OUT_DIR") or os.path.join(root, "bench_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "prune_bounds.txt"), "w") as f:
        f.write(f"tests/test_prune_forms_gpu.py on one MI355X: {len(TIMES)} tests, {time.time() - t0:.1f} s wall for the file.\n"
                "Per bounded output, the largest fraction of its bound the device used (1 = the bound; bounds derived in\n"
                "tests/_prune_np.py). Outputs not listed were compared bit for bit.\n"
                f"CPU, tests/test_prune_ref.py: fraction the float32 restatement with a correctly rounded exp uses: {P.BOUND_USED}\n")
        for k in sorted(USED):
            f.write(f"  {k:36s} {USED[k]:.4f}\n")
        f.write("Denormals and NaN payloads (keys at lvar = 0, where the key is |mean| unless the device changes it):\n")
        for k in sorted(FOUND):
            f.write(f"  {k:36s} {FOUND[k]}\n")
        f.write("Seconds per test:\n")
        for name, s in TIMES:
            f.write(f"  {s:8.3f}  {name}\n")


class Buf:
    """n (+ extra spare) elements of `dt`, off_bytes past a 256-byte boundary, inside a 0xA5-filled allocation with guards."""

    def __init__(self, n, dt, off_bytes=0, fill=None, extra=0):
        self.dt, self.n, self.extra = np.dtype(dt), int(n), int(extra)
        self.front = GUARD + int(off_bytes)
        self.size = (self.n + self.extra) * self.dt.itemsize
        self.raw = torch.full((self.front + self.size + GUARD,), SB, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        if fill is not None:
            self.set(fill)

    def set(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype.itemsize == self.dt.itemsize and a.size <= self.n + self.extra
        if a.size:
            self.raw[self.front:self.front + a.nbytes].copy_(torch.from_numpy(a.view(u8).copy()).cuda())

    @property
    def p(self):
        return C.c_void_p(self.raw.data_ptr() + self.front)

    def at(self, i):
        return C.c_void_p(self.raw.data_ptr() + self.front + int(i) * self.dt.itemsize)

    def read(self, name):
        """All n + extra elements, after checking the guards on both sides."""
        h = self.raw.cpu().numpy()
        assert (h[:self.front] == SB).all(), f"{name}: written in front of the buffer"
        assert (h[self.front + self.size:] == SB).all(), f"{name}: written behind the buffer"
        return h[self.front:self.front + self.size].copy().view(self.dt)


def _same(name, got, want):
    """Every element, bit for bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    if bad.size:
        i = tuple(int(q) for q in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} differ; first at {i}: got {_bits(got)[i]:#x} want {_bits(want)[i]:#x}")


def _same_runs(name, a, b):
    assert a.keys() == b.keys()
    for k in a:
        _same(f"{name} {k}: two runs", a[k], b[k])


def _params(O, I, seed):
    """means ~ N(0, 1), lvars = log 1e-2 + 0.75 N(0, 1), as the engine-level tests; O x I float32."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((O, I)).astype(F)
    l = (F(np.log(1e-2)) + F(0.75) * rng.standard_normal((O, I)).astype(F)).astype(F)
    return m, l


def _dev_exp(l):
    """The device's own float32 expf(l), element-wise: var_p of a vbnn_prune_pack at tau = 0 (nothing is pruned)."""
    L, lib, h = _ctx()
    shape, l = np.shape(l), np.ascontiguousarray(l, F).reshape(-1)
    W = l.size
    dm, dl = Buf(W, F, fill=np.zeros(W, F)), Buf(W, F, fill=l)
    mu, var, st = Buf(W, F), Buf(W, F), Buf(4, f8)
    d = (L.PruneDesc * 1)(L.PruneDesc(means=dm.p, lvars=dl.p, O=1, I=W, mu_p=mu.p, var_p=var.p, ld_w=W, stats=st.p, mask=None))
    L.check(lib.vbnn_prune_pack(h, L.F32, 1, d, None, 0.0))
    v = var.read("var_p")
    assert not _bits(mu.read("mu_p")).any() and (v > 0).all()
    return v.reshape(shape)


def _dev_prep(m, l, dtype):
    """vbnn_prep_layer's mu_s / var_s for the O x I parameters, as stored (float32, or bf16 bit patterns)."""
    L, lib, h = _ctx()
    O, I = m.shape
    ld, dt = L.pad_ld(I + 1), _np_dt(dtype)
    dm, dl = Buf(O * I, F, fill=m), Buf(O * I, F, fill=l)
    mu, var, st = Buf(O * ld, dt), Buf(O * ld, dt), Buf(4, f8)
    L.check(lib.vbnn_prep_layer(h, _code(dtype), dm.p, dl.p, O, I, mu.p, var.p, ld, None, None, 0, st.p))
    return (mu.read("mu_s").reshape(O, ld)[:, :I].copy(), var.read("var_s").reshape(O, ld)[:, :I].copy())


def _dev_keys(m, l):
    L, lib, h = _ctx()
    m, l = np.ascontiguousarray(m, F).reshape(-1), np.ascontiguousarray(l, F).reshape(-1)
    dm, dl, out = Buf(m.size, F, fill=m), Buf(m.size, F, fill=l), Buf(m.size, F)
    L.check(lib.vbnn_snr(h, dm.p, dl.p, m.size, out.p))
    return out.read("snr")


def _with_ties(m, l, seed, empty_rows=False):
    """Copies the median-key weight over an eighth of the others (signs alternating), so that a tau at that key ties; optionally
    rows 3, 8, 13, ... get means a millionth the size: empty rows at that tau. Returns (m, l, v, keys, tau)."""
    O, I = m.shape
    m, l = m.copy(), l.copy()
    rng = np.random.default_rng(seed + 17)
    if empty_rows:
        m[3::5] *= F(1e-6)
    k0 = P.weight_key32(m, P.exp32(l)).ravel()
    j0 = int(np.argsort(k0, kind="stable")[k0.size // 2])
    others = rng.permutation(k0.size)[:k0.size // 8]
    if empty_rows:
        others = others[(others // I) % 5 != 3]
    m.flat[others] = m.flat[j0] * np.where(np.arange(others.size) & 1, F(-1), F(1)).astype(F)
    l.flat[others] = l.flat[j0]
    v = _dev_exp(l)
    keys = P.weight_key32(m, v)
    return m, l, v, keys, F(keys.flat[j0])


# ------------------------------------------------------------------------------------------------ vbnn_snr
@pytest.mark.parametrize("W", [1, 3, 4, 5, 1023, 4096, 4097, 12289])
def test_snr(W):
    L, lib, h = _ctx()
    m, l = (a.reshape(-1) for a in _params(1, W, W))
    want = P.weight_key32(m, _dev_exp(l))
    exp = _sentinel(W + 4, F)
    exp[:W] = want
    for om, ol, oo in itertools.product((0, 4), repeat=3):
        outs = []
        for _ in range(2):
            dm, dl, out = Buf(W, F, om, m), Buf(W, F, ol, l), Buf(W, F, oo, extra=4)
            L.check(lib.vbnn_snr(h, dm.p, dl.p, W, out.p))
            outs.append(out.read("snr_out"))
        _same(f"snr W={W} offsets {om},{ol},{oo}: two runs", outs[0], outs[1])
        _same(f"snr W={W} offsets {om},{ol},{oo}", outs[0], exp)
    _use("weight_key", (np.abs(want.astype(f8) - P.weight_key64(m, l)) / P.key_bound(m, l)).max())


def test_key_edges():
    """Denormal means, inf and NaNs with payloads at lvar = 0: what the device's key is, on record and as the header states it."""
    for name in ("edges", "full"):
        b = P.population(name, 1000)
        m = P.means_of(b)
        got = _bits(_dev_keys(m, np.zeros(1000, F)))
        assert P.coverage(name, got) == [], (name, P.coverage(name, got))
        den, nan = (b > 0) & (b < 0x00800000), b > P.INF_BITS
        quiet = nan & ((b & 0x00400000) != 0)
        FOUND[f"{name}: denormal keys kept"] = bool((got[den] == b[den]).all())
        FOUND[f"{name}: denormal keys flushed to 0"] = bool((got[den] == 0).any())
        FOUND[f"{name}: quiet NaN payloads kept"] = bool((got[quiet] == b[quiet]).all())
        FOUND[f"{name}: NaN keys stay NaN"] = bool((got[nan] > P.INF_BITS).all())
        if (nan & ~quiet).any():
            FOUND[f"{name}: signalling NaNs made quiet, payload kept"] = bool((got[nan & ~quiet] == (b[nan & ~quiet] | 0x00400000)).all())
        print({k: v for k, v in FOUND.items() if k.startswith(name)})
        assert (got[~den & ~nan] == b[~den & ~nan]).all()                  # zero, normals, inf: |mean| bit for bit
        assert (got[nan] > P.INF_BITS).all()
        assert FOUND[f"{name}: denormal keys kept"] == P.DEVICE_FINDINGS["denormal_keys_kept"]
        assert FOUND[f"{name}: quiet NaN payloads kept"] == P.DEVICE_FINDINGS["nan_payload_kept"]
    # 0 / 0: mean 0 under a variance that underflows to 0
    assert np.isnan(_dev_keys(np.zeros(4, F), np.full(4, -200.0, F))).all()


# ------------------------------------------------------------------------------------------------ vbnn_prune_select
def _split(W, n_layers):
    """n_layers shapes (O, I) whose sizes add up to W, from one weight up."""
    if n_layers == 1:
        return [(1, W)]
    if n_layers == 2:
        return [(1, 1), (1, W - 1)]
    head = [(1, 1), (1, 3), (2, 2), (3, 5), (1, 64), (7, 9), (5, 4)]
    return head + [(1, W - sum(o * i for o, i in head))]


def _select(m, l, shapes, ks):
    """vbnn_prune_select at every k of ks over the layers `shapes` cut from the flat m, l: one tau slot per k, read back once."""
    L, lib, h = _ctx()
    n = len(shapes)
    d, keep, at = (L.PruneDesc * n)(), [], 0
    for j, (O, I) in enumerate(shapes):
        dm = Buf(O * I, F, 4 * (j % 2), m[at:at + O * I])                  # some bases misaligned
        dl = Buf(O * I, F, 4 * (j % 3 == 1), l[at:at + O * I])
        keep += [dm, dl]
        d[j] = L.PruneDesc(means=dm.p, lvars=dl.p, O=O, I=I)
        at += O * I
    assert at == m.size
    nb = C.c_size_t()
    L.check(lib.vbnn_prune_workspace_bytes(n, d, C.byref(nb)))
    ws = Buf(nb.value, u8)                                                 # exactly the bytes asked for, every one 0xA5
    ws.raw[ws.front:ws.front + nb.value] = 0xFF
    tau = Buf(len(ks), F, extra=1)
    for j, k in enumerate(ks):
        L.check(lib.vbnn_prune_select(h, n, d, int(k), tau.at(j), ws.p, nb.value))
    out = tau.read("tau")
    ws.read("workspace")
    assert _bits(out)[-1] == _bits(_sentinel(1, F))[0]
    return out[:-1]


@pytest.mark.parametrize("name", P.POPULATIONS)
def test_select_every_k(name):
    W = 1100
    m = P.means_of(P.population(name, W))
    l = np.zeros(W, F)
    keys = _bits(_dev_keys(m, l))
    assert P.coverage(name, keys) == [], P.coverage(name, keys)
    want = np.sort(keys)
    for n_layers in (1, 2, 8):
        got = _select(m, l, _split(W, n_layers), range(W))
        _same(f"select {name} {n_layers} layers: two runs", got, _select(m, l, _split(W, n_layers), range(W)))
        _same(f"select {name} {n_layers} layers", got, want)
    for w in (1, 2, 3, 5):                                                 # layers of one weight and little more
        mm = m[:w]
        kk = np.sort(_bits(_dev_keys(mm, l[:w])))
        for n_layers in (1, 2)[:1 + (w > 1)]:
            _same(f"select {name} W={w}", _select(mm, l[:w], _split(w, n_layers), range(w)), kk)
    L, lib, h = _ctx()
    dm, t = Buf(4, F, fill=m[:4]), Buf(1, F)
    d = (L.PruneDesc * 1)(L.PruneDesc(means=dm.p, lvars=dm.p, O=1, I=4))
    ws = Buf(_ws_bytes(), u8)
    assert lib.vbnn_prune_select(h, 1, d, 4, t.p, ws.p, ws.n) != 0 and lib.vbnn_prune_select(h, 1, d, -1, t.p, ws.p, ws.n) != 0
    assert lib.vbnn_prune_select(h, 1, d, 0, t.p, ws.p, ws.n - 1) != 0
    assert (_bits(t.read("tau")) == _bits(_sentinel(1, F))).all()           # a refused call writes nothing


def _ws_bytes():
    L, lib, h = _ctx()
    dm = Buf(1, F, fill=np.zeros(1, F))
    nb = C.c_size_t()
    L.check(lib.vbnn_prune_workspace_bytes(1, (L.PruneDesc * 1)(L.PruneDesc(means=dm.p, lvars=dm.p, O=1, I=1)), C.byref(nb)))
    return nb.value


_BIG = {}


def _big():
    """The W = 4096 x 1025 + 3 layer (more than 1024 workgroups' worth): `full` patterns at lvar = 0, its device keys sorted."""
    if not _BIG:
        m = P.means_of(P.population("full", W_BIG))
        l = np.zeros(W_BIG, F)
        keys = _bits(_dev_keys(m, l))
        assert P.coverage("full", keys) == []
        _BIG.update(m=m, l=l, keys=keys, sorted=np.sort(keys))
    return _BIG


def test_select_at_the_workgroup_cap():
    b = _big()
    assert P.prune_grid(W_BIG) == 1024 and (W_BIG + 4095) // 4096 > 1024
    ks = [0, 1, 2, W_BIG // 1000, W_BIG // 7, W_BIG // 2, W_BIG - W_BIG // 9, W_BIG - 3, W_BIG - 2, W_BIG - 1]
    got = _select(b["m"], b["l"], [(1, W_BIG)], ks)
    _same("select at the cap: two runs", got, _select(b["m"], b["l"], [(1, W_BIG)], ks))
    _same("select at the cap", got, b["sorted"][ks])
    got = _select(b["m"], b["l"], [(1, 5), (1, W_BIG - 5)], ks[::3])       # the large layer on a misaligned base
    _same("select at the cap, two layers", got, b["sorted"][ks[::3]])


# ------------------------------------------------------------------------------------------------ vbnn_prune_pack
SHAPES = [(1, 1), (3, 5), (5, 4), (7, 64), (33, 67), (130, 256)]


def _pack(specs, dtype, tau, how):
    """One vbnn_prune_pack over the layers `specs` (dicts: m, l, ld, mask: None / 0 / 1 byte offset, out_off and in_off in
    elements). Returns per layer the WHOLE buffers: mu, var (O + 1 rows of ld), mask (O I + 4 bytes), stats (5 doubles)."""
    L, lib, h = _ctx()
    n, dt = len(specs), _np_dt(dtype)
    isz = np.dtype(dt).itemsize
    d, bufs = (L.PruneDesc * n)(), []
    for j, s in enumerate(specs):
        O, I = s["m"].shape
        b = dict(dm=Buf(O * I, F, 4 * s["in_off"], s["m"]), dl=Buf(O * I, F, 4 * s["in_off"], s["l"]),
                 mu=Buf(O * s["ld"], dt, isz * s["out_off"], extra=s["ld"]), var=Buf(O * s["ld"], dt, isz * s["out_off"], extra=s["ld"]),
                 stats=Buf(4, f8, extra=1), mask=None if s["mask"] is None else Buf(O * I, u8, s["mask"], extra=4))
        bufs.append(b)
        d[j] = L.PruneDesc(means=b["dm"].p, lvars=b["dl"].p, O=O, I=I, mu_p=b["mu"].p, var_p=b["var"].p, ld_w=s["ld"],
                           stats=b["stats"].p, mask=None if b["mask"] is None else b["mask"].p)
    if how == "dev":
        t = Buf(1, F, fill=np.array([tau], F))
        L.check(lib.vbnn_prune_pack(h, _code(dtype), n, d, t.p, -1.0))
    else:
        L.check(lib.vbnn_prune_pack(h, _code(dtype), n, d, None, float(tau)))
    out = []
    for b, s in zip(bufs, specs):
        r = {k: b[k].read(k) for k in ("mu", "var", "stats")}
        if b["mask"] is not None:
            r["mask"] = b["mask"].read("mask")
        _same("means (unchanged)", b["dm"].read("means"), s["m"].ravel())
        out.append(r)
    return out


def _pack_expect(s, dtype, tau, keys, prep, v):
    O, I = s["m"].shape
    ld, dt = s["ld"], _np_dt(dtype)
    mask, mu, var = P.pack_ref(keys, tau, prep[0], prep[1])
    e = {}
    for name, val in (("mu", mu), ("var", var)):
        a = _sentinel((O + 1) * ld, dt)
        a[:O * ld].reshape(O, ld)[:, :I] = val
        e[name] = a
    if s["mask"] is not None:
        e["mask"] = _sentinel(O * I + 4, u8)
        e["mask"][:O * I] = mask.ravel()
    return e, mask


def _pack_check(tag, got, s, dtype, tau, keys, prep, v, stats_cache=None):
    e, mask = _pack_expect(s, dtype, tau, keys, prep, v)
    for k in e:
        _same(f"{tag} {k}", got[k], e[k])
    key = (id(v), repr(float(tau)))
    if stats_cache is None or key not in stats_cache:
        ref = P.pack_stats(mask, v)
        if stats_cache is not None:
            stats_cache[key] = ref
    else:
        ref = stats_cache[key]
    (want, rel), st = ref, got["stats"]
    assert _bits(st)[4] == _bits(_sentinel(1, f8))[0], f"{tag}: written behind the fourth statistic"
    assert st[0] == want[0] and st[3] == want[3], (tag, st, want)
    for q in (1, 2):
        assert abs(st[q] - want[q]) <= rel * want[q], (tag, q, st[q], want[q], rel)
        if want[q] > 0:
            _use("pack_stats", abs(st[q] - want[q]) / (rel * want[q]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack(shape, dtype):
    O, I = shape
    m, l, v, keys, tie = _with_ties(*_params(O, I, 10 * O + I), seed=O + I)
    if O * I >= 16:
        assert (keys == tie).sum() >= 2
    prep = _dev_prep(m, l, dtype)
    _same("the prepared variance is the expf the reference was given", prep[1], v if dtype == "f32" else P.bf16_bits(v))
    cache = {}
    for ld in dict.fromkeys([I, I + 1, I + 4, (I + 7) // 8 * 8]):
        for mask, out_off in itertools.product((None, 0, 1), (0, 1)):
            for tau in (F(0), F(np.inf), F(np.nan), tie):
                runs = []
                for how, in_off in (("host", 0), ("dev", 1)):                 # tau_dev also reads means / lvars one float off
                    s = dict(m=m, l=l, ld=ld, mask=mask, out_off=out_off, in_off=in_off)
                    runs += [_pack([s], dtype, tau, how)[0], _pack([s], dtype, tau, how)[0]]
                tag = f"pack {O}x{I} {dtype} ld={ld} mask={mask} out_off={out_off} tau={tau}"
                for r in runs[1:]:
                    _same_runs(tag, runs[0], r)
                _pack_check(tag, runs[0], s, dtype, tau, keys, prep, v, cache)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pack_eight_layers(dtype):
    shapes = SHAPES + [(1, 7), (2, 130)]
    specs, refs = [], []
    for j, (O, I) in enumerate(shapes):
        m, l = _params(O, I, 300 + j)
        v = _dev_exp(l)
        specs.append(dict(m=m, l=l, ld=[I, I + 1, I + 4, (I + 7) // 8 * 8][j % 4], mask=[None, 0, 1][j % 3], out_off=j % 2,
                          in_off=(j // 2) % 2))
        refs.append((P.weight_key32(m, v), _dev_prep(m, l, dtype), v))
    pool = np.concatenate([r[0].ravel() for r in refs])
    tau = F(np.partition(pool, pool.size // 2)[pool.size // 2])
    runs = [_pack(specs, dtype, tau, how) for how in ("host", "dev", "host", "dev")]
    for j, s in enumerate(specs):
        for r in runs[1:]:
            _same_runs(f"pack 8 layers, layer {j}", runs[0][j], r[j])
        _pack_check(f"pack 8 layers {dtype}, layer {j}", runs[0][j], s, dtype, tau, *refs[j])


def test_pack_more_than_256_workgroups():
    """1030 x 1030: 260 workgroups, so k_prune_finish's threads 0 .. 3 add a second partial each."""
    O = I = 1030
    assert P.prune_grid(O * I) == 260
    m, l = _params(O, I, 99)
    v = _dev_exp(l)
    keys, prep = P.weight_key32(m, v), _dev_prep(m, l, "f32")
    tau = F(np.partition(keys.ravel(), O * I // 2)[O * I // 2])
    for ld, mask in ((1030, 1), (1032, 0)):
        s = dict(m=m, l=l, ld=ld, mask=mask, out_off=0, in_off=0)
        a, b = _pack([s], "f32", tau, "dev")[0], _pack([s], "f32", tau, "host")[0]
        _same_runs("pack 1030x1030", a, b)
        _pack_check(f"pack 1030x1030 ld={ld}", a, s, "f32", tau, keys, prep, v)


def test_pack_at_the_workgroup_cap():
    b = _big()
    m, l = b["m"].reshape(1, W_BIG), b["l"].reshape(1, W_BIG)
    keys = b["keys"].view(F).reshape(1, W_BIG)                             # the device's keys are the truth for the selection
    prep = _dev_prep(m, l, "f32")
    v = prep[1]
    assert (_bits(v) == 0x3f800000).all() and (_bits(prep[0]) == _bits(m)).all()
    tau = b["sorted"][W_BIG // 2:W_BIG // 2 + 1].view(F)[0]
    s = dict(m=m, l=l, ld=W_BIG, mask=0, out_off=0, in_off=0)
    a, c = _pack([s], "f32", tau, "dev")[0], _pack([s], "f32", tau, "host")[0]
    _same_runs("pack at the cap", a, c)
    _pack_check("pack at the cap", a, s, "f32", tau, keys, prep, v)
    assert a["stats"][0] == W_BIG // 2 - ((b["sorted"][:W_BIG // 2] == b["sorted"][W_BIG // 2]).sum())


# ------------------------------------------------------------------------------------------------ vbnn_prune_compress
C_SHAPES = SHAPES + [(255, 5), (256, 5), (257, 5), (1000, 5), (7, 63), (9, 65)]
SPARE = 8


def _compress(specs, dtype, tau, how):
    """One vbnn_prune_compress. specs: dicts m, l, idx (2 / 4), cap, room (entries the arrays really hold), var (bool). Returns
    per layer the WHOLE buffers and the status."""
    L, lib, h = _ctx()
    n, dt = len(specs), _np_dt(dtype)
    d, sp, bufs = (L.PruneDesc * n)(), (L.SparseDesc * n)(), []
    for j, s in enumerate(specs):
        O, I = s["m"].shape
        room = s["room"] + SPARE
        b = dict(dm=Buf(O * I, F, 0, s["m"]), dl=Buf(O * I, F, 0, s["l"]), row_ptr=Buf(O + 1, u32, extra=1),
                 cols=Buf(room, u16 if s["idx"] == 2 else u32), mu_v=Buf(room, dt), var_v=Buf(room, dt) if s["var"] else None,
                 nnz=Buf(1, u32, extra=1))
        bufs.append(b)
        d[j] = L.PruneDesc(means=b["dm"].p, lvars=b["dl"].p, O=O, I=I)
        sp[j] = L.SparseDesc(row_ptr=b["row_ptr"].p, cols=b["cols"].p, mu_v=b["mu_v"].p, var_v=b["var_v"].p if s["var"] else None,
                             O=O, I=I, nnz_cap=s["cap"], nnz_dev=b["nnz"].p, idx_bytes=s["idx"], reserved=0)
    if how == "dev":
        t = Buf(1, F, fill=np.array([tau], F))
        st = lib.vbnn_prune_compress(h, _code(dtype), n, d, sp, t.p, -1.0)
    else:
        st = lib.vbnn_prune_compress(h, _code(dtype), n, d, sp, None, float(tau))
    return st, [{k: b[k].read(k) for k in ("row_ptr", "cols", "mu_v", "var_v", "nnz") if b[k] is not None} for b in bufs]


def _compress_expect(s, dtype, csr):
    O, I = s["m"].shape
    dt, room, w = _np_dt(dtype), s["room"] + SPARE, min(s["cap"], csr["nnz"])
    e = dict(row_ptr=_sentinel(O + 2, u32), nnz=_sentinel(2, u32), cols=_sentinel(room, u16 if s["idx"] == 2 else u32),
             mu_v=_sentinel(room, dt))
    e["row_ptr"][:O + 1] = csr["row_ptr"]                                  # the true counts whatever the capacity
    e["nnz"][0] = csr["nnz"]
    e["cols"][:w] = csr["cols"][:w]
    e["mu_v"][:w] = csr["mu_v"][:w]
    if s["var"]:
        e["var_v"] = _sentinel(room, dt)
        e["var_v"][:w] = csr["var_v"][:w]
    return e


def _dense(got, O, I, nnz):
    csr = dict(row_ptr=got["row_ptr"][:O + 1], cols=got["cols"][:nnz].astype(np.int64), mu_v=got["mu_v"][:nnz],
               var_v=got["var_v"][:nnz], nnz=nnz)
    return csr_to_dense(csr, O, I), csr_to_dense(csr, O, I, which="var_v")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", C_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compress(shape, dtype):
    O, I = shape
    m, l, v, keys, tie = _with_ties(*_params(O, I, 20 * O + I), seed=O + 2 * I, empty_rows=True)
    prep = _dev_prep(m, l, dtype)
    for tau in (tie, F(np.inf), F(0), F(np.nan)):
        csr = P.csr_build(keys, tau, prep[0], prep[1])
        nnz = csr["nnz"]
        if tau == tie and O >= 10:
            assert (np.diff(csr["row_ptr"].astype(np.int64)) == 0).any() and nnz > 0      # empty rows among others
        if np.isinf(tau):
            assert nnz == 0                                                                # all rows empty
        cols = {}
        for idx, cap, var in [(i, c, True) for i in (2, 4) for c in dict.fromkeys([nnz, max(nnz - 1, 0), 0])] + [(4, nnz, False)]:
            s = dict(m=m, l=l, idx=idx, cap=cap, room=nnz, var=var)
            tag = f"compress {O}x{I} {dtype} tau={tau} idx={idx} cap={cap} of {nnz} var={var}"
            how = "dev" if idx == 2 else "host"
            (st, (a,)), (st2, (b,)) = _compress([s], dtype, tau, how), _compress([s], dtype, tau, how)
            assert st == 0 and st2 == 0, tag
            _same_runs(tag, a, b)
            e = _compress_expect(s, dtype, csr)
            assert a.keys() == e.keys()
            for k in e:
                _same(f"{tag} {k}", a[k], e[k])
            if cap == nnz and var:
                cols[idx] = a["cols"][:nnz].astype(np.int64)
                packed = _pack([dict(m=m, l=l, ld=I, mask=None, out_off=0, in_off=0)], dtype, tau, how)[0]
                mu_d, var_d = _dense(a, O, I, nnz) if nnz else (np.zeros((O, I), _np_dt(dtype)),) * 2
                _same(f"{tag}: scattered mu_v is mu_p", mu_d, packed["mu"][:O * I].reshape(O, I))
                _same(f"{tag}: scattered var_v is var_p", var_d, packed["var"][:O * I].reshape(O, I))
        assert np.array_equal(cols[2], cols[4])


def test_compress_two_byte_indices_at_their_limit():
    L, lib, h = _ctx()
    O, I = 2, 65536
    m, l = _params(O, I, 65536)
    m[:, I - 1] = F(100.0)                                                 # column 65535 is kept
    v = _dev_exp(l)
    keys, prep = P.weight_key32(m, v), _dev_prep(m, l, "f32")
    tau = F(np.partition(keys.ravel(), O * I // 2)[O * I // 2])
    csr = P.csr_build(keys, tau, prep[0], prep[1])
    assert (csr["cols"] == I - 1).sum() == 2
    for idx in (2, 4):
        s = dict(m=m, l=l, idx=idx, cap=csr["nnz"], room=csr["nnz"], var=True)
        (st, (a,)), (_, (b,)) = _compress([s], "f32", tau, "host"), _compress([s], "f32", tau, "host")
        assert st == 0
        _same_runs("compress I=65536", a, b)
        e = _compress_expect(s, "f32", csr)
        for k in e:
            _same(f"compress I=65536 idx={idx} {k}", a[k], e[k])
        assert (a["cols"][:csr["nnz"]] == 65535).sum() == 2
    m2, l2 = _params(1, 65537, 7)
    s = dict(m=m2, l=l2, idx=2, cap=4, room=4, var=True)
    st, (a,) = _compress([s], "f32", F(0), "host")
    assert st != 0                                                         # refused, and nothing written
    for k in a:
        assert (_bits(a[k]) == _bits(_sentinel(a[k].size, a[k].dtype))).all(), k
    s["idx"] = 4
    assert _compress([s], "f32", F(np.inf), "host")[0] == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_compress_eight_layers(dtype):
    specs, csrs = [], []
    data = []
    for j, (O, I) in enumerate(C_SHAPES[1:9]):
        m, l = _params(O, I, 500 + j)
        m[3::5] *= F(1e-6)
        v = _dev_exp(l)
        data.append((m, l, P.weight_key32(m, v), _dev_prep(m, l, dtype)))
    pool = np.concatenate([q[2].ravel() for q in data])
    tau = F(np.partition(pool, pool.size // 2)[pool.size // 2])
    for j, (m, l, keys, prep) in enumerate(data):
        csr = P.csr_build(keys, tau, prep[0], prep[1])
        csrs.append(csr)
        specs.append(dict(m=m, l=l, idx=2 if j % 2 else 4, cap=[csr["nnz"], max(csr["nnz"] - 1, 0), 0][j % 3], room=csr["nnz"],
                          var=j != 5))
    (st, a), (st2, b) = _compress(specs, dtype, tau, "dev"), _compress(specs, dtype, tau, "host")
    assert st == 0 and st2 == 0
    for j, s in enumerate(specs):
        _same_runs(f"compress 8 layers, layer {j}", a[j], b[j])
        e = _compress_expect(s, dtype, csrs[j])
        assert a[j].keys() == e.keys()
        for k in e:
            _same(f"compress 8 layers {dtype}, layer {j} {k}", a[j][k], e[k])


# ------------------------------------------------------------------------------------------------ vbnn_unit_snr
U_SHAPES = [(1, 1), (5, 3), (1030, 7), (4, 1025), (3, 2048), (3, 2049)]      # the last three: a workgroup per row


def _unit_snr(layers, offs):
    """One vbnn_unit_snr over `layers` ((m, l) pairs), every base offs[j] = (means, lvars, key) floats off alignment."""
    L, lib, h = _ctx()
    n = len(layers)
    d, keep = (L.UnitDesc * n)(), []
    for j, (m, l) in enumerate(layers):
        O, I = m.shape
        om, ol, ok = offs[j]
        dm, dl, key = Buf(O * I, F, 4 * om, m), Buf(O * I, F, 4 * ol, l), Buf(O, F, 4 * ok, extra=4)
        keep.append((dm, dl, key))
        d[j] = L.UnitDesc(means=dm.p, lvars=dl.p, O=O, I=I, key=key.p, keep=None, n_keep=None)
    L.check(lib.vbnn_unit_snr(h, n, d))
    return [k[2].read("key") for k in keep]


def _unit_expect(m, l):
    O, I = m.shape
    k, other, close = P.unit_key_value(m, _dev_exp(l))
    assert not close.any(), f"{O}x{I}: a quotient within the reordering distance of a rounding midpoint: pick another seed"
    e = _sentinel(O + 4, F)
    e[:O] = k
    _use("unit_key", (np.abs(k.astype(f8) - U.unit_key64(m, l)) / (P.unit_rel(I) * U.unit_key64(m, l))).max())
    return e


@pytest.mark.parametrize("shape", U_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unit_snr(shape):
    O, I = shape
    m, l = _params(O, I, 7 * O + I)
    e = _unit_expect(m, l)
    for off in itertools.product((0, 1), repeat=3):
        a, b = _unit_snr([(m, l)], [off])[0], _unit_snr([(m, l)], [off])[0]
        _same(f"unit_snr {O}x{I} offsets {off}: two runs", a, b)
        _same(f"unit_snr {O}x{I} offsets {off}", a, e)
    if I == 3:                                                             # NaN parameters and 0 / 0: the canonical quiet NaN
        m2, l2 = m.copy(), l.copy()
        m2[1, 2], m2[3], l2[3] = np.nan, 0.0, -200.0
        got = _unit_snr([(m2, l2)], [(0, 0, 0)])[0]
        assert _bits(got)[1] == 0x7fc00000 and _bits(got)[3] == 0x7fc00000
        _same("unit_snr beside the NaNs", got[[0, 2, 4]], e[[0, 2, 4]])


def test_unit_snr_six_layers_in_one_call():
    layers = [_params(O, I, 7 * O + I) for O, I in U_SHAPES]
    offs = [((j >> 0) & 1, (j >> 1) & 1, (j >> 2) & 1) for j in range(len(layers))]
    a, b = _unit_snr(layers, offs), _unit_snr(layers, offs)
    for j, (m, l) in enumerate(layers):
        _same(f"unit_snr layer {j}: two runs", a[j], b[j])
        _same(f"unit_snr layer {j}", a[j], _unit_expect(m, l))


# ------------------------------------------------------------------------------------------------ vbnn_unit_select / vbnn_unit_index
def _unit_desc(keys):
    L, lib, h = _ctx()
    n = len(keys)
    d, bufs = (L.UnitDesc * n)(), []
    for j, k in enumerate(keys):
        b = dict(key=Buf(k.size, F, fill=k, extra=4), keep=Buf(k.size, u32, extra=4), n_keep=Buf(1, u32, extra=1))
        bufs.append(b)
        d[j] = L.UnitDesc(means=None, lvars=None, O=k.size, I=1, key=b["key"].p, keep=b["keep"].p, n_keep=b["n_keep"].p)
    return d, bufs


def _unit_index(keys, taus, how, multiple):
    """One vbnn_unit_index over the key arrays: per layer the WHOLE keep buffer (O + 4 words) and n_keep (2 words)."""
    L, lib, h = _ctx()
    d, bufs = _unit_desc(keys)
    if how == "dev":
        t = Buf(len(keys), F, fill=np.asarray(taus, F))
        L.check(lib.vbnn_unit_index(h, len(keys), d, t.p, -1.0, int(multiple)))
    else:
        assert len(set(_bits(np.asarray(taus, F)).tolist())) == 1
        L.check(lib.vbnn_unit_index(h, len(keys), d, None, float(taus[0]), int(multiple)))
    out = [dict(keep=b["keep"].read("keep"), n_keep=b["n_keep"].read("n_keep")) for b in bufs]
    for b, k in zip(bufs, keys):
        _same("keys (unchanged)", b["key"].read("key")[:k.size], k)
    return out


def _index_expect(keys, tau, multiple):
    want = U.kept(keys, tau, multiple)
    e = dict(keep=_sentinel(keys.size + 4, u32), n_keep=_sentinel(2, u32))
    e["keep"][:want.size] = want                                           # the words past n keep the sentinel
    e["n_keep"][0] = want.size
    return e


def _index_case(tag, keys, tau, multiple, hows=("host", "dev")):
    e = _index_expect(keys, tau, multiple)
    for how in hows:
        a, b = _unit_index([keys], [tau], how, multiple)[0], _unit_index([keys], [tau], how, multiple)[0]
        _same_runs(f"{tag} {how}", a, b)
        for k in e:
            _same(f"{tag} {how} {k}", a[k], e[k])
    return int(e["n_keep"][0])


def _unit_select(keys, ks):
    """vbnn_unit_select over the key arrays at every k of ks: (len(ks), n_layers + 1) floats, the last column spare."""
    L, lib, h = _ctx()
    d, bufs = _unit_desc(keys)
    n = len(keys)
    tau = Buf(len(ks) * (n + 1), F)
    for j, k in enumerate(ks):
        L.check(lib.vbnn_unit_select(h, n, d, int(k), tau.at(j * (n + 1))))
    return tau.read("tau").reshape(len(ks), n + 1)


def _select_case(tag, keys, ks):
    pool = np.concatenate(keys)
    n = len(keys)
    e = _sentinel(len(ks) * (n + 1), F).reshape(len(ks), n + 1)
    srt = np.sort(U.code(pool))
    for j, k in enumerate(ks):
        assert srt[k] == _bits(np.array([U.kth(pool, k)], F))[0]
        e[j, :n] = srt[k:k + 1].view(F)[0]                                 # one copy per listed layer
    a, b = _unit_select(keys, ks), _unit_select(keys, ks)
    _same(f"{tag}: two runs", a, b)
    _same(tag, a, e)


def _key_sets(O, seed):
    rng = np.random.default_rng(seed)
    full = P.population("full", O, seed=seed).view(F).copy()
    if O >= 8:
        full[rng.permutation(O)[:4]] = np.array([0x7fc00001, 0x7fffffff, 0x7f800001, 0x7fc00000], u32).view(F)
    low16 = (np.uint32(0x3f000000) | rng.integers(0, 1 << 16, O).astype(u32)).view(F)
    return dict(full=full, equal=np.full(O, 0.25, F), two=P.tie_keys(O, O // 3, seed), low16=low16)


def _spread(O, seed):
    if O <= 65:
        return list(range(O))
    rng = np.random.default_rng(seed)
    return sorted(set([0, 1, O // 3, O // 2, O - 2, O - 1] + rng.integers(0, O, 10).tolist()))


@pytest.mark.parametrize("O", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 5000, 16385])
def test_unit_select_and_index(O):
    per = P.run_length(O)
    L, lib, h = _ctx()
    for name, keys in _key_sets(O, O).items():
        _select_case(f"unit_select O={O} {name}", [keys], _spread(O, O))
        fin = keys[~np.isnan(keys)]
        tie = F(np.sort(fin)[fin.size // 2]) if fin.size else F(1)
        for tau in (F(np.nan), F(0), F(np.inf), tie):
            for multiple in (1, 4, 256, O + 1):
                _index_case(f"unit_index O={O} {name} tau={tau} multiple={multiple}", keys, tau, multiple)
    d, bufs = _unit_desc([np.zeros(O, F)])
    t = Buf(1, F)
    assert lib.vbnn_unit_select(h, 1, d, O, t.p) != 0 and lib.vbnn_unit_select(h, 1, d, -1, t.p) != 0
    # the kept ties: 1, 63, 64, 65 (inside a 64-unit chunk, on its boundary, just past it), per and per + 1 (a wave's whole run, one more)
    for t_keep in (1, 63, 64, 65, per, per + 1):
        if t_keep > O:
            continue
        n = _index_case(f"unit_index O={O} all equal, {t_keep} ties kept", np.full(O, 0.25, F), F(np.inf), t_keep, hows=("dev",))
        assert n == t_keep
        H = (O - t_keep) // 2
        if H >= 1:
            two = P.tie_keys(O, H, seed=t_keep)
            n = _index_case(f"unit_index O={O} two-valued, {H} above and {t_keep} ties kept", two, F(0.5), H + t_keep, hows=("dev",))
            assert n == H + t_keep


def test_unit_select_and_index_eight_layers():
    Os = [1, 63, 64, 65, 1023, 1024, 1025, 5000]
    names = ["full", "two", "equal", "low16"]
    keys = [_key_sets(O, 40 + j)[names[j % 4]] for j, O in enumerate(Os)]
    pool = np.concatenate(keys)
    _select_case("unit_select 8 layers", keys, _spread(pool.size, 5))
    taus = [F(np.inf), F(0.5), F(np.inf), F(np.nan), F(U.kth(keys[4], 500)), F(0.25), F(0.5), F(U.kth(keys[7], 2500))]
    for multiple in (1, 4, 256):
        a, b = _unit_index(keys, taus, "dev", multiple), _unit_index(keys, taus, "dev", multiple)
        for j, k in enumerate(keys):
            _same_runs(f"unit_index 8 layers, layer {j}", a[j], b[j])
            e = _index_expect(k, taus[j], multiple)
            for q in e:
                _same(f"unit_index 8 layers multiple={multiple}, layer {j} {q}", a[j][q], e[q])
    one = F(U.kth(pool, pool.size // 2))
    a = _unit_index(keys, [one] * 8, "host", 4)
    for j, k in enumerate(keys):
        e = _index_expect(k, one, 4)
        for q in e:
            _same(f"unit_index 8 layers tau_host, layer {j} {q}", a[j][q], e[q])


def test_engine_prune_units_wider_than_one_chunk_per_wave(oracle):
    """FusedMLP.prune_units on 16-1100-2100-10: k_unit_index's waves own 128 and 192 units. Then compact: a bit copy."""
    from tests.test_prune_gpu import host, make, same_bits
    from tests.test_units_gpu import _check_compact, unit_keys
    eng = make(oracle, "odd", input_size=16, hidden=[1100, 2100])
    assert [P.run_length(v.O) for v in eng.vb] == [128, 192]
    keys = unit_keys(eng)
    for kw in (dict(fraction=0.5, scope="global", multiple=1), dict(fraction=0.9, scope="layer", multiple=4),
               dict(fraction=0.3, scope="global", multiple=256), dict(fraction=1.0, scope="layer", multiple=1)):
        r = eng.prune_units(**kw)
        tau, keep = U.prune_units(keys, **kw)
        assert same_bits(np.float32(r.tau), np.float32(tau)), (kw, r.tau, tau)
        for li in range(2):
            assert np.array_equal(host(r.keep[li]).astype(u32), keep[li]), (kw, li)
        _check_compact(eng, r, eng.compact(r))


# ------------------------------------------------------------------------------------------------ vbnn_unit_gather
def _gather(src, O, I, rows, n_rows, cols, n_cols, src_off, dst_off):
    """One vbnn_unit_gather. src: dict means (+ lvars, bias) of (O + 4) x I (and O + 4): four spare rows behind O."""
    L, lib, h = _ctx()
    b = {k: Buf(O * I if k != "bias" else O, F, 4 * src_off if k != "bias" else 0, v[:O], extra=4 * I if k != "bias" else 4)
         for k, v in src.items()}
    for k, v in src.items():
        b[k].set(v)                                                        # the spare rows hold other data, not the sentinel
    dst = {k: Buf(n_rows * n_cols if k != "bias" else n_rows, F, 4 * dst_off if k != "bias" else 0, extra=4) for k in src}
    br = None if rows is None else Buf(len(rows), u32, fill=np.asarray(rows, u32))
    bc = None if cols is None else Buf(len(cols), u32, fill=np.asarray(cols, u32))
    g = lambda q, k: q[k].p if k in q else None                            # noqa: E731
    a = L.UnitGatherArgs(means=b["means"].p, lvars=g(b, "lvars"), bias=g(b, "bias"), O=O, I=I, rows=br.p if br else None,
                         n_rows=n_rows, cols=bc.p if bc else None, n_cols=n_cols, dst_means=dst["means"].p,
                         dst_lvars=g(dst, "lvars"), dst_bias=g(dst, "bias"))
    L.check(lib.vbnn_unit_gather(h, C.byref(a)))
    return {k: q.read("dst_" + k) for k, q in dst.items()}


@pytest.mark.parametrize("n_cols", [1, 3, 4, 5, 67])
def test_unit_gather(n_cols):
    O = 9
    BIG = 0xFFFFFFFF
    rng = np.random.default_rng(n_cols)
    for use_rows, use_cols, dual, with_bias in itertools.product((False, True), repeat=4):
        I = n_cols + 3 if use_cols else n_cols
        n_rows = 6 if use_rows else O
        rows = [3, O, 0, O + 3, BIG, 7] if use_rows else None             # O, O + 3 and 0xFFFFFFFF are read as O - 1
        cols = None
        if use_cols:
            cols = rng.permutation(I)[:n_cols].astype(np.int64)
            cols[:3] = [BIG, I, I + 3][:min(3, n_cols)]                    # read as I - 1
        src = dict(means=P.means_of(P.population("full", (O + 4) * I, seed=n_cols)).reshape(O + 4, I))
        if dual:
            src["lvars"] = P.means_of(P.population("full", (O + 4) * I, seed=n_cols + 100)).reshape(O + 4, I)
        if with_bias:
            src["bias"] = P.means_of(P.population("full", O + 4, seed=n_cols + 200))
        for src_off, dst_off in itertools.product((0, 1), repeat=2):
            tag = f"gather n_cols={n_cols} rows={use_rows} cols={use_cols} dual={dual} bias={with_bias} offsets {src_off},{dst_off}"
            a = _gather(src, O, I, rows, n_rows, cols, n_cols, src_off, dst_off)
            _same_runs(tag, a, _gather(src, O, I, rows, n_rows, cols, n_cols, src_off, dst_off))
            assert a.keys() == src.keys()
            for k, v in src.items():
                want = P.gather_ref(v[:O], rows, cols, O, I)
                e = _sentinel(want.size + 4, F)
                e[:want.size] = want.ravel()
                _same(f"{tag} dst_{k}", a[k], e)
