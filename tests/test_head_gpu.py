"""Every form of the classifier head (head.hip: forward by type, from slots, the one-launch step, the four tile backward
instantiations per type, the streaming backward, both finishes) and the small kernels of the classification loss path
(vbnn_logsoftmax_nll, vbnn_nll_forward / _backward, vbnn_logsoftmax_backward, vbnn_relu_*, vbnn_acc_grad_bias), through direct
C ABI calls, against the float64 reference of tests/_head_np.py (itself held to the oracle by test_head_ref.py).

Every head case first asserts WHICH form ran (vbnn_debug_get(VBNN_DEBUG_LAST_HEAD_FORM)); where the form depends on the CU
count the expectation is computed from vbnn_ctx_stream's n_cus_out by the same rule the host states. Outputs are allocated with
pad elements and a spare row of a sentinel, which must come back untouched; inputs keep zero pads.

What is compared how:
  (a) bit for bit   integer-valued operands (h 0..3, w3 / g -3..3, r +-0.5 / 1 / 2, integer bias): every sum is exact in fp32 and
                    |gx| <= 144 is exact in bf16, so gradInput, its transposes, gradWeight, both bias gradients and the logits
                    are compared as bits, every element; hits exactly. out, g_logits and the loss hold expf: the derived
                    bound of _head_np.row_bounds.
  (b) the bound     log-softmax edges on exact integer logits: a peak 120 above the rest, the target 100 below the maximum, a
                    bias of +-30000, ties, out-of-range targets, a NaN row -- on all kernels that hold the row arithmetic.
  (c) element-wise  random real operands: logits 4e-6 (|h| |w3|^T) + 1e-6; fp32 sums 2e-6 (sum of absolute terms) + 1e-6 |base|;
                    bf16 outputs 2^-8 |exact| + the fp32 sum bound of that element -- never relative to a matrix maximum.
  (d) the small pieces, bitwise on integer data and with the sum bound on random data.
The streaming backward takes whole 64-row tiles only (it needs FULL), so 32 x 128 and 1056 x 1024 run the tile form whatever is
forced: they are kept as tile-form cases, and 64 x 128 and the smallest N with a short last row chunk on this device (2176 rows
at 256 CUs) stand in for them as the streaming cases. The last test prints, per group, the largest fraction of each bound the
device used."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _head_np as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
SENT = 7.0
DTYPES = ("f32", "bf16")
LAST_HEAD_FORM, HEAD_BACKWARD = 11, 10                     # VBNN_DEBUG_LAST_HEAD_FORM, VBNN_DEBUG_HEAD_BACKWARD
FORWARD, SLOTS, STEP, TILE, STREAM = 1, 2, 3, 4, 5         # VBNN_HEAD_ENTRY_*
FIN_NONE, FIN_INLINE, FIN_KERNEL = 0, 1, 2                 # VBNN_HEAD_FINISH_*
SCRATCH_FLOATS = 1 << 22                                   # the context's reduction scratch (caps the row chunks of a backward)
CNT_TILES_MAX = 1008
SEEN = set()                                               # every form asserted by a case of this module
USED = {}                                                  # (group, quantity) -> largest fraction of its bound used


def form(entry, bf16=0, vec=0, full=0, cp=0, finish=0):
    """VBNN_HEAD_FORM of include/vbnn_hip.h."""
    return entry | (bf16 << 4) | (vec << 5) | (full << 6) | (cp << 8) | (finish << 16)


def form_name(f):
    return (f"entry {f & 15} bf16 {(f >> 4) & 1} VEC {(f >> 5) & 1} FULL {(f >> 6) & 1} CP {(f >> 8) & 255} finish {(f >> 16) & 3}")


def _mods():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, nn


def _ctx():
    L, nn = _mods()
    return L, L.lib(), nn.Context.get().h


def n_cus():
    L, lib, h = _ctx()
    sp, n = C.c_void_p(), C.c_int()
    L.check(lib.vbnn_ctx_stream(h, C.byref(sp), C.byref(n)))
    return n.value


def assert_form(want):
    _, lib, _ = _ctx()
    got = lib.vbnn_debug_get(LAST_HEAD_FORM)
    assert got == want, f"ran [{form_name(got)}], expected [{form_name(want)}]"
    SEEN.add(got)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _tdt(dtype):
    return {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]


def _code(dtype):
    L, _ = _mods()
    return {"f32": L.F32, "bf16": L.BF16}[dtype]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host(t):
    """A device tensor as float32 / float64 / int values on the host (bf16 widened exactly)."""
    if t.dtype == torch.bfloat16:
        return t.float().cpu().numpy()
    return t.cpu().numpy()


def packed(a, dtype, ld, rows=None):
    """A zero-padded operand of `dtype` with pitch ld holding the values of a (which the type holds exactly)."""
    a = np.asarray(a, F)
    t = torch.zeros((rows or a.shape[0], ld), dtype=_tdt(dtype), device="cuda")
    t[:a.shape[0], :a.shape[1]] = torch.from_numpy(a).cuda().to(_tdt(dtype))
    return t


def sentinel(rows, ld, tdt=torch.float32):
    """An output of rows x ld plus one spare row, all sentinel."""
    return torch.full((rows + 1, ld), SENT, dtype=tdt, device="cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tail_buf(values):
    """A dense float32 output (a gradient) holding `values`, followed by 16 sentinel words."""
    v = np.asarray(values, F).ravel()
    t = torch.full((v.size + 16,), SENT, dtype=torch.float32, device="cuda")
    t[:v.size] = dev(v)
    return t


def tail_data(name, t, shape):
    a = t.cpu().numpy()
    n = int(np.prod(shape))
    assert (a[n:] == SENT).all(), f"{name}: written past its end"
    return a[:n].reshape(shape)


def data(name, t, rows, cols):
    """The rows x cols data of an output; its pads and spare row must still be the sentinel."""
    a = _host(t)
    assert (a[:rows, cols:] == SENT).all() and (a[rows:] == SENT).all(), f"{name}: a pad element or the spare row was written"
    return a[:rows, :cols]


def bitwise(name, got, want):
    got, want = np.asarray(got), np.asarray(want).astype(np.asarray(got).dtype)
    bad = np.argwhere(_u(got) != _u(want))
    if bad.size:
        i = tuple(int(q) for q in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} differ; first at {i}: got {got[i]!r} want {want[i]!r}")


def within(name, got, want, bound, group):
    """|got - want| <= bound element by element (a zero bound asks for equality); records the fraction of the bound used."""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    bound = np.broadcast_to(np.atleast_1d(np.asarray(bound, np.float64)), got.shape)
    diff = np.abs(got - want)
    bad = np.argwhere(~(diff <= bound))
    if bad.size:
        i = tuple(int(q) for q in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} outside their bound; first at {i}: got {got[i]!r} want {want[i]!r} "
                             f"diff {diff[i]:.3e} bound {bound[i]:.3e}")
    pos = bound > 0
    if pos.any():
        USED[(group, name)] = max(USED.get((group, name), 0.0), float((diff[pos] / bound[pos]).max()))


# ------------------------------------------------------------------------------------------------ forward entries
class Rows:
    """The outputs every forward entry shares, with sentinels; loss / hits start as `base` (garbage unless accumulating)."""

    def __init__(self, N, Cn, logits=True, out=True, base=(123.456, -77)):
        self.N, self.C = N, Cn
        self.logits = sentinel(N, Cn) if logits else None
        self.out = sentinel(N, Cn) if out else None
        self.g = sentinel(N, Cn)
        self.loss = torch.tensor([base[0], SENT], dtype=torch.float64, device="cuda")
        self.hits = torch.tensor([base[1], 7], dtype=torch.int32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        res = {k: data(k, t, self.N, self.C) for k, t in (("logits", self.logits), ("out", self.out), ("g_logits", self.g)) if t is not None}
        loss, hits = self.loss.cpu().numpy(), self.hits.cpu().numpy()
        assert loss[1] == SENT and hits[1] == 7, "the word after an accumulator was written"
        res["loss"], res["hits"] = float(loss[0]), int(hits[0])
        return res


def head_forward(dtype, h, w3, bias, target, inv_n, Cn, rpd=0, accumulate=0, **kw):
    L, lib, ctx = _ctx()
    N, H = h.shape
    ld = L.pad_ld(H)
    th, tw = packed(h, dtype, ld), packed(w3, dtype, ld)
    tb, tt = (None if bias is None else dev(np.asarray(bias, F))), dev(np.asarray(target, np.int32))
    o = Rows(N, Cn, **kw)
    L.check(lib.vbnn_head_forward(ctx, _code(dtype), _p(th), ld, _p(tw), ld, _p(tb), _p(tt), N, H, Cn, float(inv_n), _p(o.logits),
                                  _p(o.out), _p(o.g), accumulate, _p(o.loss), _p(o.hits), rpd))
    assert_form(form(FORWARD, bf16=int(dtype == "bf16")))
    return o.host()


def head_slots(slots, bias, target, inv_n, Cn, rpd=0, accumulate=0, **kw):
    L, lib, ctx = _ctx()
    n_slots, N, _ = slots.shape
    ts, tt = dev(np.asarray(slots, F)), dev(np.asarray(target, np.int32))
    tb = None if bias is None else dev(np.asarray(bias, F))
    o = Rows(N, Cn, **kw)
    L.check(lib.vbnn_head_forward_slots(ctx, _p(ts), n_slots, _p(tb), _p(tt), N, Cn, float(inv_n), _p(o.logits), _p(o.out), _p(o.g),
                                        accumulate, _p(o.loss), _p(o.hits), rpd))
    assert_form(form(SLOTS))
    return o.host()


def logsoftmax_nll(lg, target, inv_n, out=True, g=True):
    """vbnn_logsoftmax_nll on logits of pitch C + 3; it ADDS to loss / hits, which start at 0."""
    L, lib, ctx = _ctx()
    N, Cn = lg.shape
    tl = packed(lg, "f32", Cn + 3)
    o = Rows(N, Cn, logits=False, out=out, base=(0.0, 0))
    L.check(lib.vbnn_logsoftmax_nll(ctx, _p(tl), Cn + 3, _p(dev(np.asarray(target, np.int32))), N, Cn, float(inv_n), _p(o.out),
                                    _p(o.g if g else None), _p(o.loss), _p(o.hits)))
    res = o.host() if g else {k: v for k, v in o.host().items() if k != "g_logits"}
    res["logits"] = np.asarray(lg, F)
    return res


def check_rows(res, lg, target, inv_n, group, rpd=0, base=None):
    """The outputs of a forward entry against the reference on the exact float32 logits lg (bias included)."""
    ref = R.criterion(lg, target, inv_n, rpd, base)
    b_out, b_g, b_loss = R.row_bounds(lg, target, inv_n, rpd)
    if "logits" in res:
        bitwise("logits", res["logits"], np.asarray(lg, F))
    assert res["hits"] == ref["hits"], f"hits: got {res['hits']} want {ref['hits']}"
    if "out" in res:
        within("out", res["out"], ref["out"], b_out, group)
    if "g_logits" in res:
        within("g_logits", res["g_logits"], ref["g_logits"], b_g, group)
    within("loss", res["loss"], ref["loss"], b_loss + (0.0 if base is None else 1e-12 * abs(base[0])), group)
    return ref


def exact_logits(o):
    return (o["h"].astype(np.float64) @ o["w3"].astype(np.float64).T + (0 if o.get("bias") is None else o["bias"])).astype(F)


# ------------------------------------------------------------------------------------------------ (a) forward, integer operands
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(R.FWD_SHAPES)), ids=[f"N{n}-H{h}-C{c}-rpd{r}" for n, h, c, r in R.FWD_SHAPES])
def test_forward_on_integer_operands(dtype, i):
    N, H, Cn, rpd = R.FWD_SHAPES[i]
    o = R.int_operands(N, H, Cn, 100 + i)
    target, inv_n = o["target"][:rpd or N], F(1.0 / (rpd or N))
    res = head_forward(dtype, o["h"], o["w3"], o["bias"], target, inv_n, Cn, rpd)
    check_rows(res, exact_logits(o), target, inv_n, "a", rpd)


@pytest.mark.parametrize("dtype,H", [("f32", 3456), ("bf16", 6912)])
def test_forward_runs_all_four_unrolled_k_loops(dtype, H):
    """27 K steps per wave: 16 + 8 + 2 + 1."""
    o = R.int_operands(17, H, 10, 7)
    res = head_forward(dtype, o["h"], o["w3"], o["bias"], o["target"], F(1 / 17), 10)
    check_rows(res, exact_logits(o), o["target"], F(1 / 17), "a")


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_optional_arguments_and_accumulation(dtype):
    """bias / logits / out NULL in turn; accumulate = 0 onto garbage, then accumulate = 1 onto its result."""
    o = R.int_operands(47, 33, 10, 21)
    inv_n = F(1 / 47)
    nobias = dict(o, bias=None)
    res = head_forward(dtype, o["h"], o["w3"], None, o["target"], inv_n, 10)
    check_rows(res, exact_logits(nobias), o["target"], inv_n, "a")
    for kw in (dict(logits=False), dict(out=False), dict(logits=False, out=False)):
        res = head_forward(dtype, o["h"], o["w3"], o["bias"], o["target"], inv_n, 10, **kw)
        assert ("logits" in res) == kw.get("logits", True) and ("out" in res) == kw.get("out", True)
        first = check_rows(res, exact_logits(o), o["target"], inv_n, "a")
    base = (2.5, 1000)
    res = head_forward(dtype, o["h"], o["w3"], o["bias"], o["target"], inv_n, 10, accumulate=1, base=base)
    ref = check_rows(res, exact_logits(o), o["target"], inv_n, "a", base=base)
    assert ref["hits"] == first["hits"] + 1000


@pytest.mark.parametrize("N", [1, 17, 47])
@pytest.mark.parametrize("n_slots", [1, 2, 3, 16, 19, 35])
def test_forward_from_slots(n_slots, N):
    """Real-valued slots, so the order of the float32 sum shows in the bits of the logits."""
    rng = np.random.default_rng(n_slots * 100 + N)
    Cn = (10, 16, 7)[N % 3]
    slots = rng.standard_normal((n_slots, N, 16)).astype(F)
    bias, target = rng.standard_normal(Cn).astype(F), rng.integers(0, Cn, N).astype(np.int32)
    lg = R.slot_logits(slots, bias)[:, :Cn]
    res = head_slots(slots, bias, target, F(1.0 / N), Cn)
    check_rows(res, lg, target, F(1.0 / N), "a")
    rpd = max(N // 3, 1)
    res = head_slots(slots, None, target[:rpd], F(1.0 / rpd), Cn, rpd=rpd, accumulate=1, base=(-1.0, 5), out=False)
    check_rows(res, R.slot_logits(slots, None)[:, :Cn], target[:rpd], F(1.0 / rpd), "a", rpd=rpd, base=(-1.0, 5))


# ------------------------------------------------------------------------------------------------ backward
def expect_backward(dtype, N, H, Cn, vec, r_f32, sums, transposes, has_g_prev, stream_mode):
    """The form head_backward_t picks, restated from its rule with this device's CU count."""
    cus = n_cus()
    tiles_c, tiles_r = -(-H // 64), -(-N // 64)
    cap = SCRATCH_FLOATS // (Cn * H + Cn + H)
    Rc = min(-(-2 * cus // tiles_c), tiles_r)
    if sums:
        Rc = min(Rc, cap)
    Rc = max(Rc, 1)
    rpc = -(-tiles_r // Rc) * 64
    Rc = -(-N // rpc)
    full = vec and H % 64 == 0 and N % 64 == 0
    inline = sums and tiles_c * Rc <= cus and tiles_c <= CNT_TILES_MAX
    if dtype == "bf16" and (stream_mode == 1 or (stream_mode == -1 and not inline)) and full and Cn <= 12 and not r_f32 and \
            has_g_prev and not transposes and H % 128 == 0 and N % 32 == 0:
        return form(STREAM, bf16=1, finish=FIN_INLINE if sums else FIN_NONE)
    cp = 12 if (full and Cn <= 12 and not r_f32) else 0
    return form(TILE, bf16=int(dtype == "bf16"), vec=int(vec), full=int(full), cp=cp,
                finish=FIN_NONE if not sums else FIN_INLINE if inline else FIN_KERNEL)


def stream_chunks(N, H):
    """(Rs, rows per chunk) of the streaming form on this device."""
    cb = H // 128
    Rs = max(-(-n_cus() // cb), 1)
    rpc = -(-(-(-N // Rs)) // 32) * 32
    return -(-N // rpc), rpc


def head_backward(dtype, o, N, H, Cn, r="T", transposes=False, pad=8, pad_r=0, relu_mask=1, accumulate=0, skip=(), gv=True,
                  stream_mode=-1, want_form=None):
    """One vbnn_head_backward on the operands o. r: "T" (the operand type), "f32" or None. pad: g_prev's pitch is H + pad, pad_r:
    r's pitch is its 64-multiple + pad_r -- a pitch that is no multiple of 8 selects the element-by-element form. skip: which of
    gradWeight / gradBias / gradBias_prev are NULL. Returns the host outputs (pads checked) and the integer bases."""
    L, lib, ctx = _ctx()
    ld = L.pad_ld(H)
    th, tw = packed(o["h"], dtype, ld), packed(o["w3"], dtype, ld)
    tg = dev(o["g"])
    ld_r, tr = 0, None
    if r is not None:
        ld_r = ld + pad_r
        tr = packed(o["r"], dtype if r == "T" else "f32", ld_r)
    ld_gp, ld_gpT = H + pad, (N + 7) // 8 * 8 + 8
    tdt = _tdt(dtype)
    gp = sentinel(N, ld_gp, tdt)
    gvp = sentinel(N, ld_gp, tdt) if (gv and r is not None) else None
    gT = sentinel(H, ld_gpT, tdt) if transposes else None
    gvT = sentinel(H, ld_gpT, tdt) if (transposes and gvp is not None) else None
    rng = np.random.default_rng(5)
    base = dict(gradWeight=rng.integers(-9, 10, (Cn, H)).astype(F), gradBias=rng.integers(-9, 10, (1, Cn)).astype(F),
                gradBias_prev=rng.integers(-9, 10, (1, H)).astype(F))
    flat = {k: tail_buf(v) for k, v in base.items() if k not in skip}
    sums = bool(flat)
    L.check(lib.vbnn_debug_set(HEAD_BACKWARD, stream_mode))
    try:
        L.check(lib.vbnn_head_backward(ctx, _code(dtype), _p(th), ld, _p(tw), ld, _p(tg), N, H, Cn, accumulate, _p(flat.get("gradWeight")),
                                       _p(flat.get("gradBias")), _p(flat.get("gradBias_prev")), relu_mask, _p(tr), ld_r,
                                       int(r == "T"), _p(gp), _p(gvp), ld_gp, _p(gT), _p(gvT), ld_gpT))
    finally:
        L.check(lib.vbnn_debug_set(HEAD_BACKWARD, -1))
    vec = ld_gp % 8 == 0 and (r is None or ld_r % 8 == 0)
    want = expect_backward(dtype, N, H, Cn, vec, r == "f32", sums, transposes, True, stream_mode)
    assert_form(want)
    if want_form is not None:
        assert want == want_form, f"the case was meant for [{form_name(want_form)}], this device runs [{form_name(want)}]"
    torch.cuda.synchronize()
    res = dict(g_prev=data("g_prev", gp, N, H))
    if gvp is not None:
        res["gv_prev"] = data("gv_prev", gvp, N, H)
    if gT is not None:
        res["gT_prev"] = data("gT_prev", gT, H, N)
    if gvT is not None:
        res["gvT_prev"] = data("gvT_prev", gvT, H, N)
    for k, t in flat.items():
        res[k] = tail_data(k, t, base[k].shape)
    return res, {k: (base[k] if accumulate else None) for k in base}


def check_backward_exact(res, o, dtype, relu_mask, r, base):
    ref = R.head_backward(o["h"], o["w3"], o["g"], dtype, relu_mask, None if r is None else o["r"], base=base)
    bitwise("g_prev", res["g_prev"], ref["g_prev"])
    if "gv_prev" in res:
        bitwise("gv_prev", res["gv_prev"], ref["gv_prev"])
    if "gT_prev" in res:
        bitwise("gT_prev", res["gT_prev"], ref["g_prev"].T)
    if "gvT_prev" in res:
        bitwise("gvT_prev", res["gvT_prev"], ref["gv_prev"].T)
    for k in ("gradWeight", "gradBias", "gradBias_prev"):
        if k in res:
            bitwise(k, res[k], ref[k].reshape(res[k].shape))


SCALAR = dict(pad=1)                                       # ld_gp = H + 1: no multiple of 8 -> <false,false>
BWD_CASES = [
    # <true,true,12>
    ("cp12", 64, 64, 12, {}), ("cp12-C1", 64, 64, 1, {}), ("cp12-no-gradWeight", 64, 64, 12, dict(skip=("gradWeight",))),
    ("cp12-accumulate-T", 128, 128, 10, dict(accumulate=1, transposes=True)),
    # <true,true,0>: C in 13..16, or an fp32 r
    ("cp0-C13-nomask", 64, 64, 13, dict(relu_mask=0)), ("cp0-C16", 64, 64, 16, dict(transposes=True)),
    ("cp0-C10-f32-r", 64, 64, 10, dict(r="f32")),
    # <true,false>: ragged tiles, 16-byte accesses
    ("vec-37x70", 37, 70, 10, dict(pad=2)), ("vec-37x70-T", 37, 70, 10, dict(pad=2, transposes=True, accumulate=1)),
    ("vec-65x64-T", 65, 64, 10, dict(transposes=True)), ("vec-65x64-no-gradBias", 65, 64, 16, dict(skip=("gradBias",))),
    ("vec-64x72-T", 64, 72, 10, dict(transposes=True, r="f32")),
    ("vec-64x72-only-g_prev", 64, 72, 10, dict(skip=("gradWeight", "gradBias", "gradBias_prev"), r=None)),
    ("vec-1056x1024", 1056, 1024, 10, {}),                 # 1056 rows are no whole 64-row tiles: never FULL, so never the streaming form either
    # <false,false>: the pitch alone selects it
    ("scalar-37x70", 37, 70, 10, dict(SCALAR, r=None)), ("scalar-37x70-T", 37, 70, 10, dict(SCALAR, transposes=True)),
    ("scalar-65x64-T", 65, 64, 13, dict(SCALAR, transposes=True, accumulate=1)),
    ("scalar-65x64-no-gradBias_prev", 65, 64, 10, dict(SCALAR, skip=("gradBias_prev",))),
    ("scalar-64x72-ld_r", 64, 72, 10, dict(pad_r=4, r="f32")), ("scalar-64x72-T-ld_r", 64, 72, 16, dict(pad_r=2, transposes=True, relu_mask=0)),
    ("scalar-64x64", 64, 64, 12, dict(SCALAR)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_tile_backward_on_integer_operands(dtype, case):
    name, N, H, Cn, kw = case
    o = R.int_operands(N, H, Cn, 300 + N + H + Cn)
    res, base = head_backward(dtype, o, N, H, Cn, stream_mode=0, **kw)
    tag = name.split("-")[0]                               # (the form was asserted inside; here: it is the form the case names)
    _, lib, _ = _ctx()
    got = lib.vbnn_debug_get(LAST_HEAD_FORM)
    want_bits = {"cp12": (1, 1, 12), "cp0": (1, 1, 0), "vec": (1, 0, 0), "scalar": (0, 0, 0)}[tag]
    assert ((got >> 5) & 1, (got >> 6) & 1, (got >> 8) & 255) == want_bits and got & 15 == TILE, f"{name} ran [{form_name(got)}]"
    check_backward_exact(res, o, dtype, kw.get("relu_mask", 1), kw.get("r", "T"), base)


@pytest.mark.parametrize("N,H,Cn,kw", [(32, 128, 12, {}), (64, 128, 12, {}), (64, 256, 1, dict(accumulate=1)), (64, 128, 10, dict(r=None, relu_mask=0)),
                                       (64, 128, 12, dict(skip=("gradWeight", "gradBias", "gradBias_prev"), gv=False))])
def test_streaming_backward_on_integer_operands(N, H, Cn, kw):
    """The streaming form forced (VBNN_DEBUG_HEAD_BACKWARD = 1) at its smallest sizes. It takes whole 64-row tiles only (FULL), so
    the 32-row case is the tile form's even when forced: asserted as such, and checked all the same."""
    o = R.int_operands(N, H, Cn, 400 + N + H + Cn)
    res, base = head_backward("bf16", o, N, H, Cn, stream_mode=1, **kw)
    _, lib, _ = _ctx()
    assert lib.vbnn_debug_get(LAST_HEAD_FORM) & 15 == (STREAM if N % 64 == 0 else TILE)
    check_backward_exact(res, o, "bf16", kw.get("relu_mask", 1), kw.get("r", "T"), base)


def test_streaming_backward_with_a_ragged_last_row_chunk():
    """The default selection at a wide size: the smallest N (whole 64-row tiles, as the streaming form needs) whose last row
    chunk is short on this device -- 2176 rows in chunks of 96 on 256 CUs."""
    H, Cn = 1024, 10
    N = next(n for n in range(64 * (n_cus() // 8), 64 * 200, 64) if (lambda rs, rpc: rs * rpc != n and rpc > 32)(*stream_chunks(n, H)))
    Rs, rpc = stream_chunks(N, H)
    assert Rs * rpc != N and N % 64 == 0
    o = R.int_operands(N, H, Cn, 77)
    res, base = head_backward("bf16", o, N, H, Cn, stream_mode=-1, want_form=form(STREAM, bf16=1, finish=FIN_INLINE))
    check_backward_exact(res, o, "bf16", 1, "T", base)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_backward_with_the_finish_kernel(dtype):
    """One 64-row tile more than the column tiles' CUs: tiles_c * R > CUs, so k_head_backward_finish adds the partials."""
    H, Cn = 1024, 10
    N = 64 * (n_cus() // (H // 64) + 1)
    o = R.int_operands(N, H, Cn, 78)
    res, base = head_backward(dtype, o, N, H, Cn, stream_mode=0, accumulate=1,
                              want_form=form(TILE, bf16=int(dtype == "bf16"), vec=1, full=1, cp=12, finish=FIN_KERNEL))
    check_backward_exact(res, o, dtype, 1, "T", base)


# ------------------------------------------------------------------------------------------------ the one-launch step
def head_step(o, N, H, Cn, inv_n, rpd=0, accumulate=0, r=True, base_rows=(123.456, -77), sums=("gradWeight", "gradBias", "gradBias_prev"),
              g_prev=True, bases=None, one_call=True):
    """vbnn_head_forward_backward (f32; one launch at these sizes), or vbnn_head_forward then vbnn_head_backward on the same
    arguments. Returns the forward outputs, the backward outputs and the forms seen."""
    L, lib, ctx = _ctx()
    ld = L.pad_ld(H)
    th, tw = packed(o["h"], "f32", ld), packed(o["w3"], "f32", ld)
    tb, tt = dev(o["bias"]), dev(np.asarray(o["target"][:rpd or N], np.int32))
    tr = packed(o["r"], "f32", ld) if r else None
    rows = Rows(N, Cn, base=base_rows)
    ld_gp = H + 2
    gp = sentinel(N, ld_gp) if g_prev else None
    gvp = sentinel(N, ld_gp) if (g_prev and r) else None
    shapes = dict(gradWeight=(Cn, H), gradBias=(1, Cn), gradBias_prev=(1, H))
    flat = {k: tail_buf(bases[k] if bases is not None else np.full(shapes[k], SENT, F)) for k in sums}
    a = L.HeadArgs(h=_p(th), ld_h=ld, w3=_p(tw), ld_w=ld, bias=_p(tb), target=_p(tt), N=N, H=H, C=Cn, rows_per_draw=rpd,
                   inv_n=float(inv_n), accumulate=accumulate, logits=_p(rows.logits), out=_p(rows.out), g_logits=_p(rows.g),
                   loss_sum_dev=_p(rows.loss), correct_dev=_p(rows.hits), gradWeight=_p(flat.get("gradWeight")),
                   gradBias=_p(flat.get("gradBias")), gradBias_prev=_p(flat.get("gradBias_prev")), relu_mask=1, r_prev_packed=0,
                   r_prev=_p(tr), ld_r_prev=ld if r else 0, g_prev=_p(gp), gv_prev=_p(gvp), ld_gp=ld_gp, gT_prev=None, gvT_prev=None,
                   ld_gpT=0, logit_slots=None, n_slots=0)
    if one_call:
        L.check(lib.vbnn_head_forward_backward(ctx, L.F32, C.byref(a)))
        assert_form(form(STEP, finish=FIN_INLINE))
    else:
        L.check(lib.vbnn_head_forward(ctx, L.F32, a.h, ld, a.w3, ld, a.bias, a.target, N, H, Cn, float(inv_n), a.logits, a.out, a.g_logits,
                                      accumulate, a.loss_sum_dev, a.correct_dev, rpd))
        assert_form(form(FORWARD))
        L.check(lib.vbnn_head_backward(ctx, L.F32, a.h, ld, a.w3, ld, a.g_logits, N, H, Cn, accumulate, a.gradWeight, a.gradBias,
                                       a.gradBias_prev, 1, a.r_prev, a.ld_r_prev, 0, a.g_prev, a.gv_prev, ld_gp, None, None, 0))
        assert_form(expect_backward("f32", N, H, Cn, ld_gp % 8 == 0, bool(r), bool(sums), False, g_prev, -1))
    fw = rows.host()
    bw = {k: tail_data(k, t, shapes[k]) for k, t in flat.items()}
    if gp is not None:
        bw["g_prev"] = data("g_prev", gp, N, H)
    if gvp is not None:
        bw["gv_prev"] = data("gv_prev", gvp, N, H)
    return fw, bw


def peaked(o, Cn, at=2):
    """The same operands with a bias that puts class `at` 20000 above the rest: exp(out) is exactly 1 there and exactly 0 elsewhere,
    so with inv_n a power of two d(loss)/d(logits) is exact and every sum of the backward is exact."""
    bias = o["bias"].copy()
    bias[min(at, Cn - 1)] += 20000
    return dict(o, bias=bias)


@pytest.mark.parametrize("N,H,Cn,rpd", [(16, 2, 10, 0), (37, 50, 10, 0), (100, 130, 16, 0), (33, 50, 7, 11)])
def test_one_launch_step_against_forward_then_backward(N, H, Cn, rpd):
    inv_n = F(2.0 ** -5)
    for o in (R.int_operands(N, H, Cn, 500 + N), peaked(R.int_operands(N, H, Cn, 500 + N), Cn)):
        exact = o["bias"].max() > 1000
        target = o["target"][:rpd or N]
        fw1, bw1 = head_step(o, N, H, Cn, inv_n, rpd)
        fw2, bw2 = head_step(o, N, H, Cn, inv_n, rpd, one_call=False)
        for k in ("logits", "out", "g_logits"):
            bitwise("one launch against two: " + k, fw1[k], fw2[k])
        assert _u(np.float64(fw1["loss"])) == _u(np.float64(fw2["loss"])) and fw1["hits"] == fw2["hits"]
        check_rows(fw1, exact_logits(o), target, inv_n, "a", rpd)
        for bw in (bw1, bw2):
            ref = R.head_backward(o["h"], o["w3"], fw1["g_logits"], "f32", 1, o["r"], g_prev_stored=bw["g_prev"])
            for k in bw:
                if exact:
                    bitwise(k, bw[k], ref[k].reshape(bw[k].shape))
                else:
                    within(k, bw[k], ref[k].reshape(bw[k].shape), 2e-6 * ref[k + "_abs"].reshape(bw[k].shape), "a step, real g")
        if exact:
            for k in bw1:
                bitwise("one launch against two: " + k, bw1[k], bw2[k])


def test_one_launch_step_accumulates_over_draws():
    """S = 3 accumulated calls on exact data: loss, hits and the three gradients add up; then the optional outputs NULL in turn."""
    N, H, Cn, inv_n = 37, 50, 10, F(2.0 ** -6)
    rng = np.random.default_rng(8)
    bases = dict(gradWeight=rng.integers(-9, 10, (Cn, H)).astype(F), gradBias=rng.integers(-9, 10, (1, Cn)).astype(F),
                 gradBias_prev=rng.integers(-9, 10, (1, H)).astype(F))
    rows_base = (0.5, 3)
    for s in range(3):
        o = peaked(R.int_operands(N, H, Cn, 600 + s), Cn, at=s)
        fw, bw = head_step(o, N, H, Cn, inv_n, accumulate=1, base_rows=rows_base, bases=bases)
        ref = check_rows(fw, exact_logits(o), o["target"], inv_n, "a", base=rows_base)
        want = R.head_backward(o["h"], o["w3"], fw["g_logits"], "f32", 1, o["r"], base=bases)
        for k in bases:
            bitwise(f"draw {s}: {k}", bw[k], want[k].reshape(bw[k].shape))
        rows_base, bases = (fw["loss"], fw["hits"]), {k: bw[k] for k in bases}
        assert fw["hits"] == ref["hits"]
    o = peaked(R.int_operands(N, H, Cn, 610), Cn)
    for kw in (dict(sums=("gradBias", "gradBias_prev")), dict(sums=("gradWeight",), r=False), dict(sums=(), r=False),
               dict(sums=("gradBias",), g_prev=False, r=False)):
        fw, bw = head_step(o, N, H, Cn, inv_n, **kw)
        want = R.head_backward(o["h"], o["w3"], fw["g_logits"], "f32", 1, o["r"] if kw.get("r", True) else None)
        for k in bw:
            bitwise(f"{kw}: {k}", bw[k], want[k].reshape(bw[k].shape))


# ------------------------------------------------------------------------------------------------ (a) ties and targets, (b) numerics
ENTRIES = ("f32", "bf16", "slots", "step", "nll")


def run_entry(entry, lg, bias, target, inv_n):
    """Integer logits lg (+ bias) through one of the kernels that hold the row arithmetic."""
    N, Cn = lg.shape
    if entry in DTYPES:
        h, w3 = R.logit_operands(lg)
        return head_forward(entry, h, w3, bias, target, inv_n, Cn)
    if entry == "slots":
        slots = np.zeros((3, N, 16), F)
        slots[0, :, :Cn], slots[1, :, :Cn], slots[2, :, :Cn] = lg - 2, 1, 1
        return head_slots(slots, bias, target, inv_n, Cn)
    if entry == "step":
        h, w3 = R.logit_operands(lg)
        o = dict(h=h, w3=w3, bias=np.asarray(bias, F), target=target, r=None)
        return head_step(o, N, 32, Cn, inv_n, r=False, sums=("gradBias",), g_prev=False)[0]
    return logsoftmax_nll((lg + bias).astype(F), target, inv_n)


def entry_classes(entry):
    return R.NLL_CLASSES if entry == "nll" else (1, 10, 16)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", R.EXTREME_KINDS)
def test_log_softmax_edges_on_every_kernel_with_the_row_arithmetic(kind, entry):
    """Peaks, far targets, a bias of +-30000 (out must match the unshifted out within the bound at that magnitude), true ties
    (first maximum wins, also across the four lane groups of a row) and out-of-range targets (clamped for loss, gradient, hits)."""
    group = "b" if kind in ("peak120", "target100", "bias+30000", "bias-30000") else "a"
    for Cn in entry_classes(entry):
        N, inv_n = 19, F(1.0 / 19)
        lg, bias, target = R.extreme_logits(kind, N, Cn)
        res = run_entry(entry, lg, bias, target, inv_n)
        check_rows(res, (lg + bias).astype(F), target, inv_n, group)
        if kind.startswith("bias"):
            unshifted = R.criterion(lg, target, inv_n)
            within("out against the unshifted out", res["out"], unshifted["out"], R.row_bounds((lg + bias).astype(F), target, inv_n)[0], group)
        if kind.startswith("target_"):
            clamped = run_entry(entry, lg, bias, np.clip(target, 0, Cn - 1).astype(np.int32), inv_n)
            for k in ("out", "g_logits"):
                bitwise(f"clamped target: {k}", res[k], clamped[k])
            assert res["hits"] == clamped["hits"]
            if entry == "nll":                               # its loss is added by atomics, in no fixed order
                assert abs(res["loss"] - clamped["loss"]) <= 1e-12 * abs(clamped["loss"])
            else:
                assert res["loss"] == clamped["loss"]


@pytest.mark.parametrize("entry", ("f32", "bf16", "slots", "step"))
def test_a_nan_row_stays_in_its_row(entry):
    N, Cn, inv_n = 19, 10, F(1.0 / 19)
    lg, bias, target = R.extreme_logits("peak120", N, Cn)
    clean = run_entry(entry, lg, bias, target, inv_n)
    bad = lg.copy()
    if entry == "slots":
        bad[5, :] = np.nan                                   # what a NaN in row 5 of h leaves in every class of a slot
    res = None
    if entry == "slots":
        res = run_entry(entry, bad, bias, target, inv_n)
    else:
        h, w3 = R.logit_operands(lg)
        h[5, 20] = np.nan                                    # one element of row 5, in a hidden unit no class reads: NaN x 0
        if entry == "step":
            res = head_step(dict(h=h, w3=w3, bias=bias, target=target, r=None), N, 32, Cn, inv_n, r=False, sums=("gradBias",), g_prev=False)[0]
        else:
            res = head_forward(entry, h, w3, bias, target, inv_n, Cn)
    others = np.arange(N) != 5
    for k in ("logits", "out", "g_logits"):
        assert np.isnan(res[k][5]).all(), f"{k} of the NaN row: {res[k][5]}"
        bitwise(f"{k} of the other rows", res[k][others], clean[k][others])
    assert math.isnan(res["loss"])
    hit5 = int(R.first_max((lg + bias)[5:6])[0] == target[5])
    assert res["hits"] == clean["hits"] - hit5, "the NaN row must not be a hit"


# ------------------------------------------------------------------------------------------------ (c) random real operands
REAL_BWD = [("cp12", 64, 64, 12, {}), ("cp0", 64, 64, 16, {}), ("vec", 37, 70, 10, dict(pad=2, transposes=True)),
            ("scalar", 37, 70, 10, dict(pad=1, transposes=True))]
REAL_BWD = [(d,) + c for d in DTYPES for c in REAL_BWD] + [("bf16", "stream", 64, 128, 12, dict(stream_mode=1))]


@pytest.mark.parametrize("case", REAL_BWD, ids=[c[0] + "-" + c[1] for c in REAL_BWD])
def test_backward_on_real_operands(case):
    dtype, name, N, H, Cn, kw = case
    kw = dict(dict(stream_mode=0), **kw)
    o = R.real_operands(N, H, Cn, 31, dtype)
    for accumulate in (0, 1):
        res, base = head_backward(dtype, o, N, H, Cn, accumulate=accumulate, **kw)
        ref = R.head_backward(o["h"], o["w3"], o["g"], dtype, 1, o["r"], g_prev_stored=res["g_prev"], base=base)
        rel = 2.0 ** -8 if dtype == "bf16" else 0.0
        for k, rk, T in (("g_prev", "g_prev", False), ("gv_prev", "gv_prev", False), ("gT_prev", "g_prev", True), ("gvT_prev", "gv_prev", True)):
            if k in res:
                want, a = (ref[rk].T, ref[rk + "_abs"].T) if T else (ref[rk], ref[rk + "_abs"])
                within(k, res[k], want, rel * np.abs(want) + 2e-6 * a, "c " + dtype)
        for k in ("gradWeight", "gradBias", "gradBias_prev"):
            b = 2e-6 * ref[k + "_abs"] + (0.0 if base[k] is None else 1e-6 * np.abs(base[k]).reshape(ref[k].shape))
            within(k, res[k], ref[k].reshape(res[k].shape), b.reshape(res[k].shape), "c " + dtype)
        if "gT_prev" in res:
            bitwise("gT_prev is g_prev transposed", res["gT_prev"], res["g_prev"].T)
            bitwise("gvT_prev is gv_prev transposed", res["gvT_prev"], res["gv_prev"].T)


@pytest.mark.parametrize("entry", ("f32", "bf16", "step"))
def test_forward_on_real_operands(entry):
    N, H, Cn = 37, 70, 10
    dtype = "bf16" if entry == "bf16" else "f32"
    o = R.real_operands(N, H, Cn, 32, dtype)
    inv_n = F(1.0 / N)
    if entry == "step":
        res, bw = head_step(o, N, H, Cn, inv_n)
        ref = R.head_backward(o["h"], o["w3"], res["g_logits"], "f32", 1, o["r"], g_prev_stored=bw["g_prev"])
        for k in bw:
            within(k, bw[k], ref[k].reshape(bw[k].shape), 2e-6 * ref[k + "_abs"].reshape(bw[k].shape), "c f32")
    else:
        res = head_forward(dtype, o["h"], o["w3"], o["bias"], o["target"], inv_n, Cn)
    exact = o["h"].astype(np.float64) @ o["w3"].astype(np.float64).T + o["bias"]
    within("logits", res["logits"], exact, 4e-6 * (np.abs(o["h"]).astype(np.float64) @ np.abs(o["w3"]).astype(np.float64).T) + 1e-6, "c " + dtype)
    check_rows({k: v for k, v in res.items() if k != "logits"}, res["logits"], o["target"], inv_n, "c " + dtype)      # on the device's own logits


# ------------------------------------------------------------------------------------------------ (d) the small pieces
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,O", [(1, 1), (31, 63), (33, 65), (1025, 130)])
def test_acc_grad_bias(dtype, N, O):
    L, lib, ctx = _ctx()
    rng = np.random.default_rng(N + O)
    for integer in (True, False):
        g = rng.integers(-3, 4, (N, O)).astype(F) if integer else R.round_t(rng.standard_normal((N, O)).astype(F), dtype)
        base = rng.integers(-9, 10, O).astype(F)
        tg = packed(g, dtype, O + 5)
        for accumulate in (0, 1):
            flat = tail_buf(base)
            L.check(lib.vbnn_acc_grad_bias(ctx, _code(dtype), _p(tg), O + 5, N, O, 0.25, accumulate, _p(flat)))
            torch.cuda.synchronize()
            want, a = R.acc_grad_bias(g, 0.25, base if accumulate else None)
            if integer:
                bitwise("gradBias", tail_data("gradBias", flat, (O,)), want)
            else:
                within("acc_grad_bias", tail_data("gradBias", flat, (O,)), want, 2e-6 * a + (1e-6 * np.abs(base) if accumulate else 0.0), "d")


@pytest.mark.parametrize("N,Cn", [(1, 1), (37, 10), (300, 17)])
def test_separate_criterion_modules(N, Cn):
    """vbnn_nll_forward, vbnn_nll_backward, vbnn_logsoftmax_backward; targets out of range are clamped by both NLL calls alike."""
    L, lib, ctx = _ctx()
    rng = np.random.default_rng(N)
    inv_n = F(1.0 / N)
    lg = (rng.standard_normal((N, Cn)) * 3).astype(F)
    out = R.log_softmax(lg).astype(F)
    if Cn > 1:
        out[N // 2, 0] = out[N // 2, 1] = out[N // 2].max() + F(0.5)              # a tie of the maximum: the first wins
    for target in (rng.integers(0, Cn, N).astype(np.int32), rng.integers(-3, Cn + 3, N).astype(np.int32)):
        tt, to = dev(target), packed(out, "f32", Cn + 3)
        loss = torch.zeros(2, dtype=torch.float64, device="cuda")
        hits = torch.zeros(2, dtype=torch.int32, device="cuda")
        L.check(lib.vbnn_nll_forward(ctx, _p(to), Cn + 3, _p(tt), N, Cn, float(inv_n), _p(loss), _p(hits)))
        g = sentinel(N, Cn)
        L.check(lib.vbnn_nll_backward(ctx, _p(tt), N, Cn, float(inv_n), _p(g)))
        gx = sentinel(N, Cn)
        gin = dev(rng.integers(-3, 4, (N, Cn)).astype(F))
        to_dense = dev(out)
        L.check(lib.vbnn_logsoftmax_backward(ctx, _p(to_dense), _p(gin), _p(gx), N, Cn))
        torch.cuda.synchronize()
        want_loss, want_hits = R.nll_forward(out, target, inv_n)
        within("nll_forward loss", loss.cpu().numpy()[0], want_loss, 1e-12 * abs(want_loss) + 1e-300, "d")
        assert int(hits.cpu().numpy()[0]) == want_hits and loss.cpu().numpy()[1] == 0 and hits.cpu().numpy()[1] == 0
        bitwise("nll_backward", data("g", g, N, Cn), R.nll_backward(target, N, Cn, inv_n))
        gi = _host(gin)
        s = np.abs(gi.astype(np.float64).sum(axis=1, keepdims=True))
        p = np.exp(out.astype(np.float64))
        # expf within E_ULP ulp, the float32 rounding of the row sum, the product and the subtraction half an ulp each
        within("logsoftmax_backward", data("gx", gx, N, Cn), R.logsoftmax_backward(out, gi),
               (R.E_ULP * R.ULP + 2 * R.U32) * p * s + R.U32 * np.abs(R.logsoftmax_backward(out, gi)) + R.TINY * s, "d")


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_relu_forward_and_backward(n):
    L, lib, ctx = _ctx()
    rng = np.random.default_rng(n)
    x, g = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    x[::7] = 0.0
    x[n // 2] = -0.0
    x[n // 3] = np.nan
    tx, tg = dev(x), dev(g)
    y, gx = sentinel(1, n + 1), sentinel(1, n + 1)
    L.check(lib.vbnn_relu_forward(ctx, _p(tx), _p(y), n))
    L.check(lib.vbnn_relu_backward(ctx, _p(tx), _p(tg), _p(gx), n))
    torch.cuda.synchronize()
    bitwise("relu_forward", data("y", y, 1, n)[0], R.relu_forward(x))
    bitwise("relu_backward", data("gx", gx, 1, n)[0], R.relu_backward(x, g))


# ------------------------------------------------------------------------------------------------ coverage of the forms, and the figures
def test_every_form_of_the_head_was_asserted_by_a_case_above():
    need = {"forward f32": lambda f: f == form(FORWARD), "forward bf16": lambda f: f == form(FORWARD, bf16=1),
            "from slots": lambda f: f == form(SLOTS), "one-launch step": lambda f: f == form(STEP, finish=FIN_INLINE),
            "streaming backward": lambda f: f & 15 == STREAM and (f >> 16) & 3 == FIN_INLINE,
            "finish kernel": lambda f: f & 15 == TILE and (f >> 16) & 3 == FIN_KERNEL,
            "in-launch finish": lambda f: f & 15 == TILE and (f >> 16) & 3 == FIN_INLINE,
            "no finish": lambda f: f & 15 == TILE and (f >> 16) & 3 == FIN_NONE}
    for bf16 in (0, 1):
        for vec, full, cp in ((1, 1, 12), (1, 1, 0), (1, 0, 0), (0, 0, 0)):
            need[f"tile {'bf16' if bf16 else 'f32'} <{vec},{full},{cp}>"] = (
                lambda f, b=bf16, v=vec, u=full, c=cp: f & 0xFFFF == form(TILE, bf16=b, vec=v, full=u, cp=c))
    missing = [k for k, ok in need.items() if not any(ok(f) for f in SEEN)]
    print("forms seen:", *sorted(form_name(f) for f in SEEN), sep="\n  ")
    print("largest fraction of each bound used on the device:")
    for (group, name), v in sorted(USED.items()):
        print(f"  ({group}) {name}: {v:.3f}")
    assert not missing, f"no case above ran: {missing}"
