"""Every launch form of the three GEMM families, through the C ABI, element by element against tests/_gemm_np.py.

vbnn_forward, vbnn_grad_input, vbnn_acc_grad_parameters and vbnn_backward_pair are called with ctypes on given operands. Every case
sets the debug keys it needs inside try / finally, asserts WHICH launch ran (vbnn_debug_get(VBNN_DEBUG_LAST_GEMM_FORM), restated
here from gemm_dispatch.h and the launchers) before it compares anything, runs the launch twice on sentinel-filled outputs (the two
runs must agree bit for bit), and holds every output to the reference:

  integer tier   mu, x, g in -3..3, sigma^2 in 0..2, gv and r_prev multiples of 1/4: exact in bf16, every partial sum below 2^24
                 (asserted), so each output without noise or a transcendental function is BITWISE the reference (bf16 stores: the
                 rounding of the exact value); y, r, h of the LRT forward and the KL terms are within the bounds derived in
                 _gemm_np.py, bf16 stores by its interval rule; h2 is bitwise the square of the stored h, every transposed output
                 bitwise the transpose of its twin; the all-zero input row gives r = 0 and h = relu(b) exactly.
  real tier      bf16-rounded normal operands, the accumulation-order bound per element from |A| |B| (4e-6, _gemm_np.ACC_REL).
  pads, guards   every output has a pitch larger than its row and guard rows behind it, filled with a sentinel bit pattern that
                 must survive (a packed output's pad column may hold +0 instead; none was found to).

The last test requires that every form of INVENTORY was seen and prints the figures (largest fraction of each bound used, bf16
elements accepted on the far side of a rounding midpoint). UNREACHABLE lists the combinations the dispatch cannot reach, and why."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _gemm_np as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, LAYER = 3, 1
f8, F = np.float64, np.float32
GUARD = 2                                              # guard rows behind every output
SENT32, SENT16 = 0xC9ABCDEF - (1 << 32), 0xC9AB - (1 << 16)          # the sentinel bit patterns (about -1.4e6)
# vbnn_debug_set keys and their defaults
GEMM_KERNEL, V2_SCHEDULE, V2_TILE, V3_MIN_K, V2_PSPLIT, KMAJOR, V3_SPLIT, V0, FOLD_SERIAL, LAST_GEMM_FORM = 0, 1, 2, 4, 5, 6, 8, 9, 12, 13
DEFAULTS = {GEMM_KERNEL: 0, V2_SCHEDULE: -1, V2_TILE: 0, V3_MIN_K: 704, V2_PSPLIT: -1, KMAJOR: 1, V3_SPLIT: -1, V0: 1, FOLD_SERIAL: 0}
K_V0, K_V0_PAIR, K_V1, K_V1_PAIR, K_V2, K_V3, K_V3_SPLIT = 1, 2, 3, 4, 5, 6, 7          # VBNN_GEMM_KERNEL_*
FWD, DX, DW = 1, 2, 3                                                                    # VBNN_GEMM_CLASS_*
SEEN = set()
TIER = ["int"]        # the tier of the cases of the running test (tier_of): "int" or "real"
USED = {}             # (family, form, output) -> largest fraction of its bound used
FAR = {}              # (family, form, output) -> bf16 elements accepted that are not the rounding of the reference itself
PADS_ZEROED = set()   # packed outputs whose pad columns came back +0 instead of the sentinel


def form(kernel, tile=0, sched=0, dual=0, psplit=0, part=0, ak=0, bk=0, sq=0, ones=0, bf16=0, fast=0, serial=0, cls=0):
    """VBNN_GEMM_FORM of include/vbnn_hip.h"""
    return (kernel | (tile << 4) | (sched << 6) | (int(dual) << 8) | (int(psplit) << 9) | (part << 10) | (int(ak) << 12) | (int(bk) << 13) |
            (sq << 14) | (int(ones) << 16) | (int(bf16) << 17) | (int(fast) << 18) | (int(serial) << 19) | (cls << 20))


def form_name(f):
    return (f"kernel {f & 15} tile {(f >> 4) & 3} sched {(f >> 6) & 3} dual {(f >> 8) & 1} psplit {(f >> 9) & 1} part {(f >> 10) & 3} "
            f"AK {(f >> 12) & 1} BK {(f >> 13) & 1} SQ {(f >> 14) & 3} ones {(f >> 16) & 1} bf16 {(f >> 17) & 1} fast {(f >> 18) & 1} "
            f"serial {(f >> 19) & 1} class {(f >> 20) & 3}")


def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return L, L.lib(), nn.Context.get().h


def n_cus(h=None):
    L, lib, h0 = _ctx()
    sp, n = C.c_void_p(), C.c_int()
    L.check(lib.vbnn_ctx_stream(h or h0, C.byref(sp), C.byref(n)))
    return n.value


@contextlib.contextmanager
def keys(**kv):
    """set debug keys (by the names above) for one case, restore every default afterwards"""
    L, lib, _ = _ctx()
    try:
        for k, v in kv.items():
            L.check(lib.vbnn_debug_set(globals()[k], v))
        yield
    finally:
        for k, v in DEFAULTS.items():
            L.check(lib.vbnn_debug_set(k, v))


@contextlib.contextmanager
def tier_of(tier):
    """run the cases inside on the integer or on the real tier"""
    TIER[0] = tier
    try:
        yield
    finally:
        TIER[0] = "int"


@pytest.fixture
def tier(request):
    """the tier of a test's cases, set by parametrisation (indirect): every form runs on integer operands, bit for bit, and once on
    bf16-rounded normal operands within the accumulation-order bound"""
    with tier_of(request.param):
        yield request.param


BOTH = pytest.mark.parametrize("tier", ["int", "real"], indirect=True)


def assert_form(want):
    _, lib, _ = _ctx()
    got = lib.vbnn_debug_get(LAST_GEMM_FORM)
    assert got == want, f"ran [{form_name(got)}], expected [{form_name(want)}]"
    SEEN.add(got)


def cdiv(a, b):
    return (a + b - 1) // b


def up(a, b):
    return cdiv(a, b) * b


def v1_form(dt, cls, M, N, dual, ta=0, tb=0, sq=0, ones=0, fast=0, part=0, v0=1):
    """launch_gemm_v1_form's choice: 128 x 128 tiles from 128 of them, 64 x 64 from 96, else the latency kernel (fp32) or 32 x 32"""
    bf = dt == "bf16"
    tile = 2 if cdiv(M, 128) * cdiv(N, 128) >= 128 else 1 if cdiv(M, 64) * cdiv(N, 64) >= 96 else 0
    if tile == 0 and not bf and v0:
        wide = not (ta and tb) and cdiv(M, 16) * cdiv(N, 32) >= 160
        return form(K_V0, int(wide), 0, dual, 0, part, ta, tb, sq, ones, 0, fast, 0, cls)
    return form(K_V1, tile, 0, dual, 0, part, ta, tb, sq, ones, bf, fast, 0, cls)


# ------------------------------------------------------------------------------------------------ buffers
def tdt(dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16}[dt]


def code(dt):
    from vbnn_amd import _lib as L
    return {"f32": L.F32, "bf16": L.BF16}[dt]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def op(a, dt, ld, rows=None, fill=0.0):
    """an operand of type dt with pitch ld holding a (values the type holds exactly), `fill` elsewhere"""
    a = np.asarray(a, F)
    t = torch.full((rows or a.shape[0], ld), fill, dtype=tdt(dt), device="cuda")
    t[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda().to(tdt(dt))
    return t


def sent(rows, ld, dt="f32"):
    """an output of rows x ld and GUARD rows behind it, all sentinel"""
    t = torch.empty((rows + GUARD, ld), dtype=tdt(dt), device="cuda")
    t.view(torch.int32 if dt == "f32" else torch.int16).fill_(SENT32 if dt == "f32" else SENT16)
    return t


def dense(rows, cols, old=None):
    """a dense fp32 rows x cols output (no pitch: a gradient) followed by guard words, all sentinel, or holding `old` (accumulate)"""
    t = torch.empty(rows * cols + 16 * GUARD, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(SENT32)
    if old is not None:
        t[:rows * cols] = torch.from_numpy(np.ascontiguousarray(old, F).reshape(-1)).cuda()
    return t


def bits(t):
    """the whole buffer as integers on the host"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def take(name, t, rows, cols, packed=False):
    """the rows x cols values of an output as float64; its pad columns and guard rows must still hold the sentinel (a packed
    output's pad columns may hold +0: the next GEMM's zero padding along K)"""
    b = bits(t)
    s = SENT32 if t.dtype == torch.float32 else SENT16
    if b.ndim == 1:
        assert (b[rows * cols:] == s).all(), f"{name}: written past its end"
        return t[:rows * cols].cpu().numpy().astype(f8).reshape(rows, cols)
    assert (b[rows:] == s).all(), f"{name}: a guard row was written"
    pad = b[:rows, cols:]
    if not (pad == s).all():
        assert packed and ((pad == s) | (pad == 0)).all(), f"{name}: a pad column was written"
        PADS_ZEROED.add(name)
    return t[:rows, :cols].float().cpu().numpy().astype(f8)


def note(key, err, bound):
    """record the largest fraction of a bound used; assert the bound"""
    err, bound = np.asarray(err, f8), np.broadcast_to(np.asarray(bound, f8), np.shape(err))
    bad = err > bound
    pos = bound > 0
    USED[key] = max(USED.get(key, 0.0), float((err[pos] / bound[pos]).max()) if pos.any() else 0.0)
    assert not bad.any(), f"{key}: {int(bad.sum())} of {bad.size} elements outside their bound, worst {float((err[bad] / np.maximum(bound[bad], 1e-300)).max()):.3f} of it"


def check(key, got, ref, e, dt):
    """one output against the reference: e None = bitwise (a bf16 store: the rounding of the exact value); else the bound e per
    element -- |got - ref| <= e for an fp32 store, the interval rule for a bf16 store"""
    assert np.isfinite(got).all(), f"{key}: not finite"
    if TIER[0] == "real" and not key[1].startswith("real"):          # the figures of the two tiers are kept apart
        key = (key[0], "real " + key[1], key[2])
    if dt == "bf16":
        ok = G.interval_ok(got, ref, 0.0 if e is None else e)
        assert ok.all(), f"{key}: {int((~ok).sum())} of {ok.size} bf16 elements are not the rounding of any value in their interval"
        far = G.far_side(got, ref)
        FAR[key] = FAR.get(key, 0) + far
        assert e is not None or far == 0
    elif e is None:
        assert np.array_equal(got, np.asarray(ref, f8).astype(F).astype(f8)), f"{key}: {int((got != ref).sum())} of {got.size} elements differ"
    else:
        note(key, np.abs(got - ref), e)


def twice(launch):
    """run a launch twice on fresh sentinel-filled outputs; the two must agree bit for bit; returns the first's buffers"""
    a = launch()
    torch.cuda.synchronize()
    b = launch()
    torch.cuda.synchronize()
    for k in a:
        if a[k] is not None and k != "slots":          # (the slots' classes past head_C are undefined)
            assert np.array_equal(bits(a[k]), bits(b[k])), f"{k}: two launches on the same operands differ"
    return a


# ------------------------------------------------------------------------------------------------ operands
def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(f8)


def rb(a):
    from oracle.ref_numpy import bf16_round
    return bf16_round(np.asarray(a, F)).astype(f8)


@functools.lru_cache(maxsize=None)
def layer_operands(N, I, O, tier="int"):
    """one set of operands per (N, I, O): asymmetric, x with an all-zero row, zeros, positives and negatives"""
    rng = np.random.default_rng(N * 1000003 + I * 1009 + O)
    if tier == "int":
        d = dict(mu=ints(rng, -3, 3, (O, I)), var=ints(rng, 0, 2, (O, I)), x=ints(rng, -3, 3, (N, I)), g=ints(rng, -3, 3, (N, O)),
                 gv=ints(rng, -6, 6, (N, O)) * 0.25, r_prev=ints(rng, -6, 6, (N, I)) * 0.25, bias=ints(rng, -8, 8, O) * 0.25)
    else:
        d = dict(mu=rb(rng.normal(0, 1, (O, I))), var=rb(np.abs(rng.normal(0, 0.1, (O, I)))), x=rb(rng.normal(0, 1, (N, I))),
                 g=rb(rng.normal(0, 1, (N, O))), gv=rb(rng.normal(0, 1, (N, O))), r_prev=rb(rng.normal(0, 1, (N, I))),
                 bias=rb(rng.normal(0, 1, O)))
    d["zero_row"] = N // 2 if N >= 3 else None
    if d["zero_row"] is not None:
        d["x"][d["zero_row"]] = 0.0
    d["x2"] = d["x"] ** 2 if tier == "int" else rb(d["x"] ** 2)
    # every partial sum of the integer tier is a multiple of 1/4 below 2^22 in magnitude, so exact in fp32 in any order: a product
    # is at most 9 . 2 = 18 (x.x sigma^2), a sum has at most max(N, I, O) of them, and gx = a1 + 2 x a2 at most 7 such sums
    if tier == "int":
        assert 7 * 18 * max(N, I, O) < 2 ** 22
    return d


def normals(dt, N, O, draw, row0, rpd=0, draw_dev=0):
    """the normals a forward of type dt draws: the oracle's bit-exact form (fp32), vbnn_fill_normal_hw read back (bf16)"""
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    if dt == "f32":
        from oracle import vbnn_oracle as vo
        fill = lambda rows, cols, d, r0: vo.fill_normal(rows, cols, SEED, L.STREAM_ZETA, LAYER, d, r0)
    else:
        def fill(rows, cols, d, r0):
            t = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
            nn.fill_normal(t, SEED, L.STREAM_ZETA, LAYER, d, row0=r0, hw=True)
            torch.cuda.synchronize()
            return t.cpu().numpy()
    return G.zeta(fill, N, O, draw, row0, rpd, draw_dev)


# ------------------------------------------------------------------------------------------------ vbnn_forward
def run_forward(dt, N, I, O, want, tag, dual=True, sq=False, raw_x=False, bias=True, relu=True, y=False, r="packed", h=True, h2=True,
                hT=False, odd=False, rpd=0, draw_dev=None, row0=5, draw=2, tier=None, fold=False, slots=0, ld=None, reference=True, ctx_h=None):
    """one forward: want = the expected form; r: None / "f32" / "packed"; odd: fp32 outputs at pitch columns + 1; fold: the
    launch accumulates the first GEMM on top of b + sqrt(v) z (the two-pass kernel); slots: classes of a head carried along"""
    L, lib, ctx = _ctx()
    ctx = ctx_h or ctx
    tier = tier or TIER[0]
    d = layer_operands(N, I, O, tier)
    ld = ld or L.pad_ld(I)
    w, w2 = op(d["mu"], dt, ld), (op(d["var"], dt, ld) if dual else None)
    if raw_x:                                           # the raw minibatch: pitch I rounded to 4, finite junk behind the row
        xs = op(d["x"], dt, up(I, 4), fill=7.0)
    else:
        xs = op(d["x"], dt, ld)
    x2 = op(d["x2"], dt, xs.shape[1]) if (dual and not sq) else None
    b = torch.from_numpy(d["bias"].astype(F)).cuda() if bias else None
    ddev = torch.tensor([draw_dev], dtype=torch.int32, device="cuda") if draw_dev is not None else None
    w3 = ints(np.random.default_rng(O), -2, 2, (slots, O)) if slots else None
    w3d = op(w3, dt, L.pad_ld(O)) if slots else None
    ld_y = O + 1 if odd else up(O, 4) + 4
    ld_rf = O + 1 if odd else up(O, 4) + 4
    ld_h, ld_hT = up(O, 8) + 8, up(N, 8) + 8

    def launch():
        o = dict(y=sent(N, ld_y) if y else None,
                 r=(sent(N, ld_rf) if r == "f32" else sent(N, ld_h, dt)) if (r and dual) else None,
                 h=sent(N, ld_h, dt) if h else None, h2=sent(N, ld_h, dt) if (h and h2) else None,
                 hT=sent(O, ld_hT, dt) if hT else None, h2T=sent(O, ld_hT, dt) if (hT and h2) else None,
                 slots=torch.full((lib.vbnn_forward_head_slots(ctx, code(dt), N, I, O, slots), N, 16), -7.0, dtype=torch.float32, device="cuda") if slots else None)
        a = L.FwdArgs(w=_p(w), w2=_p(w2), x=_p(xs), x2=_p(x2), ld_w=ld, ld_x=xs.shape[1], N=N, I=I, O=O, bias=_p(b), seed=SEED, layer=LAYER,
                      draw=draw, row0=row0, y=_p(o["y"]), ld_y=ld_y, r=_p(o["r"]), ld_r=(ld_rf if r == "f32" else ld_h), r_packed=int(r == "packed"),
                      relu=int(relu), h=_p(o["h"]), h2=_p(o["h2"]), ld_h=ld_h, hT=_p(o["hT"]), h2T=_p(o["h2T"]), ld_hT=ld_hT, rows_per_draw=rpd,
                      draw_dev=_p(ddev), head_w3=_p(w3d), head_ld_w=L.pad_ld(O) if slots else 0, head_C=slots, head_slots=_p(o["slots"]))
        torch.cuda.synchronize()
        L.check(lib.vbnn_forward(ctx, code(dt), C.byref(a)))
        assert_form(want)
        L.check(lib.vbnn_sync(ctx))
        return o

    o = twice(launch)
    if not reference:
        return o
    key = lambda name: ("FWD", tag, name)
    z = normals(dt, N, O, draw, row0, rpd, draw_dev or 0) if dual else None
    x2ref = d["x2"] if tier == "int" else (rb(d["x"] ** 2) if (not sq or dt == "bf16") else (d["x"].astype(F) ** 2).astype(f8))
    ref = G.forward(d["x"], d["mu"], d["bias"] if bias else None, d["var"] if dual else None, x2ref, z, relu)
    absm = np.abs(d["x"]) @ np.abs(d["mu"]).T + (np.abs(d["bias"]) if bias else 0.0)
    if dual:
        e_y, e_r = G.bound_y(ref), G.bound_r(ref)
        if fold or tier == "real":
            e_y = e_y + G.accum_bound(absm + np.abs(ref["y"] - ref["m"]))
        if tier == "real":
            e_r = e_r + G.ACC_REL * np.abs(ref["r"])
    else:
        e_y, e_r = (None if tier == "int" else G.accum_bound(absm)), None
    zr = d["zero_row"]                                    # (None: fewer than three rows)
    if y:
        check(key("y"), take("y", o["y"], N, O), ref["y"], e_y, "f32")
    if o["r"] is not None:
        got_r = take("r", o["r"], N, O, packed=r == "packed")
        check(key("r"), got_r, ref["r"], e_r, dt if r == "packed" else "f32")
        assert zr is None or (got_r[zr] == 0).all(), "v = 0 must give r = 0"
    if h:
        got_h = take("h", o["h"], N, O, packed=True)
        check(key("h"), got_h, ref["h"], e_y, dt)
        want0 = np.maximum(d["bias"], 0) if (bias and relu) else (d["bias"] if bias else np.zeros(O))
        assert zr is None or np.array_equal(got_h[zr], want0 if dt == "f32" else G.bf16_rne(want0)), "v = 0 must give h = relu(b)"
        sq_stored = (got_h.astype(F) * got_h.astype(F)).astype(f8) if dt == "f32" else G.bf16_rne(got_h * got_h)
        if h2:
            assert np.array_equal(take("h2", o["h2"], N, O, packed=True), sq_stored), "h2 is the square of the stored h"
        if hT:
            assert np.array_equal(take("hT", o["hT"], O, N, packed=True), got_h.T), "hT is the transpose of h"
            if h2:
                assert np.array_equal(take("h2T", o["h2T"], O, N, packed=True), sq_stored.T), "h2T is the transpose of h2"
        if slots:
            got = o["slots"].double().sum(dim=0).cpu().numpy()[:, :slots]
            check(key("head slots"), got, G.head_logits(got_h, w3), G.accum_bound(np.abs(got_h) @ np.abs(w3).T) if (dual or tier == "real") else None, "f32")
    return o


# ------------------------------------------------------------------------------------------------ vbnn_grad_input
def run_grad_input(dt, N, I, O, want, tag, dual=True, kmajor=False, gx=False, hand=True, relu_mask=True, r_prev="packed", gT=False, odd=False,
                   tier=None, args_only=False, reference=True):
    """one gradInput (M = I, N = rows, K = O). kmajor: the weights as the forward holds them (w, w2: O x ld_w), else wT, w2T;
    hand: the hand-off outputs g_prev, gv_prev (gv_prev only with r_prev); r_prev: None / "f32" / "packed\""""
    L, lib, ctx = _ctx()
    tier = tier or TIER[0]
    d = layer_operands(N, I, O, tier)
    ldk = L.pad_ld(O)
    if kmajor:
        ld_w = up(I, 8) + (8 if dt == "f32" else 0)
        A, A2 = op(d["mu"], dt, ld_w), (op(d["var"], dt, ld_w) if dual else None)
    else:
        A, A2 = op(d["mu"].T, dt, ldk), (op(d["var"].T, dt, ldk) if dual else None)
    g, gv = op(d["g"], dt, ldk), (op(d["gv"], dt, ldk) if dual else None)
    ld_x = up(I, 8) + 8
    xs = op(d["x"], dt, ld_x)
    rp = None if not r_prev else (op(d["r_prev"], "f32", I + 1 if odd else up(I, 4) + 4) if r_prev == "f32" else op(d["r_prev"], dt, ld_x))
    ld_gx, ld_gp, ld_gpT = (I + 1 if odd else up(I, 4) + 4), up(I, 8) + 8, up(N, 8) + 8
    holder = {}

    def make():
        o = dict(gx=sent(N, ld_gx) if gx else None, g_prev=sent(N, ld_gp, dt) if hand else None,
                 gv_prev=sent(N, ld_gp, dt) if (hand and r_prev) else None, gT_prev=sent(I, ld_gpT, dt) if (hand and gT) else None,
                 gvT_prev=sent(I, ld_gpT, dt) if (hand and gT and r_prev) else None)
        a = L.DxArgs(wT=None if kmajor else _p(A), w2T=None if kmajor else _p(A2), g=_p(g), gv=_p(gv), ld_wT=ldk, ld_g=ldk, N=N, I=I, O=O,
                     x=_p(xs), ld_x=ld_x, gx=_p(o["gx"]), ld_gx=ld_gx, relu_mask=int(relu_mask), r_prev=_p(rp),
                     ld_r_prev=rp.shape[1] if rp is not None else 0, r_prev_packed=int(r_prev == "packed"), g_prev=_p(o["g_prev"]),
                     gv_prev=_p(o["gv_prev"]), ld_gp=ld_gp, gT_prev=_p(o["gT_prev"]), gvT_prev=_p(o["gvT_prev"]), ld_gpT=ld_gpT,
                     w=_p(A) if kmajor else None, w2=_p(A2) if kmajor else None, ld_w=A.shape[1] if kmajor else 0)
        holder["keep"] = (A, A2, g, gv, xs, rp)
        return o, a

    def verify(o):
        key = lambda name: ("DX", tag, name)
        ref = G.grad_input(d["g"], d["mu"], d["gv"] if dual else None, d["var"] if dual else None, d["x"], relu_mask,
                           d["r_prev"] if r_prev else None)
        e = e_gv = None
        if tier == "real":
            e = G.accum_bound(np.abs(d["g"]) @ np.abs(d["mu"]) + (2 * np.abs(d["x"]) * (np.abs(d["gv"]) @ d["var"]) if dual else 0.0)) \
                + G.U * G.SLACK * np.abs(ref["gx"])
            e_gv = e * np.abs(d["r_prev"]) + G.U * G.SLACK * np.abs(ref["gv_prev"])
        if gx:
            check(key("gx"), take("gx", o["gx"], N, I), ref["gx"], e, "f32")
        if hand:
            got = take("g_prev", o["g_prev"], N, I, packed=True)
            check(key("g_prev"), got, ref["g_prev"], e, dt)
            if relu_mask:
                assert (got[d["x"] <= 0] == 0).all(), "g_prev is exactly 0 where x <= 0"
            if r_prev:
                got_v = take("gv_prev", o["gv_prev"], N, I, packed=True)
                check(key("gv_prev"), got_v, ref["gv_prev"], e_gv, dt)
            if gT:
                assert np.array_equal(take("gT_prev", o["gT_prev"], I, N, packed=True), got.T), "gT_prev is the transpose of g_prev"
                if r_prev:
                    assert np.array_equal(take("gvT_prev", o["gvT_prev"], I, N, packed=True), got_v.T), "gvT_prev is the transpose of gv_prev"

    if args_only:
        return make, verify

    def launch():
        o, a = make()
        L.check(lib.vbnn_grad_input(ctx, code(dt), C.byref(a)))
        assert_form(want)
        return o

    o = twice(launch)
    if reference:
        verify(o)
    return o


# ------------------------------------------------------------------------------------------------ vbnn_acc_grad_parameters
VAR_HAT, BB = 0.75, 8.0


def run_acc_grad(dt, N, I, O, want, tag, dual=True, layout="T", sq=False, bias="stored", accumulate=False, scale=0.5, gw=True, gs=True,
                 fused=False, shadows=False, kl=0.0, S=2.0, part=0, lvars="zero", tier=None, pad256=False, args_only=False, then=None, reference=True):
    """one accGradParameters (M = I (+ 1), N = O, K = rows). layout: "T" (xT, gT: the packed K-contiguous form), "K" (x, g K-major),
    "mixed" (x, x2 K-major with gT, gvT). bias: None / "stored" (a row / column of ones in the operand) / "synth" (fp32 K-major).
    lvars: "zero" (stdv = 1, vars = 1: exact) or "real". then: a second part to launch after this one into the same outputs."""
    L, lib, ctx = _ctx()
    tier = tier or TIER[0]
    d = layer_operands(N, I, O, tier)
    rng = np.random.default_rng(I + O)
    ldn = L.pad_ld(N)
    x, x2 = d["x"], d["x2"]
    ones = np.ones((N, 1))
    xb, x2b = (np.hstack([x, ones]), np.hstack([x2, ones])) if bias == "stored" else (x, x2)
    T = dict(xT=None, x2T=None, gT=None, gvT=None, x=None, x2=None, g=None, gv=None)
    if layout == "T":
        T.update(xT=op(xb.T, dt, ldn), gT=op(d["g"].T, dt, ldn))
        if dual:
            T.update(x2T=op(x2b.T, dt, ldn), gvT=op(d["gv"].T, dt, ldn))
    if layout in ("K", "mixed"):
        ld_x = up(xb.shape[1], 256) if pad256 else (up(xb.shape[1], 8) + (8 if not pad256 else 0))
        ld_g = up(O, 8) + 8
        T.update(x=op(xb, dt, ld_x))
        if dual and not sq:
            T.update(x2=op(x2b, dt, ld_x))
        if layout == "K":
            T.update(g=op(d["g"], dt, ld_g), gv=op(d["gv"], dt, ld_g) if dual else None)
        else:
            T.update(gT=op(d["g"].T, dt, ldn), gvT=op(d["gv"].T, dt, ldn))
    lv = np.zeros((O, I), F) if lvars == "zero" else rng.normal(np.log(0.05), 0.4, (O, I)).astype(F)
    means = ints(rng, -3, 3, (O, I)).astype(F)
    mu_s, var_s = (rb(means), ints(rng, 0, 2, (O, I)) if tier == "int" else rb(np.exp(lv.astype(f8)))) if shadows else (None, None)
    ld_w = L.pad_ld(I)
    dev = dict(lv=torch.from_numpy(lv).cuda(), means=torch.from_numpy(means).cuda(),
               stats=torch.tensor([0.0, 0.0, VAR_HAT, 0.0], dtype=torch.float64, device="cuda"),
               mu_s=op(mu_s, dt, ld_w) if shadows else None, var_s=op(var_s, dt, ld_w) if shadows else None)
    old = None
    if accumulate:
        old = dict(gradWeight=ints(rng, -9, 9, (O, I)), gradSum=ints(rng, -9, 9, (O, I)), gradBias=ints(rng, -9, 9, O),
                   grad_mu=ints(rng, -9, 9, (O, I)), grad_lv=ints(rng, -9, 9, (O, I)))
    e_wn = None
    if not dual and (gs or fused):
        from oracle import vbnn_oracle as vo
        e_wn = vo.fill_normal(O, I, SEED, L.STREAM_EPS, LAYER, 4).astype(f8)
    holder = {}

    def make(p=part, o=None):
        o = o or dict(gradWeight=dense(O, I, old and old["gradWeight"]) if gw else None, gradSum=dense(O, I, old and old["gradSum"]) if gs else None,
                      grad_mu=dense(O, I, old and old["grad_mu"]) if fused else None, grad_lv=dense(O, I, old and old["grad_lv"]) if fused else None,
                      gradBias=dense(1, O, old and old["gradBias"]) if bias else None)
        a = L.DwArgs(xT=_p(T["xT"]), x2T=_p(T["x2T"]), gT=_p(T["gT"]), gvT=_p(T["gvT"]), ld_n=ldn, N=N, I=I, O=O,
                     scale=scale, accumulate=int(accumulate), gradWeight=_p(o["gradWeight"]), gradSum=_p(o["gradSum"]), seed=SEED, layer=LAYER,
                     draw=4, lvars=_p(dev["lv"]), grad_mu=_p(o["grad_mu"]), grad_lv=_p(o["grad_lv"]), means=_p(dev["means"]) if fused else None,
                     stats=_p(dev["stats"]) if fused else None, B=BB, S=S, kl_scale=kl, gradBias=_p(o["gradBias"]),
                     x=_p(T["x"]), x2=_p(T["x2"]), g=_p(T["g"]), gv=_p(T["gv"]), ld_x=T["x"].shape[1] if T["x"] is not None else 0,
                     ld_g=T["g"].shape[1] if T["g"] is not None else 0, mu_s=_p(dev["mu_s"]), var_s=_p(dev["var_s"]), ld_w=ld_w if shadows else 0,
                     part=p, draw_dev=None)
        holder["keep"] = (T, dev)
        return o, a

    def verify(o, p=part):
        key = lambda name: ("DW", tag, name)
        x2ref = x2 if (not sq or tier == "int") else (x.astype(F) ** 2).astype(f8)
        ref = G.acc_grad(x, d["g"], d["gv"] if dual else None, x2ref, scale, lv, e_wn, means, VAR_HAT if fused else None, BB, S, kl, mu_s, var_s,
                         old, p)
        abs1 = np.abs(d["g"]).T @ np.abs(x)
        abs2 = np.abs(d["gv"]).T @ np.abs(x2ref) if dual else None
        real = tier == "real"
        exact = not real and lvars == "zero"
        if p and not accumulate:                            # a part leaves what depends on the other accumulator alone
            for k in (("gradWeight", "grad_mu", "gradBias") if p == 2 else ("gradSum", "grad_lv")):
                assert o[k] is None or (bits(o[k]) == SENT32).all(), f"part {p} wrote {k}"
        if gw and p != 2:
            check(key("gradWeight"), take("gradWeight", o["gradWeight"], O, I), ref["gradWeight"],
                  G.accum_bound(scale * abs1) + G.U * np.abs(ref["gradWeight"]) if real else None, "f32")
        if bias and p != 2:
            check(key("gradBias"), take("gradBias", o["gradBias"], 1, O), ref["gradBias"][None, :],
                  G.accum_bound(scale * np.abs(d["g"]).sum(0))[None, :] + G.U * np.abs(ref["gradBias"])[None, :] if real else None, "f32")
        if gs and p != 1:
            got = take("gradSum", o["gradSum"], O, I)
            if dual:
                e = None if exact else G.bound_grad_sum(ref["a2"], lv, ref["gradSum"]) + (G.accum_bound(2 * abs2 * np.exp(lv / 2.0)) if real else 0.0)
            else:
                e = G.bound_grad_sum_wn(ref["a1"], e_wn, ref["gradSum"]) + (G.ACC_REL * abs1 * np.abs(e_wn) if real else 0.0)
            check(key("gradSum"), got, ref["gradSum"], e, "f32")
        if fused:
            var = np.asarray(var_s, f8) if shadows else np.exp(lv.astype(f8))
            mu = np.asarray(mu_s if shadows else means, f8)
            bitwise = exact and kl == 0.0 and S in (1.0, 2.0)
            if p != 2:
                e = None if bitwise else G.bound_grad_mu(ref["a1"], mu, scale, S, BB, VAR_HAT, kl, ref["grad_mu"], accumulate) + \
                    (G.accum_bound(scale * abs1 / S) if real else 0.0)
                check(key("grad_mu"), take("grad_mu", o["grad_mu"], O, I), ref["grad_mu"], e, "f32")
            if p != 1:
                if dual:
                    e = None if bitwise else G.bound_grad_lv(ref["a2"], var, S, BB, VAR_HAT, kl, ref["grad_lv"], accumulate, shadows or lvars == "zero") + \
                        (G.accum_bound(abs2 * var / S) if real else 0.0)
                else:
                    e = G.bound_grad_lv_wn(ref["a1"], e_wn, lv, var, S, BB, VAR_HAT, kl, ref["grad_lv"], accumulate) + \
                        (G.ACC_REL * abs1 * np.abs(e_wn) * np.exp(lv / 2.0) / (2.0 * S) if real else 0.0)
                check(key("grad_lv"), take("grad_lv", o["grad_lv"], O, I), ref["grad_lv"], e, "f32")

    if args_only:
        return make, verify

    def launch():
        o, a = make()
        L.check(lib.vbnn_acc_grad_parameters(ctx, code(dt), C.byref(a)))
        assert_form(want)
        if then is not None:
            p2, want2 = then
            _, a2 = make(p2, o)
            L.check(lib.vbnn_acc_grad_parameters(ctx, code(dt), C.byref(a2)))
            assert_form(want2)
        return o

    o = twice(launch)
    if reference:
        verify(o, 0 if then is not None else part)
    return o


def fwd_fast(y, r, h):
    return (not y) and r != "f32" and h


def dx_fast(gx, hand, r_prev):
    return (not gx) and hand and r_prev != "f32"


# ================================================================================================ the general kernel, fp32 and bf16
GEOMETRY = {"32": (37, 50), "32-one": (1, 1), "64": (763, 511), "128": (2045, 1023)}       # M x N of the output
KS = {"f32": (1, 32, 33, 72), "bf16": (8, 64, 65, 200)}


def _cases_general():
    """every K on the integer tier; the real tier at the ragged tail, where every form runs as well"""
    return [(dt, geo, K, t) for dt in ("f32", "bf16") for geo in GEOMETRY for K in KS[dt] for t in ("int", "real") if t == "int" or K == KS[dt][-1]]


def _force(dt):
    return dict(GEMM_KERNEL=1) if dt == "bf16" else {}


@pytest.mark.parametrize("dt,geo,K,tier", _cases_general(), indirect=["tier"])
def test_general_kernel_forward(dt, geo, K, tier):
    """FWD (M = O, N = rows, K = I) single and dual in every geometry; fp32 also SQ = 1 (x2 = NULL) and the raw minibatch (K mask)"""
    M, N = GEOMETRY[geo]
    with keys(**_force(dt)):
        for dual in (False, True):
            tag = f"v1 {dt} {'dual' if dual else 'single'}"
            # guarded: y, float r at an odd pitch, transposes; then the packed outputs alone (fast where a tile allows)
            run_forward(dt, N, K, M, v1_form(dt, FWD, M, N, dual, fast=0), tag, dual, y=True, r="f32", hT=True, odd=True)
            run_forward(dt, N, K, M, v1_form(dt, FWD, M, N, dual, fast=1), tag, dual)
            if dt == "f32" and dual:
                run_forward(dt, N, K, M, v1_form(dt, FWD, M, N, True, sq=1, fast=0), tag + " SQ1", True, sq=True, y=True)
                run_forward(dt, N, K, M, v1_form(dt, FWD, M, N, True, sq=1, fast=1), tag + " SQ1 raw", True, sq=True, raw_x=True, bias=False, h2=False)
            if dt == "f32" and not dual:
                run_forward(dt, N, K, M, v1_form(dt, FWD, M, N, False, fast=0), tag + " raw", False, raw_x=True, y=True, relu=False)


@pytest.mark.parametrize("dt,geo,K,tier", _cases_general(), indirect=["tier"])
def test_general_kernel_grad_input(dt, geo, K, tier):
    """DX (M = I, N = rows, K = O) single and dual; fp32 also TA (the weights K-major, from w)"""
    M, N = GEOMETRY[geo]
    with keys(**_force(dt)):
        for dual in (False, True):
            tag = f"v1 {dt} {'dual' if dual else 'single'}"
            run_grad_input(dt, N, M, K, v1_form(dt, DX, M, N, dual, fast=0), tag, dual, gx=True, r_prev="f32", gT=True, odd=True)
            run_grad_input(dt, N, M, K, v1_form(dt, DX, M, N, dual, fast=1), tag, dual)
            run_grad_input(dt, N, M, K, v1_form(dt, DX, M, N, dual, fast=0), tag + " gx only", dual, gx=True, hand=False, relu_mask=False, r_prev=None)
            if dt == "f32":
                run_grad_input(dt, N, M, K, v1_form(dt, DX, M, N, dual, ta=1, fast=0), tag + " TA", dual, kmajor=True, gx=True, r_prev=None)
                run_grad_input(dt, N, M, K, v1_form(dt, DX, M, N, dual, ta=1, fast=1), tag + " TA", dual, kmajor=True)


@pytest.mark.parametrize("dt,geo,K,tier", _cases_general(), indirect=["tier"])
def test_general_kernel_acc_grad(dt, geo, K, tier):
    """DW (M = I + 1, N = O, K = rows) single and dual; fp32 also TA + TB with and without SQ = 2 and with the synthesised ones row"""
    M, N = GEOMETRY[geo]
    I = M - 1 if M > 1 else 1           # the stored row of ones is output row I: the GEMM's M is I + 1
    with keys(**_force(dt)):
        for dual in (False, True):
            tag = f"v1 {dt} {'dual' if dual else 'single'}"
            run_acc_grad(dt, K, I, N, v1_form(dt, DW, I + 1, N, dual), tag, dual)
            run_acc_grad(dt, K, I, N, v1_form(dt, DW, I + 1, N, dual), tag + " accumulate", dual, accumulate=True, scale=2.0, fused=dual, S=1.0)
            run_acc_grad(dt, K, I, N, v1_form(dt, DW, I, N, dual), tag + " no bias", dual, bias=None, gw=False, fused=dual, kl=1.0)
            if dt == "f32":
                run_acc_grad(dt, K, I, N, v1_form(dt, DW, I + 1, N, dual, ta=1, tb=1, sq=2 if dual else 0, ones=1), tag + " TA TB synth", dual,
                             layout="K", sq=True, bias="synth")
                run_acc_grad(dt, K, I, N, v1_form(dt, DW, I, N, dual, ta=1, tb=1), tag + " TA TB", dual, layout="K", bias=None, accumulate=True)
        If = M - M % 4
        if dt == "bf16" and If:         # the fast protocol of the fused total gradients (I % 4 == 0, the shadows), edge tiles included
            for kl in (0.0, 1.0):
                run_acc_grad(dt, K, If, N, v1_form(dt, DW, If + 1, N, True, fast=1), "v1 bf16 dual fused", gw=False, gs=False, fused=True,
                             shadows=True, kl=kl)


@BOTH
def test_general_kernel_parts_and_transcendental_epilogue(tier):
    """part 2 then part 1 give bit for bit the outputs of part 0, and each part alone leaves the other's outputs untouched; the guarded
    epilogue's expf / sqrtf and KL terms within their derived bounds on the fp32 parameters, first draw and accumulating, with
    I % 4 != 0 and == 0"""
    for dt in ("f32", "bf16"):
        with keys(**_force(dt)):
            for I, O, N in ((37, 50, 33), (36, 50, 64)):
                kw = dict(fused=True, kl=1.0, S=2.0)
                p2, p1 = v1_form(dt, DW, I, O, False, part=2), v1_form(dt, DW, I + 1, O, False, part=1)
                full = run_acc_grad(dt, N, I, O, v1_form(dt, DW, I + 1, O, True), f"v1 {dt} part 0", **kw)
                two = run_acc_grad(dt, N, I, O, p2, f"v1 {dt} part 2 + 1", part=2, then=(1, p1), **kw)
                for k in full:
                    assert np.array_equal(bits(full[k]), bits(two[k])), f"{k}: part 2 then part 1 is not part 0"
                run_acc_grad(dt, N, I, O, p2, f"v1 {dt} part 2", part=2, **kw)
                run_acc_grad(dt, N, I, O, p1, f"v1 {dt} part 1", part=1, **kw)
                for acc in (False, True):
                    run_acc_grad(dt, N, I, O, v1_form(dt, DW, I + 1, O, True), f"v1 {dt} expf", fused=True, kl=1.0, S=3.0, lvars="real", accumulate=acc)
                run_acc_grad(dt, N, I, O, v1_form(dt, DW, I + 1, O, False), f"v1 {dt} WN", dual=False, fused=True, kl=1.0, lvars="real")
                if dt == "bf16":        # the shadows with gradSum / the weight-noise d/dlvars: stdv from lvars, element by element
                    for dual in (False, True):
                        run_acc_grad(dt, N, I, O, v1_form(dt, DW, I + 1, O, dual), f"v1 {dt} shadows + stdv", dual, fused=True, shadows=True,
                                     kl=1.0, lvars="real")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_general_kernel_noise_addressing(dt):
    """rows_per_draw of 1, 5 and N with a ragged N / rpd, the device-resident draw counter, row0 above 2^16"""
    N, I, O = 37, 33, 50
    with keys(**_force(dt)):
        want = v1_form(dt, FWD, O, N, True, fast=0)
        for rpd in (1, 5, N):
            run_forward(dt, N, I, O, want, f"v1 {dt} rpd", y=True, rpd=rpd)
        run_forward(dt, N, I, O, want, f"v1 {dt} draw_dev", y=True, draw_dev=3, rpd=5)
        run_forward(dt, N, I, O, want, f"v1 {dt} draw_dev alone", y=True, draw_dev=7)
        run_forward(dt, N, I, O, want, f"v1 {dt} row0", y=True, row0=(1 << 16) + 123)
    # the counter keeps a bf16 forward of ANY size on the general kernel, here in its 128 x 128 tile, and so does a pitch that is
    # no multiple of 64 -- no key set
    if dt == "bf16":
        M, Nn = GEOMETRY["128"]
        run_forward(dt, Nn, 65, M, form(K_V1, 2, dual=1, bf16=1, fast=1, cls=FWD), "v1 bf16 128 by draw_dev", draw_dev=1)
        run_forward(dt, Nn, 65, M, form(K_V1, 2, dual=1, bf16=1, fast=1, cls=FWD), "v1 bf16 128 by pitch", ld=72)
        # stacked draws on the pipelined kernel (only the two-pass kernel refuses them: EpiFwd::v3_ok()), both protocols, whole and
        # ragged tiles, a draw boundary inside a tile; and row0 above 2^16 there
        with keys(GEMM_KERNEL=2, V2_TILE=256):
            for Mo, Nr in V2_OUT:
                for guarded in (False, True):
                    for rpd in (1, 5, Nr):
                        run_forward(dt, Nr, 200, Mo, v2_form(FWD, True, not guarded, 256, -1), "v2 256 rpd", y=guarded, rpd=rpd)
                    run_forward(dt, Nr, 200, Mo, v2_form(FWD, True, not guarded, 256, -1), "v2 256 row0", y=guarded, row0=(1 << 16) + 123)


SMALL = [(50, 33, 37), (256, 72, 400), (256, 400, 72)]       # N, I, O: 400 x 256 outputs are 25 x 8 = 200 wide tiles of the latency kernel


@BOTH
@pytest.mark.parametrize("v0", [1, 0])
@pytest.mark.parametrize("N,I,O", SMALL)
def test_latency_kernel_and_the_32_tile(v0, N, I, O, tier):
    """both VBNN_DEBUG_V0 settings at the 32 geometry: the latency kernel's narrow and wide tile / gemm_v1's own 32 x 32 tile"""
    with keys(V0=v0):
        for dual in (False, True):
            tag = f"{'v0' if v0 else 'v1-32'} {'dual' if dual else 'single'}"
            f = lambda cls, M, Nn, **kw: v1_form("f32", cls, M, Nn, dual, v0=v0, **kw)
            run_forward("f32", N, I, O, f(FWD, O, N, sq=int(dual), fast=0), tag, dual, sq=True, y=True, r="f32", raw_x=True)
            run_forward("f32", N, I, O, f(FWD, O, N, sq=int(dual), fast=1), tag, dual, sq=True)
            run_grad_input("f32", N, I, O, f(DX, I, N, ta=1, fast=0), tag, dual, kmajor=True, gx=True, r_prev="f32")
            run_grad_input("f32", N, I, O, f(DX, I, N, ta=1, fast=1), tag, dual, kmajor=True)
            run_grad_input("f32", N, I, O, f(DX, I, N, fast=1), tag + " packed", dual)
            run_acc_grad("f32", N, I, O, f(DW, I + 1, O, ta=1, tb=1, sq=2 if dual else 0, ones=1), tag, dual, layout="K", sq=True, bias="synth")
            run_acc_grad("f32", N, I, O, f(DW, I, O, ta=1, tb=1), tag + " x2 given", dual, layout="K", bias=None)
            run_acc_grad("f32", N, I, O, f(DW, I + 1, O), tag + " packed", dual)


@pytest.mark.parametrize("v0", [1, 0])
@pytest.mark.parametrize("N,I,O", SMALL)
@pytest.mark.parametrize("dual", [False, True])
@BOTH
def test_backward_pair_is_its_two_calls(v0, N, I, O, dual, tier):
    """vbnn_backward_pair in one launch (both kernels of the pair launch) against the reference and against its two calls"""
    L, lib, ctx = _ctx()
    with keys(V0=v0):
        mk_dx, vf_dx = run_grad_input("f32", N, I, O, 0, "pair", dual, kmajor=True, gx=True, r_prev="f32", args_only=True)
        mk_dw, vf_dw = run_acc_grad("f32", N, I, O, 0, "pair", dual, layout="K", sq=True, bias="synth", args_only=True)
        wide = cdiv(I, 16) * cdiv(N, 32) >= 160
        want = form(K_V0_PAIR if v0 else K_V1_PAIR, int(wide) if v0 else 0, dual=dual, ak=1, bk=1, sq=2 if dual else 0, ones=1, cls=DW)

        def pair():
            (ox, ax), (ow, aw) = mk_dx(), mk_dw()
            L.check(lib.vbnn_backward_pair(ctx, L.F32, C.byref(ax), C.byref(aw)))
            assert_form(want)
            return dict(ox, **ow)

        def two():
            (ox, ax), (ow, aw) = mk_dx(), mk_dw()
            L.check(lib.vbnn_acc_grad_parameters(ctx, L.F32, C.byref(aw)))
            L.check(lib.vbnn_grad_input(ctx, L.F32, C.byref(ax)))
            return dict(ox, **ow)

        o, t = twice(pair), twice(two)
        vf_dx(o)
        vf_dw(o)
        for k in o:
            if o[k] is not None:
                assert np.array_equal(bits(o[k]), bits(t[k])), f"{k}: the pair launch is not its two calls"


# ================================================================================================ the pipelined kernel
def v2_form(cls, dual, fast, tile, sched, psplit=0, kmajor=0):
    """launch_gemm_v2's choice under the keys of a case: tile 256 / 128 / 64 -> variant 0 / 1 / 2; by default schedule 0 for the 128
    tile and 4 otherwise; the four-wave tiles run 4 as 2; the K-major pair split runs 0 as 2"""
    vi = 0 if psplit else {256: 0, 128: 1, 64: 2}[tile]
    s = sched if sched in (0, 2, 4) else (0 if vi == 1 else 4)
    if vi and s == 4:
        s = 2
    if psplit and kmajor and s != 4:
        s = 2
    return form(K_V2, vi, s >> 1, dual and not psplit, psplit, 0, kmajor, kmajor, 0, 0, 1, fast, 0, cls)


V2_OUT = ((257, 129), (256, 128))
# every tile at its own schedule over 1 .. 5 K steps and the ragged tail; the schedules crossed with the tiles at K = 192, 200
V2_CASES = [(t, -1, K) for t in (256, 128, 64) for K in (64, 128, 192, 200, 256, 320)] + \
           [(t, s, K) for t, ss in ((256, (0, 2, 4)), (128, (0, 2)), (64, (0, 2))) for s in ss for K in (192, 200)]
V2_CASES = [c + ("int",) for c in V2_CASES] + [c + ("real",) for c in V2_CASES if c[2] == 200]       # the real tier at the ragged tail


@pytest.mark.parametrize("tile,sched,K,tier", V2_CASES, indirect=["tier"])
def test_pipelined_kernel(tile, sched, K, tier):
    """all three families, dual and single, the fast and the guarded protocol, every tile and schedule; the transposed outputs go
    through the kernel's LDS transpose"""
    with keys(GEMM_KERNEL=2, V2_TILE=tile, V2_SCHEDULE=sched, V2_PSPLIT=0):
        for dual in (False, True):
            tag = f"v2 {tile} {'dual' if dual else 'single'}"
            for M, N in V2_OUT:
                for guarded in (False, True):
                    run_forward("bf16", N, K, M, v2_form(FWD, dual, not guarded, tile, sched), tag, dual, y=guarded, hT=True)
                    run_grad_input("bf16", N, M, K, v2_form(DX, dual, not guarded, tile, sched), tag, dual, gx=guarded, gT=True)
            for I, O in ((256, 129), (256, 128), (255, 129)):          # I % 4 != 0: no vector accesses, the guarded form alone
                for guarded in (False, True):
                    fast = dual and not guarded and I % 4 == 0
                    run_acc_grad("bf16", K, I, O, v2_form(DW, dual, fast, tile, sched), tag, dual, gw=guarded, gs=guarded, fused=dual,
                                 shadows=dual, kl=1.0)
                # the shadows together with gradSum (LRT) and with the weight-noise d/dlvars: stdv is exp(lvars / 2) of the fp32
                # parameter at THIS element (lvars differ element by element; the shadows are unrelated integers on the integer tier)
                run_acc_grad("bf16", K, I, O, v2_form(DW, dual, 0, tile, sched), tag + " shadows + stdv", dual, fused=True, shadows=True, kl=1.0,
                             lvars="real")


@BOTH
@pytest.mark.parametrize("K", [64, 192, 200, 320])
def test_pipelined_kernel_pair_split(K, tier):
    """the pair's two GEMMs in different workgroups (VBNN_DEBUG_V2_PSPLIT = 1), K-contiguous: fast and guarded"""
    with keys(GEMM_KERNEL=2, V2_PSPLIT=1):
        for I, O in ((256, 129), (256, 128)):
            for guarded in (False, True):
                run_acc_grad("bf16", K, I, O, v2_form(DW, True, not guarded, 256, -1, psplit=1), "v2 psplit", gw=guarded, gs=guarded,
                             fused=True, shadows=True, kl=1.0)


@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("bias", [None, "stored"])
@BOTH
def test_pipelined_kernel_pair_split_kmajor(N, bias, tier):
    """the K-major pair split: I = 1024, O = 1536 are the 96 tiles of 128 gemm_v2_eligible asks for; x, g as the forward holds them"""
    I, O = 1024, 1536
    with keys(V2_PSPLIT=1, V3_SPLIT=0):
        run_acc_grad("bf16", N, I, O, v2_form(DW, True, 1, 256, -1, psplit=1, kmajor=1), "v2 psplit K-major", layout="K", bias=bias, gw=False,
                     gs=False, fused=True, shadows=True, kl=1.0)


# ================================================================================================ the two-pass kernel
def v3_form(cls, dual, ak=0, bk=0, serial=0, part=0):
    return form(K_V3, 0, 0, dual, 0, part, ak, bk, 0, 0, 1, 1, serial, cls)


FUSED = dict(bias=None, gw=False, gs=False, fused=True, shadows=True)


@pytest.mark.parametrize("M,N,K,tier", [(M, N, K, t) for M, N in ((256, 256), (512, 256)) for K in (64, 128, 192, 256, 320, 784)
                                        for t in ("int", "real") if t == "int" or K in (192, 320)], indirect=["tier"])
def test_two_pass_kernel(M, N, K, tier):
    """K-contiguous operands, all three families, dual and single (accGradParameters: its parts); the forward on both forms of its
    fold, as an inner and as the last layer; K = 784 in an 832-wide row"""
    with keys(GEMM_KERNEL=3):
        for dual in (False, True):
            tag = f"v3 {'dual' if dual else 'single'}"
            run_forward("bf16", N, K, M, v3_form(FWD, dual), tag, dual, fold=dual, hT=(K == 192))
            run_grad_input("bf16", N, M, K, v3_form(DX, dual), tag, dual, gT=(K == 192))
            run_grad_input("bf16", N, M, K, v3_form(DX, dual), tag + " no r_prev", dual, r_prev=None)
        kl = float(K % 128 == 0)
        full = run_acc_grad("bf16", K, M, N, v3_form(DW, True), "v3 dual", kl=kl, **FUSED)
        two = run_acc_grad("bf16", K, M, N, v3_form(DW, False, part=2), "v3 part 2 + 1", kl=kl, part=2, then=(1, v3_form(DW, False, part=1)), **FUSED)
        for k in full:
            if full[k] is not None:
                assert np.array_equal(bits(full[k]), bits(two[k])), f"{k}: part 2 then part 1 is not part 0"
        run_forward("bf16", N, K, M, v3_form(FWD, True), "v3 dual last layer", fold=True, h2=False, bias=False)
    with keys(GEMM_KERNEL=3, FOLD_SERIAL=1):
        run_forward("bf16", N, K, M, v3_form(FWD, True, serial=1), "v3 dual serial fold", fold=True)
        run_forward("bf16", N, K, M, v3_form(FWD, True, serial=1), "v3 dual serial fold last layer", fold=True, h2=False, bias=False)


@pytest.mark.parametrize("serial", [0, 1])
def test_two_pass_kernel_head_slots(serial):
    """the head's logits from the forward's own tiles, on both forms of the fold: the slots summed are h_stored w3^T"""
    N, I, O, Cn = 256, 320, 512, 10
    with keys(GEMM_KERNEL=3, FOLD_SERIAL=serial):
        run_forward("bf16", N, I, O, v3_form(FWD, True, serial=serial), "v3 head slots", fold=True, h2=False, slots=Cn)
        if not serial:      # the single GEMM (MAP / weight noise): integer-valued h, so the summed slots are exact
            run_forward("bf16", N, I, O, v3_form(FWD, False), "v3 head slots single", False, h2=False, slots=Cn)


@BOTH
@pytest.mark.parametrize("K", [64, 192, 320])
def test_two_pass_kernel_kmajor(K, tier):
    """A K-major: DX from w, w2 (the ReLU mask rides through the second pass as NaN) and the mixed DW form (x, x2 with gT, gvT);
    A and B K-major: DW dual and part 1 / 2; the shadows at kl_scale 0 and 1"""
    M, N = 512, 256
    with keys(GEMM_KERNEL=3):
        for dual in (False, True):
            run_grad_input("bf16", N, M, K, v3_form(DX, dual, ak=1), "v3 K-major", dual, kmajor=True)
        run_grad_input("bf16", N, M, K, v3_form(DX, True, ak=1), "v3 K-major no r_prev", True, kmajor=True, r_prev=None)
        run_grad_input("bf16", N, M, K, v3_form(DX, True, ak=1), "v3 K-major no mask", True, kmajor=True, relu_mask=False)
        for kl in (0.0, 1.0):
            run_acc_grad("bf16", K, M, N, v3_form(DW, True, ak=1), "v3 mixed", layout="mixed", kl=kl, **FUSED)
            full = run_acc_grad("bf16", K, M, N, v3_form(DW, True, ak=1, bk=1), "v3 K-major", layout="K", kl=kl, **FUSED)
            two = run_acc_grad("bf16", K, M, N, v3_form(DW, False, ak=1, bk=1, part=2), "v3 K-major part 2 + 1", layout="K", kl=kl, part=2,
                               then=(1, v3_form(DW, False, ak=1, bk=1, part=1)), **FUSED)
            for k in full:
                if full[k] is not None:
                    assert np.array_equal(bits(full[k]), bits(two[k])), f"{k}: part 2 then part 1 is not part 0"
            run_acc_grad("bf16", K, M, N, v3_form(DW, False, ak=1, bk=1, part=2), "v3 K-major part 2", layout="K", kl=kl, part=2, **FUSED)


@pytest.mark.parametrize("I,O,N", [(100, 256, 64), (252, 256, 192), (260, 512, 320), (100, 512, 192)])
@BOTH
def test_two_pass_kernel_half_height_split(I, O, N, tier):
    """the pair-split half-height launch (VBNN_DEBUG_V3_SPLIT = 1): the ones row in a ragged last tile, x allocated in whole 256-column
    tiles as vbnn_kmajor_supported_dw = 2 asks"""
    L, lib, ctx = _ctx()
    with keys(V3_SPLIT=1):
        assert lib.vbnn_ctx_kmajor_supported_dw(ctx, I, O, N, 1) == 2
        for kl in (0.0, 1.0):
            run_acc_grad("bf16", N, I, O, form(K_V3_SPLIT, psplit=1, ak=1, bk=1, bf16=1, fast=1, cls=DW), "v3 split", layout="K", pad256=True,
                         gw=False, gs=False, fused=True, shadows=True, kl=kl)


# ================================================================================================ the real tier, one case per form
def test_real_tier():
    """bf16-rounded normal operands, the accumulation-order bound per element from |A| |B|"""
    for dt in ("f32", "bf16"):
        with keys(**_force(dt)):
            N, I, O = 50, 72, 37
            run_forward(dt, N, I, O, v1_form(dt, FWD, O, N, True), f"real v1 {dt}", y=True, r="f32", tier="real")
            run_grad_input(dt, N, I, O, v1_form(dt, DX, I, N, True), f"real v1 {dt}", gx=True, r_prev="f32", tier="real")
            run_acc_grad(dt, N, I, O, v1_form(dt, DW, I + 1, O, True), f"real v1 {dt}", fused=True, kl=1.0, lvars="real", tier="real")
    with keys(GEMM_KERNEL=2, V2_PSPLIT=0, V2_TILE=256):
        run_forward("bf16", 129, 200, 257, v2_form(FWD, True, 1, 256, -1), "real v2", tier="real")
        run_grad_input("bf16", 129, 257, 200, v2_form(DX, True, 1, 256, -1), "real v2", tier="real")
        run_acc_grad("bf16", 200, 256, 129, v2_form(DW, True, 1, 256, -1), "real v2", gw=False, gs=False, fused=True, shadows=True, kl=1.0,
                     lvars="real", tier="real")
    with keys(GEMM_KERNEL=3):
        run_forward("bf16", 256, 320, 256, v3_form(FWD, True), "real v3", fold=True, tier="real")
        run_grad_input("bf16", 256, 256, 320, v3_form(DX, True, ak=1), "real v3 K-major", kmajor=True, tier="real")
        run_acc_grad("bf16", 320, 256, 256, v3_form(DW, True, ak=1, bk=1), "real v3 K-major", layout="K", kl=1.0, lvars="real", tier="real", **FUSED)


# ================================================================================================ selection by shape, refusals
def _v3_tiles(cus):
    """the fewest 256 x 256 tiles gemm_v3_shape_ok takes on `cus` compute units: 3/4 of them busy, rounds no dearer than the half tiles'"""
    return next(t for t in range(1, 8 * cus) if 4 * t >= 3 * cus and 185 * cdiv(t, cus) <= 100 * cdiv(2 * t, cus))


def _tile_grid(t):
    """t tiles as (rows of tiles, columns of tiles) with at most 16 rows: O = 256 rows, N = 256 columns"""
    a = max(d for d in range(1, 17) if t % d == 0)
    return a, t // a


def _same_bits(a, b):
    for k in a:
        if a[k] is not None and k != "slots":
            assert np.array_equal(bits(a[k]), bits(b[k])), f"{k}: the launch chosen by shape is not the forced launch"


def test_selection_by_shape_is_what_the_queries_promise():
    """no key set: the form read back is the one vbnn_kmajor_supported and vbnn_forward_head_slots answer for, computed from the
    context's CU count; the forced launch's bits on the same operands are the reference (no reference product)"""
    L, lib, ctx = _ctx()
    t3 = _v3_tiles(n_cus())
    ta, tb = _tile_grid(t3)
    O, N, I = 256 * ta, 256 * tb, 704
    assert lib.vbnn_ctx_kmajor_supported(ctx, O, N, I) == 1 and lib.vbnn_forward_head_slots(ctx, L.BF16, N, I, O, 10) == 2 * ta
    kw = dict(fold=True, h2=False, reference=False)
    by_shape = run_forward("bf16", N, I, O, v3_form(FWD, True), "by shape v3", slots=10, **kw)
    with keys(GEMM_KERNEL=3):
        _same_bits(by_shape, run_forward("bf16", N, I, O, v3_form(FWD, True), "by shape v3", slots=10, **kw))
    # below VBNN_DEBUG_V3_MIN_K the same output goes to the pipelined kernel, and both queries say no
    assert lib.vbnn_ctx_kmajor_supported(ctx, O, N, 640) == 0 and lib.vbnn_forward_head_slots(ctx, L.BF16, N, 640, O, 10) == 0
    if cdiv(O, 128) * cdiv(N, 128) >= 96:
        t256, t128 = cdiv(O, 256) * cdiv(N, 128), cdiv(O, 128) * cdiv(N, 128)
        small = t256 < 192 and t128 > t256
        want = form(K_V2, int(small), 0 if small else 2, dual=1, bf16=1, fast=1, cls=FWD)
        by_shape = run_forward("bf16", N, 640, O, want, "by shape v2", reference=False)
        with keys(GEMM_KERNEL=2):
            _same_bits(by_shape, run_forward("bf16", N, 640, O, want, "by shape v2", reference=False))


def _split_ok(M, N, K, cus):
    """gemm_v3_split_shape_ok by shape (VBNN_DEBUG_V3_SPLIT = -1), restated"""
    if N % 256 or K % 64:
        return False
    tiles, blocks = cdiv(M, 256) * (N // 256), cdiv(M, 128) * (N // 256) * 2
    return tiles * 16 <= 5 * cus and tiles * 16 >= 3 * cus and K >= 2048 and blocks <= cus and blocks * 8 >= 5 * cus


def test_selection_by_shape_of_the_backward_launches():
    """no key set: gradInput and accGradParameters launch what vbnn_ctx_kmajor_supported and vbnn_ctx_kmajor_supported_dw answer
    for -- 1 through the K-major two-pass launch, 1 through the pipelined kernel's K-major pair split, 2 through the half-height
    split -- with the shapes computed from the context's CU count; the forced launch's bits are the reference"""
    L, lib, ctx = _ctx()
    cus = n_cus()
    ta, tb = _tile_grid(_v3_tiles(cus))
    A, Bn, K = 256 * ta, 256 * tb, 704
    # gradInput: M = I = A, N = rows = Bn, K = O
    assert lib.vbnn_ctx_kmajor_supported(ctx, A, Bn, K) == 1
    by_shape = run_grad_input("bf16", Bn, A, K, v3_form(DX, True, ak=1), "by shape v3", kmajor=True, reference=False)
    with keys(GEMM_KERNEL=3):
        _same_bits(by_shape, run_grad_input("bf16", Bn, A, K, v3_form(DX, True, ak=1), "by shape v3", kmajor=True, reference=False))
    # accGradParameters, answer 1, the two-pass kernel: M = I = A, N = O = Bn, K = rows; no ones row (acc_grad_t: try_kmajor only then)
    assert lib.vbnn_ctx_kmajor_supported_dw(ctx, A, Bn, K, 0) == 1
    kw = dict(layout="K", kl=1.0, reference=False, **FUSED)
    by_shape = run_acc_grad("bf16", K, A, Bn, v3_form(DW, True, ak=1, bk=1), "by shape v3", **kw)
    with keys(GEMM_KERNEL=3):
        _same_bits(by_shape, run_acc_grad("bf16", K, A, Bn, v3_form(DW, True, ak=1, bk=1), "by shape v3", **kw))
    # answer 1, the pipelined kernel's K-major pair split: at least 96 tiles of 128, at most 128 of 256 x 128, 16 K steps, the ones row
    I, O, N = 1024, 1536, 1024
    kw = dict(layout="K", bias="stored", gw=False, gs=False, fused=True, shadows=True, kl=1.0, reference=False)
    if not _split_ok(I + 1, O, N, cus):
        assert lib.vbnn_ctx_kmajor_supported_dw(ctx, I, O, N, 1) == 1
        want = v2_form(DW, True, 1, 256, -1, psplit=1, kmajor=1)
        by_shape = run_acc_grad("bf16", N, I, O, want, "by shape v2 K-major", **kw)
        with keys(V2_PSPLIT=1, V3_SPLIT=0):
            _same_bits(by_shape, run_acc_grad("bf16", N, I, O, want, "by shape v2 K-major", **kw))
    # answer 2, the half-height split: one round of 128-row tiles x 2 on 5/8 .. all of the CUs, K >= 2048, x in whole 256-column tiles
    I, N = 784, 2048
    O = next((o for o in range(256, 256 * 129, 256) if _split_ok(I + 1, o, N, cus)), None)
    print(f"{cus} CUs: the half-height split by shape at I = {I}, O = {O}, {N} rows")
    if O is not None:
        assert lib.vbnn_ctx_kmajor_supported_dw(ctx, I, O, N, 1) == 2
        want = form(K_V3_SPLIT, psplit=1, ak=1, bk=1, bf16=1, fast=1, cls=DW)
        by_shape = run_acc_grad("bf16", N, I, O, want, "by shape v3 split", pad256=True, **kw)
        with keys(V3_SPLIT=1):
            _same_bits(by_shape, run_acc_grad("bf16", N, I, O, want, "by shape v3 split", pad256=True, **kw))


def test_cu_budget_context_plans_for_its_budget():
    """a vbnn_ctx_create_cu_budget context answers, and launches, for its own compute units: an output that fills 3/4 of HALF the
    device takes the two-pass kernel there and the pipelined kernel on the whole device"""
    L, lib, ctx = _ctx()
    from vbnn_amd import nn
    cus = n_cus()
    c2 = nn.Context.with_cu_budget(0, cus // 2)
    try:
        budget = n_cus(c2.h)
        assert budget == cus // 2
        t3, full = _v3_tiles(budget), _v3_tiles(cus)
        ta, tb = _tile_grid(t3)
        O, N, I = 256 * ta, 256 * tb, 704
        assert lib.vbnn_ctx_kmajor_supported(c2.h, O, N, I) == 1
        run_forward("bf16", N, I, O, v3_form(FWD, True), "budget v3", fold=True, h2=False, reference=False, ctx_h=c2.h)
        if t3 < full and cdiv(O, 128) * cdiv(N, 128) >= 96:
            assert lib.vbnn_ctx_kmajor_supported(ctx, O, N, I) == 0
            t256, t128 = cdiv(O, 256) * cdiv(N, 128), cdiv(O, 128) * cdiv(N, 128)
            small = t256 < 192 and t128 > t256
            run_forward("bf16", N, I, O, form(K_V2, int(small), 0 if small else 2, dual=1, bf16=1, fast=1, cls=FWD), "budget v2", h2=False,
                        reference=False)
    finally:
        torch.cuda.synchronize()
        L.check(lib.vbnn_ctx_destroy(c2.h))


def test_launchers_refuse_what_they_cannot_address():
    """a misaligned operand pointer is refused by the launcher of each kernel a forward can take (general, pipelined, two-pass, and
    the latency kernel's caller): an error, nothing launched, the recorded form as it was; an unknown key of the read side answers -1.
    (The launchers' other refusals -- VBNN_ERR_UNSUPPORTED of the latency kernel, the pair launch, the K-major pair split and the
    half-height split, after which their callers fall back -- are not provoked here.)"""
    L, lib, ctx = _ctx()
    before = lib.vbnn_debug_get(LAST_GEMM_FORM)
    for dt, force in (("f32", 0), ("bf16", 1), ("bf16", 2), ("bf16", 3)):
        with keys(GEMM_KERNEL=force):
            N = I = O = 256
            t = op(np.zeros((N + 1, I)), dt, I)
            h = sent(N, O, dt)
            a = L.FwdArgs(w=C.c_void_p(t.data_ptr() + 4), x=_p(t), ld_w=I, ld_x=I, N=N, I=I, O=O, h=_p(h), ld_h=O, relu=1)
            assert lib.vbnn_forward(ctx, code(dt), C.byref(a)) == 1 and len(lib.vbnn_last_error()) > 0
            assert lib.vbnn_debug_get(LAST_GEMM_FORM) == before
            torch.cuda.synchronize()
            assert (bits(h) == (SENT16 if dt == "bf16" else SENT32)).all()
    assert lib.vbnn_debug_get(0) == -1 and lib.vbnn_debug_get(99) == -1


# ================================================================================================ the inventory
def _inventory():
    """Every launch the dispatch (gemm_dispatch.h; gemm_fwd.hip, gemm_dx.hip, gemm_dw.hip; vbnn_backward_pair) can reach, as a
    predicate on the recorded form, derived by hand from the launchers. Each must have been asserted by a case above."""
    kern = lambda f: f & 15
    tile = lambda f: (f >> 4) & 3
    sched = lambda f: (f >> 6) & 3
    bit = lambda f, b: (f >> b) & 1
    part = lambda f: (f >> 10) & 3
    sq = lambda f: (f >> 14) & 3
    cls = lambda f: (f >> 20) & 3
    inv = {}
    for c, cn in ((FWD, "FWD"), (DX, "DX"), (DW, "DW")):
        for d, dn in ((0, "single"), (1, "dual")):
            base = lambda f, c=c, d=d: cls(f) == c and bit(f, 8) == d and part(f) == 0 and not bit(f, 9)
            # the general kernel: three tiles, both types, both protocols (EpiDw::fast_ok(): bf16 LRT pairs only)
            for bf, tn in ((0, "f32"), (1, "bf16")):
                for t in (0, 1, 2):
                    for fa in (0, 1):
                        if c == DW and fa and not (bf and d):
                            continue
                        inv[f"v1 {tn} tile {t} {cn} {dn} fast {fa}"] = lambda f, b=base, bf=bf, t=t, fa=fa: (
                            b(f) and kern(f) == K_V1 and bit(f, 17) == bf and tile(f) == t and bit(f, 18) == fa)
            # its fp32 operand forms, in all three tiles
            for t in (0, 1, 2):
                if c == FWD and d:
                    inv[f"v1 f32 tile {t} FWD SQ 1"] = lambda f, b=base, t=t: b(f) and kern(f) == K_V1 and tile(f) == t and sq(f) == 1
                if c == DX:
                    inv[f"v1 f32 tile {t} DX TA {dn}"] = lambda f, b=base, t=t: b(f) and kern(f) == K_V1 and tile(f) == t and bit(f, 12) and not bit(f, 13)
                if c == DW:
                    inv[f"v1 f32 tile {t} DW TA TB {dn} SQ {2 * d} ones row synthesised"] = lambda f, b=base, t=t, d=d: (
                        b(f) and kern(f) == K_V1 and tile(f) == t and bit(f, 12) and bit(f, 13) and sq(f) == 2 * d and bit(f, 16))
                    inv[f"v1 f32 tile {t} DW TA TB {dn} SQ 0"] = lambda f, b=base, t=t: (
                        b(f) and kern(f) == K_V1 and tile(f) == t and bit(f, 12) and bit(f, 13) and sq(f) == 0 and not bit(f, 16))
            # the latency kernel: narrow and wide (with both sides K-major: narrow only), packed and K-major
            for w, wn in ((0, "narrow"), (1, "wide")):
                if not (c == DW and w):
                    inv[f"v0 {wn} {cn} {dn}"] = lambda f, b=base, w=w: b(f) and kern(f) == K_V0 and tile(f) == w
            if c != FWD:                                    # (the forward has no K-major side: both its operands are K-contiguous)
                inv[f"v0 {cn} {dn} K-major"] = lambda f, b=base: b(f) and kern(f) == K_V0 and bit(f, 12)
            inv[f"v0 {cn} {dn} packed"] = lambda f, b=base: b(f) and kern(f) == K_V0 and not bit(f, 12)
            # the pipelined kernel: three tiles with their schedules, both protocols
            for vi, ss in ((0, (0, 1, 2)), (1, (0, 1)), (2, (0, 1))):
                for s in ss:
                    for fa in (0, 1):
                        if c == DW and fa and not d:
                            continue
                        inv[f"v2 variant {vi} schedule {2 * s} {cn} {dn} fast {fa}"] = lambda f, b=base, vi=vi, s=s, fa=fa: (
                            b(f) and kern(f) == K_V2 and tile(f) == vi and sched(f) == s and bit(f, 18) == fa)
            # the two-pass kernel, K-contiguous (a single accGradParameters accumulator there is a part: below)
            if not (c == DW and not d):
                inv[f"v3 {cn} {dn}"] = lambda f, b=base: b(f) and kern(f) == K_V3 and not bit(f, 12) and not bit(f, 13)
    for p in (1, 2):
        inv[f"f32 DW part {p}"] = lambda f, p=p: kern(f) in (K_V1, K_V0) and not bit(f, 17) and part(f) == p and not bit(f, 8)
        inv[f"v1 bf16 DW part {p}"] = lambda f, p=p: kern(f) == K_V1 and bit(f, 17) and part(f) == p and not bit(f, 8)
        inv[f"v3 DW part {p}"] = lambda f, p=p: kern(f) == K_V3 and not bit(f, 12) and part(f) == p and not bit(f, 8)
        inv[f"v3 DW K-major part {p}"] = lambda f, p=p: kern(f) == K_V3 and bit(f, 12) and bit(f, 13) and part(f) == p and not bit(f, 8)
    inv["v3 FWD serial fold"] = lambda f: kern(f) == K_V3 and cls(f) == FWD and bit(f, 19) and bit(f, 8)
    for d, dn in ((0, "single"), (1, "dual")):
        inv[f"v3 DX A K-major {dn}"] = lambda f, d=d: kern(f) == K_V3 and cls(f) == DX and bit(f, 12) and not bit(f, 13) and bit(f, 8) == d
        for kk, kn in ((K_V0_PAIR, "v0"), (K_V1_PAIR, "v1")):
            inv[f"{kn} pair launch {dn}"] = lambda f, kk=kk, d=d: kern(f) == kk and bit(f, 8) == d and sq(f) == 2 * d and bit(f, 16)
    inv["v0 pair launch wide"] = lambda f: kern(f) == K_V0_PAIR and tile(f) == 1
    inv["v0 pair launch narrow"] = lambda f: kern(f) == K_V0_PAIR and tile(f) == 0
    inv["v3 DW mixed (A K-major)"] = lambda f: kern(f) == K_V3 and cls(f) == DW and bit(f, 12) and not bit(f, 13) and bit(f, 8)
    inv["v3 DW A and B K-major dual"] = lambda f: kern(f) == K_V3 and cls(f) == DW and bit(f, 12) and bit(f, 13) and bit(f, 8)
    inv["v3 half-height split"] = lambda f: kern(f) == K_V3_SPLIT and bit(f, 9) and bit(f, 12) and bit(f, 13) and cls(f) == DW
    for fa in (0, 1):
        inv[f"v2 pair split K-contiguous fast {fa}"] = lambda f, fa=fa: (kern(f) == K_V2 and bit(f, 9) and not bit(f, 12) and not bit(f, 8) and
                                                                         sched(f) == 2 and bit(f, 18) == fa)
    inv["v2 pair split K-major"] = lambda f: kern(f) == K_V2 and bit(f, 9) and bit(f, 12) and bit(f, 13) and sched(f) == 2
    return inv


# What the dispatch cannot reach, and why (read from gemm_dispatch.h, the launchers and the functors' fast_ok() / v3_ok()).
UNREACHABLE = [
    ("v3 with rows_per_draw, or an LRT forward on it without a packed r",
     "EpiFwd::v3_ok(): the fold addresses the noise by the launch's (draw, row0) and stores r unconditionally"),
    ("v2 / v3 with draw_dev", "launch_gemm's v2_ok and try_kmajor ask !epi.has_draw_dev(): only the general kernel reads the counter"),
    ("v3 on a ragged output or with the guarded protocol (y, gx, gradWeight, a float r)", "gemm_v3_possible(): whole 256 x 256 tiles and epi.fast_ok()"),
    ("v3 accGradParameters, single accumulator, part 0", "EpiDw::fast_ok() asks lrt: a weight-noise gradient never has the fast protocol"),
    ("K-major accGradParameters on v3 with the ones row", "acc_grad_t: try_kmajor only when !gradBias (the split launch and gemm_v2 carry the row)"),
    ("a forward with a K-major side", "forward_t builds V1Form with sq alone: w and x are both stored K-contiguous"),
    ("bf16 on the latency kernel or in a pair launch", "launch_gemm_v1_form: if constexpr (sizeof(T) == 4); vbnn_backward_pair: dtype == VBNN_F32"),
    ("bf16 with TA / TB / SQ on the general kernel", "launch_gemm_v1: the operand forms are instantiated for fp32 only (VBNN_ERR_UNSUPPORTED)"),
    ("fp32 TA + TB with SQ = 1, TA alone with SQ, TB alone", "launch_gemm_v1 instantiates the forms the three entry points build, no other"),
    ("the latency kernel's wide tile with both sides K-major", "launch_gemm_v0: !(TA && TB) && v0_wide_tile()"),
    ("fp32, or single-accumulator, accGradParameters with fast_ok()", "make_dw_epi takes the shadows for sizeof(T) == 2 only; EpiDw::fast_ok() asks lrt"),
    ("v2's four-wave tiles at schedule 4; the pair split on them; K-major without the pair split",
     "launch_gemm_v2: (small || pairs) && sched == 4 runs 2; psplit = !pairs && tile != 128; kmajor && !psplit answers UNSUPPORTED"),
    ("v2's pair split for the forward or gradInput", "Epi::SPLITTABLE is EpiDw's alone"),
    ("v2's pair split at schedules 0 / 2", "reachable by VBNN_DEBUG_V2_SCHEDULE; NOT in the inventory: the split is run at its own schedule, 4"),
    ("the v3 split launch for another functor, type or with transposed outputs", "launch_gemm_v3_split: Epi::SPLITTABLE && Epi::EDGE_FAST, sizeof(T) == 2"),
    ("part 1 / 2 through the fp32 K-major forms or the pair-split launches", "acc_grad_t: a part is one single-accumulator launch via try_kmajor or launch_gemm on xT, gT"),
    ("the serial fold on anything but the dual forward", "launch_gemm_v3: if constexpr (DUAL && v3_fold_pipe<Epi>::value != 0)"),
]


def test_every_form_of_the_inventory_was_asserted_by_a_case_above():
    inv = _inventory()
    missing = [n for n, ok in inv.items() if not any(ok(f) for f in SEEN)]
    print(f"{len(SEEN)} forms seen, {len(inv)} required:", *sorted(form_name(f) for f in SEEN), sep="\n  ")
    print("largest fraction of each bound used on the device [bf16 elements accepted on the far side of a rounding midpoint]:")
    group = lambda tag: " ".join(tag.split(" ")[:2]) if tag.startswith("real") else tag.split(" ")[0]
    used, far = {}, {}
    for (fam, tag, name), v in USED.items():
        used[(fam, group(tag), name)] = max(used.get((fam, group(tag), name), 0.0), v)
    for (fam, tag, name), v in FAR.items():
        far[(fam, group(tag), name)] = far.get((fam, group(tag), name), 0) + v
    for kk in sorted(set(used) | set(far)):            # (a bf16 store has no fraction: the interval rule holds or it does not)
        print(f"  {kk[0]} {kk[1]} {kk[2]}: " + (f"{used[kk]:.3f}" if kk in used else "interval") + (f" [{far[kk]}]" if kk in far else ""))
    print("packed outputs whose pad columns came back +0:", sorted(PADS_ZEROED) or "none")
    assert not missing, f"no case above ran: {missing}"
