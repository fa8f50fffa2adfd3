"""vbnn_backward_chain (include/vbnn_hip.h): updateGradInput and accGradParameters of one bf16 layer as ONE launch of the two-pass
256 x 256 kernel -- workgroup t runs tile t of the first problem, then tile t of the second (csrc/gemm_v3.h, gemm_nt_v3_chain) --
against the two separate calls, BYTE FOR BYTE: every tile runs the instruction stream of its own launch on the same operands, only
the moment it starts differs. Called through the C ABI on seeded operands; every output is a buffer of sentinels with guard rows
behind it and is compared whole (pads and guards included).

Shapes: the smallest at which both halves take the two-pass kernel on a 256-CU device (gemm_v3_shape_ok: whole 256 x 256 tiles, at
least 3/4 of the CUs, the rounds rule) -- 192 tiles each way, and 256 against 192 tiles (workgroups 192..255 run one body only).
On another CU count the shape selection differs and the cases skip."""
import ctypes as C
import functools

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 2                                   # guard rows behind every output
SENT16, SENT32 = 0x7FA5, 0x7FA5B6C7         # bf16 / fp32 NaN patterns no kernel produces
LAST_GEMM_FORM = 13
SHAPES = [(3072, 4096, 3072), (4096, 4096, 3072)]      # N, I, O: 16 x 12 / 12 x 16 tiles; 16 x 16 against 16 x 12
VAR_HAT, BB, SS = 0.75, 1e6, 1.0


def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return L, L.lib(), nn.Context.get().h


def _need_256_cus():
    L, lib, h = _ctx()
    sp, n = C.c_void_p(), C.c_int()
    L.check(lib.vbnn_ctx_stream(h, C.byref(sp), C.byref(n)))
    if n.value != 256:
        pytest.skip(f"the shapes are the smallest that take the two-pass kernel on 256 CUs; this context plans for {n.value}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _normal(gen, rows, cols, ld, std, dtype=torch.bfloat16, relu=False, square_of=None, mean=0.0):
    """rows x ld of `dtype`: seeded normals in the first `cols` columns, zero pads"""
    t = torch.zeros((rows, ld), dtype=dtype, device="cuda")
    if square_of is not None:
        v = square_of[:, :cols].float() ** 2
    else:
        v = torch.randn((rows, cols), generator=gen, device="cuda", dtype=torch.float32) * std + mean
        if relu:
            v = torch.relu(v)
    t[:, :cols] = v.to(dtype)
    return t


@functools.lru_cache(maxsize=2)
def _operands(N, I, O):
    """the seeded operands of one layer (built once per shape, never written by a launch)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * N + I + O)
    ld_w, ld_g, ld_x = I + 8, O + 8, I + 8             # K-major pitches: multiples of 8, not of the tile
    d = dict(ld_w=ld_w, ld_g=ld_g, ld_x=ld_x)
    d["w"] = _normal(gen, O, I, ld_w, 0.02)
    d["w2"] = _normal(gen, O, I, ld_w, 3e-4, mean=1e-3).abs_()
    d["g"] = _normal(gen, N, O, ld_g, 1e-2)
    d["gv"] = _normal(gen, N, O, ld_g, 1e-3)
    d["x"] = _normal(gen, N, I, ld_x, 1.0, relu=True)             # about half of it <= 0: the ReLU mask matters
    d["x2"] = _normal(gen, N, I, ld_x, 0.0, square_of=d["x"])
    d["r_prev"] = _normal(gen, N, I, ld_x, 1.0)
    d["means"] = torch.randn((O, I), generator=gen, device="cuda", dtype=torch.float32) * 0.02
    d["lvars"] = torch.randn((O, I), generator=gen, device="cuda", dtype=torch.float32) * 0.3 - 6.9
    d["mu_s"] = torch.zeros((O, ld_w), dtype=torch.bfloat16, device="cuda")
    d["mu_s"][:, :I] = d["means"].to(torch.bfloat16)
    d["var_s"] = torch.zeros((O, ld_w), dtype=torch.bfloat16, device="cuda")
    d["var_s"][:, :I] = torch.exp(d["lvars"]).to(torch.bfloat16)
    d["stats"] = torch.tensor([0.0, 0.0, VAR_HAT, 0.0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return d


def _sent16(rows, ld):
    t = torch.empty((rows + GUARD, ld), dtype=torch.bfloat16, device="cuda")
    t.view(torch.int16).fill_(SENT16)
    return t


def _sent32(n):
    t = torch.empty(n + 16 * GUARD, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(SENT32)
    return t


def _blocks(N, I, O, relu_mask, r_prev, kl, part=0):
    """fresh sentinel outputs and the two argument blocks that write them"""
    L, _, _ = _ctx()
    d = _operands(N, I, O)
    ld_gp = I + 8
    o = dict(g_prev=_sent16(N, ld_gp), gv_prev=_sent16(N, ld_gp) if r_prev else None, grad_mu=_sent32(O * I), grad_lv=_sent32(O * I))
    ax = L.DxArgs(g=_p(d["g"]), gv=_p(d["gv"]), ld_g=d["ld_g"], N=N, I=I, O=O, x=_p(d["x"]), ld_x=d["ld_x"], relu_mask=int(relu_mask),
                  r_prev=_p(d["r_prev"]) if r_prev else None, ld_r_prev=d["ld_x"] if r_prev else 0, r_prev_packed=1,
                  g_prev=_p(o["g_prev"]), gv_prev=_p(o["gv_prev"]), ld_gp=ld_gp, w=_p(d["w"]), w2=_p(d["w2"]), ld_w=d["ld_w"])
    aw = L.DwArgs(N=N, I=I, O=O, scale=1.0, accumulate=0, seed=3, layer=1, draw=4, lvars=_p(d["lvars"]), grad_mu=_p(o["grad_mu"]),
                  grad_lv=_p(o["grad_lv"]), means=_p(d["means"]), stats=_p(d["stats"]), B=BB, S=SS, kl_scale=kl,
                  x=_p(d["x"]), x2=_p(d["x2"]), g=_p(d["g"]), gv=_p(d["gv"]), ld_x=d["ld_x"], ld_g=d["ld_g"],
                  mu_s=_p(d["mu_s"]), var_s=_p(d["var_s"]), ld_w=d["ld_w"], part=part, draw_dev=None)
    return o, ax, aw


def _two_calls(N, I, O, order, **kw):
    L, lib, ctx = _ctx()
    o, ax, aw = _blocks(N, I, O, **kw)
    calls = [lambda: lib.vbnn_grad_input(ctx, L.BF16, C.byref(ax)), lambda: lib.vbnn_acc_grad_parameters(ctx, L.BF16, C.byref(aw))]
    for call in (calls if order == L.CHAIN_DX_FIRST else calls[::-1]):
        L.check(call())
    return o, lib.vbnn_debug_get(LAST_GEMM_FORM)


def _one_call(N, I, O, order, **kw):
    L, lib, ctx = _ctx()
    o, ax, aw = _blocks(N, I, O, **kw)
    L.check(lib.vbnn_backward_chain(ctx, L.BF16, C.byref(ax), C.byref(aw), order))
    return o, lib.vbnn_debug_get(LAST_GEMM_FORM), lib.vbnn_debug_get(L.DEBUG_LAST_CHAINED)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bytes(got, want, N, I, O, untouched=()):
    torch.cuda.synchronize()
    for k, w in want.items():
        if w is None:
            assert got[k] is None
            continue
        assert torch.equal(_bits(got[k]), _bits(w)), f"{k}: the one call and the two calls differ"
        b = _bits(got[k])
        if k in untouched:
            assert bool((b == SENT32).all()), f"{k} was written"
        elif b.ndim == 2:
            assert bool((b[N:] == SENT16).all()), f"{k}: a guard row was written"
            assert bool((b[:N, :I] != SENT16).any(dim=1).all()), f"{k}: a row was left unwritten"
        else:
            assert bool((b[O * I:] == SENT32).all()), f"{k}: written past its end"
            assert not bool((b[:O * I] == SENT32).any()), f"{k}: an element was left unwritten"


@pytest.mark.parametrize("N,I,O", SHAPES)
@pytest.mark.parametrize("order", ["dx", "dw"])
@pytest.mark.parametrize("relu_mask", [True, False])
@pytest.mark.parametrize("r_prev", [True, False])
@pytest.mark.parametrize("kl", [0.0, 0.5])
def test_chained_launch_is_its_two_launches(N, I, O, order, relu_mask, r_prev, kl):
    """g_prev, gv_prev, grad_mu, grad_lv of one vbnn_backward_chain call equal the two separate calls byte for byte, the call says it
    went out as one launch, and the last-form query reads as after the two calls"""
    _need_256_cus()
    L, lib, _ = _ctx()
    code = L.CHAIN_DX_FIRST if order == "dx" else L.CHAIN_DW_FIRST
    kw = dict(relu_mask=relu_mask, r_prev=r_prev, kl=kl)
    want, form2 = _two_calls(N, I, O, code, **kw)
    got, form1, chained = _one_call(N, I, O, code, **kw)
    assert chained == 1, "both halves take the two-pass kernel at this shape: the call must chain"
    assert form1 == form2 and (form1 & 15) == 6, (hex(form1), hex(form2))         # VBNN_GEMM_KERNEL_V3
    _same_bytes(got, want, N, I, O)


@pytest.mark.parametrize("order", ["dx", "dw"])
def test_ineligible_or_switched_off_is_the_two_calls(order):
    """part = 2 (one GEMM of the pair: not the plain two-pass form) and VBNN_DEBUG_CHAIN_OFF take the two-call path and say so"""
    _need_256_cus()
    L, lib, _ = _ctx()
    N, I, O = SHAPES[0]
    code = L.CHAIN_DX_FIRST if order == "dx" else L.CHAIN_DW_FIRST
    kw = dict(relu_mask=True, r_prev=True, kl=0.0)
    want, form2 = _two_calls(N, I, O, code, part=2, **kw)
    got, form1, chained = _one_call(N, I, O, code, part=2, **kw)
    assert chained == 0 and form1 == form2
    _same_bytes(got, want, N, I, O, untouched=("grad_mu",))
    want, form2 = _two_calls(N, I, O, code, **kw)
    L.check(lib.vbnn_debug_set(L.DEBUG_CHAIN_OFF, 1))
    try:
        got, form1, chained = _one_call(N, I, O, code, **kw)
    finally:
        L.check(lib.vbnn_debug_set(L.DEBUG_CHAIN_OFF, 0))
    assert chained == 0 and form1 == form2
    _same_bytes(got, want, N, I, O)
    got, _, chained = _one_call(N, I, O, code, **kw)
    assert chained == 1                                                            # and the key's default is back
    _same_bytes(got, want, N, I, O)


@pytest.mark.parametrize("order", ["dx", "dw"])
def test_engine_step_with_the_chained_backward_is_bitwise_the_step_without(order):
    """two engines from one seed, 784-4096-3072-10 on 3072 rows (the second layer is the first shape above), opt.chain_backward on and
    off: after one step the gradient arena, the loss and the hit count are equal byte for byte"""
    _need_256_cus()
    L, lib, _ = _ctx()
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    N, I0 = SHAPES[0][0], 784
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    res = []
    for chain in (False, order):
        eng = FusedMLP(dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=I0, hidden=[4096, 3072],
                            n_classes=10, type="vb", keep_e=True, testSamples=2, fuse_kl=True, chain_backward=chain))
        eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t); eng.finish()
        loss, hits = eng.loss_and_accuracy()
        if chain:
            assert eng.chain_backward == order and lib.vbnn_debug_get(L.DEBUG_LAST_CHAINED) == 1, "the second layer's pair must chain"
        res.append((eng.grads.clone(), loss, hits))
        del eng
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2], (res[0][1:], res[1][1:])
    assert bool(torch.isfinite(res[0][0]).all()) and float(res[0][0].abs().max()) > 0.0
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
