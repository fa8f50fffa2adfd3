"""GPU tests of the MSE criterion, vbnn_mse_forward / _backward (include/vbnn_hip.h), through the C ABI, in the shape of the
`gauss` and `bce` criterion tests: every access path (dense, odd pitches, a base one float off a 16-byte boundary -- the scalar
path --, and 16-byte aligned rows with pitches that are multiples of four -- the vector path), against NumPy on the same fp32
inputs.

The bounds are derived. g = 2 inv_nd (y - t): the difference is one fp32 rounding, the doubling of inv_nd is exact, the product
one more rounding -- so g is BITWISE fl((2 inv_nd) fl(y - t)) in NumPy fp32. The loss is inv_nd times a double sum of the squares
of the fp32 differences: every square is exact in double (24 x 24 bits), every term is non-negative, so N D - 1 additions, the
scaling and one conversion are off by at most (N D + 2) 2^-53 relative of inv_nd math.fsum(d^2)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (7, 64), (5, 67), (33, 130)]
SENT = 0x7FA5B6C7                       # an fp32 NaN pattern no kernel produces
GUARD = 2                               # guard rows behind g
U = 2.0 ** -53


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def layouts(D):
    """name: (ld_y, ld_t, ld_g, base offset of y / t / g in floats, whether the kernel may take 16-byte accesses)"""
    x4 = (D + 3) // 4 * 4 + 4
    return {"dense": (D, D, D, 0, D % 4 == 0),
            "pitch+3": (D + 3, D + 3, D + 3, 0, False),
            "off-by-one-float": (D, D, D, 1, False),
            "pitch-x4": (x4, x4 + 4, x4 + 8, 0, D % 4 == 0)}


def data(N, D, seed=41):
    rng = np.random.default_rng(seed + 1000 * N + D)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)


def _padded(a2d, ld, offset):
    rows, W = a2d.shape
    buf = torch.full((rows * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + rows * ld].view(rows, ld)[:, :W] = dev(a2d)
    assert buf.data_ptr() % 16 == 0
    return buf, C.c_void_p(buf.data_ptr() + 4 * offset)


def run_mse(y, t, inv_nd, layout, accumulate=0, loss0=0.0, backward=False, with_g=True):
    """One call. Returns (loss or None, g as N x D or None, True where every pad column and guard row of g kept the sentinel)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    N, D = y.shape
    ld_y, ld_t, ld_g, off, _ = layout
    ybuf, yptr = _padded(y, ld_y, off)
    tbuf, tptr = _padded(t, ld_t, off)
    gbuf = torch.full(((N + GUARD) * ld_g + off + 4,), 0, dtype=torch.int32, device="cuda")
    gbuf.fill_(SENT)
    gptr = C.c_void_p(gbuf.data_ptr() + 4 * off)
    loss = torch.full((1,), loss0, dtype=torch.float64, device="cuda")
    if backward:
        L.check(lib.vbnn_mse_backward(ctx, yptr, ld_y, tptr, ld_t, N, D, inv_nd, gptr, ld_g))
    else:
        L.check(lib.vbnn_mse_forward(ctx, yptr, ld_y, tptr, ld_t, N, D, inv_nd, gptr if with_g else None, ld_g if with_g else 0,
                                     accumulate, _p(loss)))
    words = host(gbuf)
    body = words[off:off + (N + GUARD) * ld_g].reshape(N + GUARD, ld_g)
    clean = bool((body[:N, D:] == SENT).all() and (body[N:] == SENT).all() and (words[:off] == SENT).all() and
                 (words[off + (N + GUARD) * ld_g:] == SENT).all())
    if not with_g:
        clean = clean and bool((body == SENT).all())
    g = np.ascontiguousarray(body[:N, :D]).view(np.float32) if with_g else None
    del ybuf, tbuf
    return (None if backward else float(host(loss)[0])), g, clean


def want_g(y, t, inv_nd):
    return (np.float32(2.0) * np.float32(inv_nd)) * (y - t)                     # fp32 throughout: two roundings


def want_loss(y, t, inv_nd):
    d = (y - t).astype(np.float64)                                              # the fp32 difference, squared exactly
    return float(np.float32(inv_nd)) * math.fsum((d * d).ravel())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", ["dense", "pitch+3", "off-by-one-float", "pitch-x4"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_forward_and_backward_on_every_layout(N, D, name):
    """g bitwise, the loss within (N D + 2) 2^-53, pads and guard rows untouched, accumulate, the optional g, _backward's g, and
    two calls agreeing bit for bit -- on every access path."""
    y, t = data(N, D)
    inv_nd = 1.0 / (N * D)
    lay = layouts(D)[name]
    loss, g, clean = run_mse(y, t, inv_nd, lay)
    assert clean, "the forward wrote outside g"
    assert same_bits(g, want_g(y, t, inv_nd))
    want = want_loss(y, t, inv_nd)
    share = abs(loss - want) / ((N * D + 2) * U * abs(want)) if want else 0.0
    print(f"mse {N}x{D} {name}: loss {loss!r} want {want!r}, err/bound {share:.3f}")
    assert abs(loss - want) <= (N * D + 2) * U * abs(want)
    # determinism: the same bits again
    loss2, g2, _ = run_mse(y, t, inv_nd, lay)
    assert loss2 == loss and same_bits(g2, g)
    # accumulate = 1 adds to the previous value: one product and one addition (or one fused step) in double
    loss0 = 3.25
    acc, _, clean = run_mse(y, t, inv_nd, lay, accumulate=1, loss0=loss0)
    assert clean and abs(acc - (loss0 + loss)) <= 2 * U * (abs(loss0) + abs(loss))
    over, _, _ = run_mse(y, t, inv_nd, lay, accumulate=0, loss0=loss0)
    assert over == loss                                                          # accumulate = 0 overwrites
    # g = NULL: the same loss bits, nothing written
    alone, _, clean = run_mse(y, t, inv_nd, lay, with_g=False)
    assert clean and alone == loss
    # _backward: the forward's g
    _, gb, clean = run_mse(y, t, inv_nd, lay, backward=True)
    assert clean and same_bits(gb, g)


@pytest.mark.parametrize("name", ["dense", "off-by-one-float"])
def test_a_nan_reaches_the_loss_and_its_own_gradient_only(name):
    N, D = 7, 64
    y, t = data(N, D)
    y[3, 17] = np.nan
    inv_nd = 1.0 / (N * D)
    loss, g, clean = run_mse(y, t, inv_nd, layouts(D)[name])
    assert clean and math.isnan(loss)
    bad = np.isnan(g)
    assert bad[3, 17] and bad.sum() == 1
    keep = ~bad
    assert np.array_equal(g[keep].view(np.uint32), want_g(y, t, inv_nd)[keep].view(np.uint32))


def test_refusals():
    """NULL arguments, N or D of 0, each leading dimension below D: a status and a message, no launch."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, ctx = L.lib(), Context.get().h
    N, D = 3, 5
    y, t = (dev(a) for a in data(N, D))
    g = torch.full((N, D), 7.0, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    inv = 1.0 / (N * D)

    def fwd(**kw):
        a = dict(ctx=ctx, y=_p(y), ld_y=D, t=_p(t), ld_t=D, N=N, D=D, g=_p(g), ld_g=D, loss=_p(loss))
        a.update(kw)
        return lib.vbnn_mse_forward(a["ctx"], a["y"], a["ld_y"], a["t"], a["ld_t"], a["N"], a["D"], inv, a["g"], a["ld_g"], 0, a["loss"])

    def bwd(**kw):
        a = dict(ctx=ctx, y=_p(y), ld_y=D, t=_p(t), ld_t=D, N=N, D=D, g=_p(g), ld_g=D)
        a.update(kw)
        return lib.vbnn_mse_backward(a["ctx"], a["y"], a["ld_y"], a["t"], a["ld_t"], a["N"], a["D"], inv, a["g"], a["ld_g"])

    for kw in (dict(ctx=None), dict(y=None), dict(t=None), dict(loss=None), dict(N=0), dict(D=0), dict(ld_y=D - 1), dict(ld_t=D - 1),
               dict(ld_g=D - 1)):
        assert fwd(**kw) != 0 and len(lib.vbnn_last_error()) > 0, kw
    for kw in (dict(ctx=None), dict(y=None), dict(t=None), dict(g=None), dict(N=0), dict(D=0), dict(ld_y=D - 1), dict(ld_t=D - 1),
               dict(ld_g=D - 1)):
        assert bwd(**kw) != 0 and len(lib.vbnn_last_error()) > 0, kw
    torch.cuda.synchronize()
    assert float(loss[0]) == 5.0 and bool((g == 7.0).all())                      # nothing ran
    assert fwd() == 0 and bwd() == 0                                             # and the calls themselves are fine
