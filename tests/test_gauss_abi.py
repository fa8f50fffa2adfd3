"""CPU tests of the heteroscedastic Gaussian head's boundary: vbnn_gauss_moments_args as gcc lays it out from the header against
the ctypes mirror, the three symbols in the library / the ctypes table / the Lua cdef, the STACKED cap, the ABI version
unchanged (additive), the engine's surface, the shipped kernels' private memory, and the float64 restatement of the criterion
(tests/_gauss_np.py) against central differences of its own loss."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
SYMBOLS = ("vbnn_gauss_nll_forward", "vbnn_gauss_nll_backward", "vbnn_predict_gauss_moments")


def _probe():
    from vbnn_amd import _lib as L
    st = L.GaussMomentsArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_gauss_moments_args));',
             'printf("cap %lld\\n", (long long)VBNN_GAUSS_MOMENTS_STACKED_MAX_D);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_gauss_moments_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_gauss_moments_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.GaussMomentsArgs
    got = _probe()
    assert int(got["size"][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_gauss_moments_args \{(.*?)\}\s*vbnn_gauss_moments_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]
    assert int(got["cap"][0]) >= 1024 and int(got["cap"][0]) == L.GAUSS_MOMENTS_STACKED_MAX_D


def test_symbols_are_exported_and_declared_everywhere_and_the_abi_is_still_6():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    so = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert name in L.exported_symbols() and name in L._SIGS, name
        assert hasattr(so, name), name
        assert re.search(r"int %s\(vbnn_ctx\* ctx, " % name, cdef), name
    args, res = L._SIGS["vbnn_predict_gauss_moments"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.GaussMomentsArgs)
    assert len(L._SIGS["vbnn_gauss_nll_forward"][0]) == 14 and len(L._SIGS["vbnn_gauss_nll_backward"][0]) == 12
    assert "typedef struct vbnn_gauss_moments_args {" in cdef
    assert int(_probe()["abi"][0]) == 6
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6
    hdr = open(HEADER).read()
    assert "WITHOUT its constant 0.5 log(2 pi)" in hdr                  # the header says what the loss leaves out


def test_engine_surface():
    from vbnn_amd.engine import FusedMLP, RegressionPredictResult
    sig = inspect.signature(FusedMLP.predict_regression)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "noise_var", "map", "row0", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, None, False, None, False]
    r = RegressionPredictResult(*range(6))
    assert (r.mean, r.var, r.row_var, r.row_sq_err, r.row_log_lik, r.draws) == tuple(range(6))
    for k in ("noise_var", "row_noise_var", "mean_noise_var", "mean_draw_nll", "mean_draw_mse", "totals", "log_lik"):
        assert getattr(r, k) is None, k
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]


def test_gauss_kernels_use_no_private_memory():
    """The shipped code object's Gaussian kernels (criterion, both moments forms at both row widths, the five-total finish):
    no scratch memory, no VGPR spills (tools/kernel_regs.py). The STACKED form has two register tiles at a workgroup per row
    (4 and 8 quads per thread); VBNN_GAUSS_MOMENTS_STACKED_MAX_D is the wider one's reach."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if "k_gauss_" in k["name"] or "GaussFamily" in k["name"] or "k_moments_finish" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_gauss_nll", "k_moments_stackedI11GaussFamily", "k_moments_accumulateI11GaussFamily", "k_moments_finishILi5E"):
        assert want in names, (want, names)
    assert len([k for k in ks if "k_moments_stackedI11GaussFamily" in k["name"]]) == 3  # a wave per row / a workgroup per row, two tiles
    assert len([k for k in ks if "k_moments_accumulateI11GaussFamily" in k["name"]]) == 2
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 8192, k


@pytest.mark.parametrize("N,D,scale", [(1, 1, 1.0), (3, 5, 4.0), (4, 16, 12.0), (8, 8, 1.0)])
def test_restated_gradients_match_central_differences(N, D, scale):
    """tests/_gauss_np.py's analytic g_m and g_s against float64 central differences of its own loss (N D <= 64, relative 1e-6),
    the exact zero of g_s outside the clamp included."""
    from tests import _gauss_np as G
    assert N * D <= 64
    rng = np.random.default_rng(N * 100 + D)
    s_min, s_max = -3.0, 3.0
    y = np.concatenate([rng.standard_normal((N, D)), scale * rng.standard_normal((N, D))], 1)
    t = rng.standard_normal((N, D))
    near = np.abs(np.abs(y[:, D:]) - 3.0) < 1e-3                         # (a difference must not straddle the clamp's kink)
    y[:, D:][near] += 0.01
    inv_nd = float(np.float32(1.0 / (N * D)))
    ref = G.criterion64(y, t, inv_nd, s_min, s_max)
    g = np.concatenate([ref["g_m"], ref["g_s"]], 1)
    h = 1e-5
    num = np.zeros_like(y)
    for i in range(N):
        for j in range(2 * D):
            yp, ym = y.copy(), y.copy()
            yp[i, j] += h
            ym[i, j] -= h
            num[i, j] = (G.loss_only64(yp, t, inv_nd, s_min, s_max) - G.loss_only64(ym, t, inv_nd, s_min, s_max)) / (2 * h)
    out = ~ref["inside"]
    assert (ref["g_s"][out] == 0.0).all() and (num[:, D:][out] == 0.0).all()
    if scale >= 4.0:
        assert out.any() and ref["inside"].any()
    # relative 1e-6, plus what the rounding of the two float64 losses leaves in their difference (2^-52 |loss| / 2 h each side)
    tol = 1e-6 * np.abs(g) + 4 * 2.0 ** -52 * max(abs(ref["loss"]), ref["loss_mag"]) / (2 * h)
    assert (np.abs(num - g) <= tol).all(), float((np.abs(num - g) / tol).max())
