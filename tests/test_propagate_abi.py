"""CPU tests of the sampling-free predictive's boundary: vbnn_relu_moments_args and vbnn_logit_draws_args as gcc lays them out
from the header against the ctypes mirrors, the three symbols in the library / the ctypes table / the Lua cdef, the constants
they lean on, the ABI version unchanged (additive), and the engine's signature."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
STRUCTS = {"vbnn_relu_moments_args": "ReluMomentsArgs", "vbnn_logit_draws_args": "LogitDrawsArgs"}


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', f'#include "{os.path.join(ROOT, "include", "vbnn_philox.h")}"',
             "int main(void){",
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);',
             'printf("consts %d %d %d %d\\n", (int)VBNN_KPAD, (int)VBNN_STREAM_ZETA, (int)VBNN_F32, (int)VBNN_BF16);']
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{cname}.size %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src, "-lm"])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


@pytest.mark.parametrize("cname", list(STRUCTS))
def test_argument_structs_match_the_header(cname):
    from vbnn_amd import _lib as L
    st = getattr(L, STRUCTS[cname])
    got = _probe()
    assert int(got[f"{cname}.size"][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"{cname}.{fname}"][0]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (cname, cname), hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]                # every field of the C struct is mirrored, in order


def test_constants_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["consts"] == [str(L.KPAD), str(L.STREAM_ZETA), str(L.F32), str(L.BF16)] == ["64", "2", "0", "1"]
    assert int(got["abi"][0]) == 6                               # additive: three symbols, two structs
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    dll = C.CDLL(L.LIB_PATH)
    for name in ("vbnn_relu_moments", "vbnn_square_shadow", "vbnn_logit_draws"):
        assert name in L.exported_symbols() and hasattr(dll, name), name
    args, res = L._SIGS["vbnn_relu_moments"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(L.ReluMomentsArgs)]
    args, res = L._SIGS["vbnn_logit_draws"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(L.LogitDrawsArgs)]
    args, res = L._SIGS["vbnn_square_shadow"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert re.search(r"int vbnn_relu_moments\(vbnn_ctx\* ctx, int dtype, const vbnn_relu_moments_args\* a\);", cdef)
    assert re.search(r"int vbnn_logit_draws\(vbnn_ctx\* ctx, const vbnn_logit_draws_args\* a\);", cdef)
    assert re.search(r"int vbnn_square_shadow\(vbnn_ctx\* ctx, int dtype, const void\* src, int64_t ld_src, int64_t rows, int64_t cols,", cdef)
    assert "typedef struct vbnn_relu_moments_args {" in cdef and "typedef struct vbnn_logit_draws_args {" in cdef


def test_the_header_states_the_arithmetic():
    hdr = open(HEADER).read()
    for phrase in ("Phi = 0.5f * erfcf(-(al * 0.70710677f))", "a = max(m * Phi + s * phi, 0)", "c = max(q - a * a, 0)",
                   "a = max(m, 0);  q = a * a;  c = 0", "y[s][r][c] = m[r][c] + sqrtf(v[r][c]) * z", "no existing path reads this stream",
                   "Non-finite inputs and negative variances are out of contract"):
        assert phrase in hdr, phrase


def test_predict_analytic_surface():
    import inspect
    from vbnn_amd.engine import FusedMLP
    sig = inspect.signature(FusedMLP.predict_analytic)
    assert list(sig.parameters) == ["self", "inputs", "targets", "noise_var", "S", "row0", "topk", "keep_probs"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, None, None, 0, True]
    assert "map" not in sig.parameters
