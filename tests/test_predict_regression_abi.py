"""CPU tests of the regression predictive's boundary: vbnn_moments_args as gcc lays it out from the header against the ctypes
mirror, the symbol in the library / the ctypes table / the Lua cdef, the STACKED cap, and the ABI version unchanged (additive)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")


def _probe():
    from vbnn_amd import _lib as L
    st = L.MomentsArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_moments_args));',
             'printf("stacked %d accumulate %d\\n", (int)VBNN_MOMENTS_STACKED, (int)VBNN_MOMENTS_ACCUMULATE);',
             'printf("cap %lld\\n", (long long)VBNN_MOMENTS_STACKED_MAX_D);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_moments_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_moments_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.MomentsArgs
    got = _probe()
    assert int(got["size"][0]) == C.sizeof(st)
    assert got["stacked"] == [str(L.MOMENTS_STACKED), "accumulate", str(L.MOMENTS_ACCUMULATE)]
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_moments_args \{(.*?)\}\s*vbnn_moments_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]


def test_stacked_cap_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert int(got["cap"][0]) >= 4096 and int(got["cap"][0]) == L.MOMENTS_STACKED_MAX_D
    assert int(got["abi"][0]) == 6                              # additive: one symbol, one struct
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_moments_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    assert "vbnn_predict_moments" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "vbnn_predict_moments")
    args, res = L._SIGS["vbnn_predict_moments"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.MomentsArgs)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert re.search(r"int vbnn_predict_moments\(vbnn_ctx\* ctx, const vbnn_moments_args\* a\);", cdef)
    assert "typedef struct vbnn_moments_args {" in cdef


def test_predict_regression_surface():
    """The engine's entry point and its result type exist with the documented signature; predict keeps its own."""
    import inspect
    from vbnn_amd.engine import FusedMLP, RegressionPredictResult
    sig = inspect.signature(FusedMLP.predict_regression)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "noise_var", "map", "row0", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, None, False, None, False]
    r = RegressionPredictResult(*range(6))
    assert (r.mean, r.var, r.row_var, r.row_sq_err, r.row_log_lik, r.draws) == tuple(range(6))
    assert r.totals is None and r.mse is None and r.mean_draw_mse is None and r.log_lik is None and r.mean_var is None
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]
