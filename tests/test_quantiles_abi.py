"""CPU tests of the quantile predictive's boundary: vbnn_quantiles_args as gcc lays it out from the header against the ctypes
mirror, the symbol in the library / the ctypes table / the Lua cdef, the caps, the ABI version unchanged (additive), and the
engine's signatures."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")


def _probe():
    from vbnn_amd import _lib as L
    st = L.QuantilesArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_quantiles_args));',
             'printf("kinds %d %d %d\\n", (int)VBNN_QUANT_EMPIRICAL, (int)VBNN_QUANT_FIXED_NOISE, (int)VBNN_QUANT_GAUSS);',
             'printf("caps %d %d\\n", (int)VBNN_QUANTILES_MAX_S, (int)VBNN_QUANTILES_MAX_Q);',
             'printf("plen %zu\\n", sizeof(((vbnn_quantiles_args*)0)->p) / sizeof(float));',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_quantiles_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_quantiles_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.QuantilesArgs
    got = _probe()
    assert int(got["size"][0]) == C.sizeof(st)
    assert got["kinds"] == [str(L.QUANT_EMPIRICAL), str(L.QUANT_FIXED_NOISE), str(L.QUANT_GAUSS)] == ["0", "1", "2"]
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order (p is the one array)
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_quantiles_args \{(.*?)\}\s*vbnn_quantiles_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]


def test_caps_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["caps"] == ["128", "8"] and (L.QUANTILES_MAX_S, L.QUANTILES_MAX_Q) == (128, 8)
    assert int(got["plen"][0]) == 8 == len(L.QuantilesArgs().p)
    assert int(got["abi"][0]) == 6                              # additive: one symbol, one struct
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_quantiles_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    assert "vbnn_predict_quantiles" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "vbnn_predict_quantiles")
    args, res = L._SIGS["vbnn_predict_quantiles"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.QuantilesArgs)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert re.search(r"int vbnn_predict_quantiles\(vbnn_ctx\* ctx, const vbnn_quantiles_args\* a\);", cdef)
    assert "typedef struct vbnn_quantiles_args {" in cdef and "float p[8];" in cdef


def test_predict_quantiles_surface():
    """The engine's entry point and its result type exist with the documented signature; predict_regression and predict keep
    theirs."""
    import inspect
    from vbnn_amd.engine import FusedMLP, QuantilePredictResult, RegressionPredictResult
    sig = inspect.signature(FusedMLP.predict_quantiles)
    assert list(sig.parameters) == ["self", "inputs", "probs", "S", "targets", "noise_var", "map", "row0", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, None, False, None, False]
    assert sig.parameters["probs"].default is inspect.Parameter.empty
    sig = inspect.signature(FusedMLP.predict_regression)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "noise_var", "map", "row0", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, None, False, None, False]
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]
    mom = RegressionPredictResult(*range(6))
    r = QuantilePredictResult([0.25, 0.75], "q", mom, "empirical")
    assert r.probs == [0.25, 0.75] and r.quantiles == "q" and r.moments is mom and r.kind == "empirical"
    assert r.pit is None and r.row_le is None and r.calibration is None and r.draws is None
    assert callable(r.interval)
