"""CPU tests of the calibration boundary: vbnn_calibration_args and vbnn_selective_args as gcc lays them out from the header
against the ctypes mirrors, the two symbols in the library / the ctypes table / the Lua cdef, the caps, the ABI version unchanged
(additive), and the engine's signatures."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
STRUCTS = {"vbnn_calibration_args": "CalibrationArgs", "vbnn_selective_args": "SelectiveArgs"}


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("caps %d %d\\n", (int)VBNN_CALIBRATION_MAX_BINS, (int)VBNN_SELECTIVE_MAX_Q);',
             'printf("klen %zu\\n", sizeof(((vbnn_selective_args*)0)->k) / sizeof(int64_t));',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for cname, pname in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(L, pname)._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


@pytest.mark.parametrize("cname", list(STRUCTS))
def test_args_match_the_header(cname):
    from vbnn_amd import _lib as L
    st = getattr(L, STRUCTS[cname])
    got = _probe()
    assert int(got[cname][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"{cname}.{fname}"][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order (k is the one array)
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (cname, cname), hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]


def test_caps_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["caps"] == ["64", "32"] and (L.CALIBRATION_MAX_BINS, L.SELECTIVE_MAX_Q) == (64, 32)
    assert int(got["klen"][0]) == 32 == len(L.SelectiveArgs().k)
    assert int(got["abi"][0]) == 6                              # additive: two symbols, two structs
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for sym, cname in (("vbnn_predict_calibration", "vbnn_calibration_args"), ("vbnn_selective", "vbnn_selective_args")):
        assert sym in L.exported_symbols()
        assert hasattr(C.CDLL(L.LIB_PATH), sym)
        args, res = L._SIGS[sym]
        assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(getattr(L, STRUCTS[cname]))
        assert re.search(r"int %s\(vbnn_ctx\* ctx, const %s\* a\);" % (sym, cname), cdef)
        assert f"typedef struct {cname} {{" in cdef
    assert "int64_t k[32];" in cdef


def test_engine_surface():
    """The two entry points and their result types exist with the documented signatures; predict and predict_classes keep theirs."""
    from vbnn_amd.engine import CalibrationResult, FusedMLP, SelectiveResult
    sig = inspect.signature(FusedMLP.calibration)
    assert list(sig.parameters) == ["self", "result", "targets", "bins", "into"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [15, None]
    assert list(inspect.signature(FusedMLP.selective).parameters) == ["self", "score", "hit", "coverages"]
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]
    sig = inspect.signature(FusedMLP.predict_classes)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "map", "row0", "topk", "keep_probs", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, None, 0, True, False]
    # the host arithmetic on integers alone (no device): two bins, merge adds
    a = CalibrationResult(2, None, [1, 3, 0, 2, 1 << 30, 5 << 31, 1 << 32, 4, 0, 0])
    assert a.bin_count == [1, 3] and a.bin_hits == [0, 2] and a.n == 4 and a.n_nan == 0 and a.accuracy == 0.5
    assert a.bin_confidence == [0.25, 2.5 / 3] and a.bin_accuracy == [0.0, 2 / 3]
    assert a.ece == (0.25 + 0.5) / 4 and a.mce == 0.25 and a.brier == 0.25
    b = a.merge(a)
    assert b.n == 8 and b.ece == a.ece and b.bin_count == [2, 6] and b.conf is None
    s = SelectiveResult([0.5], [2], [0.0], [[0, 0, 4, 3]])
    assert s.accuracy == [0.75] and s.k == [2] and s.threshold == [0.0]
