"""CPU tests of the class-probability predictive's boundary: vbnn_class_moments_args as gcc lays it out from the header against
the ctypes mirror, the symbol in the library / the ctypes table / the Lua cdef, the STACKED cap, the ABI version unchanged
(additive), predict_classes' signature, and the fp32 restatement of tests/_classes_np.py inside the bounds its GPU tests use."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from tests._classes_np import KERNEL_CASES, case_inputs, check_classes, classes32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")


def _probe():
    from vbnn_amd import _lib as L
    st = L.ClassMomentsArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_class_moments_args));',
             'printf("stacked %d accumulate %d\\n", (int)VBNN_MOMENTS_STACKED, (int)VBNN_MOMENTS_ACCUMULATE);',
             'printf("cap %lld\\n", (long long)VBNN_CLASS_MOMENTS_STACKED_MAX_C);',
             'printf("maxk %lld\\n", (long long)VBNN_CLASS_MOMENTS_MAX_K);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_class_moments_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_class_moments_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.ClassMomentsArgs
    got = _probe()
    assert int(got["size"][0]) == C.sizeof(st)
    assert got["stacked"] == [str(L.MOMENTS_STACKED), "accumulate", str(L.MOMENTS_ACCUMULATE)]
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_class_moments_args \{(.*?)\}\s*vbnn_class_moments_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]


def test_stacked_cap_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert int(got["cap"][0]) == 4096 == L.CLASS_MOMENTS_STACKED_MAX_C
    assert int(got["maxk"][0]) == 8 == L.CLASS_MOMENTS_MAX_K
    assert int(got["abi"][0]) == 6                              # additive: one symbol, one struct
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_class_moments_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    assert "vbnn_predict_class_moments" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "vbnn_predict_class_moments")
    args, res = L._SIGS["vbnn_predict_class_moments"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.ClassMomentsArgs)
    assert re.search(r"^int vbnn_predict_class_moments\(vbnn_ctx\* ctx, const vbnn_class_moments_args\* a\);$", open(HEADER).read(),
                     flags=re.M)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert re.search(r"int vbnn_predict_class_moments\(vbnn_ctx\* ctx, const vbnn_class_moments_args\* a\);", cdef)
    assert "typedef struct vbnn_class_moments_args {" in cdef


def test_predict_classes_surface():
    """The engine's entry point exists with the documented signature, the result carries the new attributes, predict keeps its own."""
    import inspect
    from vbnn_amd.engine import FusedMLP, PredictResult
    sig = inspect.signature(FusedMLP.predict_classes)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "map", "row0", "topk", "keep_probs", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, None, 0, True, False]
    r = PredictResult(*range(6))
    assert (r.probs, r.log_probs, r.entropy, r.expected_entropy, r.mutual_info, r.pred) == tuple(range(6))
    assert r.topk_idx is None and r.topk_prob is None and r.topk_accuracy is None and r.draws is None
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_fp32_restatement_is_inside_the_bounds(name):
    """The arithmetic the header states, in plain fp32 with sequential row sums, passes check_classes on every kernel case:
    the bounds leave room for any order of the row sums."""
    y, t, K = case_inputs(name)
    got = classes32(y, t, K)
    check_classes(got, y, t, K, label=name + " fp32 restatement")
    bare = classes32(y, None, 0)
    assert "totals" not in bare and "topk_idx" not in bare
    check_classes(bare, y, None, 0, label=name + " fp32 restatement, no target, K = 0")
