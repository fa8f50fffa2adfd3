"""CPU tests of the Bernoulli head's boundary: vbnn_label_moments_args as gcc lays it out from the header against the ctypes
mirror, the three symbols in the library / the ctypes table / the Lua cdef, the STACKED cap, the ABI version unchanged
(additive), the engine's surface, and the shipped kernels' private memory."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
SYMBOLS = ("vbnn_bce_forward", "vbnn_bce_backward", "vbnn_predict_label_moments")


def _probe():
    from vbnn_amd import _lib as L
    st = L.LabelMomentsArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_label_moments_args));',
             'printf("cap %lld\\n", (long long)VBNN_LABEL_MOMENTS_STACKED_MAX_D);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_label_moments_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_label_moments_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.LabelMomentsArgs
    got = _probe()
    assert int(got["size"][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_label_moments_args \{(.*?)\}\s*vbnn_label_moments_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]
    assert int(got["cap"][0]) >= 1024 and int(got["cap"][0]) == L.LABEL_MOMENTS_STACKED_MAX_D


def test_symbols_are_exported_and_declared_everywhere_and_the_abi_is_still_6():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    so = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert name in L.exported_symbols() and name in L._SIGS, name
        assert hasattr(so, name), name
        assert re.search(r"int %s\(vbnn_ctx\* ctx, " % name, cdef), name
    args, res = L._SIGS["vbnn_predict_label_moments"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.LabelMomentsArgs)
    assert len(L._SIGS["vbnn_bce_forward"][0]) == 13 and len(L._SIGS["vbnn_bce_backward"][0]) == 10
    assert "typedef struct vbnn_label_moments_args {" in cdef
    assert int(_probe()["abi"][0]) == 6
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6
    hdr = open(HEADER).read()
    assert "no log of an average is ever -inf" in hdr                   # the header says what the clamp is for


def test_engine_surface():
    from vbnn_amd.engine import FusedMLP, LabelPredictResult
    sig = inspect.signature(FusedMLP.predict_labels)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "map", "row0", "keep_draws"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, None, False]
    r = LabelPredictResult(*range(5))
    assert (r.probs, r.entropy, r.mutual_info, r.row_entropy, r.row_mutual_info) == tuple(range(5))
    for k in ("row_log_lik", "row_marg_log_lik", "row_hits", "log_lik", "marg_log_lik", "mean_draw_bce", "label_accuracy",
              "exact_match", "draws", "totals"):
        assert getattr(r, k) is None, k
    from vbnn_amd import data
    assert list(inspect.signature(data.synthetic_multilabel).parameters)[:5] == ["n_train", "n_test", "n_labels", "seed", "noise"]


def test_label_kernels_use_no_private_memory():
    """The shipped code object's Bernoulli kernels (criterion, STACKED at a wave per row and at the three register tiles of a
    workgroup per row, ACCUMULATE at both row widths): no scratch memory, no VGPR spills (tools/kernel_regs.py). The widest
    STACKED tile (4 quads a thread, D <= VBNN_LABEL_MOMENTS_STACKED_MAX_D; 234 VGPRs as built) stays within 256 VGPRs, two
    waves per SIMD; every other kernel within 168, three waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if "k_label_" in k["name"] or "k_bce" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_bce", "k_label_stacked", "k_label_accumulate"):
        assert want in names, (want, names)
    assert len([k for k in ks if "k_label_stacked" in k["name"]]) == 4
    assert len([k for k in ks if "k_label_accumulate" in k["name"]]) == 2
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 8192, k
        assert int(k["vgpr"]) + int(k["agpr"]) <= (256 if "k_label_stackedILi4ELi4EE" in k["name"] else 168), k
