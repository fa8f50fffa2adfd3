"""CPU tests of the rank-metrics boundary: vbnn_rank_metrics_args as gcc lays it out from the header against the ctypes mirror, the
two symbols in the library / the ctypes table / the Lua cdef, the cap, the ABI version unchanged (additive), the engine's
signature and the host arithmetic of RankingResult on integers alone, and the two kernels as built (no scratch, no spills)."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
CNAME, PNAME = "vbnn_rank_metrics_args", "RankMetricsArgs"


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("cap %d\\n", (int)VBNN_RANK_MAX_Q);',
             f'printf("taulen %zu\\n", sizeof((({CNAME}*)0)->tau) / sizeof(float));',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);', f'printf("{CNAME} %zu\\n", sizeof({CNAME}));']
    for fname, _ in getattr(L, PNAME)._fields_:
        lines.append(f'printf("{CNAME}.{fname} %zu\\n", offsetof({CNAME}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


def test_args_match_the_header():
    from vbnn_amd import _lib as L
    st = getattr(L, PNAME)
    got = _probe()
    assert int(got[CNAME][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"{CNAME}.{fname}"][0]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (CNAME, CNAME), hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]              # every field of the C struct is mirrored, in order


def test_cap_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["cap"] == ["16"] and L.RANK_MAX_Q == 16
    assert int(got["taulen"][0]) == 16 == len(L.RankMetricsArgs().tau)
    assert int(got["abi"][0]) == 6                              # additive: two symbols, one struct
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for sym in ("vbnn_rank_metrics", "vbnn_rank_metrics_workspace_bytes"):
        assert sym in L.exported_symbols()
        assert hasattr(C.CDLL(L.LIB_PATH), sym)
    args, res = L._SIGS["vbnn_rank_metrics"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.RankMetricsArgs)
    args, res = L._SIGS["vbnn_rank_metrics_workspace_bytes"]
    assert res is C.c_int and args == [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
    assert re.search(r"int vbnn_rank_metrics\(vbnn_ctx\* ctx, const %s\* a\);" % CNAME, cdef)
    assert re.search(r"int vbnn_rank_metrics_workspace_bytes\(int64_t R, int64_t D, size_t\* bytes\);", cdef)
    assert f"typedef struct {CNAME} {{" in cdef and "float tau[16];" in cdef


def test_workspace_bytes_needs_no_device():
    """The size formula of the header: 16 R D bytes; shapes outside the contract are refused and leave `bytes` alone."""
    from vbnn_amd import _lib as L
    n = C.c_size_t(7)
    for R, D in ((1, 1), (5000, 67), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1), (46340, 46340)):
        assert L.lib().vbnn_rank_metrics_workspace_bytes(R, D, C.byref(n)) == 0 and n.value == 16 * R * D
    n = C.c_size_t(7)
    for R, D in ((0, 1), (1, 0), (-1, 5), (2 ** 31, 1), (46341, 46341), (2 ** 40, 2 ** 40)):
        assert L.lib().vbnn_rank_metrics_workspace_bytes(R, D, C.byref(n)) != 0 and n.value == 7
    assert L.lib().vbnn_rank_metrics_workspace_bytes(4, 4, None) != 0


def test_engine_surface():
    from vbnn_amd.engine import FusedMLP, RankingResult
    sig = inspect.signature(FusedMLP.ranking)
    assert list(sig.parameters) == ["self", "scores", "targets", "thresholds", "micro"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [(0.5,), False]
    # the host arithmetic on integers alone (no device): two labels, one threshold; the second label has no negatives
    r = RankingResult([[2, 3, 1, 9, 3 << 31, 0, 1, 1], [4, 0, 0, 0, 4 << 32, 0, 4, 0]], [0.5], [6, 3, 1, 27, 9 << 31, 0, 5, 1])
    assert (r.n_pos, r.n_neg, r.n_nan, r.u2) == ([2, 4], [3, 0], [1, 0], [9, 0])
    assert r.auroc[0] == 0.75 and math.isnan(r.auroc[1]) and r.average_precision == [0.75, 1.0]
    assert r.macro_auroc == 0.75 and r.macro_average_precision == 0.875 and r.n_defined == (1, 2)
    assert r.tp == [[1, 4]] and r.fp == [[1, 0]] and r.precision == [[0.5, 1.0]] and r.recall == [[0.5, 1.0]] and r.tpr is r.recall
    assert r.fpr[0][0] == 1 / 3 and math.isnan(r.fpr[0][1]) and r.f1 == [[0.5, 1.0]]
    assert r.micro_auroc == 0.75 and r.micro_average_precision == 0.75 and r.micro_tp == [5] and r.micro_fpr == [1 / 3]
    assert RankingResult([[0, 0, 5, 0, 0, 0]], []).micro_auroc is None


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if "k_rank_" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_rank_pack", "k_rank_column"):
        assert want in names, (want, names)
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 65536, k
        assert int(k["vgpr"]) + int(k["agpr"]) <= 128, k       # (k_rank_column: 16 waves a workgroup, four per SIMD)
