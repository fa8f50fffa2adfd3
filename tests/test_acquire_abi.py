"""CPU tests of the acquisition boundary: vbnn_top_rows_args as gcc lays it out from the header against the ctypes mirror, the
two symbols in the library / the ctypes table / the Lua cdef, the cap and the stream id, the ABI version unchanged (additive),
and the engine's signatures."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
PHILOX = os.path.join(ROOT, "include", "vbnn_philox.h")


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', f'#include "{PHILOX}"', "int main(void){",
             'printf("cap %d\\n", (int)VBNN_TOP_ROWS_MAX_K);', 'printf("stream %u\\n", (unsigned)VBNN_STREAM_ACQUIRE);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);', 'printf("vbnn_top_rows_args %zu\\n", sizeof(vbnn_top_rows_args));',
             "(void)vbnn_det_logf; (void)vbnn_normal4; (void)vbnn_box_muller;"]
    for fname, _ in L.TopRowsArgs._fields_:
        lines.append(f'printf("vbnn_top_rows_args.{fname} %zu\\n", offsetof(vbnn_top_rows_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-o", exe, src, "-lm"])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1] for l in out if l}


def test_args_match_the_header():
    from vbnn_amd import _lib as L
    st, got = L.TopRowsArgs, _probe()
    assert int(got["vbnn_top_rows_args"]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"vbnn_top_rows_args.{fname}"]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_top_rows_args \{(.*?)\}\s*vbnn_top_rows_args;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?=[,;])", body) == [f for f, _ in st._fields_]       # every field mirrored, in order


def test_cap_stream_id_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["cap"] == "4096" and L.TOP_ROWS_MAX_K == 4096
    assert got["stream"] == "6" and L.STREAM_ACQUIRE == 6
    ids = re.findall(r"^#define VBNN_STREAM_\w+\s+(\d+)u", open(PHILOX).read(), flags=re.M)
    assert sorted(ids) == ["1", "2", "3", "4", "5", "6"]            # beside the other stream ids, no id used twice
    assert got["abi"] == "6"                                          # additive: two symbols, one struct
    assert L.lib().vbnn_abi_version() == 6


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    lib = C.CDLL(L.LIB_PATH)
    for sym in ("vbnn_top_rows", "vbnn_top_rows_workspace_bytes"):
        assert sym in L.exported_symbols() and hasattr(lib, sym)
    args, res = L._SIGS["vbnn_top_rows"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.TopRowsArgs)
    assert re.search(r"int vbnn_top_rows\(vbnn_ctx\* ctx, const vbnn_top_rows_args\* a\);", cdef)
    assert re.search(r"int vbnn_top_rows_workspace_bytes\(int64_t R, int32_t k, size_t\* bytes\);", cdef)
    assert "typedef struct vbnn_top_rows_args {" in cdef
    # the size query needs no device: it refuses what the entry point refuses; a fixed part and one word per row (the stored keys)
    n, m = C.c_size_t(), C.c_size_t()
    assert L.lib().vbnn_top_rows_workspace_bytes(1, 1, C.byref(n)) == 0 and n.value > 4
    assert L.lib().vbnn_top_rows_workspace_bytes((1 << 31) - 1, 4096, C.byref(m)) == 0
    assert m.value - n.value == 4 * ((1 << 31) - 2)
    for R, k in ((0, 1), (1 << 31, 1), (5, 0), (5, 4097)):
        assert L.lib().vbnn_top_rows_workspace_bytes(R, k, C.byref(n)) != 0
        assert len(L.lib().vbnn_last_error()) > 0


def test_engine_surface():
    from vbnn_amd import acquisition, active
    from vbnn_amd.engine import AcquireResult, FusedMLP
    sig = inspect.signature(FusedMLP.top_rows)
    assert list(sig.parameters) == ["self", "score", "k", "largest", "exclude", "beta", "draw", "row0"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [True, None, None, None, 0]
    sig = inspect.signature(FusedMLP.acquire)
    assert list(sig.parameters) == ["self", "pool", "k", "score", "S", "map", "analytic", "exclude", "beta", "row0"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, False, False, None, None, None]
    r = AcquireResult(None, None, None, [3, 5, 1, 2])
    assert (r.n_selected, r.n_candidates, r.n_nan, r.n_excluded) == (3, 5, 1, 2)
    for f in ("indices", "values", "keys", "score_name", "S", "chunks", "predictive"):
        assert hasattr(r, f)
    assert acquisition.SCORES == {"nll": ("mutual_info", "entropy", "least_confidence", "margin", "random"),
                                  "bce": ("mutual_info", "entropy", "random"), "mse": ("variance", "random"),
                                  "gauss": ("variance", "total_variance", "random")}
    sig = inspect.signature(active.active_learning)
    assert list(sig.parameters)[:10] == ["opt", "x_pool", "y_pool", "x_test", "y_test", "n_init", "k", "rounds", "score", "beta"]
    assert "epochs" in sig.parameters
    # the existing predictives keep their signatures
    assert list(inspect.signature(FusedMLP.selective).parameters) == ["self", "score", "hit", "coverages"]
