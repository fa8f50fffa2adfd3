"""CPU tests of the k-centre boundary: vbnn_kcentre_args as gcc lays it out from the header against the ctypes mirror, the two
symbols in the library / the ctypes table / the Lua cdef, the caps, the ABI version unchanged (additive), the size query's
refusals without a device, and the engine's signatures -- the new ones, and the old ones unmoved."""
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
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("cap_k %d\\n", (int)VBNN_KCENTRE_MAX_K);', 'printf("cap_d %d\\n", (int)VBNN_KCENTRE_MAX_D);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);', 'printf("vbnn_kcentre_args %zu\\n", sizeof(vbnn_kcentre_args));']
    for fname, _ in L.KcentreArgs._fields_:
        lines.append(f'printf("vbnn_kcentre_args.{fname} %zu\\n", offsetof(vbnn_kcentre_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1] for l in out if l}


def test_args_match_the_header():
    from vbnn_amd import _lib as L
    st, got = L.KcentreArgs, _probe()
    assert int(got["vbnn_kcentre_args"]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"vbnn_kcentre_args.{fname}"]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_kcentre_args \{(.*?)\}\s*vbnn_kcentre_args;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?=[,;])", body) == [f for f, _ in st._fields_]       # every field mirrored, in order


def test_caps_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["cap_k"] == "4096" and L.KCENTRE_MAX_K == 4096
    assert int(got["cap_d"]) == L.KCENTRE_MAX_D >= 4096               # at least the headline network's hidden width
    assert got["abi"] == "6" and L.lib().vbnn_abi_version() == 6      # additive: two symbols, one struct
    ids = re.findall(r"^#define VBNN_STREAM_\w+\s+(\d+)u", open(PHILOX).read(), flags=re.M)
    assert sorted(ids) == ["1", "2", "3", "4", "5", "6"]              # a deterministic selection: no Philox stream added


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    lib = C.CDLL(L.LIB_PATH)
    for sym in ("vbnn_kcentre", "vbnn_kcentre_workspace_bytes"):
        assert sym in L.exported_symbols() and hasattr(lib, sym)
    args, res = L._SIGS["vbnn_kcentre"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.KcentreArgs)
    assert re.search(r"int vbnn_kcentre\(vbnn_ctx\* ctx, const vbnn_kcentre_args\* a\);", cdef)
    assert re.search(r"int vbnn_kcentre_workspace_bytes\(int64_t R, int64_t D, int32_t k, size_t\* bytes\);", cdef)
    assert "typedef struct vbnn_kcentre_args {" in cdef


def test_the_size_query_refuses_what_the_entry_point_refuses():
    from vbnn_amd import _lib as L
    lib = L.lib()
    n, m = C.c_size_t(), C.c_size_t()
    assert lib.vbnn_kcentre_workspace_bytes(1, 1, 1, C.byref(n)) == 0 and n.value > 8 * 4097
    assert lib.vbnn_kcentre_workspace_bytes((1 << 31) - 1, L.KCENTRE_MAX_D, 4096, C.byref(m)) == 0
    assert m.value - n.value == (1 << 31) - 2                         # a fixed part and one byte per row
    for R, D, k in ((0, 4, 1), (1 << 31, 4, 1), (5, 0, 1), (5, L.KCENTRE_MAX_D + 1, 1), (5, 4, 0), (5, 4, 4097), (-1, 4, 1)):
        n.value = 12345
        assert lib.vbnn_kcentre_workspace_bytes(R, D, k, C.byref(n)) != 0 and n.value == 12345
        assert len(lib.vbnn_last_error()) > 0
    assert lib.vbnn_kcentre_workspace_bytes(5, 4, 1, None) != 0


def test_engine_surface():
    from vbnn_amd import active
    from vbnn_amd.engine import AcquireResult, FusedMLP, SpreadResult            # noqa: F401 (exported beside AcquireResult)
    sig = inspect.signature(FusedMLP.features)
    assert list(sig.parameters) == ["self", "inputs", "layer"] and sig.parameters["layer"].default == -1
    sig = inspect.signature(FusedMLP.spread_rows)
    assert list(sig.parameters) == ["self", "features", "k", "weight", "exclude", "centres", "state"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, None, None]
    sig = inspect.signature(FusedMLP.acquire_diverse)
    assert list(sig.parameters) == ["self", "pool", "k", "score", "S", "map", "analytic", "exclude", "weighted", "cover_labelled",
                                    "features", "row0"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, False, False, None, True, True, None, None]
    r = SpreadResult(None, None, None, None, [3, 5, 1, 2], 4)
    assert (r.n_selected, r.n_candidates, r.n_void, r.n_excluded, r.n_ignored_centres) == (3, 5, 1, 2, 4)
    for f in ("indices", "keys", "dists", "min_dist", "score_name", "S", "chunks", "predictive"):
        assert hasattr(r, f)
    sig = inspect.signature(active.active_learning)
    assert list(sig.parameters)[:10] == ["opt", "x_pool", "y_pool", "x_test", "y_test", "n_init", "k", "rounds", "score", "beta"]
    assert list(sig.parameters)[-1] == "diverse" and sig.parameters["diverse"].default is False      # appended
    assert list(sig.parameters)[10:12] == ["epochs", "device"]
    # acquire / top_rows: unchanged
    sig = inspect.signature(FusedMLP.top_rows)
    assert list(sig.parameters) == ["self", "score", "k", "largest", "exclude", "beta", "draw", "row0"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [True, None, None, None, 0]
    sig = inspect.signature(FusedMLP.acquire)
    assert list(sig.parameters) == ["self", "pool", "k", "score", "S", "map", "analytic", "exclude", "beta", "row0"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, False, False, None, None, None]
