"""CPU tests of the pruning entry points' boundary (mainviz.lua:20-27 on the device): vbnn_prune_desc as gcc lays it out from
the header against the ctypes mirror, the four symbols in the library / the ctypes table / the Lua cdef, the ABI version
unchanged (additive), the three hosts' prune issuing the same library calls in the same order, the engine's surface, and the
shipped sweep kernels free of scratch memory."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
SYMBOLS = {"vbnn_snr": 5, "vbnn_prune_workspace_bytes": 3, "vbnn_prune_select": 7, "vbnn_prune_pack": 6}


def test_prune_desc_matches_the_header():
    from vbnn_amd import _lib as L
    st = L.PruneDesc
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_prune_desc));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_prune_desc, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {l.split()[0]: l.split()[1:] for l in out if l}
    assert int(got["size"][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_prune_desc \{(.*?)\}\s*vbnn_prune_desc;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?=[,;])", body) == [f for f, _ in st._fields_]        # every C field is mirrored


def test_prune_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]

    def protos(s):
        return {m.group(1): len([p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"])
                for m in re.finditer(r"(vbnn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", s, flags=re.S)}
    ph, pl = protos(hdr), protos(cdef)
    for name, n in SYMBOLS.items():
        assert name in L.exported_symbols() and hasattr(lib, name), name
        assert ph[name] == pl[name] == n == len(L._SIGS[name][0]), (name, ph.get(name), pl.get(name))
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)                                # an int status, as every entry point
    assert "typedef struct vbnn_prune_desc {" in cdef
    assert L.lib().vbnn_abi_version() == 6                                              # additive
    assert "#define VBNN_ABI_VERSION 6" in open(HEADER).read()


def test_the_three_hosts_issue_prune_calls_in_the_same_order():
    """FusedMLP.prune, lua FusedMLP:prune and c_host's fm_prune: the same library calls in the same order, so what the GPU test
    proves of the C program holds for the Lua file."""
    sys.path.insert(0, ROOT)
    from tests.test_predict_abi import READ_BACK, _c_fn, _lua, _ordered_calls, _section, _src
    py = _ordered_calls(_src("prune"), r"lib\.(vbnn_[a-z0-9_]+)\(", {})
    raw, lua = _lua()
    lu = _ordered_calls(_section(lua, "function FusedMLP:prune(", "function FusedMLP:use_pruned("), r"\bC\.(vbnn_[a-z0-9_]+)\s*\(",
                        {}, drop=READ_BACK)
    c = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "tools", "c_host.c")).read(), flags=re.S)
    cc = _ordered_calls(_c_fn(c, "fm_prune"), r"\b(vbnn_[a-z0-9_]+)\s*\(", {}, drop=READ_BACK)
    assert py == lu == cc == ["vbnn_prune_workspace_bytes", "vbnn_prune_select", "vbnn_prune_pack"], (py, lu, cc)
    # placement: outside the ranges the predict lints slice, and outside run .. finish; the predict functions do not prune
    assert raw.index("function FusedMLP:loss_and_accuracy") < raw.index("function FusedMLP:prune(") < \
        raw.index("function FusedMLP:use_pruned(") < raw.index("function FusedMLP:predict(")
    for fn in ("predict", "_predictive_plan", "_predictive_inputs", "_chunks", "_draw_forward", "_consume_draws", "_predict_forward"):
        assert "vbnn_prune" not in _src(fn) and "vbnn_snr" not in _src(fn), fn
    for fn in ("fm_predict", "fm_predict_forward"):
        assert "vbnn_prune" not in _c_fn(c, fn)
    assert "vbnn_prune" not in raw[raw.index("function FusedMLP:predict("):]
    # the module-level key
    assert re.search(r"function VBLinear:snr\(\)", open(os.path.join(ROOT, "lua", "VBLinear.lua")).read())
    from vbnn_amd import nn
    assert callable(nn.VBLinear.snr)


def test_prune_surface():
    from vbnn_amd.engine import FusedMLP, PruneResult
    assert list(inspect.signature(FusedMLP.predict).parameters) == ["self", "inputs", "S", "targets", "map", "row0"]
    sig = inspect.signature(FusedMLP.prune)
    assert list(sig.parameters) == ["self", "fraction", "threshold", "scope"]
    assert (sig.parameters["fraction"].default, sig.parameters["threshold"].default, sig.parameters["scope"].default) == \
        (None, None, "global")
    assert list(inspect.signature(FusedMLP.use_pruned).parameters) == ["self", "result"]
    assert list(inspect.signature(FusedMLP.pruned).parameters) == ["self", "result"]
    sig = inspect.signature(FusedMLP.prune_curve)
    assert list(sig.parameters) == ["self", "inputs", "targets", "fractions", "S", "map", "scope", "compress"]
    assert [sig.parameters[n].default for n in ("S", "map", "scope", "compress")] == [None, False, "global", False]
    r = PruneResult(None, "layer", [0.5, 0.25], [(1.0, 0.5, 8.0, 4.0), (0.0, 0.0, 6.0, 6.0)], ["m0", "m1"], ["v0", "v1"], 7)
    assert r.tau == [0.5, 0.25] and r.scope == "layer" and r.version == 7 and r.mu_p == ["m0", "m1"]
    assert (r.n_pruned, r.W, r.fraction_pruned, r.mean_var, r.mean_pruned_var) == (1, 10, 0.1, 1.4, 0.5)
    assert r.layers[0] == dict(n_pruned=1, W=4, fraction_pruned=0.25, mean_var=2.0, mean_pruned_var=0.5)
    assert r.layers[1]["n_pruned"] == 0 and r.layers[1]["mean_pruned_var"] != r.layers[1]["mean_pruned_var"]     # nan: nothing pruned
    assert callable(r.mask)


def test_prune_kernels_use_no_scratch():
    """The shipped code object's sweep kernels: no scratch memory, no spills (tools/kernel_regs.py reads the metadata)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if re.search(r"k_snr|k_prune_(hist|pick|pack|finish)", k["name"])]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_snr", "k_prune_hist", "k_prune_pick", "k_prune_pack", "k_prune_finish"):
        assert want in names, (want, names)
    assert len([k for k in ks if "k_prune_pack" in k["name"]]) == 2                      # f32 and bf16
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 2048 * 4, k                                              # nothing beyond the histogram
