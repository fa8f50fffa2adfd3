"""CPU tests of the compressed pruned form's boundary: vbnn_sparse_desc / vbnn_sparse_fwd_args as gcc lays them out from the
header against the ctypes mirrors, the two entry points in the library / the ctypes table / the Lua cdef, the ABI version
unchanged (additive), the three hosts' compress and sparse predict forward issuing the same library calls in the same order,
the engine's surface, the shipped kernels free of scratch memory, and the NumPy restatement of the format (tests/_sparse_np.py)
against itself on a hand-made layer."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
SYMBOLS = {"vbnn_prune_compress": 7, "vbnn_forward_sparse": 3}
sys.path.insert(0, ROOT)


def _layout(cname, st):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
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
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (cname, cname), hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?=[,;])", body) == [f for f, _ in st._fields_]        # every C field is mirrored


def test_sparse_structs_match_the_header():
    from vbnn_amd import _lib as L
    _layout("vbnn_sparse_desc", L.SparseDesc)
    _layout("vbnn_sparse_fwd_args", L.SparseFwdArgs)


def test_sparse_entry_points_are_exported_and_declared_everywhere():
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
        assert L._SIGS[name][1] is C.c_int
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)                                # an int status, as every entry point
    assert "typedef struct vbnn_sparse_desc {" in cdef and "typedef struct vbnn_sparse_fwd_args {" in cdef
    assert L.lib().vbnn_abi_version() == 6                                              # additive
    assert "#define VBNN_ABI_VERSION 6" in open(HEADER).read()


def test_the_three_hosts_issue_sparse_calls_in_the_same_order():
    """FusedMLP._compress / _predict_forward_sparse, lua FusedMLP:compress / :_predict_forward_sparse and c_host's fm_compress /
    fm_predict_forward_sparse: the same library calls in the same order, in no function (Python) or range (Lua, C) the predict and
    prune lints read, reached from each host's _predict_forward by an early return."""
    from tests.test_predict_abi import READ_BACK, _c_fn, _lua, _ordered_calls, _section, _src
    raw, lua = _lua()
    c = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "tools", "c_host.c")).read(), flags=re.S)
    py_re, lua_re, c_re = r"lib\.(vbnn_[a-z0-9_]+)\(", r"\bC\.(vbnn_[a-z0-9_]+)\s*\(", r"\b(vbnn_[a-z0-9_]+)\s*\("
    # compress
    py = _ordered_calls(_src("_compress"), py_re, {})
    lu = _ordered_calls(_section(lua, "function FusedMLP:compress(", "function FusedMLP:_predict_forward_sparse("), lua_re, {}, drop=READ_BACK)
    cc = _ordered_calls(_c_fn(c, "fm_compress"), c_re, {}, drop=READ_BACK)
    assert py == lu == cc == ["vbnn_prune_compress"], (py, lu, cc)
    # the forward
    py = _ordered_calls(_src("_predict_forward_sparse"), py_re, {})
    lu = _ordered_calls(_section(lua, "function FusedMLP:_predict_forward_sparse(", "function FusedMLP:predict("), lua_re, {})
    cc = _ordered_calls(_c_fn(c, "fm_predict_forward_sparse"), c_re, {})
    assert py == lu == cc == ["vbnn_pack_input", "vbnn_forward_sparse"], (py, lu, cc)
    # placement: the dense functions make no sparse call
    for fn in ("predict", "_predictive_plan", "_predictive_inputs", "_chunks", "_draw_forward", "_consume_draws", "_predict_forward", "prune"):
        assert "vbnn_prune_compress" not in _src(fn) and "vbnn_forward_sparse" not in _src(fn), fn
    assert "self._predict_forward_sparse(" in _src("_predict_forward")
    assert raw.index("function FusedMLP:use_pruned(") < raw.index("function FusedMLP:compress(") < \
        raw.index("function FusedMLP:_predict_forward_sparse(") < raw.index("function FusedMLP:predict(")
    tail = raw[raw.index("function FusedMLP:predict("):]
    assert "vbnn_prune_compress" not in tail and "vbnn_forward_sparse" not in tail and "self:_predict_forward_sparse(" in tail
    for fn in ("fm_predict", "fm_predict_forward", "fm_prune"):
        body = _c_fn(c, fn)
        assert "vbnn_prune_compress" not in body and "vbnn_forward_sparse" not in body
    assert "fm_predict_forward_sparse(" in _c_fn(c, "fm_predict_forward")
    # every field the Lua file sets exists
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = {m.group(2): set(re.findall(r"(\w+)\s*(?=[,;])", m.group(1)))
               for m in re.finditer(r"typedef struct \w+ \{(.*?)\}\s*(vbnn_\w+);", hdr, flags=re.S)}
    chunk = raw[raw.index("function FusedMLP:compress("):raw.index("function FusedMLP:predict(")]
    assert re.search(r"local sa = ffi\.new\('vbnn_sparse_fwd_args'\)", chunk)
    checked = 0
    for m in re.finditer(r"(?<![\w.])sa\.(\w+)", chunk):
        assert m.group(1) in structs["vbnn_sparse_fwd_args"], m.group(1)
        checked += 1
    for m in re.finditer(r"(?<![\w.])sd\[0\]\.(\w+)", chunk):
        assert m.group(1) in structs["vbnn_sparse_desc"], m.group(1)
        checked += 1
    assert checked >= 25, checked


def test_sparse_surface():
    from vbnn_amd.engine import FusedMLP, PruneResult, SparsePruneResult
    assert issubclass(SparsePruneResult, PruneResult)
    assert list(inspect.signature(PruneResult.compress).parameters) == ["self"]
    assert list(inspect.signature(SparsePruneResult.to_dense).parameters) == ["self", "li"]
    sig = inspect.signature(FusedMLP.prune_curve_sparse)
    assert list(sig.parameters) == ["self", "inputs", "targets", "fractions", "S", "map", "scope"]
    assert (sig.parameters["S"].default, sig.parameters["map"].default, sig.parameters["scope"].default) == (None, False, "global")
    base = PruneResult("eng", "layer", [0.5, 0.25], [(1.0, 0.5, 8.0, 4.0), (0.0, 0.0, 6.0, 6.0)], ["m0", "m1"], ["v0", "v1"], 7)
    import torch
    rp = [torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)]
    cols = [torch.zeros(3, dtype=torch.int16), torch.zeros(6, dtype=torch.int16)]
    vals = [torch.zeros(3, dtype=torch.bfloat16), torch.zeros(6, dtype=torch.bfloat16)]
    s = SparsePruneResult(base, rp, cols, vals, [v.clone() for v in vals], [3, 6], [2, 2], 1024)
    assert (s.engine, s.scope, s.tau, s.version) == ("eng", "layer", [0.5, 0.25], 7)
    assert (s.n_pruned, s.W, s.fraction_pruned) == (1, 10, 0.1) and s.layers[0] == base.layers[0] and s.stats == base.stats
    assert s.nnz == [3, 6] and s.idx_bytes == [2, 2] and s.mu_p is None and s.var_p is None
    assert s.nbytes == 4 * (3 + 4) + 2 * (3 + 6) + 2 * 2 * (3 + 6) and s.dense_nbytes == 1024
    assert s.row_ptr is rp and s.cols is cols and s.mu_v is vals and callable(s.mask) and s.compress() is s


def test_sparse_kernels_use_no_scratch():
    """The shipped code object's compress and forward kernels: no scratch memory, no spills (tools/kernel_regs.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if "k_sparse_" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_sparse_count", "k_sparse_scan", "k_sparse_fill", "k_sparse_fwd"):
        assert want in names, (want, names)
    assert len([k for k in ks if "k_sparse_fill" in k["name"]]) == 4                     # f32 / bf16 x uint16 / uint32
    assert len([k for k in ks if "k_sparse_fwd" in k["name"]]) == 6                      # f32 / bf16 x MAP / LRT / LRT with x2T
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 2048, k


def test_csr_helper_round_trip():
    """tests/_sparse_np.py on a hand-made 5 x 7 layer: empty rows, a NaN key, ties at tau, a kept weight that is zero."""
    from tests import _sparse_np as S
    O, I, tau = 5, 7, np.float32(0.5)
    keys = np.full((O, I), 0.25, np.float32)                        # all pruned ...
    keys[1, [0, 3, 6]] = [0.5, 0.75, 0.5]                           # ... but: ties at tau are kept (strict <)
    keys[3, 2] = np.nan                                             # a NaN key is kept
    keys[3, 5] = 2.0
    keys[4, :] = 1.0                                                # a full row
    mu = (np.arange(O * I, dtype=np.float64).reshape(O, I) - 17.0)  # mu[2, 3] = 0, pruned; mu[4, ...] non-zero
    mu[4, 1] = 0.0                                                  # a KEPT weight that is zero: still an entry
    var = 2.0 ** -(np.arange(O * I).reshape(O, I) % 5).astype(np.float64)
    csr = S.csr_build(keys, tau, mu, var)
    S.csr_check(csr, O, I)
    assert csr["row_ptr"].tolist() == [0, 0, 3, 3, 5, 12] and csr["nnz"] == 12 == O * I - int((keys < tau).sum())
    assert csr["cols"].tolist() == [0, 3, 6, 2, 5, 0, 1, 2, 3, 4, 5, 6]
    kept = ~(keys < tau)
    assert np.array_equal(S.csr_to_dense(csr, O, I), np.where(kept, mu, 0.0))
    assert np.array_equal(S.csr_to_dense(csr, O, I, ld=64, which="var_v")[:, :I], np.where(kept, var, 0.0))
    assert not S.csr_to_dense(csr, O, I, ld=64)[:, I:].any()
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, (6, I)).astype(np.float64)
    z = rng.normal(size=(6, O))
    b = rng.normal(size=O)
    y, h, absprod = S.forward64(csr, O, x, None, b, z)
    mu_d, var_d = np.where(kept, mu, 0.0), np.where(kept, var, 0.0)
    v = (x * x) @ var_d.T
    want = x @ mu_d.T + b + np.sqrt(v) * z
    assert np.allclose(y, want, rtol=1e-14, atol=1e-12) and np.array_equal(h, np.maximum(y, 0.0))
    assert np.array_equal(y[:, [0, 2]], np.broadcast_to(b[[0, 2]], (6, 2)))            # rows without entries: the bias alone
    assert np.allclose(absprod, np.abs(x) @ np.abs(mu_d).T + np.abs(b) + np.sqrt(v) * np.abs(z))
    ym, _, _ = S.forward64(csr, O, x, None, b, None)
    assert np.allclose(ym, x @ mu_d.T + b, rtol=1e-14, atol=1e-12)
    # everything pruned, nothing pruned
    e = S.csr_build(keys, np.float32(np.inf), mu, var)
    assert e["nnz"] == 1 and e["cols"].tolist() == [2]              # only the NaN key survives tau = +inf
    f = S.csr_build(keys, np.float32(0.0), mu, var)
    assert f["nnz"] == O * I and np.array_equal(S.csr_to_dense(f, O, I), mu)
