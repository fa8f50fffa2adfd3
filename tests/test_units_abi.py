"""CPU tests of structured (unit-level) pruning's boundary: vbnn_unit_desc / vbnn_unit_gather_args as gcc lays them out from the
header against the ctypes mirrors, the vbnn_unit_* entry points in the library / the ctypes table / the Lua cdef, the ABI version
unchanged (additive), the three hosts' prune_units and compact issuing the same library calls in the same order, the engine's
surface, the shipped kernels free of scratch memory, and the NumPy restatement of the rule (tests/_units_np.py) against itself
on a hand-made network."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
SYMBOLS = {"vbnn_unit_snr": 3, "vbnn_unit_select": 5, "vbnn_unit_index": 6, "vbnn_unit_gather": 2}
sys.path.insert(0, ROOT)


def test_unit_structs_match_the_header():
    from tests.test_sparse_abi import _layout
    from vbnn_amd import _lib as L
    _layout("vbnn_unit_desc", L.UnitDesc)
    _layout("vbnn_unit_gather_args", L.UnitGatherArgs)


def test_unit_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]

    def protos(s):
        return {m.group(1): len([p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"])
                for m in re.finditer(r"(vbnn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", s, flags=re.S)}
    ph, pl = protos(hdr), protos(cdef)
    assert {n for n in ph if n.startswith("vbnn_unit_")} == set(SYMBOLS)                # every vbnn_unit_* symbol is covered here
    for name, n in SYMBOLS.items():
        assert name in L.exported_symbols() and hasattr(lib, name), name
        assert ph[name] == pl[name] == n == len(L._SIGS[name][0]), (name, ph.get(name), pl.get(name))
        assert L._SIGS[name][1] is C.c_int
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)                                # an int status, as every entry point
    assert "typedef struct vbnn_unit_desc {" in cdef and "typedef struct vbnn_unit_gather_args {" in cdef
    assert L.lib().vbnn_abi_version() == 6                                              # additive
    assert "#define VBNN_ABI_VERSION 6" in open(HEADER).read()
    assert "mainviz.lua:20" in open(HEADER).read().split("structured pruning")[1]       # the Lua lines the entries generalise


def test_the_three_hosts_issue_unit_calls_in_the_same_order():
    """FusedMLP.prune_units / compact, lua FusedMLP:prune_units / :compact and c_host's fm_prune_units / fm_compact: the same
    library calls in the same order, in no function (Python) or range (Lua, C) the predict, prune and sparse lints read."""
    from tests.test_predict_abi import READ_BACK, _c_fn, _lua, _ordered_calls, _section, _src
    from vbnn_amd.engine import FusedMLP
    raw, lua = _lua()
    c = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "tools", "c_host.c")).read(), flags=re.S)
    py_re, lua_re, c_re = r"lib\.(vbnn_[a-z0-9_]+)\(", r"\bC\.(vbnn_[a-z0-9_]+)\s*\(", r"\b(vbnn_[a-z0-9_]+)\s*\("
    py = _ordered_calls(_src("prune_units"), py_re, {})
    lu = _ordered_calls(_section(lua, "function FusedMLP:prune_units(", "function FusedMLP:compact("), lua_re, {}, drop=READ_BACK)
    cc = _ordered_calls(_c_fn(c, "fm_prune_units"), c_re, {}, drop=READ_BACK)
    assert py == lu == cc == ["vbnn_unit_snr", "vbnn_unit_select", "vbnn_unit_index"], (py, lu, cc)
    py = _ordered_calls(_src("compact"), py_re, {})
    lu = _ordered_calls(_section(lua, "function FusedMLP:compact(", "function FusedMLP:prune("), lua_re, {}, drop=READ_BACK)
    cc = _ordered_calls(_c_fn(c, "fm_compact"), c_re, {}, drop=READ_BACK)
    assert py == lu == cc == ["vbnn_unit_gather", "vbnn_sample"], (py, lu, cc)   # (the counter: device_draw engines only)
    # each host builds the compact network's engine first and prepares it after the gather
    sec = _src("compact")
    assert sec.index("FusedMLP(opt") < sec.index("vbnn_unit_gather") < sec.index("new.prepare()")
    sec = _section(lua, "function FusedMLP:compact(", "function FusedMLP:prune(")
    assert sec.index("FusedMLP.new(") < sec.index("vbnn_unit_gather") < sec.index(":prepare()")
    sec = _c_fn(c, "fm_compact")
    assert sec.index("fm_new(") < sec.index("vbnn_unit_gather") < sec.index("fm_prepare(")
    # placement: the unit functions exist; the weight-pruning, sparse and predict functions make no unit call
    for fn in ("unit_snr", "prune_units", "compact", "prune_units_curve"):
        assert callable(getattr(FusedMLP, fn)), fn
    for fn in ("_prune_descs", "snr", "prune", "_prune_mask", "use_pruned", "pruned", "prune_curve", "prune_curve_sparse", "_compress",
               "_sparse_buffers", "_predict_forward_sparse", "predict", "_predictive_plan", "_predictive_inputs", "_chunks",
               "_draw_forward", "_consume_draws", "_predict_wn_sample", "_predict_forward"):
        assert "vbnn_unit_" not in _src(fn), fn
    assert raw.index("function FusedMLP:loss_and_accuracy") < raw.index("function FusedMLP:prune_units(") < \
        raw.index("function FusedMLP:compact(") < raw.index("function FusedMLP:prune(")
    assert "vbnn_unit_" not in raw[raw.index("function FusedMLP:prune("):]
    for fn in ("fm_predict", "fm_predict_forward", "fm_prune", "fm_compress"):
        assert "vbnn_unit_" not in _c_fn(c, fn)
    # the module-level key
    vbl = open(os.path.join(ROOT, "lua", "VBLinear.lua")).read()
    assert re.search(r"function VBLinear:unit_snr\(\)", vbl) and "C.vbnn_unit_snr(" in vbl
    from vbnn_amd import nn
    assert callable(nn.VBLinear.unit_snr)
    # every field the Lua file sets exists
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = {m.group(2): set(re.findall(r"(\w+)\s*(?=[,;])", m.group(1)))
               for m in re.finditer(r"typedef struct \w+ \{(.*?)\}\s*(vbnn_\w+);", hdr, flags=re.S)}
    chunk = raw[raw.index("function FusedMLP:prune_units("):raw.index("function FusedMLP:prune(")]
    assert re.search(r"local ga = ffi\.new\('vbnn_unit_gather_args'\)", chunk)
    checked = 0
    for m in re.finditer(r"(?<![\w.])ga\.(\w+)", chunk):
        assert m.group(1) in structs["vbnn_unit_gather_args"], m.group(1)
        checked += 1
    for m in re.finditer(r"(?<![\w.])e\.(\w+)", chunk):
        assert m.group(1) in structs["vbnn_unit_desc"], m.group(1)
        checked += 1
    assert checked >= 15, checked


def test_unit_surface():
    from vbnn_amd.engine import FusedMLP, UnitPruneResult
    assert list(inspect.signature(FusedMLP.unit_snr).parameters) == ["self", "li"]
    sig = inspect.signature(FusedMLP.prune_units)
    assert list(sig.parameters) == ["self", "fraction", "threshold", "scope", "multiple"]
    assert [sig.parameters[n].default for n in ("fraction", "threshold", "scope", "multiple")] == [None, None, "global", 1]
    sig = inspect.signature(FusedMLP.compact)
    assert list(sig.parameters) == ["self", "result", "opt_overrides"]
    assert sig.parameters["opt_overrides"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(FusedMLP.prune_units_curve)
    assert list(sig.parameters) == ["self", "inputs", "targets", "fractions", "S", "map", "scope", "multiple"]
    assert [sig.parameters[n].default for n in ("S", "map", "scope", "multiple")] == [None, False, "global", 1]
    import torch
    keep = [torch.tensor([0, 2, 3], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)]
    r = UnitPruneResult("eng", "global", 1, [0.5, 0.5], keep, [5, 6, 4], 10, 7)
    assert (r.engine, r.scope, r.multiple, r.tau, r.version) == ("eng", "global", 1, [0.5, 0.5], 7)
    assert r.keep[0] is keep[0] and r.hidden == [3, 1]
    assert r.layers == [dict(n_units=6, n_pruned=3, fraction_pruned=0.5), dict(n_units=4, n_pruned=3, fraction_pruned=0.75)]
    assert (r.n_units, r.n_pruned, r.fraction_pruned) == (10, 6, 0.6)
    assert r.n_weights_before == 5 * 6 + 6 * 4 + 4 * 10 and r.n_weights == 5 * 3 + 3 * 1 + 1 * 10


def test_unit_kernels_use_no_scratch():
    """The shipped code object's k_unit_* kernels: no scratch memory, no spills, LDS within 8 KiB (tools/kernel_regs.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels() if "k_unit_" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("k_unit_snr", "k_unit_select", "k_unit_index", "k_unit_gather"):
        assert want in names, (want, names)
    assert len([k for k in ks if "k_unit_snr" in k["name"]]) == 2                       # a wave per row / a workgroup per row
    assert len([k for k in ks if "k_unit_gather" in k["name"]]) == 2                    # a VB layer / the final Linear
    for k in ks:
        assert int(k["scratch"]) == 0 and int(k["spill"]) == 0, k
        assert int(k["lds"]) <= 8192, k


def test_unit_helper_on_a_hand_made_network():
    """tests/_units_np.py on a 6 x 5 / 4 x 6 network: equal keys across the tau boundary, a NaN key, a layer where everything is
    below tau (it keeps exactly its best unit, the lower index of a tie), `multiple` rounding up past O (clamped to O)."""
    from tests import _units_np as U
    a0 = np.array([3.0, 1.0, 2.0, np.nan, 2.0, 0.5])
    a1 = np.array([0.1, 0.3, 0.3, 0.2])
    means0, means1 = np.zeros((6, 5)), np.zeros((4, 6))
    means0[:, 1], means1[:, 4] = a0, -a1                              # one non-zero weight per unit: key = |a| / sqrt(I)
    means0[0, :] = 3.0 / np.sqrt(5.0)                                 # ... or the norm spread over the row: the same key
    lvars0, lvars1 = np.zeros((6, 5)), np.zeros((4, 6))
    k0, k1 = U.unit_key64(means0, lvars0), U.unit_key64(means1, lvars1)
    assert np.allclose(k0[[0, 1, 2, 4, 5]], a0[[0, 1, 2, 4, 5]] / np.sqrt(5.0), rtol=1e-15) and np.isnan(k0[3])
    assert np.allclose(k1, a1 / np.sqrt(6.0), rtol=1e-15)
    assert np.isnan(U.unit_key64(np.zeros((1, 3)), np.full((1, 3), -np.inf))[0])        # 0 / 0
    assert U.unit_key64(np.array([[-0.5]]), np.array([[np.log(4.0)]]))[0] == 0.25       # I = 1: mainviz.lua:20's |mu| / sigma
    keys = [k0.astype(np.float32), k1.astype(np.float32)]
    pool = np.concatenate(keys)
    # the order statistic: every layer-1 key is below every layer-0 key; NaN is the largest
    assert [U.kth(pool, k) for k in range(4)] == sorted(keys[1].tolist())
    assert U.kth(pool, 6) == U.kth(pool, 7) == keys[0][2] and np.isnan(U.kth(pool, 9)) and U.kth(pool, 8) == keys[0][0]
    # k = 7: tau = the tied key 2 / sqrt(5); `key < tau` prunes six units, not seven; the ties at tau stay
    tau, keep = U.prune_units(keys, fraction=0.7)
    assert tau[0] == tau[1] == keys[0][2]
    assert keep[0].tolist() == [0, 2, 3, 4]                                             # the NaN unit is kept
    assert keep[1].tolist() == [1]                                                      # all below tau: the best, lower index of the tie
    with np.errstate(invalid="ignore"):
        assert int((pool < tau[0]).sum()) == 6                                          # at most k = 7 below tau ...
    assert sum(k.size - kp.size for k, kp in zip(keys, keep)) == 5                      # ... and layer 1 takes its best unit back
    # multiple: the best of the pruned units come back, lower index first on ties; clamped at O
    assert U.kept(keys[0], tau[0], 5).tolist() == [0, 1, 2, 3, 4]
    assert U.kept(keys[0], tau[0], 4).tolist() == [0, 2, 3, 4]
    assert U.kept(keys[1], tau[1], 2).tolist() == [1, 2] and U.kept(keys[1], tau[1], 3).tolist() == [1, 2, 3]
    tau5, keep5 = U.prune_units(keys, fraction=0.5, multiple=4)                         # n0 = 5 -> 8 > O = 6: every unit
    assert tau5[0] == keys[0][1] and keep5[0].tolist() == [0, 1, 2, 3, 4, 5] and keep5[1].tolist() == [0, 1, 2, 3]
    # inside a tie: tau above both tied units, room for one of them
    assert U.kept(keys[0], np.float32(1.0), 1).tolist() == [0, 3] and U.kept(keys[0], np.float32(1.0), 3).tolist() == [0, 2, 3]
    # the ends: tau = +inf keeps the NaN unit (never pruned) / the best unit; fraction 0 keeps everything; scope = layer
    tinf, kinf = U.prune_units(keys, fraction=1.0)
    assert np.isinf(tinf[0]) and kinf[0].tolist() == [3] and kinf[1].tolist() == [1]
    assert [k.tolist() for k in U.prune_units(keys, fraction=0.0)[1]] == [list(range(6)), list(range(4))]
    tl, kl = U.prune_units(keys, fraction=0.5, scope="layer")
    assert tl[0] == keys[0][2] and tl[1] == keys[1][1] and kl[0].tolist() == [0, 2, 3, 4] and kl[1].tolist() == [1, 2]
    tt, kt = U.prune_units(keys, threshold=0.1)
    assert kt[0].tolist() == list(range(6)) and kt[1].tolist() == [1, 2]
    # compaction by fancy indexing
    rng = np.random.default_rng(5)
    P = [(rng.normal(size=(6, 5)), rng.normal(size=(6, 5)), rng.normal(size=6)), (rng.normal(size=(4, 6)), rng.normal(size=(4, 6)), rng.normal(size=4))]
    w3 = rng.normal(size=(3, 4))
    out, w3c = U.compact(P, w3, keep)
    assert out[0][0].shape == (4, 5) and out[1][0].shape == (1, 4) and w3c.shape == (3, 1)
    assert np.array_equal(out[0][1], P[0][1][[0, 2, 3, 4]]) and np.array_equal(out[0][2], P[0][2][[0, 2, 3, 4]])
    assert np.array_equal(out[1][0], P[1][0][[1]][:, [0, 2, 3, 4]]) and np.array_equal(out[1][2], P[1][2][[1]])
    assert np.array_equal(w3c, w3[:, [1]])
    assert U.n_weights([5, 4, 1], 3) == 5 * 4 + 4 * 1 + 1 * 3
    # the function of the compact network is the big one's with the dropped units' activations forced to zero
    x = rng.normal(size=(7, 5))
    h = x
    for (m, _, b), kp in zip(P, keep):
        y = np.maximum(h @ m.T + b, 0.0)
        dead = ~np.isin(np.arange(m.shape[0]), kp)
        y[:, dead] = 0.0
        h = y
    want = h @ w3.T
    h = x
    for m, _, b in out:
        h = np.maximum(h @ m.T + b, 0.0)
    assert np.allclose(h @ w3c.T, want, rtol=1e-13, atol=1e-13)
