"""CPU tests of the posterior-predictive entry point's boundary: vbnn_predict_args as gcc lays it out from the header against
the ctypes mirror, the symbol in the library / the ctypes table / the Lua cdef, and the ABI version unchanged (additive)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")


def test_predict_args_match_the_header():
    from vbnn_amd import _lib as L
    st = L.PredictArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vbnn_predict_args));',
             'printf("stacked %d accumulate %d\\n", (int)VBNN_PREDICT_STACKED, (int)VBNN_PREDICT_ACCUMULATE);']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(vbnn_predict_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {l.split()[0]: l.split()[1:] for l in out if l}
    assert int(got["size"][0]) == C.sizeof(st)
    assert got["stacked"] == [str(L.PREDICT_STACKED), "accumulate", str(L.PREDICT_ACCUMULATE)]
    for fname, _ in st._fields_:
        assert int(got[fname][0]) == getattr(st, fname).offset, fname
    # every field of the C struct is mirrored
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbnn_predict_args \{(.*?)\}\s*vbnn_predict_args;", hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]


def test_predict_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    assert "vbnn_head_predict" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "vbnn_head_predict")
    assert L.lib().vbnn_abi_version() == 6                      # additive: one symbol, one struct
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert re.search(r"int vbnn_head_predict\(vbnn_ctx\* ctx, int dtype, const vbnn_predict_args\* a\);", cdef)
    assert "typedef struct vbnn_predict_args {" in cdef


def test_predict_surface():
    """The engine's entry point and its result type exist with the documented signature."""
    import inspect
    from vbnn_amd.engine import FusedMLP, PredictResult
    sig = inspect.signature(FusedMLP.predict)
    assert list(sig.parameters) == ["self", "inputs", "S", "targets", "map", "row0"]
    r = PredictResult(*range(6))
    assert (r.probs, r.log_probs, r.entropy, r.expected_entropy, r.mutual_info, r.pred) == tuple(range(6))
    assert r.nll is None and r.mean_draw_accuracy is None


# ---- the three hosts' predict: lua/FusedMLP.lua (no interpreter here: linted), tools/c_host.c (run by the GPU tests), FusedMLP
HOST_ONLY_WN = ("vbnn_wn_sample", "vbnn_pack")        # the engine's weight-noise draws: the Lua and C hosts are LRT hosts
READ_BACK = ("vbnn_buf_download",)                    # the totals' read-back, which the engine does through torch (.cpu())


def _section(txt, start, end):
    i = txt.index(start)
    return txt[i:txt.index(end, i + len(start))]


def _src(name):
    """The text of FusedMLP.<name>, whichever module of the engine defines it (through the stream-ordering wrapper)."""
    import inspect
    from vbnn_amd.engine import FusedMLP
    return inspect.getsource(getattr(FusedMLP, name))


def _ordered_calls(body, call_re, helpers, drop=()):
    """Library calls of `body` in source order, a helper's calls (and its helpers') in place of each call of it, consecutive
    repeats folded."""
    pat = "|".join([call_re] + [re.escape(h) for h in helpers])
    out = []
    for m in re.finditer(pat, body):
        tok = m.group(0)
        names = _ordered_calls(helpers[tok], call_re, helpers) if tok in helpers else [m.group(1)]
        for n in names:
            if n not in drop and (not out or out[-1] != n):
                out.append(n)
    return out


def _lua():
    raw = open(os.path.join(ROOT, "lua", "FusedMLP.lua")).read()
    return raw, re.sub(r"--[^\n]*", " ", raw)


def _c_fn(c, name):
    i = re.search(r"static void %s\([^;{]*\)\s*\{" % name, c).end() - 1
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(c[j], 0)
        j += 1
    return c[i:j]


def _host_orders():
    py = _ordered_calls(_src("predict"), r"lib\.(vbnn_[a-z0-9_]+)\(",
                        {"self.%s(" % h: _src(h) for h in ("_predictive_plan", "_draw_forward", "_predict_wn_sample", "_predict_forward",
                                                           "_consume_draws")},
                        drop=HOST_ONLY_WN)
    _, lua = _lua()
    lu = _ordered_calls(_section(lua, "function FusedMLP:predict(", "function FusedMLP:_predict_forward("), r"\bC\.(vbnn_[a-z0-9_]+)\s*\(",
                        {"self:_predict_forward(": _section(lua, "function FusedMLP:_predict_forward(", "return FusedMLP")}, drop=READ_BACK)
    c = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "tools", "c_host.c")).read(), flags=re.S)
    cc = _ordered_calls(_c_fn(c, "fm_predict"), r"\b(vbnn_[a-z0-9_]+)\s*\(", {"fm_predict_forward(": _c_fn(c, "fm_predict_forward")},
                        drop=READ_BACK)
    return py, lu, cc


def test_the_three_hosts_issue_predict_calls_in_the_same_order():
    """FusedMLP.predict, lua FusedMLP:predict and c_host's fm_predict: the same library calls in the same order (the stacked
    branch, the one-draw branch, the device counter), so what the GPU test proves of the C program holds for the Lua file."""
    py, lu, cc = _host_orders()
    assert py == lu == cc, (py, lu, cc)
    assert py == ["vbnn_pack_input", "vbnn_forward", "vbnn_head_predict", "vbnn_pack_input", "vbnn_forward", "vbnn_head_predict",
                  "vbnn_sample"], py


def test_lua_predict_structure():
    """lua/FusedMLP.lua's predict (+ its forward helper), linted: after :loss_and_accuracy (outside the ranges the other lints
    slice), blocks balance, every C.vbnn_* call is declared with that many parameters, every field it sets exists."""
    import sys
    sys.path.insert(0, ROOT)
    from tests.test_abi import _calls, _lua_tokens  # noqa: E402
    raw, lua = _lua()
    assert raw.index("function FusedMLP:loss_and_accuracy") < raw.index("function FusedMLP:predict(") < \
        raw.index("function FusedMLP:_predict_forward(") < raw.index("\nreturn FusedMLP")
    chunk = raw[raw.index("function FusedMLP:predict("):raw.index("\nreturn FusedMLP")]
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "chunk.lua")
        open(p, "w").write(chunk)
        txt, toks = _lua_tokens(p)
    opens = sum(toks.count(k) for k in ("function", "if", "for", "while"))
    bare_do = toks.count("do") - toks.count("for") - toks.count("while")
    assert bare_do == 0 and opens == toks.count("end"), (opens, bare_do, toks.count("end"))
    assert txt.count("(") == txt.count(")") and txt.count("{") == txt.count("}") and txt.count("[") == txt.count("]")
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): len([q for q in m.group(2).split(",") if q.strip() and q.strip() != "void"])
              for m in re.finditer(r"(vbnn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    calls = _calls(txt)
    assert {n for n, _ in calls} == {"vbnn_pack_input", "vbnn_forward", "vbnn_head_predict", "vbnn_sample", "vbnn_buf_download"}
    for name, n in calls:
        assert n == protos[name], (name, n, protos[name])
    structs = {m.group(2): set(re.findall(r"(\w+)\s*(?=[,;])", m.group(1)))
               for m in re.finditer(r"typedef struct \w+ \{(.*?)\}\s*(vbnn_\w+);", hdr, flags=re.S)}
    checked = 0
    for var, st in (("pa", "vbnn_predict_args"), ("fa", "vbnn_fwd_args")):
        assert re.search(r"local %s = ffi\.new\('%s'\)" % (var, st), chunk)
        for m in re.finditer(r"(?<![\w.])%s\.(\w+)" % var, chunk):
            assert m.group(1) in structs[st], f"{var}.{m.group(1)}: no such field in {st}"
            checked += 1
    assert checked >= 30, checked
