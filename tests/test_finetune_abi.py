"""Training under a held pruning mask, the parts that need no GPU: the three masked entry points are declared in
include/vbnn_hip.h, exported by the library and bound by ctypes; the Lua cdef carries them; lua/FusedMLP.lua and tools/c_host.c
reach them (and the C host still builds warning-free); the engine and the trainer expose the feature."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbnn_prepare_masked", "vbnn_update_masked", "vbnn_calc_lc_masked")


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "vbnn_hip.h")).read(), flags=re.S)


def _params(name, text):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    return [p.strip() for p in m.group(1).split(",")]


def test_masked_entry_points_are_declared_exported_and_bound():
    from vbnn_amd import _lib as L
    hdr = _header()
    assert "#define VBNN_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "vbnn_hip.h")).read()      # additive: the ABI stays 6
    lib = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        params = _params(name, hdr)
        assert hasattr(lib, name), f"{name} is not exported by libvbnn_hip.so"
        args, res = L._SIGS[name]
        assert len(args) == len(params) and res is C.c_int, (name, len(args), params)
    # the descriptor structs are reused: the masks are one more argument, a host array of device byte pointers
    for name, base in (("vbnn_prepare_masked", "vbnn_prepare"), ("vbnn_update_masked", "vbnn_update")):
        got, want = _params(name, hdr), _params(base, hdr)
        assert got[:4] == want[:4] and got[5:] == want[4:], (got, want)
        assert re.sub(r"\s+", " ", got[4]) == "const uint8_t* const* masks"
    assert any("uint8_t" in p and "mask" in p for p in _params("vbnn_calc_lc_masked", hdr))


def test_lua_cdef_and_lua_host_carry_the_masked_calls():
    cdef = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    hdr = _header()
    for name in NAMES:
        assert len(_params(name, cdef)) == len(_params(name, hdr)), name
    lua = re.sub(r"--[^\n]*", " ", open(os.path.join(ROOT, "lua", "FusedMLP.lua")).read())
    for method in ("hold_pruned", "release_pruned"):
        assert re.search(r"function FusedMLP:%s\(" % method, lua), method
    run = lua[lua.index("function FusedMLP:run"):lua.index("function FusedMLP:finish")]
    assert "masked" not in run                                          # the step itself does not know about the mask

    def body(name, until):
        i = lua.index("function FusedMLP:%s" % name)
        return lua[i:lua.index("function FusedMLP:%s" % until, i + 1)]
    assert "C.vbnn_prepare_masked(" in body("prepare", "sample")
    assert "C.vbnn_update_masked(" in body("update", "calc_lc")
    assert "C.vbnn_calc_lc_masked(" in body("calc_lc", "loss_and_accuracy")
    # the masks' vb.alloc cdata (whose finaliser frees the buffer) must stay referenced for as long as the mask is held
    hold = body("hold_pruned", "release_pruned")
    assert re.search(r"bufs\[li\]\s*=\s*mask|bufs\[li\]\s*=.*\bmask\b", hold) and "self.held_bufs" in hold
    assert "held_bufs" in lua[lua.index("function FusedMLP:release_pruned"):][:400]


def test_c_host_has_the_hold_flag_and_builds(tmp_path):
    from tests.test_c_host import SRC, build
    src = re.sub(r"/\*.*?\*/", " ", open(SRC).read(), flags=re.S)
    assert '"--hold"' in src
    for name in ("vbnn_prepare_masked", "vbnn_update_masked"):
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert os.path.exists(build(tmp_path))                              # -Wall -Wextra -Werror against the header alone


def test_engine_and_trainer_expose_the_feature():
    from vbnn_amd import train
    from vbnn_amd.engine import FusedMLP
    for name in ("hold_pruned", "release_pruned", "held_mask"):
        assert callable(getattr(FusedMLP, name)), name
    assert isinstance(FusedMLP.held, property)
    doc = FusedMLP.hold_pruned.__doc__
    assert "follow-up" in doc and "exceed" in doc                       # what is left for later, and the gradual-schedule caveat
    # run() is compared with lua/FusedMLP.lua by source text: the mask must not appear in it
    assert "held" not in inspect.getsource(FusedMLP.run) and "masked" not in inspect.getsource(FusedMLP.run)
    src = inspect.getsource(train.Main)
    assert "prune_schedule" in src and "held fraction" in src and "prune_scope" in src
    assert "prune_schedule" not in train.default_opt()                  # off by default
