"""CPU tests of the checkpoint's boundary: vbnn_digest in the library / the ctypes table / the header / the Lua cdef, the ABI version
unchanged (additive), and the engine's and the trainer's signatures."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
DECL = r"int vbnn_digest\(vbnn_ctx\* ctx, const void\* buf, uint64_t n_words, uint64_t index0, uint64_t\* out\);"


def test_digest_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    assert "vbnn_digest" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "vbnn_digest")
    args, res = L._SIGS["vbnn_digest"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    hdr = open(HEADER).read()
    assert re.search(DECL, hdr)
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    assert re.search(DECL, lua[lua.index("ffi.cdef[["):lua.index("]]")])
    assert "digest.hip" in open(os.path.join(ROOT, "vbnn_amd", "csrc", "Makefile")).read()


def test_the_header_states_the_digest_contract():
    hdr = open(HEADER).read()
    doc = hdr[hdr.index("a device digest of a buffer"):hdr.index("int vbnn_digest(")]
    for piece in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "z >> 30", "z >> 27", "z >> 31", "index0 + i + 1", "NOT cryptographic",
                  "2^32 - 1", "4-byte aligned", "n_words = 0"):
        assert piece in doc, piece


def test_abi_version_is_still_6():
    from vbnn_amd import _lib as L
    assert re.search(r"^#define VBNN_ABI_VERSION 6$", open(HEADER).read(), flags=re.M)
    assert L.lib().vbnn_abi_version() == 6


def test_engine_and_trainer_surface():
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import engine
    from vbnn_amd.engine import FusedMLP
    assert list(inspect.signature(FusedMLP.state_dict).parameters) == ["self"]
    assert list(inspect.signature(FusedMLP.load_state_dict).parameters) == ["self", "state"]
    assert list(inspect.signature(FusedMLP.save).parameters)[:2] == ["self", "path"]
    sig = inspect.signature(FusedMLP.load)
    assert list(sig.parameters) == ["path", "device", "opt_overrides"] and sig.parameters["device"].default is None
    assert sig.parameters["opt_overrides"].kind is inspect.Parameter.VAR_KEYWORD
    assert isinstance(inspect.getattr_static(FusedMLP, "load"), classmethod)
    assert list(inspect.signature(FusedMLP.check_replicas).parameters) == ["self"]
    assert list(inspect.signature(engine.digest).parameters)[0] == "tensor"
    assert (ck.FORMAT, ck.VERSION) == ("vbnn_amd.checkpoint", 1)
    from vbnn_amd import train
    assert not train.default_opt().get("checkpoint") and not train.default_opt().get("network_to_load")     # both off by default


def test_the_sharded_update_is_refused_with_the_follow_up_named():
    """The refusal's condition on the CPU side: both entry points ask the same guard before touching the device."""
    import pytest
    from vbnn_amd.checkpoint import _Checkpoint

    class Sharded(_Checkpoint):
        sharded = True

    for call in (lambda e: e.state_dict.__wrapped__(e), lambda e: e.load_state_dict.__wrapped__(e, {}),
                 lambda e: e._refuse_sharded("check_replicas")):
        with pytest.raises(RuntimeError, match="sharded update.*follow-up"):
            call(Sharded())
