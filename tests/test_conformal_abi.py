"""CPU tests of the conformal boundary: vbnn_conformal_args as gcc lays it out from the header against the ctypes mirror, the
symbol in the library / the ctypes table / the Lua cdef, the constants, the ABI version unchanged (additive), the engine's
signatures and result classes, and every host-side refusal that needs no device."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
CNAME, PNAME = "vbnn_conformal_args", "ConformalArgs"


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("caps %d %d %d\\n", (int)VBNN_CONFORMAL_MAX_Q, (int)VBNN_CONFORMAL_LAC, (int)VBNN_CONFORMAL_APS);',
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
    st = L.ConformalArgs
    got = _probe()
    assert int(got[CNAME][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"{CNAME}.{fname}"][0]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (CNAME, CNAME), hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]           # every field of the C struct is mirrored, in order


def test_constants_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["caps"] == ["8", "0", "1"] and (L.CONFORMAL_MAX_Q, L.CONFORMAL_LAC, L.CONFORMAL_APS) == (8, 0, 1)
    assert int(got["abi"][0]) == 6                              # additive: one symbol, one struct
    assert L.lib().vbnn_abi_version() == 6


def test_entry_point_is_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert "vbnn_conformal" in L.exported_symbols() and hasattr(C.CDLL(L.LIB_PATH), "vbnn_conformal")
    args, res = L._SIGS["vbnn_conformal"]
    assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(L.ConformalArgs)
    assert re.search(r"int vbnn_conformal\(vbnn_ctx\* ctx, const vbnn_conformal_args\* a\);", cdef)
    assert f"typedef struct {CNAME} {{" in cdef
    # the header states what the method rests on, and the kernel is built without contraction
    hdr = open(HEADER).read()
    assert "PREFIX OF THE RANKING" in hdr and "NON-DECREASING" in hdr
    mk = open(os.path.join(ROOT, "vbnn_amd", "csrc", "Makefile")).read()
    assert "conformal.hip" in mk.split("SRCS =")[1].split("\n")[0]
    assert "$(LIBDIR)/obj/conformal.o" in [l for l in mk.split("\n") if "-ffp-contract=off" in l and l.startswith("$(LIBDIR)")][0]


def test_engine_surface():
    from vbnn_amd.engine import ConformalCalibration, ConformalResult, FusedMLP
    sig = inspect.signature(FusedMLP.conformal_calibrate)
    assert list(sig.parameters) == ["self", "result", "targets", "levels", "score"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [(0.9,), "aps"]
    sig = inspect.signature(FusedMLP.conformal_sets)
    assert list(sig.parameters) == ["self", "result", "calibration", "targets", "members", "into"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, False, None]
    # the host arithmetic on integers alone (no device): two levels, merge adds
    words = [10, 8, 25, 1, 4, 3, 2, 0,   10, 10, 60, 0, 0, 0, 5, 0,   2, 0]
    a = ConformalResult([0.8, 0.95], 6, None, words)
    assert a.n == [10, 10] and a.n_nan == 2 and a.coverage == [0.8, 1.0] and a.mean_size == [2.5, 6.0]
    assert a.empty_fraction == [0.1, 0.0] and a.singleton_fraction == [0.4, 0.0] and a.full_fraction == [0.2, 0.5]
    assert a.singleton_accuracy[0] == 0.75 and a.singleton_accuracy[1] != a.singleton_accuracy[1]       # 0 / 0: NaN
    b = a.merge(a)
    assert b.n == [20, 20] and b.n_nan == 4 and b.coverage == a.coverage and b.mean_size == a.mean_size and b.size is None
    assert b.counts() == [2 * w for w in words]
    with pytest.raises(ValueError, match="merge"):
        a.merge(ConformalResult([0.8], 6, None, [0] * 10))
    blind = ConformalResult([0.8], 6, None, [4, 0, 8, 0, 0, 0, 0, 0, 0, 0], targets=False)
    assert blind.coverage[0] != blind.coverage[0] and blind.mean_size == [2.0]
    cal = ConformalCalibration("aps", 6, [0.9], 99, [90], None, None, None)
    assert (cal.score_kind, cal.classes, cal.levels, cal.n, cal.k) == ("aps", 6, [0.9], 99, [90])


class _Engine:
    """The mixin without a device: what it refuses before it touches one."""
    def __init__(self, criterion="nll"):
        self.criterion = criterion

    def _on_stream(self):
        import contextlib
        return contextlib.nullcontext()


def _engine(criterion="nll"):
    from vbnn_amd.conformal import _Conformal
    return type("E", (_Engine, _Conformal), {})(criterion)


class _Result:
    def __init__(self, probs):
        self.probs = probs


def test_refusals_that_need_no_device():
    import torch
    from vbnn_amd.conformal import ConformalCalibration, conformal_rank
    assert conformal_rank(99, 0.9) == 90 and conformal_rank(5, 0.9) == 6
    eng = _engine()
    probs, t = torch.full((4, 3), 1 / 3), torch.zeros(4, dtype=torch.int32)
    for crit in ("bce", "mse", "gauss"):
        with pytest.raises(ValueError, match="follow-ups"):
            _engine(crit).conformal_calibrate(_Result(probs), t)
        with pytest.raises(ValueError, match=crit):
            _engine(crit).conformal_sets(_Result(probs), ConformalCalibration("aps", 3, [0.9], 4, [5], None, None, None))
    with pytest.raises(ValueError, match="score = 'raps'"):
        eng.conformal_calibrate(_Result(probs), t, score="raps")
    for levels in ((), (0.0,), (1.0,), (0.5, 1.5), (-0.1,), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="levels"):
            eng.conformal_calibrate(_Result(probs), t, levels=levels)
    with pytest.raises(ValueError, match="keep_probs=True"):
        eng.conformal_calibrate(_Result(None), t)
    with pytest.raises(ValueError, match="on the device"):                  # a host tensor
        eng.conformal_calibrate(_Result(probs), t)
    with pytest.raises(ValueError, match="fp32"):
        eng.conformal_calibrate(_Result(probs.double()), t)
    with pytest.raises(ValueError, match="fp32"):
        eng.conformal_calibrate(_Result(probs[0]), t)
    with pytest.raises(ValueError, match="empty list"):
        eng.conformal_calibrate([], [])
    with pytest.raises(ValueError, match="ConformalCalibration"):
        eng.conformal_sets(_Result(probs), object())
