"""CPU tests of the conformal-interval boundary: vbnn_conformal_interval_args and vbnn_select_columns_args as gcc lays them out
from the header against the ctypes mirrors, the symbols in the library / the ctypes table / the Lua cdef, the constants, the ABI
version unchanged (additive), the engine's signatures and result classes, and every host-side refusal that needs no device."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbnn_hip.h")
STRUCTS = {"vbnn_conformal_interval_args": "ConformalIntervalArgs", "vbnn_select_columns_args": "SelectColumnsArgs"}


def _probe():
    from vbnn_amd import _lib as L
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("caps %d %d\\n", (int)VBNN_CONFORMAL_MAX_Q, (int)VBNN_SELECT_COLUMNS_MAX_Q);',
             'printf("abi %d\\n", (int)VBNN_ABI_VERSION);']
    for cname, pname in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(L, pname)._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {l.split()[0]: l.split()[1:] for l in out if l}


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_args_match_the_header(cname):
    from vbnn_amd import _lib as L
    st = getattr(L, STRUCTS[cname])
    got = _probe()
    assert int(got[cname][0]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[f"{cname}.{fname}"][0]) == getattr(st, fname).offset, fname
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (cname, cname), hdr, flags=re.S).group(1)
    cfields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert cfields == [f for f, _ in st._fields_]           # every field of the C struct is mirrored, in order


def test_constants_and_abi_version():
    from vbnn_amd import _lib as L
    got = _probe()
    assert got["caps"] == ["8", "8"] and (L.CONFORMAL_MAX_Q, L.SELECT_COLUMNS_MAX_Q) == (8, 8)
    assert int(got["abi"][0]) == 6                              # additive: two symbols, two structs
    assert L.lib().vbnn_abi_version() == 6
    from vbnn_amd import conformal
    assert conformal.W_MIN == 2.0 ** -60


def test_entry_points_are_exported_and_declared_everywhere():
    from vbnn_amd import _lib as L
    lua = open(os.path.join(ROOT, "lua", "vbnn_ffi.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for sym, cname in (("vbnn_conformal_interval", "vbnn_conformal_interval_args"), ("vbnn_select_columns", "vbnn_select_columns_args")):
        assert sym in L.exported_symbols() and hasattr(C.CDLL(L.LIB_PATH), sym)
        args, res = L._SIGS[sym]
        assert res is C.c_int and len(args) == 2 and args[1] is C.POINTER(getattr(L, STRUCTS[cname]))
        assert re.search(r"int %s\(vbnn_ctx\* ctx, const %s\* a\);" % (sym, cname), cdef)
        assert f"typedef struct {cname} {{" in cdef
    # the header states why covered follows the score, and the kernels are built without contraction
    hdr = open(HEADER).read()
    assert "COVERED FOLLOWS THE SCORE" in hdr
    mk = open(os.path.join(ROOT, "vbnn_amd", "csrc", "Makefile")).read()
    assert "conformal_interval.hip" in mk.split("SRCS =")[1].split("\n")[0].split()
    assert "$(LIBDIR)/obj/conformal_interval.o" in [l for l in mk.split("\n") if "-ffp-contract=off" in l and l.startswith("$(LIBDIR)")][0]


def test_engine_surface():
    from vbnn_amd.engine import FusedMLP, IntervalCalibration, IntervalResult
    sig = inspect.signature(FusedMLP.conformal_calibrate_intervals)
    assert list(sig.parameters) == ["self", "result", "targets", "levels", "score", "scope", "noise_var"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [(0.9,), "scaled", "per_output", None]
    sig = inspect.signature(FusedMLP.conformal_intervals)
    assert list(sig.parameters) == ["self", "result", "calibration", "targets", "keep_covered", "into"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, False, None]
    # the host arithmetic on integers alone (no device): two levels, merge adds
    words = [40, 30, 10, 4, 2, 0, 0, 0,   40, 40, 10, 10, 0, 0, 0, 0,   3, 1]
    a = IntervalResult([0.8, 0.95], 4, None, words)
    assert a.n == [40, 40] and a.n_rows == [10, 10] and a.n_nan == 3 and a.n_nan_rows == 1
    assert a.coverage == [0.75, 1.0] and a.joint_coverage == [0.4, 1.0] and a.empty_fraction == [0.05, 0.0]
    assert a.lo is None and a.mean_width is None and a.coverage_per_output is None
    b = a.merge(a)
    assert b.n == [80, 80] and b.n_nan == 6 and b.coverage == a.coverage and b.joint_coverage == a.joint_coverage
    assert b.counts() == [2 * w for w in words]
    with pytest.raises(ValueError, match="merge"):
        a.merge(IntervalResult([0.8], 4, None, [0] * 10))
    with pytest.raises(ValueError, match="merge"):
        a.merge(IntervalResult([0.8, 0.95], 5, None, [0] * 18))
    blind = IntervalResult([0.8], 4, None, [8, 0, 2, 0, 1, 0, 0, 0, 0, 0], targets=False)
    assert blind.coverage[0] != blind.coverage[0] and blind.joint_coverage[0] != blind.joint_coverage[0]
    assert blind.empty_fraction == [0.125]
    zero = IntervalResult([0.8], 4, None, [0] * 10)
    assert zero.coverage[0] != zero.coverage[0]                 # 0 / 0: NaN
    cal = IntervalCalibration("scaled", "joint", [0.9], 99, [90], 3, 0.5, 2.0 ** -60, "mse", None, None, None, None)
    assert (cal.score, cal.scope, cal.levels, cal.n, cal.k, cal.D, cal.noise_var, cal.criterion) == ("scaled", "joint", [0.9], 99, [90], 3, 0.5, "mse")


class _Engine:
    """The mixin without a device: what it refuses before it touches one."""
    def __init__(self, criterion="mse"):
        self.criterion = criterion

    def _on_stream(self):
        import contextlib
        return contextlib.nullcontext()


def _engine(criterion="mse"):
    from vbnn_amd.conformal import _Conformal
    return type("E", (_Engine, _Conformal), {})(criterion)


class _Reg:
    def __init__(self, mean, var, noise_var=None):
        self.mean, self.var, self.noise_var = mean, var, noise_var


class _Quant:
    def __init__(self, probs, quantiles, moments):
        self.probs, self.quantiles, self.moments = probs, quantiles, moments


def test_refusals_that_need_no_device():
    import torch
    from vbnn_amd.conformal import IntervalCalibration, IntervalResult, conformal_rank
    assert conformal_rank(199, 0.9) == 180 and conformal_rank(5, 0.9) == 6
    eng = _engine()
    m, t = torch.zeros(4, 3), torch.zeros(4, 3)
    reg = _Reg(m, m)

    def cal(**kw):
        base = dict(score="scaled", scope="per_output", levels=[0.9], n=4, k=[5], D=3, noise_var=None, w_min=2.0 ** -60,
                    criterion="mse", probs=None, scores=None, qhat_dev=None, acc_dev=None)
        base.update(kw)
        return IntervalCalibration(**base)

    for crit in ("nll", "bce"):
        with pytest.raises(ValueError, match=crit):
            _engine(crit).conformal_calibrate_intervals(reg, t)
        with pytest.raises(ValueError, match=crit):
            _engine(crit).conformal_intervals(reg, cal())
    with pytest.raises(ValueError, match="score = 'aps'"):
        eng.conformal_calibrate_intervals(reg, t, score="aps")
    with pytest.raises(ValueError, match="scope = 'row'"):
        eng.conformal_calibrate_intervals(reg, t, scope="row")
    for levels in ((), (0.0,), (1.0,), (0.5, 1.5), (-0.1,), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="levels"):
            eng.conformal_calibrate_intervals(reg, t, levels=levels)
    # "cqr": a quantile result, with both probabilities of every level, at most 4 levels
    with pytest.raises(ValueError, match="QuantilePredictResult"):
        eng.conformal_calibrate_intervals(reg, t, score="cqr")
    q = _Quant([0.05000000074505806, 0.5, 0.8999999761581421], torch.zeros(3, 4, 3), reg)
    with pytest.raises(ValueError, match=r"0\.05 and 0\.95"):
        eng.conformal_calibrate_intervals(q, t, score="cqr", levels=(0.9,))
    with pytest.raises(ValueError, match=r"0\.1 and 0\.9"):
        eng.conformal_calibrate_intervals(q, t, score="cqr", levels=(0.8,))
    with pytest.raises(ValueError, match="at most 4"):
        eng.conformal_calibrate_intervals(q, t, score="cqr", levels=(0.5, 0.6, 0.7, 0.8, 0.9))
    # noise_var: "mse" + "scaled" only
    with pytest.raises(ValueError, match="noise_var"):
        eng.conformal_calibrate_intervals(reg, t, score="absolute", noise_var=0.5)
    with pytest.raises(ValueError, match="noise_var"):
        _engine("gauss").conformal_calibrate_intervals(_Reg(m, m, m), t, noise_var=0.5)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="noise_var"):
            eng.conformal_calibrate_intervals(reg, t, noise_var=bad)
    # tensors: on the device, fp32, R x D
    with pytest.raises(ValueError, match="on the device"):
        eng.conformal_calibrate_intervals(reg, t)
    with pytest.raises(ValueError, match="fp32"):
        eng.conformal_calibrate_intervals(_Reg(m.double(), m), t)
    with pytest.raises(ValueError, match="fp32"):
        eng.conformal_calibrate_intervals(_Reg(m[0], m), t)
    with pytest.raises(ValueError, match="RegressionPredictResult"):
        eng.conformal_calibrate_intervals(object(), t)
    with pytest.raises(ValueError, match="empty list"):
        eng.conformal_calibrate_intervals([], [])
    # a calibration that does not match, by name
    with pytest.raises(ValueError, match="IntervalCalibration"):
        eng.conformal_intervals(reg, object())
    with pytest.raises(ValueError, match="criterion"):
        eng.conformal_intervals(reg, cal(criterion="gauss"))
    with pytest.raises(ValueError, match="score"):
        eng.conformal_intervals(reg, cal(score="aps"))
    with pytest.raises(ValueError, match="scope"):
        eng.conformal_intervals(reg, cal(scope="row"))
    with pytest.raises(ValueError, match="w_min"):
        eng.conformal_intervals(reg, cal(w_min=1e-3))
    with pytest.raises(ValueError, match="noise_var"):
        eng.conformal_intervals(reg, cal(score="absolute", noise_var=0.5))
    with pytest.raises(ValueError, match="QuantilePredictResult"):
        eng.conformal_intervals(reg, cal(score="cqr"))
    with pytest.raises(ValueError, match="levels"):
        eng.conformal_intervals(reg, cal(levels=[0.9, 1.5], k=[5, 5]))
    # the options alone, as the trainer checks them before its pass
    from vbnn_amd.conformal import check_interval_options
    p32 = torch.tensor([0.05, 0.1, 0.9, 0.95], dtype=torch.float32).tolist()     # (as predict_quantiles holds them)
    assert check_interval_options("opt", [0.8, 0.9], "cqr", "joint", p32) == [0.8, 0.9]
    for kw, msg in ((dict(levels=[1.5]), "levels"), (dict(score="aps"), "score = 'aps'"), (dict(scope="row"), "scope = 'row'"),
                    (dict(levels=[0.5, 0.6, 0.7, 0.8, 0.9], score="cqr"), "at most 4"),
                    (dict(score="cqr", probs=[0.1, 0.95]), r"0\.05 and 0\.95")):
        with pytest.raises(ValueError, match=msg):
            check_interval_options("opt", **{**dict(levels=[0.9], score="scaled", scope="per_output"), **kw})


def test_split_rows_cuts_results_and_targets_at_the_same_row():
    """The helper that splits the trainer's dev rows into a calibration half and a test half. (What conformal_intervals compares
    after it has the planes -- D, probs, the thresholds' shape, into= -- needs device tensors:
    tests/test_interval_gpu.py::test_engine_refusals_that_need_device_tensors.)"""
    import torch
    from vbnn_amd.conformal import split_rows
    a, b = _Reg(torch.arange(6.0).view(3, 2), torch.zeros(3, 2)), _Reg(torch.arange(8.0).view(4, 2) + 10, torch.ones(4, 2))
    ta, tb = torch.zeros(3, 2), torch.ones(4, 2)
    (r1, t1), (r2, t2) = split_rows([a, b], [ta, tb], 3)
    assert r1 == [a] and r2 == [b] and t1[0].shape[0] == 3 and t2[0].shape[0] == 4
    (r1, t1), (r2, t2) = split_rows([a, b], [ta, tb], 5)
    assert r1[0] is a and torch.equal(r1[1].mean, b.mean[:2]) and torch.equal(r2[0].mean, b.mean[2:]) and r2[0].noise_var is None
    assert [t.shape[0] for t in t1] == [3, 2] and [t.shape[0] for t in t2] == [2]
    q = _Quant([0.1, 0.9], torch.arange(28.0).view(2, 7, 2), _Reg(torch.zeros(7, 2), torch.zeros(7, 2)))
    (r1, _), (r2, _) = split_rows([q], [torch.zeros(7, 2)], 3)
    assert torch.equal(r1[0].quantiles, q.quantiles[:, :3]) and torch.equal(r2[0].quantiles, q.quantiles[:, 3:])
    assert r1[0].probs == q.probs and r2[0].moments.mean.shape[0] == 4
