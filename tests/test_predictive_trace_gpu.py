"""GPU test of the predictive driver's CALL SEQUENCE: every library call each posterior-predictive entry point makes (predict,
predict_classes, predict_regression, predict_quantiles, predict_analytic), in order, with every scalar argument and, for every
pointer, whether it is null -- against tests/golden/predictive_trace.json. The oracle tests hold the results within float
tolerances and the chunking tests hold the pointer offsets; what a change to the driver (vbnn_amd/predictive.py) can break
unseen by both is which call is made when, with which counts, draws, rows and forms. Addresses are never recorded.

The fixture is a RECORDING of the commit before the driver was last rearranged, made by this module's own recorder,

    python -m tests.test_predictive_trace_gpu OUT.json        (from the root of a checkout of THAT commit, this file copied in)

and is never regenerated from the code under test: a driver that is meant to issue other calls gets a new recording from its
parent, and the change says why they differ."""
import ctypes as C
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predictive_trace.json")
# the smallest network with two hidden widths and a ragged last chunk: predict_rows = 16 gives chunks of 16, 16, 5 rows one draw
# at a time and of 5, 5, 5, 5, 5, 5, 5, 2 with the S = 3 draws stacked
I0, HIDDEN, R, S, SEED, ROWS = 70, [50, 34], 37, 3, 3, 16
D = 6                                                           # regression outputs
CT, RT = "class targets", "regression targets"
PREDICT = dict(S=S, targets=CT)
CLASSES = dict(S=S, targets=CT, topk=3)
MSE = dict(criterion="mse", n_classes=D)

# name: (engine options, pruned view, entry point, its keyword arguments)
CASES = {
    "predict lrt f32 stacked": (dict(), None, "predict", PREDICT),
    "predict lrt f32 per draw": (dict(predict_stacked=False), None, "predict", PREDICT),
    "predict lrt bf16 per draw": (dict(dtype="bf16", predict_stacked=False), None, "predict", PREDICT),
    "predict wn f32": (dict(mode="wn"), None, "predict", PREDICT),
    "predict map": (dict(), None, "predict", dict(PREDICT, map=True)),
    "predict dense view": (dict(), "dense", "predict", PREDICT),
    "predict compressed view": (dict(), "compressed", "predict", PREDICT),
    "classes stacked": (dict(n_classes=20), None, "predict_classes", CLASSES),
    "classes stacked keep_draws": (dict(n_classes=20), None, "predict_classes", dict(CLASSES, keep_draws=True)),
    "classes per draw no probs": (dict(n_classes=20, predict_stacked=False), None, "predict_classes", dict(CLASSES, keep_probs=False)),
    "regression mse stacked": (MSE, None, "predict_regression", dict(S=S, targets=RT, noise_var=0.3)),
    "regression mse per draw": (dict(MSE, predict_stacked=False), None, "predict_regression", dict(S=S, targets=RT, noise_var=0.3)),
    "regression gauss stacked": (dict(criterion="gauss", n_classes=2 * D), None, "predict_regression", dict(S=S, targets=RT)),
    "quantiles mse": (MSE, None, "predict_quantiles", dict(probs=[0.05, 0.5, 0.95], S=S, targets=RT)),
    "analytic mse": (MSE, None, "predict_analytic", dict(targets=RT, noise_var=0.3)),
    "analytic nll keep_probs": (dict(), None, "predict_analytic", dict(S=S, targets=CT, keep_probs=True)),
    "analytic nll topk": (dict(), None, "predict_analytic", dict(S=S, targets=CT, keep_probs=False, topk=2)),
}


class Recorder:
    """A proxy around the loaded library: forwards every call and, while `calls` is a list, logs [name, argument, ...] per
    vbnn_amd._lib._SIGS -- a scalar's value; 1 / 0 for a pointer that is set / null; for byref(struct) the same of every field."""

    def __init__(self, real, sigs):
        self._real, self._sigs, self.calls = real, sigs, None

    @staticmethod
    def _set(a):
        return int(bool(a.value if isinstance(a, C.c_void_p) else a))

    @classmethod
    def _value(cls, ctype, a):
        if ctype is C.c_void_p or ctype is C.c_char_p:
            return cls._set(a)
        if issubclass(ctype, C.Array):
            return [cls._value(ctype._type_, v) for v in a]
        if issubclass(ctype, C._Pointer):
            if a is None or not issubclass(ctype._type_, C.Structure):
                return cls._set(a)
            return [cls._value(ft, getattr(a._obj, fname)) for fname, ft in ctype._type_._fields_]
        return a.value if isinstance(a, C._SimpleCData) else a

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._sigs:
            return fn

        def call(*args):
            if self.calls is not None:
                self.calls.append([name] + [self._value(t, a) for t, a in zip(self._sigs[name][0], args)])
            return fn(*args)
        return call


def trace(name, rec):
    """One case on an engine of its own: {"draw": eng.draw after the call, "calls": what `rec` logged during it}, and the result."""
    import torch
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    eng_kw, view, entry, kw = CASES[name]
    opt = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=SEED, input_size=I0, hidden=list(HIDDEN),
               n_classes=10, type="vb", testSamples=2, predict_rows=ROWS)
    opt.update(eng_kw)
    eng = FusedMLP(opt)
    eng.prepare()
    x = nn.fill_normal(torch.empty(R, I0, dtype=torch.float32, device="cuda"), SEED, 4, 0, 0)
    kw = dict(kw)
    if kw.get("targets") == CT:
        kw["targets"] = (torch.arange(R, device="cuda") * 7 % opt["n_classes"]).to(torch.int32)
    elif kw.get("targets") == RT:
        kw["targets"] = nn.fill_normal(torch.empty(R, D, dtype=torch.float32, device="cuda"), SEED, 4, 1, 0)
    pruned = eng.prune(fraction=0.5) if view else None
    if view == "compressed":
        pruned = pruned.compress()
    torch.cuda.synchronize()
    if pruned is not None:
        eng.use_pruned(pruned)
    rec.calls = []
    try:
        res = getattr(eng, entry)(x, **kw)
    finally:
        calls, rec.calls = rec.calls, None
    return {"draw": eng.draw, "calls": calls}, res


def recorder(setattr_):
    """The recorder in place of the loaded library (after a first real lib() call), put there through `setattr_`."""
    import torch  # noqa: F401  (before the library is loaded: both then share the HIP runtime torch brings)
    from vbnn_amd import _lib as L
    rec = Recorder(L.lib(), L._SIGS)
    setattr_(L, "_lib", rec)
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_entry_point_makes_the_recorded_calls(name, golden, monkeypatch):
    got, _ = trace(name, recorder(monkeypatch.setattr))
    got = json.loads(json.dumps(got))                           # (floats and lists as the fixture holds them)
    want = golden[name]
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {k} differs\n  recorded: {w}\n  made:     {g}"
    n, m = len(got["calls"]), len(want["calls"])
    assert n == m, f"{name}: {n} calls made, {m} recorded; the first one beyond: {(got if n > m else want)['calls'][min(n, m)]}"
    assert got["draw"] == want["draw"], f"{name}: eng.draw = {got['draw']} after the call, {want['draw']} recorded"


def record(path):
    from vbnn_amd import _lib as L
    rec = recorder(setattr)
    out = {name: trace(name, rec)[0] for name in CASES}
    with open(path, "w") as f:                                  # one call per line
        f.write("{\n" + ",\n".join(
            f'{json.dumps(n)}: {{"draw": {c["draw"]}, "calls": [\n' + ",\n".join(json.dumps(call) for call in c["calls"]) + "\n]}"
            for n, c in out.items()) + "\n}\n")
    assert json.load(open(path)) == json.loads(json.dumps(out)) and isinstance(L._lib, Recorder)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
