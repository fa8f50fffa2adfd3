"""GPU tests of conformal prediction sets: vbnn_conformal (include/vbnn_hip.h) called directly on uploaded arrays, and
FusedMLP.conformal_calibrate / FusedMLP.conformal_sets / train.py's series over it. Everything is compared BIT FOR BIT with the
fp32 / integer restatement of tests/_conformal_np.py (which tests/test_conformal_ref.py holds to a score-every-class form and to
the float64 definition on the CPU): there are no tolerances here. The thresholds are the restatement's own scores, so that a
kernel that compared with < where the contract says <= (or summed in another order) would move a class across a cut."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._calibration_np import selective32, softmax_case
from tests._conformal_np import (APS, F32, LAC, QNAN_BITS, clamp_targets, conformal32, conformal_rank, derived, member_words,
                                 n_words, tied_case)

pytestmark = pytest.mark.gpu

OUT_KEYS = ("score", "size", "cut_index", "cut_prob", "covered", "member")
SENTINEL_I, SENTINEL_U = -7, 0xDEADBEEF
LAYOUTS = ("dense", "padded", "odd", "offset")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_conformal(probs, target, kind, qhat, layout="dense", outputs=OUT_KEYS, acc=None, with_acc=True, ctx=None):
    """vbnn_conformal on NumPy arrays. layout: dense; padded (16-byte rows, NaN in every pad column); odd (pitch C + 3); offset
    (the base one float past a 16-byte boundary). Every output starts as a sentinel (NaN / -7 / 0xdeadbeef); acc: the
    accumulator's words before the call (zero without). Returns the outputs asked for and acc as uint64. ctx: a context
    handle of the caller's (its stream is its own: the uploads are awaited before the call and vbnn_sync after) in place of the default one."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    R, Cn = probs.shape
    ld = {"dense": Cn, "padded": Cn + 4 - Cn % 4 + 4, "odd": Cn + 3, "offset": Cn}[layout]
    offset = 1 if layout == "offset" else 0
    buf = torch.full((R * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + R * ld].view(R, ld)[:, :Cn] = dev(probs)
    assert buf.data_ptr() % 16 == 0
    qhat = np.asarray(qhat, F32).reshape(-1)
    Q, nw = qhat.size, member_words(Cn)
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    i = lambda *shape: torch.full(shape, SENTINEL_I, dtype=torch.int32, device="cuda")
    make = dict(score=lambda: f(R), size=lambda: i(Q, R), cut_index=lambda: i(Q, R), cut_prob=lambda: f(Q, R),
                covered=lambda: i(Q, R), member=lambda: dev(np.full((Q, R, nw), SENTINEL_U, np.uint32).view(np.int32)))
    out = {k: make[k]() for k in outputs if not (target is None and k in ("score", "covered")) and (Q or k == "score")}
    accd = dev(np.zeros(n_words(Q), np.uint64).view(np.int64) if acc is None else acc.view(np.int64)) if with_acc else None
    td = dev(np.asarray(target, np.int32)) if target is not None else None
    qd = dev(qhat) if Q else None
    a = L.ConformalArgs(probs=buf.data_ptr() + 4 * offset, ld=ld, target=_p(td), R=R, C=Cn, kind=kind, Q=Q, qhat=_p(qd),
                        acc=_p(accd), **{k: _p(v) for k, v in out.items()})
    if ctx is not None:
        torch.cuda.synchronize()
    L.check(L.lib().vbnn_conformal(ctx or Context.get().h, C.byref(a)))
    if ctx is not None:
        L.check(L.lib().vbnn_sync(ctx))
    got = {k: host(v) for k, v in out.items()}
    if "member" in got:
        got["member"] = got["member"].view(np.uint32)
    if with_acc:
        got["acc"] = host(accd).view(np.uint64)
    return got


def assert_equals_restatement(got, want, what):
    for k in got:
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])


def assert_invariants(got, probs, target, qhat, want):
    """What the device outputs say about each other, whatever the restatement says."""
    R, Cn = probs.shape
    qh = np.where(np.isnan(qhat), F32(np.inf), np.asarray(qhat, F32))
    ok = ~want["nan"]
    t = clamp_targets(target, Cn)
    with np.errstate(invalid="ignore"):
        assert ((got["score"][None, :] <= qh[:, None]).astype(np.int32)[:, ok] == got["covered"][:, ok]).all()
    word = got["member"][:, np.arange(R), t >> 5]
    assert (((word >> (t & 31).astype(np.uint32)) & 1).astype(np.int32)[:, ok] == got["covered"][:, ok]).all()
    bits = ((got["member"][..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(qh), R, -1)
    assert (bits[:, :, Cn:] == 0).all()
    assert (bits.sum(2).astype(np.int32)[:, ok] == got["size"][:, ok]).all()
    pos = np.empty_like(want["order"])
    np.put_along_axis(pos, want["order"], np.broadcast_to(np.arange(Cn), pos.shape), axis=1)
    assert ((bits[:, :, :Cn] == 1) == (pos[None] < np.maximum(got["size"], 0)[:, :, None])).all()


def thresholds(probs, target, kind, Q, seed):
    """Q thresholds: the restatement's own scores of some rows first (so that <= against < decides), then a value right below
    every score (empty sets), 0, -1, +inf, NaN and 1 as far as Q reaches."""
    s = conformal32(probs, target, kind)["score"]
    s = s[~np.isnan(s)]
    rng = np.random.default_rng(seed)
    special = [np.nextafter(s.min(), F32(-np.inf)), F32(np.nan), F32(0), F32(np.inf), F32(-1), F32(1)]
    own = list(rng.choice(s, size=max(1, Q - len(special)), replace=True))
    return np.array((own + special + [F32(0.25), F32(0.75)])[:Q], F32)


def case(R, Cn, seed):
    probs, _, target = softmax_case(R, Cn, seed=seed, scale=2.0 if Cn < 1000 else 4.0)
    return probs, target


@pytest.mark.parametrize("kind", [LAC, APS])
@pytest.mark.parametrize("Cn", [1, 2, 3, 10, 16, 17, 255, 256, 257, 1000, 4096, 4099])
def test_kernel_equals_the_restatement(Cn, kind):
    """Every C x R; the layout and the number of thresholds rotate so that each C sees every layout and Q = 1, 3 and 8."""
    for i, R in enumerate((1, 3, 5, 64, 257)):
        probs, target = case(R, Cn, seed=Cn + R)
        Q = (1, 3, 8, 3, 1)[i] if Cn >= 1000 else (8, 3, 1, 8, 3)[i]
        qhat = thresholds(probs, target, kind, Q, seed=R)
        want = conformal32(probs, target, kind, qhat)
        layouts = [LAYOUTS[(i + k) % 4] for k in range(2 if Cn >= 1000 else 4)]
        for layout in layouts:
            got = run_conformal(probs, target, kind, qhat, layout=layout)
            assert_equals_restatement(got, want, (Cn, R, Q, layout))
        assert_invariants(got, probs, target, qhat, want)
        assert int(got["acc"][0]) == R and int(got["acc"][7]) == 0 and int(got["acc"][8 * Q + 1]) == 0


@pytest.mark.parametrize("kind", [LAC, APS])
@pytest.mark.parametrize("Cn", [17, 257, 4099])
@pytest.mark.parametrize("Q", [1, 3, 8])
def test_every_layout_and_threshold_count(Cn, Q, kind):
    R = 5
    probs, target = case(R, Cn, seed=Q)
    qhat = thresholds(probs, target, kind, Q, seed=Cn)
    want = conformal32(probs, target, kind, qhat)
    for layout in LAYOUTS:
        assert_equals_restatement(run_conformal(probs, target, kind, qhat, layout=layout), want, (Cn, Q, layout))


def adversarial_rows(Cn):
    """Sixteenths (tie groups, a cut inside a group), a uniform row, a one-hot row, -0 and subnormals, an entry above 1."""
    P = tied_case(12, Cn, seed=Cn)
    P[1] = F32(1.0 / Cn)
    P[2] = 0
    P[2, Cn // 2] = 1
    P[3, ::2] = F32(-0.0)
    P[3, 1::3] = F32(1e-41)
    P[4] = 0
    P[4, 0] = np.nextafter(np.nextafter(F32(1), F32(2)), F32(2))
    P[5] = F32(-0.0)
    P[5, Cn - 1] = 0.0                                       # +0 ranks above every -0
    rng = np.random.default_rng(Cn)
    target = rng.integers(0, Cn, 12).astype(np.int32)
    target[0], target[1], target[6], target[7] = -3, Cn + 5, Cn, -1
    return P, target


@pytest.mark.parametrize("kind", [LAC, APS])
@pytest.mark.parametrize("Cn", [3, 40, 300, 1100])
def test_adversarial_rows(Cn, kind):
    P, target = adversarial_rows(Cn)
    base = conformal32(P, target, kind)["score"]
    qhat = np.array(list(base[[0, 6, 8, 3]]) + [0, -1, np.inf, np.nan], F32)
    want = conformal32(P, target, kind, qhat)
    got = run_conformal(P, target, kind, qhat)
    assert_equals_restatement(got, want, (Cn, kind))
    assert_invariants(got, P, target, qhat, want)
    assert_equals_restatement(run_conformal(P, clamp_targets(target, Cn).astype(np.int32), kind, qhat), want, "clamp")
    assert (got["size"][6] == Cn).all() and (got["size"][7] == Cn).all()     # +inf, and NaN taken as +inf: every class
    assert (got["size"][5] == 0).all() and (got["cut_index"][5] == -1).all()  # -1: empty sets
    assert (got["cut_prob"][5].view(np.uint32) == QNAN_BITS).all()


@pytest.mark.parametrize("kind", [LAC, APS])
def test_a_nan_row_between_clean_rows(kind):
    R, Cn = 9, 20
    probs, target = case(R, Cn, seed=5)
    qhat = thresholds(probs, target, kind, 3, seed=1)
    clean = run_conformal(probs, target, kind, qhat)
    bad = probs.copy()
    bad[4, next(c for c in range(Cn) if c != target[4])] = np.nan
    got = run_conformal(bad, target, kind, qhat)
    assert_equals_restatement(got, conformal32(bad, target, kind, qhat), "NaN row")
    keep = np.arange(R) != 4
    assert same_bits(got["score"][keep], clean["score"][keep])
    for k in ("size", "cut_index", "cut_prob", "covered", "member"):
        assert same_bits(got[k][:, keep], clean[k][:, keep]), k
    assert np.isnan(got["score"][4]) and np.isnan(got["cut_prob"][:, 4]).all() and (got["member"][:, 4] == 0).all()
    assert (got["size"][:, 4] == -1).all() and (got["cut_index"][:, 4] == -1).all() and (got["covered"][:, 4] == -1).all()
    assert int(got["acc"][8 * 3]) == 1 and [int(got["acc"][8 * q]) for q in range(3)] == [R - 1] * 3
    neg = probs.copy()
    neg[4, 0] = np.array([0xFFFFFFFF], np.uint32).view(F32)[0]          # a NaN with its sign set is a NaN
    assert_equals_restatement(run_conformal(neg, target, kind, qhat), conformal32(neg, target, kind, qhat), "negative NaN")


@pytest.mark.parametrize("kind", [LAC, APS])
@pytest.mark.parametrize("Cn", [10, 300])
def test_acc_does_not_depend_on_the_calls_or_the_outputs(Cn, kind):
    R, Q = 257, 3
    probs, target = case(R, Cn, seed=9)
    qhat = thresholds(probs, target, kind, Q, seed=2)
    want = conformal32(probs, target, kind, qhat)
    one = run_conformal(probs, target, kind, qhat)
    assert same_bits(one["acc"], want["acc"])
    acc = None
    for lo, hi in ((0, 100), (100, 101), (101, R)):          # three calls: the same words
        acc = run_conformal(probs[lo:hi], target[lo:hi], kind, qhat, acc=acc)["acc"]
    assert same_bits(acc, want["acc"])
    bare = run_conformal(probs, target, kind, qhat, outputs=())             # every optional output NULL
    assert list(bare) == ["acc"] and same_bits(bare["acc"], want["acc"])
    blind = run_conformal(probs, None, kind, qhat)                          # no targets: words 1 and 5 untouched
    w = conformal32(probs, None, kind, qhat)
    assert same_bits(blind["acc"], w["acc"]) and all(int(blind["acc"][8 * q + j]) == 0 for q in range(Q) for j in (1, 5))
    for k in ("size", "cut_index", "cut_prob", "member"):
        assert same_bits(blind[k], want[k]), k
    no_acc = run_conformal(probs, target, kind, qhat, with_acc=False)
    assert_equals_restatement(no_acc, want, "acc NULL")
    scores = run_conformal(probs, target, kind, ())                         # Q = 0: the scores and n_nan alone
    assert same_bits(scores["score"], want["score"]) and scores["acc"].tolist() == [0, 0]


def test_argument_checks():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    probs, target = case(4, 5, seed=1)
    pb, td, qd = dev(probs), dev(target), dev(np.array([0.5, 0.7], F32))
    out = torch.full((2, 4), SENTINEL_I, dtype=torch.int32, device="cuda")
    acc = torch.zeros(20, dtype=torch.int64, device="cuda")
    good = dict(probs=_p(pb), ld=5, target=_p(td), R=4, C=5, kind=APS, Q=2, qhat=_p(qd), size=_p(out), acc=_p(acc))
    bad = [dict(kind=2), dict(kind=-1), dict(Q=-1), dict(Q=9), dict(qhat=None), dict(R=0), dict(C=0), dict(ld=4),
           dict(R=1 << 31), dict(target=None, score=_p(out)), dict(target=None, covered=_p(out)), dict(probs=pb.data_ptr() + 2),
           dict(acc=acc.data_ptr() + 4), dict(size=out.data_ptr() + 1), dict(probs=None)]
    for change in bad:
        a = L.ConformalArgs(**{**good, **change})
        with pytest.raises(L.VbnnError):
            L.check(L.lib().vbnn_conformal(Context.get().h, C.byref(a)))
    assert (host(out) == SENTINEL_I).all() and (host(acc) == 0).all()      # nothing written
    L.check(L.lib().vbnn_conformal(Context.get().h, C.byref(L.ConformalArgs(**good))))
    assert (host(out) >= 0).all() and host(acc)[0] == 4


# ------------------------------------------------------------------------------------------------ the engine
def opt_for(Cn, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=784, hidden=[64], n_classes=Cn,
             type="vb", testSamples=4)
    o.update(kw)
    return o


def digits(R, Cn):
    from vbnn_amd import data as D
    d, _ = D.synthetic_digits(R, 1, classes=Cn, seed=3, noise=2.0)
    return dev(d["inputs"].reshape(R, 784)), dev(np.asarray(d["targets"]).astype(np.int32))


class Rows:
    """A slice of a PredictResult, as far as the conformal calls look at one."""
    def __init__(self, probs):
        self.probs = probs


@pytest.mark.parametrize("score", ["aps", "lac"])
def test_engine_sets_cover_their_own_calibration_rows(score):
    from vbnn_amd.engine import ConformalCalibration, ConformalResult, FusedMLP
    R, Cn, levels = 400, 10, (0.5, 0.9, 0.99)
    eng = FusedMLP(opt_for(Cn))
    x, y = digits(R, Cn)
    r = eng.predict(x, targets=y)
    cal = eng.conformal_calibrate(r, y, levels=levels, score=score)
    assert isinstance(cal, ConformalCalibration)
    assert cal.n == R and cal.k == [conformal_rank(R, l) for l in levels] and cal.n_nan == 0 and cal.classes == Cn
    kind = APS if score == "aps" else LAC
    probs, t = host(r.probs), host(y)
    want_scores = conformal32(probs, t, kind)["score"]
    assert same_bits(host(cal.score), want_scores)
    tau, counts = selective32(want_scores, np.zeros(R, np.int32), cal.k)
    assert same_bits(np.array(cal.qhat, F32), tau) and same_bits(host(cal.qhat_dev), tau)
    res = eng.conformal_sets(r, cal, targets=y, members=True)
    assert isinstance(res, ConformalResult)
    want = conformal32(probs, t, kind, tau)
    for k in ("size", "cut_index", "cut_prob", "covered"):
        assert same_bits(host(getattr(res, k)), want[k]), k
    assert same_bits(host(res.members).view(np.uint32), want["member"])
    assert res.counts() == [int(v) for v in want["acc"]]
    d, n_nan = derived(want["acc"], 3)
    for q in range(3):
        covered = res.counts()[8 * q + 1]
        assert covered == int(counts[q][0] + counts[q][2]) >= cal.k[q]       # the n_below + n_tied rows at or below the cut
        assert res.coverage[q] == d[q]["coverage"] == covered / R and res.mean_size[q] == d[q]["mean_size"]
        assert res.singleton_fraction[q] == d[q]["singleton_fraction"] and res.full_fraction[q] == d[q]["full_fraction"]
        assert res.empty_fraction[q] == d[q]["empty_fraction"]
    assert res.n == [R] * 3 and res.n_nan == n_nan == 0
    lists = res.to_lists(1)
    assert [len(l) for l in lists] == want["size"][1].tolist()
    assert all(l == want["order"][i, :len(l)].tolist() for i, l in enumerate(lists))
    # minibatches into one accumulator, and a merge of the pieces: the integers of the one call
    acc, parts = None, []
    for lo, hi in ((0, 130), (130, 131), (131, R)):
        acc = eng.conformal_sets(Rows(r.probs[lo:hi]), cal, targets=y[lo:hi], into=acc)
        parts.append(eng.conformal_sets(Rows(r.probs[lo:hi]), cal, targets=y[lo:hi]))
    assert acc.counts() == res.counts() and torch.equal(acc.size, res.size) and torch.equal(acc.covered, res.covered)
    merged = parts[0].merge(parts[1]).merge(parts[2])
    assert merged.counts() == res.counts() and merged.coverage == res.coverage and torch.equal(merged.size, res.size)
    blind = eng.conformal_sets(r, cal)
    assert blind.covered is None and blind.members is None and all(v != v for v in blind.coverage) and blind.mean_size == res.mean_size
    # a level whose rank is past the calibration set: +inf on the device, every class in every set
    few = eng.conformal_calibrate(Rows(r.probs[:5]), y[:5], levels=(0.5, 0.9), score=score)
    assert few.k == [3, 6] and few.qhat[1] == float("inf")
    assert eng.conformal_sets(r, few).full_fraction[1] == 1.0


def test_engine_accepts_the_other_class_predictives():
    from vbnn_amd.engine import FusedMLP
    R, Cn = 120, 20
    eng = FusedMLP(opt_for(Cn))
    x, y = digits(R, Cn)
    for res in (eng.predict_classes(x, targets=y), eng.predict_analytic(x, targets=y)):
        cal = eng.conformal_calibrate([Rows(res.probs[:50]), Rows(res.probs[50:])], [y[:50], y[50:]], levels=(0.8, 0.95), score="aps")
        assert cal.n == R and cal.k == [97, 115]
        out = eng.conformal_sets(res, cal, targets=y)
        want = conformal32(host(res.probs), host(y), APS, np.array(cal.qhat, F32))
        assert out.counts() == [int(v) for v in want["acc"]] and same_bits(host(out.size), want["size"])
        assert all(out.counts()[8 * q + 1] >= cal.k[q] for q in range(2))
    with pytest.raises(ValueError, match="keep_probs=True"):
        eng.conformal_calibrate(eng.predict_classes(x, targets=y, keep_probs=False), y)
    ten = FusedMLP(opt_for(10))
    with pytest.raises(ValueError, match="20 classes"):
        ten.conformal_sets(ten.predict(x), cal)


def test_trainer_series_appear_only_when_switched_on(tmp_path):
    from vbnn_amd import data as D, train
    trainSet, testSet = D.synthetic_digits(400, 200, classes=10, seed=3, noise=2.0)
    base = dict(hidden=[32], n_classes=10, batchSize=100, testBatchSize=100, trainSize=400, testSize=200, S=2, testSamples=3,
                mode="lrt", dtype="f32", predictive=True, state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3},
                varState={"learningRate": 5e-2})
    off = train.Main(train.default_opt(network_name=str(tmp_path / "off"), **base)).run(trainSet, testSet, epochs=1)[-1]
    assert set(off) == {"devacc", "trainacc", "deverr", "trainerr", "lc", "devacc_pred", "devnll_pred", "dev_mi"}
    on = train.Main(train.default_opt(network_name=str(tmp_path / "on"), conformal_levels=[0.8, 0.95], conformal_score="lac", **base))
    hist = on.run(trainSet, testSet, epochs=2)
    new = {"dev_cov@0.8", "dev_cov@0.95", "dev_set_size@0.8", "dev_set_size@0.95"}
    for rec in hist:
        assert set(rec) == set(off) | new
        assert all(0.0 <= rec[f"dev_cov@{l}"] <= 1.0 and 0.0 <= rec[f"dev_set_size@{l}"] <= 10.0 for l in ("0.8", "0.95"))
        assert rec["dev_cov@0.8"] <= rec["dev_cov@0.95"] and rec["dev_set_size@0.8"] <= rec["dev_set_size@0.95"]
    import os
    from vbnn_amd.logger import read_data
    for k in sorted(new):
        assert len(read_data(os.path.join(str(tmp_path / "on"), k))) == 2, k
    assert not any(f.startswith(("dev_cov@", "dev_set_size@")) for f in os.listdir(str(tmp_path / "off")))
