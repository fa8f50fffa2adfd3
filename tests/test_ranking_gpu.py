"""GPU tests of the rank metrics: vbnn_rank_metrics (include/vbnn_hip.h) called directly on uploaded arrays, and
FusedMLP.ranking / train.py's series over it. Every word of `out` is compared BIT FOR BIT with the integer restatement of
tests/_ranking_np.py (which tests/test_ranking_ref.py holds to the brute-force definitions on the CPU): there are no tolerances.

The sizes straddle every switch of csrc/ranking.hip: the sort and the walk work tiles of 1024 records (R = 1023, 1024, 1025); a
pack tile is 4096 elements, min(64, D rounded up to a power of two) columns wide -- 4096 rows at D = 1 (R = 4095 .. 4097), 1024
at D = 3 and 4, 512 at D = 5 (R = 511 .. 513), 64 at D = 67 (R = 63 .. 65), where the columns also take a second tile (D > 64);
and a pack workgroup walks several row tiles once there are more of them than eight workgroups per compute unit (R = 66000 at
D = 67 on 256 units)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests._ranking_np import F32, SEVEN, derived, n_words, rank_metrics, scores, targets01

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
KINDS = ["distinct", "normal", "seven", "equal", "low_byte", "high_byte", "saturated"]
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2500, 4095, 4096, 4097, 5000]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(a, ld, offset):
    """a (R x D fp32) on the device with row pitch ld, NaN in every pad, its first element `offset` floats past a 16-byte boundary."""
    R, D = a.shape
    buf = torch.full((R * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + R * ld].view(R, ld)[:, :D] = dev(a)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * offset


def run_rank(s, target=None, target_class=None, tau=(), ld=None, ld_t=None, offset=0, calls=1, expect_refusal=False, over=None):
    """vbnn_rank_metrics on NumPy arrays. The workspace is filled with 0xFF bytes and `out` with a guard pattern before the call;
    four guard words follow each. Returns the D lists of 6 + 2 Q Python ints (of the LAST of `calls` calls, all of which must
    agree), or with expect_refusal the status after checking that nothing was written; `over` sets fields of the argument block
    last (what a refusal is provoked with)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    R, D = s.shape
    Q, W = len(tau), n_words(len(tau))
    ld, ld_t = ld or D, ld_t or D
    keep = [padded(s, ld, offset)]
    a = L.RankMetricsArgs(score=keep[0][1], ld=ld, R=R, D=D, Q=Q)
    if target is not None:
        keep.append(padded(np.asarray(target, F32), ld_t, offset))
        a.target, a.ld_t = keep[1][1], ld_t
    if target_class is not None:
        keep.append(dev(np.asarray(target_class, np.int32)))
        a.target_class = _p(keep[-1])
    for q, v in enumerate(tau):
        a.tau[q] = v
    need = C.c_size_t()
    L.check(L.lib().vbnn_rank_metrics_workspace_bytes(R, D, C.byref(need)))
    assert need.value == 16 * R * D
    ws = torch.full((need.value // 8 + 4,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((D * W + 4,), GUARD, dtype=torch.int64, device="cuda")
    a.out, a.workspace, a.workspace_bytes = _p(out), _p(ws), need.value
    for k, v in (over or {}).items():
        setattr(a, k, v)
    if expect_refusal:
        st = L.lib().vbnn_rank_metrics(Context.get().h, C.byref(a))
        torch.cuda.synchronize()
        assert (out == GUARD).all() and (ws == -1).all()
        return st
    got = None
    for _ in range(calls):
        L.check(L.lib().vbnn_rank_metrics(Context.get().h, C.byref(a)))
        torch.cuda.synchronize()
        words = [v & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist()]
        assert words[D * W:] == [GUARD] * 4 and (ws[-4:] == -1).all()
        now = [words[j * W:(j + 1) * W] for j in range(D)]
        assert got is None or got == now
        got = now
    return got


def sprinkle_nan(s, t, seed):
    rng = np.random.default_rng(seed)
    s, t = s.copy(), t.copy()
    s[rng.random(s.shape) < 0.03] = np.nan
    t[rng.random(t.shape) < 0.03] = np.nan
    return s, t


@pytest.mark.parametrize("D", [1, 3, 4, 5, 67])
def test_every_size_and_layout_equals_the_restatement(D):
    tau = (0.5, -0.25)
    for R in SIZES:
        kind = "normal" if R * D <= 40000 else "seven"        # (ties in plenty at the large sizes)
        s, t = sprinkle_nan(scores(kind, R, D, seed=D), targets01(R, D, seed=D), seed=R)
        want = rank_metrics(s, target=t, tau=tau)
        assert run_rank(s, target=t, tau=tau) == want, (R, D, "dense")
        # the layout changes the addresses, never a bit: NaN pads would show in n_nan if they were read
        assert run_rank(s, target=t, tau=tau, ld=D + 3, ld_t=D + 5, offset=1) == want, (R, D, "odd pitch, off the 16-byte boundary")
        if R in (65, 1025):
            assert run_rank(s, target=t, tau=tau, ld=D + 4 - D % 4, ld_t=D + 8 - D % 4) == want, (R, D, "padded, 16-byte rows")


@pytest.mark.parametrize("kind", KINDS)
def test_score_patterns(kind):
    for R, D in ((1025, 3), (2500, 5)):
        s, t = scores(kind, R, D, seed=9), targets01(R, D, seed=9)
        t[:, 0] = 0.0                                        # a column without positives
        t[:, 1] = 1.0                                        # ... and one without negatives
        tau = (0.5, float(s[0, 0]), float(s[R // 2, D - 1]))
        want = rank_metrics(s, target=t, tau=tau)
        assert run_rank(s, target=t, tau=tau, calls=2) == want, (kind, R, D)
        assert want[0][0] == 0 and want[0][3] == 0 and want[1][1] == 0
        sn, tn = sprinkle_nan(s, t, seed=R)
        assert run_rank(sn, target=tn, tau=tau, offset=1) == rank_metrics(sn, target=tn, tau=tau), (kind, R, D, "NaN")


@pytest.mark.parametrize("D", [3, 17])
def test_class_targets(D):
    R = 1500
    s = scores("saturated", R, D, seed=D)
    s[np.random.default_rng(D).random(s.shape) < 0.02] = np.nan
    tc = np.random.default_rng(D + 1).integers(-2, D + 2, R).astype(np.int32)       # out of range on both sides: clamped
    want = rank_metrics(s, target_class=tc, tau=(0.5, 1.0))
    assert run_rank(s, target_class=tc, tau=(0.5, 1.0), ld=D + 1) == want
    onehot = (np.clip(tc, 0, D - 1)[:, None] == np.arange(D)[None, :]).astype(F32)
    assert run_rank(s, target=onehot, tau=(0.5, 1.0)) == want


@pytest.mark.parametrize("Q", [0, 1, 16])
def test_thresholds(Q):
    R, D = 700, 4
    s, t = scores("seven", R, D, seed=Q), targets01(R, D, seed=Q)
    tau = ([float(v) for v in SEVEN] + [float("inf"), float("-inf"), float("nan"), 0.5, 2.0 ** -140, -1.5, 0.75, 1.0, 3.0])[:Q]
    assert len(tau) == Q
    got = run_rank(s, target=t, tau=tau)
    assert got == rank_metrics(s, target=t, tau=tau) and len(got[0]) == 6 + 2 * Q


def test_a_pack_workgroup_walks_several_row_tiles():
    R, D = 66000, 67
    s, t = scores("seven", R, D, seed=1), targets01(R, D, seed=1, p=0.01)
    assert run_rank(s, target=t, tau=(0.5,)) == rank_metrics(s, target=t, tau=(0.5,))


def test_refusals_write_nothing():
    from vbnn_amd.nn import _p
    R, D = 40, 3
    s, t = scores("normal", R, D), targets01(R, D)
    tc = dev(np.zeros(R, np.int32))
    assert run_rank(s, target=t, tau=(0.5,)) == rank_metrics(s, target=t, tau=(0.5,))
    cases = [dict(R=0), dict(D=0), dict(R=-1), dict(R=2 ** 31), dict(R=2 ** 30, D=2, ld=2, ld_t=2), dict(Q=-1), dict(Q=17),
             dict(ld=D - 1), dict(ld_t=D - 1), dict(target_class=_p(tc)), dict(target=None), dict(score=None), dict(out=None),
             dict(workspace=None), dict(workspace_bytes=16 * R * D - 1)]
    for over in cases:
        assert run_rank(s, target=t, tau=(0.5,), expect_refusal=True, over=over) != 0, over
    for field in ("score", "target", "out", "workspace"):
        buf = torch.zeros(64, dtype=torch.int64, device="cuda")
        assert run_rank(s, target=t, expect_refusal=True, over={field: buf.data_ptr() + 2}) != 0, field
    for field in ("out", "workspace"):
        buf = torch.zeros(16 * R * D // 8 + 8, dtype=torch.int64, device="cuda")
        assert run_rank(s, target=t, expect_refusal=True, over={field: buf.data_ptr() + 4}) != 0, field


# ------------------------------------------------------------------------------------------------ engine level
def engine(criterion="bce", D=5):
    from vbnn_amd.engine import FusedMLP
    return FusedMLP(dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=16, hidden=[32],
                         n_classes=D, criterion=criterion, type="vb", testSamples=3, fuse_kl=True, state={"learningRate": 5e-2},
                         meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2}))


def fields(r):
    return (r.words, r.thresholds, r.auroc, r.average_precision, r.tp, r.fp, r.n_defined)


def test_engine_results_lists_micro_and_classes():
    R, D = 300, 5
    eng = engine("bce", D)
    rng = np.random.default_rng(2)
    x = dev(rng.standard_normal((R, 16)).astype(F32))
    t = targets01(R, D, seed=4)
    res = eng.predict_labels(x, targets=dev(t))
    a, b = eng.ranking(res, dev(t), thresholds=(0.5, 0.25)), eng.ranking(res.probs, dev(t), thresholds=(0.5, 0.25))
    assert fields(a) == fields(b)
    probs = res.probs.cpu().numpy()
    want = rank_metrics(probs, target=t, tau=(0.5, 0.25))
    assert a.words == want and a.thresholds == [0.5, 0.25]
    d = [derived(w, 2) for w in want]
    assert a.auroc == [v["auroc"] for v in d] and a.average_precision == [v["average_precision"] for v in d]
    assert a.f1 == [[v["f1"][q] for v in d] for q in range(2)] and a.fpr == [[v["fpr"][q] for v in d] for q in range(2)]
    assert a.macro_auroc == sum(a.auroc) / D and a.n_defined == (D, D) and a.micro_auroc is None
    # a list of minibatches is their concatenation
    cut = [0, 100, 101, 300]
    pieces = [res.probs[i:j] for i, j in zip(cut, cut[1:])]
    c = eng.ranking(pieces, [dev(t[i:j]) for i, j in zip(cut, cut[1:])], thresholds=(0.5, 0.25))
    assert fields(c) == fields(a)
    # micro is the flattened call
    m = eng.ranking(res.probs, dev(t), thresholds=(0.5, 0.25), micro=True)
    flat = eng.ranking(res.probs.reshape(-1, 1), dev(t.reshape(-1, 1)), thresholds=(0.5, 0.25))
    assert fields(m) == fields(a) and m.micro.words == flat.words == rank_metrics(probs.reshape(-1, 1), target=t.reshape(-1, 1), tau=(0.5, 0.25))
    assert m.micro_auroc == flat.auroc[0] and m.micro_average_precision == flat.average_precision[0] and m.micro_tp == [v[0] for v in flat.tp]
    # refusals, by name
    res.probs = None
    for bad, tt, kw in ((res, dev(t), {}), (probs, dev(t), {}), (dev(probs), t, {}), (dev(probs), dev(t[:, :4]), {}),
                        (dev(probs), dev(t.astype(np.float64)), {}), (dev(probs), dev(np.zeros(R, np.int32)), dict(micro=True)),
                        (dev(probs), dev(t), dict(thresholds=[0.1] * 17)), (dev(probs).double(), dev(t), {})):
        with pytest.raises((ValueError, TypeError)):
            eng.ranking(bad, tt, **kw)


def test_engine_one_against_the_rest_equals_the_one_hot_route():
    R, Cn = 257, 7
    eng = engine("nll", Cn)
    x = dev(np.random.default_rng(3).standard_normal((R, 16)).astype(F32))
    tc = np.random.default_rng(4).integers(0, Cn, R).astype(np.int32)
    res = eng.predict(x, targets=dev(tc))
    a = eng.ranking(res, dev(tc))
    onehot = (tc[:, None] == np.arange(Cn)[None, :]).astype(F32)
    b = eng.ranking(res.probs, dev(onehot))
    assert fields(a) == fields(b) and a.words == rank_metrics(res.probs.cpu().numpy(), target_class=tc, tau=(0.5,))


def test_trainer_logs_the_rank_metrics_of_the_whole_dev_set():
    from vbnn_amd.data import synthetic_multilabel
    from vbnn_amd.train import Main, default_opt
    n, D = 96, 3
    train, test = synthetic_multilabel(n, n, D, seed=5, noise=0.3)
    kw = dict(criterion="bce", n_classes=D, hidden=[24], input_size=16, geometry=(1, 16), testBatchSize=32, testSize=n, batchSize=32,
              trainSize=n, testSamples=3, S=2, log=False, predictive=True, var_init=1e-2)
    m = Main(default_opt(ranking=True, **kw))
    seen, inner = [], m.net.predict_labels

    def spy(x, targets=None, **k):
        r = inner(x, targets=targets, **k)
        seen.append((r.probs, targets))
        return r
    m.net.predict_labels = spy
    m.test(test)
    assert set(m.predictive) == {"devll_pred", "dev_label_acc", "dev_exact_match", "dev_label_mi", "dev_auroc", "dev_avg_precision"}
    assert len(seen) == 3
    direct = m.net.ranking(torch.cat([p for p, _ in seen]), torch.cat([t for _, t in seen]))
    assert m.predictive["dev_auroc"] == direct.macro_auroc and m.predictive["dev_avg_precision"] == direct.macro_average_precision
    assert 0.0 <= direct.macro_auroc <= 1.0 and 0.0 < direct.macro_average_precision <= 1.0
    off = Main(default_opt(**kw))                              # off: the series an existing run sees
    off.test(test)
    assert set(off.predictive) == {"devll_pred", "dev_label_acc", "dev_exact_match", "dev_label_mi"}


def test_trainer_ranks_a_class_network_one_against_the_rest():
    from vbnn_amd import data as D, train
    trainSet, testSet = D.synthetic_digits(200, 200, classes=10, seed=3, noise=2.0)
    m = train.Main(train.default_opt(hidden=[32], n_classes=10, batchSize=100, testBatchSize=100, trainSize=200, testSize=200, S=2,
                                     testSamples=3, mode="lrt", dtype="f32", predictive=True, ranking=True, log=False,
                                     state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2}))
    seen, inner = [], m.net.predict

    def spy(x, targets=None, **k):
        r = inner(x, targets=targets, **k)
        seen.append((r.probs, targets))
        return r
    m.net.predict = spy
    m.test(testSet)
    assert set(m.predictive) == {"devacc_pred", "devnll_pred", "dev_mi", "dev_auroc", "dev_avg_precision"}
    assert len(seen) == 2 and seen[0][1].dtype == torch.int32
    direct = m.net.ranking([p for p, _ in seen], [t for _, t in seen])
    assert direct.words == rank_metrics(torch.cat([p for p, _ in seen]).cpu().numpy(),
                                        target_class=torch.cat([t for _, t in seen]).cpu().numpy(), tau=(0.5,))
    assert m.predictive["dev_auroc"] == direct.macro_auroc and m.predictive["dev_avg_precision"] == direct.macro_average_precision
    assert len(direct.auroc) == 10 and 0.0 <= direct.macro_auroc <= 1.0


def test_what_the_label_accuracy_cannot_see():
    """1 % positives: a scorer that ranks every positive above every negative but stays below 0.5, beside a constant one. At the
    threshold 0.5 their hit counts are the same; the AUROC is exactly 1 against exactly 0.5."""
    R = 2000
    eng = engine("bce", 2)
    t = np.zeros((R, 2), F32)
    t[np.random.default_rng(8).choice(R, R // 100, replace=False)] = 1.0
    s = np.empty((R, 2), F32)
    s[:, 0] = np.where(t[:, 0] > 0.5, 0.4, 0.1) + np.random.default_rng(9).random(R).astype(F32) * F32(0.05)
    s[:, 1] = 0.2
    r = eng.ranking(dev(s), dev(t))
    assert r.n_pos == [R // 100] * 2 and r.tp == [[0, 0]] and r.fp == [[0, 0]]          # the same 99 % label accuracy
    assert r.auroc == [1.0, 0.5] and r.average_precision[0] == 1.0
    assert math.isclose(r.average_precision[1], 0.01, abs_tol=2.0 ** -32) and r.average_precision[1] <= 0.01
