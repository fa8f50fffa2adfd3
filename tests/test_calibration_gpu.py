"""GPU tests of classifier calibration and selective prediction: vbnn_predict_calibration and vbnn_selective
(include/vbnn_hip.h) called directly on uploaded arrays, and FusedMLP.calibration / FusedMLP.selective / train.py's series over
them. Everything is compared BIT FOR BIT with the fp32 / integer restatement of tests/_calibration_np.py (which
tests/test_calibration_ref.py holds to the float64 definition on the CPU): there are no tolerances here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests._calibration_np import F32, calibration32, derived, ranks, selective32, selective_accuracy, softmax_case

pytestmark = pytest.mark.gpu

ROW_KEYS = ("conf", "hit", "brier", "bin")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_calibration(probs, pred, target, M, ld=None, offset=0, outputs=True, acc=None):
    """vbnn_predict_calibration on NumPy arrays: probs with row pitch ld (NaN in every pad column), its first element `offset`
    floats past a 16-byte boundary; acc: the accumulator's words before the call (zero without). Returns the row outputs (NaN /
    -7 where the call wrote nothing) and acc as uint64."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    R, Cn = probs.shape
    ld = ld or Cn
    buf = torch.full((R * ld + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:offset + R * ld].view(R, ld)[:, :Cn] = dev(probs)
    assert buf.data_ptr() % 16 == 0
    out = dict(conf=torch.full((R,), float("nan"), dtype=torch.float32, device="cuda"),
               hit=torch.full((R,), -7, dtype=torch.int32, device="cuda"),
               brier=torch.full((R,), float("nan"), dtype=torch.float32, device="cuda"),
               bin=torch.full((R,), -7, dtype=torch.int32, device="cuda")) if outputs else {}
    accd = dev(np.zeros(3 * M + 4, np.uint64).view(np.int64) if acc is None else acc.view(np.int64))
    pd, td = dev(pred), dev(target)
    a = L.CalibrationArgs(probs=buf.data_ptr() + 4 * offset, ld=ld, pred=_p(pd), target=_p(td), R=R, C=Cn, bins=M,
                          conf=_p(out.get("conf")), hit=_p(out.get("hit")), brier=_p(out.get("brier")), bin=_p(out.get("bin")),
                          acc=_p(accd))
    L.check(L.lib().vbnn_predict_calibration(Context.get().h, C.byref(a)))
    got = {k: host(v) for k, v in out.items()}
    got["acc"] = host(accd).view(np.uint64)
    return got


def assert_equals_restatement(got, want, what):
    for k in got:
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])


@pytest.mark.parametrize("Cn", [2, 3, 10, 16, 17, 255, 256, 257, 1000, 4099])
def test_kernel_equals_the_restatement_in_every_layout(Cn):
    M = 15
    for R in (1, 3, 5, 64, 257):
        probs, pred, target = softmax_case(R, Cn, seed=Cn + R, scale=2.0 if Cn < 1000 else 4.0)
        want = calibration32(probs, pred, target, M)
        dense = run_calibration(probs, pred, target, M)
        assert_equals_restatement(dense, want, (Cn, R, "dense"))
        assert int(dense["acc"][3 * M + 1]) == R and int(dense["acc"][3 * M + 3]) == 0
        # the layout changes the access path, never a bit: NaN pads are not read; a base off the 16-byte boundary goes scalar
        assert_equals_restatement(run_calibration(probs, pred, target, M, ld=Cn + 4 - Cn % 4 + 4), want, (Cn, R, "padded, 16-byte rows"))
        assert_equals_restatement(run_calibration(probs, pred, target, M, ld=Cn + 3), want, (Cn, R, "odd pitch"))
        assert_equals_restatement(run_calibration(probs, pred, target, M, offset=1), want, (Cn, R, "off the 16-byte boundary"))


@pytest.mark.parametrize("M", [1, 2, 15, 64])
def test_bin_counts(M):
    probs, pred, target = softmax_case(257, 10, seed=M)
    got, want = run_calibration(probs, pred, target, M), calibration32(probs, pred, target, M)
    assert_equals_restatement(got, want, M)
    d = derived(got["acc"], M)
    assert d["count"].sum() == 257 and 0.0 <= d["ece"] <= 1.0 and 0.0 <= d["brier"] <= 2.0 and d["ece"] <= d["mce"] + 1e-15


def test_every_row_in_one_bin():
    """A confident classifier: every workgroup adds to the last bin's words, and the sums are still exact."""
    R, Cn, M = 1031, 10, 15
    rng = np.random.default_rng(4)
    probs = np.full((R, Cn), 0.004, F32)
    pred = rng.integers(0, Cn, R).astype(np.int32)
    probs[np.arange(R), pred] = (0.95 + 0.01 * rng.random(R)).astype(F32)
    target = np.where(rng.random(R) < 0.9, pred, (pred + 1) % Cn).astype(np.int32)
    got, want = run_calibration(probs, pred, target, M), calibration32(probs, pred, target, M)
    assert_equals_restatement(got, want, "one bin")
    assert int(got["acc"][M - 1]) == R and got["acc"][:M - 1].sum() == 0 and (got["bin"] == M - 1).all()


def test_a_nan_row_between_clean_rows():
    R, Cn, M = 9, 20, 15
    probs, pred, target = softmax_case(R, Cn)
    clean = run_calibration(probs, pred, target, M)
    bad = probs.copy()
    col = next(c for c in range(Cn) if c not in (pred[4], target[4]))
    bad[4, col] = np.nan                                     # neither the predicted class nor the target: ss alone shows it
    got = run_calibration(bad, pred, target, M)
    assert_equals_restatement(got, calibration32(bad, pred, target, M), "NaN row")
    keep = np.arange(R) != 4
    for k in ROW_KEYS:
        assert same_bits(got[k][keep], clean[k][keep]), k
    assert np.isnan(got["conf"][4]) and np.isnan(got["brier"][4]) and got["hit"][4] == -1 and got["bin"][4] == -1
    assert int(got["acc"][3 * M + 1]) == R - 1 and int(got["acc"][3 * M + 2]) == 1


def test_out_of_range_classes_null_outputs_and_halves():
    R, Cn, M = 257, 17, 15
    probs, pred, target = softmax_case(R, Cn, seed=9)
    pred[0], pred[1], target[2], target[3] = -7, 99, -1, Cn
    want = calibration32(probs, pred, target, M)
    one = run_calibration(probs, pred, target, M)
    assert_equals_restatement(one, want, "clamped")
    assert_equals_restatement(one, run_calibration(probs, np.clip(pred, 0, Cn - 1), np.clip(target, 0, Cn - 1), M), "clamp")
    bare = run_calibration(probs, pred, target, M, outputs=False)             # every optional output NULL
    assert list(bare) == ["acc"] and same_bits(bare["acc"], want["acc"])
    h = 100                                                                     # two calls on halves: the same words
    first = run_calibration(probs[:h], pred[:h], target[:h], M)["acc"]
    both = run_calibration(probs[h:], pred[h:], target[h:], M, acc=first)["acc"]
    assert same_bits(both, want["acc"])


def test_calibration_argument_checks():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    probs, pred, target = softmax_case(4, 5)
    pb, pd, td, acc = dev(probs), dev(pred), dev(target), torch.zeros(3 * 64 + 8, dtype=torch.int64, device="cuda")
    for M in (0, 65):
        a = L.CalibrationArgs(probs=_p(pb), ld=5, pred=_p(pd), target=_p(td), R=4, C=5, bins=M, acc=_p(acc))
        with pytest.raises(L.VbnnError, match="bins"):
            L.check(L.lib().vbnn_predict_calibration(Context.get().h, C.byref(a)))
    a = L.CalibrationArgs(probs=_p(pb), ld=4, pred=_p(pd), target=_p(td), R=4, C=5, bins=4, acc=_p(acc))
    with pytest.raises(L.VbnnError, match="ld"):
        L.check(L.lib().vbnn_predict_calibration(Context.get().h, C.byref(a)))
    a = L.CalibrationArgs(probs=_p(pb), ld=5, pred=_p(pd), target=None, R=4, C=5, bins=4, acc=_p(acc))
    with pytest.raises(L.VbnnError, match="null"):
        L.check(L.lib().vbnn_predict_calibration(Context.get().h, C.byref(a)))
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0                          # a refused call adds nothing


# ------------------------------------------------------------------------------------------------ selective
def run_selective(score, hit, ks):
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    Q = len(ks)
    sd, hd = dev(score), dev(hit)
    tau = torch.full((Q,), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((Q, 4), -1, dtype=torch.int64, device="cuda")
    a = L.SelectiveArgs(score=_p(sd), hit=_p(hd), R=score.size, Q=Q, tau=_p(tau), counts=_p(counts))
    for j, k in enumerate(ks):
        a.k[j] = k
    L.check(L.lib().vbnn_selective(Context.get().h, C.byref(a)))
    return host(tau), host(counts).view(np.uint64)


def assert_selective(score, hit, ks, what):
    tau, counts = run_selective(score, hit, ks)
    wtau, wcounts = selective32(score, hit, ks)
    assert same_bits(tau, wtau), (what, tau, wtau)
    assert same_bits(counts, wcounts), (what, counts, wcounts)
    return tau, counts


def special_scores(R, rng):
    """Entropy-like scores with duplicates, both signs, both zeros, both infinities and NaNs (of both signs) mixed in."""
    s = (rng.integers(-30, 30, R).astype(F32) / F32(7)).astype(F32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45], F32)
    idx = rng.random(R) < 0.25
    s[idx] = specials[rng.integers(0, specials.size, int(idx.sum()))]
    bits = s.view(np.uint32)
    neg = np.isnan(s) & (rng.random(R) < 0.5)
    bits[neg] = 0xFFC00123                                   # a negative NaN with a payload: still ranks last
    if R >= 16:                                              # every special value at least once
        s[:specials.size] = specials
        bits[specials.size] = 0xFFC00123
    return s


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 1000, 5000])
def test_selective_equals_the_restatement(R):
    rng = np.random.default_rng(R)
    hit = (rng.random(R) < 0.6).astype(np.int32) * rng.integers(1, 5, R).astype(np.int32)      # any nonzero value is a hit
    mid = (R + 1) // 2
    for name, score in (("normal", rng.standard_normal(R).astype(F32)), ("specials", special_scores(R, rng)),
                        ("equal", np.full(R, 0.0, F32)), ("two values", np.where(np.arange(R) % 3 == 0, F32(-1.5), F32(2.0)).astype(F32))):
        for k in (1, mid, R):                                # Q = 1
            assert_selective(score, hit, [k], (R, name, k))
        ks = [max(1, min(R, int(round(j * R / 31)))) for j in range(32)]         # Q = 32, repeats and any order allowed
        ks[5], ks[20] = ks[20], ks[5]
        tau, counts = assert_selective(score, hit, ks, (R, name, "Q = 32"))
        if name == "equal":                                  # ties are shared out: the overall accuracy at every rank
            assert all(abs(a - (hit != 0).mean()) <= 1e-15 for a in selective_accuracy(counts, ks))
        if name == "two values" and R >= 63:                 # duplicates straddling tau
            nb, _, nt, _ = (int(v) for v in run_selective(score, hit, [mid])[1][0])
            assert nb < mid < nb + nt or nb + nt == mid


def test_selective_argument_checks():
    from vbnn_amd import _lib as L
    s, h = np.zeros(4, F32), np.ones(4, np.int32)
    for ks in ([0], [5]):
        with pytest.raises(L.VbnnError, match="k outside"):
            run_selective(s, h, ks)


# ------------------------------------------------------------------------------------------------ engine level
def opt_for(Cn, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=8, hidden=[16, 16], n_classes=Cn,
             type="vb", testSamples=4)
    o.update(kw)
    return o


def engine_data(oracle, R, Cn):
    return dev(oracle.fill_normal(R, 8, 3, 4, 0, 0)), dev((np.arange(R) * 7 % Cn).astype(np.int32))


def result_of(eng, how, x, t, **kw):
    if how == "predict":
        return eng.predict(x, targets=t, **kw)
    if how == "predict_classes":
        return eng.predict_classes(x, targets=t, **kw)
    return eng.predict_analytic(x, targets=t)


@pytest.mark.parametrize("how,Cn", [("predict", 10), ("predict_classes", 40), ("predict_analytic", 40)])
def test_engine_calibration_equals_the_restatement(oracle, how, Cn):
    from vbnn_amd.engine import CalibrationResult, FusedMLP
    R, M = 90, 15
    eng = FusedMLP(opt_for(Cn))
    x, t = engine_data(oracle, R, Cn)
    res = result_of(eng, how, x, t)
    cal = eng.calibration(res, t)
    assert isinstance(cal, CalibrationResult) and cal.bins == M
    want = calibration32(host(res.probs), host(res.pred), host(t), M)
    assert cal.counts() == [int(v) for v in want["acc"]]
    assert same_bits(host(cal.conf), want["conf"]) and same_bits(host(cal.hit), want["hit"])
    assert torch.equal(cal.entropy, res.entropy) and torch.equal(cal.mutual_info, res.mutual_info)
    d = derived(want["acc"], M)
    assert (cal.ece, cal.mce, cal.brier, cal.accuracy, cal.n, cal.n_nan) == (d["ece"], d["mce"], d["brier"], d["accuracy"], R, 0)
    assert abs(100.0 * cal.accuracy - res.accuracy) <= 1e-9 and 0.0 <= cal.ece <= 1.0 and 0.0 <= cal.brier <= 2.0
    assert cal.bin_count == [int(v) for v in d["count"]] and cal.bin_hits == [int(v) for v in d["hits"]]
    # into= over three minibatches: the integers of one call on their concatenation; merge() adds on the host
    acc, parts = None, []
    for lo, hi in ((0, 30), (30, 47), (47, 90)):
        sub = type(res)(res.probs[lo:hi], None, res.entropy[lo:hi], None, res.mutual_info[lo:hi], res.pred[lo:hi])
        acc = eng.calibration(sub, t[lo:hi], into=acc)
        parts.append(eng.calibration(sub, t[lo:hi]))
    assert acc.counts() == cal.counts() and torch.equal(acc.conf, cal.conf) and torch.equal(acc.hit, cal.hit)
    assert torch.equal(acc.entropy, cal.entropy)
    merged = parts[0].merge(parts[1]).merge(parts[2])
    assert merged.counts() == cal.counts() and merged.ece == cal.ece and torch.equal(merged.conf, cal.conf)
    # selective by entropy: the restatement's integers, and full coverage is the accuracy
    covs = [0.1, 0.5, 0.9, 1.0]
    sel = eng.selective(cal.entropy, cal.hit, covs)
    ks = ranks(covs, R)
    wtau, wcounts = selective32(host(cal.entropy), want["hit"], ks)
    assert sel.k == ks and sel.counts == wcounts.astype(np.int64).tolist() and same_bits(np.array(sel.threshold, F32), wtau)
    assert sel.accuracy == selective_accuracy(wcounts, ks) and abs(sel.accuracy[-1] - cal.accuracy) <= 1e-15
    with pytest.raises(ValueError, match="bins"):
        eng.calibration(res, t, bins=65)
    with pytest.raises(ValueError, match="into"):
        eng.calibration(res, t, bins=10, into=cal)
    with pytest.raises(ValueError, match="coverages"):
        eng.selective(cal.entropy, cal.hit, [0.0])


def test_keep_probs_false_is_refused_and_map_ties_give_the_overall_accuracy(oracle):
    from vbnn_amd.engine import FusedMLP
    R, Cn = 90, 40
    eng = FusedMLP(opt_for(Cn))
    x, t = engine_data(oracle, R, Cn)
    with pytest.raises(ValueError, match="keep_probs=True"):
        eng.calibration(eng.predict_classes(x, targets=t, keep_probs=False), t)
    res = eng.predict_classes(x, targets=t, map=True)
    cal = eng.calibration(res, t)
    assert float(cal.mutual_info.abs().max()) == 0.0         # one pass on the means: no epistemic part on any row
    sel = eng.selective(cal.mutual_info, cal.hit, [0.05, 0.3, 1.0])
    assert all(c == [0, 0, R, round(cal.accuracy * R)] for c in sel.counts)
    assert all(abs(a - cal.accuracy) <= 1e-15 for a in sel.accuracy)


def test_trainer_logs_the_calibration_series(tmp_path):
    from vbnn_amd import data as D, train
    trainSet, testSet = D.synthetic_digits(400, 200, classes=10, seed=3, noise=2.0)
    base = dict(hidden=[32], n_classes=10, batchSize=100, testBatchSize=100, trainSize=400, testSize=200, S=2, testSamples=3,
                mode="lrt", dtype="f32", predictive=True, state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3},
                varState={"learningRate": 5e-2})
    off = train.Main(train.default_opt(network_name=str(tmp_path / "off"), **base)).run(trainSet, testSet, epochs=1)[-1]
    assert set(off) == {"devacc", "trainacc", "deverr", "trainerr", "lc", "devacc_pred", "devnll_pred", "dev_mi"}
    on = train.Main(train.default_opt(network_name=str(tmp_path / "on"), calibration_bins=10, selective_coverages=[0.5, 1.0], **base))
    hist = on.run(trainSet, testSet, epochs=3)
    new = {"dev_ece", "dev_mce", "dev_brier", "dev_acc@cov0.5", "dev_acc@cov1"}
    for rec in hist:
        assert set(rec) == set(off) | new
        assert all(math.isfinite(rec[k]) for k in new)
        assert 0.0 <= rec["dev_ece"] <= 1.0 and 0.0 <= rec["dev_brier"] <= 2.0 and rec["dev_ece"] <= rec["dev_mce"] + 1e-15
        assert abs(100.0 * rec["dev_acc@cov1"] - rec["devacc_pred"]) <= 1e-9
    from vbnn_amd.logger import read_data
    import os
    for k in sorted(new):
        assert len(read_data(os.path.join(str(tmp_path / "on"), k))) == 3, k
    assert not any(f.startswith(("dev_ece", "dev_acc@cov")) for f in os.listdir(str(tmp_path / "off")))
