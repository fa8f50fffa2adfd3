"""vbnn_top_rows through the C ABI and FusedMLP.top_rows / acquire / active_learning on the device, against the NumPy
restatement of tests/_acquire_np.py (itself held to a plain sort and to the C oracle's det_logf by test_acquire_ref.py).
Everything is compared bit for bit: index, value, key, the four counts, and the guard words before and after every output.

Rules of the kernel-level cases. Every output is a run of bytes inside an allocation filled with 0xA5, 64 guard bytes either side,
compared WHOLE against an expectation that starts as the sentinel. Every case runs twice -- first on a workspace full of the
sentinel (it needs no preparation), then on the workspace the first run left -- and both runs must give the expected bits. The
score pointer sits on a 16-byte boundary or 4 bytes past one (the 16-byte and the 4-byte load paths)."""
import ctypes as C

import numpy as np
import pytest

from tests import _acquire_np as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
SB, GUARD = 0xA5, 64
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097, 70001, 300007)     # the last two: several workgroups, a ragged tail
SEED = 0x0123456789ABCDEF


def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, L.lib(), nn.Context.get().h


class Out:
    """n elements of itemsize bytes between two guards, all 0xA5 before the launch."""

    def __init__(self, n, itemsize):
        self.nbytes = n * itemsize
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), SB, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def expect(self, payload):
        want = np.full(GUARD + self.nbytes + GUARD, SB, np.uint8)
        want[GUARD:GUARD + self.nbytes] = np.ascontiguousarray(payload).view(np.uint8)
        return np.array_equal(self.raw.cpu().numpy(), want)


class Score:
    """The scores on the device, `off` floats past a 256-byte boundary."""

    def __init__(self, s, off):
        words = np.zeros(len(s) + off + 4, np.int32)                  # (uploaded as integers: every NaN payload arrives as it is)
        words[off:off + len(s)] = np.ascontiguousarray(s, F32).view(np.int32)
        self.raw = torch.from_numpy(words).cuda()
        self.ptr = C.c_void_p(self.raw.data_ptr() + 4 * off)
        assert (self.raw.data_ptr() + 4 * off) % 16 == (4 * off) % 16


_WS = {}


def _workspace(L, lib, R, k, fresh):
    n = C.c_size_t()
    assert lib.vbnn_top_rows_workspace_bytes(R, k, C.byref(n)) == 0
    if fresh or "ws" not in _WS or _WS["ws"].numel() < n.value + 16:
        _WS["ws"] = torch.full((n.value + 16,), SB, dtype=torch.uint8, device="cuda")
    return _WS["ws"], n.value


def launch(score_ptr, exclude, R, k, largest, beta=None, draw=0, row0=0, fresh=True, with_key=True, ws_bytes=None, ws_off=0):
    """One call: (status, index, value, key, counts) with the four outputs as Out."""
    L, lib, ctx = _ctx()
    ws, need = _workspace(L, lib, max(R, 1), min(max(k, 1), 4096), fresh)
    index, value, key, counts = Out(max(k, 1), 4), Out(max(k, 1), 4), Out(max(k, 1), 4), Out(4, 8)
    a = L.TopRowsArgs(score=score_ptr, exclude=None if exclude is None else C.c_void_p(exclude.data_ptr()), R=R, k=k,
                      largest=int(largest), stochastic=int(beta is not None), beta=0.0 if beta is None else beta, seed=SEED,
                      draw=draw, row0=row0, index=index.ptr, value=value.ptr, key=key.ptr if with_key else None,
                      counts=counts.ptr, workspace=C.c_void_p(ws.data_ptr() + ws_off), workspace_bytes=need if ws_bytes is None else ws_bytes)
    st = lib.vbnn_top_rows(ctx, C.byref(a))
    torch.cuda.synchronize()
    return st, index, value, key, counts


def expected(full, k):
    """The contract's outputs for k from the restatement's full ordering (index, value bits, key bits, counts of k = all)."""
    index, value, key, counts = full
    n = min(k, counts[1])
    ei, ev, ek = np.full(k, -1, np.int32), np.full(k, A.QNAN, np.uint32), np.full(k, A.QNAN, np.uint32)
    ei[:n], ev[:n], ek[:n] = index[:n], value[:n], key[:n]
    return ei, ev, ek, np.array([n, counts[1], counts[2], counts[3]], np.int64)


def check(score_ptr, exclude, R, k, largest, full, label, **kw):
    want = expected(full, k)
    for run in (0, 1):
        st, index, value, key, counts = launch(score_ptr, exclude, R, k, largest, fresh=run == 0, **kw)
        assert st == 0, label
        for out, w, what in zip((index, value, key, counts), want, ("index", "value", "key", "counts")):
            assert out.expect(w), f"{label}, run {run}: {what} (or its guards)"


def ks_for(R, n_cand):
    ks = {1, 2, 7, 64, 4096, R, R - 1, n_cand + 3}
    return sorted(k for k in ks if 1 <= k <= 4096 and (k <= R + 3))


# ------------------------------------------------------------------------------------------------ kernel level: deterministic
@pytest.mark.parametrize("name", ["normal", "equal", "two_values", "small_ints", "ascending", "descending", "low_bits", "top_bits",
                                  "specials"])
def test_top_rows_is_the_restatement_bit_for_bit(name):
    n_case = 0
    for R in SIZES:
        s = A.population(name, R)
        scores = {off: Score(s, off) for off in (0, 1)}
        for ex in ("none", "half", "all", "all_but_one"):
            e = A.exclusion(ex, R)
            e_dev = None if e is None else torch.from_numpy(e).cuda()
            for largest in ((True, False) if ex == "none" else (R % 2 == 0,)):
                full = A.top_rows(s, R, largest, e)
                ks = ks_for(R, full[3][1])
                for k in (ks if ex == "none" else [k for k in ks if k in (1, 7, ks[-1])]):
                    n_case += 1
                    off = n_case % 2
                    check(scores[off].ptr, e_dev, R, k, largest, full, f"{name} R={R} k={k} largest={largest} exclude={ex} off={off}")
    print(f"{name}: {n_case} cases, each run twice")


def test_the_tie_rule_across_workgroup_boundaries():
    """Mass ties whose wanted part ends in a LATER workgroup: 0 .. 15 repeated, the k-th row deep inside the run of one value."""
    R = 300007
    s = (np.arange(R) % 16).astype(F32)
    sc = Score(s, 0)
    for largest in (True, False):
        full = A.top_rows(s, R, largest, None)
        for k in (1, 2, 64, 4096):
            check(sc.ptr, None, R, k, largest, full, f"ties R={R} k={k} largest={largest}")
    s = np.zeros(R, F32)
    s[70000:] = 1.0                                                   # largest: every tied row wanted lies in a later workgroup than the first
    sc = Score(s, 1)
    full = A.top_rows(s, R, True, None)
    assert full[0][0] == 70000
    check(sc.ptr, None, R, 4096, True, full, "ties that begin late")
    e = np.zeros(R, np.uint8)
    e[70000:299000] = 1                                               # ... and with most of them excluded
    full = A.top_rows(s, R, True, e)
    check(sc.ptr, torch.from_numpy(e).cuda(), R, 4096, True, full, "ties that begin late, excluded")


def test_key_is_optional_and_exclude_may_be_misaligned():
    R = 4097
    s = A.population("specials", R)
    sc = Score(s, 0)
    e = A.exclusion("half", R)
    raw = torch.zeros(R + 8, dtype=torch.uint8, device="cuda")
    raw[1:1 + R] = torch.from_numpy(e).cuda()
    full = A.top_rows(s, R, True, e)
    check(sc.ptr, raw[1:], R, 64, True, full, "exclude one byte past a boundary")
    want = expected(full, 64)
    st, index, value, key, counts = launch(sc.ptr, raw[1:], R, 64, True, with_key=False)
    assert st == 0 and index.expect(want[0]) and value.expect(want[1]) and counts.expect(want[3])
    assert key.expect(np.full(64 * 4, SB, np.uint8)), "key = NULL: nothing may be written there"


# ------------------------------------------------------------------------------------------------ kernel level: stochastic
@pytest.mark.parametrize("beta", [0.5, 1.0, 4.0])
def test_stochastic_keys_are_the_restatement_bit_for_bit(beta):
    n_case = 0
    for R in (1, 65, 1023, 4097, 70001):
        s = A.population("positive", R) * F32(3.0)
        rs = np.random.RandomState(R)
        odd = A.floats(np.array([0, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF, 0x7F800000, 0x7FC00000, 0xFFC00001,
                                 0x7F7FFFFF, 0x00800000], np.uint32))
        where = rs.rand(R) < 0.2
        s[where] = odd[rs.randint(0, len(odd), int(where.sum()))]
        for row0 in (0, 7, 2 ** 31):
            for ex in ("none", "half"):
                e = A.exclusion(ex, R)
                e_dev = None if e is None else torch.from_numpy(e).cuda()
                for score in (s, None):
                    n_case += 1
                    off = n_case % 2
                    sc = Score(s, off) if score is not None else None
                    draw = 3 + n_case
                    full = A.top_rows(score, min(R, 4096), True, e, R=R, beta=beta, seed=SEED, draw=draw, row0=row0)
                    for k in sorted({1, 7, 64, min(R, 4096)} & set(range(1, R + 1))):
                        check(sc.ptr if sc else None, e_dev, R, k, True, full,
                              f"beta={beta} R={R} k={k} row0={row0} exclude={ex} score={'given' if sc else 'NULL'} off={off}",
                              beta=beta, draw=draw, row0=row0)
    print(f"beta {beta}: {n_case} cases")


def test_a_workspace_off_the_16_byte_boundary():
    """The stored stochastic keys then take 4-byte stores and loads."""
    R = 70001
    s = A.population("specials", R)
    e = A.exclusion("half", R)
    sc = Score(s, 0)
    full = A.top_rows(s, 4096, True, e, beta=1.0, seed=SEED, draw=2, row0=5)
    check(sc.ptr, torch.from_numpy(e).cuda(), R, 4096, True, full, "workspace 4 bytes past a boundary", beta=1.0, draw=2, row0=5,
          ws_off=4)
    check(sc.ptr, None, R, 64, False, A.top_rows(s, 64, False, None), "the same, deterministic", ws_off=12)


def test_stochastic_keys_of_a_pool_scored_in_pieces():
    R, cut = 70001, 30001
    s = A.population("positive", R)
    whole = A.top_rows(s, 4096, True, None, beta=1.0, seed=SEED, draw=5, row0=11)
    a = A.top_rows(s[:cut], 4096, True, None, beta=1.0, seed=SEED, draw=5, row0=11)
    b = A.top_rows(s[cut:], 4096, True, None, beta=1.0, seed=SEED, draw=5, row0=11 + cut)
    sa, sb = Score(s[:cut], 0), Score(s[cut:], 1)
    check(sa.ptr, None, cut, 4096, True, a, "first piece", beta=1.0, draw=5, row0=11)
    check(sb.ptr, None, R - cut, 4096, True, b, "second piece", beta=1.0, draw=5, row0=11 + cut)
    keys = dict(zip(a[0].tolist(), a[2].tolist()))
    keys.update(zip((b[0] + cut).tolist(), b[2].tolist()))
    assert all(keys[i] == kk for i, kk in zip(whole[0].tolist(), whole[2].tolist()) if i in keys)
    assert set(whole[0][:100].tolist()) <= set(keys)                  # the whole pool's best rows are the pieces' best rows


# ------------------------------------------------------------------------------------------------ kernel level: refusals
def test_every_refusal_writes_nothing():
    L, lib, ctx = _ctx()
    s = A.population("normal", 100)
    sc = Score(s, 0)
    cases = [dict(R=100, k=0), dict(R=100, k=4097), dict(R=0, k=1), dict(R=100, k=5, beta=0.0), dict(R=100, k=5, beta=-1.0),
             dict(R=100, k=5, beta=float("inf")), dict(R=100, k=5, beta=float("nan")), dict(R=100, k=5, beta=1.0, largest=False),
             dict(R=100, k=5, ws_bytes=1024), dict(R=100, k=5, beta=1.0, row0=2 ** 32 - 99), dict(R=100, k=5, score=None)]
    for c in cases:
        st, index, value, key, counts = launch(c.get("score", sc.ptr), None, c["R"], c["k"], c.get("largest", True),
                                               beta=c.get("beta"), row0=c.get("row0", 0), ws_bytes=c.get("ws_bytes"))
        assert st != 0 and len(lib.vbnn_last_error()) > 0, c
        for out in (index, value, key, counts):
            assert out.expect(np.full(out.nbytes, SB, np.uint8)), c
    st, *_ = launch(sc.ptr, None, 100, 5, True, beta=1.0, row0=2 ** 32 - 100)          # the last legal row0
    assert st == 0


# ------------------------------------------------------------------------------------------------ engine level
R_POOL = 37


def opt_for(criterion, n_classes, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=5, input_size=20, hidden=[16, 12],
             n_classes=n_classes, type="vb", testSamples=4, criterion=criterion)
    o.update(kw)
    return o


CRITERIA = {"nll": 5, "bce": 3, "mse": 2, "gauss": 4}


def pool(oracle):
    return torch.from_numpy(oracle.fill_normal(R_POOL, 20, 7, 4, 0, 0)).cuda()


def vector_of(name, criterion, pred):
    if name == "least_confidence":
        return 1.0 - pred.topk_prob[:, 0]
    if name == "margin":
        return pred.topk_prob[:, 1] - pred.topk_prob[:, 0]
    if name == "total_variance":
        return pred.row_var + pred.row_noise_var
    if name == "variance":
        return pred.row_var
    if criterion == "bce":
        return pred.row_mutual_info if name == "mutual_info" else pred.row_entropy
    return pred.mutual_info if name == "mutual_info" else pred.entropy


def twin_predictive(twin, criterion, x, analytic=False, **kw):
    if analytic:
        return twin.predict_analytic(x, topk=2, keep_probs=False) if criterion == "nll" else twin.predict_analytic(x)
    if criterion == "nll":
        return twin.predict_classes(x, topk=2, keep_probs=False, **kw)
    return twin.predict_labels(x, **kw) if criterion == "bce" else twin.predict_regression(x, **kw)


def same(res, want):
    index, value, key, counts = want
    return (np.array_equal(res.indices.cpu().numpy(), index) and np.array_equal(A.bits(res.values.cpu().numpy()), value)
            and np.array_equal(A.bits(res.keys.cpu().numpy()), key)
            and [res.n_selected, res.n_candidates, res.n_nan, res.n_excluded] == counts)


@pytest.mark.parametrize("criterion", list(CRITERIA))
def test_acquire_is_top_rows_of_the_predictives_own_vector(oracle, criterion):
    from vbnn_amd.acquisition import SCORES
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    e = A.exclusion("half", R_POOL, seed=3)
    e_dev = torch.from_numpy(e).cuda()
    for name in SCORES[criterion]:
        eng, twin = FusedMLP(opt_for(criterion, CRITERIA[criterion])), FusedMLP(opt_for(criterion, CRITERIA[criterion]))
        if name == "random":
            res = eng.acquire(x, 9, score="random", exclude=e_dev.bool())
            assert eng.draw == 1 and res.predictive is None and res.score_name == "random"
            assert same(res, A.top_rows(None, 9, True, e, R=R_POOL, beta=1.0, seed=5, draw=1, row0=0))
            continue
        res = eng.acquire(x, 9, score=name, exclude=e_dev)
        pred = twin_predictive(twin, criterion, x)
        vec = vector_of(name, criterion, pred).cpu().numpy()
        assert same(res, A.top_rows(vec, 9, True, e)), name
        assert eng.draw == twin.draw == 4 and res.S == 4 and res.score_name == name and res.chunks == 1
        assert not e[res.indices.cpu().numpy()].any() and res.n_excluded == int((e != 0).sum())
        # chunked: the same bits; stochastic: draw self.draw + 1 after the predictive's, consumed; repeatable from the counters
        small = FusedMLP(opt_for(criterion, CRITERIA[criterion], predict_rows=3 * 4))
        r3 = small.acquire(x, 9, score=name, exclude=e_dev)
        assert r3.chunks > 1 and same(r3, A.top_rows(vec, 9, True, e)), name
        eng.draw = twin.draw = 0
        if name == "margin":                                          # never positive: score^beta would weigh every row 0
            with pytest.raises(ValueError, match="least_confidence"):
                eng.acquire(x, 9, score=name, beta=2.0)
            assert eng.draw == 0
            continue
        r1 = eng.acquire(x, 9, score=name, beta=2.0, row0=100)
        pred = twin_predictive(twin, criterion, x, row0=100)
        vec = vector_of(name, criterion, pred).cpu().numpy()
        assert eng.draw == 5 and same(r1, A.top_rows(vec, 9, True, None, beta=2.0, seed=5, draw=5, row0=100)), name
        r2 = eng.acquire(x, 9, score=name, beta=2.0, row0=100)
        assert eng.draw == 10 and not torch.equal(r1.keys, r2.keys)
        eng.draw = 0
        r4 = eng.acquire(x, 9, score=name, beta=2.0, row0=100)
        assert torch.equal(r1.indices, r4.indices) and torch.equal(r1.keys, r4.keys) and torch.equal(r1.values, r4.values)
    # the default score is the first
    eng = FusedMLP(opt_for(criterion, CRITERIA[criterion]))
    assert eng.acquire(x, 3).score_name == SCORES[criterion][0]


@pytest.mark.parametrize("criterion", ["nll", "mse"])
def test_acquire_analytic(oracle, criterion):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    eng, twin = FusedMLP(opt_for(criterion, CRITERIA[criterion])), FusedMLP(opt_for(criterion, CRITERIA[criterion]))
    name = "entropy" if criterion == "nll" else "variance"
    res = eng.acquire(x, 5, score=name, analytic=True)
    pred = twin_predictive(twin, criterion, x, analytic=True)
    assert same(res, A.top_rows(vector_of(name, criterion, pred).cpu().numpy(), 5, True, None))
    assert eng.draw == twin.draw == (4 if criterion == "nll" else 0)


def test_acquire_analytic_is_refused_as_predict_analytic_refuses(oracle):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    for criterion in ("bce", "gauss"):
        eng = FusedMLP(opt_for(criterion, CRITERIA[criterion]))
        with pytest.raises(ValueError) as own:
            eng.predict_analytic(x)
        with pytest.raises(ValueError) as got:
            eng.acquire(x, 5, score="entropy" if criterion == "bce" else "variance", analytic=True)
        assert str(got.value) == str(own.value) and eng.draw == 0


def test_top_rows_on_a_result_field_and_device_draw(oracle):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    eng = FusedMLP(opt_for("nll", 5, device_draw=True))
    pred = eng.predict_classes(x)
    ent = pred.entropy.cpu().numpy()
    assert same(eng.top_rows(pred.entropy, 6, largest=False), A.top_rows(ent, 6, False, None))
    assert same(eng.top_rows(pred.entropy[1:], 40), A.top_rows(ent[1:], 40, True, None))            # the 4-byte path, k > R
    assert eng.draw == 4 and eng._draw_dev.cpu().tolist() == [4]
    r = eng.top_rows(pred.entropy, 6, beta=1.0, row0=3)
    assert eng.draw == 5 and eng._draw_dev.cpu().tolist() == [5]     # host and device counter
    assert same(r, A.top_rows(ent, 6, True, None, beta=1.0, seed=5, draw=5, row0=3))
    r = eng.top_rows(pred.entropy, 6, beta=1.0, draw=77)
    assert eng.draw == 5 and same(r, A.top_rows(ent, 6, True, None, beta=1.0, seed=5, draw=77, row0=0))
    ws = eng._top_rows_ws[1]
    eng.top_rows(pred.entropy, 6)
    eng.top_rows(pred.entropy, 9)
    assert eng._top_rows_ws[1] is ws                                  # re-used while R holds


def test_every_refusal_leaves_the_draw_counter_alone(oracle):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    eng = FusedMLP(opt_for("nll", 5))
    ok = torch.zeros(R_POOL, dtype=torch.uint8, device="cuda")
    bad = [dict(score="mutual_info", map=True), dict(score="mutual_info", S=1), dict(score="variance"), dict(score="nonsense"),
           dict(k=0), dict(k=4097), dict(k=2.5), dict(exclude=ok[:-1]), dict(exclude=ok.int()), dict(exclude=ok.cpu()),
           dict(exclude=[0] * R_POOL), dict(beta=0.0), dict(beta=-1.0), dict(beta=float("nan")), dict(score="random", beta=0.0),
           dict(analytic=True, map=True), dict(score="entropy", beta=1.0, row0=2 ** 32 - R_POOL + 1),
           dict(score="entropy", beta=1.0, row0=-1), dict(score="random", row0=2 ** 32)]
    for kw in bad:
        kw = dict(dict(k=5), **kw)
        with pytest.raises(ValueError) as err:
            eng.acquire(x, **kw)
        assert eng.draw == 0 and len(str(err.value)) > 20, kw
    with pytest.raises(ValueError):
        eng.acquire(x.cpu(), 5)
    for kw in (dict(k=0), dict(k=4097), dict(beta=0.0), dict(beta=1.0, largest=False), dict(exclude=ok[:-1]),
               dict(beta=1.0, row0=2 ** 32)):
        kw = dict(dict(k=5), **kw)
        with pytest.raises(ValueError):
            eng.top_rows(torch.zeros(R_POOL, device="cuda"), **kw)
    with pytest.raises(ValueError):
        eng.top_rows(torch.zeros(R_POOL, device="cuda").double(), 5)
    assert eng.draw == 0
    assert eng.acquire(x, 5, score="entropy", map=True).S == 1 and eng.draw == 0       # a MAP pass consumes nothing


def test_active_learning_grows_the_labelled_set_and_repeats():
    from vbnn_amd import data
    from vbnn_amd.active import active_learning
    from vbnn_amd.train import default_opt
    train, test = data.synthetic_digits(200, 100)
    xp = torch.from_numpy(train["inputs"]).cuda().reshape(200, -1)
    yp = torch.from_numpy(train["targets"].astype(np.int32)).cuda()
    xt = torch.from_numpy(test["inputs"]).cuda().reshape(100, -1)
    yt = torch.from_numpy(test["targets"].astype(np.int32)).cuda()
    opt = default_opt(hidden=[32], batchSize=50, S=2, testSamples=4, log=False)
    for kw in (dict(score="mutual_info"), dict(score="entropy", beta=1.0)):
        curve = active_learning(opt, xp, yp, xt, yt, n_init=50, k=10, rounds=3, epochs=2, **kw)
        assert [c["labels"] for c in curve] == [50, 60, 70]
        seen = set(range(50))
        for c in curve:
            new = c["acquired"]
            assert len(new) == 10 == len(set(new)) and not (set(new) & seen) and all(0 <= r < 200 for r in new)
            seen |= set(new)
            assert np.isfinite(c["nll"]) and 0.0 <= c["accuracy"] <= 100.0
        assert active_learning(opt, xp, yp, xt, yt, n_init=50, k=10, rounds=3, epochs=2, **kw) == curve
