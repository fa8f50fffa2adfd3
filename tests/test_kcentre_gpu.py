"""vbnn_kcentre through the C ABI and FusedMLP.features / spread_rows / acquire_diverse / active_learning(diverse=True) on the
device, against the NumPy restatement of tests/_kcentre_np.py (itself held to a float64 greedy by test_kcentre_ref.py).
Index, key, dist, min_dist and the four counts are compared bit for bit, with the guard bytes before and after every output.

Rules of the kernel-level cases. Every output is a run of bytes inside an allocation filled with 0xA5, 64 guard bytes either
side, compared WHOLE. Every case runs twice -- on a workspace full of the sentinel (it needs no preparation), then on the
workspace the first run left. The features lie `off` floats past a 256-byte boundary with a row pitch ld >= D whose pads hold a
NaN: a pad read into a sum would show in every output."""
import ctypes as C

import numpy as np
import pytest

from tests import _kcentre_np as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
SB, GUARD = 0xA5, 64
PAD = np.uint32(0x7fc12345)                                         # what the pads of a pitched feature matrix hold


def _ctx():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, L.lib(), nn.Context.get().h


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Out:
    """n elements of itemsize bytes between two guards; 0xA5 before the launch, or `init` (min_dist on resume)."""

    def __init__(self, n, itemsize, init=None):
        self.nbytes = n * itemsize
        raw = np.full(GUARD + self.nbytes + GUARD, SB, np.uint8)
        if init is not None:
            raw[GUARD:GUARD + self.nbytes] = np.ascontiguousarray(init).view(np.uint8)
        self.raw = torch.from_numpy(raw).cuda()
        assert self.raw.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def expect(self, payload):
        want = np.full(GUARD + self.nbytes + GUARD, SB, np.uint8)
        want[GUARD:GUARD + self.nbytes] = np.ascontiguousarray(payload).view(np.uint8)
        return np.array_equal(self.raw.cpu().numpy(), want)

    def untouched(self):
        return self.expect(np.full(self.nbytes, SB, np.uint8))


class Feat:
    """R x D features on the device: `off` floats past a 256-byte boundary, row pitch ld, every pad a NaN."""

    def __init__(self, F, ld=None, off=0):
        R, D = F.shape
        self.ld = ld = D if ld is None else ld
        words = np.full(off + R * ld + 8, PAD, np.uint32)
        body = words[off:off + R * ld].reshape(R, ld)
        body[:, :D] = bits(F)
        self.raw = torch.from_numpy(words.view(np.int32)).cuda()       # (as integers: every NaN payload arrives as it is)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.raw.data_ptr() + 4 * off)


def dev_words(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


_WS = {}


def launch(feat, R, D, k, w=None, ex=None, cen=None, resume=None, ctx=None, fresh=True, with_key=True, with_dist=True,
           ws_bytes=None, ws_off=0, n_centres=None, min_dist=True, resume_flag=None, ld=None, null=(), odd=()):
    """One call: (status, index, key, dist, min_dist, counts, ignored) with the outputs as Out."""
    L, lib, own = _ctx()
    n = C.c_size_t()
    ws_R = R if 1 <= R < 1 << 31 else 100                            # (a refused R: any workspace will do)
    assert lib.vbnn_kcentre_workspace_bytes(ws_R, min(max(D, 1), K.MAX_D), min(max(k, 1), K.MAX_K), C.byref(n)) == 0
    if fresh or "ws" not in _WS or _WS["ws"].numel() < n.value + 16:
        _WS["ws"] = torch.full((n.value + 16,), SB, dtype=torch.uint8, device="cuda")
    ws = _WS["ws"]
    kk = max(k, 1)
    index, key, dist, counts = Out(kk, 4), Out(kk, 4), Out(kk, 4), Out(4, 8)
    md = Out(ws_R, 4, init=resume)
    w_dev, ex_dev = dev_words(None if w is None else bits(w), np.int32), dev_words(ex, np.uint8)
    cen_dev = None if cen is None or len(cen) == 0 else torch.from_numpy(np.asarray(cen, np.int32)).cuda()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731

    def out(name, o):                                                 # a refusal's NULL or misaligned (2 bytes off) output
        if name == "counts" and "counts4" in odd:                     # on a 4-byte boundary that is no 8-byte one
            return C.c_void_p(o.ptr.value + 4)
        return None if name in null else (C.c_void_p(o.ptr.value + 2) if name in odd else o.ptr)
    a = L.KcentreArgs(feat=feat.ptr if feat is not None else None, ld=(feat.ld if feat is not None else D) if ld is None else ld, weight=p(w_dev), exclude=p(ex_dev),
                      centres=p(cen_dev), R=R, D=D, n_centres=(0 if cen_dev is None else cen_dev.numel()) if n_centres is None else n_centres,
                      k=k, resume=int(resume is not None) if resume_flag is None else resume_flag, reserved=0, index=out("index", index),
                      key=out("key", key) if with_key else None, dist=out("dist", dist) if with_dist else None,
                      min_dist=out("min_dist", md) if min_dist else None, counts=out("counts", counts), workspace=C.c_void_p(ws.data_ptr() + ws_off),
                      workspace_bytes=n.value if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    st = lib.vbnn_kcentre(own if ctx is None else ctx, C.byref(a))
    L.check(lib.vbnn_sync(own if ctx is None else ctx))
    torch.cuda.synchronize()
    ignored = int(ws[ws_off:ws_off + 8].cpu().numpy().view(np.int64)[0]) if st == 0 else None
    return st, index, key, dist, md, counts, ignored


def check(F, k, label, w=None, ex=None, cen=None, ld=None, off=0, resume=None, ctx=None, want=None, feat=None):
    R, D = F.shape
    feat = feat or Feat(F, ld, off)
    want = want or K.kcentre(F, k, w, ex, () if cen is None else cen, resume=resume is not None, min_dist=resume)
    for run in (0, 1):
        st, index, key, dist, md, counts, ignored = launch(feat, R, D, k, w, ex, cen, resume, ctx, fresh=run == 0)
        assert st == 0, label
        assert counts.expect(np.array(want["counts"], np.int64)), f"{label}, run {run}: counts {want['counts']} (or their guards)"
        assert index.expect(want["index"]), f"{label}, run {run}: index (or its guards)"
        assert key.expect(bits(want["key"])), f"{label}, run {run}: key"
        assert dist.expect(bits(want["dist"])), f"{label}, run {run}: dist"
        assert md.expect(bits(want["min_dist"])), f"{label}, run {run}: min_dist"
        assert ignored == want["ignored"], f"{label}, run {run}: ignored centres"
    return want


def features(R, D, seed, voids=False):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((R, D)).astype(F32)
    if R >= 4:
        F[R // 2] = F[0]                                            # duplicate rows R / 2 apart: ties across workgroups
        F[R // 2 + 1] = F[1]
    if voids and R >= 8:
        F[3, D // 2] = np.nan
        F[4, 0] = np.inf
        F[R - 1, :] = 3e19                                          # finite entries, an overflowing norm
    return F, rng


def pitch(D, i):
    c4, c2 = (D + 3) // 4 * 4, (D + 1) // 2 * 2
    return [(D, 0), (D + 3, 1), (c4 + 4, 2), (c2 + 2, 0), (c4 + 4, 0), (D + 1, 3)][i % 6]     # (ld, off): every load path, with pads


# D x R crossed sparsely; k = 1, 2, R and more than the candidates among them
SHAPES = [(1, 1, (1, 3)), (1, 5000, (2,)), (3, 2, (1, 2, 5)), (3, 257, (257,)), (4, 63, (63,)), (5, 65, (68,)), (63, 5000, (6,)),
          (64, 257, (257,)), (255, 63, (63,)), (256, 5000, (6,)), (257, 65, (65,)), (257, 5000, (3,)), (1000, 257, (24,)),
          (1000, 2, (2,)), (1024, 63, (4,)), (1025, 63, (4,)), (2000, 65, (5,)), (4096, 63, (63,)), (4096, 257, (4,)), (K.MAX_D, 65, (10,)), (K.MAX_D, 2, (1, 2))]


@pytest.mark.parametrize("D,R,ks", SHAPES)
def test_kcentre_is_the_restatement_bit_for_bit(D, R, ks):
    n_case = 0
    blk = K.block(D)
    for k in ks:
        for variant in range(4):
            n_case += 1
            i = n_case + D + R
            F, rng = features(R, D, 1000 * D + R + variant, voids=variant % 2 == 1)
            w = None
            if variant >= 2:
                w = (rng.random(R) + 0.25).astype(F32)
                if R >= 16:
                    w[[2, 5, 6, 7, 9]] = [0.0, -0.0, np.nan, -1.0, np.inf]
            ex = (rng.random(R) < 0.25).astype(np.uint8) if i % 3 == 0 else None
            nc = [0, 1, blk, blk + 1][i % 4] if R * D * (blk + 1) <= 40_000_000 else [0, 1][i % 2]
            cen = list(rng.integers(0, R, size=nc))
            if nc >= 3:
                cen[1] = cen[0]                                     # a duplicate, an index past the matrix, a negative one
                cen[2], cen[-1] = R + 5, -1
                if R >= 8:
                    cen[nc // 2] = 3                                # a void centre (with voids), an excluded one (with exclude)
                    if ex is not None:
                        ex[cen[0]] = 1
            ld, off = pitch(D, i)
            check(F, k, f"D={D} R={R} k={k} variant={variant} nc={nc} ld={ld} off={off}", w, ex, cen, ld, off)
    print(f"D={D} R={R}: {n_case} cases, each run twice")


def test_void_rows_change_no_other_row():
    R, D = 300, 70
    F, rng = features(R, D, 77)
    w = (rng.random(R) + 0.5).astype(F32)
    base = check(F, 40, "no void rows", w, None, [9])
    G = np.vstack([F, np.zeros((3, D), F32)])
    G[R, 4], G[R + 1, 0], G[R + 2, :] = np.nan, -np.inf, -3e19
    got = check(G, 40, "three void rows", np.concatenate([w, np.ones(3, F32)]), None, [9, R + 1])
    assert got["counts"] == [40, R, 3, 0]
    assert np.array_equal(got["index"], base["index"]) and np.array_equal(bits(got["key"]), bits(base["key"]))
    assert np.array_equal(bits(got["min_dist"][:R]), bits(base["min_dist"]))


def test_ties_go_to_the_lower_row_across_workgroups():
    R, D = 5000, 1100                                               # one workgroup per row: duplicates always in different ones
    rng = np.random.default_rng(5)
    base = rng.integers(-3, 4, size=(10, D)).astype(F32)
    F = base[np.arange(R) % 10]                                     # ten distinct rows, each 500 times: every step is a 500-way tie
    want = check(F, 14, "mass ties", None, None, None)
    assert want["index"][0] == 0
    assert all(int(r) < 10 for r in want["index"][:10]) and list(want["index"][10:]) == [10, 11, 12, 13]
    Fw, _ = features(2049, 64, 6)                                   # a wave per row: duplicates R / 2 apart
    check(Fw, 9, "wave rows, duplicates", None, None, [1])


def test_everything_excluded_and_candidates_running_out():
    F, rng = features(65, 33, 8)
    ex = np.ones(65, np.uint8)
    want = check(F, 5, "all excluded", None, ex, [0, 1])
    assert want["counts"] == [0, 0, 0, 65] and np.all(want["index"] == -1)
    ex[[7, 40]] = 0
    want = check(F, 5, "two candidates", rng.random(65).astype(F32), ex, None)
    assert want["counts"][0] == 2 and list(want["index"][2:]) == [-1, -1, -1]


def test_resume_equals_one_call():
    R, D = 400, 130
    F, rng = features(R, D, 9, voids=True)
    w = (rng.random(R) + 0.1).astype(F32)
    ex = (rng.random(R) < 0.2).astype(np.uint8)
    feat = Feat(F, D + 2, 0)
    for weight in (None, w):
        whole = check(F, 21, "a + b", weight, ex, [17, 18], feat=feat)
        first = check(F, 8, "a", weight, ex, [17, 18], feat=feat)
        ex2 = ex.copy()
        ex2[first["index"]] = 1
        second = check(F, 13, "then b", weight, ex2, None, resume=first["min_dist"], feat=feat)
        for f in ("index", "key", "dist"):
            assert np.array_equal(np.concatenate([first[f], second[f]]).view(np.uint32), whole[f].view(np.uint32)), f
        assert np.array_equal(bits(second["min_dist"]), bits(whole["min_dist"]))


def test_the_bits_do_not_depend_on_the_grid():
    L, lib, _ = _ctx()
    from vbnn_amd import nn
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    small = nn.Context.with_cu_budget(0, max(1, cus // 16))
    try:
        assert small.cu_budget != cus
        for R, D, k in ((5000, 48, 20), (9000, 260, 12), (5000, 1030, 6)):  # more rows than either grid holds workgroups
            F, rng = features(R, D, R + D)
            w = rng.random(R).astype(F32)
            want = K.kcentre(F, k, w, None, [3, 4])
            check(F, k, f"default context R={R} D={D}", w, None, [3, 4], want=want)
            check(F, k, f"{small.cu_budget}-CU context R={R} D={D}", w, None, [3, 4], want=want, ctx=small.h)
    finally:
        torch.cuda.synchronize()
        L.check(lib.vbnn_ctx_destroy(small.h))


def test_key_and_dist_are_optional():
    F, _ = features(100, 20, 10)
    want = K.kcentre(F, 7)
    st, index, key, dist, md, counts, _ = launch(Feat(F), 100, 20, 7, with_key=False, with_dist=False)
    assert st == 0 and index.expect(want["index"]) and md.expect(bits(want["min_dist"])) and key.untouched() and dist.untouched()


def test_every_refusal_writes_nothing():
    L, lib, _ = _ctx()
    F, _ = features(100, 20, 11)
    feat = Feat(F)
    odd = Feat(F)
    odd.ptr = C.c_void_p(feat.raw.data_ptr() + 2)                   # a misaligned feature pointer
    cases = [dict(R=0), dict(R=1 << 31), dict(D=0), dict(D=K.MAX_D + 1), dict(k=0), dict(k=4097), dict(ld=19), dict(n_centres=-1),
             dict(n_centres=2), dict(resume_flag=2), dict(resume_flag=-1), dict(feat=None), dict(min_dist=False), dict(ws_bytes=64),
             dict(ws_off=4), dict(feat=odd), dict(null=("index",)), dict(null=("counts",)), dict(odd=("index",)), dict(odd=("key",)),
             dict(odd=("dist",)), dict(odd=("min_dist",)), dict(odd=("counts",)), dict(odd=("counts4",))]
    for c in cases:
        kw = dict(c)
        st, index, key, dist, md, counts, _ = launch(kw.pop("feat", feat), kw.pop("R", 100), kw.pop("D", 20), kw.pop("k", 5), **kw)
        assert st != 0 and len(lib.vbnn_last_error()) > 0, c
        for out in (index, key, dist, md, counts):
            assert out.untouched(), c
    L.check(lib.vbnn_sync(_ctx()[2]))


# ------------------------------------------------------------------------------------------------ engine level
R_POOL = 37


def opt_for(criterion, n_classes, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=5, input_size=20, hidden=[16, 12],
             n_classes=n_classes, type="vb", testSamples=4, criterion=criterion)
    o.update(kw)
    return o


CRITERIA = {"nll": 5, "bce": 3, "mse": 2, "gauss": 4}


def pool(oracle, R=R_POOL):
    return torch.from_numpy(oracle.fill_normal(R, 20, 7, 4, 0, 0)).cuda()


def vector_of(name, criterion, pred):
    if name == "least_confidence":
        return 1.0 - pred.topk_prob[:, 0]
    if name == "total_variance":
        return pred.row_var + pred.row_noise_var
    if name == "variance":
        return pred.row_var
    if criterion == "bce":
        return pred.row_mutual_info if name == "mutual_info" else pred.row_entropy
    return pred.mutual_info if name == "mutual_info" else pred.entropy


def twin_predictive(twin, criterion, x, **kw):
    if criterion == "nll":
        return twin.predict_classes(x, topk=2, keep_probs=False, **kw)
    return twin.predict_labels(x, **kw) if criterion == "bce" else twin.predict_regression(x, **kw)


def same(res, want):
    return (np.array_equal(res.indices.cpu().numpy(), want["index"]) and np.array_equal(bits(res.keys.cpu().numpy()), bits(want["key"]))
            and np.array_equal(bits(res.dists.cpu().numpy()), bits(want["dist"]))
            and np.array_equal(bits(res.min_dist.cpu().numpy()), bits(want["min_dist"]))
            and [res.n_selected, res.n_candidates, res.n_void, res.n_excluded] == want["counts"]
            and res.n_ignored_centres == want["ignored"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_features_do_not_depend_on_the_chunks_and_feed_the_final_linear(oracle, dtype, mode):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle, 45)
    whole = FusedMLP(opt_for("nll", 5, dtype=dtype, mode=mode, predict_rows=32768))
    small = FusedMLP(opt_for("nll", 5, dtype=dtype, mode=mode, predict_rows=7))
    f = whole.features(x)
    assert f.dtype == torch.float32 and tuple(f.shape) == (45, 12) and whole.draw == 0
    assert torch.equal(f, small.features(x)) and torch.equal(f, whole.features(x, layer=1))
    f0 = whole.features(x, layer=0)
    assert tuple(f0.shape) == (45, 16) and torch.equal(f0, small.features(x, layer=-2))
    for bad in (2, -3, 1.5):
        with pytest.raises(ValueError):
            whole.features(x, layer=bad)
    # the final Linear on them reproduces the MAP log-probabilities within the fp32 GEMM bound of the parity tests
    # (|d| <= 4e-6 sum |a b| on a logit, which moves a log-softmax value by at most twice that)
    ref = whole.predict_classes(x, map=True)
    assert whole.draw == 0
    w3 = whole.w3_s.t[:5, :12].double().cpu().numpy()               # the operand the head reads (bf16: the packed copy)
    b3 = whole.bias3.double().cpu().numpy()
    h = f.double().cpu().numpy()
    lg = h @ w3.T + b3
    e = 4e-6 * (np.abs(h) @ np.abs(w3).T + np.abs(b3)).max()
    lp = lg - lg.max(1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(1, keepdims=True))
    d = np.abs(ref.log_probs.cpu().numpy() - lp).max()
    tol = max(1e-5, 2 * e)
    print(f"{dtype} {mode}: max |d log p| {d:.3e}, tolerance {tol:.3e}")
    assert d <= tol


@pytest.mark.parametrize("criterion", list(CRITERIA))
def test_acquire_diverse_is_the_restatement_on_the_engines_own_features_and_scores(oracle, criterion):
    from vbnn_amd.acquisition import SCORES
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    e = (np.random.default_rng(3).random(R_POOL) < 0.3).astype(np.uint8)
    e_dev = torch.from_numpy(e).cuda()
    labelled = list(np.nonzero(e)[0])
    for name in SCORES[criterion]:
        eng, twin = FusedMLP(opt_for(criterion, CRITERIA[criterion])), FusedMLP(opt_for(criterion, CRITERIA[criterion]))
        if name in ("random", "margin"):
            with pytest.raises(ValueError, match="weighted=False" if name == "random" else "least_confidence"):
                eng.acquire_diverse(x, 9, score=name)
            assert eng.draw == 0
            continue
        res = eng.acquire_diverse(x, 9, score=name, exclude=e_dev)
        vec = vector_of(name, criterion, twin_predictive(twin, criterion, x)).cpu().numpy()
        feats = twin.features(x).cpu().numpy()
        assert same(res, K.kcentre(feats, 9, vec, e, labelled)), name
        assert eng.draw == twin.draw == 4 and res.S == 4 and res.score_name == name and res.chunks == 1 and res.predictive is not None
        assert not e[res.indices.cpu().numpy()].any()
        # chunked scoring and features: the same bits; without cover_labelled: no initial centres
        small = FusedMLP(opt_for(criterion, CRITERIA[criterion], predict_rows=3 * 4))
        r2 = small.acquire_diverse(x, 9, score=name, exclude=e_dev.bool(), cover_labelled=False)
        assert r2.chunks > 1 and same(r2, K.kcentre(feats, 9, vec, e, ())), name
        # features given: used as they are
        given = torch.from_numpy(np.random.default_rng(4).standard_normal((R_POOL, 6)).astype(F32)).cuda()
        eng.draw = 0
        r3 = eng.acquire_diverse(x, 5, score=name, features=given)
        assert same(r3, K.kcentre(given.cpu().numpy(), 5, vec, None, ())), name
    # plain k-centre: no predictive, no draw
    eng = FusedMLP(opt_for(criterion, CRITERIA[criterion]))
    res = eng.acquire_diverse(x, 6, weighted=False, exclude=e_dev)
    assert eng.draw == 0 and res.predictive is None and res.score_name is None and res.S == 0
    assert same(res, K.kcentre(eng.features(x).cpu().numpy(), 6, None, e, labelled))
    assert eng.acquire_diverse(x, 3).score_name == SCORES[criterion][0]      # the default score is the first


def test_spread_rows_state_continues_a_selection(oracle):
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("nll", 5))
    rng = np.random.default_rng(12)
    F = rng.standard_normal((200, 50)).astype(F32)
    w, e = rng.random(200).astype(F32), (rng.random(200) < 0.2).astype(np.uint8)
    wide = torch.from_numpy(np.hstack([F, np.full((200, 6), 9.0, F32)])).cuda()
    view = wide[:, :50]                                             # a row pitch of 56: honoured, not copied
    assert view.stride(0) == 56
    mask = torch.zeros(200, dtype=torch.bool, device="cuda")
    mask[[4, 9]] = True
    whole = eng.spread_rows(view, 15, torch.from_numpy(w).cuda(), torch.from_numpy(e).cuda(), mask)
    assert same(whole, K.kcentre(F, 15, w, e, [4, 9]))
    first = eng.spread_rows(view, 6, torch.from_numpy(w).cuda(), torch.from_numpy(e).cuda(), torch.tensor([4, 9, 700, -3], device="cuda"))
    assert first.n_ignored_centres == 2
    second = eng.spread_rows(view, 9, torch.from_numpy(w).cuda(), state=first)
    assert torch.equal(torch.cat([first.indices, second.indices]), whole.indices)
    assert torch.equal(torch.cat([first.keys, second.keys]), whole.keys) and torch.equal(second.min_dist, whole.min_dist)
    assert eng.draw == 0
    for kw in (dict(k=0), dict(k=4097), dict(k=2.5), dict(weight=torch.zeros(199, device="cuda")), dict(exclude=mask[:-1]),
               dict(centres=torch.zeros(3, device="cuda")), dict(centres=mask[:-1]), dict(state=object())):
        kw = dict(dict(k=5), **kw)
        with pytest.raises(ValueError):
            eng.spread_rows(view, **kw)
    for bad in (view.double(), view.cpu(), view[0], torch.zeros(5, 8193, device="cuda")):
        with pytest.raises(ValueError):
            eng.spread_rows(bad, 3)


def test_every_refusal_leaves_the_draw_counter_alone(oracle):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    eng = FusedMLP(opt_for("nll", 5))
    ok = torch.zeros(R_POOL, dtype=torch.uint8, device="cuda")
    feats = torch.zeros(R_POOL, 12, device="cuda")
    bad = [dict(score="random"), dict(score="margin"), dict(score="mutual_info", map=True), dict(score="mutual_info", S=1),
           dict(score="variance"), dict(score="nonsense"), dict(analytic=True, map=True), dict(k=0), dict(k=4097), dict(k=2.5),
           dict(exclude=ok[:-1]), dict(exclude=ok.int()), dict(features=feats[:-1]), dict(features=feats.double()),
           dict(features=feats.cpu()), dict(features=feats[0]), dict(weighted=False, score="entropy")]
    for kw in bad:
        kw = dict(dict(k=5), **kw)
        with pytest.raises(ValueError) as err:
            eng.acquire_diverse(x, **kw)
        assert eng.draw == 0 and len(str(err.value)) > 20, kw
    with pytest.raises(ValueError):
        eng.acquire_diverse(x.cpu(), 5)
    for criterion in ("bce", "gauss"):                              # analytic: refused as predict_analytic refuses it
        other = FusedMLP(opt_for(criterion, CRITERIA[criterion]))
        with pytest.raises(ValueError) as own:
            other.predict_analytic(x)
        with pytest.raises(ValueError) as got:
            other.acquire_diverse(x, 5, score="entropy" if criterion == "bce" else "variance", analytic=True)
        assert str(got.value) == str(own.value) and other.draw == 0
    assert eng.acquire_diverse(x, 5, score="entropy", map=True).S == 1 and eng.draw == 0       # a MAP pass consumes nothing
    assert eng.acquire_diverse(x, 5, score="entropy", analytic=True).n_selected == 5 and eng.draw == 4  # as acquire(analytic=True)


def test_acquire_is_not_moved_by_a_diverse_call_in_between(oracle):
    from vbnn_amd.engine import FusedMLP
    x = pool(oracle)
    a, b = FusedMLP(opt_for("nll", 5)), FusedMLP(opt_for("nll", 5))
    a1, a2 = a.acquire(x, 9), a.acquire(x, 9, score="entropy", beta=2.0)
    b1 = b.acquire(x, 9)
    b.acquire_diverse(x, 9)
    assert b.draw == 8
    b.draw = 4                                                       # apart from the draws it consumed
    b2 = b.acquire(x, 9, score="entropy", beta=2.0)
    for p, q in ((a1, b1), (a2, b2)):
        assert torch.equal(p.indices, q.indices) and torch.equal(p.keys, q.keys) and torch.equal(p.values, q.values)
    assert a.draw == b.draw == 9


def test_diverse_takes_one_row_of_every_cluster_where_top_k_takes_one_cluster(oracle):
    from vbnn_amd.engine import FusedMLP
    c, m = 8, 8
    centres = oracle.fill_normal(c, 20, 11, 4, 0, 0)                # well separated: about 6 apart in 20 dimensions
    x = torch.from_numpy(np.repeat(centres, m, axis=0).astype(F32)[np.random.default_rng(2).permutation(c * m)]).cuda()
    cluster = {r: int(np.argmin(((centres - x[r].cpu().numpy()) ** 2).sum(1))) for r in range(c * m)}
    eng = FusedMLP(opt_for("nll", 5))
    ent = eng.predict_classes(x, map=True).entropy.cpu().numpy()
    per = [ent[[r for r in range(c * m) if cluster[r] == j]] for j in range(c)]
    assert all(len(set(p.tolist())) == 1 for p in per)              # exact duplicates score alike on the means
    tops = sorted(float(p[0]) for p in per)
    assert tops[-1] > tops[-2] and tops[0] > 0                                  # one cluster holds the highest scores
    top = eng.acquire(x, c, score="entropy", map=True)
    assert len({cluster[r] for r in top.indices.cpu().tolist()}) == 1
    div = eng.acquire_diverse(x, c, score="entropy", map=True)
    assert sorted(cluster[r] for r in div.indices.cpu().tolist()) == list(range(c))
    assert cluster[int(div.indices[0])] == cluster[int(top.indices[0])]      # the most uncertain cluster first
    assert eng.draw == 0


def test_active_learning_diverse_grows_the_labelled_set_and_repeats():
    from vbnn_amd import data
    from vbnn_amd.active import active_learning
    from vbnn_amd.train import default_opt
    train, test = data.synthetic_digits(200, 100)
    xp = torch.from_numpy(train["inputs"]).cuda().reshape(200, -1)
    yp = torch.from_numpy(train["targets"].astype(np.int32)).cuda()
    xt = torch.from_numpy(test["inputs"]).cuda().reshape(100, -1)
    yt = torch.from_numpy(test["targets"].astype(np.int32)).cuda()
    opt = default_opt(hidden=[32], batchSize=50, S=2, testSamples=4, log=False)
    curve = active_learning(opt, xp, yp, xt, yt, n_init=50, k=10, rounds=3, epochs=2, score="entropy", diverse=True)
    assert [c["labels"] for c in curve] == [50, 60, 70]
    seen = set(range(50))
    for c in curve:
        new = c["acquired"]
        assert len(new) == 10 == len(set(new)) and not (set(new) & seen) and all(0 <= r < 200 for r in new)
        seen |= set(new)
        assert np.isfinite(c["nll"]) and 0.0 <= c["accuracy"] <= 100.0
    again = active_learning(opt, xp, yp, xt, yt, n_init=50, k=10, rounds=3, epochs=2, score="entropy", diverse=True)
    assert again == curve                                           # bit for bit: the floats compare equal
    with pytest.raises(ValueError):
        active_learning(opt, xp, yp, xt, yt, n_init=50, k=10, rounds=1, diverse=True, beta=1.0)
