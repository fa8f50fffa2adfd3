"""Checkpoint and resume on the GPU: vbnn_digest bit for bit against its NumPy restatement (tests/_digest_np.py) on every path of the
kernel; FusedMLP.state_dict / load_state_dict / save / load -- an engine that loaded a state continues BIT FOR BIT like the one that saved
it (parameters, Adam moments, draw counter, predictions), under a held mask, with the device draw counter, across dtypes, for a compact
network; the refusals; a training run resumed in a fresh process against the uninterrupted one; the replica check with two ranks.

Bitwise throughout: every kernel that writes a parameter is deterministic and the noise is addressed by (seed, layer, draw, row). The one
exception is the logged loss (the criterion's double-precision atomic sum), compared to rel = 1e-12 as tests/test_train_gpu.py does."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from tests import _children
from tests import _digest_np as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one trip of the whole grid: DIGEST_MAX_BLOCKS x DIGEST_THREADS threads x DIGEST_UNROLL loads x 4 words (csrc/digest.hip)
GRID_PASS = 2048 * 256 * 2 * 4


# ------------------------------------------------------------------------------------------------ 1. the digest
def _mods():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    return L, nn


@pytest.fixture(scope="module")
def words():
    """Random bit patterns (NaNs, denormals and -0.0 among them), 16-byte aligned on the device, and their host copy."""
    n = GRID_PASS + 7 + 64
    host = np.random.RandomState(21).randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    host[:6] = [0x7fc00001, 0x80000000, 0x00000001, 0xffffffff, 0, 0x7f800000]
    dev = torch.from_numpy(host.view(np.int32)).cuda()
    assert dev.data_ptr() % 16 == 0
    return host, dev


def _digest(dev_view, n, index0=0, out=None):
    L, nn = _mods()
    if out is None:
        out = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = L.lib().vbnn_digest(nn.Context.get().h, C.c_void_p(dev_view.data_ptr()), n, index0, C.c_void_p(out.data_ptr()))
    return st, out


def _value(out):
    return int(out.cpu()[0]) & D.M64


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 257, GRID_PASS + 7])
def test_digest_is_the_restatement(words, n):
    host, dev = words
    st, out = _digest(dev, n)
    assert st == 0
    assert _value(out) == D.digest(host[:n])


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 6, 257, 1030])
def test_digest_of_views_off_the_16_byte_boundary(words, offset, n):
    """Start pointers 4, 8 and 12 bytes past a 16-byte boundary: a head of 3, 2, 1 words, then the vector body, then the tail."""
    host, dev = words
    view = dev[offset:offset + n]
    assert view.data_ptr() % 16 == 4 * offset
    st, out = _digest(view, n, index0=5)
    assert st == 0 and _value(out) == D.digest(host[offset:offset + n], 5)


def test_digest_index0_pieces_and_accumulation(words):
    host, dev = words
    n, cut = 5000, 1237                                               # the second piece starts off the boundary
    st, whole = _digest(dev, n, index0=77)
    st1, acc = _digest(dev, cut, index0=77)
    st2, acc = _digest(dev[cut:], n - cut, index0=77 + cut, out=acc)  # two calls accumulating into one word
    assert (st, st1, st2) == (0, 0, 0)
    assert _value(acc) == _value(whole) == D.digest(host[:n], 77)
    st, top = _digest(dev, 9, index0=(1 << 32) - 1 - 9)               # the last legal positions
    assert st == 0 and _value(top) == D.digest(host[:9], (1 << 32) - 1 - 9)


def test_digest_refusals_leave_out_untouched(words):
    L, nn = _mods()
    host, dev = words
    out = torch.full((1,), 0x1234567, dtype=torch.int64, device="cuda")
    h = nn.Context.get().h
    lib = L.lib()
    assert lib.vbnn_digest(h, C.c_void_p(dev.data_ptr() + 2), 8, 0, C.c_void_p(out.data_ptr())) == 1          # misaligned
    assert b"4-byte" in lib.vbnn_last_error()
    assert lib.vbnn_digest(h, C.c_void_p(dev.data_ptr()), 9, (1 << 32) - 9, C.c_void_p(out.data_ptr())) == 1  # one position too far
    assert b"2^32 - 1" in lib.vbnn_last_error()
    assert lib.vbnn_digest(h, C.c_void_p(dev.data_ptr()), 1 << 32, 0, C.c_void_p(out.data_ptr())) == 1
    assert lib.vbnn_digest(h, C.c_void_p(dev.data_ptr()), 8, 0, None) == 1                                     # out NULL
    torch.cuda.synchronize()
    assert int(out.cpu()[0]) == 0x1234567


def test_digest_helper_of_tensors(words):
    from vbnn_amd import checkpoint as ck
    from vbnn_amd.engine import digest
    host, dev = words
    f = dev[:600].view(torch.float32).reshape(20, 30)
    assert digest(f) == D.digest(host[:600])
    m = (dev[:15] & 1).to(torch.uint8)                                # 15 bytes: digested as four words, the last zero-padded
    padded = np.zeros(16, dtype=np.uint8)
    padded[:15] = m.cpu().numpy()
    assert ck.digests([m, f]) == [D.digest(padded), D.digest(host[:600])]


# ------------------------------------------------------------------------------------------------ 2. the engine
I0, HIDDEN, NC, N = 20, [24, 16], 5, 32


def _opt(dtype="f32", mode="lrt", seed=3, **over):
    opt = dict(var_init=1e-3, mu_init=1, B=1e3, S=2, mode=mode, dtype=dtype, seed=seed, input_size=I0, hidden=list(HIDDEN), n_classes=NC,
               fuse_kl=True, state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
    opt.update(over)
    return opt


def _engine(dtype="f32", mode="lrt", seed=3, **over):
    from vbnn_amd.engine import FusedMLP
    opt = _opt(dtype, mode, seed, **over)
    return opt, FusedMLP(opt)


@pytest.fixture(scope="module")
def batches():
    """Six minibatches of 32 rows (the noise of each addressed by its own global rows) with class targets."""
    _, nn = _mods()
    out = []
    for b in range(6):
        x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
        nn.fill_normal(x, 3, 4, 0, 0, row0=b * N)
        t = ((torch.arange(N, device="cuda", dtype=torch.int64) + b * N) * 7 % NC).to(torch.int32)
        out.append((x, t))
    return out


def _train(e, opt, some):
    for x, t in some:
        e.resetGradients()
        for _ in range(int(opt["S"])):
            e.sample()
            e.run(x, t)
        e.update(opt)


def _tensors(e):
    out = {}
    for li, v in enumerate(e.vb):
        out.update({f"layers[{li}].{k}": getattr(v, k) for k in ("means", "lvars", "bias")})
    out.update(weight3=e.weight3, bias3=e.bias3)
    for (li, key), s in sorted(e._opt_state.items()):
        out.update({f"adam[{li}].{key}.m": s["m"], f"adam[{li}].{key}.v": s["v"]})
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def _assert_same_engines(a, b):
    ta, tb = _tensors(a), _tensors(b)
    assert sorted(ta) == sorted(tb)
    for k in ta:
        assert torch.equal(_bits(ta[k]), _bits(tb[k])), k
    assert {k: s["t"] for k, s in a._opt_state.items()} == {k: s["t"] for k, s in b._opt_state.items()}
    assert a.draw == b.draw and a.seed == b.seed


@pytest.mark.parametrize("route", ["dict", "file"])
@pytest.mark.parametrize("mode", ["lrt", "wn"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_loaded_engine_continues_bit_for_bit(tmp_path, batches, dtype, mode, route):
    from vbnn_amd.engine import FusedMLP
    opt, A = _engine(dtype, mode)
    A.prepare()
    _train(A, opt, batches[:3])
    if route == "dict":
        _, Bn = _engine(dtype, mode, seed=11)                         # fresh, another seed: other parameters, other noise
        assert not torch.equal(Bn.vb[0].means, A.vb[0].means) and Bn.seed != A.seed
        ptrs = [v.means.data_ptr() for v in Bn.vb]
        Bn.load_state_dict(A.state_dict())
        assert ptrs == [v.means.data_ptr() for v in Bn.vb]           # in place: argument blocks keep their addresses
    else:
        path = A.save(str(tmp_path / "model"))
        Bn = FusedMLP.load(path)
        assert Bn.dtype == dtype and Bn.mode == mode and Bn.sizes == A.sizes
    _assert_same_engines(A, Bn)
    assert A.draw == 6 and sorted(A._opt_state) == [(0, "mean"), (0, "var"), (1, "mean"), (1, "var")]
    _train(A, opt, batches[3:])
    _train(Bn, opt, batches[3:])
    torch.cuda.synchronize()
    _assert_same_engines(A, Bn)
    assert all(s["t"] == 6 for s in Bn._opt_state.values())
    pa, pb = A.predict(batches[0][0], S=4), Bn.predict(batches[0][0], S=4)
    assert torch.equal(pa.probs, pb.probs) and A.draw == Bn.draw == 16
    assert bool(torch.isfinite(pa.probs).all())


def test_state_dict_contents(batches):
    opt, A = _engine("f32")
    A.prepare()
    s0 = A.state_dict()                                               # before any update: no Adam slots
    assert s0["adam"] == [{}, {}] and "held" not in s0 and s0["draw"] == 0 and s0["seed"] == 3
    _train(A, opt, batches[:1])
    s = A.state_dict()
    assert s["format"] == "vbnn_amd.checkpoint" and s["version"] == 1
    assert s["arch"] == {"sizes": [20, 24, 16], "n_classes": 5, "criterion": "nll", "dtype": "f32", "mode": "lrt"}
    assert s["layers"][1]["means"].shape == (16, 24) and s["layers"][1]["means"].dtype == np.float32
    assert s["adam"][0]["var"]["t"] == 1 and s["adam"][0]["var"]["v"].shape == (24, 20) and s["draw"] == 2
    # the digests are the restatement's of the downloaded arrays: taken on the device, before the copy
    assert s["digests"]["layers"][0]["means"] == D.digest(s["layers"][0]["means"])
    assert s["digests"]["adam"][1]["mean"]["m"] == D.digest(s["adam"][1]["mean"]["m"])
    assert s["digests"]["bias3"] == D.digest(s["bias3"])
    # loading a state without Adam slots drops them
    A.load_state_dict(s0)
    assert A._opt_state == {} and A.draw == 0


def test_a_held_mask_comes_with_the_state(tmp_path, batches):
    from vbnn_amd.engine import FusedMLP
    opt, A = _engine("f32")
    A.prepare()
    counts = A.hold_pruned(A.prune(fraction=0.5))
    masks = [A.held_mask(li).clone() for li in range(len(A.vb))]
    frozen = [(_bits(v.means)[m].clone(), _bits(v.lvars)[m].clone()) for v, m in zip(A.vb, masks)]
    _train(A, opt, batches[:2])
    path = A.save(str(tmp_path / "model"))
    Bn = FusedMLP.load(path)
    assert Bn.held == counts == A.held
    for li, m in enumerate(masks):
        assert torch.equal(Bn.held_mask(li), m)
    _train(A, opt, batches[2:4])
    _train(Bn, opt, batches[2:4])
    torch.cuda.synchronize()
    _assert_same_engines(A, Bn)
    assert Bn.held == counts
    for v, m, (mu, lv) in zip(Bn.vb, masks, frozen):                  # the frozen weights' bits are the ones they were frozen with
        assert torch.equal(_bits(v.means)[m], mu) and torch.equal(_bits(v.lvars)[m], lv)
        assert not bool(_bits(v.mu_s.t[:, :v.I])[m].any())           # and they are out of the network: +0 shadows
    Bn.release_pruned()                                               # ... and back with those values
    torch.cuda.synchronize()
    assert Bn.held is None
    for v, m, (mu, lv) in zip(Bn.vb, masks, frozen):
        assert torch.equal(_bits(v.mu_s.t[:, :v.I])[m], mu) and bool(mu.ne(0).any())
    # a state without a mask, loaded into an engine that holds one, drops the mask
    assert A.held == counts
    A.load_state_dict(Bn.state_dict())
    assert A.held is None and A._held is None
    _assert_same_engines(A, Bn)
    for v, w in zip(A.vb, Bn.vb):
        assert torch.equal(_bits(v.mu_s.t), _bits(w.mu_s.t)) and torch.equal(_bits(v.var_s.t), _bits(w.var_s.t))


def test_the_device_draw_counter_is_restored(batches):
    x = batches[0][0]
    _, A = _engine("f32", device_draw=True)
    A.prepare()
    A.predict(x, S=3)                                                 # the counter moves: host mirror and device word
    _, Bn = _engine("f32", seed=11, device_draw=True)
    Bn.load_state_dict(A.state_dict())
    assert Bn.draw == A.draw == 3 and int(Bn._draw_dev.item()) == int(A._draw_dev.item()) == 3
    pa, pb = A.predict(x, S=4), Bn.predict(x, S=4)
    assert torch.equal(pa.probs, pb.probs) and int(Bn._draw_dev.item()) == 7
    _, Cn = _engine("f32", device_draw=True)                          # (the draws matter: an engine three draws behind predicts otherwise)
    Cn.load_state_dict(dict(A.state_dict(), draw=0))
    assert not torch.equal(Cn.predict(x, S=4).probs, A.predict(x, S=4).probs)


def test_an_fp32_state_serves_a_bf16_engine(batches):
    x = batches[0][0]
    opt, A = _engine("f32")
    A.prepare()
    _train(A, opt, batches[:2])
    _, Bn = _engine("bf16", seed=11)
    Bn.load_state_dict(A.state_dict())
    _assert_same_engines(A, Bn)                                       # the fp32 masters and moments, bit for bit
    _, Cn = _engine("bf16")                                           # the same parameters by direct copy and prepare()
    for v, w in zip(A.vb, Cn.vb):
        w.means.copy_(v.means); w.lvars.copy_(v.lvars); w.bias.copy_(v.bias)
    Cn.weight3.copy_(A.weight3); Cn.bias3.copy_(A.bias3)
    Cn.draw = A.draw
    Cn.prepare()
    pb, pc = Bn.predict(x, S=4), Cn.predict(x, S=4)
    assert torch.equal(pb.probs, pc.probs) and bool(torch.isfinite(pb.probs).all())


def test_a_compact_network_is_an_ordinary_engine(tmp_path, batches):
    from vbnn_amd.engine import FusedMLP
    x = batches[0][0]
    _, E = _engine("f32", hidden=[32, 32])
    E.prepare()
    small = E.compact(E.prune_units(fraction=0.25))
    assert small.sizes[1:] != E.sizes[1:]
    path = small.save(str(tmp_path / "compact"))
    back = FusedMLP.load(path)
    assert back.sizes == small.sizes
    _assert_same_engines(small, back)
    assert torch.equal(small.predict(x, S=4).probs, back.predict(x, S=4).probs)


def test_refusals(tmp_path, batches):
    from vbnn_amd.engine import CheckpointError, FusedMLP
    opt, A = _engine("f32")
    A.prepare()
    _train(A, opt, batches[:1])
    state = A.state_dict()
    _, other = _engine("f32", hidden=[24, 20])
    with pytest.raises(CheckpointError, match="sizes"):
        other.load_state_dict(state)
    _, mse = _engine("f32", criterion="mse")
    with pytest.raises(CheckpointError, match="criterion"):
        mse.load_state_dict(state)
    with pytest.raises(CheckpointError, match="version"):
        A.load_state_dict(dict(state, version=2))
    Sh = FusedMLP(_opt("bf16", exchange_mode="sharded"), force_reduce=True)     # a sharded-update engine in one process
    assert Sh.sharded
    for call in (Sh.state_dict, lambda: Sh.load_state_dict(state), lambda: Sh.save(str(tmp_path / "no"))):
        with pytest.raises(RuntimeError, match="sharded update.*follow-up"):
            call()
    assert not os.path.exists(str(tmp_path / "no"))
    # a PruneResult taken before load_state_dict is void afterwards
    res = A.prune(fraction=0.3)
    A.load_state_dict(state)
    with pytest.raises(RuntimeError, match="parameters changed"):
        A.hold_pruned(res)
    with pytest.raises(RuntimeError, match="parameters changed"):
        res.mask(0)


def test_one_flipped_bit_in_the_file_is_caught_and_named(tmp_path, batches):
    from vbnn_amd.engine import CheckpointError, FusedMLP
    opt, A = _engine("f32")
    A.prepare()
    _train(A, opt, batches[:1])
    path = A.save(str(tmp_path / "model"))
    FusedMLP.load(path)                                               # intact: loads
    blob = bytearray(open(path, "rb").read())
    needle = A.vb[1].means.cpu().numpy().tobytes()                    # layer 1's means storage, as the file holds it
    at = blob.find(needle)
    assert at > 0 and blob.find(needle, at + 1) < 0
    blob[at + 4 * 100 + 1] ^= 0x10                                    # one bit of one float
    open(path, "wb").write(bytes(blob))
    with pytest.raises(CheckpointError, match=r"digest mismatch in layers\[1\]\.means"):
        FusedMLP.load(path)


# ------------------------------------------------------------------------------------------------ 3. resume in a fresh process
SERIES = ("devacc", "trainacc", "deverr", "trainerr", "lc")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Run U: two epochs in one process. Run R: one epoch, the process ends, a new process resumes from the run directory for one more.
    Each process trains both variants (tests/_checkpoint_worker.py). Nothing more is started after a non-zero exit."""
    worker = os.path.join(ROOT, "tests", "_checkpoint_worker.py")
    base = tmp_path_factory.mktemp("resume")
    U, R = str(base / "U"), str(base / "R")
    for root, epochs, resume in ((U, 2, 0), (R, 1, 0), (R, 1, 1)):
        res = _children.run([sys.executable, worker, root, str(epochs), str(resume)], capture_output=True, text=True, timeout=240)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return U, R


def _same_tables(a, b, path="engine"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), path
        for k in a:
            _same_tables(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tables(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("variant", ["plain", "pruned"])
def test_a_resumed_run_is_the_uninterrupted_one(runs, variant):
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import logger
    U, R = (os.path.join(d, variant) for d in runs)
    mu, mr = ck.read_checkpoint(os.path.join(U, "model")), ck.read_checkpoint(os.path.join(R, "model"))
    _same_tables(mu["engine"], mr["engine"])                          # tensors, moments, t, draw, seed, masks, digests: bit for bit
    assert mu["engine"]["draw"] == mr["engine"]["draw"] > 0
    assert mu["engine"]["adam"][0]["mean"]["t"] == 12                 # 2 epochs x 6 minibatches
    _same_tables(mu["trainer"], mr["trainer"], "trainer")
    assert mr["trainer"]["epoch"] == 2 and mr["trainer"]["rng"]["key"].shape == (624,)
    for d in (U, R):
        assert os.path.isfile(os.path.join(d, "model.old"))
    one = ck.read_checkpoint(os.path.join(R, "model.old"))            # R's first process left epoch 1 behind
    assert one["trainer"]["epoch"] == 1 and one["engine"]["adam"][0]["mean"]["t"] == 6
    for series in SERIES + (("held fraction",) if variant == "pruned" else ()):
        vu, vr = logger.read_data(os.path.join(U, series)), logger.read_data(os.path.join(R, series))
        assert len(vr) == 2 and len(vu) == 2, (series, vu, vr)
        assert vr == pytest.approx(vu, rel=1e-12), series
    if variant == "pruned":                                           # the schedule's epoch 1 is the RESUMED epoch
        held = logger.read_data(os.path.join(R, "held fraction"))
        assert held[0] == 0.0 and 0.49 < held[1] <= 0.5
        assert "held" not in one["engine"] and mr["engine"]["held"]["counts"] == mu["engine"]["held"]["counts"]
        assert sum(mr["engine"]["held"]["counts"]) == round(held[1] * (784 * 32 + 32 * 24))
    else:
        assert "held" not in mr["engine"]


# ------------------------------------------------------------------------------------------------ 4. the replica check
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_check_replicas_with_two_ranks_on_one_gpu():
    """Identical replicas pass; one weight moved by one ulp on one rank and EVERY rank raises, naming the layer. One time limit for both
    children (the launcher's), and nothing follows a non-zero exit."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_replica_worker.py")]
    res = _children.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("identical ok") == 2 and res.stdout.count("caught (named)") == 2, res.stdout[-2000:]


def test_check_replicas_of_one_process_returns_at_once():
    _, A = _engine("f32")
    assert A.world == 1 and A.check_replicas() is None
