"""CPU tests of the checkpoint's host side: the digest's NumPy restatement (tests/_digest_np.py) against the word-by-word Python-integer
form and committed known answers, its two algebraic properties (position-dependent; pieces add up), and the file packing -- a fabricated
state through vbnn_amd.t7file and back bit for bit, a RandomState restored from the file, the refusals. No engine, no GPU."""
import json
import os

import numpy as np
import pytest

from tests import _digest_np as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "digest_kat.json")


def _patterns(n, seed=7):
    """n random 32-bit patterns with the awkward floats among them: NaNs (quiet, signalling, negative), -0.0, denormals, infinities."""
    w = np.random.RandomState(seed).randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00000, 0x7f800001, 0xffc12345, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0],
                       dtype=np.uint32)
    k = min(n, special.size)
    if k:
        w[np.random.RandomState(seed + 1).permutation(n)[:k]] = special[:k]
    return w


@pytest.mark.parametrize("n", [0, 1, 2, 5, 1000])
@pytest.mark.parametrize("index0", [0, 3, (1 << 32) - 1 - 1001])      # (one below the last legal start: the test also shifts by one)
def test_the_numpy_form_is_the_word_by_word_form(n, index0):
    w = _patterns(n)
    assert D.digest(w, index0) == D.digest_py(w, index0)
    z = np.zeros(n, dtype=np.uint32)                                  # all-zero words still carry their positions
    assert D.digest(z, index0) == D.digest_py(z, index0)
    if n:
        assert D.digest(z, index0) != 0 and D.digest(z, index0) != D.digest(z, index0 + 1)
    else:
        assert D.digest(w, index0) == 0


def test_float_bit_patterns_are_digested_as_bits():
    f = np.array([np.nan, -0.0, 0.0, 1e-45, -1e-40, np.inf, 1.5], dtype=np.float32)
    assert D.digest(f) == D.digest_py(f) == D.digest(f.view(np.uint32))
    g = f.copy()
    g[1] = 0.0                                                         # -0.0 == 0.0 as floats, not as bits
    assert D.digest(g) != D.digest(f)
    h = f.view(np.uint32).copy()
    h[0] ^= 1                                                          # another NaN payload
    assert D.digest(h) != D.digest(f)


def test_known_answers():
    kat = json.load(open(KAT))
    assert len(kat["cases"]) >= 4
    for c in kat["cases"]:
        w = np.array(c["words"], dtype=np.uint32)
        assert D.digest(w, c["index0"]) == int(c["digest"], 16), c
        assert D.digest_py(w, c["index0"]) == int(c["digest"], 16), c
    assert D.mix_py(0) == 0 and int(D.mix(np.array([1], dtype=np.uint64))[0]) == D.mix_py(1) == int(kat["mix_of_1"], 16)


def test_swapping_two_unequal_words_changes_the_digest():
    w = _patterns(64)
    for i, j in [(0, 1), (3, 60), (17, 18)]:
        assert w[i] != w[j]
        s = w.copy()
        s[i], s[j] = w[j], w[i]
        assert D.digest(s) != D.digest(w)
    assert D.digest(w, 1) != D.digest(w, 0)


@pytest.mark.parametrize("cut", [0, 1, 3, 4, 500, 999, 1000])
def test_the_pieces_of_a_buffer_add_up(cut):
    w = _patterns(1000, seed=11)
    whole = D.digest(w, 40)
    assert (D.digest(w[:cut], 40) + D.digest(w[cut:], 40 + cut)) & D.M64 == whole
    a, b = sorted((cut, 321))
    parts = D.digest(w[:a], 40) + D.digest(w[a:b], 40 + a) + D.digest(w[b:], 40 + b)
    assert parts & D.M64 == whole


def test_the_position_limit():
    with pytest.raises(ValueError):
        D.digest(np.zeros(2, dtype=np.uint32), (1 << 32) - 2)
    D.digest(np.zeros(1, dtype=np.uint32), (1 << 32) - 2)


# ---- the file: host-only packing
def _fabricated_state(seed=5):
    r = np.random.RandomState(seed)
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    layers = [{"means": f(24, 20), "lvars": f(24, 20), "bias": f(24)}, {"means": f(16, 24), "lvars": f(16, 24), "bias": f(16)}]
    layers[0]["means"][0, :4] = np.array([np.nan, -0.0, 1e-45, np.inf], dtype=np.float32)
    adam = [{"mean": {"t": 3, "m": f(24, 20), "v": f(24, 20)}, "var": {"t": 3, "m": f(24, 20), "v": f(24, 20)}}, {}]
    masks = [(r.rand(24, 20) < 0.5).astype(np.uint8), (r.rand(16, 24) < 0.5).astype(np.uint8)]
    dig = {"layers": [{k: (1 << 63) + 12345 + i for i, k in enumerate(l)} for l in layers], "weight3": (1 << 64) - 1, "bias3": 0,
           "adam": [{"mean": {"m": (1 << 63), "v": (1 << 53) + 1}, "var": {"m": 7, "v": (1 << 63) - 1}}, {}],
           "held": {"masks": [0x8000000000000001, 0xfedcba9876543210]}}
    return {"format": "vbnn_amd.checkpoint", "version": 1, "layers": layers, "weight3": f(5, 16), "bias3": f(5), "adam": adam,
            "draw": 17, "seed": (1 << 64) - 59, "held": {"masks": masks, "counts": [int(m.sum()) for m in masks]}, "digests": dig,
            "arch": {"sizes": [20, 24, 16], "n_classes": 5, "criterion": "nll", "dtype": "f32", "mode": "lrt"}}


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (path, sorted(a), sorted(b) if isinstance(b, dict) else type(b))
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (path, a.dtype, getattr(b, "dtype", None))
        assert a.tobytes() == b.tobytes(), path                        # bit for bit: NaN payloads and -0.0 included
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


def test_a_fabricated_state_goes_through_the_file_bit_for_bit(tmp_path):
    from vbnn_amd import checkpoint as ck
    state = _fabricated_state()
    rng = np.random.RandomState(3)
    rng.standard_normal(3)                                             # an odd count: the Gaussian cache is in use
    rng.permutation(10)
    trainer = {"epoch": 4, "indices": list(range(0, 600, 100)), "rng": ck.rng_state_table(rng)}
    opt = {"hidden": [24, 16], "input_size": 20, "n_classes": 5, "B": 1e6, "seed": 3, "dtype": "f32", "geometry": (4, 5),
           "state": {"learningRate": 1e-3}, "checkpoint": True, "nothing": None}
    path = str(tmp_path / "model")
    ck.write_checkpoint(path, opt, state, trainer)
    table = ck.read_checkpoint(path)
    assert table["format"] == "vbnn_amd.checkpoint" and table["version"] == 1
    _same(state, table["engine"])
    _same(state["arch"], table["arch"])
    assert table["opt"]["hidden"] == [24, 16] and table["opt"]["geometry"] == [4, 5] and "nothing" not in table["opt"]
    assert table["opt"]["state"] == {"learningRate": 1e-3} and table["opt"]["checkpoint"] is True
    assert table["trainer"]["epoch"] == 4 and table["trainer"]["indices"].tolist() == trainer["indices"]
    key = table["trainer"]["rng"]["key"]
    assert key.dtype == np.int64 and key.shape == (624,) and (key.astype(np.uint32) == rng.get_state()[1]).all()
    # as any Torch7 user reads it: the digests are LongTensors of the uint64's bits, no number above 2^53 anywhere
    from vbnn_amd import t7file
    raw = t7file.load(path)
    d = raw["engine"]["digests"]["weight3"]
    assert isinstance(d, np.ndarray) and d.dtype == np.int64 and d.tolist() == [-1]
    assert raw["engine"]["seed"].view(np.uint64).tolist() == [(1 << 64) - 59]
    assert raw["engine"]["held"]["masks"][0].dtype == np.uint8
    # the previous file survives as .old
    ck.write_checkpoint(path, opt, state, None)
    assert os.path.isfile(path + ".old") and "trainer" in ck.read_checkpoint(path + ".old") and "trainer" not in ck.read_checkpoint(path)


def test_a_restored_random_state_continues_the_sequence(tmp_path):
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import utils as u
    rng = np.random.RandomState(3)
    for _ in range(5):
        u.shuffle(range(6), rng)
    rng.standard_normal(1)                                             # leaves a cached Gaussian behind
    path = str(tmp_path / "model")
    ck.write_checkpoint(path, {}, _fabricated_state(), {"epoch": 5, "indices": [0, 100], "rng": ck.rng_state_table(rng)})
    want = [u.shuffle(range(6), rng) for _ in range(3)] + [float(rng.standard_normal())]
    got_rng = ck.rng_from_table(ck.read_checkpoint(path)["trainer"]["rng"], np.random.RandomState(99))
    got = [u.shuffle(range(6), got_rng) for _ in range(3)] + [float(got_rng.standard_normal())]
    assert got == want


def test_an_unknown_version_is_refused(tmp_path):
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import t7file
    path = str(tmp_path / "model")
    ck.write_checkpoint(path, {}, _fabricated_state(), None)
    raw = t7file.load(path)
    raw["version"] = 2
    t7file.save(path, raw)
    with pytest.raises(ck.CheckpointError, match="version 2"):
        ck.read_checkpoint(path)
    state = _fabricated_state()
    state["version"] = 0
    with pytest.raises(ck.CheckpointError, match="version 0"):
        ck.unpack_state(ck.pack_state(state))


def test_a_file_that_is_no_checkpoint_table_is_refused(tmp_path):
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import t7file
    path = str(tmp_path / "means")
    t7file.save(path, np.zeros(7, dtype=np.float32))                  # what Main.save writes next to it
    with pytest.raises(ck.CheckpointError, match="not a vbnn_amd.checkpoint"):
        ck.read_checkpoint(path)
    t7file.save(path, {"format": "something else", "version": 1})
    with pytest.raises(ck.CheckpointError, match="not a vbnn_amd.checkpoint"):
        ck.read_checkpoint(path)
