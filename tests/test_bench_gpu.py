"""bench.py as the driver runs it: a plain `--gpus 1 --steps K --warmup W` line carries the headline alone, from exactly K timed
steps; `--dump-outputs DIR` leaves the last timed step's outputs, the same in every run with the same arguments; `--full` adds
what is measured beside the headline."""
import json
import os
import sys

import numpy as np
import pytest

from tests import _children

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}


def _bench(*args):
    res = _children.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                        timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _small_step_at(draw):
    """A fresh engine of bench.py's small configuration (same seed, same minibatch) running ONE step that draws the noise of
    `draw`: what the bench's step number `draw` computes, since a bench step changes no parameter."""
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    eng = FusedMLP(dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=784, hidden=[400, 400], n_classes=10,
                        fuse_kl=True))
    x = torch.empty(256, 784, dtype=torch.float32, device="cuda")
    fill_normal(x, 3, L.STREAM_DATA, 0, 0, row0=0)
    t = eng.synthetic_targets(x, 0)
    eng.prepare()
    eng.draw = draw - 1
    eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
    loss, correct = eng.loss_and_accuracy()
    got = {"loss.npy": np.array([loss]), "correct.npy": np.array([float(correct)]),
           "final_gradWeight.npy": eng.gradWeight3, "final_gradBias.npy": eng.gradBias3}
    for li, v in enumerate(eng.vb):
        got.update({f"layer{li}_gradWeight.npy": v.gradWeight, f"layer{li}_gradSum.npy": v.gradSum, f"layer{li}_gradBias.npy": v.gradBias})
    return {k: (a.reshape(-1).cpu().numpy() if hasattr(a, "cpu") else a) for k, a in got.items()}


def test_plain_line_times_exactly_the_steps_asked_for_and_dumps_the_same_outputs_every_run(tmp_path):
    W, K = 2, 7
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _bench("--config", "small", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(d))
        assert HEADLINE <= set(out) and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert out["steps"] == K and len(out["config"]["repeats_wall_ms"]) == 1 and out["config"]["warmup_steps_run"] >= W
        assert not {"roofline", "box", "train_step", "cpu_baseline", "reporting_config", "deep_config"} & set(out), sorted(out)
        files = sorted(os.listdir(d))
        assert {"loss.npy", "correct.npy", "layer0_gradWeight.npy", "final_gradBias.npy"} <= set(files), files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert float(arrays["loss.npy"][0]) == pytest.approx(out["config"]["loss"], abs=1e-5)
        runs.append(arrays)
    for f, a in runs[0].items():
        np.testing.assert_allclose(runs[1][f], a, rtol=1e-6, atol=0, err_msg=f)
    # the dump is the LAST timed step's: W warm-up draws (the longer warm-up sets the counter back), then K timed ones -- the
    # step of draw W + K, and not its neighbour (every draw has its own noise; the small configuration's blocks are whole)
    last, before = _small_step_at(W + K), _small_step_at(W + K - 1)
    assert sorted(last) == sorted(runs[0])
    for f, a in runs[0].items():
        scale = float(np.abs(last[f]).max()) or 1.0
        np.testing.assert_allclose(a, last[f], rtol=0, atol=1e-6 * scale, err_msg=f)
    for f in ("layer0_gradWeight.npy", "layer1_gradSum.npy", "final_gradWeight.npy"):
        assert np.abs(before[f] - last[f]).max() > 1e-4 * np.abs(last[f]).max(), f


def test_full_line_carries_what_is_measured_beside_the_headline():
    out = _bench("--config", "small", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert HEADLINE <= set(out) and len(out["config"]["repeats_wall_ms"]) == 7
    assert out["roofline"]["timed_region_kernels_ms"] and out["box"]["mfma_clock_ghz"] > 0
    assert out["train_step"]["ms_per_train_step"] > 0 and out["config"]["probed_block_ms"] > 0
