#!/usr/bin/env python3
"""What a checkpoint costs: vbnn_digest and FusedMLP.state_dict / save / load / load_state_dict.

    python tools/checkpoint_bench.py [--kernel-reps 10] [--rounds 5] [--wall-rounds 3] [--out profiles/checkpoint_bench.json]

The protocol of tools/quantile_predict_bench.py: blocks of calls between HIP events (never one launch on its own), the variants
interleaved round by round, medians of the rounds, the box's held clock and stream-copy rate (vbnn_box_calibrate) beside every figure,
and the outputs asserted against the NumPy restatement (tests/_digest_np.py) before anything is timed.

(a) vbnn_digest on one 4096 x 4096 fp32 tensor (67 MB) and its share of the stream-copy rate by the bytes it must move (n_words x 4,
    nothing written) -- beside the MSE ACCUMULATE moments kernel at R 4096 x D 4096 timed TWICE in the same process: that kernel's
    share is the yardstick, its own spread the allowance. HIT or MISS.
(b) vbnn_digest on the tensors of the 784-4096-4096-10 network's two VB layers: the six parameter tensors (means, lvars, bias: 160 MB)
    and the same with Adam's m and v of means and lvars, what state_dict digests after a training step (480 MB) -- one launch per tensor.
(c) the wall time (host clock, device-synchronised) of state_dict, save, load and load_state_dict on that network after one training
    step. Recorded, not judged.
Whatever is measured is written down, including where the kernel misses the byte-derived figure."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block_ms(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _interleaved(fns, n, rounds):
    """median over `rounds` of ms per call, the variants alternating round by round (one warm-up round)."""
    times = {k: [] for k in fns}
    for rnd in range(rounds + 1):
        for k, fn in fns.items():
            ms = _block_ms(fn, n)
            if rnd:
                times[k].append(ms)
    return {k: statistics.median(v) for k, v in times.items()}


def _box(L, h):
    box = L.BoxInfo()
    L.check(L.lib().vbnn_box_calibrate(h, C.byref(box)))
    return box, {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
                 "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus}


def digest_point(a, box):
    import torch
    from tests import _digest_np as D
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    f32 = dict(dtype=torch.float32, device="cuda")
    bw = box.hbm_TBps * 1e12
    R = Dm = 4096
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn(2, R, Dm, generator=g, **f32)               # two draws for the moments kernel; the digest reads the first
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    n = R * Dm

    def kernel():
        L.check(lib.vbnn_digest(h, _p(y), n, 0, _p(out)))
    kernel()
    assert int(out.cpu()[0]) & D.M64 == D.digest(y[0].cpu().numpy()), "vbnn_digest against the restatement"
    view = y.view(-1)[3:3 + 1000003]                             # off the 16-byte boundary, a ragged tail
    out.zero_()
    L.check(lib.vbnn_digest(h, _p(view), view.numel(), 9, _p(out)))
    assert int(out.cpu()[0]) & D.M64 == D.digest(view.cpu().numpy(), 9), "vbnn_digest on an unaligned view"
    # the MSE ACCUMULATE moments kernel, one middle draw, twice (the family's yardstick: tools/gauss_predict_bench.py)
    t = torch.randn(R, Dm, generator=g, **f32)
    st = torch.empty(R, 2 * Dm + 2, **f32)
    om = {k: torch.empty((R, Dm) if k in ("mean", "var") else (R,), **f32) for k in ("mean", "var", "row_var", "row_sq_err", "row_log_lik")}
    tot = torch.zeros(4, dtype=torch.float64, device="cuda")
    mm = L.MomentsArgs(y=_p(y), ld_y=Dm, target=_p(t), ld_t=Dm, R=R, D=Dm, S=2, noise_var=0.1, state=_p(st), form=L.MOMENTS_ACCUMULATE,
                       mean=_p(om["mean"]), var=_p(om["var"]), ld_out=Dm, row_var=_p(om["row_var"]), row_sq_err=_p(om["row_sq_err"]),
                       row_log_lik=_p(om["row_log_lik"]), totals=_p(tot))

    def mse_draw(s=1):
        mm.draw, mm.y = s, C.c_void_p(y.data_ptr() + 4 * s * R * Dm)
        L.check(lib.vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    ms = _interleaved({"kernel": kernel, "mse_first": mse_draw, "mse_second": mse_draw}, a.kernel_reps, a.rounds)
    rd = 4.0 * R * Dm
    nbytes, bm = rd, (1 + 1 + 2 + 2) * rd
    share = lambda nb, t_ms: nb / (t_ms * 1e-3) / bw
    sk, s1, s2 = share(nbytes, ms["kernel"]), share(bm, ms["mse_first"]), share(bm, ms["mse_second"])
    allowance = abs(s1 - s2)
    return {"n_words": n, "bytes_moved": int(nbytes), "kernel_us": round(ms["kernel"] * 1e3, 2),
            "byte_floor_us": round(nbytes / bw * 1e6, 2), "GBps": round(nbytes / (ms["kernel"] * 1e-3) / 1e9, 1),
            "fraction_of_stream_copy": round(sk, 4), "mse_accumulate_us": [round(ms["mse_first"] * 1e3, 2), round(ms["mse_second"] * 1e3, 2)],
            "mse_fraction_of_stream_copy": [round(s1, 4), round(s2, 4)], "allowance": round(allowance, 4),
            "verdict": "HIT" if sk >= min(s1, s2) - allowance else "MISS"}


def engine_points(a, box):
    import torch
    from tests import _digest_np as D
    from vbnn_amd import checkpoint as ck
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    bw = box.hbm_TBps * 1e12
    N = 256
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=784, hidden=[4096, 4096], n_classes=10, type="vb",
               fuse_kl=True, state={"learningRate": 1e-3}, meanState={"learningRate": 1e-4}, varState={"learningRate": 5e-2})
    eng = FusedMLP(opt)
    x = torch.empty(N, 784, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    eng.prepare()
    eng.resetGradients(); eng.sample(); eng.run(x, t); eng.update(opt)       # one step: Adam's moments exist
    items = eng._state_tensors()
    params = [tt for p, tt in items if p[0] == "layers"]
    vb_all = [tt for p, tt in items if p[0] in ("layers", "adam")]
    assert len(params) == 6 and len(vb_all) == 14
    got = ck.digests(params[:1] + params[2:3], eng.ctx)
    assert got == [D.digest(params[0].cpu().numpy()), D.digest(params[2].cpu().numpy())], "engine digests against the restatement"
    lib, h = ck.L.lib(), eng.ctx.h
    out = torch.zeros(len(vb_all), dtype=torch.int64, device="cuda")

    def run(ts):
        def go():
            for i, tt in enumerate(ts):
                ck.L.check(lib.vbnn_digest(h, C.c_void_p(tt.data_ptr()), tt.numel(), 0, C.c_void_p(out.data_ptr() + 8 * i)))
        return go
    ms = _interleaved({"six_parameter_tensors": run(params), "vb_layers_with_moments": run(vb_all)}, a.kernel_reps, a.rounds)
    res = {"net": "784-4096-4096-10", "dtype": "bf16", "digest": {}}
    for k, ts in (("six_parameter_tensors", params), ("vb_layers_with_moments", vb_all)):
        nb = sum(4 * tt.numel() for tt in ts)
        res["digest"][k] = {"tensors": len(ts), "bytes_moved": nb, "us": round(ms[k] * 1e3, 2), "byte_floor_us": round(nb / bw * 1e6, 2),
                            "fraction_of_stream_copy": round(nb / (ms[k] * 1e-3) / bw, 4)}
    # ---- wall times (host clock around device-synchronised calls)
    wall = {k: [] for k in ("state_dict", "save", "load", "load_state_dict")}

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        wall[key].append(time.perf_counter() - t0)
        return r
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model")
        for _ in range(a.wall_rounds):
            state = timed("state_dict", eng.state_dict)
            timed("save", lambda: eng.save(path))
            other = timed("load", lambda: FusedMLP.load(path))
            timed("load_state_dict", lambda: other.load_state_dict(state))
            for v, w in zip(eng.vb, other.vb):
                assert torch.equal(v.means, w.means) and torch.equal(v.lvars, w.lvars)
            del other
        res["file_bytes"] = os.path.getsize(path)
    res["state_bytes"] = sum(tt.numel() * tt.element_size() for _, tt in items)
    res["wall_ms"] = {k: round(statistics.median(v) * 1e3, 1) for k, v in wall.items()}
    res["wall_note"] = "save and load each include a state_dict / load_state_dict; host clock, median of the rounds, recorded not judged"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=10, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wall-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    box, box_d = _box(L, Context.get().h)
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "wall_rounds": a.wall_rounds, "box": box_d}
    out["digest_4096x4096"] = digest_point(a, box)
    out["engine"] = engine_points(a, box)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
