#!/usr/bin/env python3
"""What the sampling-free predictive (FusedMLP.predict_analytic over vbnn_amd/csrc/propagate.hip) costs, and what it gives up.

    python tools/analytic_predict_bench.py [--reps 5] [--rounds 5] [--out profiles/analytic_predict_bench.json]
    python tools/analytic_predict_bench.py --section kernel | engine | gap        (one section, in this process)

Each section runs as a child process under a time limit (--timeout seconds), the sections one after the other; nothing more is
started after one that failed. Timing follows the other predictive benches: blocks of calls between HIP events, the variants
interleaved in one process, the median of `rounds` rounds after a warm-up round, the box's clock and stream-copy rate
(vbnn_box_calibrate) recorded beside them; outputs are asserted against the NumPy restatement (tests/_propagate_np.py) before
anything is timed: the kernel's first 64 rows against the fp32 op sequence; every engine point's first 4 rows stage by stage from
the device's own stage inputs within one stage's bound, and as a whole network within the bound carried through all layers.

(kernel) vbnn_relu_moments alone at 4096 x 4096, fp32 in (m, v1, v2), bf16 out (a, q, c), beside the MSE ACCUMULATE moments kernel
(one middle draw at R = D = 4096) timed TWICE in the same process. Expectation: that kernel's share of the stream-copy rate, by
the bytes each must move; allowance: the spread of its two timings. Hit or miss is written down.
(engine) predict_analytic against predict_regression (S = 30) at 784-400-400 fp32 D = 10 with 100 rows and at BASELINE configs[4]
(bf16), and against predict_classes (S = 30) at 784-4096-4096-10 bf16 with 100 and 3000 rows. Expectation by flops: three single
GEMMs per hidden layer (two for the first) against S dual ones; the ratio found is recorded beside it.
(gap) the approximation gap, recorded and not judged: on the 784-64-48-10 network trained three epochs on data.synthetic_digits
(the README's accuracy recipe) and on a 2-hidden-layer "mse" toy with random parameters -- |analytic mean - MC mean| in units of the
MC standard error at S = 1024 (max and mean), the variance ratio, and accuracy / NLL of the classifier under both routes."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("kernel", "engine", "gap")


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


# ------------------------------------------------------------------------------------------------ (kernel)
def kernel_section(a):
    import numpy as np
    import torch
    from tests import _propagate_np as P
    from tests._update_np import bf16_round
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    lib, h = L.lib(), Context.get().h
    box, box_d = _box(L, h)
    N = O = 4096
    g = torch.Generator(device="cuda").manual_seed(5)
    f32 = dict(dtype=torch.float32, device="cuda")
    m = torch.randn(N, O, generator=g, **f32) * 3
    v1, v2 = torch.rand(N, O, generator=g, **f32) + 0.01, torch.rand(N, O, generator=g, **f32) * 0.5
    outs = [torch.zeros(N, O, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    ra = L.ReluMomentsArgs(m=_p(m), ld_m=O, v1=_p(v1), v2=_p(v2), ld_v=O, N=N, O=O, a=_p(outs[0]), q=_p(outs[1]), c=_p(outs[2]), ld_out=O)
    relu = lambda: L.check(lib.vbnn_relu_moments(h, L.BF16, C.byref(ra)))
    relu()
    rows = 64                                                  # asserted against the restatement on the first rows
    mh, v1h, v2h = (t[:rows].cpu().numpy() for t in (m, v1, v2))
    want = P.relu_moments32(mh, v1h, v2h)
    sc = P.relu_scale(mh, v1h + v2h)
    for k, (o, w) in enumerate(zip(outs, want)):
        w = bf16_round(w).astype(np.float64)
        d = np.abs(o[:rows].float().cpu().numpy() - w)
        assert (d <= 4 * P.EPS_RELU * sc ** (1 if k == 0 else 2) + np.abs(w) * 2.0 ** -7).all(), "aqc"[k]
    # the MSE ACCUMULATE moments kernel, one middle draw
    R = D = 4096
    y, t = torch.randn(R, D, generator=g, **f32), torch.randn(R, D, generator=g, **f32)
    state = torch.zeros(R, 2 * D + 2, **f32)
    ma = L.MomentsArgs(y=_p(y), ld_y=D, target=_p(t), ld_t=D, R=R, D=D, S=8, noise_var=0.1, state=_p(state), form=L.MOMENTS_ACCUMULATE,
                       draw=1, ld_out=D)
    mom = lambda: L.check(lib.vbnn_predict_moments(h, C.byref(ma)))
    ma.draw = 0
    mom()
    ma.draw = 1
    ms = _interleaved({"moments_1": mom, "relu_moments": relu, "moments_2": mom}, a.kernel_reps, a.rounds)
    rate = box.hbm_TBps * 1e12
    relu_bytes = N * O * (3 * 4 + 3 * 2)
    mom_bytes = 4.0 * R * D * 6                                # state in (2), y, t, state out (2)
    frac = lambda nbytes, t_ms: nbytes / (t_ms * 1e-3) / rate
    f1, f2, fr = frac(mom_bytes, ms["moments_1"]), frac(mom_bytes, ms["moments_2"]), frac(relu_bytes, ms["relu_moments"])
    expect, allow = min(f1, f2), abs(f1 - f2)
    return {"shape": [N, O], "in": "fp32 m, v1, v2", "out": "bf16 a, q, c", "relu_moments_us": round(ms["relu_moments"] * 1e3, 2),
            "relu_moments_bytes": int(relu_bytes), "relu_moments_fraction_of_stream_copy": round(fr, 4),
            "moments_accumulate_us": [round(ms["moments_1"] * 1e3, 2), round(ms["moments_2"] * 1e3, 2)], "moments_bytes": int(mom_bytes),
            "moments_fraction_of_stream_copy": [round(f1, 4), round(f2, 4)], "expectation": round(expect, 4), "allowance": round(allow, 4),
            "verdict": "hit" if fr >= expect - allow else "miss", "box": box_d}


# ------------------------------------------------------------------------------------------------ (engine)
ENGINE_POINTS = [
    dict(name="launch_bound", input_size=784, hidden=[400, 400], W=10, dtype="f32", R=100, criterion="mse"),
    dict(name="configs4", input_size=4096, hidden=[4096] * 8, W=4096, dtype="bf16", R=4096, criterion="mse"),
    dict(name="wide_classifier_100", input_size=784, hidden=[4096, 4096], W=10, dtype="bf16", R=100, criterion="nll"),
    dict(name="wide_classifier_3000", input_size=784, hidden=[4096, 4096], W=10, dtype="bf16", R=3000, criterion="nll"),
]


def _assert_against_restatement(eng, x, mean, var, rows):
    """predict_analytic's outputs of the first `rows` rows against tests/_propagate_np.py, two ways. Stage by stage, from the DEVICE's
    own input moments of every stage whose buffers the call left intact (the ping-pong pairs keep the last two layers of a deep
    network, every layer of a two-layer one) and of the final Linear: one stage's products, ReLU moments and rounding within ONE
    stage's bound (4e-6 sum |a||b| per product, 4 EPS_RELU, a rounding boundary within that) -- the tight check at this point's
    shapes. And the whole network from x within the bound carried through all layers, which over many bf16 layers grows past the
    values themselves (every rounding point may flip): asserted, and its size recorded so that nobody reads more into it."""
    import numpy as np
    from tests import _propagate_np as P
    h = lambda t: t.detach().float().cpu().numpy().astype(np.float64)
    dtype, nl, act = eng.dtype, len(eng.vb), eng._ana_bufs.act
    rnd = P.rounder(dtype)
    ps = [(h(v.means), h(v.lvars), h(v.bias)) for v in eng.vb]
    layers = [P.operands(mu, lv, dtype) for mu, lv, _ in ps]
    w3, w3sq = P.final_operands(h(eng.weight3), dtype)
    intact = [all(act[k] is not act[j] for k in range(j + 1, nl + 1)) for j in range(nl + 1)]
    worst, stages = 0.0, []

    def held(got, want, bound, what):
        nonlocal worst
        d = np.abs(got - want)
        assert (d <= bound).all(), (what, float((d - bound).max()), float(bound.max()))
        worst = max(worst, float((d / np.where(bound > 0, bound, 1.0)).max()))

    def moments(b, cols):
        z = np.zeros((rows, cols))
        return tuple(h(t.t[:rows, :cols]) if t is not None else z for t in (b.a, b.q, b.c))
    for li, v in enumerate(eng.vb):
        if not (intact[li] and intact[li + 1]):
            continue
        mom = moments(act[li], v.I)
        (a, q, c), (ea, eq, ec) = P.layer64(mom, (np.zeros_like(mom[0]),) * 3, layers[li], ps[li][2], li == 0, rnd)
        got = moments(act[li + 1], v.O)
        held(got[0], a, ea, f"layer {li}: a")
        held(got[2], c, ec, f"layer {li}: c")
        if li < nl - 1:
            held(got[1], q, eq, f"layer {li}: q")
        stages.append(li)
    a, _, c = moments(act[nl], eng.sizes[-1])
    z = np.zeros_like(a)
    wm, wv, em, ev = P.final64(a, c, z, z, w3, w3sq, h(eng.bias3))
    held(h(mean[:rows]), wm, em, "final mean")
    held(h(var[:rows]), wv, ev, "final variance")
    stage_worst = worst
    wm, wv, em, ev = P.propagate64(h(x[:rows]), layers, [p[2] for p in ps], w3, w3sq, h(eng.bias3), dtype)
    dm, dv = np.abs(h(mean[:rows]) - wm), np.abs(h(var[:rows]) - wv)
    assert (dm <= em).all() and (dv <= ev).all(), ("whole network", float((dm / em).max()), float((dv / ev).max()))
    return {"rows": rows, "outputs": int(wm.size), "stages_checked_from_device_inputs": stages + ["final"],
            "max_stage_error_over_bound": round(stage_worst, 4), "whole_network_max_mean_error": float(dm.max()),
            "whole_network_max_variance_error": float(dv.max()), "whole_network_largest_mean_bound": float(em.max()),
            "whole_network_largest_variance_bound": float(ev.max()), "largest_mean": float(np.abs(wm).max()),
            "largest_variance": float(wv.max())}


def engine_point(p, a):
    import torch
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    S, R, W = 30, p["R"], p["W"]
    opt = dict(var_init=1e-3, B=1e6, S=1, mode="lrt", dtype=p["dtype"], seed=3, input_size=p["input_size"], hidden=p["hidden"],
               n_classes=W, criterion=p["criterion"], type="vb", testSamples=S)
    eng = FusedMLP(opt)
    eng.prepare()
    x = torch.empty(R, p["input_size"], dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    if p["criterion"] == "mse":
        fns = {"sampled": lambda: eng.predict_regression(x), "analytic": lambda: eng.predict_analytic(x)}
        ana, mc = eng.predict_analytic(x), eng.predict_regression(x)
        am, mm = ana.mean, mc.mean
    else:
        fns = {"sampled": lambda: eng.predict_classes(x, keep_probs=False), "analytic": lambda: eng.predict_analytic(x, keep_probs=False)}
        ana, mc = eng.predict_analytic(x), eng.predict_classes(x, keep_draws=True)
        am, mm = ana.logit_mean, mc.draws.mean(0)
    assert bool(torch.isfinite(am).all()) and ana.chunks == 1 and mc.chunks == 1
    # before timing: the analytic outputs of the first rows against the float64 restatement within ITS bound (the GPU tests'
    # check, at this point's shapes); the sampled route's mean beside it is recorded, not judged (section `gap` measures that)
    av = ana.var if p["criterion"] == "mse" else ana.logit_var
    checked = _assert_against_restatement(eng, x, am, av, rows=4)
    spread = float((am - mm).abs().max() / mm.abs().max().clamp(min=1e-6))
    sizes = [p["input_size"]] + p["hidden"]
    pairs = [sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1)]
    flops_analytic = sum((2 if i == 0 else 3) * w for i, w in enumerate(pairs)) + 2 * sizes[-1] * W
    flops_sampled = S * (sum(2 * w for w in pairs) + sizes[-1] * W)
    ms = _interleaved(fns, a.reps, a.rounds)
    return {"point": p["name"], "net": "-".join(map(str, sizes + [W])), "dtype": p["dtype"], "criterion": p["criterion"], "R": R, "S": S,
            "sampled_entry": "predict_regression" if p["criterion"] == "mse" else "predict_classes", "sampled_ms": round(ms["sampled"], 4),
            "analytic_ms": round(ms["analytic"], 4), "analytic_over_sampled": round(ms["analytic"] / ms["sampled"], 4),
            "expected_by_flops": round(flops_analytic / flops_sampled, 4), "asserted_against_restatement": checked,
            "sampled_mean_difference_over_max_mean": round(spread, 4)}


# ------------------------------------------------------------------------------------------------ (gap)
def _gap(am, av, draws):
    """am, av: analytic mean and variance; draws: S x ... Monte-Carlo outputs. Units of the MC standard error of the mean."""
    S = draws.shape[0]
    d = draws.double()
    mm, mv = d.mean(0), d.var(0, unbiased=True)
    se = (mv / S).sqrt().clamp(min=1e-30)
    z = (am.double() - mm).abs() / se
    ratio = av.double() / mv.clamp(min=1e-30)
    return {"S": S, "max_mean_gap_in_se": round(float(z.max()), 3), "mean_mean_gap_in_se": round(float(z.mean()), 3),
            "variance_ratio_mean": round(float(ratio.mean()), 4), "variance_ratio_median": round(float(ratio.median()), 4),
            "variance_ratio_min": round(float(ratio.min()), 4), "variance_ratio_max": round(float(ratio.max()), 4)}


def gap_section(a):
    import tempfile
    import numpy as np
    import torch
    from vbnn_amd import data, train
    from vbnn_amd.engine import FusedMLP
    S = 1024
    out = {}
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    with tempfile.TemporaryDirectory() as d:
        opt = train.default_opt(network_name=os.path.join(d, "exp"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                                trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32", log=False,
                                state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
        m = train.Main(opt)
        m.run(trainSet, testSet, epochs=3)
        inputs, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
        x, t = m._to_device(inputs, targets)
        net = m.net
        mc = net.predict_classes(x, targets=t, S=S, keep_draws=True)
        ana = net.predict_analytic(x, targets=t, S=S)
        rec = _gap(ana.logit_mean, ana.logit_var, mc.draws)
        rec.update(net="784-64-48-10", dtype="f32", data="synthetic_digits(2000, 500, seed=3, noise=2.0), 3 epochs, the 500 test rows",
                   quantity="logits", sampled={"accuracy": mc.accuracy, "nll": mc.nll}, analytic={"accuracy": ana.accuracy, "nll": ana.nll},
                   mean_abs_probability_difference=float((ana.probs - mc.probs).abs().mean()),
                   max_abs_probability_difference=float((ana.probs - mc.probs).abs().max()))
        out["classifier"] = rec
    g = np.random.default_rng(11)
    eng = FusedMLP(dict(var_init=1e-2, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=16, hidden=[32, 32], n_classes=2,
                        criterion="mse", type="vb", testSamples=2))
    for v in eng.vb:
        v.lvars.copy_(torch.from_numpy(np.log(g.uniform(0.005, 0.05, (v.O, v.I))).astype(np.float32)).cuda())
        v.bias.copy_(torch.from_numpy((g.standard_normal(v.O) * 0.1).astype(np.float32)).cuda())
    eng.prepare()
    x = torch.from_numpy(g.standard_normal((256, 16)).astype(np.float32)).cuda()
    mc = eng.predict_regression(x, S=S, keep_draws=True)
    ana = eng.predict_analytic(x)
    rec = _gap(ana.mean, ana.var, mc.draws)
    rec.update(net="16-32-32-2", dtype="f32", data="random parameters (He means, variances uniform in [0.005, 0.05]), 256 normal rows",
               quantity="outputs")
    out["mse_toy"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=SECTIONS)
    ap.add_argument("--reps", type=int, default=5, help="engine calls per timed block")
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per section (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analytic_predict_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.section:
        if a.section == "kernel":
            res = kernel_section(a)
        elif a.section == "engine":
            res = [engine_point(p, a) for p in ENGINE_POINTS]
        else:
            res = gap_section(a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    out = {"reps": a.reps, "kernel_reps": a.kernel_reps, "rounds": a.rounds}
    for name in SECTIONS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--section", name, "--reps", str(a.reps),
               "--kernel-reps", str(a.kernel_reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(json.dumps({"section": name, "error": f"exit status {r.returncode}"}), flush=True)
            return r.returncode or 1                            # nothing more on the GPU after a failed section
        out[name] = json.loads(lines[-1][len("RESULT "):])
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
