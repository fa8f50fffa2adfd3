#!/usr/bin/env python3
"""What training under a held pruning mask (FusedMLP.hold_pruned) costs and what it buys.

    python tools/finetune_bench.py [--reps 30] [--rounds 4] [--steps 10] [--out profiles/finetune_bench.json]
    python tools/finetune_bench.py --skip-cost | --skip-recovery

(a) Cost, 784-4096-4096-10 bf16, minibatch 4096: the update sweep alone (vbnn_update against vbnn_update_masked on the SAME
tensors, both layers in one call, no extra matrix) and the whole training step (resetGradients, sample, run, update), unmasked
against a mask held at 50 / 90 / 98 %. One process, the variants interleaved call by call (sweep) or block by block (step), HIP
events on the engine's stream, medians; the unmasked sweep is timed TWICE per round and the spread of its two medians is the
allowance the comparison gets. By bytes the masked sweep moves 61 B per weight against 60 (the mask byte): 1.017x expected.
Quoted with the box's held clock and stream-copy rate (vbnn_box_calibrate), as the other pruning benches are.

(b) Recovery, the README's accuracy recipe (784-64-48-10 fp32, data.synthetic_digits(2000, 500, seed=3, noise=2.0), 3 epochs):
at 90 / 95 / 98 / 99 % of the weights pruned globally the MAP accuracy and NLL on the test set right after pruning, after 1 and
after 3 epochs under the held mask; beside them a gradual schedule to 98 % (50 -> 75 -> 90 -> 95 -> 98 %, one epoch each,
opt.prune_schedule). Whatever is measured is written down, including points where fine-tuning does not help."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def cost(a):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import _p
    opt = dict(var_init=1e-2, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=784, hidden=[4096, 4096], n_classes=10,
               type="vb", fuse_kl=True, state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-6),
               varState=dict(learningRate=1e-6))
    N = 4096
    x = torch.empty(N, 784, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)

    def engine():
        eng = FusedMLP(opt)
        for li, v in enumerate(eng.vb):                  # sigma varies per weight (the inputs of tools/prune_bench.py)
            z = torch.empty_like(v.lvars)
            nn.fill_normal(z, 3, L.STREAM_INIT, li, 7)
            v.lvars.copy_(float(torch.log(torch.tensor(1e-2))) + 0.75 * z)
        eng.prepare()
        return eng
    U, M = engine(), engine()
    lib, h = L.lib(), U.ctx.h
    box = L.BoxInfo()
    L.check(lib.vbnn_box_calibrate(h, C.byref(box)))
    W = sum(v.O * v.I for v in U.vb)
    fractions = (0.5, 0.9, 0.98)

    # ---- the sweep alone: U's own tensors, gradients as one step left them, Adam state of this tool
    U.resetGradients(); U.sample(); U.run(x, t); U.finish()
    state = [[torch.zeros_like(v.means) for _ in range(4)] for v in U.vb]
    masks = {q: [U.prune(fraction=q).mask(li).to(torch.uint8).contiguous() for li in range(len(U.vb))] for q in fractions}
    held = {q: sum(int(m.sum()) for m in ms) / W for q, ms in masks.items()}
    step_no = [0]

    def descs():
        step_no[0] += 1
        d = (L.UpdateDesc * len(U.vb))()
        for k, (v, (mm, vm, ml, vl)) in enumerate(zip(U.vb, state)):
            use_t = v.muT_s is not None and getattr(v, "use_muT", True)
            cfg = lambda lr: L.AdamCfg(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, lambda_=1.0, t=step_no[0])
            d[k] = L.UpdateDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, mu_s=v.mu_s.ptr, var_s=v.var_s.ptr, ld_w=v.mu_s.ld,
                                muT_s=v.muT_s.ptr if use_t else None, varT_s=v.varT_s.ptr if use_t else None,
                                ld_wT=v.muT_s.ld if v.muT_s else 0, stats=_p(v.stats), grad_mu=_p(v.gradWeight), grad_lv=_p(v.gradSum),
                                m_mu=_p(mm), v_mu=_p(vm), m_lv=_p(ml), v_lv=_p(vl), mu=cfg(1e-6), lv=cfg(1e-6), bias=_p(v.bias),
                                grad_bias=_p(v.gradBias), lr_bias=1e-6, B=U.B, log14=None, kl_add=1.0 if U.kl_in_update else 0.0)
        return d

    def sweep(q):
        d = descs()
        if q is None:
            return lambda: L.check(lib.vbnn_update(h, U.code, len(U.vb), d, None))
        ptrs = (C.c_void_p * len(U.vb))(*[m.data_ptr() for m in masks[q]])
        return lambda: L.check(lib.vbnn_update_masked(h, U.code, len(U.vb), d, ptrs, None))
    variants = [("unmasked", None), ("held_50", 0.5), ("held_90", 0.9), ("held_98", 0.98), ("unmasked_again", None)]
    times = {name: [] for name, _ in variants}
    for rep in range(a.reps + 3):
        for name, q in variants:                         # interleaved call by call
            ms = _event_ms(sweep(q))
            if rep >= 3:
                times[name].append(ms)
    sweep_ms = {name: statistics.median(v) for name, v in times.items()}
    base = sweep_ms["unmasked"]
    spread = abs(sweep_ms["unmasked_again"] - base) / base
    form = "flat" if not any(v.muT_s is not None and getattr(v, "use_muT", True) for v in U.vb) else "tiled"

    # ---- the whole training step, block by block: U unmasked, M under the mask of each fraction
    def block(eng):
        def run():
            for _ in range(a.steps):
                eng.resetGradients(); eng.sample(); eng.run(x, t); eng.update(opt)
        return run
    step_times = {name: [] for name, _ in variants}
    for rnd in range(a.rounds + 1):
        for name, q in variants:
            eng = U if q is None else M
            if q is not None:
                M.release_pruned()
                M.hold_pruned(M.prune(fraction=q))
            ms = _event_ms(block(eng)) / a.steps
            if rnd >= 1:
                step_times[name].append(ms)
    step_ms = {name: statistics.median(v) for name, v in step_times.items()}
    sbase = step_ms["unmasked"]
    return {
        "net": "784-4096-4096-10", "dtype": "bf16", "batch": N, "W": W, "sweep_form": form,
        "held_fraction": {f"held_{int(q * 100)}": round(held[q], 6) for q in fractions},
        "update_sweep_ms": {k: round(v, 5) for k, v in sweep_ms.items()},
        "update_sweep_over_unmasked": {k: round(v / base, 4) for k, v in sweep_ms.items()},
        "unmasked_spread": round(spread, 4), "expected_ratio_by_bytes": round(61 / 60, 4),
        "allowed_ratio": round(61 / 60 + spread, 4),
        "within_allowance": {k: bool(v / base <= 61 / 60 + spread) for k, v in sweep_ms.items() if k.startswith("held")},
        # (the unmasked sweep moves 60 B per weight; what a held sweep moves depends on how its groups of four fall: no figure)
        "unmasked_sweep_fraction_of_stream_copy": {k: round(W * 60 / (v * 1e-3) / (box.hbm_TBps * 1e12), 3)
                                                   for k, v in sweep_ms.items() if k.startswith("unmasked")},
        "train_step_ms": {k: round(v, 5) for k, v in step_ms.items()},
        "train_step_over_unmasked": {k: round(v / sbase, 4) for k, v in step_ms.items()},
        "reps": a.reps, "rounds": a.rounds, "steps_per_block": a.steps,
        "box": {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
                "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus},
    }


def recovery():
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)

    def trained(d, **over):
        opt = train.default_opt(network_name=os.path.join(d, "exp"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                                trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32", log=False,
                                state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2}, **over)
        m = train.Main(opt)
        m.run(trainSet, testSet, epochs=3)
        inputs, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
        return m, m._to_device(inputs, targets)

    def point(net, x, t):
        p = net.predict(x, targets=t, map=True)
        return {"accuracy": round(p.accuracy, 2), "nll": round(p.nll, 5)}
    out = {"net": "784-64-48-10", "dtype": "f32", "recipe": "data.synthetic_digits(2000, 500, seed=3, noise=2.0), 3 epochs, MAP on the 500 test rows",
           "fractions": {}}
    with tempfile.TemporaryDirectory() as d:
        for q in (0.90, 0.95, 0.98, 0.99):
            m, (x, t) = trained(d)                       # the same seeds: the same trained network at every fraction
            row = {"unpruned": point(m.net, x, t)}
            counts = m.net.hold_pruned(m.net.prune(fraction=q))
            row["held_weights"] = sum(counts)
            row["pruned"] = point(m.net, x, t)
            for ep in (1, 2, 3):
                m.train(trainSet)
                if ep in (1, 3):
                    row[f"after_{ep}_held_epoch" + ("s" if ep > 1 else "")] = point(m.net, x, t)
            assert m.net.held == counts
            out["fractions"][f"{q:g}"] = row
        sched = [(3, 0.5), (4, 0.75), (5, 0.9), (6, 0.95), (7, 0.98)]
        m, (x, t) = trained(d, prune_schedule=sched)
        W = sum(v.O * v.I for v in m.net.vb)
        rows = []
        for e, q in sched:
            m.start_epoch()                              # what Main.run does before the epoch, with the points in between
            row = {"epoch": e, "requested": q, "held_fraction": round(sum(m.net.held) / W, 5), "pruned": point(m.net, x, t)}
            m.train(trainSet)
            row["after_1_epoch"] = point(m.net, x, t)
            rows.append(row)
        out["gradual_to_98"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-recovery", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {}
    if not a.skip_cost:
        out["cost"] = cost(a)
    if not a.skip_recovery:
        out["recovery"] = recovery()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
