#!/usr/bin/env python3
"""Structured (unit-level) pruning measured: FusedMLP.prune_units / compact (vbnn_unit_snr, vbnn_unit_select, vbnn_unit_index,
vbnn_unit_gather) on the wide configuration 784-4096-4096-10 bf16, LRT, one MI355X -- the protocol of
tools/sparse_predict_bench.py.

    python tools/unit_prune_bench.py                         # the three sections, each in a child process under its own time limit
    python tools/unit_prune_bench.py --section cost          # one section in this process (one JSON line)

cost:     device time of key / select / index / gather at unit fractions {0.5, 0.75, 0.9} of every layer (scope = "layer": 0.75
          leaves 784-1024-1024-10) with multiple = 256 (HIP events around
          a batch of back-to-back launches), against (a) the PyTorch device route on the same tensors -- row norms, torch.kthvalue,
          topk for the rounding, index_select -- after asserting that both give the same kept sets and the same parameters bit
          for bit and thresholds within 1e-6 relative (torch's row sums add in another order, so its keys may differ from the
          library's in the last bit: whether the thresholds' bits agreed is recorded, `same_tau_bits_as_torch`, not asserted), (b) the streaming bound of the bytes moved at the box's measured copy rate
          (vbnn_box_calibrate), and for the key sweep (c) the vbnn_snr pass over the same layers, which reads the same 8 B per
          weight (and writes 4 more). Per point also the default scope: one select over all 8192 units (`global_select_ms`) and
          a whole prune_units(scope="global") call.
predict:  ms per predict() call (host clock around device-synchronised calls, median) at 30 / 64 / 256 / 3000 operand rows on the
          full network, on the compact network, and under the compressed weight-pruned view of the full network at the same
          kept-weight budget (the weight fraction that leaves as many VB weights as the compact network has); scope = "layer",
          and scope = "global" for comparison (on these parameters one threshold over both layers strips the 4096-input layer
          first: for weights of one scale the unit key falls as 1 / sqrt(I)).
accuracy: a 784-64-48-10 fp32 network trained three epochs on data.synthetic_digits (the recipe of tests/test_prune_gpu.py),
          then accuracy / NLL over the test set of unit pruning (compact network) and weight pruning (pruned view) at equal
          kept-weight budgets. Reported, not gated.
All of it goes to profiles/unit_prune_bench.json (--out) with the `box` block: held MFMA clock and stream-copy rate."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_predict_bench import ROWS, batch_ms, wall_ms  # noqa: E402

UNIT_FRACTIONS = (0.5, 0.75, 0.9)
MULTIPLE = 256
SECTIONS = ("cost", "predict", "accuracy")


def wide_engine(S=1):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    opt = dict(var_init=1e-2, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=784, hidden=[4096, 4096], n_classes=10,
               type="vb", testSamples=S, predict_stacked=True)
    eng = FusedMLP(opt)
    for li, v in enumerate(eng.vb):                      # sigma varies per weight (the inputs of tools/prune_bench.py)
        z = torch.empty_like(v.lvars)
        nn.fill_normal(z, 3, L.STREAM_INIT, li, 7)
        v.lvars.copy_(math.log(1e-2) + 0.75 * z)
    eng.prepare()
    return eng


def box_info(eng):
    from vbnn_amd import _lib as L
    box = L.BoxInfo()
    L.check(L.lib().vbnn_box_calibrate(eng.ctx.h, C.byref(box)))
    return {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
            "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus}


def torch_route(eng, q, multiple):
    """The same pruning (scope = "layer") through PyTorch device ops: (tau per layer, kept lists, compact parameters)."""
    import torch
    keys = [(v.means.double().square().sum(1).sqrt() / v.lvars.exp().double().sum(1).sqrt()).float() for v in eng.vb]
    taus, keep = [], []
    for key in keys:                                     # scope = "layer": the fraction of every layer's units
        k = min(int(math.floor(q * key.numel())), key.numel() - 1)
        tau = torch.kthvalue(key, k + 1).values
        taus.append(tau)
        n0 = (~(key < tau)).sum().clamp(min=1)
        n = int(torch.clamp((n0 + multiple - 1) // multiple * multiple, max=key.numel()).item())       # (a read-back, as prune_units')
        keep.append(torch.topk(key, n).indices.sort().values)
    params, cols = [], None
    for v, rows in zip(eng.vb, keep):
        sel = (lambda a: a.index_select(0, rows)) if cols is None else (lambda a, c=cols: a.index_select(0, rows).index_select(1, c))
        params.append((sel(v.means), sel(v.lvars), v.bias.index_select(0, rows)))
        cols = rows
    return torch.stack(taus), keep, params, eng.weight3.index_select(1, cols)


def section_cost(reps, warmup):
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import _p
    eng = wide_engine()
    box = box_info(eng)
    lib, ctx, nl = L.lib(), eng.ctx.h, len(eng.vb)
    W = sum(v.O * v.I for v in eng.vb)
    n_units = sum(v.O for v in eng.vb)
    snr_out = [torch.empty_like(v.means) for v in eng.vb]

    def f_snr():
        for v, o in zip(eng.vb, snr_out):
            L.check(lib.vbnn_snr(ctx, _p(v.means), _p(v.lvars), v.O * v.I, _p(o)))
    snr_ms = batch_ms(f_snr, reps, warmup)
    keys = [torch.empty(v.O, dtype=torch.float32, device="cuda") for v in eng.vb]
    keep = [torch.zeros(v.O, dtype=torch.int32, device="cuda") for v in eng.vb]
    words = torch.zeros(2 * nl, dtype=torch.int32, device="cuda")
    descs = eng._unit_descs(keys, keep, words[nl:], list(range(nl)))
    key_ms = batch_ms(lambda: L.check(lib.vbnn_unit_snr(ctx, nl, descs)), reps, warmup)
    key_bound = W * 8 / (box["hbm_TBps"] * 1e12) * 1e3
    points = []
    for q in UNIT_FRACTIONS:
        r = eng.prune_units(fraction=q, scope="layer", multiple=MULTIPLE)
        c = eng.compact(r)

        kg = min(int(math.floor(q * n_units)), n_units - 1)   # scope = "global" (the default): ONE select over every unit
        global_select_ms = batch_ms(lambda: L.check(lib.vbnn_unit_select(ctx, nl, descs, kg, _p(words))), reps, warmup)
        global_call_ms = wall_ms(lambda: eng.prune_units(fraction=q, multiple=MULTIPLE), reps, warmup)

        def f_select():                                  # scope = "layer": one select per layer, tau into that layer's word
            for li, v in enumerate(eng.vb):
                d1 = eng._unit_descs(keys, keep, words[nl:], [li])
                L.check(lib.vbnn_unit_select(ctx, 1, d1, min(int(math.floor(q * v.O)), v.O - 1), C.c_void_p(words.data_ptr() + 4 * li)))
        select_ms = batch_ms(f_select, reps, warmup)
        index_ms = batch_ms(lambda: L.check(lib.vbnn_unit_index(ctx, nl, descs, _p(words), 0.0, MULTIPLE)), reps, warmup)
        args, cols = [], None
        for v, w, rows in zip(eng.vb, c.vb, r.keep):
            args.append(L.UnitGatherArgs(means=_p(v.means), lvars=_p(v.lvars), bias=_p(v.bias), O=v.O, I=v.I, rows=_p(rows), n_rows=w.O,
                                         cols=_p(cols), n_cols=w.I, dst_means=_p(w.means), dst_lvars=_p(w.lvars), dst_bias=_p(w.bias)))
            cols = rows
        args.append(L.UnitGatherArgs(means=_p(eng.weight3), O=eng.n_classes, I=eng.sizes[-1], n_rows=eng.n_classes, cols=_p(cols),
                                     n_cols=c.sizes[-1], dst_means=_p(c.weight3)))

        def f_gather():
            for a in args:
                L.check(lib.vbnn_unit_gather(ctx, C.byref(a)))
        gather_ms = batch_ms(f_gather, reps, warmup)
        kept_vb = sum(w.O * w.I for w in c.vb)
        gather_bytes = 2 * (2 * kept_vb * 4) + 2 * eng.n_classes * c.sizes[-1] * 4        # read + write of what is kept (lists: KiB)
        gather_bound = gather_bytes / (box["hbm_TBps"] * 1e12) * 1e3
        prune_call_ms = wall_ms(lambda: eng.prune_units(fraction=q, scope="layer", multiple=MULTIPLE), reps, warmup)   # with allocations + the read-back
        compact_call_ms = wall_ms(lambda: eng.compact(r), 5, 1)                          # with the new engine's construction + prepare
        # the PyTorch route: the same result, then its time (events around the whole route, its one read-back included)
        tau, tkeep, tparams, tw3 = torch_route(eng, q, MULTIPLE)
        tau_lib = torch.tensor(r.tau, dtype=torch.float32)
        same_tau_bits = torch.equal(tau.cpu().view(torch.int32), tau_lib.view(torch.int32))
        assert torch.all((tau.cpu() - tau_lib).abs() <= 1e-6 * tau_lib), (tau, r.tau)
        for li, w in enumerate(c.vb):
            assert torch.equal(tkeep[li].int(), r.keep[li]), li
            for got, want in zip((w.means, w.lvars, w.bias), tparams[li]):
                assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), li
        assert torch.equal(c.weight3.view(torch.int32), tw3.contiguous().view(torch.int32))
        torch_ms = batch_ms(lambda: torch_route(eng, q, MULTIPLE), reps, warmup, batch=1)
        torch_keys_ms = batch_ms(lambda: [(v.means.double().square().sum(1).sqrt() / v.lvars.exp().double().sum(1).sqrt()).float()
                                          for v in eng.vb], reps, warmup)
        lib_ms = key_ms + select_ms + index_ms + gather_ms
        points.append({"unit_fraction": q, "scope": "layer", "multiple": MULTIPLE, "hidden": r.hidden, "n_weights": r.n_weights,
                       "n_weights_before": r.n_weights_before, "tau": r.tau, "same_tau_bits_as_torch": same_tau_bits,
                       "key_ms": round(key_ms, 4), "select_ms": round(select_ms, 4), "index_ms": round(index_ms, 4),
                       "gather_ms": round(gather_ms, 4), "library_device_ms": round(lib_ms, 4),
                       "global_select_ms": round(global_select_ms, 4), "global_prune_units_call_wall_ms": round(global_call_ms, 3),
                       "torch_route_ms": round(torch_ms, 4), "torch_keys_ms": round(torch_keys_ms, 4),
                       "torch_over_library": round(torch_ms / lib_ms, 2),
                       "gather_bytes_moved": gather_bytes, "gather_streaming_bound_ms": round(gather_bound, 4),
                       "gather_fraction_of_bound": round(gather_bound / gather_ms, 3),
                       "prune_units_call_wall_ms": round(prune_call_ms, 3), "compact_call_wall_ms": round(compact_call_ms, 3)})
    return {"section": "cost", "net": "784-4096-4096-10", "dtype": "bf16", "W": W, "n_units": n_units,
            "key_ms": round(key_ms, 4), "key_bytes_moved": W * 8, "key_streaming_bound_ms": round(key_bound, 4),
            "key_fraction_of_bound": round(key_bound / key_ms, 3), "vbnn_snr_ms": round(snr_ms, 4),
            "key_over_vbnn_snr": round(key_ms / snr_ms, 3), "points": points, "box": box}


def section_predict(reps, warmup):
    import torch
    from vbnn_amd import nn
    eng = wide_engine(S=30)
    box = box_info(eng)
    W = sum(v.O * v.I for v in eng.vb)
    out = []
    for scope, q in [("layer", q) for q in UNIT_FRACTIONS] + [("global", q) for q in UNIT_FRACTIONS]:
        r = eng.prune_units(fraction=q, scope=scope, multiple=MULTIPLE)
        c = eng.compact(r)
        kept_vb = sum(w.O * w.I for w in c.vb)
        qw = 1.0 - kept_vb / W                                          # the weight fraction that leaves the same VB weight budget
        sp = eng.prune(fraction=qw).compress()
        for rows, (R, S) in ROWS.items():
            x = torch.empty(R, 784, dtype=torch.float32, device="cuda")
            nn.fill_normal(x, 3, 4, 0, 0)
            assert eng.predict(x, S=S).stacked and c.predict(x, S=S).stacked
            full_ms = wall_ms(lambda: eng.predict(x, S=S), reps, warmup)
            compact_ms = wall_ms(lambda: c.predict(x, S=S), reps, warmup)
            with eng.pruned(sp):
                sparse_ms = wall_ms(lambda: eng.predict(x, S=S), reps, warmup)
            full2_ms = wall_ms(lambda: eng.predict(x, S=S), reps, warmup)       # the full network again: the spread of the box
            out.append({"unit_fraction": q, "scope": scope, "multiple": MULTIPLE, "hidden": r.hidden, "n_weights": r.n_weights,
                        "kept_vb_weights": kept_vb, "equivalent_weight_fraction": round(qw, 6), "nnz": sum(sp.nnz),
                        "operand_rows": rows, "R": R, "S": S, "full_predict_ms": round(full_ms, 4),
                        "full_predict_again_ms": round(full2_ms, 4), "compact_predict_ms": round(compact_ms, 4),
                        "sparse_view_predict_ms": round(sparse_ms, 4), "compact_speedup_over_full": round(full_ms / compact_ms, 3),
                        "compact_speedup_over_sparse_view": round(sparse_ms / compact_ms, 3)})
        del c, sp
    return {"section": "predict", "net": "784-4096-4096-10", "dtype": "bf16", "W": W, "points": out, "box": box}


def section_accuracy(reps, warmup):
    from vbnn_amd import data, train
    trainSet, testSet = data.synthetic_digits(2000, 500, seed=3, noise=2.0)
    with tempfile.TemporaryDirectory() as d:
        opt = train.default_opt(network_name=os.path.join(d, "exp_units"), hidden=[64, 48], batchSize=100, testBatchSize=100,
                                trainSize=2000, testSize=500, S=2, testSamples=3, mode="lrt", dtype="f32",
                                state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
        m = train.Main(opt)
        hist = m.run(trainSet, testSet, epochs=3)
        inputs, targets = testSet.create_minibatch(0, 500, 500, opt.get("geometry"))
        x, t = m._to_device(inputs, targets)
        net = m.net
        W = sum(v.O * v.I for v in net.vb)
        rows = []
        for scope in ("global", "layer"):
            for q in (0.0, 0.125, 0.25, 0.5, 0.75):
                r = net.prune_units(fraction=q, scope=scope)
                c = net.compact(r)
                kept_vb = sum(w.O * w.I for w in c.vb)
                qw = 1.0 - kept_vb / W
                pr = net.prune(fraction=qw, scope=scope)
                row = {"scope": scope, "unit_fraction": q, "hidden": r.hidden, "kept_vb_weights": kept_vb,
                       "equivalent_weight_fraction": round(qw, 6), "weights_pruned": pr.n_pruned}
                for name, kw in (("map", dict(map=True)), ("S10", dict(S=10))):
                    d0 = net.draw
                    pu = c.predict(x, targets=t, **kw)
                    with net.pruned(pr):
                        pw = net.predict(x, targets=t, **kw)
                    net.draw = d0                                       # every point sees the same draws
                    row[name] = {"units_accuracy": pu.accuracy, "units_nll": round(pu.nll, 6), "weights_accuracy": pw.accuracy,
                                 "weights_nll": round(pw.nll, 6)}
                rows.append(row)
    return {"section": "accuracy", "net": "784-64-48-10", "dtype": "f32", "data": "synthetic_digits(2000, 500, seed=3, noise=2.0), 3 epochs",
            "devacc_after_training": hist[-1]["devacc"], "W": W, "points": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=SECTIONS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per section (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_prune_bench.json"))
    a = ap.parse_args()
    if a.section:
        sys.path.insert(0, ROOT)
        fn = {"cost": section_cost, "predict": section_predict, "accuracy": section_accuracy}[a.section]
        print(json.dumps(fn(a.reps, a.warmup)), flush=True)
        return 0
    out = {}
    for name in SECTIONS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--section", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(json.dumps({"section": name, "error": f"exit status {p.returncode}", "stderr": p.stderr[-3000:]}), flush=True)
            return p.returncode                     # nothing more on the GPU after a failed section
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        out[name] = json.loads(line)
    out["box"] = out["cost"]["box"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
