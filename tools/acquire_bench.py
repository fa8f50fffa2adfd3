#!/usr/bin/env python3
"""What pool acquisition costs (vbnn_top_rows, csrc/acquire.hip; FusedMLP.acquire; vbnn_amd.active.active_learning).

    python tools/acquire_bench.py [--kernel-reps 20] [--rounds 5] [--out profiles/acquire_bench.json]

The family's protocol: before anything is timed the outputs are asserted BIT FOR BIT against the restatement of
tests/_acquire_np.py on the same inputs; us per call come from blocks of calls between HIP events (never one call on its own),
the variants interleaved, medians of the rounds; the box's held clock and stream-copy rate (vbnn_box_calibrate) are recorded.

(a) vbnn_top_rows at R = 10^4, 10^6, 10^7 x k = 10, 1000, 4096, deterministic and stochastic (beta = 1), beside torch.topk on the
    same tensor (the same values asserted, and the same indices wherever a selected value is not repeated) and vbnn_selective at
    Q = 1 on the same scores. The byte floor is what the shape's passes move: three digit passes and the take pass, 4 B read per
    row each (distinct scores: the tie count pass returns at once) -- 16 B per row deterministic; the stochastic form's first pass
    also WRITES the 4 B key, 20 B per row; `fraction_of_stream_copy` is each form's floor over its time over the box's copy rate. Beside it, in the same process, the MSE form's ACCUMULATE middle draw's share (vbnn_predict_moments), the
    family's yardstick for a streaming kernel.
(b) a whole FusedMLP.acquire at 784-4096-4096-10 bf16 on a 10^5-row pool with S = 30, and analytic=True beside it, each split
    into the predictive and the selection.
(c) active_learning on synthetic_digits: "mutual_info", "entropy", "random", and "mutual_info" with beta = 1. Recorded, not judged.
Whatever is measured is written down, including where the kernel misses."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3


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


def _mse_share(a, L, h, rate):
    """The MSE form's ACCUMULATE middle draw at R = D = 4096, as tools/calibration_bench.py times it: its share of the copy rate."""
    import torch
    from vbnn_amd.nn import _p
    R = D = 4096
    f32 = dict(dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    draws, tt, st = torch.randn(2, R, D, generator=g, **f32), torch.randn(R, D, generator=g, **f32), torch.empty(R, 2 * D + 2, **f32)
    mm = L.MomentsArgs(y=_p(draws), ld_y=D, target=_p(tt), ld_t=D, R=R, D=D, S=4, noise_var=0.1, state=_p(st),
                       form=L.MOMENTS_ACCUMULATE, ld_out=D)

    def mse_draw(s=1):
        mm.draw = s
        mm.y = C.c_void_p(draws.data_ptr() + 4 * s * R * D)
        L.check(L.lib().vbnn_predict_moments(h, C.byref(mm)))
    mse_draw(0)
    ms = _interleaved({"a": mse_draw, "b": mse_draw}, a.kernel_reps, a.rounds)
    nbytes = 6 * 4.0 * R * D
    return [round(nbytes / (ms[k] * 1e-3) / rate, 4) for k in ("a", "b")]


def kernel_points(a, L, h, rate):
    import numpy as np
    import torch
    from tests import _acquire_np as A
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    for R in (10 ** 4, 10 ** 6, 10 ** 7):
        g = torch.Generator(device="cuda").manual_seed(7)
        score = (2.3 * torch.rand(R, generator=g, dtype=torch.float32, device="cuda") + 1e-3).contiguous()   # entropy-like, > 0
        hit = torch.zeros(R, dtype=torch.int32, device="cuda")
        s_host = score.cpu().numpy()
        nb = C.c_size_t()
        L.check(lib.vbnn_top_rows_workspace_bytes(R, 4096, C.byref(nb)))
        ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        want = {False: A.top_rows(s_host, 4096, True, None),
                True: A.top_rows(s_host, 4096, True, None, beta=1.0, seed=SEED, draw=9, row0=0)}
        for k in (10, 1000, 4096):
            out = {n: torch.empty(k, dtype=dt, device="cuda") for n, dt in (("index", torch.int32), ("value", torch.float32),
                                                                            ("key", torch.float32))}
            counts = torch.empty(4, dtype=torch.int64, device="cuda")
            fns = {}
            for stoch in (False, True):
                m = L.TopRowsArgs(score=_p(score), exclude=None, R=R, k=k, largest=1, stochastic=int(stoch), beta=1.0, seed=SEED,
                                  draw=9, row0=0, index=_p(out["index"]), value=_p(out["value"]), key=_p(out["key"]),
                                  counts=_p(counts), workspace=_p(ws), workspace_bytes=nb.value)
                fn = (lambda m=m: L.check(lib.vbnn_top_rows(h, C.byref(m))))
                fn()
                wi, wv, wk, _ = want[stoch]
                assert np.array_equal(out["index"].cpu().numpy(), wi[:k]), (R, k, stoch, "index")
                assert np.array_equal(A.bits(out["value"].cpu().numpy()), wv[:k]), (R, k, stoch, "value")
                assert np.array_equal(A.bits(out["key"].cpu().numpy()), wk[:k]), (R, k, stoch, "key")
                assert counts.cpu().tolist() == [k, R, 0, 0]
                fns["stochastic" if stoch else "deterministic"] = fn
            tv, ti = torch.topk(score, k)
            wi, wv, _, _ = want[False]
            assert np.array_equal(A.bits(tv.cpu().numpy()), wv[:k]), (R, k, "torch.topk values")
            v = wv[:k]
            lone = np.ones(k, bool)
            lone[1:] &= v[1:] != v[:-1]
            lone[:-1] &= v[:-1] != v[1:]
            if k < 4096:
                lone[-1] &= wv[k] != v[-1]
            assert np.array_equal(ti.cpu().numpy()[lone], wi[:k][lone]), (R, k, "torch.topk indices")
            tau = torch.empty(1, dtype=torch.float32, device="cuda")
            sc = torch.empty(1, 4, dtype=torch.int64, device="cuda")
            sm = L.SelectiveArgs(score=_p(score), hit=_p(hit), R=R, Q=1, tau=_p(tau), counts=_p(sc))
            sm.k[0] = R - k + 1                                  # the k-th LARGEST score: the same threshold
            fns["torch_topk"] = lambda: torch.topk(score, k)
            fns["selective_q1"] = lambda: L.check(lib.vbnn_selective(h, C.byref(sm)))
            fns["selective_q1"]()
            assert A.bits(tau.cpu().numpy())[0] == wv[k - 1]
            ms = _interleaved(fns, a.kernel_reps, a.rounds)
            floor = {"deterministic": 4 * 4.0 * R, "stochastic": 5 * 4.0 * R}       # four reads; the stored keys' write
            row = {"R": R, "k": k, "passes": 4, "bytes_moved": {n: int(v) for n, v in floor.items()},
                   "byte_floor_us": {n: round(v / rate * 1e6, 2) for n, v in floor.items()},
                   "repeated_values_among_selected": int((~lone).sum())}
            for name in fns:
                row[name + "_us"] = round(ms[name] * 1e3, 2)
            row["fraction_of_stream_copy"] = {n: round(floor[n] / (ms[n] * 1e-3) / rate, 4) for n in ("deterministic", "stochastic")}
            row["kernel_over_torch_topk"] = {n: round(ms[n] / ms["torch_topk"], 4) for n in ("deterministic", "stochastic")}
            row["kernel_over_selective"] = round(ms["deterministic"] / ms["selective_q1"], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del score, hit, ws
    return rows


def acquire_points(a):
    """A whole acquire at 784-4096-4096-10 bf16 on a 10^5-row pool, S = 30: sampled and analytic, each beside its own predictive
    and the selection alone (the three are timed in one interleaved set)."""
    import torch
    from vbnn_amd.engine import FusedMLP
    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=SEED, input_size=784, hidden=[4096, 4096],
               n_classes=10, type="vb", testSamples=30)
    eng = FusedMLP(opt)
    R, k = 10 ** 5, 1000
    g = torch.Generator(device="cuda").manual_seed(11)
    pool = torch.randn(R, 784, generator=g, dtype=torch.float32, device="cuda")
    out = []
    for analytic in (False, True):
        predictive = ((lambda: eng.predict_analytic(pool, topk=2, keep_probs=False)) if analytic
                      else (lambda: eng.predict_classes(pool, topk=2, keep_probs=False)))
        vec = predictive().mutual_info
        fns = {"acquire": lambda: eng.acquire(pool, k, analytic=analytic), "predictive": predictive,
               "selection": lambda: eng.top_rows(vec, k)}
        res = fns["acquire"]()
        assert res.n_selected == k and res.S == 30
        ms = _interleaved(fns, max(1, a.kernel_reps // 10), max(3, a.rounds - 2))
        row = {"R": R, "k": k, "S": 30, "analytic": analytic, "score": res.score_name, "chunks": res.chunks,
               "acquire_ms": round(ms["acquire"], 3), "predictive_ms": round(ms["predictive"], 3),
               "selection_ms": round(ms["selection"], 4), "selection_share": round(ms["selection"] / ms["acquire"], 5)}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def curves():
    import numpy as np
    import torch
    from vbnn_amd import data
    from vbnn_amd.active import active_learning
    from vbnn_amd.train import default_opt
    train, test = data.synthetic_digits(2000, 500)
    xp = torch.from_numpy(train["inputs"]).cuda().reshape(2000, -1)
    yp = torch.from_numpy(train["targets"].astype(np.int32)).cuda()
    xt = torch.from_numpy(test["inputs"]).cuda().reshape(500, -1)
    yt = torch.from_numpy(test["targets"].astype(np.int32)).cuda()
    opt = default_opt(hidden=[64], batchSize=50, S=2, testSamples=10, log=False, seed=SEED)
    out = []
    for score, beta in (("mutual_info", None), ("entropy", None), ("random", None), ("mutual_info", 1.0)):
        curve = active_learning(opt, xp, yp, xt, yt, n_init=100, k=50, rounds=8, score=score, beta=beta, epochs=5)
        out.append({"score": score, "beta": beta, "labels": [c["labels"] for c in curve],
                    "accuracy": [round(c["accuracy"], 2) for c in curve], "nll": [round(c["nll"], 4) for c in curve]})
        print(json.dumps(out[-1]), flush=True)
    return {"pool": 2000, "test": 500, "n_init": 100, "k": 50, "rounds": 8, "epochs": 5, "hidden": [64], "curves": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=20, help="kernel launches per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acquire_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = _box(L, h)
    rate = box.hbm_TBps * 1e12
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d,
           "mse_accumulate_fraction_of_stream_copy": _mse_share(a, L, h, rate),
           "top_rows": kernel_points(a, L, h, rate), "acquire": acquire_points(a), "active_learning": curves()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
