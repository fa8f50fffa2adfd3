#!/usr/bin/env python3
"""What diverse pool acquisition costs (vbnn_kcentre, csrc/kcentre.hip; FusedMLP.spread_rows / acquire_diverse).

    python tools/kcentre_bench.py [--kernel-reps 3] [--rounds 5] [--out profiles/kcentre_bench.json]

The protocol of tools/acquire_bench.py (whose helpers this imports): before anything is timed the outputs are asserted -- BIT
FOR BIT against the restatement of tests/_kcentre_np.py on the leading rows of the same tensor, and against a PyTorch composition
(broadcast difference, square, sum(1), torch.minimum, argmax) on the whole of it; the features are integer-valued, so every route
is exact and the picks must be the same rows. Times come from blocks of calls between HIP events, the variants interleaved,
medians of the rounds; the box's held clock and stream-copy rate are recorded, and the MSE form's ACCUMULATE middle draw is timed
twice in the same process as the family's yardstick for a streaming kernel.

(a) the time per greedy step -- the slope between a call with k = 8 and one with k = 40 steps, so the call's fixed part drops
    out -- at R x D = 10^4 x 4096 and 10^5 x 512 (164 and 205 MB: resident in the Infinity Cache between steps), at 10^5 x 4096
    (1.6 GB: not resident) and at 64 x 64 (the fixed cost of a step). A step's byte floor is R D 4 plus 9 B per row (min_dist
    read and written where it moved, the standing byte) at the box's stream-copy rate. The expectation for the non-resident
    point is the MSE kernel's share of that rate, the allowance the spread of its two timings; outside it is a MISS.
    The PyTorch composition's step is timed beside it.
(b) the initial-centres pass at 10^3 and 10^4 centres: a call with the centres and k = 1 minus the same call without.
(c) a whole FusedMLP.acquire_diverse beside acquire at 784-4096-4096-10 bf16 on a 10^5-row pool, k = 1000, S = 30, with the
    selection alone (its share) and the features alone.
(d) active_learning(diverse=True) on synthetic_digits, the set-up of profiles/acquire_bench.json's curves. Recorded, not judged.
Whatever is measured is written down, including where the kernel misses."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SEED = 3


def _torch_steps(F, m, c, n):
    """n greedy steps of the PyTorch composition from centre row c (a 0-d device tensor) and minimum m; returns the picks."""
    import torch
    picks = []
    for _ in range(n):
        d = ((F - F[c]) ** 2).sum(1)
        m = torch.minimum(m, d)
        c = torch.argmax(m)
        picks.append(c)
    return torch.stack(picks), m


def step_points(a, L, h, rate, share):
    import numpy as np
    import torch
    import acquire_bench as AB
    from tests import _kcentre_np as K
    from vbnn_amd.nn import _p
    lib, rows = L.lib(), []
    for R, D, resident in ((10 ** 4, 4096, True), (10 ** 5, 512, True), (10 ** 5, 4096, False), (64, 64, True)):
        g = torch.Generator(device="cuda").manual_seed(7)
        F = torch.randint(-8, 9, (R, D), generator=g, device="cuda").float().contiguous()
        nb = C.c_size_t()
        L.check(lib.vbnn_kcentre_workspace_bytes(R, D, 4096, C.byref(nb)))
        ws = torch.empty((nb.value + 7) // 8, dtype=torch.int64, device="cuda")
        k_lo, k_hi = 8, 40
        out = {n: torch.empty(k_hi, dtype=dt, device="cuda") for n, dt in (("index", torch.int32), ("key", torch.float32),
                                                                           ("dist", torch.float32))}
        md = torch.empty(R, dtype=torch.float32, device="cuda")
        counts = torch.empty(4, dtype=torch.int64, device="cuda")
        cen = torch.zeros(1, dtype=torch.int32, device="cuda")

        def call(k, feat=F, rows_=R, n_centres=1):
            m = L.KcentreArgs(feat=_p(feat), ld=D, weight=None, exclude=None, centres=_p(cen), R=rows_, D=D, n_centres=n_centres, k=k,
                              resume=0, reserved=0, index=_p(out["index"]), key=_p(out["key"]), dist=_p(out["dist"]),
                              min_dist=_p(md), counts=_p(counts), workspace=_p(ws), workspace_bytes=ws.numel() * 8)
            L.check(lib.vbnn_kcentre(h, C.byref(m)))

        # asserted first: the restatement on the leading rows, the PyTorch composition on all of them (exact integers: the
        # same distances; the pick is the lowest row that attains torch.argmax's maximum)
        sub = min(R, 1500)
        call(6, rows_=sub)
        want = K.kcentre(F[:sub].cpu().numpy(), 6, None, None, [0])
        assert np.array_equal(out["index"][:6].cpu().numpy(), want["index"]), (R, D, "index against the restatement")
        assert np.array_equal(out["dist"][:6].cpu().numpy().view(np.uint32), want["dist"].view(np.uint32)), (R, D, "dist")
        assert np.array_equal(md[:sub].cpu().numpy().view(np.uint32), want["min_dist"].view(np.uint32)), (R, D, "min_dist")
        call(k_lo)
        got_i, got_d = out["index"][:k_lo].long(), out["dist"][:k_lo]
        m_k = ((F - F[0]) ** 2).sum(1)                                 # the given centre, row 0
        for j in range(k_lo):
            top = torch.nonzero(m_k == m_k[torch.argmax(m_k)]).flatten()
            assert int(got_i[j]) == int(top[0]), (R, D, j, "pick against the PyTorch composition")
            assert float(got_d[j]) == float(m_k[top[0]]), (R, D, j, "dist against the PyTorch composition")
            m_k = torch.minimum(m_k, ((F - F[got_i[j]]) ** 2).sum(1))
        assert torch.equal(md, m_k), (R, D, "min_dist against the PyTorch composition")
        m0 = torch.full((R,), float("inf"), device="cuda")
        c0 = cen[0].long()
        fns = {"k_lo": lambda: call(k_lo), "k_hi": lambda: call(k_hi),
               "torch_lo": lambda: _torch_steps(F, m0, c0, k_lo), "torch_hi": lambda: _torch_steps(F, m0, c0, k_hi)}
        ms = AB._interleaved(fns, a.kernel_reps, a.rounds)
        step_us = (ms["k_hi"] - ms["k_lo"]) / (k_hi - k_lo) * 1e3
        torch_us = (ms["torch_hi"] - ms["torch_lo"]) / (k_hi - k_lo) * 1e3
        floor = 4.0 * R * D + 9.0 * R
        frac = floor / (step_us * 1e-6) / rate
        row = {"R": R, "D": D, "feature_MB": round(4.0 * R * D / 1e6, 1), "cache_resident": resident, "step_us": round(step_us, 2),
               "call_k8_us": round(ms["k_lo"] * 1e3, 1), "call_k40_us": round(ms["k_hi"] * 1e3, 1),
               "byte_floor_us": round(floor / rate * 1e6, 2), "achieved_TBps": round(floor / (step_us * 1e-6) / 1e12, 3),
               "fraction_of_stream_copy": round(frac, 4), "torch_step_us": round(torch_us, 2),
               "kernel_over_torch": round(step_us / torch_us, 4)}
        if not resident:
            exp, allow = sum(share) / 2, abs(share[0] - share[1])
            row.update(expectation=round(exp, 4), allowance=round(allow, 4), verdict="MET" if frac >= exp - allow else "MISS")
        rows.append(row)
        print(json.dumps(row), flush=True)

        if R * D >= 10 ** 7 and resident:                              # (b) the initial centres, on the two resident points
            for n in (10 ** 3, 10 ** 4):
                g2 = torch.Generator(device="cuda").manual_seed(n)
                many = torch.randint(0, R, (n,), generator=g2, device="cuda").int()

                def with_centres(many=many, n=n):
                    m = L.KcentreArgs(feat=_p(F), ld=D, weight=None, exclude=None, centres=_p(many), R=R, D=D, n_centres=n, k=1,
                                      resume=0, reserved=0, index=_p(out["index"]), key=_p(out["key"]), dist=_p(out["dist"]),
                                      min_dist=_p(md), counts=_p(counts), workspace=_p(ws), workspace_bytes=ws.numel() * 8)
                    L.check(lib.vbnn_kcentre(h, C.byref(m)))
                with_centres()
                ref = torch.full((R,), float("inf"), device="cuda")
                for c in many[:50].tolist():
                    ref = torch.minimum(ref, ((F - F[c]) ** 2).sum(1))
                assert bool((md <= ref).all()) and int(counts[0]) == 1, (R, D, n, "initial centres")
                ms2 = AB._interleaved({"with": with_centres, "without": lambda: call(1, n_centres=0)}, 1, max(3, a.rounds - 2))
                blk = K.block(D)
                passes = (n + blk - 1) // blk
                r2 = {"R": R, "D": D, "n_centres": n, "centres_per_pass": blk, "passes": passes,
                      "initial_centres_ms": round(ms2["with"] - ms2["without"], 3),
                      "per_pass_us": round((ms2["with"] - ms2["without"]) / passes * 1e3, 2),
                      "per_centre_us": round((ms2["with"] - ms2["without"]) / n * 1e3, 3)}
                rows.append(r2)
                print(json.dumps(r2), flush=True)
        del F, ws, md, m0
        torch.cuda.empty_cache()
    return rows


def acquire_points(a):
    import torch
    import acquire_bench as AB
    from vbnn_amd.engine import FusedMLP
    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=SEED, input_size=784, hidden=[4096, 4096],
               n_classes=10, type="vb", testSamples=30)
    eng = FusedMLP(opt)
    R, k = 10 ** 5, 1000
    g = torch.Generator(device="cuda").manual_seed(11)
    pool = torch.randn(R, 784, generator=g, dtype=torch.float32, device="cuda")
    feats = eng.features(pool)
    vec = eng.predict_classes(pool, topk=2, keep_probs=False).mutual_info
    fns = {"acquire": lambda: eng.acquire(pool, k), "acquire_diverse": lambda: eng.acquire_diverse(pool, k),
           "features": lambda: eng.features(pool), "selection": lambda: eng.spread_rows(feats, k, weight=vec)}
    res = fns["acquire_diverse"]()
    assert res.n_selected == k and res.S == 30 and len(set(res.indices.cpu().tolist())) == k
    ms = AB._interleaved(fns, 1, max(3, a.rounds - 2))
    row = {"R": R, "k": k, "S": 30, "H": 4096, "score": res.score_name, "n_void": res.n_void,
           "acquire_ms": round(ms["acquire"], 3), "acquire_diverse_ms": round(ms["acquire_diverse"], 3),
           "features_ms": round(ms["features"], 3), "selection_ms": round(ms["selection"], 3),
           "selection_per_step_us": round(ms["selection"] / (k + 1) * 1e3, 2),
           "selection_share": round(ms["selection"] / ms["acquire_diverse"], 4),
           "diverse_over_acquire": round(ms["acquire_diverse"] / ms["acquire"], 3)}
    print(json.dumps(row), flush=True)
    return [row]


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
    for score in ("mutual_info", "entropy"):
        curve = active_learning(opt, xp, yp, xt, yt, n_init=100, k=50, rounds=8, score=score, epochs=5, diverse=True)
        out.append({"score": score, "diverse": True, "labels": [c["labels"] for c in curve],
                    "accuracy": [round(c["accuracy"], 2) for c in curve], "nll": [round(c["nll"], 4) for c in curve]})
        print(json.dumps(out[-1]), flush=True)
    return {"pool": 2000, "test": 500, "n_init": 100, "k": 50, "rounds": 8, "epochs": 5, "hidden": [64], "curves": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=3, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcentre_bench.json"))
    a = ap.parse_args()
    import acquire_bench as AB
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    h = Context.get().h
    box, box_d = AB._box(L, h)
    rate = box.hbm_TBps * 1e12
    mse = argparse.Namespace(kernel_reps=20, rounds=a.rounds)
    share = AB._mse_share(mse, L, h, rate)
    out = {"kernel_reps": a.kernel_reps, "rounds": a.rounds, "box": box_d, "mse_accumulate_fraction_of_stream_copy": share,
           "steps": step_points(a, L, h, rate, share), "acquire": acquire_points(a), "active_learning": curves()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
