#!/usr/bin/env python3
"""predict() under the compressed pruned view (PruneResult.compress: vbnn_prune_compress + vbnn_forward_sparse) against the
dense pruned view of the same pruning, on the wide configuration 784-4096-4096-10 bf16 (W = 19,988,480).

    python tools/sparse_predict_bench.py                     # every point, each in a child process under its own time limit
    python tools/sparse_predict_bench.py --point 0.9 30      # one point in this process (one JSON line)

Points: pruned fraction {0.5, 0.9, 0.95, 0.98} x operand rows {30 (batch 1 x S 30 stacked), 64, 256, 3000 (100 x 30 stacked)}.
Per point, in one process on one box: ms per predict call under the dense pruned view (the dense GEMM kernels on mu_p / var_p)
and under the compressed view, after asserting that the two agree (host clock around device-synchronised calls, median); the
device time of each layer's forward alone in both forms (HIP events around a batch of back-to-back launches); the device time
of compress against its streaming bound (the count sweep reads 8 B per weight, the fill sweep 8 B per weight and writes
2 + 2 x 2 B per entry; vbnn_box_calibrate's copy rate); the bytes of the two representations; the `box` block. All points go to
profiles/sparse_predict_bench.json (--out)."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.5, 0.9, 0.95, 0.98)
ROWS = {30: (1, 30), 64: (64, 1), 256: (256, 1), 3000: (100, 30)}       # operand rows -> (minibatch rows R, draws S), stacked


def wall_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def batch_ms(fn, reps, warmup, batch=10):
    """Device time of one fn(): events around `batch` back-to-back calls (launch gaps hidden by the queue), median over reps."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / batch)
    return sorted(ts)[len(ts) // 2]


def run_point(q, rows, reps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import _p
    R, S = ROWS[rows]
    hidden = [4096, 4096]
    opt = dict(var_init=1e-2, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=784, hidden=hidden, n_classes=10, type="vb",
               testSamples=S, predict_stacked=True)
    eng = FusedMLP(opt)
    for li, v in enumerate(eng.vb):                      # sigma varies per weight (the inputs of tools/prune_bench.py)
        z = torch.empty_like(v.lvars)
        nn.fill_normal(z, 3, L.STREAM_INIT, li, 7)
        v.lvars.copy_(math.log(1e-2) + 0.75 * z)
    eng.prepare()
    lib, ctx = L.lib(), eng.ctx.h
    box = L.BoxInfo()
    L.check(lib.vbnn_box_calibrate(ctx, C.byref(box)))
    x = torch.empty(R, 784, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, 3, 4, 0, 0)
    t = eng.synthetic_targets(x)
    res = eng.prune(fraction=q)
    sp = res.compress()
    W = res.W

    # ---- the two views agree (one bf16 rounding per hidden layer: tests/test_sparse_gpu.py), then ms per call
    d0 = eng.draw
    with eng.pruned(res):
        a = eng.predict(x, S=S, targets=t)
    hbuf = eng._pred_bufs[len(eng.vb)].x.t[:, :hidden[-1]].double().abs()
    tol = 4 * 2.0 ** -8 * float((hbuf @ eng.weight3.double().abs().T).max())
    eng.draw = d0
    with eng.pruned(sp):
        b = eng.predict(x, S=S, targets=t)
    dlp = float((a.log_probs.double() - b.log_probs.double()).abs().max())
    assert dlp <= tol and a.stacked and b.stacked, (dlp, tol)
    with eng.pruned(res):
        dense_ms = wall_ms(lambda: eng.predict(x, S=S), reps, warmup)
    with eng.pruned(sp):
        sparse_ms = wall_ms(lambda: eng.predict(x, S=S), reps, warmup)

    # ---- each layer's forward alone, on the operands the last predict left
    N, rpd = R * S, (R if S > 1 else 0)
    bufs, T = eng._pred_bufs, eng._sparse_bufs
    layer_ms = []
    for li, v in enumerate(eng.vb):
        last = li == len(eng.vb) - 1
        out = bufs[li + 1]
        r = bufs.r if rpd == 0 else None                 # as predict(): one-draw forwards get the throwaway r (kernel selection)
        fa = L.FwdArgs(w=res.mu_p[li].ptr, w2=res.var_p[li].ptr, x=bufs[li].x.ptr, x2=bufs[li].x2.ptr, ld_w=res.mu_p[li].ld,
                       ld_x=bufs[li].x.ld, N=N, I=v.I, O=v.O, bias=_p(v.bias), seed=eng.seed, layer=v.layer_id, draw=1, row0=0,
                       r=r.ptr if r else None, ld_r=r.ld if r else 0, r_packed=1, relu=1, h=out.x.ptr, h2=None if last else out.x2.ptr,
                       ld_h=out.x.ld, rows_per_draw=rpd)
        sa = L.SparseFwdArgs(row_ptr=_p(sp.row_ptr[li]), cols=_p(sp.cols[li]), mu_v=_p(sp.mu_v[li]), var_v=_p(sp.var_v[li]),
                             idx_bytes=sp.idx_bytes[li], xT=T[li].ptr, ld_xT=T[li].ld, N=N, I=v.I, O=v.O, bias=_p(v.bias),
                             seed=eng.seed, layer=v.layer_id, draw=1, row0=0, relu=1, h=out.x.ptr if last else None,
                             ld_h=out.x.ld if last else 0, hT=None if last else T[li + 1].ptr, ld_hT=0 if last else T[li + 1].ld,
                             rows_per_draw=rpd)
        dm = batch_ms(lambda: L.check(lib.vbnn_forward(ctx, eng.code, C.byref(fa))), reps, warmup)
        sm = batch_ms(lambda: L.check(lib.vbnn_forward_sparse(ctx, eng.code, C.byref(sa))), reps, warmup)
        layer_ms.append({"layer": f"{v.I}x{v.O}", "nnz": sp.nnz[li], "dense_ms": round(dm, 4), "sparse_ms": round(sm, 4)})

    # ---- compress against its streaming bound
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res.compress()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    compress_wall = sorted(ts)[len(ts) // 2]                            # with the allocations and the count read-back
    nl = len(eng.vb)
    pd = [(L.PruneDesc * 1)(L.PruneDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I)) for v in eng.vb]
    nnz_dev = torch.zeros(nl, dtype=torch.int32, device="cuda")
    sd = [(L.SparseDesc * 1)(L.SparseDesc(row_ptr=_p(sp.row_ptr[li]), cols=_p(sp.cols[li]), mu_v=_p(sp.mu_v[li]), var_v=_p(sp.var_v[li]),
                                          O=v.O, I=v.I, nnz_cap=sp.nnz[li], nnz_dev=C.c_void_p(nnz_dev.data_ptr() + 4 * li),
                                          idx_bytes=sp.idx_bytes[li])) for li, v in enumerate(eng.vb)]

    def f_compress():
        for li in range(nl):
            L.check(lib.vbnn_prune_compress(ctx, eng.code, 1, pd[li], sd[li], None, res.tau[li]))
    compress_ms = batch_ms(f_compress, reps, warmup, batch=1)
    moved = W * 16 + sum(sp.nnz) * (2 + 2 * 2)
    bound_ms = moved / (box.hbm_TBps * 1e12) * 1e3
    return {"net": "784-4096-4096-10", "dtype": "bf16", "W": W, "fraction": q, "n_pruned": res.n_pruned, "nnz": sum(sp.nnz),
            "operand_rows": rows, "R": R, "S": S, "dense_predict_ms": round(dense_ms, 4), "sparse_predict_ms": round(sparse_ms, 4),
            "sparse_speedup": round(dense_ms / sparse_ms, 3), "max_abs_dlogp": dlp, "dlogp_tol": tol, "layers": layer_ms,
            "compress_ms": round(compress_ms, 4), "compress_call_wall_ms": round(compress_wall, 3), "compress_bytes_moved": moved,
            "compress_streaming_bound_ms": round(bound_ms, 4), "compress_fraction_of_bound": round(bound_ms / compress_ms, 3),
            "nbytes": sp.nbytes, "dense_nbytes": sp.dense_nbytes, "nbytes_ratio": round(sp.nbytes / sp.dense_nbytes, 4),
            "box": {"mfma_clock_ghz": round(box.mfma_clock_ghz, 4), "mfma_tflops": round(box.mfma_tflops, 1),
                    "hbm_TBps": round(box.hbm_TBps, 3), "cus": box.cus}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", nargs=2, metavar=("FRACTION", "ROWS"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per point (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_predict_bench.json"))
    a = ap.parse_args()
    if a.point:
        print(json.dumps(run_point(float(a.point[0]), int(a.point[1]), a.reps, a.warmup)), flush=True)
        return 0
    points = []
    for q in FRACTIONS:
        for rows in ROWS:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--point", str(q), str(rows),
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                print(json.dumps({"fraction": q, "operand_rows": rows, "error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}),
                      flush=True)
                return p.returncode             # nothing more on the GPU after a failed point
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            points.append(json.loads(line))
    out = {"points": points, "box": points[0]["box"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
