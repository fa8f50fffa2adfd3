"""Worker of tests/test_checkpoint_gpu.py's replica check: one rank of a world of 2 on ONE GPU (gloo carries the collectives, as in
tests/_dist_gpu_worker.py). Both ranks train one minibatch through the real data-parallel step (all-reduced gradients, the rank-local
update), so parameters and Adam moments exist and are identical: check_replicas() passes. Then rank 1 moves one weight of VB layer 1 by
one ulp: check_replicas() must raise on EVERY rank, naming the tensor and the ranks. Exit status 0 only if both happened."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vbnn_amd.engine import CheckpointError, FusedMLP        # noqa: E402
from vbnn_amd.nn import fill_normal                          # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    opt = dict(var_init=1e-3, mu_init=1, B=1e3, S=1, mode="lrt", dtype="f32", seed=3, input_size=20, hidden=[24, 16], n_classes=5,
               fuse_kl=True, state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3}, varState={"learningRate": 5e-2})
    eng = FusedMLP(opt, world_size=world, rank=rank)
    n_loc = 16
    x = torch.empty(n_loc, 20, dtype=torch.float32, device="cuda")
    fill_normal(x, 3, 4, 0, 0, row0=rank * n_loc)
    t = ((torch.arange(n_loc, device="cuda", dtype=torch.int64) + rank * n_loc) * 7 % 5).to(torch.int32)
    eng.prepare()
    eng.resetGradients(); eng.sample(); eng.run(x, t)
    eng.update(opt)
    status = 0
    try:
        eng.check_replicas()
        print(f"rank {rank}: identical ok", flush=True)
    except CheckpointError as e:
        print(f"rank {rank}: identical replicas were refused: {e}", flush=True)
        status = 3
    if rank == 1:
        eng.vb[1].means.view(torch.int32)[3, 5] += 1          # one ulp
    try:
        eng.check_replicas()
        print(f"rank {rank}: the perturbed replica went unnoticed", flush=True)
        status = 4
    except CheckpointError as e:
        msg = str(e)
        ok = "layers[1].means" in msg and "ranks [0]" in msg and "ranks [1]" in msg
        print(f"rank {rank}: caught ({'named' if ok else 'NOT named'}): {msg}", flush=True)
        status = status or (0 if ok else 5)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(status)


if __name__ == "__main__":
    main()
