"""The active-learning loop over the fused engine: train on the labelled rows, evaluate, let FusedMLP.acquire choose the next
k rows of the unlabelled rest, move them over. prune_curve's style: a list of dicts, no plotting."""
import numpy as np
import torch

from .engine import FusedMLP


def _train_epoch(net, opt, x, t, order, S):
    """One pass over the labelled rows `order` (row numbers into x / t, device tensors) in minibatches of opt.batchSize, the
    step of train.Main.train; a short last minibatch is skipped, as there."""
    bs = int(opt["batchSize"])
    stacked = net.mode == "lrt" and S > 1 and bool(opt.get("stack_draws", True))
    for b0 in range(0, len(order) - bs + 1, bs):
        rows = order[b0:b0 + bs]
        xb, tb = x[rows].contiguous(), t[rows].contiguous()
        net.resetGradients()
        if stacked:
            net.run_draws(xb, tb, S)
        else:
            for _ in range(S):
                net.sample()
                net.run(xb, tb)
        loss, _ = net.loss_and_accuracy()
        if not np.isfinite(loss):
            raise FloatingPointError(f"active_learning: the loss is {loss} -- the run has diverged; no parameter was updated")
        net.update(opt)


def active_learning(opt, x_pool, y_pool, x_test, y_test, n_init, k, rounds, score=None, beta=None, epochs=5, device=None, diverse=False):
    """Pool-based active learning with the NLL criterion. x_pool (R x input_size fp32) / y_pool (R int32 class indices) are the
    pool and the labels an annotator would give, x_test / y_test the held-out rows; all device tensors. The first n_init pool
    rows start labelled. Each of `rounds` rounds trains ONE engine (built once from opt; training continues from round to
    round) for `epochs` passes over the labelled rows in their order of acquisition, evaluates it on the test rows
    (predict_classes: opt.testSamples draws), then acquires k rows of the unlabelled rest by `score` (FusedMLP.acquire with
    exclude = the labelled rows; beta as there; diverse=True: FusedMLP.acquire_diverse instead -- k rows spread over the
    network's last hidden representation, away from the labelled rows, weighted by `score`; beta must be None) and labels them. Returns one dict per round: labels (the labelled rows the
    round trained on), accuracy (percent), nll, acquired (the k rows chosen after it, best first). Deterministic for a given
    opt.seed: a second run gives the same curve."""
    if opt.get("criterion", "nll") != "nll":
        raise ValueError("active_learning: the curve is accuracy and NLL -- criterion = 'nll' only (FusedMLP.acquire itself "
                         "serves every criterion)")
    R, bs = int(x_pool.shape[0]), int(opt["batchSize"])
    if not bs <= int(n_init) <= R:
        raise ValueError(f"active_learning: n_init = {n_init} (opt.batchSize = {bs} .. R = {R})")
    if int(n_init) + int(k) * int(rounds) > R:
        raise ValueError(f"active_learning: n_init + k * rounds = {int(n_init) + int(k) * int(rounds)} exceeds the pool's {R} rows")
    if diverse and beta is not None:
        raise ValueError("active_learning: diverse=True selects deterministically (beta must be None)")
    net = FusedMLP(opt, device=device)
    opt = dict(opt, kl_in_update=bool(getattr(net, "kl_in_update", False)))
    S = int(opt["S"]) if opt.get("type", "vb") == "vb" else 1
    x = x_pool.reshape(R, -1)
    labelled = torch.zeros(R, dtype=torch.uint8, device=x.device)
    labelled[:int(n_init)] = 1
    order = torch.arange(int(n_init), device=x.device)
    curve = []
    net.prepare()
    for _ in range(int(rounds)):
        for _e in range(int(epochs)):
            _train_epoch(net, opt, x, y_pool, order, S)
        ev = net.predict_classes(x_test, targets=y_test, keep_probs=False)
        if diverse:
            got = net.acquire_diverse(x, int(k), score=score, exclude=labelled)
        else:
            got = net.acquire(x, int(k), score=score, exclude=labelled, beta=beta)
        new = got.indices[:got.n_selected].long()
        curve.append(dict(labels=int(order.numel()), accuracy=ev.accuracy, nll=ev.nll, acquired=new.cpu().tolist()))
        labelled[new] = 1
        order = torch.cat([order, new])
    return curve
