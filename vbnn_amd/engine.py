"""Fused whole-step engine: mlp.lua's protocol (resetGradients / sample / run / calc_lc) with the
elementwise modules folded into the GEMM epilogues, activations and packed operands resident in
HBM, one process per GPU and an RCCL all-reduce of the gradient arena after accGradParameters.

Per minibatch (main.lua:28-40):   resetGradients(); prepare(); S x { sample(); run(x, t) }
One `run` = forward of every VB layer (dual MFMA GEMM, Philox noise + ReLU + operand packing in the
epilogue), final Linear + LogSoftMax + ClassNLL, backward (gradInput GEMMs with the ReLU mask and the
dL/dv hand-off in the epilogue, accGradParameters GEMMs with the gradSum / KL-gradient epilogue).

Everything here is argument plumbing around include/vbnn_hip.h; torch is device memory, the
stream and torch.distributed.
"""
import contextlib
import ctypes as C
import functools
import math

import torch

from . import _lib as L
from . import partition
from .nn import Context, _DT, _Packed, _p, fill_normal


class _VB:
    pass


_NULL_CM = contextlib.nullcontext()


def _ordered(fn):
    """Engine entry points that launch or allocate: the body runs with the engine's stream as torch's current stream, that
    stream ordered behind whatever the caller queued on ITS current stream before the call (FusedMLP._on_stream)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with self._on_stream():
            return fn(self, *args, **kwargs)
    return wrapped


class _View:
    """A caller's 2-D fp32 tensor handed to a GEMM as it lies (ptr, row pitch): the raw minibatch of the fp32 path."""

    def __init__(self, t):
        self.t, self.ld = t, t.stride(0)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())


class _StepGraph:
    """A captured step (FusedMLP.capture_step): launch() replays it on the engine's stream."""

    def __init__(self, eng, handle, draws):
        self.eng, self.h, self.draws = eng, handle, draws
        k, n = C.c_int(), C.c_int()
        L.check(L.lib().vbnn_graph_info(self.h, C.byref(k), C.byref(n)))
        self.kernel_nodes, self.nodes = k.value, n.value

    def launch(self):
        # the replay reads the captured input buffers: it goes behind the copies the caller queued on its own stream
        with self.eng._on_stream():
            L.check(L.lib().vbnn_graph_launch(self.h))
        self.eng.draw += self.draws                      # the host's mirror of the device counter
        self.eng._first = False

    def close(self):
        if self.h:
            L.check(L.lib().vbnn_graph_destroy(self.h))
            self.h = None


class _PredictBuffers(list):
    """predict's operands per layer input (+ .r, the sequential bf16 forwards' throwaway noise factor)."""
    r = None


class PredictResult:
    """FusedMLP.predict's outputs for R minibatch rows. Device tensors: probs / log_probs (R x C fp32: the S-draw average
    1/S sum_s softmax(f_s(x)) and its log), entropy (H[p]), expected_entropy (1/S sum_s H(p_s)), mutual_info (their difference:
    the epistemic part), pred (int32, argmax p). With targets also Python floats: nll (mean -log p[t]) and accuracy (percent)
    of the averaged prediction, and mean_draw_nll / mean_draw_accuracy -- the mean over draws of each draw's NLL and accuracy,
    the two numbers test() returns. None without targets."""

    def __init__(self, probs, log_probs, entropy, expected_entropy, mutual_info, pred):
        self.probs, self.log_probs, self.entropy = probs, log_probs, entropy
        self.expected_entropy, self.mutual_info, self.pred = expected_entropy, mutual_info, pred
        self.nll = self.accuracy = self.mean_draw_nll = self.mean_draw_accuracy = None
        self.S, self.stacked, self.chunks = None, None, None


class RegressionPredictResult:
    """FusedMLP.predict_regression's outputs for R minibatch rows of D outputs. Device tensors: mean (R x D: 1/S sum_s f_s(x)),
    var (R x D: the population variance of the S draws per output, the epistemic part -- the total predictive variance is
    var + noise_var), row_var (R: its mean over the outputs); with targets row_sq_err (R: sum_d (t - mean)^2) and, with
    noise_var, row_log_lik (R: the log density of the equal-weight mixture of N(f_s(x), noise_var I) at t); draws (S x R x D)
    with keep_draws. With targets also Python floats: totals (the library's four sums), mse (of the predictive mean),
    mean_draw_mse (the mean over draws of each draw's MSE: test()'s number), log_lik (mean row_log_lik; None without noise_var)
    and mean_var.
    criterion = "gauss" (the network predicts its own noise; None for "mse"): noise_var (R x D: 1/S sum_s exp(s_c), the
    aleatoric part -- the total predictive variance is var + noise_var), row_noise_var (R: its mean over the outputs), and with
    targets mean_noise_var and mean_draw_nll (the mean over draws of each draw's Gaussian criterion: test()'s number); totals
    then has five sums, mean_draw_mse is None, draws is S x R x 2 D and row_log_lik / log_lik are those of the mixture of
    N(m_s, diag exp(s_s))."""

    def __init__(self, mean, var, row_var, row_sq_err, row_log_lik, draws):
        self.mean, self.var, self.row_var = mean, var, row_var
        self.row_sq_err, self.row_log_lik, self.draws = row_sq_err, row_log_lik, draws
        self.totals = self.mse = self.mean_draw_mse = self.log_lik = self.mean_var = None
        self.noise_var = self.row_noise_var = self.mean_noise_var = self.mean_draw_nll = None
        self.S, self.stacked, self.chunks = None, None, None


class PruneResult:
    """FusedMLP.prune's outcome: the signal-to-noise pruning of mainviz.lua:20-27 at one threshold per VB layer, and the pruned
    operand shadows (mu_p / var_p per layer, owned here) that predict() reads while this result is the engine's pruned view
    (FusedMLP.use_pruned / pruned). Per layer (lists, VB layer order): tau (the threshold: key < tau is pruned; one value
    repeated when scope = "global"), layers[li] = dict(n_pruned, W, fraction_pruned, mean_var, mean_pruned_var); the same five
    names as attributes are the totals over all layers -- n_pruned and mean_pruned_var are what mainviz.lua:22-27 prints
    (`pruned count`, `pruned var mean`; mean_pruned_var is nan when nothing was pruned, as the mean of an empty tensor).
    mask(li): the layer's `pruned` tensor (mainviz.lua:21) as an O x I bool tensor, produced on request by one more pack
    sweep of that layer. A result is a snapshot of the parameters it was taken from (version)."""

    def __init__(self, engine, scope, tau, stats, mu_p, var_p, version):
        self.engine, self.scope, self.version = engine, scope, version
        self.tau = [float(t) for t in tau]
        self.mu_p, self.var_p = mu_p, var_p
        self.stats = [tuple(float(x) for x in st) for st in stats]         # per layer: pruned, sum pruned vars, sum vars, W
        self.layers = [self._summary(*st) for st in self.stats]
        tot = self._summary(*[sum(col) for col in zip(*self.stats)]) if self.stats else self._summary(0.0, 0.0, 0.0, 0.0)
        self.n_pruned, self.W, self.fraction_pruned = tot["n_pruned"], tot["W"], tot["fraction_pruned"]
        self.mean_var, self.mean_pruned_var = tot["mean_var"], tot["mean_pruned_var"]

    @staticmethod
    def _summary(n, s_pruned, s_all, W):
        return dict(n_pruned=int(n), W=int(W), fraction_pruned=n / W if W else 0.0, mean_var=s_all / W if W else float("nan"),
                    mean_pruned_var=s_pruned / n if n else float("nan"))

    def mask(self, li):
        return self.engine._prune_mask(self, li)

    def compress(self):
        """The same pruning in compressed form (a SparsePruneResult: the kept weights only, CSR per layer): under that view
        predict() multiplies by the entries directly (vbnn_forward_sparse). Synchronises to check the entry counts."""
        return self.engine._compress(self)


class SparsePruneResult(PruneResult):
    """PruneResult.compress()'s outcome: a PruneResult (use_pruned / pruned take it unchanged; tau, layers, totals and the
    version guard are the dense result's) whose weights are per-layer CSR over output rows instead of dense shadows -- lists in
    VB layer order: row_ptr[li] (O + 1 offsets, int32 storage of the library's uint32), cols[li] (ascending within a row;
    int16 storage of uint16 when idx_bytes[li] == 2, int32 otherwise), mu_v[li] / var_v[li] (the packed dtype), nnz[li]
    (= W - n_pruned: a kept weight that is zero is still an entry). nbytes / dense_nbytes: device bytes of this form and of
    the dense shadows it replaces. It owns no dense shadows (mu_p / var_p are None): dropping the dense result frees them.
    to_dense(li) rebuilds them (for checking), mask(li) the layer's `pruned` tensor."""

    def __init__(self, base, row_ptr, cols, mu_v, var_v, nnz, idx_bytes, dense_nbytes):
        super().__init__(base.engine, base.scope, base.tau, base.stats, None, None, base.version)
        self.row_ptr, self.cols, self.mu_v, self.var_v = row_ptr, cols, mu_v, var_v
        self.nnz, self.idx_bytes = [int(n) for n in nnz], list(idx_bytes)
        self.nbytes = sum(t[li].numel() * t[li].element_size() for t in (row_ptr, cols, mu_v, var_v) for li in range(len(nnz)))
        self.dense_nbytes = int(dense_nbytes)

    def _coords(self, li):
        rp = self.row_ptr[li].to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])
        mask = 0xffff if self.idx_bytes[li] == 2 else 0xffffffff
        return rows, self.cols[li][:self.nnz[li]].to(torch.int64) & mask

    def to_dense(self, li):
        """(mu_p, var_p) of layer li as vbnn_prune_pack writes them: O x ld_w of the packed dtype, +0 wherever no entry is."""
        v = self.engine.vb[li]
        rows, cols = self._coords(li)
        out = []
        for vals in (self.mu_v[li], self.var_v[li]):
            d = torch.zeros(v.O, L.pad_ld(v.I), dtype=vals.dtype, device=vals.device)
            d[rows, cols] = vals[:self.nnz[li]]
            out.append(d)
        return tuple(out)

    def mask(self, li):
        v = self.engine.vb[li]
        m = torch.ones(v.O, v.I, dtype=torch.bool, device=self.row_ptr[li].device)
        rows, cols = self._coords(li)
        m[rows, cols] = False
        return m

    def compress(self):
        return self


class UnitPruneResult:
    """FusedMLP.prune_units' outcome: structured signal-to-noise pruning, whole hidden units by ||mu_o|| / ||sigma_o|| (the group
    form of mainviz.lua:20-21). Lists in VB layer order: tau (the threshold: a unit with key < tau goes; one value repeated when
    scope = "global"), keep[li] (the kept units, an ascending int32 device tensor), hidden (their counts: the widths of the
    compact network), layers[li] = dict(n_units, n_pruned, fraction_pruned); the same three names as attributes are the totals.
    n_weights / n_weights_before: weights of the VB layers plus the final Linear, after and before. A result is a snapshot of
    the parameters it was taken from (version); FusedMLP.compact(result) builds the smaller dense engine."""

    def __init__(self, engine, scope, multiple, tau, keep, sizes, n_classes, version):
        self.engine, self.scope, self.multiple, self.version = engine, scope, int(multiple), version
        self.tau = [float(t) for t in tau]
        self.keep = list(keep)
        self.hidden = [int(k.numel()) for k in self.keep]
        units = [int(o) for o in sizes[1:]]
        self.layers = [self._summary(o, o - n) for o, n in zip(units, self.hidden)]
        tot = self._summary(sum(units), sum(units) - sum(self.hidden))
        self.n_units, self.n_pruned, self.fraction_pruned = tot["n_units"], tot["n_pruned"], tot["fraction_pruned"]
        self.n_weights_before = self._weights([int(sizes[0])] + units, n_classes)
        self.n_weights = self._weights([int(sizes[0])] + self.hidden, n_classes)

    @staticmethod
    def _summary(n_units, n_pruned):
        return dict(n_units=int(n_units), n_pruned=int(n_pruned), fraction_pruned=n_pruned / n_units if n_units else 0.0)

    @staticmethod
    def _weights(sizes, n_classes):
        return sum(sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1)) + sizes[-1] * int(n_classes)


class FusedMLP:
    def __init__(self, opt, device=None, world_size=1, rank=0, process_group=None, force_reduce=False, stream=None):
        """stream: a torch.cuda.Stream for this engine's launches (a library context of its own, hence its own reduction
        scratch and tickets): two engines on two streams may compute on one device at the same time. Default: the
        device's shared context on torch's current stream."""
        self.opt = opt
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # opt.cu_budget (data-parallel runs): the engine's launches go on a stream of the library's own limited to that many
        # compute units, leaving the rest to RCCL's channels for the whole step (Context.with_cu_budget)
        cu_budget = int(opt.get("cu_budget", 0) or 0)
        if cu_budget > 0:
            assert stream is None, "cu_budget creates the engine's stream itself"
            self.ctx = Context.with_cu_budget(self.device.index or 0, cu_budget)
        else:
            self.ctx = Context.get(self.device) if stream is None else Context(self.device.index or 0, stream=stream)
        with self._on_stream():                # every allocation / fill below is queued on the engine's own stream
            self._build(opt, world_size, rank, process_group, force_reduce)

    def _on_stream(self):
        """With a stream of the engine's own (stream= / cu_budget) the library launches there while torch's fills, copies
        and allocations go to torch's CURRENT stream: make the ordering the engine's job. The engine stream
        first waits for the caller's current stream (a minibatch copied there is complete before a kernel reads it), then
        is torch's current stream for the body (the engine's own zero fills / repeats queue in launch order). Results are
        ordered for the caller by join() or any device synchronisation (loss_and_accuracy does one)."""
        ts = self.ctx.torch_stream
        if ts is None:
            return _NULL_CM
        cur = torch.cuda.current_stream(self.device)
        if cur != ts:
            ts.wait_stream(cur)
        return torch.cuda.stream(ts)

    def join(self):
        """The caller's current stream waits for everything this engine has queued (no host block)."""
        ts = self.ctx.torch_stream
        if ts is not None:
            cur = torch.cuda.current_stream(self.device)
            if cur != ts:
                cur.wait_stream(ts)

    def _build(self, opt, world_size, rank, process_group, force_reduce):
        self.dtype = opt.get("dtype", "bf16")
        self.code, self.tdt = _DT[self.dtype]
        self.mode = opt.get("mode", "lrt")
        assert self.mode in ("wn", "lrt")
        self.seed = int(opt.get("seed", 3))
        self.world, self.rank, self.pg = world_size, rank, process_group
        self.reduce = world_size > 1 or force_reduce
        self._exchange = None                 # made on first use (vbnn_amd/comm.py): RCCL through the C ABI
        self.exchange_dtype = str(opt.get("exchange_dtype", "f32"))      # "bf16": the optional half-size exchange (_reduce)
        assert self.exchange_dtype in ("f32", "bf16")
        self._stage, self._staged = None, []
        # opt.exchange_mode = "sharded" (or VBNN_EXCHANGE_MODE=sharded): the SHARDED-UPDATE exchange instead of north_star's
        # all-reduce (partition.py): reduce-scatter of the likelihood gradients by layer rows, update() on this
        # rank's rows only (Adam state + fp32 master rows sharded), all-gather of the operand shadows + prior statistics. An option
        # beside the all-reduce, never its replacement: update() is then part of every step.
        import os as _os
        self.exchange_mode = str(opt.get("exchange_mode", _os.environ.get("VBNN_EXCHANGE_MODE", "")) or "allreduce")
        assert self.exchange_mode in ("allreduce", "sharded")
        self.sharded = self.reduce and self.exchange_mode == "sharded"
        self._params_stale = False            # sharded: the fp32 means / lvars of OTHER ranks' rows are stale after an update
        self._dx_first_opt = opt.get("dx_first", None)      # None: decided from the layer sizes once they are known (below)
        self.fuse_kl = bool(opt.get("fuse_kl", True))
        # "nll": LogSoftMax + ClassNLLCriterion (mlp.lua:30-32); "mse": nn.MSECriterion on the final Linear's outputs
        # (BASELINE.json configs[4], a regression target of n_classes dimensions -- not in the reference); "gauss": the
        # heteroscedastic Gaussian likelihood (vbnn_gauss_nll_forward) -- the final Linear's n_classes = 2 D outputs are D means
        # and D log noise variances, the targets R x D; opt.logvar_clamp = (s_min, s_max) clamps the log variance
        self.criterion = opt.get("criterion", "nll")
        assert self.criterion in ("nll", "mse", "gauss")
        self.logvar_clamp = tuple(float(v) for v in opt.get("logvar_clamp", (-20.0, 20.0)))
        if self.criterion == "gauss":
            if int(opt["n_classes"]) % 2:
                raise ValueError(f"criterion = 'gauss': the final Linear holds D means and D log variances (n_classes = "
                                 f"{opt['n_classes']} is odd)")
            if not (len(self.logvar_clamp) == 2 and self.logvar_clamp[0] <= self.logvar_clamp[1]):
                raise ValueError(f"opt.logvar_clamp = {self.logvar_clamp}: (s_min, s_max) with s_min <= s_max")
        self.kl_from_shadows = self.dtype == "bf16" and bool(opt.get("kl_from_shadows", True))
        # opt.kl_in_update: the gradient arena holds the LIKELIHOOD parts only (vbnn_dw_args.kl_scale = 0) and update() adds the
        # KL gradient from the fp32 means / lvars (vbnn_update_desc.kl_add) -- exact, where the epilogue's shadow form carries
        # bf16(sigma^2) / var_hat - 1; in a data-parallel run the exchanged sum is then a pure sum of likelihoods.
        # DEFAULT (r04): on wherever the fused epilogue would otherwise take the KL terms from the bf16 shadows -- the exact form is
        # what every host gets unless it asks for the A/B form (kl_in_update = False); fp32 epilogues read the fp32 parameters
        # and are exact either way, so they keep the total gradients in the arena.
        self.kl_in_update = bool(opt.get("kl_in_update", self.kl_from_shadows and self.fuse_kl and self.mode == "lrt"))
        if self.sharded:
            assert self.fuse_kl and self.mode == "lrt" and self.exchange_dtype == "f32" and not opt.get("overlap", False), \
                "exchange_mode = sharded: the fused LRT engine, fp32 sums, one compute stream"
            # bf16 only: there the step reads the parameters through the operand shadows alone (GEMM operands and the
            # accGradParameters epilogue's sigma^2: vbnn_dw_args.var_s) -- which is what is gathered, at half the bytes of the
            # gradients. The fp32 configuration's epilogue forms exp(lvars) from the fp32 master rows, which other ranks hold stale,
            # and its "shadows" are as large as the gradients: nothing to gain there.
            assert self.dtype == "bf16" and self.kl_from_shadows, "exchange_mode = sharded: the bf16 configuration (operand shadows)"
            self.kl_in_update = True          # what is reduce-scattered is a pure sum of likelihood parts; the slice update adds the KL
        assert not self.kl_in_update or (self.fuse_kl and self.mode == "lrt"), "kl_in_update: the fused LRT engine"
        # optional second HIP stream (+ its own context, hence its own reduction scratch) for the accGradParameters
        # GEMMs. Measured on MI355X (wide config): 1.32 ms with, 1.29 ms without -- two 512-block GEMMs sharing the
        # CUs thrash each other's L2 panels more than the staggered epilogues save -- so it is off by default.
        self.overlap = bool(opt.get("overlap", False))
        self.head_step = bool(opt.get("head_step", True))     # the fused head's forward + backward as one call (A/B, tests: False = two calls)
        if self.overlap:
            self._side = torch.cuda.Stream(device=self.device)
            self.ctx2 = Context(self.device.index or 0, stream=self._side)
        self.B, self.S = float(opt.get("B", 1e6)), float(opt.get("S", 1))
        hidden = list(opt["hidden"])
        sizes = [opt["input_size"]] + hidden
        self.n_classes = opt["n_classes"]
        self.sizes = sizes
        weights = [sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1)]
        self.dx_first = bool(self._dx_first_opt) if self._dx_first_opt is not None else (2 * min(weights) <= max(weights))
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # ---- gradient arena: [gradWeight | gradSum | gradBias] per VB layer, then the final Linear (partition.arena_layout)
        # early_lv: layers whose accGradParameters runs as two launches (d/dlvars first) so that its exchange starts one
        # GEMM earlier; default: the big layers of a data-parallel run
        el = opt.get("early_lv", None)
        if el is None:
            el = [(world_size > 1 or force_reduce) and self.mode == "lrt" and bool(opt.get("fuse_kl", True)) and
                  sizes[i] * sizes[i + 1] >= (1 << 22) for i in range(len(hidden))]
        elif isinstance(el, bool):
            el = [el and self.mode == "lrt"] * len(hidden)
        self.early_lv = list(el)
        lay, fin, n_g, self._bucket_ranges = partition.arena_layout(sizes, self.n_classes, self.early_lv)
        self._lay = lay
        # opt.exchange = "p2p" (or VBNN_EXCHANGE=p2p): the direct reduce-scatter + all-gather over peer-mapped arenas
        # (vbnn_p2p_*, csrc/p2p.hip) instead of RCCL; that exchange owns the arena (an IPC-exportable allocation of the library's)
        import os
        self.exchange_kind = str(opt.get("exchange", os.environ.get("VBNN_EXCHANGE", "")) or "")
        n_layers = len(hidden)
        self._plan = partition.sharded_plan(lay, world_size) if self.sharded else None
        arena_extra = None
        if self.reduce and self.exchange_kind == "p2p":
            assert self.exchange_dtype == "f32", "the p2p exchange sums fp32 arenas"
            from .comm import P2PExchange
            n_arena = (n_g + 3) // 4 * 4
            if self.sharded:            # what the sharded exchange all-gathers lives in the peer-mapped arena too
                n_arena += sum(2 * _Packed.floats(sizes[i + 1], sizes[i], self.tdt) for i in range(n_layers)) + 8 * world_size * n_layers
            self._exchange = P2PExchange(self.ctx, rank, world_size, n_arena, process_group)
            self.grads = self._exchange.arena[:n_g]
            arena_extra = self._exchange.arena[(n_g + 3) // 4 * 4:]
        else:
            self.grads = torch.zeros(n_g, **f32)

        def carve(n_floats):
            nonlocal arena_extra
            if arena_extra is None:
                return None
            piece, arena_extra = arena_extra[:n_floats], arena_extra[n_floats:]
            return piece

        def take(span, shape):
            return self.grads[span[0]:span[0] + span[1]].view(*shape)

        var_init = opt["var_init"] if not opt.get("msr_init") else None
        self.vb = []
        for li in range(len(hidden)):
            I, O = sizes[li], sizes[li + 1]
            v = _VB()
            v.I, v.O, v.layer_id = I, O, li
            v.var_init = var_init if var_init is not None else 2.0 / I           # VBLinear.lua:12-16
            v.means = torch.zeros(O, I, **f32)                                     # :22-23
            v.lvars = torch.full((O, I), math.log(v.var_init), **f32)              # :18
            v.bias = torch.zeros(O, **f32)                                         # :13
            v.weight = torch.zeros(O, I, **f32) if self.mode == "wn" else None
            # with fuse_kl the first two blocks hold the TOTAL gradients d/dmeans, d/dlvars
            # (likelihood / S + KL, VBLinear.lua:90-98); otherwise the reference's gradWeight / gradSum
            v.gradWeight = take(lay[li]["mu"], (O, I))
            v.gradSum = take(lay[li]["lv"], (O, I))
            v.gradBias = take(lay[li]["bias"], (O,))
            v.bucket = self.grads[lay[li]["bucket"][0]:lay[li]["bucket"][1]]
            v.stats = torch.zeros(4, dtype=torch.float64, device=dev)
            nf = _Packed.floats(O, I, self.tdt)
            v.mu_s = _Packed(O, I, self.tdt, dev, storage=carve(nf) if self.sharded else None)
            v.var_s = _Packed(O, I, self.tdt, dev, storage=carve(nf) if self.sharded else None)
            if li > 0:
                v.muT_s, v.varT_s = _Packed(I, O, self.tdt, dev), _Packed(I, O, self.tdt, dev)
            else:
                v.muT_s = v.varT_s = None
            self.vb.append(v)
        H = sizes[-1]
        self.weight3 = torch.zeros(self.n_classes, H, **f32)
        self.bias3 = torch.zeros(self.n_classes, **f32)
        self.gradWeight3 = take(fin["weight"], (self.n_classes, H))
        self.gradBias3 = take(fin["bias"], (self.n_classes,))
        self.bucket3 = self.grads[fin["bucket"][0]:fin["bucket"][1]]
        # the final Linear's gradients sit right behind the last VB layer's in the arena: ONE all-reduce covers both (the
        # head's backward finishes before that layer's accGradParameters is even launched), a collective fewer per step
        self.bucket_tail = self.grads[lay[-1]["bucket"][0]:fin["bucket"][1]]
        for li, v in enumerate(self.vb):                         # the layer's message(s): [d/dlvars] early (optional), the rest late
            v.msg_early = self.grads[lay[li]["early"][0]:lay[li]["early"][1]] if lay[li]["early"] else None
            v.msg_late = self.grads[lay[li]["late"][0]:lay[li]["late"][1]]
        self.w3_s = _Packed(self.n_classes, H, self.tdt, dev)
        self.w3T_s = _Packed(H, self.n_classes, self.tdt, dev)
        if self.sharded:
            # every rank's statistics of its row slices, [world][layers][4] doubles, gathered after the slice update; and this
            # rank's block of it as the in / out `stats` of the slice update (in: the whole layer's pre-update statistics)
            st = carve(8 * world_size * n_layers)
            self._stat_parts = (st.view(torch.float64) if st is not None else
                                torch.zeros(4 * world_size * n_layers, dtype=torch.float64, device=dev)).view(world_size, n_layers, 4)
            self._stat_parts.zero_()
        self._acc = torch.zeros(2, dtype=torch.float64, device=dev)
        self._corr = torch.zeros(1, dtype=torch.int32, device=dev)
        self._lc = torch.zeros(1, dtype=torch.float64, device=dev)
        self.draw = 0
        # opt.device_draw: the draw counter lives in device memory (vbnn_fwd_args.draw_dev), sample() is a device-side
        # increment (vbnn_sample) -- what makes a step CAPTURABLE (capture_step): every replay of the graph advances the
        # counter and draws its own noise. `self.draw` stays the host's mirror of the count.
        self.device_draw = bool(opt.get("device_draw", False))
        assert not self.device_draw or self.mode == "lrt", "device_draw: LRT (weight noise draws in vbnn_wn_sample, a host-addressed launch)"
        self._draw_dev = torch.zeros(1, dtype=torch.int32, device=dev) if self.device_draw else None
        self._map = False
        self._first = True
        self._draws_run = 0
        self._exchange_now = True
        self._exchange_done = False
        self._N = None
        self._argcache = {}
        self._rpd = 0            # > 0 inside run_draws: rows per Monte-Carlo draw of the stacked minibatch
        self._x_in = None        # fp32: the raw minibatch of the current run, read in place by layer 1's GEMMs
        self._draws = None
        self._shadows_ready = False       # prepare() / update() have packed the operand shadows (predict prepares otherwise)
        self._pruned = None               # the pruned view predict() reads its operands from (use_pruned), or None
        self._pver = 0                    # parameter version: a pruned view is a snapshot of ONE version (prune / predict)
        self._prune_ws = None
        self._held = None                 # the held pruning masks (hold_pruned): one O x I uint8 tensor per VB layer, 1 = frozen
        self._held_counts = None
        self.init_parameters()

    # mlp.lua:47-55 (He rule for every weight, bias zero) + the bench's non-degenerate means
    # (means ~ N(0, sqrt(2/I)); the shipped mu_init = 0 gives an all-zero net).
    @_ordered
    def init_parameters(self):
        self._pver += 1
        for v in self.vb:
            fill_normal(v.means, self.seed, L.STREAM_HEINIT, v.layer_id, 0, scale=math.sqrt(2.0 / v.I), ctx=self.ctx)
            v.bias.zero_()
        fill_normal(self.weight3, self.seed, L.STREAM_HEINIT, len(self.vb), 0, scale=math.sqrt(2.0 / self.sizes[-1]), ctx=self.ctx)
        self.bias3.zero_()

    # ---- buffers that depend on the local batch size
    def _alloc_batch(self, N):
        if self._N == N:
            return
        self._N = N
        self._argcache = {}                     # the argument blocks hold pointers into the buffers allocated below
        dev, tdt = self.device, self.tdt
        lib = L.lib()
        # K-major operands (vbnn_kmajor_supported): when a layer's parameter-gradient GEMM reads x and g as the forward
        # / gradInput GEMMs hold them, nobody has to write x^T, (x.x)^T, g^T, gv^T for it; when its gradInput GEMM reads
        # mu, sigma^2 as stored, the parameter sweep writes no transposed shadows. The library decides by shape; the
        # fused configuration that takes that kernel is bf16, LRT, total gradients from the epilogue, one draw.
        km_ok = (self.opt.get("dtype", "f32") == "bf16") and not self.opt.get("keep_transposes", False)
        # fp32 (the general kernel, gemm_v1.h): every GEMM takes its operands as the producer left them -- the minibatch raw,
        # x.x formed in registers, x / g / mu / sigma^2 K-major, the bias gradient from a synthetic row of ones -- so the fp32
        # step has no packing launch, no squared and no transposed copy of anything. (Not with an exchange: the two-launch
        # accGradParameters of a data-parallel run wants x.x as an operand.)
        self.f32_direct = (self.dtype == "f32" and self.mode == "lrt" and not self.reduce and
                           not self.opt.get("keep_transposes", False))
        need_prepare = False
        for li, v in enumerate(self.vb):
            last_fused = (v is self.vb[-1]) and self.n_classes <= 16 and self.criterion == "nll"
            v.bias_from_dw = (v.I % 256 != 0) and not last_fused
            if self.f32_direct:
                v.dw_km, v.x_pad256, v.early_ok, v.dx_km = True, False, False, li > 0
                v.use_muT = False
                continue
            # (the K-major launches take the epilogue's fast protocol, which reads mu / sigma^2 from the operand shadows
            # only: vbnn_dw_args.mu_s / var_s are REQUIRED for them, include/vbnn_hip.h)
            km = lib.vbnn_ctx_kmajor_supported_dw(self.ctx.h, v.I, v.O, N, 1 if v.bias_from_dw else 0) if (
                km_ok and self.mode == "lrt" and self.fuse_kl and int(self.S) == 1 and self.kl_from_shadows) else 0
            v.dw_km = km > 0
            v.x_pad256 = km == 2         # the split launch of gemm_v3 reads x / x.x in whole 256-column tiles
            # the two-launch form of accGradParameters (early d/dlvars message) needs either the transposed operands or the
            # plain K-major launch of the two-pass kernel; the few-tile K-major launches compute both GEMMs in one grid
            v.early_ok = (not v.dw_km) or bool(not v.bias_from_dw and lib.vbnn_ctx_kmajor_supported(self.ctx.h, v.I, v.O, N))
            v.dx_km = bool(km_ok and li > 0 and lib.vbnn_ctx_kmajor_supported(self.ctx.h, v.I, N, v.O))
            use_muT = (li > 0) and not v.dx_km
            if use_muT and not getattr(v, "use_muT", True):
                need_prepare = True                            # the shadows' transposes were being skipped: refresh them
            v.use_muT = use_muT
        for v in self.vb:
            # Layers whose parameter-gradient GEMM is not the whole-tile 256 x 256 kernel anyway (I % 256 != 0: the
            # 784-wide input layer) get their bias gradient from that GEMM: x^T carries one more row, all ones, whose
            # output row is sum_n g[n][o] (vbnn_dw_args.gradBias). Written once here: the packers only touch rows < I.
            # K-major the row of ones is COLUMN I of x (in the K padding of the forward operand, where the packed
            # weights are zero, so the forward does not see it).
            extra = 1 if v.bias_from_dw else 0
            if self.f32_direct:
                v.x_s = _Packed(N, v.I, tdt, dev)        # (layer 1: used only when the raw minibatch cannot be read in place)
                v.x2_s = None
                v.xT_s = v.x2T_s = v.gT_s = v.gvT_s = None
                v.mixed_g = False
                v.g_s, v.gv_s = _Packed(N, v.O, tdt, dev), _Packed(N, v.O, tdt, dev)
                v.r = torch.zeros(N, v.O, dtype=tdt, device=dev)
                continue
            xcols = v.I + (extra if v.dw_km else 0)
            if v.x_pad256:
                xcols = (xcols + 255) // 256 * 256
            v.x_s = _Packed(N, xcols, tdt, dev)
            v.x2_s = _Packed(N, xcols, tdt, dev)
            if v.dw_km and v.bias_from_dw:
                v.x_s.t[:, v.I] = 1.0
            # opt.mixed_g (A/B, off): the last VB layer below the fused head gets g, gv from vbnn_head_backward TRANSPOSED as
            # well, and accGradParameters reads x K-major with g K-contiguous. Measured in the step (r02): the GEMM 220 ->
            # 216 us, the head's backward 32 -> 40 us for the extra stores: a net loss, so it stays off.
            v.mixed_g = bool(v.dw_km and v is self.vb[-1] and self.n_classes <= 16 and self.criterion == "nll" and
                             self.opt.get("mixed_g", False) and lib.vbnn_ctx_kmajor_supported(self.ctx.h, v.I, v.O, N) and not v.bias_from_dw)
            if v.dw_km:
                v.xT_s = v.x2T_s = v.gT_s = v.gvT_s = None
                if v.mixed_g:
                    v.gT_s, v.gvT_s = _Packed(v.O, N, tdt, dev), _Packed(v.O, N, tdt, dev)
            else:
                v.xT_s, v.x2T_s = _Packed(v.I + extra, N, tdt, dev), _Packed(v.I + extra, N, tdt, dev)
                v.gT_s, v.gvT_s = _Packed(v.O, N, tdt, dev), _Packed(v.O, N, tdt, dev)
                if v.bias_from_dw:
                    v.xT_s.t[v.I, :N] = 1.0
            v.g_s, v.gv_s = _Packed(N, v.O, tdt, dev), _Packed(N, v.O, tdt, dev)
            v.r = torch.zeros(N, v.O, dtype=tdt, device=dev)          # z / (2 sqrt(v)), stored in the operand type
        H = self.sizes[-1]
        self.h_s = _Packed(N, H, tdt, dev)            # input of the final Linear
        self.hT_s = _Packed(H, N, tdt, dev)
        self.logits = torch.zeros(N, self.n_classes, dtype=torch.float32, device=dev)
        self.g_logits = torch.zeros(N, self.n_classes, dtype=torch.float32, device=dev)
        self.out = torch.zeros(N, self.n_classes, dtype=torch.float32, device=dev)
        self.g3_s = _Packed(N, self.n_classes, tdt, dev)
        self.g3T_s = _Packed(self.n_classes, N, tdt, dev)
        # the fused head's logits from the last VB layer's forward tiles (vbnn_fwd_args.head_slots): where the library's forward
        # of that layer can carry them, the head never re-reads h. opt.head_from_h = True keeps the head's own pass over h (A/B).
        vl = self.vb[-1]
        self.n_head_slots, self.head_slots = 0, None
        if self.n_classes <= 16 and self.criterion == "nll" and not self.device_draw and not self.opt.get("head_from_h", False):
            ns = lib.vbnn_forward_head_slots(self.ctx.h, self.code, N, vl.I, vl.O, self.n_classes)
            if ns > 0:
                self.n_head_slots, self.head_slots = ns, torch.zeros(ns * N * 16, dtype=torch.float32, device=dev)
        if need_prepare:
            self.prepare()

    # ---- mlp.lua:62-67. Nothing is zeroed: the first accGradParameters of the minibatch overwrites the gradients
    # and the first criterion pass overwrites the loss / hit accumulators.
    def resetGradients(self):
        self._first = True
        self._draws_run = 0          # sequential draws since the reset: the exchange leaves with the LAST one (run)
        self._exchange_done = False

    # ---- once per minibatch, after the parameters changed: VBLinear:compute_prior (VBLinear.lua:77-88)
    # fused with the packing of the GEMM shadows.
    @_ordered
    def prepare(self):
        lib = L.lib()
        self._shadows_ready = True                             # (predict: the operand shadows hold the parameters)
        if self._params_stale:
            # after a sharded update: every rank already holds what this sweep would produce -- the gathered operand shadows, the
            # combined prior statistics, the packed final weight (_update_sharded; "update leaves what prepare would" is a test)
            # -- while the fp32 rows of other ranks are stale. No sweep, and NO collective hidden in here: only the
            # transposed shadows of a layer that did not keep them so far are rebuilt, locally, from the gathered ones.
            for v in self.vb:
                if v.muT_s is not None and getattr(v, "use_muT", True):
                    L.check(lib.vbnn_transpose_packed(self.ctx.h, self.code, v.mu_s.ptr, v.mu_s.ld, v.O, v.I, v.muT_s.ptr, v.muT_s.ld))
                    L.check(lib.vbnn_transpose_packed(self.ctx.h, self.code, v.var_s.ptr, v.var_s.ld, v.O, v.I, v.varT_s.ptr, v.varT_s.ld))
            return
        self._pver += 1                                       # re-packed from the fp32 parameters: a caller may have changed them
        if self.mode == "lrt":                                # one call: a sweep per layer + ONE finish kernel
            descs = (L.PrepDesc * len(self.vb))()
            for k, v in enumerate(self.vb):
                descs[k] = L.PrepDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, mu_s=v.mu_s.ptr, var_s=v.var_s.ptr,
                                      ld_w=v.mu_s.ld, muT_s=v.muT_s.ptr if (v.muT_s and getattr(v, "use_muT", True)) else None,
                                      varT_s=v.varT_s.ptr if (v.varT_s and getattr(v, "use_muT", True)) else None,
                                      ld_wT=v.muT_s.ld if v.muT_s else 0,
                                      stats=_p(v.stats))
            w3 = L.PackDesc(src=_p(self.weight3), rows=self.n_classes, cols=self.sizes[-1], ld_src=self.sizes[-1],
                            dst=self.w3_s.ptr, ld_dst=self.w3_s.ld, dstT=self.w3T_s.ptr, ld_dstT=self.w3T_s.ld)
            if self._held is not None:                        # a held pruning mask: +0 shadows, the kept network's statistics
                L.check(lib.vbnn_prepare_masked(self.ctx.h, self.code, len(self.vb), descs, self._held_ptrs(), C.byref(w3)))
            else:
                L.check(lib.vbnn_prepare(self.ctx.h, self.code, len(self.vb), descs, C.byref(w3)))
            return
        for v in self.vb:
            L.check(lib.vbnn_compute_prior(self.ctx.h, _p(v.means), _p(v.lvars), v.O * v.I, None, None, None, _p(v.stats)))
        L.check(lib.vbnn_pack(self.ctx.h, self.code, L.PACK_COPY, _p(self.weight3), None, self.sizes[-1],
                              self.n_classes, self.sizes[-1], self.w3_s.ptr, self.w3_s.ld, self.w3T_s.ptr, self.w3T_s.ld))

    def _lrt(self):
        return self.mode == "lrt" and not self._map

    # ---- measurement hook (bench.py): when `self.probe` is (layer index, dict), every launch of that layer's three
    # GEMM families is bracketed by HIP events on the launch stream; bench.py reads the elapsed times after the
    # timed region. Off (None) it costs nothing.
    probe = None

    def _probed(self, name, li):
        import contextlib
        if self.probe is None or (self.probe[0] != li and self.probe[0] != "all"):
            return contextlib.nullcontext()
        if self.probe[0] == "all":                       # lab (tools/overlap_standin.py): every layer's launches, keyed by layer
            name = f"{name}[{li}]"
        eng = self

        class _Bracket:
            def __enter__(self_inner):
                self_inner.e0 = torch.cuda.Event(enable_timing=True)
                self_inner.e1 = torch.cuda.Event(enable_timing=True)
                self_inner.e0.record()

            def __exit__(self_inner, *exc):
                self_inner.e1.record()
                eng.probe[1].setdefault(name, []).append((self_inner.e0, self_inner.e1))
                return False
        return _Bracket()

    def _probed_part(self, name, li):
        """The two launches of an early-message accGradParameters separately: only in the lab's all-layers probe."""
        if self.probe is None or self.probe[0] != "all" or not self._early(self.vb[li], self._lrt()):
            return _NULL_CM
        return self._probed(name, li)

    # ---- VBLinear:clamp_to_map on every VB layer (mlp.lua:88-91): the forward uses the means as weights.
    @_ordered
    def clamp_to_map(self):
        self._map = True
        if self.mode == "wn":                 # the weight shadows currently hold a sampled draw: repack the means
            lib = L.lib()
            for v in self.vb:
                L.check(lib.vbnn_pack(self.ctx.h, self.code, L.PACK_COPY, _p(v.means), None, v.I, v.O, v.I,
                                      v.mu_s.ptr, v.mu_s.ld, v.muT_s.ptr if v.muT_s else None,
                                      v.muT_s.ld if v.muT_s else 0))

    # ---- mlp:test (mlp.lua:86-107): `quicktest` = one MAP pass, otherwise the average over testSamples draws.
    # The reference's `run` also back-propagates at test time and throws the gradients away; here the test pass
    # is forward + criterion only. Returns (mean error, accuracy in percent) of THIS rank's rows.
    def test(self, inputs, targets):
        N = inputs.shape[0]
        self.prepare()
        draws = 1 if self.opt.get("quicktest") else int(self.opt["testSamples"])
        err = acc = 0.0
        for _ in range(draws):
            self._first = True                      # this draw's criterion pass overwrites the accumulators
            if self.opt.get("quicktest"):
                self.clamp_to_map()
            else:
                self.sample()
            self.run(inputs, targets, backward=False)
            loss, correct = self.loss_and_accuracy()
            err += loss * self.world            # the criterion divides by the global batch; this is the local mean
            acc += 100.0 * correct / N
        return err / draws, acc / draws

    # ---- the posterior predictive (vbnn_head_predict): what mlp:test averages as per-draw criteria (mlp.lua:86-107, main.lua:55-74),
    # averaged as PROBABILITIES, with the per-example uncertainty of visualize.lua:66-100 (show_uncertainties). A forward-only
    # path on buffers of its own: no r, no transposed outputs, no head slots, no squares out of the last layer, and nothing of
    # the training step (operands it produces, gradient arena, loss accumulators, batch buffers, argument cache) is written.
    # It reads the operand shadows as prepare() / update() leave them -- on an engine that has had neither it calls prepare()
    # first, as test() does; after changing the parameters by hand call prepare(), as before run() -- or draws its own weights
    # from means / lvars (WN).
    @_ordered
    def predict(self, inputs, S=None, targets=None, map=False, row0=None):
        """p(y | x, D) ~ 1/S sum_s softmax(f_s(x)) over draws self.draw + 1 .. self.draw + S -- the draws test() with
        opt.testSamples = S consumes -- and `self.draw` advances by S (host and device counter). map=True (or opt.quicktest):
        one pass on the means, S = 1, no draw consumed. row0: the global row of inputs[0] that addresses the noise (default:
        this rank's first row, as run()). Returns a PredictResult of this rank's rows (no collective, as test())."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        Cn = self.n_classes
        if Cn > 16:
            raise ValueError(f"predict: the predictive head takes at most 16 classes (n_classes = {Cn})")
        if self.criterion != "nll":
            raise ValueError(f"predict: a class-probability predictive needs the NLL criterion (criterion = '{self.criterion}' has "
                             "none: use predict_regression)")
        map = bool(map or self.opt.get("quicktest"))
        S = 1 if map else int(self.opt["testSamples"] if S is None else S)
        if S < 1:
            raise ValueError(f"predict: S = {S} draws (at least one)")
        x = inputs.reshape(inputs.shape[0], -1)
        R = x.shape[0]
        assert x.shape[1] == self.sizes[0] and x.dtype == torch.float32 and x.is_cuda and R > 0
        if targets is not None:
            assert targets.dtype == torch.int32 and targets.is_cuda and targets.numel() == R
            targets = targets.contiguous()
        row0 = self.rank * R if row0 is None else int(row0)
        if not self._shadows_ready:            # a fresh engine: the shadows test() would have prepared
            self.prepare()
        if self._pruned is not None:           # a pruned view replaces the operand shadows: it must be of THESE parameters
            if self.mode == "wn" and not map:
                raise ValueError("predict: weight-noise draws under a pruned view are not supported -- they sample from the fp32 "
                                 "means / lvars, which the view does not replace (use map=True, or mode = 'lrt')")
            if self._pruned.version != self._pver:
                raise RuntimeError("predict: the pruned view was taken from older parameters (update / prepare / init_parameters "
                                   "ran since): prune() again, or use_pruned(None)")
        lrt = self.mode == "lrt" and not map
        stacked = self._predict_stacked(R, S, lrt)
        cap = max(1, int(self.opt.get("predict_rows", 32768)))
        Rc = max(1, min(R, cap // S if stacked else cap))           # minibatch rows per chunk: S Rc (stacked) or Rc operand rows
        bufs = self._predict_buffers(S * Rc if stacked else Rc, lrt)
        wts = self._predict_weights() if self.mode == "wn" else None
        f32 = dict(dtype=torch.float32, device=self.device)
        res = PredictResult(torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32), torch.empty(R, **f32), torch.empty(R, **f32),
                            torch.empty(R, **f32), torch.empty(R, dtype=torch.int32, device=self.device))
        n_chunks = (R + Rc - 1) // Rc
        totals = torch.zeros(n_chunks, 4, dtype=torch.float64, device=self.device) if targets is not None else None
        state = torch.empty(Rc, Cn + 3, **f32) if not stacked else None
        d0 = self.draw + 1                                           # the first draw's counter (sample() then run())
        nl = len(self.vb)
        a = L.PredictArgs(w3=self.w3_s.ptr, ld_w=self.w3_s.ld, bias=_p(self.bias3), H=self.sizes[-1], C=Cn, S=S,
                          form=L.PREDICT_STACKED if stacked else L.PREDICT_ACCUMULATE, state=_p(state))
        for k in range(n_chunks):
            c0 = k * Rc
            rows = min(Rc, R - c0)
            xc = x[c0:c0 + rows]
            a.h, a.ld_h = bufs[nl].x.ptr, bufs[nl].x.ld
            a.R = rows
            a.target = C.c_void_p(targets.data_ptr() + 4 * c0) if targets is not None else None
            a.totals = C.c_void_p(totals[k].data_ptr()) if totals is not None else None
            for name, t in (("probs", res.probs), ("log_probs", res.log_probs)):
                setattr(a, name, C.c_void_p(t.data_ptr() + 4 * Cn * c0))
            for name, t in (("entropy", res.entropy), ("expected_entropy", res.expected_entropy), ("mutual_info", res.mutual_info),
                            ("pred", res.pred)):
                setattr(a, name, C.c_void_p(t.data_ptr() + 4 * c0))
            if stacked:                        # every draw in one pass: the chunk stacked S times as rows, draw s = rows [s rows, (s+1) rows)
                if wts is not None:            # (weight noise: S = 1)
                    self._predict_wn_sample(wts, None if map else d0)
                self._predict_forward(bufs, wts, xc, S * rows, rows if S > 1 else 0, d0, row0 + c0, lrt)
                L.check(lib.vbnn_head_predict(ctx, code, C.byref(a)))
                continue
            for s in range(S):                 # one draw per forward, the running state between the head's launches
                if wts is not None:
                    self._predict_wn_sample(wts, d0 + s)
                self._predict_forward(bufs, wts, xc, rows, 0, d0 + s, row0 + c0, lrt, pack=(s == 0))
                a.first, a.final = int(s == 0), int(s == S - 1)
                L.check(lib.vbnn_head_predict(ctx, code, C.byref(a)))
        if not map:                            # the draws test() would have consumed
            self.draw += S
            if self.device_draw:
                L.check(lib.vbnn_sample(ctx, _p(self._draw_dev), S))
        if totals is not None:
            tot = [sum(col) for col in zip(*totals.cpu().tolist())]     # chunk order (synchronises)
            res.totals = tot
            res.nll, res.accuracy = tot[0] / R, 100.0 * tot[1] / R
            res.mean_draw_nll, res.mean_draw_accuracy = tot[2] / (R * S), 100.0 * tot[3] / (R * S)
        res.S, res.stacked, res.chunks = S, stacked, n_chunks
        return res

    def _predict_stacked(self, R, S, lrt):
        """opt.predict_stacked: True / False / "auto" (default). Weight noise draws a weight matrix per draw: sequential always.
        "auto": stacked while one draw's widest forward is small (R I O < 2^32 multiply-adds: the reference's operating points,
        launch-bound, where S launches become one), sequential above -- stacked rows never run on the two-pass 256 x 256 kernel
        (vbnn_fwd_args.rows_per_draw), which is what the large bf16 forwards take one draw at a time (tools/predict_bench.py)."""
        if not lrt or S == 1:
            return S == 1 or lrt
        ps = self.opt.get("predict_stacked", "auto")
        if ps != "auto":
            return bool(ps)
        rows = min(R, max(1, int(self.opt.get("predict_rows", 32768))))
        return rows * max(v.I * v.O for v in self.vb) < (1 << 32)

    def _predict_buffers(self, rows, lrt):
        """predict's operands: the packed input, then one ping-pong PAIR of activation (+ square) buffers per hidden width --
        layer li writes slot (O, li % 2), so a layer never overwrites its own input and a buffer always holds one layout (its
        pads stay zero). bufs[li] is layer li's input, bufs[len(vb)] the head's. Kept across calls while the row count holds."""
        sq = lrt and self.dtype == "bf16"                       # (fp32: the forward forms x.x from x itself)
        key = (rows, sq)
        if getattr(self, "_pred_key", None) != key:
            self._pred_bufs, self._pred_key = None, None
            dev, tdt, nl = self.device, self.tdt, len(self.vb)
            slots = {}

            def slot(cols, parity, square):
                b = slots.get((cols, parity))
                if b is None:
                    b = slots[(cols, parity)] = _VB()
                    b.x, b.x2 = _Packed(rows, cols, tdt, dev), None
                if square and b.x2 is None:
                    b.x2 = _Packed(rows, cols, tdt, dev)
                return b
            bufs = _PredictBuffers([slot(self.sizes[0], "in", sq)])
            for li, v in enumerate(self.vb):
                bufs.append(slot(v.O, li % 2, sq and li < nl - 1))
            bufs.r = _Packed(rows, max(v.O for v in self.vb), tdt, dev) if sq else None
            self._pred_bufs, self._pred_key = bufs, key
        return self._pred_bufs

    def _predict_weights(self):
        """WN: predict's own sampled weights (fp32) and their packed shadows, per layer (sample() keeps its draw in the training
        operands; predict leaves them alone)."""
        if getattr(self, "_pred_wts", None) is None:
            self._pred_wts = [(torch.zeros(v.O, v.I, dtype=torch.float32, device=self.device), _Packed(v.O, v.I, self.tdt, self.device))
                              for v in self.vb]
        return self._pred_wts

    def _predict_wn_sample(self, wts, draw):
        """VBLinear:sample (VBLinear.lua:49-64) for `draw` into predict's weights; draw None: the means (clamp_to_map)."""
        lib = L.lib()
        for v, (w, ws) in zip(self.vb, wts):
            if draw is not None:
                L.check(lib.vbnn_wn_sample(self.ctx.h, _p(v.means), None, _p(v.lvars), _p(w), None, v.O, v.I, self.seed, v.layer_id, draw))
            L.check(lib.vbnn_pack(self.ctx.h, self.code, L.PACK_COPY, _p(w if draw is not None else v.means), None, v.I, v.O, v.I,
                                  ws.ptr, ws.ld, None, 0))

    def _predict_forward(self, bufs, wts, x, N, rpd, draw, row0, lrt, pack=True):
        """vbnn_pack_input + every VB layer's forward for predict: N operand rows (rpd > 0: stacked draws of rpd rows each)."""
        if isinstance(self._pruned, SparsePruneResult):        # the compressed view: its own forward (below prune_curve)
            return self._predict_forward_sparse(bufs, x, N, rpd, draw, row0, lrt, pack)
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        if pack:
            b0 = bufs[0]
            L.check(lib.vbnn_pack_input(ctx, code, _p(x), x.stride(0), N, self.sizes[0], b0.x.ptr, b0.x2.ptr if b0.x2 else None,
                                        b0.x.ld, None, None, 0, rpd))
        nl = len(self.vb)
        pv = self._pruned                      # a pruned view: ITS shadows in place of mu_s / var_s (or of WN's packed means)
        for li, v in enumerate(self.vb):
            xin, out = bufs[li], bufs[li + 1]
            w = pv.mu_p[li] if pv is not None else (wts[li][1] if wts is not None else v.mu_s)
            w2 = pv.var_p[li] if pv is not None else v.var_s
            # r: nobody reads it. Only the sequential bf16 LRT forwards are handed a throwaway one -- the two-pass 256 x 256
            # kernel, which the large one-draw forwards take, stores r as part of its fold and is not selected without it.
            r = bufs.r if (lrt and rpd == 0 and bufs.r is not None) else None
            a = L.FwdArgs(w=w.ptr, w2=w2.ptr if lrt else None, x=xin.x.ptr, x2=xin.x2.ptr if (lrt and xin.x2) else None,
                          ld_w=w.ld, ld_x=xin.x.ld, N=N, I=v.I, O=v.O, bias=_p(v.bias), seed=self.seed, layer=v.layer_id,
                          draw=draw, draw_dev=None, row0=row0, y=None, ld_y=0, r=r.ptr if r else None, ld_r=r.ld if r else 0,
                          r_packed=1, relu=1,
                          h=out.x.ptr, h2=out.x2.ptr if (lrt and li < nl - 1 and out.x2) else None, ld_h=out.x.ld,
                          hT=None, h2T=None, ld_hT=0, rows_per_draw=rpd)
            L.check(lib.vbnn_forward(ctx, code, C.byref(a)))

    # ---- mlp.lua:69-74
    @_ordered
    def sample(self, by=1):
        self.draw += by
        self._map = False
        if self.device_draw:
            L.check(L.lib().vbnn_sample(self.ctx.h, _p(self._draw_dev), by))
        if self.mode == "wn":
            lib = L.lib()
            for v in self.vb:
                L.check(lib.vbnn_wn_sample(self.ctx.h, _p(v.means), None, _p(v.lvars), _p(v.weight), None, v.O, v.I,
                                           self.seed, v.layer_id, self.draw))
                L.check(lib.vbnn_pack(self.ctx.h, self.code, L.PACK_COPY, _p(v.weight), None, v.I, v.O, v.I,
                                      v.mu_s.ptr, v.mu_s.ld, v.muT_s.ptr if v.muT_s else None,
                                      v.muT_s.ld if v.muT_s else 0))

    # ---- the regression criterion's posterior predictive (vbnn_predict_moments): predict()'s contract and buffers, the final
    # Linear as _generic_head runs it (f32 outputs), then the moments of the S draws -- mean, spread, and with targets the
    # squared errors and the mixture's log-likelihood. Nothing of the training step is written.
    @_ordered
    def predict_regression(self, inputs, S=None, targets=None, noise_var=None, map=False, row0=None, keep_draws=False):
        """E[y | x, D] ~ 1/S sum_s f_s(x) over draws self.draw + 1 .. self.draw + S, with the draws' variance per output; S, map
        and row0 as predict(), and `self.draw` advances by S likewise. targets: R x D fp32. noise_var (tau^2 > 0, or None): the
        observation noise of the predictive log-likelihood. keep_draws: the S x R x D outputs are returned too. Returns a
        RegressionPredictResult of this rank's rows (no collective, as test()).
        criterion = "gauss": D = n_classes / 2, the network supplies the noise (noise_var must be None), the result carries the
        aleatoric noise_var beside the epistemic var, and keep_draws returns the S x R x 2 D outputs (means, log variances)."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        if self.criterion not in ("mse", "gauss"):
            raise ValueError("predict_regression: the regression predictive needs the MSE criterion or the Gaussian one "
                             "(criterion = 'nll': use predict)")
        gauss = self.criterion == "gauss"
        Wd = self.n_classes                                          # the final Linear's width: D, or { m[D], s[D] }
        D = Wd // 2 if gauss else Wd
        if gauss and noise_var is not None:
            raise ValueError("predict_regression: criterion = 'gauss' predicts its own noise variance (noise_var must be None)")
        if noise_var is not None:
            noise_var = float(noise_var)
            if not (noise_var > 0.0 and math.isfinite(noise_var)):
                raise ValueError(f"predict_regression: noise_var = {noise_var} (a finite variance above zero, or None)")
        map = bool(map or self.opt.get("quicktest"))
        S = 1 if map else int(self.opt["testSamples"] if S is None else S)
        if S < 1:
            raise ValueError(f"predict_regression: S = {S} draws (at least one)")
        x = inputs.reshape(inputs.shape[0], -1)
        R = x.shape[0]
        assert x.shape[1] == self.sizes[0] and x.dtype == torch.float32 and x.is_cuda and R > 0
        if targets is not None:
            if gauss and tuple(targets.shape) != (R, D):
                raise ValueError(f"predict_regression: targets of shape {tuple(targets.shape)} (criterion = 'gauss' takes R x D = "
                                 f"{R} x {D}: one target per mean)")
            assert targets.dtype == torch.float32 and targets.is_cuda and tuple(targets.shape) == (R, D)
            targets = targets.contiguous()
        row0 = self.rank * R if row0 is None else int(row0)
        if not self._shadows_ready:
            self.prepare()
        if self._pruned is not None:
            if self.mode == "wn" and not map:
                raise ValueError("predict_regression: weight-noise draws under a pruned view are not supported (use map=True, or "
                                 "mode = 'lrt')")
            if self._pruned.version != self._pver:
                raise RuntimeError("predict_regression: the pruned view was taken from older parameters (update / prepare / "
                                   "init_parameters ran since): prune() again, or use_pruned(None)")
        lrt = self.mode == "lrt" and not map
        stacked = self._predict_stacked(R, S, lrt)
        cap = max(1, int(self.opt.get("predict_rows", 32768)))
        Rc = max(1, min(R, cap // S if stacked else cap))
        op_rows = S * Rc if stacked else Rc
        bufs = self._predict_buffers(op_rows, lrt)
        wts = self._predict_weights() if self.mode == "wn" else None
        f32 = dict(dtype=torch.float32, device=self.device)
        n_chunks = (R + Rc - 1) // Rc
        has_t = targets is not None
        res = RegressionPredictResult(torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, **f32),
                                      torch.empty(R, **f32) if has_t else None,
                                      torch.empty(R, **f32) if (has_t and (gauss or noise_var is not None)) else None,
                                      torch.empty(S, R, Wd, **f32) if keep_draws else None)
        if gauss:
            res.noise_var, res.row_noise_var = torch.empty(R, D, **f32), torch.empty(R, **f32)
        direct = keep_draws and (not stacked or n_chunks == 1)      # the final Linear writes into res.draws itself
        ybuf = None
        if not direct:                                               # the y buffer: kept with the predict buffers
            ybuf = getattr(bufs, "y_reg", None)
            if ybuf is None or tuple(ybuf.shape) != (op_rows, Wd):
                ybuf = bufs.y_reg = torch.empty(op_rows, Wd, **f32)
        one_call = stacked and D <= (L.GAUSS_MOMENTS_STACKED_MAX_D if gauss else L.MOMENTS_STACKED_MAX_D)   # else: ACCUMULATE per draw
        state = None if one_call else torch.empty(Rc, (3 if gauss else 2) * D + 2, **f32)
        totals = torch.zeros(n_chunks, 5 if gauss else 4, dtype=torch.float64, device=self.device) if has_t else None
        d0 = self.draw + 1
        nl, H = len(self.vb), self.sizes[-1]
        form = L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE
        if gauss:
            a = L.GaussMomentsArgs(ld_y=Wd, ld_t=D, D=D, S=S, form=form, s_min=self.logvar_clamp[0], s_max=self.logvar_clamp[1],
                                   state=_p(state), ld_out=D)
            moments = lib.vbnn_predict_gauss_moments
        else:
            a = L.MomentsArgs(ld_y=D, ld_t=D, D=D, S=S, form=form, noise_var=noise_var or 0.0, state=_p(state), ld_out=D)
            moments = lib.vbnn_predict_moments

        def off(t, row):
            return C.c_void_p(t.data_ptr() + 4 * row) if t is not None else None

        def final_linear(N, y_ptr):
            fa = L.FwdArgs(w=self.w3_s.ptr, w2=None, x=bufs[nl].x.ptr, x2=None, ld_w=self.w3_s.ld, ld_x=bufs[nl].x.ld,
                           N=N, I=H, O=Wd, bias=_p(self.bias3), y=y_ptr, ld_y=Wd)
            L.check(lib.vbnn_forward(ctx, code, C.byref(fa)))

        for k in range(n_chunks):
            c0 = k * Rc
            rows = min(Rc, R - c0)
            xc = x[c0:c0 + rows]
            a.R = rows
            a.target = off(targets, c0 * D)
            a.totals = C.c_void_p(totals[k].data_ptr()) if has_t else None
            a.mean, a.var = off(res.mean, c0 * D), off(res.var, c0 * D)
            a.row_var, a.row_sq_err, a.row_log_lik = off(res.row_var, c0), off(res.row_sq_err, c0), off(res.row_log_lik, c0)
            if gauss:
                a.noise_var, a.row_noise_var = off(res.noise_var, c0 * D), off(res.row_noise_var, c0)
            if stacked:                        # every draw in one forward: draw s = rows [s rows, (s+1) rows) of y
                if wts is not None:
                    self._predict_wn_sample(wts, None if map else d0)
                self._predict_forward(bufs, wts, xc, S * rows, rows if S > 1 else 0, d0, row0 + c0, lrt)
                y = res.draws if direct else ybuf
                final_linear(S * rows, _p(y))
                if one_call:
                    a.y = _p(y)
                    L.check(moments(ctx, C.byref(a)))
                else:
                    for s in range(S):
                        a.y, a.draw = off(y, s * rows * Wd), s
                        L.check(moments(ctx, C.byref(a)))
                if keep_draws and not direct:
                    res.draws[:, c0:c0 + rows].copy_(ybuf[:S * rows].view(S, rows, Wd))
                continue
            for s in range(S):                 # one draw per forward, the running moments in `state` between the launches
                if wts is not None:
                    self._predict_wn_sample(wts, d0 + s)
                self._predict_forward(bufs, wts, xc, rows, 0, d0 + s, row0 + c0, lrt, pack=(s == 0))
                yp = off(res.draws, (s * R + c0) * Wd) if direct else _p(ybuf)
                final_linear(rows, yp)
                a.y, a.draw = yp, s
                L.check(moments(ctx, C.byref(a)))
        if not map:
            self.draw += S
            if self.device_draw:
                L.check(lib.vbnn_sample(ctx, _p(self._draw_dev), S))
        if has_t:
            tot = [sum(col) for col in zip(*totals.cpu().tolist())]     # chunk order (synchronises)
            res.totals = tot
            res.mse = tot[0] / (R * D)
            if gauss:
                res.mean_draw_nll, res.mean_noise_var = tot[1] / (R * S * D), tot[4] / (R * D)
            else:
                res.mean_draw_mse = tot[1] / (R * S * D)
            res.log_lik = tot[2] / R if (gauss or noise_var is not None) else None
            res.mean_var = tot[3] / (R * D)
        res.S, res.stacked, res.chunks = S, stacked, n_chunks
        return res

    # ---- final Linear + criterion through the generic GEMM kernels (class counts above 16)
    def _generic_head(self, N, targets, inv_n, accumulate, backward=True):
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        lrt = self._lrt()
        H, Cn = self.sizes[-1], self.n_classes
        a = L.FwdArgs(w=self.w3_s.ptr, w2=None, x=self.h_s.ptr, x2=None, ld_w=self.w3_s.ld, ld_x=self.h_s.ld,
                      N=N, I=H, O=Cn, bias=_p(self.bias3), y=_p(self.logits), ld_y=Cn)
        L.check(lib.vbnn_forward(ctx, code, C.byref(a)))
        if self.criterion == "mse":
            assert targets.dtype == torch.float32 and tuple(targets.shape) == (N, Cn) and targets.is_contiguous()
            L.check(lib.vbnn_mse_forward(ctx, _p(self.logits), Cn, _p(targets), Cn, N, Cn, inv_n / Cn, _p(self.g_logits), Cn,
                                         accumulate, _p(self._acc)))
            if not accumulate:
                L.check(lib.vbnn_buf_zero(ctx, _p(self._corr), 4))
        elif self.criterion == "gauss":
            D = Cn // 2
            assert targets.dtype == torch.float32 and tuple(targets.shape) == (N, D) and targets.is_contiguous()
            L.check(lib.vbnn_gauss_nll_forward(ctx, _p(self.logits), Cn, _p(targets), D, N, D, inv_n / D, self.logvar_clamp[0],
                                               self.logvar_clamp[1], _p(self.g_logits), Cn, accumulate, _p(self._acc)))
            if not accumulate:
                L.check(lib.vbnn_buf_zero(ctx, _p(self._corr), 4))
        else:
            if not accumulate:                          # vbnn_logsoftmax_nll adds into its accumulators
                L.check(lib.vbnn_buf_zero(ctx, _p(self._acc), 16))
                L.check(lib.vbnn_buf_zero(ctx, _p(self._corr), 4))
            L.check(lib.vbnn_logsoftmax_nll(ctx, _p(self.logits), Cn, _p(targets), N, Cn, inv_n, _p(self.out),
                                            _p(self.g_logits), _p(self._acc), _p(self._corr)))
        if not backward:
            return
        L.check(lib.vbnn_pack(ctx, code, L.PACK_COPY, _p(self.g_logits), None, Cn, N, Cn, self.g3_s.ptr, self.g3_s.ld,
                              self.g3T_s.ptr, self.g3T_s.ld))
        d = L.DwArgs(xT=self.hT_s.ptr, x2T=None, gT=self.g3T_s.ptr, gvT=None, ld_n=self.hT_s.ld, N=N, I=H, O=Cn,
                     scale=1.0, accumulate=accumulate, gradWeight=_p(self.gradWeight3), gradSum=None)
        L.check(lib.vbnn_acc_grad_parameters(ctx, code, C.byref(d)))
        L.check(lib.vbnn_acc_grad_bias(ctx, L.F32, _p(self.g_logits), Cn, N, Cn, 1.0, accumulate, _p(self.gradBias3)))
        vl = self.vb[-1]
        dx = L.DxArgs(wT=self.w3T_s.ptr, w2T=None, g=self.g3_s.ptr, gv=None, ld_wT=self.w3T_s.ld, ld_g=self.g3_s.ld,
                      N=N, I=H, O=Cn, x=self.h_s.ptr, ld_x=self.h_s.ld, gx=None, ld_gx=0, relu_mask=1,
                      r_prev=_p(vl.r) if lrt else None, ld_r_prev=vl.O, r_prev_packed=1, g_prev=vl.g_s.ptr,
                      gv_prev=vl.gv_s.ptr if lrt else None, ld_gp=vl.g_s.ld, gT_prev=vl.gT_s.ptr if vl.gT_s else None,
                      gvT_prev=vl.gvT_s.ptr if (lrt and vl.gvT_s) else None, ld_gpT=vl.gT_s.ld if vl.gT_s else 0)
        L.check(lib.vbnn_grad_input(ctx, code, C.byref(dx)))

    # ---- argument blocks of the three GEMM families for VB layer `li` (also used by bench.py to time
    # exactly the launches of the step in isolation)
    # The blocks are built once per (layer, batch shape, ...) and kept (the launch-bound step is ~50 us of GPU time: rebuilding
    # five ctypes structures per step cost the Python host ~20 us of it); what varies from call to call -- the draw counter, the
    # raw minibatch's address -- is patched in.
    def _fwd_args(self, li, N, row0):
        direct_x = li == 0 and self._x_in is not None
        key = ("fwd", li, N, row0, self._rpd, direct_x, self._lrt())     # (the block bakes in the LRT / MAP operand set)
        a = self._argcache.get(key)
        if a is None:
            a = self._argcache[key] = self._build_fwd_args(li, N, row0)
        if direct_x:
            a.x, a.ld_x = self._x_in.ptr, self._x_in.ld
        a.draw = 0 if self.device_draw else self.draw
        return a

    def _build_fwd_args(self, li, N, row0):
        v, lrt = self.vb[li], self._lrt()
        last = li == len(self.vb) - 1
        nxt = None if last else self.vb[li + 1]
        xin = self._x_in if (li == 0 and self._x_in is not None) else v.x_s       # the raw minibatch, read in place (fp32)
        sq = lrt and not self.f32_direct                                          # squares as operands (else formed by the kernel)
        return L.FwdArgs(w=v.mu_s.ptr, w2=v.var_s.ptr if lrt else None, x=xin.ptr, x2=v.x2_s.ptr if sq else None,
                         ld_w=v.mu_s.ld, ld_x=xin.ld, N=N, I=v.I, O=v.O, bias=_p(v.bias), seed=self.seed,
                         layer=v.layer_id, draw=0 if self.device_draw else self.draw,
                         draw_dev=_p(self._draw_dev) if self.device_draw else None, row0=row0, y=None, ld_y=0,
                         r=_p(v.r) if lrt else None, ld_r=v.O, r_packed=1, relu=1,
                         h=self.h_s.ptr if last else nxt.x_s.ptr,
                         h2=None if (last or not sq) else nxt.x2_s.ptr,
                         ld_h=self.h_s.ld if last else nxt.x_s.ld,
                         hT=(None if (self.n_classes <= 16 and self.criterion == "nll") else self.hT_s.ptr) if last else (nxt.xT_s.ptr if nxt.xT_s else None),
                         h2T=None if (last or not lrt or not nxt.x2T_s) else nxt.x2T_s.ptr,
                         ld_hT=self.hT_s.ld if last else (nxt.xT_s.ld if nxt.xT_s else 0), rows_per_draw=self._rpd,
                         **(dict(head_w3=self.w3_s.ptr, head_ld_w=self.w3_s.ld, head_C=self.n_classes, head_slots=_p(self.head_slots))
                            if (last and self._use_head_slots()) else {}))

    def _use_head_slots(self):
        return self.n_head_slots > 0 and not self._rpd

    def _dw_args(self, li, N, accumulate):
        direct_x = li == 0 and self._x_in is not None
        key = ("dw", li, N, accumulate, float(self._draws or self.S), direct_x, self._lrt())
        d = self._argcache.get(key)
        if d is None:
            d = self._argcache[key] = self._build_dw_args(li, N, accumulate)
        if direct_x:
            d.x, d.ld_x = self._x_in.ptr, self._x_in.ld
        d.draw, d.part = self.draw, 0
        return d

    def _build_dw_args(self, li, N, accumulate):
        v, lrt = self.vb[li], self._lrt()
        has_t = v.xT_s is not None
        has_gt = v.gT_s is not None
        xin = self._x_in if (li == 0 and self._x_in is not None) else v.x_s
        d = L.DwArgs(xT=v.xT_s.ptr if has_t else None, x2T=v.x2T_s.ptr if (lrt and has_t) else None,
                     gT=v.gT_s.ptr if has_gt else None, gvT=v.gvT_s.ptr if (lrt and has_gt) else None,
                     ld_n=v.gT_s.ld if has_gt else 0, N=N, I=v.I, O=v.O, scale=1.0,
                     accumulate=accumulate, seed=self.seed, layer=v.layer_id, draw=self.draw, lvars=_p(v.lvars),
                     x=xin.ptr, x2=v.x2_s.ptr if (lrt and v.x2_s is not None) else None, g=v.g_s.ptr, gv=v.gv_s.ptr if lrt else None,
                     ld_x=xin.ld, ld_g=v.g_s.ld)
        if self.fuse_kl:
            d.gradWeight, d.gradSum = None, None
            d.grad_mu, d.grad_lv = _p(v.gradWeight), _p(v.gradSum)
            d.means, d.stats = _p(v.means), _p(v.stats)
            d.B, d.S, d.kl_scale = self.B, float(self._draws or self.S), partition.scales(1, self.world)["kl_scale"]
            if self.kl_in_update:
                d.kl_scale = 0.0                      # likelihood parts only: update() adds the KL gradient from the fp32 parameters
            if self.kl_from_shadows and lrt:
                # the epilogue reads mu, sigma^2 from the bf16 operand shadows (4 B per weight instead of 8, no exp): the
                # values the forward GEMMs multiplied by
                d.mu_s, d.var_s, d.ld_w = v.mu_s.ptr, v.var_s.ptr, v.mu_s.ld
        else:
            d.gradWeight, d.gradSum = _p(v.gradWeight), _p(v.gradSum)
        d.gradBias = _p(v.gradBias) if v.bias_from_dw else None
        return d

    def _dx_args(self, li, N):
        key = ("dx", li, N, self._lrt())
        a = self._argcache.get(key)
        if a is None:
            a = self._argcache[key] = self._build_dx_args(li, N)
        return a

    def _build_dx_args(self, li, N):
        v, p, lrt = self.vb[li], self.vb[li - 1], self._lrt()
        use_t = v.use_muT
        return L.DxArgs(wT=v.muT_s.ptr if use_t else None, w2T=v.varT_s.ptr if (lrt and use_t) else None, g=v.g_s.ptr,
                        gv=v.gv_s.ptr if lrt else None, ld_wT=v.muT_s.ld, ld_g=v.g_s.ld, N=N, I=v.I, O=v.O,
                        x=v.x_s.ptr, ld_x=v.x_s.ld, gx=None, ld_gx=0, relu_mask=1,
                        r_prev=_p(p.r) if lrt else None, ld_r_prev=p.O, r_prev_packed=1, g_prev=p.g_s.ptr,
                        gv_prev=p.gv_s.ptr if lrt else None, ld_gp=p.g_s.ld,
                        gT_prev=p.gT_s.ptr if p.gT_s else None, gvT_prev=p.gvT_s.ptr if (lrt and p.gvT_s) else None,
                        ld_gpT=p.gT_s.ld if p.gT_s else 0,
                        w=v.mu_s.ptr, w2=v.var_s.ptr if lrt else None, ld_w=v.mu_s.ld)

    # ---- mlp.lua:76-84, fused
    @_ordered
    def run(self, inputs, targets, row0=None, backward=True, last_draw=None):
        """last_draw (data-parallel only): whether this run's gradients are the minibatch's final ones, i.e. whether the
        buckets' all-reduces are issued. Default: the opt.S-th sequential run since resetGradients() (always, inside
        run_draws). The draws of a minibatch ACCUMULATE in the arena (main.lua:32-37): exchanging after every draw would
        all-reduce sums that already contain other ranks' contributions, and the exchange stream's in-place write would
        race with the next draw's accumulate epilogue -- so earlier draws only accumulate."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        if backward:
            self._draws_run += 1
            if last_draw is None:
                last_draw = bool(self._rpd) or self._draws_run >= int(self.S)
            if self.reduce and not self._rpd and self._draws_run > int(self.S) and self._exchange_done:
                raise RuntimeError(f"run() called {self._draws_run} times since resetGradients() with opt.S = {int(self.S)}: the "
                                   "gradient buckets were already exchanged after draw S")
            self._exchange_now = bool(last_draw)
            self._exchange_done = self._exchange_now
        x = inputs.reshape(inputs.shape[0], -1)                         # nn.Reshape (mlp.lua:12)
        # stacked draws (run_draws): the operands have S x rows_per_draw rows, the input and the targets one minibatch's --
        # the packer and the head address row n % rows_per_draw (no S-fold copy of the input is ever made)
        N = x.shape[0] * (self._draws if self._rpd else 1)
        assert x.shape[1] == self.sizes[0] and x.dtype == torch.float32 and x.is_cuda
        assert not self._rpd or x.shape[0] == self._rpd
        self._alloc_batch(N)
        if row0 is None:
            row0 = self.rank * (self._rpd or N)
        lrt = self._lrt()
        accumulate = 0 if self._first else 1
        inv_n = partition.scales(self._rpd or N, self.world)["inv_n"]       # per DRAW: stacked draws sum their criteria
        v0 = self.vb[0]
        self._x_in = None
        if self.f32_direct and not self._rpd and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
            self._x_in = _View(x)                        # the GEMMs read the minibatch where it lies: no packing launch
        else:
            L.check(lib.vbnn_pack_input(ctx, code, _p(x), x.stride(0), N, v0.I, v0.x_s.ptr,
                                        v0.x2_s.ptr if (lrt and v0.x2_s is not None) else None,
                                        v0.x_s.ld, v0.xT_s.ptr if v0.xT_s else None,
                                        v0.x2T_s.ptr if (lrt and v0.x2T_s) else None, v0.xT_s.ld if v0.xT_s else 0, self._rpd))
        nl = len(self.vb)
        # ---------------- forward
        for li in range(nl):
            a = self._fwd_args(li, N, row0)
            with self._probed("forward", li):
                L.check(lib.vbnn_forward(ctx, code, C.byref(a)))
        H, Cn = self.sizes[-1], self.n_classes
        vl = self.vb[-1]
        fused_head = Cn <= 16 and self.criterion == "nll"
        if fused_head:
            # ---------------- fused classifier head (mlp.lua:29-32): streaming kernels, no 10-wide MFMA tiles
            if backward and self.head_step:
                # forward + backward of the head as ONE call (vbnn_head_forward_backward: one launch for fp32 at launch-bound
                # sizes -- the logits recomputed per workgroup instead of a second kernel waiting for g_logits --, the two
                # launches below everywhere else)
                key = ("head", N, self._rpd, accumulate, lrt)
                a = self._argcache.get(key)
                if a is None:
                    a = self._argcache[key] = L.HeadArgs()
                    a.h, a.ld_h, a.w3, a.ld_w, a.bias = self.h_s.ptr, self.h_s.ld, self.w3_s.ptr, self.w3_s.ld, _p(self.bias3)
                    a.N, a.H, a.C, a.rows_per_draw, a.inv_n, a.accumulate = N, H, Cn, self._rpd, inv_n, accumulate
                    a.logits, a.out, a.g_logits = _p(self.logits), _p(self.out), _p(self.g_logits)
                    a.loss_sum_dev, a.correct_dev = _p(self._acc), _p(self._corr)
                    a.gradWeight, a.gradBias, a.gradBias_prev = _p(self.gradWeight3), _p(self.gradBias3), _p(vl.gradBias)
                    a.relu_mask, a.r_prev_packed, a.r_prev, a.ld_r_prev = 1, 1, (_p(vl.r) if lrt else None), vl.O
                    a.g_prev, a.gv_prev, a.ld_gp = vl.g_s.ptr, (vl.gv_s.ptr if lrt else None), vl.g_s.ld
                    a.gT_prev = vl.gT_s.ptr if vl.gT_s else None
                    a.gvT_prev = vl.gvT_s.ptr if (lrt and vl.gvT_s) else None
                    a.ld_gpT = vl.gT_s.ld if vl.gT_s else 0
                    if self._use_head_slots():            # the logits' partial sums are in the slots the forward just wrote
                        a.logit_slots, a.n_slots = _p(self.head_slots), self.n_head_slots
                a.target = _p(targets)
                L.check(lib.vbnn_head_forward_backward(ctx, code, C.byref(a)))
            else:
                if self._use_head_slots():
                    L.check(lib.vbnn_head_forward_slots(ctx, _p(self.head_slots), self.n_head_slots, _p(self.bias3), _p(targets), N, Cn,
                                                        inv_n, _p(self.logits), _p(self.out), _p(self.g_logits), accumulate,
                                                        _p(self._acc), _p(self._corr), self._rpd))
                else:
                    L.check(lib.vbnn_head_forward(ctx, code, self.h_s.ptr, self.h_s.ld, self.w3_s.ptr, self.w3_s.ld,
                                                  _p(self.bias3), _p(targets), N, H, Cn, inv_n, _p(self.logits), _p(self.out),
                                                  _p(self.g_logits), accumulate, _p(self._acc), _p(self._corr), self._rpd))
                if not backward:
                    self._first = False
                    return
                L.check(lib.vbnn_head_backward(ctx, code, self.h_s.ptr, self.h_s.ld, self.w3_s.ptr, self.w3_s.ld,
                                               _p(self.g_logits), N, H, Cn, accumulate, _p(self.gradWeight3),
                                               _p(self.gradBias3), _p(vl.gradBias), 1, _p(vl.r) if lrt else None, vl.O, 1,
                                               vl.g_s.ptr,
                                               vl.gv_s.ptr if lrt else None, vl.g_s.ld, vl.gT_s.ptr if vl.gT_s else None,
                                               vl.gvT_s.ptr if (lrt and vl.gvT_s) else None, vl.gT_s.ld if vl.gT_s else 0))
        else:
            if self._rpd:                                 # (the generic criteria take one target per operand row)
                targets = targets.repeat(self._draws) if targets.dim() == 1 else targets.repeat(self._draws, 1)
            self._generic_head(N, targets, inv_n, accumulate, backward)
            if not backward:
                self._first = False
                return
        # ---------------- backward: VB layers, last to first. accGradParameters (+ bias gradient + the bucket's
        # all-reduce) of layer li and updateGradInput of layer li are independent of each other (both consume
        # g_li): with `overlap` they run on two HIP streams, so the HBM-bound epilogue of one GEMM sits beside the
        # MFMA main loop of the other instead of every CU hitting its epilogue at the same moment.
        if self.f32_direct and not self.overlap:
            # fp32, launch-bound sizes: accGradParameters and updateGradInput of a layer are independent (both consume g_li) and
            # go out as ONE launch where the library can carry both (vbnn_backward_pair: the general kernel's K-major forms at
            # its 32 x 32 geometry; elsewhere the call is the two launches) -- each tile bitwise what its own launch computes
            for li in range(nl - 1, -1, -1):
                v = self.vb[li]
                d = self._dw_args(li, N, accumulate)
                with self._probed("accGradParameters", li):
                    if li > 0:
                        L.check(lib.vbnn_backward_pair(ctx, code, C.byref(self._dx_args(li, N)), C.byref(d)))
                    else:
                        L.check(lib.vbnn_acc_grad_parameters(ctx, code, C.byref(d)))
                if not (fused_head and li == nl - 1) and not v.bias_from_dw:
                    L.check(lib.vbnn_acc_grad_bias(ctx, code, v.g_s.ptr, v.g_s.ld, N, v.O, 1.0, accumulate, _p(v.gradBias)))
        elif self.dx_first and not self.reduce and not self.overlap:
            # every updateGradInput first, then the accGradParameters from the first layer up: in the wide net the two 4096^3
            # launches are then separated by the lighter 784-wide gradient. The chip is power-bound in these launches
            # (LAB_NOTES.md section 3, r02): alternating heavy and light ones lets it hold a higher clock -- measured -25 / -7 / +3 us on a
            # slow / middle / fast box of the pool; gradients are the same launches on the same operands, bit for bit.
            # Not with an exchange (the widest layer's buckets must leave first) and not for stacks of equal layers (no
            # lighter launch to put between: +0.5 % on the deep stack).
            for li in range(nl - 1, 0, -1):
                with self._probed("updateGradInput", li):
                    L.check(lib.vbnn_grad_input(ctx, code, C.byref(self._dx_args(li, N))))
            for li in range(nl):
                v = self.vb[li]
                d = self._dw_args(li, N, accumulate)
                with self._probed("accGradParameters", li):
                    L.check(lib.vbnn_acc_grad_parameters(ctx, code, C.byref(d)))
                if not (fused_head and li == nl - 1) and not v.bias_from_dw:
                    L.check(lib.vbnn_acc_grad_bias(ctx, code, v.g_s.ptr, v.g_s.ld, N, v.O, 1.0, accumulate, _p(v.gradBias)))
        elif not self.overlap:
            for li in range(nl - 1, -1, -1):
                v = self.vb[li]
                d = self._dw_args(li, N, accumulate)
                with self._probed("accGradParameters", li):
                    if self._early(v, lrt):
                        # two launches (vbnn_dw_args.part): the sigma^2 GEMM and d/dlvars first -- its exchange starts while the
                        # mu GEMM still runs
                        d.part = 2
                        with self._probed_part("accGradParameters.lv", li):
                            L.check(lib.vbnn_acc_grad_parameters(ctx, code, C.byref(d)))
                        if self.sharded:
                            self._scatter(li, ("lv",))
                        else:
                            self._reduce(v.msg_early)
                        d.part = 1
                    with self._probed_part("accGradParameters.mu", li):
                        L.check(lib.vbnn_acc_grad_parameters(ctx, code, C.byref(d)))
                # the fused head already summed the last layer's g columns; ones-row layers got theirs from the GEMM
                if not (fused_head and li == nl - 1) and not v.bias_from_dw:
                    L.check(lib.vbnn_acc_grad_bias(ctx, code, v.g_s.ptr, v.g_s.ld, N, v.O, 1.0, accumulate, _p(v.gradBias)))
                if self.sharded:
                    self._scatter(li, ("mu", "small") if self._early(v, lrt) else ("lv", "mu", "small"))
                else:
                    self._reduce(v.msg_late if self._early(v, lrt) else (self.bucket_tail if li == nl - 1 else v.bucket))
                if li > 0:
                    dx = self._dx_args(li, N)
                    with self._probed("updateGradInput", li):
                        L.check(lib.vbnn_grad_input(ctx, code, C.byref(dx)))
        else:
            main, side, ctx2 = torch.cuda.current_stream(self.device), self._side, self.ctx2.h
            for li in range(nl - 1, -1, -1):
                v = self.vb[li]
                ready = torch.cuda.Event()
                ready.record(main)                           # g_li is complete on the main stream
                side.wait_event(ready)
                d = self._dw_args(li, N, accumulate)
                L.check(lib.vbnn_acc_grad_parameters(ctx2, code, C.byref(d)))
                if not (fused_head and li == nl - 1) and not v.bias_from_dw:
                    L.check(lib.vbnn_acc_grad_bias(ctx2, code, v.g_s.ptr, v.g_s.ld, N, v.O, 1.0, accumulate, _p(v.gradBias)))
                if self.reduce:                              # the exchange orders itself behind the MAIN stream: bring the
                    filled = torch.cuda.Event()              # side stream's accGradParameters in front of it first
                    filled.record(side)
                    main.wait_event(filled)
                    self._reduce(self.bucket_tail if li == nl - 1 else v.bucket)
                if li > 0:
                    dx = self._dx_args(li, N)
                    L.check(lib.vbnn_grad_input(ctx, code, C.byref(dx)))
            done = torch.cuda.Event()
            done.record(side)
            main.wait_event(done)                            # the next launch on the main stream sees every gradient
        self._first = False

    # ---- main.lua:32-37's S draws as ONE pass: the minibatch stacked S times as rows (draw s = rows [s N, (s + 1) N)), each
    # row's noise addressed by (its draw, its minibatch row) -- vbnn_fwd_args.rows_per_draw -- so every draw sees bit for bit
    # the z of its own sequential launch; the backward GEMMs sum over all draws at once (K = S N), the criterion over all
    # stacked rows with the per-draw 1 / N. One launch per GEMM family instead of S; the gradients equal the S sequential
    # draws' up to fp32 summation order. LRT only (weight noise draws a different weight matrix per draw). The gain is for the
    # reference's own operating point -- a handful of rows, S = 30 (config.lua:11,32) -- which is launch-bound.
    def run_draws(self, inputs, targets, S):
        assert self.mode == "lrt" and not self._map and self._first, "run_draws: LRT, right after resetGradients()"
        x = inputs.reshape(inputs.shape[0], -1)
        N = x.shape[0]
        self.sample()                                    # the first draw's counter; row n uses draw + n // N
        self._rpd, self._draws = N, S
        try:
            self.run(x, targets)
        finally:
            self._rpd, self._draws = 0, None
        if S > 1:
            self.sample(S - 1)

    # ---- one step as ONE graph launch (include/vbnn_hip.h: vbnn_capture_*). `issue` is a callable that issues the step's
    # calls on this engine (resetGradients / sample / run or run_draws / finish) exactly as it would to run them; between
    # begin and end they are recorded instead. Needs opt.device_draw (the noise counter must not be a launch argument), a
    # stream of the engine's own (FusedMLP(..., stream=...): the NULL stream cannot be captured) and one un-captured call
    # of `issue` before (allocations and first-launch configuration cannot be recorded). The inputs are read from the
    # same device buffers at every replay: copy the next minibatch into them.
    def capture_step(self, issue):
        assert self.device_draw, "capture_step needs opt.device_draw = True"
        assert self.ctx.torch_stream is not None, "capture_step needs an engine stream: FusedMLP(opt, stream=torch.cuda.Stream())"
        assert not self.reduce, "capture_step: single-GPU steps (the exchange runs on the communicator's own stream)"
        lib = L.lib()
        draws0 = self.draw
        with torch.cuda.stream(self.ctx.torch_stream):
            L.check(lib.vbnn_capture_begin(self.ctx.h))
            h = C.c_void_p()
            try:
                issue()
            finally:
                st = lib.vbnn_capture_end(self.ctx.h, C.byref(h))
            L.check(st)
        draws = self.draw - draws0
        self.draw = draws0                               # nothing ran: the recorded vbnn_sample nodes advance the counter at replay
        return _StepGraph(self, h, draws)

    # ---- data-parallel exchange: sum all-reduce of one layer's gradient bucket over RCCL/xGMI, issued
    # right after that layer's accGradParameters so it overlaps the rest of backward. The criterion
    # already divides by the GLOBAL batch and the KL gradient carries 1/world, so the sum is the result.
    # opt.exchange_dtype = "bf16" (default "f32"): the bucket is rounded to bf16 into a half-size staging arena, THAT is
    # all-reduced (80 instead of 160 MB per step of the wide configuration), and finish() widens the sums
    # back into the fp32 arena. A different gradient (every rank's contribution rounded, RCCL sums in bf16): an option for
    # hosts whose step is exchange-bound, never the default, and the bench line says which one ran.
    skip_exchange = False      # bench.py: the step with its collective calls left out (what the exchange costs beyond the overlap)

    def _reduce(self, bucket):
        if not self.reduce or not self._exchange_now or self.skip_exchange:
            return
        if self.exchange_dtype != "bf16":
            self.exchange().allreduce(bucket)
            return
        if self._stage is None:
            self._stage = torch.zeros(self.grads.numel(), dtype=torch.bfloat16, device=self.device)
        off = bucket.storage_offset() - self.grads.storage_offset()
        stage = self._stage[off:off + bucket.numel()]
        L.check(L.lib().vbnn_cast_grads(self.ctx.h, 1, _p(bucket), _p(stage), bucket.numel()))
        self.exchange().allreduce(stage)
        self._staged.append((bucket, stage))

    def _scatter(self, li, what):
        """Sharded mode: layer li's messages (partition.sharded_plan): reduce-scatter of d/dlvars, of d/dmeans; the small all-reduce."""
        if not self._exchange_now or self.skip_exchange:
            return
        p, ex, W = self._plan[li], self.exchange(), self.world
        for key in what:
            if key == "small":
                s0, e0 = p["small"]
                ex.allreduce(self.grads[s0:e0])
            else:
                off, per = p[key]
                ex.reduce_scatter(self.grads[off:off + per * W], per)

    def gather_parameters(self):
        """Sharded mode: bring every rank's fp32 means / lvars rows to every rank (checkpoints, calc_lc, tests). A COLLECTIVE --
        every rank calls it at the same point of its program -- and never a hidden part of another call: prepare() / test() do
        not need it (the sharded update leaves the gathered shadows and combined statistics they would produce), calc_lc() and
        anything else that reads other ranks' fp32 rows RAISES while they are stale instead of gathering on one rank and
        deadlocking the others. On the device wherever a device transport exists: the RCCL exchange's own in-place
        all-gather (rank r's rows are its contribution), else the out-of-band group -- nccl: all_gather_into_tensor on the
        device; gloo (rehearsals, CPU tests): through the host."""
        if not self.sharded or self.world == 1:
            self._params_stale = False
            return
        import torch.distributed as dist
        from .comm import RcclExchange
        ex = self.exchange()
        self.finish()
        on_exchange = isinstance(ex, RcclExchange)
        backend = dist.get_backend(self.pg)
        if not on_exchange:
            torch.cuda.synchronize(self.device)
        for v in self.vb:
            r0, nr = partition.layer_row_shard(v.O, self.world, self.rank)
            for t in (v.means, v.lvars):
                assert t.is_contiguous()
                if on_exchange:
                    ex.all_gather(t)
                elif backend == "nccl":
                    mine = t[r0:r0 + nr].clone()
                    dist.all_gather_into_tensor(t.view(-1), mine.view(-1), group=self.pg)
                else:
                    mine = t[r0:r0 + nr].cpu()
                    pieces = [torch.empty_like(mine) for _ in range(self.world)]
                    dist.all_gather(pieces, mine, group=self.pg)
                    for r, pc in enumerate(pieces):
                        if r != self.rank:
                            t[r * nr:(r + 1) * nr].copy_(pc)
        if on_exchange:
            ex.finish()
        self._params_stale = False

    def _need_gathered_parameters(self, what):
        if self._params_stale:
            raise RuntimeError(f"{what}: the fp32 means / lvars of other ranks' rows are stale after a sharded update -- call "
                               "gather_parameters() on EVERY rank first (a collective; it is never issued implicitly)")

    def _update_sharded(self, opt):
        """mlp:update / VBLinear:update with the parameters SHARDED by layer rows: the reduce-scatter left this rank the summed
        likelihood gradients of its rows; vbnn_update runs on those rows alone (+ the exact KL gradient, kl_add), then the new
        operand shadows and the slices' prior statistics are all-gathered and every rank forms the layers' statistics from the
        same gathered parts (vbnn_stats_combine). Biases and the final Linear: all-reduced gradients, replicated SGD."""
        lib, h, W, R = L.lib(), self.ctx.h, self.world, self.rank
        self._pver += 1
        ex = self.exchange()
        lr = float(opt["state"]["learningRate"])
        st = self.__dict__.setdefault("_opt_state", {})
        L.check(lib.vbnn_sgd_step(h, _p(self.weight3), _p(self.gradWeight3), self.weight3.numel(), lr))
        L.check(lib.vbnn_sgd_step(h, _p(self.bias3), _p(self.gradBias3), self.bias3.numel(), lr))
        n = len(self.vb)
        descs = (L.UpdateDesc * n)()
        mine = self._stat_parts[R]
        for k, v in enumerate(self.vb):
            L.check(lib.vbnn_sgd_step(h, _p(v.bias), _p(v.gradBias), v.O, lr))
            r0, nr = partition.layer_row_shard(v.O, W, R)
            mine[k].copy_(v.stats)                           # in: the WHOLE layer's pre-update statistics (var_hat of the KL terms)
            cfgs = []
            for key, cfg in (("mean", opt["meanState"]), ("var", opt["varState"])):
                s = st.setdefault((v.layer_id, key), {"t": 0})
                if "m" not in s:
                    s["m"] = torch.zeros(nr, v.I, dtype=torch.float32, device=self.device)
                    s["v"] = torch.zeros(nr, v.I, dtype=torch.float32, device=self.device)
                s["t"] += 1
                cfgs.append((s, L.AdamCfg(lr=float(cfg["learningRate"]), beta1=float(cfg.get("beta1", 0.9)),
                                          beta2=float(cfg.get("beta2", 0.999)), eps=float(cfg.get("epsilon", 1e-8)),
                                          lambda_=float(cfg.get("lambda", 1.0)), t=s["t"])))
            (sm, cm), (sv, cv) = cfgs
            descs[k] = L.UpdateDesc(means=_p(v.means[r0:r0 + nr]), lvars=_p(v.lvars[r0:r0 + nr]), O=nr, I=v.I,
                                    mu_s=_p(v.mu_s.t[r0:r0 + nr]), var_s=_p(v.var_s.t[r0:r0 + nr]), ld_w=v.mu_s.ld,
                                    muT_s=None, varT_s=None, ld_wT=0, stats=_p(mine[k]), grad_mu=_p(v.gradWeight[r0:r0 + nr]),
                                    grad_lv=_p(v.gradSum[r0:r0 + nr]), m_mu=_p(sm["m"]), v_mu=_p(sm["v"]), m_lv=_p(sv["m"]),
                                    v_lv=_p(sv["v"]), mu=cm, lv=cv, bias=None, grad_bias=None, lr_bias=lr, B=self.B,
                                    log14=None, kl_add=1.0)
        w3 = L.PackDesc(src=_p(self.weight3), rows=self.n_classes, cols=self.sizes[-1], ld_src=self.sizes[-1],
                        dst=self.w3_s.ptr, ld_dst=self.w3_s.ld, dstT=self.w3T_s.ptr, ld_dstT=self.w3T_s.ld)
        L.check(lib.vbnn_update(h, self.code, n, descs, C.byref(w3)))
        # what the next forward reads, from every rank: the shadows (in place: rank r's rows are its contribution), the parts
        for v in self.vb:
            ex.all_gather(v.mu_s.t)
            ex.all_gather(v.var_s.t)
        ex.all_gather(self._stat_parts)
        ex.finish()
        ptrs = (C.c_void_p * n)(*[v.stats.data_ptr() for v in self.vb])
        L.check(lib.vbnn_stats_combine(h, n, W, _p(self._stat_parts), ptrs))
        for v in self.vb:
            if v.muT_s is not None and getattr(v, "use_muT", True):       # transposed shadows: rebuilt locally from the gathered ones
                L.check(lib.vbnn_transpose_packed(h, self.code, v.mu_s.ptr, v.mu_s.ld, v.O, v.I, v.muT_s.ptr, v.muT_s.ld))
                L.check(lib.vbnn_transpose_packed(h, self.code, v.var_s.ptr, v.var_s.ld, v.O, v.I, v.varT_s.ptr, v.varT_s.ld))
        self._params_stale = W > 1
        self._shadows_ready = True

    def exchange(self):
        if self._exchange is None:
            from .comm import make_exchange
            self._exchange = make_exchange(self.ctx, self.rank, self.world, self.pg)
        return self._exchange

    def comm_backend(self):
        return self.exchange().backend if self.reduce else "none"

    @_ordered
    def finish(self):
        """Order the compute stream behind the outstanding all-reduces (end of the step)."""
        if self._exchange is not None:
            self._exchange.finish()
        for bucket, stage in self._staged:            # (bf16 exchange) the sums, widened back behind the exchange
            L.check(L.lib().vbnn_cast_grads(self.ctx.h, 0, _p(stage), _p(bucket), bucket.numel()))
        self._staged = []

    def check_exchange(self):
        """Raise if the exchange cannot vouch for the sums in the arena (the p2p exchange: a barrier that gave up -- ADVICE r03).
        Blocks on the exchange stream; update() and loss_and_accuracy() call it, a loop that does neither (a benchmark, a
        custom host) calls it before it believes a gradient or a timing."""
        if self._exchange is not None and hasattr(self._exchange, "check"):
            self._exchange.check()

    def _early(self, v, lrt=True):
        return v.msg_early is not None and lrt and self.fuse_kl and getattr(v, "early_ok", True)

    def buckets(self):
        """The all-reduce messages of one step, in issue order (last VB layer + final Linear first)."""
        out, nl = [], len(self.vb)
        for li in range(nl - 1, -1, -1):
            v = self.vb[li]
            if self._early(v):
                out += [v.msg_early, v.msg_late]
            else:
                out.append(self.bucket_tail if li == nl - 1 else v.bucket)
        return out

    @_ordered
    def time_buckets(self, reps=5):
        """Each bucket's all-reduce alone on an otherwise idle GPU: milliseconds (host clock around reps exchanges,
        device-synchronised), algorithm GB/s and bus GB/s (x 2 (world - 1) / world). Collective: every rank calls it."""
        import time
        out = []
        for b in self.buckets():
            if self.exchange_kind == "p2p":
                scratch = b                                # the p2p exchange sums regions of ITS arena: time it on the bucket itself
            else:
                scratch = torch.zeros_like(b) if self.exchange_dtype == "f32" else torch.zeros(b.numel(), dtype=torch.bfloat16, device=b.device)
            for _ in range(2):
                self.exchange().allreduce(scratch); self.finish()
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for _ in range(reps):
                self.exchange().allreduce(scratch)
            self.finish()
            torch.cuda.synchronize(self.device)
            ms = (time.perf_counter() - t0) / reps * 1e3
            nbytes = b.numel() * scratch.element_size()
            alg = nbytes / (ms * 1e-3) / 1e9
            out.append({"bytes": nbytes, "ms": round(ms, 4), "alg_GBps": round(alg, 1),
                        "bus_GBps": round(alg * 2 * (self.world - 1) / max(self.world, 1), 1)})
        return out

    def synthetic_targets(self, x, row0=0):
        """bench / tests: class targets uniform in 0..n_classes-1 by GLOBAL row (data.lua:16 convention, 0-based); for the
        regression criteria y* = x R / sqrt(I) with a fixed Philox-drawn R (D columns: n_classes
        for "mse", n_classes / 2 for "gauss") -- data preparation outside the timed step, so a plain torch matmul."""
        N = x.shape[0]
        if self.criterion in ("mse", "gauss"):
            D = self.n_classes if self.criterion == "mse" else self.n_classes // 2
            R = torch.empty(x.shape[1], D, dtype=torch.float32, device=x.device)
            fill_normal(R, self.seed, L.STREAM_DATA, 1, 0)
            return (x @ R / math.sqrt(x.shape[1])).contiguous()
        return ((torch.arange(N, device=x.device, dtype=torch.int64) + row0) * 2654435761 % self.n_classes).to(torch.int32)

    # ---- mlp:update + VBLinear:update (mlp.lua:117-142, VBLinear.lua:124-166) on the device: the dW epilogue
    # already produced the TOTAL gradients (likelihood / S + KL), so the update is ONE sweep per layer (vbnn_update):
    # SGD on the bias, Adam on means and lvars, and -- from the new parameters, in the same pass -- the GEMM shadows
    # and prior statistics of the next minibatch (the reference's update calls compute_prior too, :130). Nothing is
    # downloaded. Needs fuse_kl (otherwise use vbnn_amd/mlp.py's module-level update). `log` = True also produces the
    # 14 series of VBLinear.lua:149-164 per layer (self.update_log, a device tensor [layers][14]).
    @_ordered
    def update(self, opt=None, log=False):
        if not self.fuse_kl:
            raise RuntimeError("FusedMLP.update needs opt.fuse_kl = True (total gradients from the dW epilogue)")
        opt = opt or self.opt
        self.finish()
        self.check_exchange()                  # BEFORE a parameter is touched: an incomplete exchange must not reach them
        if self.sharded:
            assert not log, "the 14 logged series need whole-layer norms: not with the sharded update"
            return self._update_sharded(opt)
        lib, h = L.lib(), self.ctx.h
        self._pver += 1
        lr = float(opt["state"]["learningRate"])
        st = self.__dict__.setdefault("_opt_state", {})
        if log and getattr(self, "update_log", None) is None:
            self.update_log = torch.zeros(len(self.vb), 14, dtype=torch.float64, device=self.device)
        L.check(lib.vbnn_sgd_step(h, _p(self.weight3), _p(self.gradWeight3), self.weight3.numel(), lr))
        L.check(lib.vbnn_sgd_step(h, _p(self.bias3), _p(self.gradBias3), self.bias3.numel(), lr))
        if self.mode != "lrt":
            # weight-noise mode keeps no parameter shadows between minibatches (sample() packs the drawn weights):
            # per-tensor Adam, then the statistics
            for v in self.vb:
                L.check(lib.vbnn_sgd_step(h, _p(v.bias), _p(v.gradBias), v.O, lr))
                for key, x, g, cfg in (("mean", v.means, v.gradWeight, opt["meanState"]), ("var", v.lvars, v.gradSum, opt["varState"])):
                    s = st.setdefault((v.layer_id, key), {"t": 0})
                    if "m" not in s:
                        s["m"], s["v"] = torch.zeros_like(x), torch.zeros_like(x)
                    s["t"] += 1
                    L.check(lib.vbnn_adam_step(h, _p(x), _p(g), None, _p(s["m"]), _p(s["v"]), x.numel(),
                                               float(cfg["learningRate"]), float(cfg.get("beta1", 0.9)),
                                               float(cfg.get("beta2", 0.999)), float(cfg.get("epsilon", 1e-8)),
                                               float(cfg.get("lambda", 1.0)), s["t"], None))
            self.prepare()
            return
        descs = (L.UpdateDesc * len(self.vb))()
        for k, v in enumerate(self.vb):
            cfgs = []
            for key, x, cfg in (("mean", v.means, opt["meanState"]), ("var", v.lvars, opt["varState"])):
                s = st.setdefault((v.layer_id, key), {"t": 0})
                if "m" not in s:
                    s["m"], s["v"] = torch.zeros_like(x), torch.zeros_like(x)
                s["t"] += 1
                cfgs.append((s, L.AdamCfg(lr=float(cfg["learningRate"]), beta1=float(cfg.get("beta1", 0.9)),
                                          beta2=float(cfg.get("beta2", 0.999)), eps=float(cfg.get("epsilon", 1e-8)),
                                          lambda_=float(cfg.get("lambda", 1.0)), t=s["t"])))
            (sm, cm), (sv, cv) = cfgs
            use_t = v.muT_s is not None and getattr(v, "use_muT", True)
            descs[k] = L.UpdateDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, mu_s=v.mu_s.ptr, var_s=v.var_s.ptr,
                                    ld_w=v.mu_s.ld, muT_s=v.muT_s.ptr if use_t else None, varT_s=v.varT_s.ptr if use_t else None,
                                    ld_wT=v.muT_s.ld if v.muT_s else 0, stats=_p(v.stats), grad_mu=_p(v.gradWeight),
                                    grad_lv=_p(v.gradSum), m_mu=_p(sm["m"]), v_mu=_p(sm["v"]), m_lv=_p(sv["m"]), v_lv=_p(sv["v"]),
                                    mu=cm, lv=cv, bias=_p(v.bias), grad_bias=_p(v.gradBias), lr_bias=lr, B=self.B,
                                    log14=C.c_void_p(self.update_log[k].data_ptr()) if log else None,
                                    kl_add=1.0 if self.kl_in_update else 0.0)
        w3 = L.PackDesc(src=_p(self.weight3), rows=self.n_classes, cols=self.sizes[-1], ld_src=self.sizes[-1],
                        dst=self.w3_s.ptr, ld_dst=self.w3_s.ld, dstT=self.w3T_s.ptr, ld_dstT=self.w3T_s.ld)
        if self._held is not None:                            # a held pruning mask: the frozen weights keep every bit
            L.check(lib.vbnn_update_masked(h, self.code, len(self.vb), descs, self._held_ptrs(), C.byref(w3)))
        else:
            L.check(lib.vbnn_update(h, self.code, len(self.vb), descs, C.byref(w3)))
        self._shadows_ready = True

    # ---- reporting (each of these synchronises)
    def loss_and_accuracy(self):
        self.finish()
        torch.cuda.synchronize(self.device)
        self.check_exchange()
        loss = float(self._acc[0].item())
        correct = int(self._corr[0].item())
        return loss, correct

    @_ordered
    def calc_lc(self, opt=None):                                         # mlp.lua:109-115, fresh statistics
        self._need_gathered_parameters("calc_lc")
        lc = 0.0
        B = float((opt or self.opt).get("B", self.B))
        for li, v in enumerate(self.vb):
            if self._held is not None:                        # the KL of the network that exists: the kept weights' sum
                L.check(L.lib().vbnn_calc_lc_masked(self.ctx.h, _p(v.means), _p(v.lvars), _p(self._held[li]), _p(v.stats), B, None,
                                                    _p(self._lc), v.O * v.I))
            else:
                L.check(L.lib().vbnn_calc_lc(self.ctx.h, _p(v.means), _p(v.lvars), None, None, _p(v.stats), B, None,
                                             _p(self._lc), v.O * v.I))
            lc += float(self._lc[0].item())
        return lc

    # ---- fine-tuning a pruned network: a pruning mask HELD through training. The GEMMs of a step read the operand shadows only,
    # so the whole feature is the parameter sweep: while a mask is held prepare() / update() / calc_lc() go through
    # vbnn_prepare_masked / vbnn_update_masked / vbnn_calc_lc_masked -- +0 in a pruned weight's shadow entries, its fp32 parameters
    # and Adam moments frozen bit for bit, the prior statistics those of the kept weights. run / test / predict are unchanged.
    def _held_ptrs(self):
        return (C.c_void_p * len(self.vb))(*[m.data_ptr() for m in self._held])

    def _refuse_held(self, what):
        if self._held is not None:
            raise RuntimeError(f"{what}: a pruning mask is held, and {what} keys on the fp32 parameters, which still hold the frozen "
                               "weights' values -- release_pruned() first")

    @property
    def held(self):
        """Per VB layer the number of weights the held mask freezes, or None when nothing is held."""
        return None if self._held is None else list(self._held_counts)

    def held_mask(self, li):
        """The held mask of VB layer li as an O x I bool tensor (True = pruned and frozen)."""
        if self._held is None:
            raise RuntimeError("held_mask: no pruning mask is held")
        return self._held[li].bool()

    @_ordered
    def hold_pruned(self, result):
        """Train the network `result` leaves: from now on the weights it prunes are out of the network AND frozen. `result`: a
        PruneResult or SparsePruneResult of this engine at the current parameter version. Its byte masks (the vbnn_prune_pack
        route of PruneResult.mask) are ORed into whatever is already held -- the held set only grows, which is what an iterative
        schedule needs -- the shadows and statistics are rewritten by the masked prepare (a parameter-version change: `result`
        and any other snapshot are void afterwards), and the per-layer held counts are returned (synchronises once).
        prune() stays legal under a held mask and reads the raw fp32 parameters, frozen values included: prune(q) followed by
        hold_pruned gives gradual pruning, but a frozen weight may rank above the new threshold, so the held fraction can exceed
        the requested one -- the returned counts are the true ones.
        Refused: weight-noise mode (sample() packs drawn weights and would need a masked draw), the sharded update, an engine
        with fuse_kl = False (its parameters are stepped by the module-level update, which knows no mask: the frozen weights would
        move), and a mask that leaves a layer without a kept weight.
        The mask tensors are allocated by the FIRST hold and updated in place by later ones, so their device addresses are stable
        while a mask is held; a step captured by capture_step whose issue() contained prepare() or update() replays the calls it
        recorded -- masked with those addresses if it was captured under a held mask, unmasked if not. Capture such a step again
        after the first hold_pruned and after release_pruned. prune_units / compact / compress are refused while a mask is held; compressing
        a held network by its mask is the follow-up. The data-parallel all-reduce mode works as it stands: the update is
        rank-local and identical on every rank (hold the same result on every rank)."""
        if not isinstance(result, PruneResult) or result.engine is not self:
            raise ValueError("hold_pruned: a PruneResult of this engine")
        if self.mode == "wn":
            raise RuntimeError("hold_pruned: weight-noise mode packs drawn weights in sample(), which knows no mask -- LRT only")
        if self.sharded:
            raise RuntimeError("hold_pruned: not with the sharded update (every rank sweeps a slice of the rows)")
        if not self.fuse_kl:
            raise RuntimeError("hold_pruned: needs opt.fuse_kl = True (FusedMLP.update is the only update that carries the mask)")
        if result.version != self._pver:
            raise RuntimeError("hold_pruned: the parameters changed since this result was taken (prune() again)")
        masks = []
        for li in range(len(self.vb)):
            m = result.mask(li).to(torch.uint8)
            masks.append(m if self._held is None else torch.bitwise_or(m, self._held[li]))
        counts = torch.stack([m.sum(dtype=torch.int64) for m in masks]).cpu().tolist()
        for li, (v, n) in enumerate(zip(self.vb, counts)):
            if n >= v.O * v.I:
                raise RuntimeError(f"hold_pruned: VB layer {li} would be left without a kept weight")
        if self._held is None:
            self._held = [m.contiguous() for m in masks]
        else:                                                 # in place: the addresses a captured update holds stay valid
            for old, m in zip(self._held, masks):
                old.copy_(m)
        self._held_counts = [int(n) for n in counts]
        self.prepare()
        return self.held

    @_ordered
    def release_pruned(self):
        """Drops the held mask and runs the ordinary prepare(): the frozen weights are back, with the values (and Adam moments)
        they had when they were held."""
        self._held = self._held_counts = None
        self.prepare()

    # ---- structured pruning (csrc/units.hip): whole hidden units by the group form of mainviz.lua:20-21, and the compact engine
    # that is left -- a smaller DENSE network for the ordinary kernels. Nothing of this engine changes: prune_units reads the
    # fp32 parameters, compact writes a new FusedMLP.
    def _unit_descs(self, keys, keep, n_keep, lis):
        descs = (L.UnitDesc * len(lis))()
        for j, li in enumerate(lis):
            v = self.vb[li]
            descs[j] = L.UnitDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, key=_p(keys[li]),
                                  keep=_p(keep[li]) if keep is not None else None,
                                  n_keep=C.c_void_p(n_keep.data_ptr() + 4 * li) if n_keep is not None else None)
        return descs

    @_ordered
    def unit_snr(self, li):
        """||means[o, :]|| / ||sigma[o, :]|| of VB layer li's output units as an O-element fp32 tensor: the unit pruning key, bit
        for bit (|mu| / sigma of mainviz.lua:20 when the layer has one input)."""
        self._need_gathered_parameters("unit_snr")
        keys = {li: torch.empty(self.vb[li].O, dtype=torch.float32, device=self.device)}
        L.check(L.lib().vbnn_unit_snr(self.ctx.h, 1, self._unit_descs(keys, None, None, [li])))
        return keys[li]

    @_ordered
    def prune_units(self, fraction=None, threshold=None, scope="global", multiple=1):
        """Prune whole hidden units by signal-to-noise ratio: every output unit of a VB layer with ||mu_o|| / ||sigma_o|| < tau.
        Exactly one of threshold (tau itself) and fraction in [0, 1] (tau = the exact k-th smallest unit key, k = floor(fraction
        n_units), so at most k units go -- fewer when keys tie at tau; fraction = 1: tau = +inf). scope = "global": one tau over
        the units of all VB layers; "layer": the fraction applies to each layer. multiple: every layer's kept count is rounded
        UP to a multiple of it (capped at the layer's width) by taking back the best of the pruned units -- 256 gives widths the
        tiled GEMM kernels take; a layer never loses its last unit. Returns a UnitPruneResult (synchronises once, to read tau and
        the kept counts); nothing changes in this engine -- compact(result) builds the smaller one."""
        if (fraction is None) == (threshold is None):
            raise ValueError("prune_units: exactly one of fraction and threshold")
        if scope not in ("global", "layer"):
            raise ValueError(f"prune_units: scope = {scope!r} ('global' or 'layer')")
        if fraction is not None and not 0.0 <= float(fraction) <= 1.0:
            raise ValueError(f"prune_units: fraction = {fraction} (0 .. 1)")
        if int(multiple) != multiple or int(multiple) < 1:
            raise ValueError(f"prune_units: multiple = {multiple} (an integer >= 1)")
        self._refuse_held("prune_units")
        self._need_gathered_parameters("prune_units")
        if not self._shadows_ready:            # (prepare() counts as a parameter change: do it before the snapshot is versioned)
            self.prepare()
        lib, ctx, dev, nl = L.lib(), self.ctx.h, self.device, len(self.vb)
        keys = [torch.empty(v.O, dtype=torch.float32, device=dev) for v in self.vb]
        keep = [torch.zeros(v.O, dtype=torch.int32, device=dev) for v in self.vb]
        words = torch.zeros(2 * nl, dtype=torch.int32, device=dev)               # [tau per layer | kept count per layer]: ONE read-back
        tau, n_keep = words[:nl].view(torch.float32), words[nl:]
        tau_host = float(threshold) if threshold is not None else float("inf")
        select = fraction is not None and float(fraction) < 1.0                   # else the threshold is a host value
        every = list(range(nl))
        L.check(lib.vbnn_unit_snr(ctx, nl, self._unit_descs(keys, keep, n_keep, every)))
        for g in ([every] if scope == "global" else [[li] for li in every]):
            if select:                         # the threshold stays on the device, behind the select
                n_g = sum(self.vb[li].O for li in g)
                k = min(int(math.floor(float(fraction) * n_g)), n_g - 1)
                L.check(lib.vbnn_unit_select(ctx, len(g), self._unit_descs(keys, keep, n_keep, g), k, C.c_void_p(tau.data_ptr() + 4 * g[0])))
        L.check(lib.vbnn_unit_index(ctx, nl, self._unit_descs(keys, keep, n_keep, every), _p(tau) if select else None, tau_host,
                                    int(multiple)))
        host = words.cpu()
        counts = host[nl:].tolist()
        return UnitPruneResult(self, scope, multiple, host[:nl].view(torch.float32).tolist() if select else [tau_host] * nl,
                               [keep[li][:counts[li]] for li in every], self.sizes, self.n_classes, self._pver)

    @_ordered
    def compact(self, result, **opt_overrides):
        """The network `result` (a UnitPruneResult of this engine) leaves, as a new, ordinary FusedMLP on the same device: hidden =
        result.hidden, one process; means / lvars / bias of every VB layer and the final weight gathered on the device (a
        layer's rows by its own kept list, its columns by the previous layer's; the first layer keeps every input), the final
        bias copied, prepare()d, with this engine's seed and draw counter and a fresh optimiser state. The removed units'
        constant activations are dropped, not folded into the next bias. The noise of the compact engine is addressed by the
        compacted unit index: its sampled predictions are the pruned network's in distribution, not draw for draw.
        opt_overrides: options of the new engine that differ from this one's."""
        if not isinstance(result, UnitPruneResult) or result.engine is not self:
            raise ValueError("compact: a UnitPruneResult of this engine")
        self._refuse_held("compact")
        if result.version != self._pver:
            raise RuntimeError("compact: the parameters changed since this result was taken (prune_units() again)")
        self._need_gathered_parameters("compact")
        opt = dict(self.opt)
        for name in ("exchange_mode", "exchange", "cu_budget"):                   # one process, this engine's stream
            opt.pop(name, None)
        opt.update(opt_overrides)
        opt["hidden"] = list(result.hidden)
        new = FusedMLP(opt, device=self.device, stream=self.ctx.torch_stream)
        lib = L.lib()
        with new._on_stream():
            cols = None
            for v, w, rows in zip(self.vb, new.vb, result.keep):
                a = L.UnitGatherArgs(means=_p(v.means), lvars=_p(v.lvars), bias=_p(v.bias), O=v.O, I=v.I, rows=_p(rows), n_rows=w.O,
                                     cols=_p(cols), n_cols=w.I, dst_means=_p(w.means), dst_lvars=_p(w.lvars), dst_bias=_p(w.bias))
                L.check(lib.vbnn_unit_gather(new.ctx.h, C.byref(a)))
                cols = rows
            a = L.UnitGatherArgs(means=_p(self.weight3), lvars=None, bias=None, O=self.n_classes, I=self.sizes[-1], rows=None,
                                 n_rows=self.n_classes, cols=_p(cols), n_cols=new.sizes[-1], dst_means=_p(new.weight3),
                                 dst_lvars=None, dst_bias=None)
            L.check(lib.vbnn_unit_gather(new.ctx.h, C.byref(a)))
            a = L.UnitGatherArgs(means=_p(self.bias3), lvars=None, bias=None, O=1, I=self.n_classes, rows=None, n_rows=1, cols=None,
                                 n_cols=self.n_classes, dst_means=_p(new.bias3), dst_lvars=None, dst_bias=None)     # (a plain copy)
            L.check(lib.vbnn_unit_gather(new.ctx.h, C.byref(a)))
            new.draw = self.draw
            if new._draw_dev is not None:      # the new engine's device counter starts at zero: advance it to the mirror
                L.check(lib.vbnn_sample(new.ctx.h, _p(new._draw_dev), self.draw))
        new.prepare()
        return new

    def prune_units_curve(self, inputs, targets, fractions, S=None, map=False, scope="global", multiple=1):
        """What unit pruning costs: for every fraction q a prune_units(fraction=q, scope=scope, multiple=multiple), the compact
        engine and its predict(inputs, S, targets, map). One dict per fraction: fraction, tau (per layer), hidden, n_weights,
        nll, accuracy, mean_draw_nll, mean_draw_accuracy, mutual_info (mean over rows). Every compact engine starts from THIS
        engine's draw counter, which does not move: the points see the same draws (addressed by their own unit indices)."""
        rows = []
        for q in fractions:
            res = self.prune_units(fraction=q, scope=scope, multiple=multiple)
            p = self.compact(res).predict(inputs, S=S, targets=targets, map=map)
            rows.append(dict(fraction=float(q), tau=res.tau, hidden=res.hidden, n_weights=res.n_weights, nll=p.nll,
                             accuracy=p.accuracy, mean_draw_nll=p.mean_draw_nll, mean_draw_accuracy=p.mean_draw_accuracy,
                             mutual_info=float(p.mutual_info.mean().item())))
        return rows

    # ---- signal-to-noise pruning (mainviz.lua:20-27) and the pruned view of predict(). Nothing of the training step is
    # touched: the pruned operands are shadows of their own (PruneResult), read by predict() alone while the view is set.
    def _prune_descs(self, mu_p, var_p, stats, lis, masks=None):
        descs = (L.PruneDesc * len(lis))()
        for j, li in enumerate(lis):
            v = self.vb[li]
            descs[j] = L.PruneDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I, mu_p=mu_p[li].ptr, var_p=var_p[li].ptr,
                                   ld_w=mu_p[li].ld, stats=C.c_void_p(stats[li].data_ptr()),
                                   mask=_p(masks[li]) if masks is not None else None)
        return descs

    @_ordered
    def snr(self, li):
        """|means / sqrt(exp(lvars))| of VB layer li (mainviz.lua:20) as an O x I fp32 tensor: the pruning key, bit for bit."""
        self._need_gathered_parameters("snr")
        v = self.vb[li]
        out = torch.empty_like(v.means)
        L.check(L.lib().vbnn_snr(self.ctx.h, _p(v.means), _p(v.lvars), v.O * v.I, _p(out)))
        return out

    @_ordered
    def prune(self, fraction=None, threshold=None, scope="global"):
        """Prune by signal-to-noise ratio: every weight with |mu| / sigma < tau (mainviz.lua:20-21). Exactly one of
        threshold (tau itself; the reference uses 0.005) and fraction in [0, 1] (tau = the exact k-th smallest key,
        k = floor(fraction W), so at most k weights go -- fewer when keys tie at tau; fraction = 1: tau = +inf, everything).
        scope = "global": one tau over all VB layers; "layer": the fraction applies to each layer (one tau per layer).
        Returns a PruneResult (synchronises to read tau and the counts); nothing changes for predict() until use_pruned.
        Under a held mask (hold_pruned) the keys are still those of the raw fp32 parameters, frozen weights included."""
        if (fraction is None) == (threshold is None):
            raise ValueError("prune: exactly one of fraction and threshold")
        if scope not in ("global", "layer"):
            raise ValueError(f"prune: scope = {scope!r} ('global' or 'layer')")
        if fraction is not None and not 0.0 <= float(fraction) <= 1.0:
            raise ValueError(f"prune: fraction = {fraction} (0 .. 1)")
        self._need_gathered_parameters("prune")
        if not self._shadows_ready:            # (predict under the view reads the packed final weight)
            self.prepare()
        lib, ctx, dev, nl = L.lib(), self.ctx.h, self.device, len(self.vb)
        mu_p = [_Packed(v.O, v.I, self.tdt, dev) for v in self.vb]
        var_p = [_Packed(v.O, v.I, self.tdt, dev) for v in self.vb]
        stats = torch.zeros(nl, 4, dtype=torch.float64, device=dev)
        tau = torch.full((nl,), float(threshold) if threshold is not None else float("inf"), dtype=torch.float32, device=dev)
        groups = [list(range(nl))] if scope == "global" else [[li] for li in range(nl)]
        nbytes = C.c_size_t()
        L.check(lib.vbnn_prune_workspace_bytes(nl, self._prune_descs(mu_p, var_p, stats, list(range(nl))), C.byref(nbytes)))
        if self._prune_ws is None or self._prune_ws.numel() < nbytes.value:
            self._prune_ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        for g in groups:
            descs = self._prune_descs(mu_p, var_p, stats, g)
            Wg = sum(self.vb[li].O * self.vb[li].I for li in g)
            k = int(math.floor(float(fraction) * Wg)) if fraction is not None else Wg
            tau_g = C.c_void_p(tau.data_ptr() + 4 * g[0]) if k < Wg else None       # on the device, behind the select
            if tau_g is not None:
                L.check(lib.vbnn_prune_select(ctx, len(g), descs, k, tau_g, _p(self._prune_ws), self._prune_ws.numel()))
                if len(g) > 1:
                    tau[g[0] + 1:g[-1] + 1] = tau[g[0]]
            L.check(lib.vbnn_prune_pack(ctx, self.code, len(g), descs, tau_g,
                                        float(threshold) if threshold is not None else float("inf")))
        return PruneResult(self, scope, tau.cpu().tolist(), stats.cpu().tolist(), mu_p, var_p, self._pver)

    @_ordered
    def _prune_mask(self, res, li):
        if res.engine is not self or res.version != self._pver:
            raise RuntimeError("PruneResult.mask: the parameters changed since this result was taken")
        self._need_gathered_parameters("mask")
        v = self.vb[li]
        masks = {li: torch.zeros(v.O, v.I, dtype=torch.uint8, device=self.device)}
        stats = {li: torch.zeros(4, dtype=torch.float64, device=self.device)}
        descs = self._prune_descs(res.mu_p, res.var_p, stats, [li], masks)          # the same sweep: the shadows get the same bits
        L.check(L.lib().vbnn_prune_pack(self.ctx.h, self.code, 1, descs, None, res.tau[li]))
        return masks[li].bool()

    def use_pruned(self, result):
        """predict() reads the pruned operands of `result` (a PruneResult of this engine) from now on; None: the unpruned
        shadows again. Nothing else looks at the view: run / test / update / prepare and their operands are untouched
        (hold_pruned is what trains a pruned network)."""
        if result is not None and (not isinstance(result, PruneResult) or result.engine is not self):
            raise ValueError("use_pruned: a PruneResult of this engine, or None")
        self._pruned = result

    @contextlib.contextmanager
    def pruned(self, result):
        """with eng.pruned(result): ... -- use_pruned(result) for the block, the previous view afterwards."""
        prev = self._pruned
        self.use_pruned(result)
        try:
            yield result
        finally:
            self._pruned = prev

    def prune_curve(self, inputs, targets, fractions, S=None, map=False, scope="global"):
        """What pruning costs: for every fraction q a prune(fraction=q, scope=scope) and a predict(inputs, S, targets, map)
        under that view. One dict per fraction: fraction, tau (per layer), n_pruned, nll, accuracy, mean_draw_nll,
        mean_draw_accuracy, mutual_info (mean over rows). The keys are re-formed by every select and pack sweep (nothing per
        weight is kept between the points). Each point consumes S draws as a predict() call of its own would (none with
        map=True), so the points see different noise; the engine's view is afterwards what it was before."""
        rows = []
        for q in fractions:
            res = self.prune(fraction=q, scope=scope)
            with self.pruned(res):
                p = self.predict(inputs, S=S, targets=targets, map=map)
            rows.append(dict(fraction=float(q), tau=res.tau, n_pruned=res.n_pruned, nll=p.nll, accuracy=p.accuracy,
                             mean_draw_nll=p.mean_draw_nll, mean_draw_accuracy=p.mean_draw_accuracy,
                             mutual_info=float(p.mutual_info.mean().item())))
        return rows

    def prune_curve_sparse(self, inputs, targets, fractions, S=None, map=False, scope="global"):
        """prune_curve with every point evaluated through the compressed form (prune(...).compress() as the view)."""
        rows = []
        for q in fractions:
            res = self.prune(fraction=q, scope=scope).compress()
            with self.pruned(res):
                p = self.predict(inputs, S=S, targets=targets, map=map)
            rows.append(dict(fraction=float(q), tau=res.tau, n_pruned=res.n_pruned, nnz=sum(res.nnz), nbytes=res.nbytes,
                             dense_nbytes=res.dense_nbytes, nll=p.nll, accuracy=p.accuracy, mean_draw_nll=p.mean_draw_nll,
                             mean_draw_accuracy=p.mean_draw_accuracy, mutual_info=float(p.mutual_info.mean().item())))
        return rows

    # ---- the compressed pruned view (csrc/sparse.hip). compress: a PruneResult's kept weights as CSR, built on the device at
    # the result's own tau (the entry count is known from its statistics: no extra synchronisation before the allocation).
    # _predict_forward_sparse: predict's forward under such a view -- K-major activations from layer to layer (xT from the
    # input packer, hT from every layer but the last, which writes the row-major h the head reads), squares formed in registers.
    @_ordered
    def _compress(self, res):
        if not isinstance(res, PruneResult) or res.engine is not self:
            raise ValueError("compress: a PruneResult of this engine")
        self._refuse_held("compress")
        if res.version != self._pver:
            raise RuntimeError("compress: the parameters changed since this result was taken (prune() again)")
        if isinstance(res, SparsePruneResult):
            return res
        self._need_gathered_parameters("compress")
        lib, ctx, dev, nl = L.lib(), self.ctx.h, self.device, len(self.vb)
        nnz = [int(st[3]) - int(st[0]) for st in res.stats]                       # W - pruned, as vbnn_prune_pack counted them
        idx = [2 if v.I <= 65536 else 4 for v in self.vb]
        row_ptr = [torch.zeros(v.O + 1, dtype=torch.int32, device=dev) for v in self.vb]
        cols = [torch.zeros(max(n, 1), dtype=torch.int16 if ib == 2 else torch.int32, device=dev) for n, ib in zip(nnz, idx)]
        mu_v = [torch.zeros(max(n, 1), dtype=self.tdt, device=dev) for n in nnz]
        var_v = [torch.zeros(max(n, 1), dtype=self.tdt, device=dev) for n in nnz]
        nnz_dev = torch.zeros(nl, dtype=torch.int32, device=dev)
        for li, v in enumerate(self.vb):
            pd = (L.PruneDesc * 1)(L.PruneDesc(means=_p(v.means), lvars=_p(v.lvars), O=v.O, I=v.I))
            sd = (L.SparseDesc * 1)(L.SparseDesc(row_ptr=_p(row_ptr[li]), cols=_p(cols[li]), mu_v=_p(mu_v[li]), var_v=_p(var_v[li]),
                                                 O=v.O, I=v.I, nnz_cap=nnz[li], nnz_dev=C.c_void_p(nnz_dev.data_ptr() + 4 * li),
                                                 idx_bytes=idx[li]))
            L.check(lib.vbnn_prune_compress(ctx, self.code, 1, pd, sd, None, res.tau[li]))
        got = [n & 0xffffffff for n in nnz_dev.cpu().tolist()]
        if got != nnz:
            raise RuntimeError(f"compress: the device kept {got} weights per layer, the pruning's statistics say {nnz}")
        esz = torch.empty(0, dtype=self.tdt).element_size()
        dense = sum(2 * v.O * L.pad_ld(v.I) * esz for v in self.vb)
        return SparsePruneResult(res, row_ptr, cols, mu_v, var_v, nnz, idx, dense)

    def _sparse_buffers(self, rows):
        """K-major operands of the sparse forward: T[0] the packed input's transpose, T[li + 1] layer li's hT (ping-pong per
        hidden width, as _predict_buffers). Kept across calls while the row count holds."""
        if getattr(self, "_sparse_key", None) != rows:
            slots = {}
            T = [_Packed(self.sizes[0], rows, self.tdt, self.device)]
            for li, v in enumerate(self.vb[:-1]):
                if (v.O, li % 2) not in slots:
                    slots[(v.O, li % 2)] = _Packed(v.O, rows, self.tdt, self.device)
                T.append(slots[(v.O, li % 2)])
            self._sparse_bufs, self._sparse_key = T, rows
        return self._sparse_bufs

    def _predict_forward_sparse(self, bufs, x, N, rpd, draw, row0, lrt, pack=True):
        """_predict_forward under a compressed view: vbnn_pack_input (with the transposed copy) + vbnn_forward_sparse per layer."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        pv, nl = self._pruned, len(self.vb)
        T = self._sparse_buffers(bufs[0].x.t.shape[0])
        if pack:                               # (the packer always writes the row-major copy too; no sparse layer reads it)
            b0 = bufs[0]
            L.check(lib.vbnn_pack_input(ctx, code, _p(x), x.stride(0), N, self.sizes[0], b0.x.ptr, None, b0.x.ld, T[0].ptr, None,
                                        T[0].ld, rpd))
        for li, v in enumerate(self.vb):
            last = li == nl - 1
            out = bufs[li + 1]
            a = L.SparseFwdArgs(row_ptr=_p(pv.row_ptr[li]), cols=_p(pv.cols[li]), mu_v=_p(pv.mu_v[li]),
                                var_v=_p(pv.var_v[li]) if lrt else None, idx_bytes=pv.idx_bytes[li], xT=T[li].ptr, x2T=None,
                                ld_xT=T[li].ld, N=N, I=v.I, O=v.O, bias=_p(v.bias), seed=self.seed, layer=v.layer_id, draw=draw,
                                row0=row0, y=None, ld_y=0, relu=1, h=out.x.ptr if last else None, h2=None,
                                ld_h=out.x.ld if last else 0, hT=None if last else T[li + 1].ptr, h2T=None,
                                ld_hT=0 if last else T[li + 1].ld, rows_per_draw=rpd)
            L.check(lib.vbnn_forward_sparse(ctx, code, C.byref(a)))
