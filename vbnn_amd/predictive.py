"""The posterior predictives of the fused engine (FusedMLP.predict / predict_classes / predict_regression / predict_quantiles /
predict_labels, and the sampling-free predict_analytic): forward-only passes on buffers of their own, dense or under a pruned view (pruning.py). A
mixin of vbnn_amd/engine.py:FusedMLP."""
import ctypes as C
import functools
import math
import types

import torch

from . import _lib as L
from .nn import _Packed, _ordered, _p
from .pruning import SparsePruneResult


def _off(t, row):
    """The address of element `row` of t (4-byte elements), None without t."""
    return C.c_void_p(t.data_ptr() + 4 * row) if t is not None else None


def _chunk_sums(totals):
    """The chunks' totals (chunks x NT doubles on the device) added in chunk order; synchronises."""
    return [sum(col) for col in zip(*totals.cpu().tolist())]


def _gemm(lib, ctx, code, w, xin, N, I, O, bias, y, ld_y):
    """One single product of vbnn_forward: y = x w^T (+ bias), fp32 out (N x O, pitch ld_y)."""
    fa = L.FwdArgs(w=w.ptr, w2=None, x=xin.ptr, x2=None, ld_w=w.ld, ld_x=xin.ld, N=N, I=I, O=O, bias=bias, y=y, ld_y=ld_y)
    L.check(lib.vbnn_forward(ctx, code, C.byref(fa)))


def _stamp(res, S, stacked, chunks):
    """The pass a result came from: its draws, whether they ran stacked, its chunks."""
    res.S, res.stacked, res.chunks = S, stacked, chunks
    return res


# ---- what the entry points (`what`, for the messages) check of their arguments before anything is prepared or allocated; each
# returns the argument as the body uses it
def _check_draws(what, S, max_S=None):
    if S < 1:
        raise ValueError(f"{what}: S = {S} draws (at least one)")
    if max_S is not None and S > max_S:
        raise ValueError(f"{what}: S = {S} draws (at most {max_S})")
    return S


def _check_noise_var(what, noise_var):
    noise_var = None if noise_var is None else float(noise_var)
    if noise_var is not None and not (noise_var > 0.0 and math.isfinite(noise_var)):
        raise ValueError(f"{what}: noise_var = {noise_var} (a finite variance above zero, or None)")
    return noise_var


def _check_topk(what, topk, n_classes):
    K = int(topk)
    if not 0 <= K <= min(L.CLASS_MOMENTS_MAX_K, n_classes):
        raise ValueError(f"{what}: topk = {K} (0 .. {L.CLASS_MOMENTS_MAX_K}, and at most n_classes = {n_classes})")
    return K


def _check_class_targets(what, targets, R):
    if targets is not None and (targets.dtype != torch.int32 or not targets.is_cuda or targets.numel() != R):
        raise ValueError(f"{what}: targets of shape {tuple(targets.shape)} (R = {R} int32 class indices on the device)")
    return None if targets is None else targets.contiguous()


def _check_regression_targets(what, targets, R, D):
    if targets is not None and (targets.dtype != torch.float32 or not targets.is_cuda or tuple(targets.shape) != (R, D)):
        raise ValueError(f"{what}: targets of shape {tuple(targets.shape)} (R x D = {R} x {D} fp32 on the device)")
    return None if targets is None else targets.contiguous()


def _refuse_bce(what, criterion):
    """The predictives of the other likelihoods on a Bernoulli engine: the remedy is predict_labels."""
    if criterion == "bce":
        raise ValueError(f"{what}: criterion = 'bce' (independent sigmoid outputs) has a multi-label predictive of its own: "
                         "use predict_labels")


class _PredictBuffers(list):
    """predict's operands per layer input (+ .r, the sequential bf16 forwards' throwaway noise factor; .y_reg: predict_regression's y)."""
    r = y_reg = None


class PredictResult:
    """FusedMLP.predict's outputs for R minibatch rows. Device tensors: probs / log_probs (R x C fp32: the S-draw average
    1/S sum_s softmax(f_s(x)) and its log), entropy (H[p]), expected_entropy (1/S sum_s H(p_s)), mutual_info (their difference:
    the epistemic part), pred (int32, argmax p). With targets also Python floats: nll (mean -log p[t]) and accuracy (percent)
    of the averaged prediction, and mean_draw_nll / mean_draw_accuracy -- the mean over draws of each draw's NLL and accuracy,
    the two numbers test() returns. None without targets.
    FusedMLP.predict_classes (any class count) returns the same fields with the same meanings (probs / log_probs None with
    keep_probs=False) and, with topk = K > 0, topk_idx (R x K int32: the K most probable classes, most probable first, ties to
    the lower index) and topk_prob (R x K: their probabilities), with targets topk_accuracy (percent of rows whose target is
    among them); with keep_draws, draws (S x R x C: every draw's logits). totals: the library's sums.
    FusedMLP.predict_analytic (criterion "nll") returns the same fields from S draws of the propagated logit distribution, with
    logit_mean / logit_var (R x C: the propagated moments they were drawn from) and, with keep_probs, draws (the sampled logits)."""

    def __init__(self, probs, log_probs, entropy, expected_entropy, mutual_info, pred):
        self.probs, self.log_probs, self.entropy = probs, log_probs, entropy
        self.expected_entropy, self.mutual_info, self.pred = expected_entropy, mutual_info, pred
        self.nll = self.accuracy = self.mean_draw_nll = self.mean_draw_accuracy = None
        self.totals = self.topk_idx = self.topk_prob = self.topk_accuracy = self.draws = None
        self.logit_mean = self.logit_var = None                # predict_analytic: the propagated logit moments (R x C)
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
    N(m_s, diag exp(s_s)).
    FusedMLP.predict_analytic (criterion "mse") returns the same fields without draws: S = 0 and draws None; mean and var are the
    PROPAGATED output mean and epistemic variance (no Monte-Carlo noise); row_log_lik / log_lik are those of ONE Gaussian
    N(mean, var + noise_var) per output; mean_draw_mse is its expectation under that Gaussian, mse + mean_var; totals =
    [sum row_sq_err, sum (row_sq_err + D row_var), sum row_log_lik (0 without noise_var), sum var]."""

    def __init__(self, mean, var, row_var, row_sq_err, row_log_lik, draws):
        self.mean, self.var, self.row_var = mean, var, row_var
        self.row_sq_err, self.row_log_lik, self.draws = row_sq_err, row_log_lik, draws
        self.totals = self.mse = self.mean_draw_mse = self.log_lik = self.mean_var = None
        self.noise_var = self.row_noise_var = self.mean_noise_var = self.mean_draw_nll = None
        self.S, self.stacked, self.chunks = None, None, None


class LabelPredictResult:
    """FusedMLP.predict_labels' outputs for R minibatch rows of D labels (criterion "bce"). Device tensors, R x D: probs (the
    S-draw average 1/S sum_s sigmoid(f_s(x)) per label), entropy (the binary entropy of probs: total uncertainty per label),
    mutual_info (entropy minus the draws' mean entropy: the epistemic part, BALD per label; exactly 0 for S = 1); R:
    row_entropy, row_mutual_info (their sums over the labels); with targets (R x D in [0, 1]) row_log_lik (R: the log of the
    equal-weight mixture over draws of the JOINT likelihood of the row's label vector), row_marg_log_lik (R: the log-likelihood
    under the product of the per-label marginals probs), row_hits (R int32: labels predicted right, a label being predicted 1 iff
    its probability exceeds that of 0); draws (S x R x D logits) with keep_draws. With targets also Python floats: totals (the
    library's five sums), log_lik and marg_log_lik (means over rows), mean_draw_bce (the mean over draws of each draw's
    criterion: test()'s number), label_accuracy (percent of the R D labels) and exact_match (percent of rows with every label
    right). None without targets."""

    def __init__(self, probs, entropy, mutual_info, row_entropy, row_mutual_info):
        self.probs, self.entropy, self.mutual_info = probs, entropy, mutual_info
        self.row_entropy, self.row_mutual_info = row_entropy, row_mutual_info
        self.row_log_lik = self.row_marg_log_lik = self.row_hits = self.draws = self.totals = None
        self.log_lik = self.marg_log_lik = self.mean_draw_bce = self.label_accuracy = self.exact_match = None
        self.S, self.stacked, self.chunks = None, None, None


class QuantilePredictResult:
    """FusedMLP.predict_quantiles' outputs for R minibatch rows of D outputs. probs: the Q probabilities (Python floats, as fp32
    holds them); quantiles (Q x R x D device tensor: per output the p_j-quantile of the S-component predictive mixture, ascending
    in j); moments: the RegressionPredictResult of the same draws, bit for bit predict_regression's; kind: "empirical" (mse
    without noise_var: the draws are the distribution -- epistemic-only intervals), "fixed_noise" (mse with noise_var) or
    "gauss"; draws (S x R x W) with keep_draws. With targets: pit (R x D: the mixture's CDF at the target -- uniform on [0, 1] for
    a calibrated predictive), row_le (R x Q int32: per row the number of outputs with t <= q_j), count_le (Q integers, their
    totals) and calibration (Q Python floats, count_le / (R D): calibrated means calibration[j] ~ probs[j]). None without."""

    def __init__(self, probs, quantiles, moments, kind):
        self.probs, self.quantiles, self.moments, self.kind = probs, quantiles, moments, kind
        self.pit = self.row_le = self.count_le = self.calibration = self.draws = None
        self.S = moments.S

    def _index(self, p):
        p32 = float(torch.tensor(p, dtype=torch.float32))
        for j, pj in enumerate(self.probs):
            if pj == p32:
                return j
        raise ValueError(f"interval: the probability {p:g} is not among probs = {self.probs}")

    def interval(self, level):
        """The central interval of mass `level`: (lo, hi, coverage, mean_width) -- the (1 - level) / 2 and (1 + level) / 2
        quantiles (R x D device tensors; both probabilities must be among probs), and with targets the fraction of targets in
        (lo, hi] (calibration_hi - calibration_lo; calibrated means ~ level), else None; mean_width: the mean of hi - lo."""
        lo, hi = self._index((1.0 - level) / 2), self._index((1.0 + level) / 2)
        cov = self.calibration[hi] - self.calibration[lo] if self.calibration is not None else None
        ql, qh = self.quantiles[lo], self.quantiles[hi]
        return ql, qh, cov, float((qh - ql).double().mean())


class _Predictive:
    def _predictive_inputs(self, what, inputs, row0):
        """What every predictive (`what`, for the messages) does with its inputs ahead of any allocation: checks them, resolves
        row0 (default: this rank's first row, as run()), prepares a fresh engine and refuses a stale pruned view. Returns x
        (R x sizes[0]), R, row0."""
        if inputs.dim() < 1 or inputs.shape[0] < 1 or inputs.numel() != inputs.shape[0] * self.sizes[0]:
            raise ValueError(f"{what}: inputs of shape {tuple(inputs.shape)} (R x {self.sizes[0]}, R >= 1)")
        x = inputs.reshape(inputs.shape[0], -1)
        if x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError(f"{what}: inputs are fp32 device tensors")
        R = x.shape[0]
        row0 = self.rank * R if row0 is None else int(row0)
        if not self._shadows_ready:            # a fresh engine: the shadows test() would have prepared
            self.prepare()
        # a pruned view replaces the operand shadows: it must be of THESE parameters
        if self._pruned is not None and self._pruned.version != self._pver:
            raise RuntimeError(f"{what}: the pruned view was taken from older parameters (update / prepare / init_parameters "
                               "ran since): prune() again, or use_pruned(None)")
        return x, R, row0

    def _predictive_plan(self, what, inputs, S, map, row0, max_S=None):
        """What the sampled predictives share ahead of their chunk loops: resolves S / map, _predictive_inputs, and decides the
        pass -- x (R rows), S, map, row0, lrt, stacked, Rc minibatch rows per chunk (n_chunks of them, op_rows operand rows
        each), the buffers, WN's weights, d0."""
        map = bool(map or self.opt.get("quicktest"))
        S = _check_draws(what, 1 if map else int(self.opt["testSamples"] if S is None else S), max_S)
        x, R, row0 = self._predictive_inputs(what, inputs, row0)
        if self._pruned is not None and self.mode == "wn" and not map:
            raise ValueError(f"{what}: weight-noise draws under a pruned view are not supported -- they sample from the fp32 "
                             "means / lvars, which the view does not replace (use map=True, or mode = 'lrt')")
        lrt = self.mode == "lrt" and not map
        stacked = self._predict_stacked(R, S, lrt)
        cap = max(1, int(self.opt.get("predict_rows", 32768)))
        Rc = max(1, min(R, cap // S if stacked else cap))           # minibatch rows per chunk: S Rc (stacked) or Rc operand rows
        op_rows = S * Rc if stacked else Rc
        return types.SimpleNamespace(x=x, R=R, S=S, map=map, row0=row0, lrt=lrt, stacked=stacked, Rc=Rc, n_chunks=(R + Rc - 1) // Rc,
                                     op_rows=op_rows, bufs=self._predict_buffers(op_rows, lrt),
                                     wts=self._predict_weights() if self.mode == "wn" else None, d0=self.draw + 1)   # (d0: draw 1's counter)

    @staticmethod
    def _chunks(p):
        """The plan's chunks in order: (k, c0, rows, xc) -- chunk k is minibatch rows [c0, c0 + rows), xc of x."""
        for k in range(p.n_chunks):
            c0 = k * p.Rc
            rows = min(p.Rc, p.R - c0)
            yield k, c0, rows, p.x[c0:c0 + rows]

    def _draw_forward(self, p, xc, rows, c0, s=None):
        """The draw step of the chunk at row c0, the one place that says which noise a row sees: WN's weights for the draw, then
        the pack and every VB layer's forward into p.bufs. s=None: all p.S draws in one pass, the chunk stacked S times as
        operand rows (draw s = rows [s rows, (s + 1) rows); S = 1 under map or WN). Otherwise draw s alone, draw 0 packing the
        chunk for the draws after it."""
        if s is None:
            N, rpd, draw, pack = p.S * rows, rows if p.S > 1 else 0, p.d0, True
            wn_draw = None if p.map else p.d0
        else:
            N, rpd, draw, pack = rows, 0, p.d0 + s, s == 0
            wn_draw = draw
        if p.wts is not None:
            self._predict_wn_sample(p.wts, wn_draw)
        self._predict_forward(p.bufs, p.wts, xc, N, rpd, draw, p.row0 + c0, p.lrt, pack=pack)

    def _consume_draws(self, S, map):          # the draws test() would have consumed: the host counter and the device's
        if not map:
            lib = L.lib()
            self.draw += S
            if self.device_draw:
                L.check(lib.vbnn_sample(self.ctx.h, _p(self._draw_dev), S))

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
        _refuse_bce("predict", self.criterion)
        if Cn > 16:
            raise ValueError(f"predict: the predictive head takes at most 16 classes (n_classes = {Cn})")
        if self.criterion != "nll":
            raise ValueError(f"predict: a class-probability predictive needs the NLL criterion (criterion = '{self.criterion}' has "
                             "none: use predict_regression)")
        targets = _check_class_targets("predict", targets, inputs.shape[0])   # (before the plan: nothing is prepared for a refused call)
        p = self._predictive_plan("predict", inputs, S, map, row0)
        R, S = p.R, p.S
        f32 = dict(dtype=torch.float32, device=self.device)
        res = PredictResult(torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32), torch.empty(R, **f32), torch.empty(R, **f32),
                            torch.empty(R, **f32), torch.empty(R, dtype=torch.int32, device=self.device))
        totals = torch.zeros(p.n_chunks, 4, dtype=torch.float64, device=self.device) if targets is not None else None
        state = torch.empty(p.Rc, Cn + 3, **f32) if not p.stacked else None
        h = p.bufs[len(self.vb)].x
        a = L.PredictArgs(h=h.ptr, ld_h=h.ld, w3=self.w3_s.ptr, ld_w=self.w3_s.ld, bias=_p(self.bias3), H=self.sizes[-1], C=Cn, S=S,
                          form=L.PREDICT_STACKED if p.stacked else L.PREDICT_ACCUMULATE, state=_p(state))
        for k, c0, rows, xc in self._chunks(p):
            a.R = rows
            a.target = _off(targets, c0)
            a.totals = _p(totals[k]) if totals is not None else None
            a.probs, a.log_probs = _off(res.probs, Cn * c0), _off(res.log_probs, Cn * c0)
            a.entropy, a.expected_entropy, a.mutual_info = _off(res.entropy, c0), _off(res.expected_entropy, c0), _off(res.mutual_info, c0)
            a.pred = _off(res.pred, c0)
            if p.stacked:                      # every draw in one pass
                self._draw_forward(p, xc, rows, c0)
                L.check(lib.vbnn_head_predict(ctx, code, C.byref(a)))
                continue
            for s in range(S):                 # one draw per forward, the running state between the head's launches
                self._draw_forward(p, xc, rows, c0, s)
                a.first, a.final = int(s == 0), int(s == S - 1)
                L.check(lib.vbnn_head_predict(ctx, code, C.byref(a)))
        self._consume_draws(S, p.map)
        self._class_moments_finish(res, totals, R, S, 0)
        return _stamp(res, S, p.stacked, p.n_chunks)

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

    def _pingpong(self, n_layers, make):
        """Activation buffers for the first n_layers VB layers, one ping-pong PAIR per width: layer li writes slot (O, li % 2), so
        a layer never overwrites its own input and a buffer always holds one layout (its pads stay zero). Returns
        [the input's buffer, layer 0's output, layer 1's, ...], each built by make(cols) on its slot's first use."""
        slots, out = {}, []
        for key in [(self.sizes[0], "in")] + [(v.O, li % 2) for li, v in enumerate(self.vb[:n_layers])]:
            if key not in slots:
                slots[key] = make(key[0])
            out.append(slots[key])
        return out

    def _predict_buffers(self, rows, lrt):
        """predict's operands (_pingpong): bufs[li] is layer li's input, bufs[len(vb)] the head's; x, and x2 (its square) where a
        layer reads one. Kept across calls while the row count holds."""
        sq = lrt and self.dtype == "bf16"                       # (fp32: the forward forms x.x from x itself)
        key = (rows, sq)
        if self._pred_key != key:
            self._pred_bufs, self._pred_key = None, None
            dev, tdt, nl = self.device, self.tdt, len(self.vb)
            bufs = _PredictBuffers(self._pingpong(nl, lambda cols: types.SimpleNamespace(x=_Packed(rows, cols, tdt, dev), x2=None)))
            if sq:                                              # (every VB layer reads its input's square; the head reads none)
                for b in bufs[:nl]:
                    b.x2 = b.x2 or _Packed(rows, b.x.cols, tdt, dev)
            bufs.r = _Packed(rows, max(v.O for v in self.vb), tdt, dev) if sq else None
            self._pred_bufs, self._pred_key = bufs, key
        return self._pred_bufs

    def _predict_weights(self):
        """WN: predict's own sampled weights (fp32) and their packed shadows, per layer (sample() keeps its draw in the training
        operands; predict leaves them alone)."""
        if self._pred_wts is None:
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
        if isinstance(self._pruned, SparsePruneResult):        # the compressed view: its own forward (below)
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
        return self._regression_predict("predict_regression", inputs, S, targets, noise_var, map, row0, keep_draws)

    def _regression_predict(self, what, inputs, S, targets, noise_var, map, row0, keep_draws, max_S=None):
        """predict_regression's body, which predict_quantiles (`what`, for the messages) runs too."""
        lib, ctx = L.lib(), self.ctx.h
        _refuse_bce(what, self.criterion)
        if self.criterion not in ("mse", "gauss"):
            raise ValueError(f"{what}: the regression predictive needs the MSE criterion or the Gaussian one "
                             "(criterion = 'nll': use predict)")
        gauss = self.criterion == "gauss"
        Wd = self.n_classes                                          # the final Linear's width: D, or { m[D], s[D] }
        D = Wd // 2 if gauss else Wd
        if gauss and noise_var is not None:
            raise ValueError(f"{what}: criterion = 'gauss' predicts its own noise variance (noise_var must be None)")
        noise_var = _check_noise_var(what, noise_var)
        targets = _check_regression_targets(what, targets, inputs.shape[0], D)      # (D: one target per mean; before the plan, as predict)
        p = self._predictive_plan(what, inputs, S, map, row0, max_S)
        R, S = p.R, p.S
        f32 = dict(dtype=torch.float32, device=self.device)
        has_t = targets is not None
        res = RegressionPredictResult(torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, **f32),
                                      torch.empty(R, **f32) if has_t else None,
                                      torch.empty(R, **f32) if (has_t and (gauss or noise_var is not None)) else None,
                                      torch.empty(S, R, Wd, **f32) if keep_draws else None)
        if gauss:
            res.noise_var, res.row_noise_var = torch.empty(R, D, **f32), torch.empty(R, **f32)
        one_call = p.stacked and D <= (L.GAUSS_MOMENTS_STACKED_MAX_D if gauss else L.MOMENTS_STACKED_MAX_D)   # else: ACCUMULATE per draw
        state = None if one_call else torch.empty(p.Rc, (3 if gauss else 2) * D + 2, **f32)
        totals = torch.zeros(p.n_chunks, 5 if gauss else 4, dtype=torch.float64, device=self.device) if has_t else None
        form = L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE
        if gauss:
            a = L.GaussMomentsArgs(ld_y=Wd, ld_t=D, D=D, S=S, form=form, s_min=self.logvar_clamp[0], s_max=self.logvar_clamp[1],
                                   state=_p(state), ld_out=D)
            moments = lib.vbnn_predict_gauss_moments
        else:
            a = L.MomentsArgs(ld_y=D, ld_t=D, D=D, S=S, form=form, noise_var=noise_var or 0.0, state=_p(state), ld_out=D)
            moments = lib.vbnn_predict_moments

        def point(c0, rows):                   # the chunk's targets and outputs
            a.R = rows
            a.target = _off(targets, c0 * D)
            a.totals = _p(totals[c0 // p.Rc]) if has_t else None
            a.mean, a.var = _off(res.mean, c0 * D), _off(res.var, c0 * D)
            a.row_var, a.row_sq_err, a.row_log_lik = _off(res.row_var, c0), _off(res.row_sq_err, c0), _off(res.row_log_lik, c0)
            if gauss:
                a.noise_var, a.row_noise_var = _off(res.noise_var, c0 * D), _off(res.row_noise_var, c0)

        self._moments_loop(p, Wd, res.draws, keep_draws, one_call, a, lambda: L.check(moments(ctx, C.byref(a))), point)
        self._consume_draws(S, p.map)
        if has_t:
            tot = _chunk_sums(totals)
            res.totals = tot
            res.mse = tot[0] / (R * D)
            if gauss:
                res.mean_draw_nll, res.mean_noise_var = tot[1] / (R * S * D), tot[4] / (R * D)
            else:
                res.mean_draw_mse = tot[1] / (R * S * D)
            res.log_lik = tot[2] / R if (gauss or noise_var is not None) else None
            res.mean_var = tot[3] / (R * D)
        return _stamp(res, S, p.stacked, p.n_chunks)

    # ---- the regression predictive's quantiles (vbnn_predict_quantiles): predict_regression's pass with the draws kept, then ONE
    # launch over all rows of them -- per output the quantiles of the S-component mixture, and with targets the probability
    # integral transform and the calibration counts.
    @_ordered
    def predict_quantiles(self, inputs, probs, S=None, targets=None, noise_var=None, map=False, row0=None, keep_draws=False):
        """The quantiles of p(y | x, D) ~ 1/S sum_s N(f_s(x), noise) per output at the probabilities `probs` (1 .. 8 of them,
        strictly ascending, each in [0.001, 0.999]) over draws self.draw + 1 .. self.draw + S (S <= 128), which `self.draw`
        advances by. Everything else is predict_regression's contract -- criteria "mse" and "gauss" only, S / targets / noise_var /
        map / row0 as there, chunking by opt.predict_rows, pruned views -- and its pass: `.moments` of the result is bit for bit
        what predict_regression gives from the same counter. The mixture follows the engine: "gauss" -> N(m_s, exp(s_s)); "mse"
        with noise_var -> N(f_s, noise_var); "mse" without -> the draws themselves (epistemic-only intervals). With targets the
        result carries pit, row_le, calibration and interval(level)'s coverage. keep_draws: the draws are returned too.
        Memory: the S x R x W fp32 draws (S R W 4 bytes, W the final Linear's width) are always held for the one quantile launch,
        returned or not; opt.predict_rows bounds the forward's buffers, NOT this. Returns a QuantilePredictResult."""
        lib, ctx = L.lib(), self.ctx.h
        probs = [float(v) for v in probs]
        Q = len(probs)
        p32 = torch.tensor(probs, dtype=torch.float32).tolist()          # as fp32 holds them: what the kernel compares
        if not 1 <= Q <= L.QUANTILES_MAX_Q:
            raise ValueError(f"predict_quantiles: {Q} probabilities (1 .. {L.QUANTILES_MAX_Q})")
        if not all(0.001 <= v <= 0.999 for v in probs) or any(b <= a for a, b in zip(p32, p32[1:])):
            raise ValueError(f"predict_quantiles: probs = {probs} (strictly ascending, each in [0.001, 0.999])")
        mom = self._regression_predict("predict_quantiles", inputs, S, targets, noise_var, map, row0, True, max_S=L.QUANTILES_MAX_S)
        draws = mom.draws
        if not keep_draws:
            mom.draws = None
        Sn, R, Wd = draws.shape
        gauss = self.criterion == "gauss"
        D = Wd // 2 if gauss else Wd
        kind = "gauss" if gauss else ("fixed_noise" if noise_var is not None else "empirical")
        res = QuantilePredictResult(p32, torch.empty(Q, R, D, dtype=torch.float32, device=self.device), mom, kind)
        res.draws = draws if keep_draws else None
        a = L.QuantilesArgs(y=_p(draws), ld_y=Wd, draw_stride=R * Wd, R=R, D=D, S=Sn, Q=Q,
                            kind={"gauss": L.QUANT_GAUSS, "fixed_noise": L.QUANT_FIXED_NOISE, "empirical": L.QUANT_EMPIRICAL}[kind],
                            noise_var=float(noise_var or 0.0), s_min=self.logvar_clamp[0] if gauss else 0.0,
                            s_max=self.logvar_clamp[1] if gauss else 0.0, q=_p(res.quantiles), ld_q=D, plane_stride=R * D)
        for j, v in enumerate(p32):
            a.p[j] = v
        count = None
        if targets is not None:
            targets = targets.contiguous()     # (the helper's own copy is local to it; a no-op on a contiguous tensor)
            res.pit = torch.empty(R, D, dtype=torch.float32, device=self.device)
            res.row_le = torch.empty(R, Q, dtype=torch.int32, device=self.device)
            count = torch.zeros(Q, dtype=torch.int64, device=self.device)
            a.target, a.ld_t, a.pit, a.ld_pit, a.row_le, a.count_le = _p(targets), D, _p(res.pit), D, _p(res.row_le), _p(count)
        L.check(lib.vbnn_predict_quantiles(ctx, C.byref(a)))
        if count is not None:
            res.count_le = count.cpu().tolist()                          # (synchronises)
            res.calibration = [c / (R * D) for c in res.count_le]
        return res

    # ---- the class-probability predictive for any class count (vbnn_predict_class_moments): predict()'s contract, buffers and
    # result, by predict_regression's route -- the final Linear as _generic_head runs it (f32 logits), then the moments of the
    # family over the S draws' log-softmaxes -- with the top-K classes. Nothing of the training step is written.
    @_ordered
    def predict_classes(self, inputs, S=None, targets=None, map=False, row0=None, topk=0, keep_probs=True, keep_draws=False):
        """predict() for any n_classes >= 2: p(y | x, D) ~ 1/S sum_s softmax(f_s(x)) over draws self.draw + 1 .. self.draw + S,
        which `self.draw` advances by; S, targets, map and row0 as predict(). topk = K (0 .. 8, at most n_classes): the K most
        probable classes per row and their probabilities, with targets the top-K accuracy. keep_probs=False: the R x C
        matrices are not stored (probs / log_probs None) -- the per-row uncertainties, pred and the top K only. keep_draws: the
        S x R x C logits are returned too. Returns a PredictResult of this rank's rows (no collective, as test())."""
        lib, ctx = L.lib(), self.ctx.h
        Cn = self.n_classes
        _refuse_bce("predict_classes", self.criterion)
        if self.criterion != "nll":
            raise ValueError(f"predict_classes: a class-probability predictive needs the NLL criterion (criterion = "
                             f"'{self.criterion}' has none: use predict_regression)")
        K = _check_topk("predict_classes", topk, Cn)
        targets = _check_class_targets("predict_classes", targets, inputs.shape[0])     # (before the plan, as predict)
        p = self._predictive_plan("predict_classes", inputs, S, map, row0)
        one_call = p.stacked and Cn <= L.CLASS_MOMENTS_STACKED_MAX_C     # else: ACCUMULATE per draw
        res, a, totals, point, _state = self._class_moments_plan(p.R, p.S, p.Rc, p.n_chunks, one_call, targets, K, keep_probs)
        if keep_draws:
            res.draws = torch.empty(p.S, p.R, Cn, dtype=torch.float32, device=self.device)
        self._moments_loop(p, Cn, res.draws, keep_draws, one_call, a,
                           lambda: L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a))), point)
        self._consume_draws(p.S, p.map)
        self._class_moments_finish(res, totals, p.R, p.S, K)
        return _stamp(res, p.S, p.stacked, p.n_chunks)

    # ---- the Bernoulli criterion's posterior predictive (vbnn_predict_label_moments): predict_regression's contract, buffers and
    # route -- the final Linear as _generic_head runs it (f32 logits), then the moments of the family over the S draws'
    # sigmoids -- with the per-label uncertainties. Nothing of the training step is written.
    @_ordered
    def predict_labels(self, inputs, S=None, targets=None, map=False, row0=None, keep_draws=False):
        """p(y_d = 1 | x, D) ~ 1/S sum_s sigmoid(f_s(x)_d) per label over draws self.draw + 1 .. self.draw + S, with the per-label
        entropy and mutual information (BALD per label); S, map and row0 as predict(), and `self.draw` advances by S likewise.
        targets: R x D fp32 labels in [0, 1] (D = n_classes). keep_draws: the S x R x D logits are returned too. Chunked by
        opt.predict_rows; pruned, compressed, compact and held-mask networks and WN (sequential) as predict_regression. Returns a
        LabelPredictResult of this rank's rows (no collective, as test())."""
        lib, ctx = L.lib(), self.ctx.h
        what = "predict_labels"
        if self.criterion != "bce":
            raise ValueError(f"{what}: the multi-label predictive needs the Bernoulli criterion (criterion = '{self.criterion}': use "
                             + ("predict_regression)" if self.criterion in ("mse", "gauss") else "predict or predict_classes)"))
        D = self.n_classes
        targets = _check_regression_targets(what, targets, inputs.shape[0], D)       # (R x D fp32; before the plan, as predict)
        p = self._predictive_plan(what, inputs, S, map, row0)
        R, S = p.R, p.S
        f32 = dict(dtype=torch.float32, device=self.device)
        has_t = targets is not None
        res = LabelPredictResult(torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, **f32),
                                 torch.empty(R, **f32))
        if has_t:
            res.row_log_lik, res.row_marg_log_lik = torch.empty(R, **f32), torch.empty(R, **f32)
            res.row_hits = torch.empty(R, dtype=torch.int32, device=self.device)
        if keep_draws:
            res.draws = torch.empty(S, R, D, **f32)
        one_call = p.stacked and D <= L.LABEL_MOMENTS_STACKED_MAX_D          # else: ACCUMULATE per draw
        state = None if one_call else torch.empty(p.Rc, 3 * D + 2, **f32)
        totals = torch.zeros(p.n_chunks, 5, dtype=torch.float64, device=self.device) if has_t else None
        a = L.LabelMomentsArgs(ld_y=D, ld_t=D, D=D, S=S, form=L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE,
                               state=_p(state), ld_out=D)

        def point(c0, rows):                   # the chunk's targets and outputs
            a.R = rows
            a.target = _off(targets, c0 * D)
            a.totals = _p(totals[c0 // p.Rc]) if has_t else None
            a.probs, a.entropy, a.mutual_info = _off(res.probs, c0 * D), _off(res.entropy, c0 * D), _off(res.mutual_info, c0 * D)
            a.row_entropy, a.row_mutual_info = _off(res.row_entropy, c0), _off(res.row_mutual_info, c0)
            a.row_log_lik, a.row_marg_log_lik = _off(res.row_log_lik, c0), _off(res.row_marg_log_lik, c0)
            a.row_hits = _off(res.row_hits, c0)

        self._moments_loop(p, D, res.draws, keep_draws, one_call, a,
                           lambda: L.check(lib.vbnn_predict_label_moments(ctx, C.byref(a))), point)
        self._consume_draws(S, p.map)
        if has_t:
            tot = _chunk_sums(totals)
            res.totals = tot
            res.log_lik, res.marg_log_lik = tot[0] / R, tot[1] / R
            res.mean_draw_bce = tot[2] / (R * S * D)
            res.label_accuracy, res.exact_match = 100.0 * tot[3] / (R * D), 100.0 * tot[4] / R
        return _stamp(res, S, p.stacked, p.n_chunks)

    def _class_moments_plan(self, R, S, Rc, n_chunks, one_call, targets, K, keep_probs):
        """What predict_classes and predict_analytic set up for vbnn_predict_class_moments over R rows in n_chunks chunks of Rc:
        the PredictResult with its output tensors, the argument block, the chunks' totals, point(c0, rows), which aims the
        block at a chunk (y / draw are the caller's), and the ACCUMULATE form's state."""
        Cn = self.n_classes
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        has_t = targets is not None
        res = PredictResult(torch.empty(R, Cn, **f32) if keep_probs else None, torch.empty(R, Cn, **f32) if keep_probs else None,
                            torch.empty(R, **f32), torch.empty(R, **f32), torch.empty(R, **f32), torch.empty(R, **i32))
        if K:
            res.topk_idx, res.topk_prob = torch.empty(R, K, **i32), torch.empty(R, K, **f32)
        ld_state = (Cn + 3 + 3) // 4 * 4                                 # a multiple of 4: every row of the state on the 16-byte path
        state = None if one_call else torch.empty(Rc, ld_state, **f32)
        totals = torch.zeros(n_chunks, 5, dtype=torch.float64, device=self.device) if has_t else None
        a = L.ClassMomentsArgs(ld_y=Cn, C=Cn, S=S, form=L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE, K=K,
                               state=_p(state), ld_state=ld_state, ld_out=Cn)

        def point(c0, rows):                   # the chunk's targets and outputs
            a.R = rows
            a.target = _off(targets, c0)
            a.totals = _p(totals[c0 // Rc]) if has_t else None
            a.probs, a.log_probs = _off(res.probs, c0 * Cn), _off(res.log_probs, c0 * Cn)
            a.entropy, a.expected_entropy, a.mutual_info = _off(res.entropy, c0), _off(res.expected_entropy, c0), _off(res.mutual_info, c0)
            a.pred, a.topk_idx, a.topk_prob = _off(res.pred, c0), _off(res.topk_idx, c0 * K), _off(res.topk_prob, c0 * K)

        return res, a, totals, point, state          # (state: the caller keeps it alive across its launches)

    @staticmethod
    def _class_moments_finish(res, totals, R, S, K):
        """The Python floats of a class predictive from the chunks' totals (synchronises); nothing without targets."""
        if totals is None:
            return
        tot = _chunk_sums(totals)
        res.totals = tot
        res.nll, res.accuracy = tot[0] / R, 100.0 * tot[1] / R
        res.mean_draw_nll, res.mean_draw_accuracy = tot[2] / (R * S), 100.0 * tot[3] / (R * S)
        res.topk_accuracy = 100.0 * tot[4] / R if K else None

    def _moments_loop(self, p, Wd, draws, keep_draws, one_call, a, call, point):
        """The chunk loop predict_regression and predict_classes share: per chunk the forward (every draw stacked, or one draw
        at a time), the final Linear's f32 outputs (Wd wide) into the y buffer kept with the predict buffers -- or straight
        into `draws` (S x R x Wd) where keep_draws allows -- and the moments of the family over them: `call()` launches the
        entry point on `a` (its y / draw set here) after `point(c0, rows)` has aimed it at the chunk; one STACKED call
        (one_call), or a call per draw on the running state."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        S, bufs = p.S, p.bufs
        direct = keep_draws and (not p.stacked or p.n_chunks == 1)  # the final Linear writes into draws itself
        if not direct and (bufs.y_reg is None or tuple(bufs.y_reg.shape) != (p.op_rows, Wd)):     # the y buffer: kept with the predict buffers
            bufs.y_reg = torch.empty(p.op_rows, Wd, dtype=torch.float32, device=self.device)
        ybuf = None if direct else bufs.y_reg

        def final_linear(N, y_ptr):
            _gemm(lib, ctx, code, self.w3_s, bufs[len(self.vb)].x, N, self.sizes[-1], Wd, _p(self.bias3), y_ptr, Wd)

        for _, c0, rows, xc in self._chunks(p):
            point(c0, rows)
            if p.stacked:                      # every draw in one forward: draw s = rows [s rows, (s+1) rows) of y
                self._draw_forward(p, xc, rows, c0)
                y = draws if direct else ybuf
                final_linear(S * rows, _p(y))
                if one_call:
                    a.y = _p(y)
                    call()
                else:
                    for s in range(S):
                        a.y, a.draw = _off(y, s * rows * Wd), s
                        call()
                if keep_draws and not direct:
                    draws[:, c0:c0 + rows].copy_(ybuf[:S * rows].view(S, rows, Wd))
                continue
            for s in range(S):                 # one draw per forward, the running moments in `state` between the launches
                self._draw_forward(p, xc, rows, c0, s)
                yp = _off(draws, (s * p.R + c0) * Wd) if direct else _p(ybuf)
                final_linear(rows, yp)
                a.y, a.draw = yp, s
                call()

    # ---- predict's forward under a compressed pruned view (csrc/sparse.hip; pruning.py: _compress): K-major activations from layer to
    # layer (xT from the input packer, hT from every layer but the last, which writes the row-major h the head reads), squares in registers.
    def _sparse_buffers(self, rows):
        """K-major operands of the sparse forward: T[0] the packed input's transpose, T[li + 1] layer li's hT (ping-pong per
        hidden width, as _predict_buffers). Kept across calls while the row count holds."""
        if self._sparse_key != rows:
            T = self._pingpong(len(self.vb) - 1, lambda cols: _Packed(cols, rows, self.tdt, self.device))
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

    # ---- the sampling-free predictive (csrc/propagate.hip): ONE pass that carries the mean, the second moment
    # and the variance of every activation through the network -- per hidden layer three single GEMMs of vbnn_forward (a mu^T + b,
    # q (sigma^2)^T, c (mu^2)^T) and vbnn_relu_moments, then the final Linear's a w3^T + b3 and c (w3^2)^T -- on buffers of its own.
    # Exact for one VB layer; with more, unit correlations are dropped and pre-activations taken as Gaussian.
    @_ordered
    def predict_analytic(self, inputs, targets=None, noise_var=None, S=None, row0=None, topk=0, keep_probs=True):
        """The posterior predictive WITHOUT Monte-Carlo forwards: the network runs once, on moments.
        criterion = "mse": a RegressionPredictResult with predict_regression's fields -- mean (the propagated output mean), var
        (the propagated epistemic variance), row_var; with targets (R x D) row_sq_err, mse, mean_var and mean_draw_mse (its
        expectation under the propagated Gaussian, mse + mean_var); with noise_var (tau^2 > 0) row_log_lik / log_lik of
        N(mean, var + tau^2) per output -- ONE Gaussian, not predict_regression's mixture over draws. draws is None, S = 0, no
        draw is consumed and two calls agree bit for bit. The row sums and the log-likelihood are torch operations on the R x D
        outputs (no kernel of the library: they are a few R x D elementwise passes beside the network's GEMMs).
        criterion = "nll" (any class count): the logit mean and variance are sampled S times (default opt.testSamples; draws
        self.draw + 1 .. self.draw + S of the final Linear's own noise stream, rows addressed from row0 as predict) by
        vbnn_logit_draws and finished by vbnn_predict_class_moments: a PredictResult with predict_classes' fields (topk,
        keep_probs), plus logit_mean / logit_var (R x C) and, with keep_probs, draws (the S x R x C sampled logits; without, they
        stay in a per-chunk buffer). `self.draw` advances by S (host and device counter). Only R x C logits are sampled; the logits are taken as independent Gaussians.
        criterion = "gauss" is refused (the clamp on the log variance makes its moments a separate piece of work). Both modes;
        dense pruned views, held masks and compact networks work through the operand shadows; compressed views are refused.
        Chunked by opt.predict_rows. Returns this rank's rows (no collective)."""
        what = "predict_analytic"
        _refuse_bce(what, self.criterion)      # (the moments of sigmoid(z) under a Gaussian logit are a follow-up)
        if self.criterion == "gauss":
            raise ValueError(f"{what}: criterion = 'gauss' is not supported -- the clamp on the log variance makes the moments of "
                             "exp(s) a separate piece of work (the follow-up); use predict_regression")
        if isinstance(self._pruned, SparsePruneResult):
            raise ValueError(f"{what}: a compressed pruned view is not supported (use the dense PruneResult it was compressed "
                             "from, or predict / predict_regression)")
        R = inputs.shape[0]
        if self.criterion == "nll":
            if noise_var is not None:
                raise ValueError(f"{what}: noise_var belongs to the regression predictive (criterion = 'nll')")
            K = _check_topk(what, topk, self.n_classes)
            S = _check_draws(what, int(self.opt["testSamples"] if S is None else S))
            return self._analytic_classes(what, inputs, _check_class_targets(what, targets, R), S, row0, K, keep_probs)
        if int(topk):
            raise ValueError(f"{what}: topk belongs to the class predictive (criterion = 'mse')")
        if S is not None or row0 is not None:
            raise ValueError(f"{what}: S and row0 address the class predictive's logit draws (criterion = 'mse' draws nothing)")
        noise_var = _check_noise_var(what, noise_var)
        return self._analytic_regression(what, inputs, _check_regression_targets(what, targets, R, self.n_classes), noise_var)

    def _analytic_plan(self, what, inputs, row0):
        """predict_analytic's plan: _predictive_inputs, the chunks (Rc rows each: nothing is stacked), the squared operands and the
        buffers of its own -- none of predict's."""
        x, R, row0 = self._predictive_inputs(what, inputs, row0)
        ops = self._analytic_operands()
        Rc = max(1, min(R, int(self.opt.get("predict_rows", 32768))))
        return types.SimpleNamespace(x=x, R=R, row0=row0, Rc=Rc, n_chunks=(R + Rc - 1) // Rc, ops=ops, B=self._analytic_buffers(Rc))

    def _propagate(self, B, ops, xc, rows, mean_ptr, var_ptr):
        """The chunk's output mean and variance (rows x n_classes fp32 each) from its inputs xc: the moments through every layer."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        nl, gemm = len(self.vb), functools.partial(_gemm, lib, ctx, code)
        b0 = B.act[0]
        L.check(lib.vbnn_pack_input(ctx, code, _p(xc), xc.stride(0), rows, self.sizes[0], b0.a.ptr, b0.q.ptr, b0.a.ld,
                                    None, None, 0, 0))
        for li, v in enumerate(self.vb):
            xin, out, ld = B.act[li], B.act[li + 1], L.pad_ld(v.O)
            gemm(ops.mu[li], xin.a, rows, v.I, v.O, _p(v.bias), _p(B.m), ld)
            gemm(ops.var[li], xin.q, rows, v.I, v.O, None, _p(B.v1), ld)
            if li > 0:                                           # (the first layer's input is deterministic: c = 0)
                gemm(ops.mu2[li], xin.c, rows, v.I, v.O, None, _p(B.v2), ld)
            ra = L.ReluMomentsArgs(m=_p(B.m), ld_m=ld, v1=_p(B.v1), v2=_p(B.v2) if li > 0 else None, ld_v=ld, N=rows, O=v.O,
                                   a=out.a.ptr, q=out.q.ptr if li < nl - 1 else None, c=out.c.ptr, ld_out=out.a.ld)
            L.check(lib.vbnn_relu_moments(ctx, code, C.byref(ra)))
        H, Wd = self.sizes[-1], self.n_classes
        gemm(self.w3_s, B.act[nl].a, rows, H, Wd, _p(self.bias3), mean_ptr, Wd)
        gemm(ops.w3sq, B.act[nl].c, rows, H, Wd, None, var_ptr, Wd)

    def _analytic_regression(self, what, inputs, targets, noise_var):
        """predict_analytic, criterion "mse": the propagated mean and variance, finished with torch on the R x D outputs."""
        p = self._analytic_plan(what, inputs, None)
        R, Wd = p.R, self.n_classes
        f32 = dict(dtype=torch.float32, device=self.device)
        res = RegressionPredictResult(torch.empty(R, Wd, **f32), torch.empty(R, Wd, **f32), None, None, None, None)
        for _, c0, rows, xc in self._chunks(p):
            self._propagate(p.B, p.ops, xc, rows, _off(res.mean, c0 * Wd), _off(res.var, c0 * Wd))
        res.row_var = res.var.mean(dim=1)
        if targets is not None:
            d2 = (targets - res.mean) ** 2
            res.row_sq_err = d2.sum(dim=1)
            if noise_var is not None:
                tv = res.var + noise_var
                res.row_log_lik = (-0.5 * (torch.log(6.2831855 * tv) + d2 / tv)).sum(dim=1)
            sq, vs = float(res.row_sq_err.double().sum()), float(res.var.double().sum())
            ll = float(res.row_log_lik.double().sum()) if noise_var is not None else 0.0
            res.totals = [sq, sq + vs, ll, vs]
            res.mse, res.mean_var = sq / (R * Wd), vs / (R * Wd)
            res.mean_draw_mse = (sq + vs) / (R * Wd)
            res.log_lik = ll / R if noise_var is not None else None
        return _stamp(res, 0, None, p.n_chunks)

    def _analytic_classes(self, what, inputs, targets, S, row0, K, keep_probs):
        """predict_analytic, criterion "nll": S draws of the propagated logit distribution (vbnn_logit_draws), finished as
        predict_classes finishes its forwards' logits (vbnn_predict_class_moments)."""
        lib, ctx = L.lib(), self.ctx.h
        p = self._analytic_plan(what, inputs, row0)
        R, Wd, B = p.R, self.n_classes, p.B
        f32 = dict(dtype=torch.float32, device=self.device)
        # keep_probs: the draws are returned, written straight into the S x R x C result (one chunk: one STACKED call; more: a call
        # per draw, each read in place). Otherwise they live in the chunk's own S x rows x C buffer, kept with the other buffers.
        stacked = (p.n_chunks == 1 or not keep_probs) and Wd <= L.CLASS_MOMENTS_STACKED_MAX_C
        res, a, totals, point, _state = self._class_moments_plan(R, S, p.Rc, p.n_chunks, stacked, targets, K, keep_probs)
        res.logit_mean, res.logit_var = torch.empty(R, Wd, **f32), torch.empty(R, Wd, **f32)
        if keep_probs:
            res.draws = torch.empty(S, R, Wd, **f32)
        elif B.y is None or B.y.numel() != S * p.Rc * Wd:
            B.y = torch.empty(S * p.Rc * Wd, **f32)
        d0 = self.draw + 1
        for _, c0, rows, xc in self._chunks(p):
            mp, vp = _off(res.logit_mean, c0 * Wd), _off(res.logit_var, c0 * Wd)
            self._propagate(B, p.ops, xc, rows, mp, vp)
            y0, stride = (_off(res.draws, c0 * Wd), R * Wd) if keep_probs else (_p(B.y), rows * Wd)
            da = L.LogitDrawsArgs(m=mp, ld_m=Wd, v=vp, ld_v=Wd, R=rows, C=Wd, S=S, seed=self.seed, layer=len(self.vb), draw=d0,
                                  row0=p.row0 + c0, y=y0, ld_y=Wd, draw_stride=stride)
            L.check(lib.vbnn_logit_draws(ctx, C.byref(da)))
            point(c0, rows)
            if stacked:
                a.y = y0
                L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a)))
            else:
                for s in range(S):
                    a.y, a.draw = C.c_void_p(y0.value + 4 * s * stride), s
                    L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a)))
        self._consume_draws(S, False)
        self._class_moments_finish(res, totals, R, S, K)
        return _stamp(res, S, False, p.n_chunks)

    def _analytic_operands(self):
        """predict_analytic's weight-side operands: mu and sigma^2 as the predictive reads them -- the pruned view's shadows, the
        operand shadows (LRT: a held mask's +0 entries included), or packed here from means / lvars (WN, whose prepare packs
        none) -- and mu^2 and w3^2 squared from them AS THEY ARE (vbnn_square_shadow). Rebuilt when the parameter version or the
        pruned view changes, and after a graph replay (a captured update() changes the shadows without a new version); kept otherwise."""
        key = (self._pver, self._pruned)
        st = self._ana_ops
        if st is not None and st.key[0] == key[0] and st.key[1] is key[1] and not self._ana_ops_stale:
            return st
        self._ana_ops_stale = False
        lib, ctx, code, dev = L.lib(), self.ctx.h, self.code, self.device
        st = st or types.SimpleNamespace(mu2=[_Packed(v.O, v.I, self.tdt, dev) for v in self.vb], own=None,
                                         w3sq=_Packed(self.n_classes, self.sizes[-1], self.tdt, dev))
        pv = self._pruned
        if pv is not None:
            st.mu, st.var = list(pv.mu_p), list(pv.var_p)
        elif self.mode == "lrt":
            st.mu, st.var = [v.mu_s for v in self.vb], [v.var_s for v in self.vb]
        else:                                  # weight noise: the shadows of means and exp(lvars), packed on demand
            if st.own is None:
                st.own = [(_Packed(v.O, v.I, self.tdt, dev), _Packed(v.O, v.I, self.tdt, dev)) for v in self.vb]
            for v, (m_s, v_s) in zip(self.vb, st.own):
                L.check(lib.vbnn_pack(ctx, code, L.PACK_COPY, _p(v.means), None, v.I, v.O, v.I, m_s.ptr, m_s.ld, None, 0))
                L.check(lib.vbnn_pack(ctx, code, L.PACK_EXP, _p(v.lvars), None, v.I, v.O, v.I, v_s.ptr, v_s.ld, None, 0))
            st.mu, st.var = [o[0] for o in st.own], [o[1] for o in st.own]
        for v, mu, mu2 in zip(self.vb, st.mu, st.mu2):
            L.check(lib.vbnn_square_shadow(ctx, code, mu.ptr, mu.ld, v.O, v.I, mu2.ptr, mu2.ld))
        L.check(lib.vbnn_square_shadow(ctx, code, self.w3_s.ptr, self.w3_s.ld, self.n_classes, self.sizes[-1], st.w3sq.ptr, st.w3sq.ld))
        st.key = key
        self._ana_ops = st
        return st

    def _analytic_buffers(self, rows):
        """predict_analytic's own buffers for `rows` operand rows: act[li] = layer li's input moments (a, q, c packed; act[0] the
        packed input and its square), one ping-pong pair per hidden width as _predict_buffers; m, v1, v2: the three products'
        fp32 outputs (rows x the widest padded layer). Kept across calls while the row count holds."""
        st = self._ana_bufs
        if st is not None and st.rows == rows:
            return st
        dev, tdt, nl = self.device, self.tdt, len(self.vb)
        act = self._pingpong(nl, lambda cols: types.SimpleNamespace(a=_Packed(rows, cols, tdt, dev), q=None, c=None))
        for j, b in enumerate(act):                              # q: what a VB layer reads of its input; c: what a layer writes
            if j < nl:
                b.q = b.q or _Packed(rows, b.a.cols, tdt, dev)
            if j > 0:
                b.c = b.c or _Packed(rows, b.a.cols, tdt, dev)
        wide = rows * max(L.pad_ld(v.O) for v in self.vb)
        f32 = dict(dtype=torch.float32, device=dev)
        st = types.SimpleNamespace(rows=rows, act=act, m=torch.zeros(wide, **f32), v1=torch.zeros(wide, **f32), v2=torch.zeros(wide, **f32),
                                   y=None)                  # (y: the class predictive's S x rows x C logit draws, on first use)
        self._ana_bufs = st
        return st
