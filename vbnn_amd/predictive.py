"""The posterior predictives of the fused engine (FusedMLP.predict / predict_classes / predict_regression / predict_quantiles):
forward-only passes on buffers of their own, dense or under a pruned view (pruning.py). A mixin of vbnn_amd/engine.py:FusedMLP."""
import ctypes as C
import math
import types

import torch

from . import _lib as L
from .nn import _Packed, _VB, _ordered, _p
from .pruning import SparsePruneResult


def _off(t, row):
    """The address of element `row` of t (4-byte elements), None without t."""
    return C.c_void_p(t.data_ptr() + 4 * row) if t is not None else None


def _chunk_sums(totals):
    """The chunks' totals (chunks x NT doubles on the device) added in chunk order; synchronises."""
    return [sum(col) for col in zip(*totals.cpu().tolist())]


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
    among them); with keep_draws, draws (S x R x C: every draw's logits). totals: the library's sums."""

    def __init__(self, probs, log_probs, entropy, expected_entropy, mutual_info, pred):
        self.probs, self.log_probs, self.entropy = probs, log_probs, entropy
        self.expected_entropy, self.mutual_info, self.pred = expected_entropy, mutual_info, pred
        self.nll = self.accuracy = self.mean_draw_nll = self.mean_draw_accuracy = None
        self.totals = self.topk_idx = self.topk_prob = self.topk_accuracy = self.draws = None
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
    def _predictive_plan(self, what, inputs, S, map, row0, max_S=None):
        """What predict and predict_regression (`what`, for the messages) share ahead of their chunk loops: resolves S / map,
        checks the inputs, prepares a fresh engine, checks the pruned view and decides the pass -- x (R rows), S, map, row0, lrt,
        stacked, Rc minibatch rows per chunk (n_chunks of them, op_rows operand rows each), the buffers, WN's weights, d0."""
        map = bool(map or self.opt.get("quicktest"))
        S = 1 if map else int(self.opt["testSamples"] if S is None else S)
        if S < 1:
            raise ValueError(f"{what}: S = {S} draws (at least one)")
        if max_S is not None and S > max_S:
            raise ValueError(f"{what}: S = {S} draws (at most {max_S})")
        x = inputs.reshape(inputs.shape[0], -1)
        R = x.shape[0]
        assert x.shape[1] == self.sizes[0] and x.dtype == torch.float32 and x.is_cuda and R > 0
        row0 = self.rank * R if row0 is None else int(row0)
        if not self._shadows_ready:            # a fresh engine: the shadows test() would have prepared
            self.prepare()
        if self._pruned is not None:           # a pruned view replaces the operand shadows: it must be of THESE parameters
            if self.mode == "wn" and not map:
                raise ValueError(f"{what}: weight-noise draws under a pruned view are not supported -- they sample from the fp32 "
                                 "means / lvars, which the view does not replace (use map=True, or mode = 'lrt')")
            if self._pruned.version != self._pver:
                raise RuntimeError(f"{what}: the pruned view was taken from older parameters (update / prepare / init_parameters "
                                   "ran since): prune() again, or use_pruned(None)")
        lrt = self.mode == "lrt" and not map
        stacked = self._predict_stacked(R, S, lrt)
        cap = max(1, int(self.opt.get("predict_rows", 32768)))
        Rc = max(1, min(R, cap // S if stacked else cap))           # minibatch rows per chunk: S Rc (stacked) or Rc operand rows
        op_rows = S * Rc if stacked else Rc
        return types.SimpleNamespace(x=x, R=R, S=S, map=map, row0=row0, lrt=lrt, stacked=stacked, Rc=Rc, n_chunks=(R + Rc - 1) // Rc,
                                     op_rows=op_rows, bufs=self._predict_buffers(op_rows, lrt),
                                     wts=self._predict_weights() if self.mode == "wn" else None, d0=self.draw + 1)   # (d0: draw 1's counter)

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
        if Cn > 16:
            raise ValueError(f"predict: the predictive head takes at most 16 classes (n_classes = {Cn})")
        if self.criterion != "nll":
            raise ValueError(f"predict: a class-probability predictive needs the NLL criterion (criterion = '{self.criterion}' has "
                             "none: use predict_regression)")
        if targets is not None:                # (before the plan: nothing is prepared or allocated for a refused call)
            assert targets.dtype == torch.int32 and targets.is_cuda and targets.numel() == inputs.shape[0]
            targets = targets.contiguous()
        p = self._predictive_plan("predict", inputs, S, map, row0)
        x, R, S, map, row0, lrt = p.x, p.R, p.S, p.map, p.row0, p.lrt
        stacked, Rc, n_chunks, bufs, wts, d0 = p.stacked, p.Rc, p.n_chunks, p.bufs, p.wts, p.d0
        f32 = dict(dtype=torch.float32, device=self.device)
        res = PredictResult(torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32), torch.empty(R, **f32), torch.empty(R, **f32),
                            torch.empty(R, **f32), torch.empty(R, dtype=torch.int32, device=self.device))
        totals = torch.zeros(n_chunks, 4, dtype=torch.float64, device=self.device) if targets is not None else None
        state = torch.empty(Rc, Cn + 3, **f32) if not stacked else None
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
        self._consume_draws(S, map)
        if totals is not None:
            tot = _chunk_sums(totals)
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
        if self._pred_key != key:
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
        if self.criterion not in ("mse", "gauss"):
            raise ValueError(f"{what}: the regression predictive needs the MSE criterion or the Gaussian one "
                             "(criterion = 'nll': use predict)")
        gauss = self.criterion == "gauss"
        Wd = self.n_classes                                          # the final Linear's width: D, or { m[D], s[D] }
        D = Wd // 2 if gauss else Wd
        if gauss and noise_var is not None:
            raise ValueError(f"{what}: criterion = 'gauss' predicts its own noise variance (noise_var must be None)")
        if noise_var is not None:
            noise_var = float(noise_var)
            if not (noise_var > 0.0 and math.isfinite(noise_var)):
                raise ValueError(f"{what}: noise_var = {noise_var} (a finite variance above zero, or None)")
        if targets is not None:                # (before the plan, as predict)
            R = inputs.shape[0]
            if gauss and tuple(targets.shape) != (R, D):
                raise ValueError(f"{what}: targets of shape {tuple(targets.shape)} (criterion = 'gauss' takes R x D = "
                                 f"{R} x {D}: one target per mean)")
            assert targets.dtype == torch.float32 and targets.is_cuda and tuple(targets.shape) == (R, D)
            targets = targets.contiguous()
        p = self._predictive_plan(what, inputs, S, map, row0, max_S)
        R, S, map, stacked, Rc, n_chunks = p.R, p.S, p.map, p.stacked, p.Rc, p.n_chunks
        f32 = dict(dtype=torch.float32, device=self.device)
        has_t = targets is not None
        res = RegressionPredictResult(torch.empty(R, D, **f32), torch.empty(R, D, **f32), torch.empty(R, **f32),
                                      torch.empty(R, **f32) if has_t else None,
                                      torch.empty(R, **f32) if (has_t and (gauss or noise_var is not None)) else None,
                                      torch.empty(S, R, Wd, **f32) if keep_draws else None)
        if gauss:
            res.noise_var, res.row_noise_var = torch.empty(R, D, **f32), torch.empty(R, **f32)
        one_call = stacked and D <= (L.GAUSS_MOMENTS_STACKED_MAX_D if gauss else L.MOMENTS_STACKED_MAX_D)   # else: ACCUMULATE per draw
        state = None if one_call else torch.empty(Rc, (3 if gauss else 2) * D + 2, **f32)
        totals = torch.zeros(n_chunks, 5 if gauss else 4, dtype=torch.float64, device=self.device) if has_t else None
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
            a.totals = C.c_void_p(totals[c0 // Rc].data_ptr()) if has_t else None
            a.mean, a.var = _off(res.mean, c0 * D), _off(res.var, c0 * D)
            a.row_var, a.row_sq_err, a.row_log_lik = _off(res.row_var, c0), _off(res.row_sq_err, c0), _off(res.row_log_lik, c0)
            if gauss:
                a.noise_var, a.row_noise_var = _off(res.noise_var, c0 * D), _off(res.row_noise_var, c0)

        self._moments_loop(p, Wd, res.draws, keep_draws, one_call, a, lambda: L.check(moments(ctx, C.byref(a))), point)
        self._consume_draws(S, map)
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
        res.S, res.stacked, res.chunks = S, stacked, n_chunks
        return res

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
        Cn, K = self.n_classes, int(topk)
        if self.criterion != "nll":
            raise ValueError(f"predict_classes: a class-probability predictive needs the NLL criterion (criterion = "
                             f"'{self.criterion}' has none: use predict_regression)")
        if not 0 <= K <= min(L.CLASS_MOMENTS_MAX_K, Cn):
            raise ValueError(f"predict_classes: topk = {K} (0 .. {L.CLASS_MOMENTS_MAX_K}, and at most n_classes = {Cn})")
        if targets is not None:                # (before the plan, as predict)
            assert targets.dtype == torch.int32 and targets.is_cuda and targets.numel() == inputs.shape[0]
            targets = targets.contiguous()
        p = self._predictive_plan("predict_classes", inputs, S, map, row0)
        R, S, map, stacked, Rc, n_chunks = p.R, p.S, p.map, p.stacked, p.Rc, p.n_chunks
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        has_t = targets is not None
        res = PredictResult(torch.empty(R, Cn, **f32) if keep_probs else None, torch.empty(R, Cn, **f32) if keep_probs else None,
                            torch.empty(R, **f32), torch.empty(R, **f32), torch.empty(R, **f32), torch.empty(R, **i32))
        if K:
            res.topk_idx, res.topk_prob = torch.empty(R, K, **i32), torch.empty(R, K, **f32)
        if keep_draws:
            res.draws = torch.empty(S, R, Cn, **f32)
        one_call = stacked and Cn <= L.CLASS_MOMENTS_STACKED_MAX_C       # else: ACCUMULATE per draw
        ld_state = (Cn + 3 + 3) // 4 * 4                                 # a multiple of 4: every row of the state on the 16-byte path
        state = None if one_call else torch.empty(Rc, ld_state, **f32)
        totals = torch.zeros(n_chunks, 5, dtype=torch.float64, device=self.device) if has_t else None
        a = L.ClassMomentsArgs(ld_y=Cn, C=Cn, S=S, form=L.MOMENTS_STACKED if one_call else L.MOMENTS_ACCUMULATE, K=K,
                               state=_p(state), ld_state=ld_state, ld_out=Cn)

        def point(c0, rows):                   # the chunk's targets and outputs
            a.R = rows
            a.target = _off(targets, c0)
            a.totals = C.c_void_p(totals[c0 // Rc].data_ptr()) if has_t else None
            a.probs, a.log_probs = _off(res.probs, c0 * Cn), _off(res.log_probs, c0 * Cn)
            a.entropy, a.expected_entropy, a.mutual_info = _off(res.entropy, c0), _off(res.expected_entropy, c0), _off(res.mutual_info, c0)
            a.pred, a.topk_idx, a.topk_prob = _off(res.pred, c0), _off(res.topk_idx, c0 * K), _off(res.topk_prob, c0 * K)

        self._moments_loop(p, Cn, res.draws, keep_draws, one_call, a,
                           lambda: L.check(lib.vbnn_predict_class_moments(ctx, C.byref(a))), point)
        self._consume_draws(S, map)
        if has_t:
            tot = _chunk_sums(totals)
            res.totals = tot
            res.nll, res.accuracy = tot[0] / R, 100.0 * tot[1] / R
            res.mean_draw_nll, res.mean_draw_accuracy = tot[2] / (R * S), 100.0 * tot[3] / (R * S)
            res.topk_accuracy = 100.0 * tot[4] / R if K else None
        res.S, res.stacked, res.chunks = S, stacked, n_chunks
        return res

    def _moments_loop(self, p, Wd, draws, keep_draws, one_call, a, call, point):
        """The chunk loop predict_regression and predict_classes share: per chunk the forward (every draw stacked, or one draw
        at a time), the final Linear's f32 outputs (Wd wide) into the y buffer kept with the predict buffers -- or straight
        into `draws` (S x R x Wd) where keep_draws allows -- and the moments of the family over them: `call()` launches the
        entry point on `a` (its y / draw set here) after `point(c0, rows)` has aimed it at the chunk; one STACKED call
        (one_call), or a call per draw on the running state."""
        lib, ctx, code = L.lib(), self.ctx.h, self.code
        x, R, S, map, row0, lrt = p.x, p.R, p.S, p.map, p.row0, p.lrt
        stacked, Rc, n_chunks, op_rows, bufs, wts, d0 = p.stacked, p.Rc, p.n_chunks, p.op_rows, p.bufs, p.wts, p.d0
        nl, H = len(self.vb), self.sizes[-1]
        direct = keep_draws and (not stacked or n_chunks == 1)      # the final Linear writes into draws itself
        ybuf = None
        if not direct:                                               # the y buffer: kept with the predict buffers
            ybuf = bufs.y_reg
            if ybuf is None or tuple(ybuf.shape) != (op_rows, Wd):
                ybuf = bufs.y_reg = torch.empty(op_rows, Wd, dtype=torch.float32, device=self.device)

        def final_linear(N, y_ptr):
            fa = L.FwdArgs(w=self.w3_s.ptr, w2=None, x=bufs[nl].x.ptr, x2=None, ld_w=self.w3_s.ld, ld_x=bufs[nl].x.ld,
                           N=N, I=H, O=Wd, bias=_p(self.bias3), y=y_ptr, ld_y=Wd)
            L.check(lib.vbnn_forward(ctx, code, C.byref(fa)))

        for k in range(n_chunks):
            c0 = k * Rc
            rows = min(Rc, R - c0)
            xc = x[c0:c0 + rows]
            point(c0, rows)
            if stacked:                        # every draw in one forward: draw s = rows [s rows, (s+1) rows) of y
                if wts is not None:
                    self._predict_wn_sample(wts, None if map else d0)
                self._predict_forward(bufs, wts, xc, S * rows, rows if S > 1 else 0, d0, row0 + c0, lrt)
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
                if wts is not None:
                    self._predict_wn_sample(wts, d0 + s)
                self._predict_forward(bufs, wts, xc, rows, 0, d0 + s, row0 + c0, lrt, pack=(s == 0))
                yp = _off(draws, (s * R + c0) * Wd) if direct else _p(ybuf)
                final_linear(rows, yp)
                a.y, a.draw = yp, s
                call()

    # ---- predict's forward under a compressed pruned view (csrc/sparse.hip; pruning.py: _compress): K-major activations from layer to
    # layer (xT from the input packer, hT from every layer but the last, which writes the row-major h the head reads), squares in registers.
    def _sparse_buffers(self, rows):
        """K-major operands of the sparse forward: T[0] the packed input's transpose, T[li + 1] layer li's hT (ping-pong per
        hidden width, as _predict_buffers). Kept across calls while the row count holds."""
        if self._sparse_key != rows:
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
