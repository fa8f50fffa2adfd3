"""Pruning for the fused engine (a mixin of vbnn_amd/engine.py:FusedMLP): weights by signal-to-noise (mainviz.lua:20-27) with the pruned
view predict() reads and its compressed form, whole hidden units with the compact engine that is left, a mask held through training."""
import contextlib
import ctypes as C
import math

import torch

from . import _lib as L
from .nn import _Packed, _ordered, _p


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


class _Pruning:
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

    def prune_curve(self, inputs, targets, fractions, S=None, map=False, scope="global", compress=False):
        """What pruning costs: for every fraction q a prune(fraction=q, scope=scope) and a predict(inputs, S, targets, map)
        under that view. One dict per fraction: fraction, tau (per layer), n_pruned, nll, accuracy, mean_draw_nll,
        mean_draw_accuracy, mutual_info (mean over rows). The keys are re-formed by every select and pack sweep (nothing per
        weight is kept between the points). Each point consumes S draws as a predict() call of its own would (none with
        map=True), so the points see different noise; the engine's view is afterwards what it was before.
        compress: every point is evaluated through the compressed form (prune(...).compress() as the view) and also carries
        nnz, nbytes and dense_nbytes."""
        rows = []
        for q in fractions:
            res = self.prune(fraction=q, scope=scope)
            res = res.compress() if compress else res
            extra = dict(nnz=sum(res.nnz), nbytes=res.nbytes, dense_nbytes=res.dense_nbytes) if compress else {}
            with self.pruned(res):
                p = self.predict(inputs, S=S, targets=targets, map=map)
            rows.append(dict(fraction=float(q), tau=res.tau, n_pruned=res.n_pruned, **extra, nll=p.nll, accuracy=p.accuracy,
                             mean_draw_nll=p.mean_draw_nll, mean_draw_accuracy=p.mean_draw_accuracy,
                             mutual_info=float(p.mutual_info.mean().item())))
        return rows

    def prune_curve_sparse(self, inputs, targets, fractions, S=None, map=False, scope="global"):
        """prune_curve(..., compress=True)."""
        return self.prune_curve(inputs, targets, fractions, S=S, map=map, scope=scope, compress=True)

    # ---- the compressed pruned view (csrc/sparse.hip; its forward: predictive.py). compress: a PruneResult's kept weights as CSR, built on
    # the device at the result's own tau (the entry count is known from its statistics: no extra synchronisation before the allocation).
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
        from .engine import FusedMLP                      # (engine.py imports this module)
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
