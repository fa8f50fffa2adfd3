"""FusedMLP's pool acquisition for active learning (the _Acquisition mixin): which k rows of an unlabelled pool to label
next, chosen on the device by vbnn_top_rows (csrc/acquire.hip) from the uncertainty the engine's own predictives report."""
import ctypes as C
import math

import torch

from . import _lib as L
from .nn import _ordered, _p

# the scores each criterion can rank a pool by: the first is the default
SCORES = {
    "nll": ("mutual_info", "entropy", "least_confidence", "margin", "random"),
    "bce": ("mutual_info", "entropy", "random"),
    "mse": ("variance", "random"),
    "gauss": ("variance", "total_variance", "random"),
}


class AcquireResult:
    """FusedMLP.top_rows' / acquire's outcome. Device tensors of k entries: indices (int32: the selected rows, best first, ties
    to the lower row; -1 past n_selected), values (their scores as given; NaN past n_selected; 1 for "random"), keys (what each
    row was ranked by: the score, or the perturbed key of a stochastic selection). Python integers: n_selected, n_candidates,
    n_nan (rows whose score is a NaN: never selected), n_excluded. acquire also sets score_name, S, chunks (the predictive's) and
    predictive (the predictive's own result; None for "random")."""

    def __init__(self, indices, values, keys, counts):
        self.indices, self.values, self.keys = indices, values, keys
        self.n_selected, self.n_candidates, self.n_nan, self.n_excluded = (int(c) for c in counts)
        self.score_name = self.S = self.chunks = self.predictive = None


class SpreadResult:
    """FusedMLP.spread_rows' / acquire_diverse's outcome (vbnn_kcentre). Device tensors: indices (k, int32: the rows in pick
    order; -1 past n_selected), keys (k: what each pick was ranked by -- its distance to the nearest centre, times its weight),
    dists (k: that distance alone; NaN past n_selected), min_dist (R: every row's squared distance to the nearest centre after the
    last pick; NaN for a void row) -- pass the result as state= to continue. Python integers: n_selected, n_candidates, n_void
    (rows whose features or weight are not usable: never selected), n_excluded, n_ignored_centres (centre indices outside the
    matrix). acquire_diverse also sets score_name, S, chunks and predictive (None with weighted=False)."""

    def __init__(self, indices, keys, dists, min_dist, counts, n_ignored_centres=0, exclude=None):
        self.indices, self.keys, self.dists, self.min_dist = indices, keys, dists, min_dist
        self.n_selected, self.n_candidates, self.n_void, self.n_excluded = (int(c) for c in counts)
        self.n_ignored_centres = int(n_ignored_centres)
        self.exclude = exclude                     # uint8, R: what the call excluded plus its own picks (what state= carries on)
        self.score_name = self.S = self.chunks = self.predictive = None


def _check_spread_k(what, k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= L.KCENTRE_MAX_K:
        raise ValueError(f"{what}: k = {k} (an integer in 1 .. {L.KCENTRE_MAX_K}: for more rows continue with state=)")
    return int(k)


def _check_k(what, k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= L.TOP_ROWS_MAX_K:
        raise ValueError(f"{what}: k = {k} (an integer in 1 .. {L.TOP_ROWS_MAX_K}: for more rows select in several calls, "
                         "excluding the rows already taken)")
    return int(k)


def _check_beta(what, beta):
    if beta is None:
        return None
    beta = float(beta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"{what}: beta = {beta} (> 0 and finite; beta=None selects the top k without noise)")
    return beta


def _check_exclude(what, exclude, R, device):
    if exclude is None:
        return None
    if (not torch.is_tensor(exclude) or exclude.dtype not in (torch.uint8, torch.bool) or not exclude.is_cuda
            or exclude.device != device or exclude.dim() != 1 or exclude.numel() != R):
        raise ValueError(f"{what}: exclude is a uint8 or bool device vector of R = {R} entries (non-zero = already labelled)")
    exclude = exclude.contiguous()
    return exclude.view(torch.uint8) if exclude.dtype == torch.bool else exclude


class _Acquisition:
    def _top_rows(self, what, score, R, k, largest, exclude, beta, draw, row0):
        """The one caller of vbnn_top_rows: every argument checked already; score None = every candidate has weight 1."""
        lib, dev = L.lib(), self.device
        ws = getattr(self, "_top_rows_ws", None)
        if ws is None or ws[0] != R:               # kept on the engine and re-used while R holds (its size does not depend on k)
            nbytes = C.c_size_t()
            L.check(lib.vbnn_top_rows_workspace_bytes(R, k, C.byref(nbytes)))
            ws = self._top_rows_ws = (R, torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev))
        index = torch.empty(k, dtype=torch.int32, device=dev)
        value = torch.empty(k, dtype=torch.float32, device=dev)
        key = torch.empty(k, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        a = L.TopRowsArgs(score=_p(score), exclude=_p(exclude), R=R, k=k, largest=int(bool(largest)),
                          stochastic=int(beta is not None), beta=beta or 0.0, seed=self.seed, draw=draw or 0, row0=row0,
                          index=_p(index), value=_p(value), key=_p(key), counts=_p(counts), workspace=_p(ws[1]),
                          workspace_bytes=ws[1].numel() * 8)
        L.check(lib.vbnn_top_rows(self.ctx.h, C.byref(a)))
        return AcquireResult(index, value, key, counts.cpu().tolist())

    @_ordered
    def top_rows(self, score, k, largest=True, exclude=None, beta=None, draw=None, row0=0):
        """The k rows of `score` (an fp32 device vector of R rows: a predictive's entropy, mutual_info, row_var, ...) with the
        largest (largest=False: smallest) scores, exactly: ties go to the lower row, NaN rows are never taken, rows with
        exclude[r] != 0 (a uint8 or bool device vector) are left out. beta=None: deterministic. beta > 0: k rows sampled without
        replacement with probability proportional to score^beta (Gumbel top-k; largest only) from the noise of (opt.seed,
        draw, row0 + r) -- draw=None uses self.draw + 1 and consumes it (host and device counter), so two calls give two
        samples; a draw given is used as it is and nothing is consumed. One call of vbnn_top_rows. Returns an AcquireResult
        (the four counts synchronise; the tensors stay on the device)."""
        what = "top_rows"
        if (not torch.is_tensor(score) or score.dtype != torch.float32 or not score.is_cuda or score.device != self.device
                or score.dim() != 1 or not 1 <= score.numel() < 1 << 31):
            raise ValueError(f"{what}: score is an fp32 device vector of 1 <= R < 2^31 rows")
        R = score.numel()
        k, beta = _check_k(what, k), _check_beta(what, beta)
        exclude = _check_exclude(what, exclude, R, self.device)
        row0 = int(row0)
        if beta is not None:
            if not largest:
                raise ValueError(f"{what}: a stochastic selection (beta) samples in proportion to score^beta: largest=True only "
                                 "(for the smallest scores rank a decreasing function of them)")
            if not 0 <= row0 <= (1 << 32) - R:
                raise ValueError(f"{what}: row0 = {row0} (0 <= row0, row0 + R <= 2^32)")
        consume = beta is not None and draw is None
        d = 0 if beta is None else (self.draw + 1 if draw is None else int(draw))
        res = self._top_rows(what, score.contiguous(), R, k, largest, exclude, beta, d, row0)
        if consume:
            self._consume_draws(1, False)
        return res

    def _score_refusals(self, what, name, S, map, analytic):
        """What acquire and acquire_diverse refuse of a scored selection before any predictive runs."""
        if analytic and map:
            raise ValueError(f"{what}: analytic=True propagates moments through the posterior: map=True does not apply to it")
        one_pass = not analytic and (map or self.opt.get("quicktest"))
        draws = 1 if one_pass else int(self.opt["testSamples"] if S is None else S)
        if name == "mutual_info" and draws == 1:
            raise ValueError(f"{what}: score = 'mutual_info' is identically zero for one draw (map=True, quicktest or S = 1): "
                             "give S >= 2 without map, or rank by 'entropy'")

    def _score_pool(self, pool, name, S, map, analytic, row0):
        """The scoring half of acquire and acquire_diverse: the criterion's predictive over the pool (its draws consumed as it
        consumes them) and the score `name` of every row. Returns (vec, pred)."""
        if analytic:                               # ("bce" / "gauss": refused there, as predict_analytic refuses them)
            pred = (self.predict_analytic(pool, S=S, row0=row0, topk=2, keep_probs=False) if self.criterion == "nll"
                    else self.predict_analytic(pool))
        elif self.criterion == "nll":
            pred = self.predict_classes(pool, S=S, map=map, row0=row0, topk=2, keep_probs=False)
        elif self.criterion == "bce":
            pred = self.predict_labels(pool, S=S, map=map, row0=row0)
        else:
            pred = self.predict_regression(pool, S=S, map=map, row0=row0)
        if name == "least_confidence":
            vec = 1.0 - pred.topk_prob[:, 0]
        elif name == "margin":
            vec = pred.topk_prob[:, 1] - pred.topk_prob[:, 0]
        elif name == "total_variance":
            vec = pred.row_var + pred.row_noise_var
        elif self.criterion == "bce":
            vec = pred.row_mutual_info if name == "mutual_info" else pred.row_entropy
        elif name == "variance":
            vec = pred.row_var
        else:
            vec = pred.mutual_info if name == "mutual_info" else pred.entropy
        return vec, pred

    @_ordered
    def acquire(self, pool, k, score=None, S=None, map=False, analytic=False, exclude=None, beta=None, row0=None):
        """Choose the next k rows of the device-resident `pool` (R x input_size fp32) to label: score every row with the
        engine's own predictive, then top_rows. score (default: the first):
          criterion "nll":   "mutual_info" (BALD), "entropy", "least_confidence" (1 - the top probability), "margin" (the second
                             probability minus the top one: larger = more uncertain), "random" -- predict_classes(keep_probs=False, topk=2)
          criterion "bce":   "mutual_info", "entropy" (summed over the labels), "random" -- predict_labels
          criterion "mse":   "variance" (the epistemic row_var), "random" -- predict_regression
          criterion "gauss": "variance", "total_variance" (row_var + the row mean of the predicted noise variance), "random"
        S, map and row0 go to the predictive as they are (the pool is chunked by opt.predict_rows inside it, which cannot change
        the outcome); analytic=True scores "nll" / "mse" through predict_analytic instead. exclude: the rows already labelled.
        beta: None = the top k; beta > 0 = k rows sampled with probability proportional to score^beta, from draw self.draw + 1
        AFTER the predictive's draws, which is consumed; "random" (uniform over the candidates; no predictive runs) takes
        beta = 1 by default. Refused with the draw counter untouched: "mutual_info" with map=True or S = 1 (identically zero);
        "margin" with beta (never positive: every weight would be 0); with beta or "random", a row0 below 0 or with
        row0 + R above 2^32 (the noise is addressed by global row). Returns an AcquireResult."""
        what = "acquire"
        names = SCORES[self.criterion]
        name = names[0] if score is None else score
        if name not in names:
            raise ValueError(f"{what}: score = {score!r} is not one of criterion = '{self.criterion}''s scores {names}")
        k, beta = _check_k(what, k), _check_beta(what, beta)
        if name == "margin" and beta is not None:
            raise ValueError(f"{what}: score = 'margin' (the second probability minus the top one) is never positive, so score^beta "
                             "gives every row the weight 0: sample by 'least_confidence' or 'entropy', or take the top k (beta=None)")
        if (not torch.is_tensor(pool) or pool.dim() < 1 or pool.shape[0] < 1 or pool.dtype != torch.float32 or not pool.is_cuda
                or pool.numel() != pool.shape[0] * self.sizes[0]):
            raise ValueError(f"{what}: pool is an fp32 device tensor of R x {self.sizes[0]} (R >= 1): a host-resident pool is "
                             "not supported, move it to the device")
        R = pool.shape[0]
        exclude = _check_exclude(what, exclude, R, self.device)
        sel_row0 = self.rank * R if row0 is None else int(row0)
        if R >= 1 << 31:
            raise ValueError(f"{what}: a pool of R = {R} rows (R < 2^31: select in pieces and merge the scores with top_rows)")
        if (beta is not None or name == "random") and not 0 <= sel_row0 <= (1 << 32) - R:
            raise ValueError(f"{what}: row0 = {sel_row0} addresses the selection's noise by global row: 0 <= row0 and "
                             f"row0 + R <= 2^32 (R = {R}); give the pool's first global row, or beta=None")
        if name == "random":
            beta = 1.0 if beta is None else beta
            res = self._top_rows(what, None, R, k, True, exclude, beta, self.draw + 1, sel_row0)
            self._consume_draws(1, False)
            res.score_name, res.S, res.chunks = name, 0, 0
            return res
        self._score_refusals(what, name, S, map, analytic)
        vec, pred = self._score_pool(pool, name, S, map, analytic, row0)
        res = self._top_rows(what, vec.contiguous(), R, k, True, exclude, beta, self.draw + 1 if beta is not None else 0, sel_row0)
        if beta is not None:
            self._consume_draws(1, False)
        res.score_name, res.S, res.chunks, res.predictive = name, pred.S, pred.chunks, pred
        return res

    # ---- diverse acquisition: greedy k-centre over the network's own representation (vbnn_kcentre, csrc/kcentre.hip)
    @_ordered
    def features(self, inputs, layer=-1):
        """The MAP activations of hidden layer `layer` (default: the last, which the final Linear reads) for R input rows: an
        R x H fp32 device tensor. One forward on the means through the predictives' own route (chunked by opt.predict_rows,
        which cannot change a bit; pruned, compact and held-mask networks as the predictives honour them; under a compressed
        view only the last layer is kept row-major); bf16 activations are widened exactly. No draw is consumed and nothing of
        the training step is written."""
        what = "features"
        nl = len(self.vb)
        if isinstance(layer, bool) or int(layer) != layer or not -nl <= int(layer) < nl:
            raise ValueError(f"{what}: layer = {layer} (one of the {nl} hidden layers: -{nl} .. {nl - 1})")
        li = int(layer) % nl
        from .pruning import SparsePruneResult
        if li != nl - 1 and isinstance(self._pruned, SparsePruneResult):
            raise ValueError(f"{what}: a compressed pruned view keeps only the last hidden layer row-major (layer = -1)")
        p = self._predictive_plan(what, inputs, None, True, None)
        H = self.vb[li].O
        out = torch.empty(p.R, H, dtype=torch.float32, device=self.device)
        for _, c0, rows, xc in self._chunks(p):
            self._draw_forward(p, xc, rows, c0)
            out[c0:c0 + rows].copy_(p.bufs[li + 1].x.t[:rows, :H])
        return out

    def _kcentre(self, what, feat, k, weight, exclude, centres, min_dist):
        """The one caller of vbnn_kcentre: every argument checked already. min_dist given = resume."""
        lib, dev = L.lib(), self.device
        R, D = feat.shape
        nbytes = C.c_size_t()
        L.check(lib.vbnn_kcentre_workspace_bytes(R, D, k, C.byref(nbytes)))
        ws = getattr(self, "_kcentre_ws", None)
        if ws is None or ws.numel() * 8 < nbytes.value:
            ws = self._kcentre_ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
        index = torch.empty(k, dtype=torch.int32, device=dev)
        key = torch.empty(k, dtype=torch.float32, device=dev)
        dist = torch.empty(k, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        resume = min_dist is not None
        md = min_dist.clone() if resume else torch.empty(R, dtype=torch.float32, device=dev)
        a = L.KcentreArgs(feat=_p(feat), ld=feat.stride(0), weight=_p(weight), exclude=_p(exclude), centres=_p(centres), R=R, D=D,
                          n_centres=0 if centres is None else centres.numel(), k=k, resume=int(resume), reserved=0,
                          index=_p(index), key=_p(key), dist=_p(dist), min_dist=_p(md), counts=_p(counts), workspace=_p(ws),
                          workspace_bytes=ws.numel() * 8)
        L.check(lib.vbnn_kcentre(self.ctx.h, C.byref(a)))
        both = torch.cat([counts, ws[:1]]).cpu().tolist()          # (one copy: synchronises)
        res = SpreadResult(index, key, dist, md, both[:4], both[4])
        taken = torch.zeros(R, dtype=torch.uint8, device=dev) if exclude is None else exclude.clone()
        taken[index[:res.n_selected].long()] = 1
        res.exclude = taken
        return res

    def _check_features(self, what, features, R=None):
        if (not torch.is_tensor(features) or features.dtype != torch.float32 or not features.is_cuda
                or features.device != self.device or features.dim() != 2 or not 1 <= features.shape[0] < 1 << 31
                or not 1 <= features.shape[1] <= L.KCENTRE_MAX_D or (R is not None and features.shape[0] != R)):
            raise ValueError(f"{what}: features is an fp32 device matrix of " + ("R" if R is None else f"{R}")
                             + f" rows (1 <= R < 2^31) by 1 .. {L.KCENTRE_MAX_D} columns on the engine's device")
        if features.stride(1) != 1 or features.stride(0) < features.shape[1]:
            features = features.contiguous()
        return features

    @_ordered
    def spread_rows(self, features, k, weight=None, exclude=None, centres=None, state=None):
        """Greedy k-centre selection on any fp32 device matrix `features` (R x D, D <= 8192; a row pitch is honoured): k times
        the candidate row farthest -- in squared Euclidean distance, weighted by weight[r] >= 0 when given -- from every row in
        `centres` (int32 / int64 row indices, or a uint8 / bool mask of R entries: the rows already labelled) and every row
        picked before it. Exact and deterministic: ties go to the lower row, rows with exclude[r] != 0 are never taken, rows
        with a non-finite norm or a NaN / negative weight neither. state: a previous SpreadResult on the same features to
        continue from (its distances are resumed, its picks and its exclude stay excluded); a + b picks in two calls are the
        a + b picks of one. One call of vbnn_kcentre, no host synchronisation inside. Returns a SpreadResult (the counts
        synchronise; the tensors stay on the device)."""
        what = "spread_rows"
        features = self._check_features(what, features)
        R = features.shape[0]
        k = _check_spread_k(what, k)
        if weight is not None:
            if (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.device != self.device or weight.dim() != 1
                    or weight.numel() != R):
                raise ValueError(f"{what}: weight is an fp32 device vector of R = {R} entries")
            weight = weight.contiguous()
        exclude = _check_exclude(what, exclude, R, self.device)
        if centres is not None:
            if not torch.is_tensor(centres) or centres.device != self.device or centres.dim() != 1:
                raise ValueError(f"{what}: centres is a device vector (int32 / int64 row indices, or a uint8 / bool mask of R entries)")
            if centres.dtype in (torch.uint8, torch.bool):
                if centres.numel() != R:
                    raise ValueError(f"{what}: a centres mask has R = {R} entries")
                centres = torch.nonzero(centres, as_tuple=False).flatten().to(torch.int32)
            elif centres.dtype in (torch.int32, torch.int64):
                centres = centres.clamp(-1, (1 << 31) - 1).to(torch.int32).contiguous()  # (an index out of range stays out of range)
            else:
                raise ValueError(f"{what}: centres is int32 / int64 row indices or a uint8 / bool mask")
            if centres.numel() == 0:
                centres = None
        min_dist = None
        if state is not None:
            if (not isinstance(state, SpreadResult) or state.min_dist is None or state.min_dist.numel() != R
                    or state.min_dist.device != self.device):
                raise ValueError(f"{what}: state is a SpreadResult of a selection on the same R = {R} rows")
            min_dist = state.min_dist
            exclude = state.exclude if exclude is None else torch.maximum(exclude, state.exclude)
        return self._kcentre(what, features, k, weight, exclude, centres, min_dist)

    @_ordered
    def acquire_diverse(self, pool, k, score=None, S=None, map=False, analytic=False, exclude=None, weighted=True,
                        cover_labelled=True, features=None, row0=None):
        """acquire's diverse sibling (core-set selection): choose k rows of the device-resident `pool` that are far from the
        labelled rows and from each other in the network's own last hidden representation, each distance weighted by the
        row's uncertainty. weighted=True scores the pool exactly as acquire does (score, S, map, analytic, row0 and the draws
        consumed as there) and runs spread_rows on features (default: self.features(pool)) with weight = the score;
        weighted=False is plain k-centre: no predictive runs, no draw is consumed, score must be None. exclude: the rows
        already labelled, never taken; with cover_labelled they are also the initial centres, so the picks stay away from
        what is labelled. Refused with the draw counter untouched: "random" (no predictive vector) and "margin" (never
        positive) with weighted=True; what acquire refuses of "mutual_info" and analytic; features of the wrong shape, dtype
        or device; k outside 1 .. 4096. Returns a SpreadResult."""
        what = "acquire_diverse"
        name = None
        if weighted:
            names = SCORES[self.criterion]
            name = names[0] if score is None else score
            if name not in names:
                raise ValueError(f"{what}: score = {score!r} is not one of criterion = '{self.criterion}''s scores {names}")
            if name == "random":
                raise ValueError(f"{what}: score = 'random' has no predictive vector to weight the distances by: weighted=False "
                                 "is plain k-centre, acquire(score='random') is uniform sampling")
            if name == "margin":
                raise ValueError(f"{what}: score = 'margin' (the second probability minus the top one) is never positive and a "
                                 "weight is not negative: weight by 'least_confidence' or 'entropy'")
        elif score is not None:
            raise ValueError(f"{what}: weighted=False runs no predictive: score must be None (got {score!r})")
        k = _check_spread_k(what, k)
        if (not torch.is_tensor(pool) or pool.dim() < 1 or pool.shape[0] < 1 or pool.dtype != torch.float32 or not pool.is_cuda
                or pool.numel() != pool.shape[0] * self.sizes[0]):
            raise ValueError(f"{what}: pool is an fp32 device tensor of R x {self.sizes[0]} (R >= 1): a host-resident pool is "
                             "not supported, move it to the device")
        R = pool.shape[0]
        if R >= 1 << 31:
            raise ValueError(f"{what}: a pool of R = {R} rows (R < 2^31)")
        exclude = _check_exclude(what, exclude, R, self.device)
        if features is not None:
            features = self._check_features(what, features, R)
        vec = pred = None
        if weighted:
            self._score_refusals(what, name, S, map, analytic)
            vec, pred = self._score_pool(pool, name, S, map, analytic, row0)
            vec = vec.contiguous()
        if features is None:
            features = self._check_features(what, self.features(pool), R)
        centres = None
        if cover_labelled and exclude is not None:
            centres = torch.nonzero(exclude, as_tuple=False).flatten().to(torch.int32)
            centres = centres if centres.numel() else None
        res = self._kcentre(what, features, k, vec, exclude, centres, None)
        res.score_name = name
        if pred is not None:
            res.S, res.chunks, res.predictive = pred.S, pred.chunks, pred
        else:
            res.S, res.chunks = 0, 0
        return res
