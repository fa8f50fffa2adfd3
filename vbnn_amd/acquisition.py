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
        if analytic and map:
            raise ValueError(f"{what}: analytic=True propagates moments through the posterior: map=True does not apply to it")
        one_pass = not analytic and (map or self.opt.get("quicktest"))
        draws = 1 if one_pass else int(self.opt["testSamples"] if S is None else S)
        if name == "mutual_info" and draws == 1:
            raise ValueError(f"{what}: score = 'mutual_info' is identically zero for one draw (map=True, quicktest or S = 1): "
                             "give S >= 2 without map, or rank by 'entropy'")
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
        res = self._top_rows(what, vec.contiguous(), R, k, True, exclude, beta, self.draw + 1 if beta is not None else 0, sel_row0)
        if beta is not None:
            self._consume_draws(1, False)
        res.score_name, res.S, res.chunks, res.predictive = name, pred.S, pred.chunks, pred
        return res
