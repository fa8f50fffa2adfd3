"""Rank metrics of the fused engine (FusedMLP.ranking) over vbnn_rank_metrics (csrc/ranking.hip): per label the exact AUROC and
average precision of a score column, and the hit counts at chosen thresholds -- what a screening model with rare positives is
judged by, where the label accuracy says almost nothing. The device sorts each column exactly and leaves integers; every ratio
is float64 on the host from exact integer division, so the values do not depend on the grid or on how the test set was cut into
minibatches. Rank metrics are NOT additive over rows: a data-parallel run gathers its probabilities before calling this. A mixin
of vbnn_amd/engine.py:FusedMLP."""
import ctypes as C

import torch

from . import _lib as L
from .nn import _ordered, _p

_TWO32 = 1 << 32
_NAN = float("nan")


def _ratio(num, den):
    return num / den if den else _NAN                       # (Python's int / int: the correctly rounded quotient)


def _mean_defined(values):
    vals = [v for v in values if v == v]
    return (sum(vals) / len(vals) if vals else _NAN), len(vals)


class RankingResult:
    """FusedMLP.ranking's outcome for D labels. The device's integers as Python ints, one per label: n_pos, n_neg, n_nan (elements
    left out for a NaN score or target), u2 (sum over the positives of 2 #{negatives below} + #{negatives tied}), ap_fix (sum over
    the positives of floor(TP 2^32 / (TP + FP)) at the positive's own score as the threshold); tp / fp (Q lists of D: positives /
    negatives with score >= thresholds[q]). From them, float64: auroc (u2 / (2 n_pos n_neg), ties counted half; NaN for a label
    without positives or without negatives), average_precision (ap_fix / (2^32 n_pos): the step-wise sum (R_n - R_{n-1}) P_n,
    within 2^-32 below the exact rational; NaN without positives), macro_auroc / macro_average_precision (the means over the
    labels where the value is defined) with n_defined = (labels with an AUROC, labels with an average precision); thresholds (as
    fp32 holds them); per threshold and label precision (tp / (tp + fp)), recall = tpr (tp / n_pos), fpr (fp / n_neg), f1
    (2 tp / (2 tp + fp + fn)) -- NaN where the denominator is 0. With micro=True micro_* hold the same fields (scalars; lists of Q)
    for all R D elements taken as one column; None otherwise."""

    def __init__(self, words, thresholds, micro_words=None):
        Q = len(thresholds)
        self.thresholds = list(thresholds)
        self.words = [list(w) for w in words]
        self.n_pos, self.n_neg, self.n_nan = ([w[k] for w in words] for k in (0, 1, 2))
        self.u2, self.ap_fix = [w[3] for w in words], [w[4] for w in words]
        self.tp = [[w[6 + 2 * q] for w in words] for q in range(Q)]
        self.fp = [[w[7 + 2 * q] for w in words] for q in range(Q)]
        self.auroc = [_ratio(u, 2 * p * n) for u, p, n in zip(self.u2, self.n_pos, self.n_neg)]
        self.average_precision = [_ratio(a, _TWO32 * p) for a, p in zip(self.ap_fix, self.n_pos)]
        self.macro_auroc, n_a = _mean_defined(self.auroc)
        self.macro_average_precision, n_p = _mean_defined(self.average_precision)
        self.n_defined = (n_a, n_p)
        self.precision = [[_ratio(t, t + f) for t, f in zip(tq, fq)] for tq, fq in zip(self.tp, self.fp)]
        self.recall = [[_ratio(t, p) for t, p in zip(tq, self.n_pos)] for tq in self.tp]
        self.tpr = self.recall
        self.fpr = [[_ratio(f, n) for f, n in zip(fq, self.n_neg)] for fq in self.fp]
        self.f1 = [[_ratio(2 * t, 2 * t + f + (p - t)) for t, f, p in zip(tq, fq, self.n_pos)] for tq, fq in zip(self.tp, self.fp)]
        self.micro = RankingResult([micro_words], thresholds) if micro_words is not None else None
        m = self.micro
        for k in ("n_pos", "n_neg", "n_nan", "u2", "ap_fix", "auroc", "average_precision"):
            setattr(self, "micro_" + k, getattr(m, k)[0] if m else None)
        for k in ("tp", "fp", "precision", "recall", "tpr", "fpr", "f1"):
            setattr(self, "micro_" + k, [v[0] for v in getattr(m, k)] if m else None)


def _rows(what, name, x):
    """A tensor or a list of tensors as one tensor, concatenated along rows."""
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError(f"{what}: {name} is an empty list")
        x = [_probs(what, v) if name == "scores" else v for v in x]
        if not all(isinstance(v, torch.Tensor) for v in x):
            raise ValueError(f"{what}: {name} is a device tensor or a list of them")
        if len({(v.dtype, v.device, v.shape[1:]) for v in x}) != 1:
            raise ValueError(f"{what}: the pieces of {name} differ in dtype, device or width")
        return x[0] if len(x) == 1 else torch.cat(x)
    return _probs(what, x) if name == "scores" else x


def _probs(what, x):
    if isinstance(x, torch.Tensor):
        return x
    if not hasattr(x, "probs"):
        raise ValueError(f"{what}: scores is an R x D fp32 device tensor, a LabelPredictResult / PredictResult, or a list of them")
    if x.probs is None:
        raise ValueError(f"{what}: the result holds no class probabilities (probs is None) -- run the predictive with "
                         "keep_probs=True")
    return x.probs


class _Ranking:
    @_ordered
    def ranking(self, scores, targets, thresholds=(0.5,), micro=False):
        """Per-label rank metrics: `scores` is an R x D fp32 device tensor, the LabelPredictResult / PredictResult of a
        predictive (its probs), or a list of either, concatenated along rows (a test set scored in minibatches); `targets` is
        R x D fp32 (a label is positive iff > 0.5, the Bernoulli criterion's hit rule) or R int32 class indices (column j
        against the rest: positive iff the clamped class is j), or a list likewise; `thresholds` up to 16 floats at which the
        hit counts are taken (score >= threshold). micro=True also takes all R D elements as one column (fp32 targets only).
        One call of vbnn_rank_metrics per view: an exact sort of every column on the device in a workspace of 16 R D bytes.
        Works with any criterion and needs no predictive state. Returns a RankingResult (synchronises)."""
        what = "ranking"
        s = _rows(what, "scores", scores)
        t = _rows(what, "targets", targets)
        if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.dtype != torch.float32 or not s.is_cuda or s.numel() < 1:
            raise ValueError(f"{what}: scores are R x D fp32 on the device (R, D >= 1)")
        R, D = s.shape
        if not isinstance(t, torch.Tensor) or t.device != s.device:
            raise ValueError(f"{what}: targets live on the scores' device ({s.device})")
        if t.dtype == torch.float32:
            if tuple(t.shape) != (R, D):
                raise ValueError(f"{what}: fp32 targets are R x D = {R} x {D} (got {tuple(t.shape)})")
        elif t.dtype == torch.int32:
            if t.numel() != R or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
                raise ValueError(f"{what}: int32 targets are R = {R} class indices (got {tuple(t.shape)})")
            if micro:
                raise ValueError(f"{what}: micro=True needs R x D fp32 targets (class indices name one column per row)")
        else:
            raise ValueError(f"{what}: targets are R x D fp32 labels or R int32 class indices (got {t.dtype})")
        tau = [float(v) for v in thresholds]
        if len(tau) > L.RANK_MAX_Q:
            raise ValueError(f"{what}: {len(tau)} thresholds (0 .. {L.RANK_MAX_Q})")
        if R * D > 2 ** 31 - 1:
            raise ValueError(f"{what}: R D = {R * D} elements (at most 2^31 - 1)")
        s, t = s.contiguous(), t.contiguous()
        tau32 = torch.tensor(tau, dtype=torch.float32).tolist()
        ws = torch.empty(2 * R * D, dtype=torch.int64, device=s.device)       # (shared by the micro view: the same size)
        words = self._rank_call(s, t, R, D, tau32, ws)
        micro_words = self._rank_call(s.view(R * D, 1), t.view(R * D, 1), R * D, 1, tau32, ws)[0] if micro else None
        return RankingResult(words, tau32, micro_words)

    def _rank_call(self, s, t, R, D, tau, ws):
        Q = len(tau)
        out = torch.empty(D, 6 + 2 * Q, dtype=torch.int64, device=s.device)
        need = C.c_size_t()
        L.check(L.lib().vbnn_rank_metrics_workspace_bytes(R, D, C.byref(need)))
        assert need.value <= ws.numel() * 8
        fp = t.dtype == torch.float32
        a = L.RankMetricsArgs(score=_p(s), ld=D, target=_p(t) if fp else None, ld_t=D if fp else 0,
                              target_class=None if fp else _p(t), R=R, D=D, Q=Q, out=_p(out), workspace=_p(ws),
                              workspace_bytes=ws.numel() * 8)
        for q, v in enumerate(tau):
            a.tau[q] = v
        L.check(L.lib().vbnn_rank_metrics(self.ctx.h, C.byref(a)))
        return [[v & 0xFFFFFFFFFFFFFFFF for v in row] for row in out.cpu().tolist()]
