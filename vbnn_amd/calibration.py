"""Classifier calibration and selective prediction of the fused engine (FusedMLP.calibration / FusedMLP.selective) over
vbnn_predict_calibration and vbnn_selective (csrc/calibration.hip): whether a prediction made at 0.9 confidence is right nine
times in ten, and what accuracy is left when the most uncertain rows are handed to somebody else. Everything the device
accumulates is an integer; ECE, MCE, the Brier score and the accuracies are float64 on the host from those integers, so they do
not depend on the minibatch size, the chunking or the number of ranks. A mixin of vbnn_amd/engine.py:FusedMLP."""
import ctypes as C
import math

import torch

from . import _lib as L
from .nn import _ordered, _p

_TWO32 = 4294967296.0


class CalibrationResult:
    """FusedMLP.calibration's outcome over every row added so far (`into=` adds minibatches, merge() adds ranks). From the
    accumulator's integers, float64: bins (M); bin_count / bin_hits (M integers: the rows whose confidence fell into
    [b / M, (b + 1) / M) and the correct ones among them); bin_accuracy / bin_confidence (M floats, NaN for an empty bin: the
    reliability diagram); ece (sum_b |hits_b - sum of the bin's confidences| / n); mce (the largest |accuracy - confidence| of a
    bin); brier (mean sum_c (p[c] - [c = t])^2); accuracy (fraction, not percent); n (rows counted); n_nan (rows skipped for a NaN).
    Reading any of them synchronises. Per-row device tensors of the rows added ON THIS RANK, in the order they were added: conf
    (the probability of the predicted class), hit (int32: 1 correct, 0 not, -1 a NaN row), entropy, mutual_info (the
    predictive's) -- what FusedMLP.selective takes."""

    def __init__(self, bins, acc_dev=None, host=None):
        self.bins = int(bins)
        self._acc_dev = acc_dev                              # int64[3 M + 4] on the device (the library's uint64 words), or None
        self._host = list(host) if host is not None else [0] * (3 * self.bins + 4)      # what merge() added
        self._rows = {"conf": [], "hit": [], "entropy": [], "mutual_info": []}

    def _append(self, **rows):
        for k, v in rows.items():
            self._rows[k].append(v)

    def _row(self, k):
        parts = self._rows[k]
        if not parts:
            return None
        if len(parts) > 1:
            parts[:] = [torch.cat(parts)]
        return parts[0]

    conf = property(lambda self: self._row("conf"))
    hit = property(lambda self: self._row("hit"))
    entropy = property(lambda self: self._row("entropy"))
    mutual_info = property(lambda self: self._row("mutual_info"))

    def counts(self):
        """The accumulator as Python integers: count[M], hits[M], conf_fix[M], brier_fix, n_rows, n_nan, reserved (synchronises)."""
        dev = [v & 0xFFFFFFFFFFFFFFFF for v in self._acc_dev.cpu().tolist()] if self._acc_dev is not None else [0] * len(self._host)
        return [a + b for a, b in zip(dev, self._host)]

    def merge(self, other):
        """The sum of two results of the same binning (another rank's, another test set's): a host-side CalibrationResult whose
        integers are the two added; the per-row tensors are this one's followed by the other's where they share a device."""
        if other.bins != self.bins:
            raise ValueError(f"merge: {self.bins} bins against {other.bins}")
        out = CalibrationResult(self.bins, None, [a + b for a, b in zip(self.counts(), other.counts())])
        for k in out._rows:
            parts = self._rows[k] + other._rows[k]
            if len({p.device for p in parts}) <= 1:
                out._rows[k] = list(parts)
        return out

    # ---- float64 from the integers
    @property
    def bin_count(self):
        return self.counts()[:self.bins]

    @property
    def bin_hits(self):
        return self.counts()[self.bins:2 * self.bins]

    def _sums(self):
        c, M = self.counts(), self.bins
        return c[:M], c[M:2 * M], [v / _TWO32 for v in c[2 * M:3 * M]], c[3 * M], c[3 * M + 1], c[3 * M + 2]

    @property
    def bin_accuracy(self):
        cnt, hits, _, _, _, _ = self._sums()
        return [h / c if c else float("nan") for c, h in zip(cnt, hits)]

    @property
    def bin_confidence(self):
        cnt, _, cs, _, _, _ = self._sums()
        return [s / c if c else float("nan") for c, s in zip(cnt, cs)]

    @property
    def ece(self):
        _, hits, cs, _, n, _ = self._sums()
        return sum(abs(h - s) for h, s in zip(hits, cs)) / n if n else float("nan")

    @property
    def mce(self):
        cnt, hits, cs, _, n, _ = self._sums()
        return max(abs(h - s) / c for c, h, s in zip(cnt, hits, cs) if c) if n else float("nan")

    @property
    def brier(self):
        _, _, _, bf, n, _ = self._sums()
        return bf / _TWO32 / n if n else float("nan")

    @property
    def accuracy(self):
        _, hits, _, _, n, _ = self._sums()
        return sum(hits) / n if n else float("nan")

    @property
    def n(self):
        return self.counts()[3 * self.bins + 1]

    @property
    def n_nan(self):
        return self.counts()[3 * self.bins + 2]


class SelectiveResult:
    """FusedMLP.selective's outcome: coverages (as given), k (the ranks, max(1, ceil(c R))), threshold (Q floats: the score of
    the k-th most certain row -- predicting only where score <= threshold covers at least k rows), accuracy (Q float64 fractions:
    the accuracy over the k most certain rows, ties at the threshold shared out evenly), counts (Q lists of the four integers
    n_below, hits_below, n_tied, hits_tied)."""

    def __init__(self, coverages, k, threshold, counts):
        self.coverages, self.k, self.threshold, self.counts = coverages, k, threshold, counts
        self.accuracy = [(c[1] + (kj - c[0]) * c[3] / c[2]) / kj for c, kj in zip(counts, k)]


class _Calibration:
    @_ordered
    def calibration(self, result, targets, bins=15, into=None):
        """The reliability of a class predictive: `result` is the PredictResult of predict / predict_classes / predict_analytic
        for R rows (with its probs: keep_probs=True), targets their R int32 class indices on the device, bins the number of
        equal-width confidence bins (1 .. 64). One launch of vbnn_predict_calibration bins every row by the probability of its
        predicted class and adds the integer sums to the result's device accumulator; `into=` a previous CalibrationResult (same
        bins, from this engine) adds to ITS accumulator instead -- a test set over many minibatches, without a synchronisation
        -- and appends this call's per-row conf, hit, entropy and mutual_info. Returns the CalibrationResult."""
        what = "calibration"
        if getattr(self, "criterion", "nll") == "bce":       # (per-label reliability is a follow-up)
            raise ValueError(f"{what}: criterion = 'bce' has no class predictive to calibrate: use predict_labels (its "
                             "label_accuracy, log_lik and per-label mutual_info); per-label calibration is not supported yet")
        probs = getattr(result, "probs", None)
        if probs is None:
            raise ValueError(f"{what}: the result holds no class probabilities (probs is None) -- run the predictive with "
                             "keep_probs=True")
        if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or result.pred is None:
            raise ValueError(f"{what}: result is the PredictResult of predict / predict_classes / predict_analytic")
        R, Cn = probs.shape
        if targets is None or targets.dtype != torch.int32 or not targets.is_cuda or targets.numel() != R:
            raise ValueError(f"{what}: targets are R = {R} int32 class indices on the device")
        M = int(bins)
        if not 1 <= M <= L.CALIBRATION_MAX_BINS:
            raise ValueError(f"{what}: bins = {M} (1 .. {L.CALIBRATION_MAX_BINS})")
        if into is not None:
            if not isinstance(into, CalibrationResult) or into.bins != M:
                raise ValueError(f"{what}: into= is a CalibrationResult of the same {M} bins")
            if into._acc_dev is None or into._acc_dev.device != probs.device:
                raise ValueError(f"{what}: into= is a merged (host-side) result or lives on another device: accumulate on the "
                                 "device first, merge() afterwards")
        res = into or CalibrationResult(M, torch.zeros(3 * M + 4, dtype=torch.int64, device=probs.device))
        probs, targets, pred = probs.contiguous(), targets.contiguous(), result.pred.contiguous()
        conf = torch.empty(R, dtype=torch.float32, device=probs.device)
        hit = torch.empty(R, dtype=torch.int32, device=probs.device)
        a = L.CalibrationArgs(probs=_p(probs), ld=Cn, pred=_p(pred), target=_p(targets), R=R, C=Cn, bins=M, conf=_p(conf),
                              hit=_p(hit), brier=None, bin=None, acc=_p(res._acc_dev))
        L.check(L.lib().vbnn_predict_calibration(self.ctx.h, C.byref(a)))
        res._append(conf=conf, hit=hit, entropy=result.entropy, mutual_info=result.mutual_info)
        return res

    @_ordered
    def selective(self, score, hit, coverages):
        """Accuracy against coverage: with the R rows ordered by `score` (fp32 on the device, lower = more certain -- a
        CalibrationResult's entropy or mutual_info, or 1 - conf; rows with a NaN score rank last) and hit (R int32, above zero =
        correct; a CalibrationResult's -1 for a NaN row counts as wrong), the accuracy over the k = max(1, ceil(c R)) most certain rows for each coverage c in (0, 1] (up to 32 of
        them). One launch of vbnn_selective -- an exact radix select, ties at the threshold shared out evenly instead of by row
        order, so scores that are all equal give the overall accuracy. Returns a SelectiveResult (synchronises)."""
        what = "selective"
        if score.dtype != torch.float32 or not score.is_cuda or score.dim() != 1 or score.numel() < 1:
            raise ValueError(f"{what}: score is an fp32 device vector of R >= 1 rows")
        R = score.numel()
        if hit.dtype != torch.int32 or not hit.is_cuda or hit.numel() != R:
            raise ValueError(f"{what}: hit is R = {R} int32 values on the device")
        cov = [float(c) for c in coverages]
        if not 1 <= len(cov) <= L.SELECTIVE_MAX_Q:
            raise ValueError(f"{what}: {len(cov)} coverages (1 .. {L.SELECTIVE_MAX_Q})")
        if not all(0.0 < c <= 1.0 for c in cov):
            raise ValueError(f"{what}: coverages = {cov} (each in (0, 1])")
        k = [max(1, min(R, math.ceil(c * R))) for c in cov]
        Q = len(k)
        score, hit = score.contiguous(), hit.clamp(min=0).contiguous()      # (-1, a CalibrationResult's NaN row, is not a hit)
        tau = torch.empty(Q, dtype=torch.float32, device=score.device)
        counts = torch.empty(Q, 4, dtype=torch.int64, device=score.device)
        a = L.SelectiveArgs(score=_p(score), hit=_p(hit), R=R, Q=Q, tau=_p(tau), counts=_p(counts))
        for j, kj in enumerate(k):
            a.k[j] = kj
        L.check(L.lib().vbnn_selective(self.ctx.h, C.byref(a)))
        return SelectiveResult(cov, k, tau.cpu().tolist(), counts.cpu().tolist())
