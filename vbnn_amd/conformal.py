"""Conformal prediction sets of the fused engine (FusedMLP.conformal_calibrate / FusedMLP.conformal_sets) over vbnn_conformal
(csrc/conformal.hip) and vbnn_selective: from a held-out calibration set ONE exact order statistic of a per-row score, from a
test row every class whose score is at or below it -- a set that holds the true class with at least the requested probability
for exchangeable data, whatever the network (calibrated or not, pruned or compact, sampled or analytic). Everything the device
accumulates is an integer; the coverage and the set sizes are float64 on the host from those integers, so they do not depend on
the minibatch size, the chunking or the number of ranks. A mixin of vbnn_amd/engine.py:FusedMLP.

Not here (follow-ups): randomised APS and RAPS regularisation; conformalised quantile regression on predict_quantiles; per-label
sets for the "bce" criterion; class-conditional (Mondrian) calibration."""
import ctypes as C
from fractions import Fraction

import torch

from . import _lib as L
from .nn import _ordered, _p
from .ranking import _rows

_KINDS = {"lac": L.CONFORMAL_LAC, "aps": L.CONFORMAL_APS}
_NAN = float("nan")


def conformal_rank(n, level):
    """k = ceil((n + 1) level): the rank of the calibration score that becomes the threshold. Exact rational arithmetic on the
    level's decimal representation (0.9 is nine tenths, so n = 99 gives 90; the float product 100 * 0.9 would give 91)."""
    x = (int(n) + 1) * Fraction(repr(float(level)))
    return -((-x.numerator) // x.denominator)


def _levels(what, levels):
    lv = [float(v) for v in (levels if isinstance(levels, (list, tuple)) else [levels])]
    if not 1 <= len(lv) <= L.CONFORMAL_MAX_Q:
        raise ValueError(f"{what}: {len(lv)} levels (1 .. {L.CONFORMAL_MAX_Q})")
    if not all(0.0 < v < 1.0 for v in lv):
        raise ValueError(f"{what}: levels = {lv} (each inside (0, 1))")
    return lv


class ConformalCalibration:
    """FusedMLP.conformal_calibrate's outcome: score_kind ("aps" / "lac"), classes (C), levels, n (calibration rows, the NaN ones
    included: they rank last), k (per level ceil((n + 1) level); k > n: the threshold is +inf), score (the n conformity scores on
    the device, NaN for a NaN row), qhat_dev (the thresholds on the device, what conformal_sets reads). Reading qhat (a list of
    floats; NaN, which the sets take as +inf, where the k-th score is a NaN row's) or n_nan synchronises; nothing else does."""

    def __init__(self, score_kind, classes, levels, n, k, score, qhat_dev, acc_dev):
        self.score_kind, self.classes, self.levels, self.n, self.k = score_kind, int(classes), list(levels), int(n), list(k)
        self.score, self.qhat_dev, self._acc_dev = score, qhat_dev, acc_dev

    @property
    def qhat(self):
        return self.qhat_dev.cpu().tolist()

    @property
    def n_nan(self):
        return int(self._acc_dev.cpu().tolist()[0])


class ConformalResult:
    """FusedMLP.conformal_sets' outcome over every row added so far (`into=` adds minibatches, merge() adds ranks), Q levels.
    Device tensors of the rows added ON THIS RANK, in the order they were added (Q x R; -1 / NaN in a NaN row): size (classes in
    the set), cut_index / cut_prob (the last admitted class and its probability; -1 / NaN for an empty set), covered (1 / 0, None
    without targets), members (Q x R x ceil(C / 32) int32 words, class j is bit j & 31 of word j >> 5; None unless asked for).
    From the accumulator's integers, float64, one per level: coverage (sets that hold the target; NaN without targets),
    mean_size, empty_fraction, singleton_fraction, singleton_accuracy (covered singletons / singletons), full_fraction (sets of
    all C classes), n (rows counted); n_nan (rows skipped for a NaN). Reading any of them synchronises."""

    _ROWS = ("size", "cut_index", "cut_prob", "covered", "members")

    def __init__(self, levels, classes, acc_dev=None, host=None, targets=True):
        self.levels, self.classes = list(levels), int(classes)
        Q = len(self.levels)
        self._acc_dev = acc_dev                              # int64[8 Q + 2] on the device (the library's uint64 words), or None
        self._host = list(host) if host is not None else [0] * (8 * Q + 2)
        self._targets = bool(targets)
        self._rows = {k: [] for k in self._ROWS}
        self._probs = []

    def _row(self, k):
        parts = self._rows[k]
        if not parts or any(p is None for p in parts):
            return None
        if len(parts) > 1:
            parts[:] = [torch.cat(parts, dim=1)]
        return parts[0]

    size = property(lambda self: self._row("size"))
    cut_index = property(lambda self: self._row("cut_index"))
    cut_prob = property(lambda self: self._row("cut_prob"))
    covered = property(lambda self: self._row("covered"))
    members = property(lambda self: self._row("members"))

    def counts(self):
        """The accumulator as Python integers: per level rows, covered, sum of size, empty, singletons, covered singletons, full,
        reserved; then n_nan, reserved (synchronises)."""
        dev = [v & 0xFFFFFFFFFFFFFFFF for v in self._acc_dev.cpu().tolist()] if self._acc_dev is not None else [0] * len(self._host)
        return [a + b for a, b in zip(dev, self._host)]

    def merge(self, other):
        """The sum of two results of the same levels and class count (another rank's, another test set's): a host-side
        ConformalResult whose integers are the two added; the per-row tensors are this one's followed by the other's where they
        share a device."""
        if other.levels != self.levels or other.classes != self.classes:
            raise ValueError(f"merge: levels {self.levels} of {self.classes} classes against {other.levels} of {other.classes}")
        out = ConformalResult(self.levels, self.classes, None, [a + b for a, b in zip(self.counts(), other.counts())],
                              self._targets and other._targets)
        for k in out._rows:
            parts = self._rows[k] + other._rows[k]
            if len({p.device for p in parts if p is not None}) <= 1:
                out._rows[k] = list(parts)
        out._probs = self._probs + other._probs
        return out

    def _word(self, j):
        c = self.counts()
        return [c[8 * q + j] for q in range(len(self.levels))]

    @staticmethod
    def _ratio(num, den):
        return [a / b if b else _NAN for a, b in zip(num, den)]

    n = property(lambda self: self._word(0))
    n_nan = property(lambda self: self.counts()[8 * len(self.levels)])
    coverage = property(lambda self: self._ratio(self._word(1), self._word(0)) if self._targets else [_NAN] * len(self.levels))
    mean_size = property(lambda self: self._ratio(self._word(2), self._word(0)))
    empty_fraction = property(lambda self: self._ratio(self._word(3), self._word(0)))
    singleton_fraction = property(lambda self: self._ratio(self._word(4), self._word(0)))
    singleton_accuracy = property(lambda self: self._ratio(self._word(5), self._word(4)) if self._targets else [_NAN] * len(self.levels))
    full_fraction = property(lambda self: self._ratio(self._word(6), self._word(0)))

    def to_lists(self, q=0):
        """The sets of level q as host lists of class indices, one per row, in ranking order (the most probable class first, ties
        to the lower index; an empty list for an empty set or a NaN row). Synchronises; a host-side convenience, not a hot path."""
        import numpy as np
        size = self.size[q].cpu().tolist()
        probs = torch.cat([p for p in self._probs]).cpu().numpy()
        u = np.ascontiguousarray(probs, dtype=np.float32).view(np.uint32)
        word = np.where(u >> 31, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)           # vbnn_order_word
        order = np.argsort(~word, axis=1, kind="stable")
        return [order[i, :max(s, 0)].tolist() for i, s in enumerate(size)]


class _Conformal:
    def _conformal_probs(self, what, result):
        if getattr(self, "criterion", "nll") in ("bce", "mse", "gauss"):
            raise ValueError(f"{what}: criterion = {self.criterion!r} has no class predictive: conformal sets need class "
                             "probabilities (per-label sets for 'bce' and conformalised quantile regression on predict_quantiles "
                             "for 'mse' / 'gauss' are follow-ups, not supported yet)")
        probs = _rows(what, "scores", result)
        if not isinstance(probs, torch.Tensor) or probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or probs.numel() < 1:
            raise ValueError(f"{what}: result is the PredictResult of predict / predict_classes / predict_analytic (its R x C fp32 "
                             "probs on the device), or a list of them")
        return probs.contiguous()

    @staticmethod
    def _conformal_targets(what, targets, probs):
        t = _rows(what, "targets", targets)
        R = probs.shape[0]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != probs.device or t.numel() != R:
            raise ValueError(f"{what}: targets are R = {R} int32 class indices on the device ({probs.device})")
        return t.contiguous().view(R)

    @_ordered
    def conformal_calibrate(self, result, targets, levels=(0.9,), score="aps"):
        """Calibrates split conformal prediction on held-out rows: `result` is the PredictResult of predict / predict_classes /
        predict_analytic for n rows (with its probs: keep_probs=True), or a list of them, concatenated along rows; `targets` their
        n int32 class indices on the device, or a list likewise; `levels` up to 8 coverage levels inside (0, 1); `score` "aps"
        (adaptive prediction sets: the probability mass ranked at or above the true class) or "lac" (1 - the true class's
        probability). One launch of vbnn_conformal (no thresholds: the n scores), then one of vbnn_selective for the k-th
        smallest score of every level at once, k = ceil((n + 1) level) in exact arithmetic; a level with k > n gets +inf. No
        host synchronisation. Returns a ConformalCalibration."""
        what = "conformal_calibrate"
        if score not in _KINDS:
            raise ValueError(f"{what}: score = {score!r} ('aps' or 'lac')")
        lv = _levels(what, levels)
        probs = self._conformal_probs(what, result)
        t = self._conformal_targets(what, targets, probs)
        n, Cn = probs.shape
        k = [conformal_rank(n, v) for v in lv]
        dv = probs.device
        s = torch.empty(n, dtype=torch.float32, device=dv)
        acc = torch.zeros(2, dtype=torch.int64, device=dv)
        a = L.ConformalArgs(probs=_p(probs), ld=Cn, target=_p(t), R=n, C=Cn, kind=_KINDS[score], Q=0, qhat=None, score=_p(s),
                            acc=_p(acc))
        L.check(L.lib().vbnn_conformal(self.ctx.h, C.byref(a)))
        qhat = torch.full((len(lv),), float("inf"), dtype=torch.float32, device=dv)
        inside = [j for j, kj in enumerate(k) if kj <= n]
        if inside:
            tau = torch.empty(len(inside), dtype=torch.float32, device=dv)
            cnt = torch.empty(len(inside), 4, dtype=torch.int64, device=dv)
            hit = torch.zeros(n, dtype=torch.int32, device=dv)
            sa = L.SelectiveArgs(score=_p(s), hit=_p(hit), R=n, Q=len(inside), tau=_p(tau), counts=_p(cnt))
            for i, j in enumerate(inside):
                sa.k[i] = k[j]
            L.check(L.lib().vbnn_selective(self.ctx.h, C.byref(sa)))
            qhat[torch.tensor(inside, device=dv)] = tau      # (an upload and a scatter: no read-back)
        return ConformalCalibration(score, Cn, lv, n, k, s, qhat, acc)

    @_ordered
    def conformal_sets(self, result, calibration, targets=None, members=False, into=None):
        """The prediction sets of R rows at every level of `calibration` (a ConformalCalibration of this class count): one launch
        of vbnn_conformal, which reads the thresholds on the device. `targets` (R int32 class indices, optional) adds `covered`
        and the coverage; members=True also writes the sets as bit words. `into=` a previous ConformalResult (same levels, from
        this engine) adds to ITS device accumulator instead -- a test set over many minibatches, without a synchronisation --
        and appends this call's per-row tensors. Returns the ConformalResult."""
        what = "conformal_sets"
        if not isinstance(calibration, ConformalCalibration):
            raise ValueError(f"{what}: calibration is the ConformalCalibration of conformal_calibrate")
        probs = self._conformal_probs(what, result)
        R, Cn = probs.shape
        if calibration.classes != Cn:
            raise ValueError(f"{what}: the calibration was made with {calibration.classes} classes, the result has {Cn}: "
                             "calibrate on this network's own predictive")
        if calibration.qhat_dev.device != probs.device:
            raise ValueError(f"{what}: the calibration lives on {calibration.qhat_dev.device}, the result on {probs.device}")
        t = self._conformal_targets(what, targets, probs) if targets is not None else None
        Q, dv = len(calibration.levels), probs.device
        if into is not None:
            if not isinstance(into, ConformalResult) or into.levels != calibration.levels or into.classes != Cn:
                raise ValueError(f"{what}: into= is a ConformalResult of the same levels and class count")
            if into._acc_dev is None or into._acc_dev.device != dv:
                raise ValueError(f"{what}: into= is a merged (host-side) result or lives on another device: accumulate on the "
                                 "device first, merge() afterwards")
            if into._targets != (t is not None):
                raise ValueError(f"{what}: into= was {'made with' if into._targets else 'made without'} targets; every minibatch "
                                 "of one result has them or none has")
        res = into or ConformalResult(calibration.levels, Cn, torch.zeros(8 * Q + 2, dtype=torch.int64, device=dv), None, t is not None)
        size = torch.empty(Q, R, dtype=torch.int32, device=dv)
        cut_index = torch.empty(Q, R, dtype=torch.int32, device=dv)
        cut_prob = torch.empty(Q, R, dtype=torch.float32, device=dv)
        covered = torch.empty(Q, R, dtype=torch.int32, device=dv) if t is not None else None
        member = torch.empty(Q, R, (Cn + 31) // 32, dtype=torch.int32, device=dv) if members else None
        a = L.ConformalArgs(probs=_p(probs), ld=Cn, target=_p(t), R=R, C=Cn, kind=_KINDS[calibration.score_kind], Q=Q,
                            qhat=_p(calibration.qhat_dev), score=None, size=_p(size), cut_index=_p(cut_index), cut_prob=_p(cut_prob),
                            covered=_p(covered), member=_p(member), acc=_p(res._acc_dev))
        L.check(L.lib().vbnn_conformal(self.ctx.h, C.byref(a)))
        for k, v in (("size", size), ("cut_index", cut_index), ("cut_prob", cut_prob), ("covered", covered), ("members", member)):
            res._rows[k].append(v)
        res._probs.append(probs)
        return res
