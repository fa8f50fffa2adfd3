"""Conformal prediction sets of the fused engine (FusedMLP.conformal_calibrate / FusedMLP.conformal_sets) over vbnn_conformal
(csrc/conformal.hip) and vbnn_selective: from a held-out calibration set ONE exact order statistic of a per-row score, from a
test row every class whose score is at or below it -- a set that holds the true class with at least the requested probability
for exchangeable data, whatever the network (calibrated or not, pruned or compact, sampled or analytic). Everything the device
accumulates is an integer; the coverage and the set sizes are float64 on the host from those integers, so they do not depend on
the minibatch size, the chunking or the number of ranks. A mixin of vbnn_amd/engine.py:FusedMLP.

The regression side (FusedMLP.conformal_calibrate_intervals / FusedMLP.conformal_intervals over vbnn_conformal_interval and
vbnn_select_columns, csrc/conformal_interval.hip): one exact order statistic PER OUTPUT of a score s = max(a - t, t - b) / w turns
the mean and variance of predict_regression / predict_analytic ("scaled", "absolute") or the quantile planes of predict_quantiles
("cqr", conformalised quantile regression) into intervals [a - q w, b + q w] that cover with at least the requested probability;
scope="joint" calibrates the row's largest score instead, so that the box holds the WHOLE target vector.

Not here (follow-ups): randomised APS and RAPS regularisation; per-label sets for the "bce" criterion; class-conditional
(Mondrian) calibration; a row-parallel column select for one output; gathering a data-parallel run's calibration rows."""
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


class _ConformalSets:
    def _conformal_probs(self, what, result):
        if getattr(self, "criterion", "nll") in ("bce", "mse", "gauss"):
            raise ValueError(f"{what}: criterion = {self.criterion!r} has no class predictive: conformal sets need class "
                             "probabilities ('mse' / 'gauss': conformal_calibrate_intervals / conformal_intervals give conformal "
                             "intervals; per-label sets for 'bce' are among the follow-ups, not supported yet)")
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


# ---- conformal intervals for the regression predictives
_SCORES = ("scaled", "absolute", "cqr")
_SCOPES = ("per_output", "joint")
W_MIN = 2.0 ** -60                                           # the smallest width of the "scaled" score (vbnn_conformal_interval's w_min)


class IntervalCalibration:
    """FusedMLP.conformal_calibrate_intervals' outcome: score ("scaled" / "absolute" / "cqr"), scope ("per_output" / "joint"),
    levels, n (calibration rows; an output's NaN scores rank last), k (per level ceil((n + 1) level); k > n: the threshold is
    +inf), D (outputs), noise_var (the scalar of an "mse" + "scaled" call, else None), w_min, criterion (the engine's), probs
    ("cqr": per level the two probabilities of its quantile planes, else None), scores (the calibration scores on the device:
    P x n x D, or P x n row scores for "joint"; P = the levels for "cqr", else 1), qhat_dev (Q x D, or Q x 1 for "joint": what
    conformal_intervals reads). Reading qhat (Q lists of floats) or n_nan (NaN scores) synchronises; nothing else does."""

    def __init__(self, score, scope, levels, n, k, D, noise_var, w_min, criterion, probs, scores, qhat_dev, acc_dev):
        self.score, self.scope, self.levels, self.n, self.k, self.D = score, scope, list(levels), int(n), list(k), int(D)
        self.noise_var, self.w_min, self.criterion, self.probs = noise_var, w_min, criterion, probs
        self.scores, self.qhat_dev, self._acc_dev = scores, qhat_dev, acc_dev

    @property
    def qhat(self):
        return self.qhat_dev.cpu().tolist()

    @property
    def n_nan(self):
        return int(self._acc_dev.cpu().tolist()[0])


class IntervalResult:
    """FusedMLP.conformal_intervals' outcome over every row added so far (`into=` adds minibatches, merge() adds ranks), Q levels
    of D outputs. Device tensors of the rows added ON THIS RANK, in the order they were added: lo, hi (Q x R x D; NaN for a NaN
    element), row_covered (Q x R int32: the row's covered outputs, -1 in a row with a NaN; None without targets), covered
    (Q x R x D uint8, 255 for a NaN element; None unless keep_covered). From the accumulator's integers, float64, one per level:
    coverage (covered elements / elements counted; NaN without targets), joint_coverage (rows with EVERY output inside / rows
    counted), empty_fraction (intervals with lo > hi), n (elements counted), n_rows (rows counted); n_nan (NaN elements) and
    n_nan_rows. Reading any of them synchronises. Computed with torch in float64 from the kept planes: mean_width (per level, the
    mean of hi - lo over the elements that are not NaN) and coverage_per_output (Q x D, an exact integer sum; needs
    keep_covered)."""

    _ROWS = ("lo", "hi", "row_covered", "covered")

    def __init__(self, levels, D, acc_dev=None, host=None, targets=True):
        self.levels, self.D = list(levels), int(D)
        Q = len(self.levels)
        self._acc_dev = acc_dev                              # int64[8 Q + 2] on the device (the library's uint64 words), or None
        self._host = list(host) if host is not None else [0] * (8 * Q + 2)
        self._targets = bool(targets)
        self._rows = {k: [] for k in self._ROWS}

    def _row(self, k):
        parts = self._rows[k]
        if not parts or any(p is None for p in parts):
            return None
        if len(parts) > 1:
            parts[:] = [torch.cat(parts, dim=1)]
        return parts[0]

    lo = property(lambda self: self._row("lo"))
    hi = property(lambda self: self._row("hi"))
    row_covered = property(lambda self: self._row("row_covered"))
    covered = property(lambda self: self._row("covered"))

    def counts(self):
        """The accumulator as Python integers: per level elements counted, covered, rows counted, rows with every output covered,
        empty intervals, three reserved; then NaN elements, NaN rows (synchronises)."""
        dev = [v & 0xFFFFFFFFFFFFFFFF for v in self._acc_dev.cpu().tolist()] if self._acc_dev is not None else [0] * len(self._host)
        return [a + b for a, b in zip(dev, self._host)]

    def merge(self, other):
        """The sum of two results of the same levels and outputs (another rank's, another test set's): a host-side IntervalResult
        whose integers are the two added; the per-row tensors are this one's followed by the other's where they share a device."""
        if other.levels != self.levels or other.D != self.D:
            raise ValueError(f"merge: levels {self.levels} of {self.D} outputs against {other.levels} of {other.D}")
        out = IntervalResult(self.levels, self.D, None, [a + b for a, b in zip(self.counts(), other.counts())],
                             self._targets and other._targets)
        for k in out._rows:
            parts = self._rows[k] + other._rows[k]
            if len({p.device for p in parts if p is not None}) <= 1:
                out._rows[k] = list(parts)
        return out

    def _word(self, j):
        c = self.counts()
        return [c[8 * q + j] for q in range(len(self.levels))]

    _ratio = staticmethod(ConformalResult._ratio)
    n = property(lambda self: self._word(0))
    n_rows = property(lambda self: self._word(2))
    n_nan = property(lambda self: self.counts()[8 * len(self.levels)])
    n_nan_rows = property(lambda self: self.counts()[8 * len(self.levels) + 1])
    coverage = property(lambda self: self._ratio(self._word(1), self._word(0)) if self._targets else [_NAN] * len(self.levels))
    joint_coverage = property(lambda self: self._ratio(self._word(3), self._word(2)) if self._targets else [_NAN] * len(self.levels))
    empty_fraction = property(lambda self: self._ratio(self._word(4), self._word(0)))

    @property
    def mean_width(self):
        lo, hi = self.lo, self.hi
        if lo is None or hi is None:
            return None
        w = (hi.double() - lo.double()).flatten(1)
        ok = ~torch.isnan(w)
        return (torch.where(ok, w, torch.zeros_like(w)).sum(1) / ok.sum(1)).cpu().tolist()

    @property
    def coverage_per_output(self):
        c = self.covered
        if c is None:
            return None
        num, den = (c == 1).sum(1), (c != 255).sum(1)       # (int64: exact)
        return (num.double() / den.double()).cpu().tolist()


def _tensor(what, name, x, R=None, D=None):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.numel() < 1:
        raise ValueError(f"{what}: {name} is an R x D fp32 tensor on the device (got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}"
                         f"{', ' + str(x.dtype) + ' on ' + str(x.device) if isinstance(x, torch.Tensor) else ''})")
    if R is not None and tuple(x.shape) != (R, D):
        raise ValueError(f"{what}: {name} is {tuple(x.shape)}, expected R x D = {R} x {D}")
    return x.contiguous()


def _cat(parts, dim=0):
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=dim)


def _cqr_probs(what, probs, levels):
    """Per level the indices of its two quantile planes among probs, found as QuantilePredictResult.interval finds them."""
    out = []
    for v in levels:
        want = [(1.0 - v) / 2, (1.0 + v) / 2]
        w32 = torch.tensor(want, dtype=torch.float32).tolist()
        idx = [next((j for j, pj in enumerate(probs) if pj == w), None) for w in w32]
        if None in idx:
            raise ValueError(f"{what}: score = 'cqr' at level {v:g} needs the probabilities {want[0]:g} and {want[1]:g} among "
                             f"predict_quantiles' probs = {list(probs)}")
        out.append(tuple(idx))
    return out


class _RowSlice:
    """Rows lo .. hi of a regression or quantile result, as far as the interval calls look at one."""

    def __init__(self, r, lo, hi):
        if hasattr(r, "quantiles"):
            self.quantiles, self.probs, self.moments = r.quantiles[:, lo:hi], r.probs, _RowSlice(r.moments, lo, hi)
        else:
            self.mean, self.var = r.mean[lo:hi], r.var[lo:hi]
            self.noise_var = r.noise_var[lo:hi] if getattr(r, "noise_var", None) is not None else None


def split_rows(results, targets, h):
    """Lists of results and of their targets cut after the first h rows: (results, targets) before, (results, targets) after."""
    first, second, r0 = ([], []), ([], []), 0
    for r, t in zip(results, targets):
        n = t.shape[0]
        cut = min(max(h - r0, 0), n)
        if cut > 0:
            first[0].append(r if cut == n else _RowSlice(r, 0, cut))
            first[1].append(t[:cut])
        if cut < n:
            second[0].append(r if cut == 0 else _RowSlice(r, cut, n))
            second[1].append(t[cut:])
        r0 += n
    return first, second


def check_interval_options(what, levels, score, scope, probs=None):
    """What conformal_calibrate_intervals refuses about its options alone, for a caller that wants the refusal BEFORE it spends a
    pass on predictions (train.py): the levels, the score, the scope, and for "cqr" the level count and -- given predict_quantiles'
    probs -- both probabilities of every level. Returns the levels as floats."""
    lv = _levels(what, levels)
    if score not in _SCORES:
        raise ValueError(f"{what}: score = {score!r} ('scaled', 'absolute' or 'cqr')")
    if scope not in _SCOPES:
        raise ValueError(f"{what}: scope = {scope!r} ('per_output' or 'joint')")
    if score == "cqr":
        if len(lv) > 4:
            raise ValueError(f"{what}: score = 'cqr' takes at most 4 levels (predict_quantiles holds 8 probabilities)")
        if probs is not None:
            _cqr_probs(what, probs, lv)
    return lv


class _ConformalIntervals:
    def _interval_planes(self, what, result, score, levels, noise_var):
        """The planes of the one contract: dict(lower, upper: P x R x D or R x D; P; scale, scale2; scale_add; R; D; probs)."""
        crit = getattr(self, "criterion", "nll")
        if crit not in ("mse", "gauss"):
            raise ValueError(f"{what}: criterion = {crit!r} has no regression predictive: conformal intervals need the 'mse' or "
                             "the 'gauss' criterion ('nll': conformal_calibrate / conformal_sets)")
        if score not in _SCORES:
            raise ValueError(f"{what}: score = {score!r} ('scaled', 'absolute' or 'cqr')")
        if noise_var is not None and not (crit == "mse" and score == "scaled"):
            raise ValueError(f"{what}: noise_var belongs to criterion = 'mse' with score = 'scaled' (criterion = {crit!r}, score = "
                             f"{score!r}; a 'gauss' result brings its own noise plane)")
        if noise_var is not None and not (isinstance(noise_var, (int, float)) and float(noise_var) > 0.0 and float(noise_var) < float("inf")):
            raise ValueError(f"{what}: noise_var = {noise_var!r} (a positive finite number, or None)")
        pieces = list(result) if isinstance(result, (list, tuple)) else [result]
        if not pieces:
            raise ValueError(f"{what}: result is an empty list")
        if score == "cqr":
            if len(levels) > 4:
                raise ValueError(f"{what}: score = 'cqr' takes at most 4 levels (predict_quantiles holds 8 probabilities)")
            if not all(hasattr(r, "quantiles") and hasattr(r, "probs") for r in pieces):
                raise ValueError(f"{what}: score = 'cqr' needs the QuantilePredictResult of predict_quantiles (or a list of them)")
            probs = list(pieces[0].probs)
            if any(list(r.probs) != probs for r in pieces):
                raise ValueError(f"{what}: the pieces of result differ in probs")
            idx = _cqr_probs(what, probs, levels)
            qs = []
            for r in pieces:
                q = r.quantiles
                if not isinstance(q, torch.Tensor) or q.dim() != 3 or q.dtype != torch.float32 or not q.is_cuda or q.shape[0] != len(probs):
                    raise ValueError(f"{what}: quantiles is a Q x R x D fp32 tensor on the device")
                qs.append(q)
            if len({(q.device, q.shape[2]) for q in qs}) != 1:
                raise ValueError(f"{what}: the pieces of result differ in device or width")
            q = _cat(qs, dim=1)
            lower = torch.stack([q[i] for i, _ in idx]).contiguous()
            upper = torch.stack([q[j] for _, j in idx]).contiguous()
            return dict(lower=lower, upper=upper, P=len(levels), scale=None, scale2=None, scale_add=0.0, R=q.shape[1], D=q.shape[2],
                        probs=[(probs[i], probs[j]) for i, j in idx])
        moms = [getattr(r, "moments", r) for r in pieces]
        if not all(hasattr(m, "mean") and hasattr(m, "var") for m in moms):
            raise ValueError(f"{what}: result is the RegressionPredictResult of predict_regression / predict_analytic, the "
                             "QuantilePredictResult of predict_quantiles, or a list of them")
        means = [_tensor(what, "mean", m.mean) for m in moms]
        if len({(v.device, v.shape[1]) for v in means}) != 1:
            raise ValueError(f"{what}: the pieces of result differ in device or width")
        mean = _cat(means)
        R, D = mean.shape
        scale = scale2 = None
        if score == "scaled":
            scale = _cat([_tensor(what, "var", m.var, *v.shape) for m, v in zip(moms, means)])
            if crit == "gauss":
                scale2 = _cat([_tensor(what, "noise_var", getattr(m, "noise_var", None), *v.shape) for m, v in zip(moms, means)])
        return dict(lower=mean, upper=mean, P=1, scale=scale, scale2=scale2, scale_add=float(noise_var or 0.0), R=R, D=D, probs=None)

    @staticmethod
    def _interval_targets(what, targets, pl):
        if isinstance(targets, (list, tuple)):
            if not targets:
                raise ValueError(f"{what}: targets is an empty list")
            targets = [_tensor(what, "targets", t) for t in targets]
            if len({(t.device, t.shape[1]) for t in targets}) != 1:
                raise ValueError(f"{what}: the pieces of targets differ in device or width")
            targets = _cat(targets)
        t = _tensor(what, "targets", targets, pl["R"], pl["D"])
        if t.device != pl["lower"].device:
            raise ValueError(f"{what}: targets live on {t.device}, the result on {pl['lower'].device}")
        return t

    @staticmethod
    def _interval_args(pl, t):
        R, D = pl["R"], pl["D"]
        return L.ConformalIntervalArgs(lower=_p(pl["lower"]), upper=_p(pl["upper"]), ld=D, plane_stride=R * D if pl["P"] > 1 else 0,
                                       P=pl["P"], scale=_p(pl["scale"]), scale2=_p(pl["scale2"]), ld_s=D, scale_add=pl["scale_add"],
                                       scale_is_variance=1, w_min=W_MIN, target=_p(t), ld_t=D, R=R, D=D)

    @_ordered
    def conformal_calibrate_intervals(self, result, targets, levels=(0.9,), score="scaled", scope="per_output", noise_var=None):
        """Calibrates split conformal intervals on held-out rows. `result`: the RegressionPredictResult of predict_regression /
        predict_analytic or the QuantilePredictResult of predict_quantiles for n rows, or a list of them, concatenated along
        rows; `targets`: their n x D fp32 targets on the device, or a list likewise; `levels`: up to 8 coverage levels inside
        (0, 1). `score`: "scaled" (|t - mean| / sqrt(var + noise): the epistemic variance plus the aleatoric plane of a "gauss"
        result, or plus the scalar `noise_var` of an "mse" engine), "absolute" (|t - mean|) or "cqr" (conformalised quantile
        regression: max(q_lo - t, t - q_hi) on the (1 - level) / 2 and (1 + level) / 2 quantile planes, which must both be among
        predict_quantiles' probs -- at most 4 levels). `scope`: "per_output" (one threshold per output and level, the k-th
        smallest score of the output's column: vbnn_select_columns) or "joint" (one per level from the row's LARGEST score:
        vbnn_selective; the box then holds the whole target vector with the stated probability). k = ceil((n + 1) level) in
        exact arithmetic; a level with k > n gets +inf. One launch of vbnn_conformal_interval for the scores, then the selects;
        no host synchronisation. Returns an IntervalCalibration."""
        what = "conformal_calibrate_intervals"
        lv = _levels(what, levels)
        if scope not in _SCOPES:
            raise ValueError(f"{what}: scope = {scope!r} ('per_output' or 'joint')")
        pl = self._interval_planes(what, result, score, lv, noise_var)
        t = self._interval_targets(what, targets, pl)
        n, D, P, Q = pl["R"], pl["D"], pl["P"], len(lv)
        k = [conformal_rank(n, v) for v in lv]
        dv = t.device
        joint = scope == "joint"
        s = torch.empty((P, n) if joint else (P, n, D), dtype=torch.float32, device=dv)
        acc = torch.zeros(2, dtype=torch.int64, device=dv)
        a = self._interval_args(pl, t)
        a.Q, a.acc = 0, _p(acc)
        if joint:
            a.row_score = _p(s)
        else:
            a.score = _p(s)
        lib = L.lib()
        L.check(lib.vbnn_conformal_interval(self.ctx.h, C.byref(a)))
        W = 1 if joint else D
        qhat = torch.full((Q, W), float("inf"), dtype=torch.float32, device=dv)
        inside = [j for j, kj in enumerate(k) if kj <= n]
        # "cqr": a score plane per level, so a select per level; otherwise one select for every level
        groups = [[j] for j in inside] if P > 1 else ([inside] if inside else [])
        hit = torch.zeros(n, dtype=torch.int32, device=dv) if joint and inside else None
        for g in groups:
            direct = len(g) == 1 or g == list(range(Q))      # the ranks' rows of qhat are neighbours: written in place
            tau = qhat[g[0]:g[0] + len(g)] if direct else torch.empty(len(g), W, dtype=torch.float32, device=dv)
            plane = s[g[0] if P > 1 else 0]
            if joint:
                cnt = torch.empty(len(g), 4, dtype=torch.int64, device=dv)
                sa = L.SelectiveArgs(score=_p(plane), hit=_p(hit), R=n, Q=len(g), tau=_p(tau), counts=_p(cnt))
                for i, j in enumerate(g):
                    sa.k[i] = k[j]
                L.check(lib.vbnn_selective(self.ctx.h, C.byref(sa)))
            else:
                sa = L.SelectColumnsArgs(x=_p(plane), ld=D, R=n, D=D, Q=len(g), tau=_p(tau), ld_tau=D)
                for i, j in enumerate(g):
                    sa.k[i] = k[j]
                L.check(lib.vbnn_select_columns(self.ctx.h, C.byref(sa)))
            if not direct:
                for i, j in enumerate(g):                    # (device-to-device row copies: no upload, no read-back)
                    qhat[j].copy_(tau[i])
        return IntervalCalibration(score, scope, lv, n, k, D, noise_var if noise_var is None else float(noise_var), W_MIN,
                                   self.criterion, pl["probs"], s, qhat, acc)

    @_ordered
    def conformal_intervals(self, result, calibration, targets=None, keep_covered=False, into=None):
        """The conformal intervals of R rows at every level of `calibration` (an IntervalCalibration made by this engine's
        criterion, score and output count): ONE launch of vbnn_conformal_interval, which reads the thresholds on the device.
        `result` as conformal_calibrate_intervals takes it. `targets` (R x D fp32, optional) adds row_covered and the coverages;
        keep_covered=True also keeps the covered bytes (coverage_per_output). `into=` a previous IntervalResult (same levels and
        outputs, from this engine) adds to ITS device accumulator instead -- a test set over many minibatches, without a
        synchronisation -- and appends this call's tensors. Returns the IntervalResult."""
        what = "conformal_intervals"
        if not isinstance(calibration, IntervalCalibration):
            raise ValueError(f"{what}: calibration is the IntervalCalibration of conformal_calibrate_intervals")
        cal = calibration
        crit = getattr(self, "criterion", "nll")
        if crit not in ("mse", "gauss"):
            raise ValueError(f"{what}: criterion = {crit!r} has no regression predictive: conformal intervals need the 'mse' or "
                             "the 'gauss' criterion ('nll': conformal_calibrate / conformal_sets)")
        if cal.criterion != crit:
            raise ValueError(f"{what}: the calibration's criterion is {cal.criterion!r}, the engine's {crit!r}")
        if cal.score not in _SCORES or cal.scope not in _SCOPES:
            raise ValueError(f"{what}: the calibration's score = {cal.score!r} / scope = {cal.scope!r} is unknown")
        if _levels(what, cal.levels) != cal.levels or len(cal.k) != len(cal.levels):
            raise ValueError(f"{what}: the calibration's levels = {cal.levels} and ranks k = {cal.k} do not belong together")
        if cal.w_min != W_MIN:
            raise ValueError(f"{what}: the calibration's w_min = {cal.w_min!r}, this engine uses {W_MIN!r}")
        pl = self._interval_planes(what, result, cal.score, cal.levels, cal.noise_var)
        if pl["D"] != cal.D:
            raise ValueError(f"{what}: the calibration's D = {cal.D} outputs, the result has {pl['D']}: calibrate on this "
                             "network's own predictive")
        if pl["probs"] != cal.probs:
            raise ValueError(f"{what}: the calibration's probs = {cal.probs}, the result gives {pl['probs']}")
        Q, R, D = len(cal.levels), pl["R"], pl["D"]
        dv = pl["lower"].device
        W = 1 if cal.scope == "joint" else D
        if not isinstance(cal.qhat_dev, torch.Tensor) or tuple(cal.qhat_dev.shape) != (Q, W):
            raise ValueError(f"{what}: the calibration's levels = {cal.levels} and scope = {cal.scope!r} need {Q} x {W} thresholds")
        if cal.qhat_dev.device != dv:
            raise ValueError(f"{what}: the calibration lives on {cal.qhat_dev.device}, the result on {dv}")
        t = self._interval_targets(what, targets, pl) if targets is not None else None
        if keep_covered and t is None:
            raise ValueError(f"{what}: keep_covered needs targets")
        if into is not None:
            if not isinstance(into, IntervalResult) or into.levels != cal.levels or into.D != D:
                raise ValueError(f"{what}: into= is an IntervalResult of the same levels and outputs")
            if into._acc_dev is None or into._acc_dev.device != dv:
                raise ValueError(f"{what}: into= is a merged (host-side) result or lives on another device: accumulate on the "
                                 "device first, merge() afterwards")
            if into._targets != (t is not None):
                raise ValueError(f"{what}: into= was {'made with' if into._targets else 'made without'} targets; every minibatch "
                                 "of one result has them or none has")
        res = into or IntervalResult(cal.levels, D, torch.zeros(8 * Q + 2, dtype=torch.int64, device=dv), None, t is not None)
        lo = torch.empty(Q, R, D, dtype=torch.float32, device=dv)
        hi = torch.empty(Q, R, D, dtype=torch.float32, device=dv)
        row_covered = torch.empty(Q, R, dtype=torch.int32, device=dv) if t is not None else None
        covered = torch.empty(Q, R, D, dtype=torch.uint8, device=dv) if keep_covered else None
        a = self._interval_args(pl, t)
        a.Q, a.qhat, a.ld_qhat, a.per_column = Q, _p(cal.qhat_dev), W, int(cal.scope == "per_output")
        a.lo, a.hi, a.covered, a.row_covered, a.acc = _p(lo), _p(hi), _p(covered), _p(row_covered), _p(res._acc_dev)
        L.check(L.lib().vbnn_conformal_interval(self.ctx.h, C.byref(a)))
        for k, v in (("lo", lo), ("hi", hi), ("row_covered", row_covered), ("covered", covered)):
            res._rows[k].append(v)
        return res


class _Conformal(_ConformalSets, _ConformalIntervals):
    """The conformal mixin of FusedMLP: prediction sets for a class predictive, intervals for a regression one."""
