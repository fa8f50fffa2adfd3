"""GPU tests of the conformal intervals: vbnn_conformal_interval and vbnn_select_columns (include/vbnn_hip.h) called directly on
uploaded arrays, and FusedMLP.conformal_calibrate_intervals / FusedMLP.conformal_intervals / train.py's series over them.
Every output word and byte is compared BIT FOR BIT with the fp32 / integer restatement of tests/_interval_np.py (which
tests/test_interval_ref.py holds to the float64 definition and to brute force on the CPU): there are no tolerances here. The
thresholds are the restatement's own scores, so that a kernel that compared with < where the contract says <= (or fused the
product into the sum) would move an element across a cut."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._interval_np import (F32, QNAN_BITS, W_MIN, calibrate32, conformal_rank, interval32, n_words, score32, select_columns32,
                                width32)

pytestmark = pytest.mark.gpu

LAYOUTS = ("dense", "padded", "odd", "offset")
GUARD = 4                                                    # sentinel elements on either side of every output
FORMS = ("none", "var", "var2", "plain", "floor")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def pitch(D, layout):
    return {"dense": D, "padded": D + 4 - D % 4 + 4, "odd": D + 3, "offset": D}[layout]


def upload(x, layout, plane_gap=0):
    """x: (P x) R x D fp32 -> a device buffer of NaNs holding it with the layout's row pitch, the base one float past a 16-byte
    boundary for "offset", the planes plane_gap floats apart beyond R ld. Returns (buffer, pointer, ld, plane_stride)."""
    x = np.asarray(x, F32)
    x3 = x if x.ndim == 3 else x[None]
    P, R, D = x3.shape
    ld = pitch(D, layout)
    off = 1 if layout == "offset" else 0
    ps = R * ld + plane_gap
    buf = torch.full((P * ps + off + 4,), float("nan"), dtype=torch.float32, device="cuda")
    for p in range(P):
        buf[off + p * ps:off + p * ps + R * ld].view(R, ld)[:, :D] = dev(x3[p])
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * off, ld, ps


class Out:
    """An output between two guards of sentinels. shift = 1 moves its base one element on: a float output then starts off the
    16-byte boundary (scalar stores whatever D is), the covered bytes off the 4-byte one."""
    def __init__(self, shape, dtype, shift=0):
        self.shape, self.n, self.lead = shape, int(np.prod(shape)), GUARD + shift
        self.sent = {torch.float32: float("nan"), torch.int32: -7, torch.uint8: 0xAB}[dtype]
        self.buf = torch.full((self.n + 2 * GUARD + shift,), self.sent, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.lead * self.buf.element_size())

    def get(self):
        h = host(self.buf)
        g = np.concatenate([h[:self.lead], h[self.lead + self.n:]])
        assert (np.isnan(g).all() if self.buf.dtype == torch.float32 else (g == self.sent).all()), "guard bytes written"
        return h[self.lead:self.lead + self.n].reshape(self.shape)


def scale_inputs(form, R, D, rng):
    """(scale, scale2, scale_add, is_variance, w_min) of a form, and the restatement's width."""
    if form == "none":
        return None, None, 0.0, 1, W_MIN, None
    s1 = rng.gamma(2.0, 0.5, (R, D)).astype(F32)
    s2, add, isv, wmin = None, 0.0, 1, W_MIN
    if form == "var2":
        s2, add = rng.gamma(2.0, 0.1, (R, D)).astype(F32), 0.125
    if form == "plain":
        isv = 0
    if form == "floor":                                      # a third of the widths are w_min itself
        s1[rng.random((R, D)) < 0.33] = 0
        wmin = 0.5
    return s1, s2, add, isv, wmin, width32(s1, s2, add, bool(isv), wmin)


def planes(P, R, D, rng, cqr):
    mean = rng.standard_normal((P, R, D)).astype(F32)
    if not cqr:
        return mean, mean
    half = rng.gamma(2.0, 0.4, (P, R, D)).astype(F32)
    return (mean - half).astype(F32), (mean + half).astype(F32)


def thresholds(s, Q, per_column, rng):
    """Q x D (or Q) thresholds: the restatement's own scores first (ties at the cut), then +inf, NaN, a negative one, 0."""
    P, R, D = s.shape
    clean = np.where(np.isnan(s), F32(0.5), s)
    q = np.empty((Q, D if per_column else 1), F32)
    for j in range(Q):
        rows = rng.integers(0, R, q.shape[1])
        q[j] = clean[min(j, P - 1), rows, np.arange(q.shape[1])]
    special = (np.inf, np.nan, -0.25, 0.0)
    first = int(rng.integers(4))                             # (the rotation starts anywhere: every Q meets every special value)
    for j in range(1, Q):
        q[j, ::2 if per_column else 1] = special[(first + j) % 4]
    if Q == 1 and rng.integers(2):                           # one threshold: a special value on the odd columns, or on all
        q[0, (slice(1, None, 2) if q.shape[1] > 1 else slice(None))] = special[first]
    return q if per_column else q[:, 0]


def run_interval(lower, upper, target, qhat=None, form_in=None, per_column=True, layout="dense", plane_gap=0, skip=(), acc=None,
                 with_acc=True, out_shift=0):
    """vbnn_conformal_interval on NumPy arrays (lower / upper: P x R x D). qhat None: score mode. skip: outputs passed as NULL.
    out_shift = 1: every output starts one element past its aligned base (Out)."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    P, R, D = lower.shape
    s1, s2, add, isv, wmin = form_in if form_in is not None else (None, None, 0.0, 1, W_MIN)
    keep = []
    lb, lp, ld, ps = upload(lower, layout, plane_gap)
    if upper is lower:
        ub, up = lb, lp
    else:
        ub, up, _, _ = upload(upper, layout, plane_gap)
    a = L.ConformalIntervalArgs(lower=lp, upper=up, ld=ld, plane_stride=ps if P > 1 else 0, P=P, scale_add=add, scale_is_variance=isv,
                                w_min=wmin, per_column=int(per_column), R=R, D=D)
    if s1 is not None:
        b, a.scale, a.ld_s, _ = upload(s1, layout)
        keep.append(b)
    if s2 is not None:
        b, a.scale2, _, _ = upload(s2, layout)
        keep.append(b)
    if target is not None:
        b, a.target, a.ld_t, _ = upload(target, layout)
        keep.append(b)
    if qhat is None:
        Q = 0
        outs = dict(score=Out((P, R, D), torch.float32, out_shift), row_score=Out((P, R), torch.float32, out_shift))
        nacc = 2
    else:
        qhat = np.asarray(qhat, F32)
        Q = qhat.shape[0]
        qd = dev(qhat)
        a.qhat, a.ld_qhat = qd.data_ptr(), (D if per_column else 1)
        outs = dict(lo=Out((Q, R, D), torch.float32, out_shift), hi=Out((Q, R, D), torch.float32, out_shift))
        if target is not None:
            outs.update(covered=Out((Q, R, D), torch.uint8, out_shift), row_covered=Out((Q, R), torch.int32, out_shift))
        nacc = n_words(Q)
    a.Q = Q
    outs = {k: v for k, v in outs.items() if k not in skip}
    for k, v in outs.items():
        setattr(a, k, v.ptr)
    accd = dev((np.zeros(nacc, np.uint64) if acc is None else acc).view(np.int64)) if with_acc else None
    a.acc = accd.data_ptr() if with_acc else None
    L.check(L.lib().vbnn_conformal_interval(Context.get().h, C.byref(a)))
    got = {k: v.get() for k, v in outs.items()}
    if with_acc:
        got["acc"] = host(accd).view(np.uint64)
    return got


def assert_equals(got, want, what):
    for k in got:
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_kernel_equals_the_restatement(D):
    """Every D x R in both modes; the layout, the number of thresholds, the plane pairs, the scale form and the scope rotate so
    that every D sees every layout, Q = 1, 3 and 8, P = 1 and P = Q."""
    for i, R in enumerate((1, 3, 5, 64, 257)):
        rng = np.random.default_rng(1000 * D + R)
        Q = (1, 3, 8, 3, 8)[(i + D) % 5]
        cqr = (i + D) % 2 == 1
        P = Q if cqr else 1
        form = "none" if cqr else FORMS[(i + D) % 5]
        layout = LAYOUTS[(i + D) % 4]
        per_column = (i + D // 2) % 3 != 0
        gap = 8 if (i % 2 and layout != "odd") else (3 if layout == "odd" else 0)
        a, b = planes(P, R, D, rng, cqr)
        if not cqr:
            b = a
        t = (a[0] + rng.standard_normal((R, D)) * 0.8).astype(F32)
        s1, s2, add, isv, wmin, w = scale_inputs(form, R, D, rng)
        fin = (s1, s2, add, isv, wmin)
        want_s = score32(a, b, t, w)
        got_s = run_interval(a, b, t, None, fin, layout=layout, plane_gap=gap)
        assert_equals(got_s, want_s, (D, R, "score", form, layout))
        q = thresholds(want_s["score"], Q, per_column, rng)
        want = interval32(a, b, q, t, w, per_column)
        got = run_interval(a, b, t, q, fin, per_column=per_column, layout=layout, plane_gap=gap)
        assert_equals(got, want, (D, R, Q, P, form, layout, per_column))
        # covered follows the score: the same bytes from the score plane and the thresholds alone
        qq = np.where(np.isnan(q), F32(np.inf), q).reshape(Q, 1, -1)
        sc = want_s["score"] if P > 1 else np.broadcast_to(want_s["score"], (Q, R, D))
        assert np.array_equal(got["covered"] == 1, sc <= qq)
        assert int(got["acc"][8 * Q]) == 0 and all(int(got["acc"][8 * j]) == R * D and int(got["acc"][8 * j + 2]) == R for j in range(Q))


@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("D", [17, 64, 257])
def test_every_layout_plane_stride_and_threshold_count(D, Q):
    R = 5
    rng = np.random.default_rng(D + Q)
    for P in (1, Q):
        a, b = planes(P, R, D, rng, P > 1 or Q == 3)
        t = (a[0] + rng.standard_normal((R, D))).astype(F32)
        s1, s2, add, isv, wmin, w = scale_inputs("var2" if P == 1 else "none", R, D, rng)
        fin = (s1, s2, add, isv, wmin)
        q = thresholds(score32(a, b, t, w)["score"], Q, True, rng)
        want, want_s = interval32(a, b, q, t, w), score32(a, b, t, w)
        for layout in LAYOUTS:
            for gap in ((0,) if P == 1 else (0, 12 if layout != "odd" else 5)):
                assert_equals(run_interval(a, b, t, q, fin, layout=layout, plane_gap=gap), want, (D, Q, P, layout, gap))
                assert_equals(run_interval(a, b, t, None, fin, layout=layout, plane_gap=gap), want_s, (D, Q, P, layout, gap))
        # outputs off their aligned bases under aligned inputs (D = 64: 16-byte loads, 4-byte stores, covered byte by byte)
        assert_equals(run_interval(a, b, t, q, fin, out_shift=1), want, (D, Q, P, "outputs shifted"))
        assert_equals(run_interval(a, b, t, None, fin, out_shift=1), want_s, (D, Q, P, "outputs shifted"))


@pytest.mark.parametrize("D", [3, 20, 300])
def test_nan_elements_in_each_input_change_nothing_else(D):
    R, Q = 9, 3
    rng = np.random.default_rng(D)
    a, _ = planes(1, R, D, rng, False)
    t = (a[0] + rng.standard_normal((R, D))).astype(F32)
    s1, s2, add, isv, wmin, w = scale_inputs("var2", R, D, rng)
    q = thresholds(score32(a, a, t, w)["score"], Q, True, rng)
    clean = run_interval(a, a, t, q, (s1, s2, add, isv, wmin))
    neg_nan = np.array([0xFFFFFFFF], np.uint32).view(F32)[0]                # a NaN with its sign set is a NaN
    for which in ("lower", "scale", "scale2", "target", "negative variance"):
        A, S1, S2, T = a.copy(), s1.copy(), s2.copy(), t.copy()
        r, d = 4, D // 2
        if which == "lower":
            A[0, r, d] = np.nan
        elif which == "scale":
            S1[r, d] = neg_nan
        elif which == "scale2":
            S2[r, d] = np.nan
        elif which == "target":
            T[r, d] = np.nan
        else:
            S1[r, d] = -100.0                                # the root of a negative sum is a NaN width
        W = width32(S1, S2, add, True, wmin)
        got = run_interval(A, A, T, q, (S1, S2, add, isv, wmin))
        assert_equals(got, interval32(A, A, q, T, W), which)
        gs = run_interval(A, A, T, None, (S1, S2, add, isv, wmin))
        assert_equals(gs, score32(A, A, T, W), which)
        assert gs["score"].view(np.uint32)[0, r, d] == QNAN_BITS and gs["row_score"].view(np.uint32)[0, r] == QNAN_BITS
        assert gs["acc"].tolist() == [1, 1]
        keep = np.ones((R, D), bool)
        keep[r, d] = False
        for k in ("lo", "hi", "covered"):
            assert same_bits(got[k][:, keep], clean[k][:, keep]), (which, k)
            assert (got[k][:, r, d] == 255).all() if k == "covered" else (got[k].view(np.uint32)[:, r, d] == QNAN_BITS).all()
        rows = np.arange(R) != r
        assert same_bits(got["row_covered"][:, rows], clean["row_covered"][:, rows]) and (got["row_covered"][:, r] == -1).all()
        assert [int(v) for v in got["acc"][8 * Q:]] == [1, 1]
        assert all(int(got["acc"][8 * j]) == R * D - 1 and int(got["acc"][8 * j + 2]) == R - 1 for j in range(Q))


@pytest.mark.parametrize("D", [3, 20, 300])
def test_a_nan_in_the_upper_plane_of_one_level(D):
    """Distinct lower and upper planes, a pair per level (P = Q): a NaN in `upper` alone, at one level, is that level's NaN
    element -- with a target (t - b is NaN), without one (b itself), and in score mode -- and the NaN words count over the pairs."""
    R, Q = 9, 3
    rng = np.random.default_rng(D + 7)
    a, b = planes(Q, R, D, rng, True)
    t = (a[0] + rng.standard_normal((R, D))).astype(F32)
    q = thresholds(score32(a, b, t)["score"], Q, True, rng)
    clean, clean_blind, clean_s = run_interval(a, b, t, q), run_interval(a, b, None, q), run_interval(a, b, t, None)
    B = b.copy()
    r, d = 4, D // 2
    B[1, r, d] = np.nan
    got, blind, gs = run_interval(a, B, t, q), run_interval(a, B, None, q), run_interval(a, B, t, None)
    assert_equals(got, interval32(a, B, q, t), "target")
    assert_equals(blind, interval32(a, B, q), "no target")
    assert_equals(gs, score32(a, B, t), "score mode")
    keep = np.ones((Q, R, D), bool)
    keep[1, r, d] = False
    for k in ("lo", "hi", "covered"):
        assert same_bits(got[k][keep], clean[k][keep]), k
    for k in ("lo", "hi"):
        assert same_bits(blind[k][keep], clean_blind[k][keep]), k
        assert got[k].view(np.uint32)[1, r, d] == QNAN_BITS and blind[k].view(np.uint32)[1, r, d] == QNAN_BITS
    assert same_bits(gs["score"][keep], clean_s["score"][keep]) and gs["score"].view(np.uint32)[1, r, d] == QNAN_BITS
    rows = np.ones((Q, R), bool)
    rows[1, r] = False
    assert same_bits(got["row_covered"][rows], clean["row_covered"][rows]) and got["row_covered"][1, r] == -1 and got["covered"][1, r, d] == 255
    assert same_bits(gs["row_score"][rows], clean_s["row_score"][rows]) and gs["row_score"].view(np.uint32)[1, r] == QNAN_BITS
    for out in (got, blind):
        assert [int(v) for v in out["acc"][8 * Q:]] == [1, 1]
        assert [int(out["acc"][8 * j]) for j in range(Q)] == [R * D, R * D - 1, R * D]
        assert [int(out["acc"][8 * j + 2]) for j in range(Q)] == [R, R - 1, R]
    assert gs["acc"].tolist() == [1, 1]
    B[2, 0, 0] = np.nan                                      # a second pair: the NaN words count over the P pairs
    assert_equals(run_interval(a, B, t, q), interval32(a, B, q, t), "two pairs")
    assert [int(v) for v in run_interval(a, B, t, q)["acc"][8 * Q:]] == [2, 2] and run_interval(a, B, t, None)["acc"].tolist() == [2, 2]


@pytest.mark.parametrize("Q", [1, 3])
def test_special_thresholds_in_every_instantiation(Q):
    """+inf, NaN (taken as +inf), a negative threshold and 0, per column and one per level, for one threshold and for three."""
    R, D = 7, 21
    rng = np.random.default_rng(Q)
    a, b = planes(1, R, D, rng, True)
    t = (a[0] + rng.standard_normal((R, D))).astype(F32)
    s1, s2, add, isv, wmin, w = scale_inputs("var", R, D, rng)
    for v in (np.inf, np.nan, -0.25, 0.0):
        for per_column in (True, False):
            q = np.full((Q, D) if per_column else (Q,), v, F32)
            if per_column:
                q[:, ::3] = score32(a, b, t, w)["score"][0, 2, ::3]
            want = interval32(a, b, q, t, w, per_column)
            got = run_interval(a, b, t, q, (s1, s2, add, isv, wmin), per_column=per_column)
            assert_equals(got, want, (Q, v, per_column))
            if not per_column:
                assert int(got["acc"][1]) == (R * D if not v < np.inf else int((score32(a, b, t, w)["score"][0] <= v).sum()))


@pytest.mark.parametrize("D", [10, 300])
def test_acc_does_not_depend_on_the_calls_or_the_outputs(D):
    R, Q = 257, 3
    rng = np.random.default_rng(D)
    a, b = planes(Q, R, D, rng, True)
    t = (a[0] + rng.standard_normal((R, D))).astype(F32)
    q = thresholds(score32(a, b, t)["score"], Q, True, rng)
    q[2] = -0.5                                              # shrinks: some intervals are empty
    want = interval32(a, b, q, t)
    assert int(want["acc"][8 * 2 + 4]) > 0
    assert same_bits(run_interval(a, b, t, q)["acc"], want["acc"])
    acc = None
    for lo, hi in ((0, 100), (100, 101), (101, R)):          # three calls: the same words
        acc = run_interval(a[:, lo:hi], b[:, lo:hi], t[lo:hi], q, acc=acc)["acc"]
    assert same_bits(acc, want["acc"])
    for k in ("lo", "hi", "covered", "row_covered"):         # every optional output NULL in turn
        got = run_interval(a, b, t, q, skip=(k,))
        assert k not in got
        assert_equals(got, want, ("skip", k))
    bare = run_interval(a, b, t, q, skip=("lo", "hi", "covered", "row_covered"))
    assert list(bare) == ["acc"] and same_bits(bare["acc"], want["acc"])
    assert_equals(run_interval(a, b, t, q, with_acc=False), want, "acc NULL")
    blind = run_interval(a, b, None, q)                      # no targets: words 1 and 3 untouched
    wb = interval32(a, b, q)
    assert same_bits(blind["acc"], wb["acc"]) and all(int(blind["acc"][8 * j + w]) == 0 for j in range(Q) for w in (1, 3))
    assert same_bits(blind["lo"], want["lo"]) and same_bits(blind["hi"], want["hi"])
    want_s = score32(a, b, t)
    for k in ("score", "row_score"):
        got = run_interval(a, b, t, None, skip=(k,))
        assert k not in got
        assert_equals(got, want_s, ("skip", k))


def test_argument_checks():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _p
    m, t, q = (torch.zeros(4, 5, device="cuda") for _ in range(3))
    lo = torch.full((2, 4, 5), -7.0, device="cuda")
    acc = torch.zeros(18, dtype=torch.int64, device="cuda")
    good = dict(lower=_p(m), upper=_p(m), ld=5, P=1, Q=2, scale=_p(t), ld_s=5, scale_is_variance=1, w_min=0.5, per_column=1,
                target=_p(t), ld_t=5, R=4, D=5, qhat=_p(q), ld_qhat=5, lo=_p(lo), acc=_p(acc))
    bad = [dict(P=0), dict(P=9), dict(Q=9), dict(Q=-1), dict(P=3), dict(qhat=None), dict(target=None, covered=_p(lo)), dict(Q=0),
           dict(score=_p(lo)), dict(scale=None, scale2=_p(t)), dict(w_min=0.0), dict(R=0), dict(D=0), dict(ld=4), dict(ld_s=4),
           dict(ld_t=4), dict(ld_qhat=4), dict(R=1 << 31), dict(lower=m.data_ptr() + 2), dict(acc=acc.data_ptr() + 4), dict(lower=None)]
    for change in bad:
        a = L.ConformalIntervalArgs(**{**good, **change})
        with pytest.raises(L.VbnnError):
            L.check(L.lib().vbnn_conformal_interval(Context.get().h, C.byref(a)))
    assert (host(lo) == -7).all() and (host(acc) == 0).all()                # nothing written
    L.check(L.lib().vbnn_conformal_interval(Context.get().h, C.byref(L.ConformalIntervalArgs(**good))))
    assert (host(lo) == 0).all() and host(acc)[0] == 20
    x, tau = torch.zeros(4, 5, device="cuda"), torch.full((2, 5), -7.0, device="cuda")
    good = dict(x=_p(x), ld=5, R=4, D=5, Q=2, tau=_p(tau), ld_tau=5)
    for change in (dict(Q=0), dict(Q=9), dict(R=0), dict(D=0), dict(ld=4), dict(ld_tau=4), dict(x=None), dict(tau=None), "k0", "k5"):
        a = L.SelectColumnsArgs(**{**good, **(change if isinstance(change, dict) else {})})
        a.k[0], a.k[1] = 1, {"k0": 0, "k5": 5}.get(change if isinstance(change, str) else "", 4)
        with pytest.raises(L.VbnnError):
            L.check(L.lib().vbnn_select_columns(Context.get().h, C.byref(a)))
    assert (host(tau) == -7).all()


# ------------------------------------------------------------------------------------------------ the column select
def special_columns(R, D, rng):
    """Random, heavily tied (eighths), all-equal, and NaN / +-inf / -0 / +0 / subnormal columns, in rotation."""
    x = rng.standard_normal((R, D)).astype(F32)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-41, -1e-41, 1.0, -1.0], F32)
    for d in range(D):
        kind = d % 4
        if kind == 1:
            x[:, d] = np.round(x[:, d] * 8) / 8
        elif kind == 2:
            x[:, d] = F32(0.375) if d % 8 == 2 else F32(np.nan)
        elif kind == 3:
            x[:, d] = rng.choice(pool, R)
    return x


def run_select(x, ks, layout="dense", skip=()):
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    R, D = x.shape
    buf, ptr, ld, _ = upload(x, layout)
    Q = len(ks)
    ld_tau = D + (3 if layout in ("odd", "padded") else 0)
    outs = dict(tau=Out((Q, ld_tau), torch.float32), counts=Out((Q, D, 2), torch.int32), n_nan=Out((D,), torch.int32))
    outs = {k: v for k, v in outs.items() if k not in skip}
    a = L.SelectColumnsArgs(x=ptr, ld=ld, R=R, D=D, Q=Q, ld_tau=ld_tau, **{k: v.ptr for k, v in outs.items()})
    for j, k in enumerate(ks):
        a.k[j] = k
    L.check(L.lib().vbnn_select_columns(Context.get().h, C.byref(a)))
    got = {k: v.get() for k, v in outs.items()}
    assert np.isnan(got["tau"][:, D:]).all()                 # the pad of tau's rows is not written
    got["tau"] = got["tau"][:, :D]
    return {k: (v.view(np.uint32) if k != "tau" else v) for k, v in got.items()}


@pytest.mark.parametrize("R", [1, 2, 3, 255, 256, 257, 1000, 5000])
def test_select_columns_equals_the_sort(R):
    for i, D in enumerate((1, 2, 15, 16, 17, 33, 257)):
        rng = np.random.default_rng(100 * R + D)
        x = special_columns(R, D, rng)
        ranks = [[1], [R], [(R + 1) // 2], [(R + 1) // 2, 1, (R + 1) // 2], sorted({max(1, (R * j) // 8) for j in range(1, 9)}),
                 [R, 1], [1 + (R * 9) // 10, 1 + (R * 19) // 20, 1 + R // 2, 1 + R // 3, 1 + R // 5, 1, R, 1 + R // 7]][(i + R) % 7]
        ranks = [min(k, R) for k in ranks]
        layout = LAYOUTS[(i + R) % 4]
        assert_equals(run_select(x, ranks, layout), select_columns32(x, ranks), (R, D, ranks, layout))
    x = special_columns(R, 33, np.random.default_rng(R))
    ranks = [min(R, k) for k in (1, 2, 3, 5, 8, 13, 21, 34)]                # 8 distinct
    want = select_columns32(x, ranks)
    assert_equals(run_select(x, ranks), want, "8 ranks")
    got = run_select(x, ranks, skip=("counts", "n_nan"))
    assert list(got) == ["tau"] and same_bits(got["tau"], want["tau"])


# ------------------------------------------------------------------------------------------------ the engine
def opt_for(criterion, D, **kw):
    o = dict(var_init=1e-2, mu_init=1, B=1e6, S=1, mode="lrt", dtype="f32", seed=3, input_size=16, hidden=[32, 32],
             n_classes=2 * D if criterion == "gauss" else D, criterion=criterion, type="vb", testSamples=4)
    o.update(kw)
    return o


def regression_set(R, D, seed=5, noise=0.5):
    """A heteroscedastic regression set of this file's own: vbnn_amd/data.py has no regression stand-in (synthetic_digits is its
    only generator), so the engine-level tests, the n = 999 / m = 1000 split included, draw from this one. The CPU pre-check of
    that split's bound (tests/test_interval_ref.py) runs the restatement on a set of the same kind, not on these rows."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, 16)).astype(F32)
    w = rng.standard_normal((16, D)).astype(F32) / 4
    t = np.tanh(x @ w) + noise * (0.3 + np.abs(x[:, :1])) * rng.standard_normal((R, D))
    return dev(x), dev(t.astype(F32))


def restated(res, t, levels, score, scope, noise_var=None, cal_rows=None):
    """The restatement fed the engine's own result tensors: (calibration scores, qhat, k, interval dict) -- calibrated on the
    rows cal_rows (default: all), intervals for all rows."""
    mom = getattr(res, "moments", res)
    tt = host(t)
    if score == "cqr":
        qs = host(res.quantiles)
        idx = [(res.probs.index(float(F32((1 - l) / 2))), res.probs.index(float(F32((1 + l) / 2)))) for l in levels]
        a, b, w = np.stack([qs[i] for i, _ in idx]), np.stack([qs[j] for _, j in idx]), None
    else:
        a = b = host(mom.mean)[None]
        w = None
        if score == "scaled":
            w = width32(host(mom.var), host(mom.noise_var) if mom.noise_var is not None else None, noise_var or 0.0, True, W_MIN)
    rows = slice(None) if cal_rows is None else cal_rows
    sc = score32(a[:, rows], b[:, rows], tt[rows], None if w is None else w[rows])
    key = "row_score" if scope == "joint" else "score"
    if len(a) > 1:
        qk = [calibrate32(sc[key][j], [l], scope) for j, l in enumerate(levels)]
        qhat, k = np.concatenate([v[0] for v in qk]), [v[1][0] for v in qk]
    else:
        qhat, k = calibrate32(sc[key][0], levels, scope)
    out = interval32(a, b, qhat if scope == "per_output" else qhat[:, 0], tt, w, scope == "per_output")
    return sc[key], qhat, k, out


def check_engine(eng, res, t, levels, score, scope, noise_var=None):
    from vbnn_amd.engine import IntervalCalibration, IntervalResult
    cal = eng.conformal_calibrate_intervals(res, t, levels=levels, score=score, scope=scope, noise_var=noise_var)
    assert isinstance(cal, IntervalCalibration)
    s, qhat, k, want = restated(res, t, levels, score, scope, noise_var)
    R, D = t.shape
    assert (cal.n, cal.k, cal.D, cal.score, cal.scope, cal.n_nan) == (R, k, D, score, scope, 0)
    assert same_bits(host(cal.scores), s) and same_bits(host(cal.qhat_dev), qhat)
    out = eng.conformal_intervals(res, cal, targets=t, keep_covered=True)
    assert isinstance(out, IntervalResult)
    for key in ("lo", "hi", "covered", "row_covered"):
        assert same_bits(host(getattr(out, key)), want[key]), key
    assert out.counts() == [int(v) for v in want["acc"]]
    Q = len(levels)
    for j in range(Q):
        c = out.counts()[8 * j:8 * j + 5]
        assert out.coverage[j] == c[1] / c[0] and out.joint_coverage[j] == c[3] / c[2] and out.empty_fraction[j] == c[4] / c[0]
        if scope == "per_output":                            # every output's own k-th score is at or below its threshold
            assert (want["covered"][j].sum(0) >= min(k[j], R)).all()
        else:
            assert c[3] >= min(k[j], R)
    width = (want["hi"].astype(np.float64) - want["lo"].astype(np.float64)).reshape(Q, -1).mean(1)
    assert np.allclose(out.mean_width, width, rtol=1e-12, atol=0) or np.isinf(width).any()
    assert np.array_equal(np.array(out.coverage_per_output), (want["covered"] == 1).mean(1))
    return cal, out


@pytest.mark.parametrize("scope", ["per_output", "joint"])
@pytest.mark.parametrize("name", ["mse sampled", "mse analytic", "gauss", "cqr"])
def test_engine_equals_the_restatement(name, scope):
    from vbnn_amd.conformal import _RowSlice
    from vbnn_amd.engine import FusedMLP
    R, D, levels = 300, 5, (0.5, 0.9, 0.99)
    crit = "gauss" if name == "gauss" else "mse"
    eng = FusedMLP(opt_for(crit, D))
    x, t = regression_set(R, D)
    nv = None
    if name == "mse sampled":
        res, score, nv = eng.predict_regression(x, S=6, targets=t, noise_var=0.25), "scaled", 0.25
    elif name == "mse analytic":
        res, score = eng.predict_analytic(x, targets=t), "scaled"
    elif name == "gauss":
        res, score = eng.predict_regression(x, S=6, targets=t), "scaled"
    else:
        res, score, levels = eng.predict_quantiles(x, (0.005, 0.05, 0.25, 0.75, 0.95, 0.995), S=8, targets=t, noise_var=0.25), "cqr", (0.5, 0.9, 0.99)
    cal, out = check_engine(eng, res, t, levels, score, scope, nv)
    if name == "mse sampled":
        check_engine(eng, res, t, (0.8,), "absolute", scope)
    # a list of results is the one concatenated result; into= over three minibatches is the one call; merge() adds
    cuts = ((0, 130), (130, 131), (131, R))
    pieces, ts = [_RowSlice(res, lo, hi) for lo, hi in cuts], [t[lo:hi] for lo, hi in cuts]
    cal2 = eng.conformal_calibrate_intervals(pieces, ts, levels=levels, score=score, scope=scope, noise_var=nv)
    assert torch.equal(cal2.qhat_dev, cal.qhat_dev) and torch.equal(cal2.scores, cal.scores) and cal2.k == cal.k
    acc, parts = None, []
    for p, tp in zip(pieces, ts):
        acc = eng.conformal_intervals(p, cal, targets=tp, keep_covered=True, into=acc)
        parts.append(eng.conformal_intervals(p, cal, targets=tp))
    assert acc.counts() == out.counts() and torch.equal(acc.lo, out.lo) and torch.equal(acc.covered, out.covered)
    merged = parts[0].merge(parts[1]).merge(parts[2])
    assert merged.counts() == out.counts() and merged.coverage == out.coverage and torch.equal(merged.hi, out.hi)
    blind = eng.conformal_intervals(res, cal)
    assert blind.row_covered is None and all(v != v for v in blind.coverage) and torch.equal(blind.lo, out.lo)
    # a level whose rank is past the calibration set: +inf on the device
    few = eng.conformal_calibrate_intervals(_RowSlice(res, 0, 5), t[:5], levels=levels[:2], score=score, scope=scope, noise_var=nv)
    assert few.k == [3, 6] and all(v == float("inf") for v in few.qhat[1]) and all(v < float("inf") for v in few.qhat[0])
    assert eng.conformal_intervals(res, few, targets=t).coverage[1] == 1.0


def test_engine_on_a_compact_and_a_pruned_network():
    from vbnn_amd.engine import FusedMLP
    R, D = 200, 3
    x, t = regression_set(R, D)
    eng = FusedMLP(opt_for("mse", D))
    with eng.pruned(eng.prune(fraction=0.5)):                # a pruned view
        res = eng.predict_regression(x, S=4, targets=t)
    check_engine(eng, res, t, (0.9,), "scaled", "per_output")
    big = FusedMLP(opt_for("mse", D))
    small = big.compact(big.prune_units(fraction=0.25))
    check_engine(small, small.predict_regression(x, S=4, targets=t), t, (0.9,), "scaled", "joint")


class Reg:
    """A regression result as far as the interval calls look at one."""
    def __init__(self, mean, var, noise_var=None):
        self.mean, self.var, self.noise_var = mean, var, noise_var


def test_engine_refusals_that_need_device_tensors():
    """What conformal_intervals compares once it has the planes -- D, the probabilities, the thresholds' shape, into= -- and the
    dtype, rank, shape and device of tensors that ARE on a device."""
    import copy
    from vbnn_amd.engine import FusedMLP
    R, D = 40, 5
    eng = FusedMLP(opt_for("mse", D))
    x, t = regression_set(R, D)
    res = eng.predict_regression(x, S=3, targets=t)
    cal = eng.conformal_calibrate_intervals(res, t, levels=(0.5, 0.9))
    out = eng.conformal_intervals(res, cal, targets=t)
    before = out.counts()
    # a calibration that does not match the result
    three = FusedMLP(opt_for("mse", 3))
    x3, t3 = regression_set(R, 3)
    with pytest.raises(ValueError, match="D = 5 outputs, the result has 3"):
        three.conformal_intervals(three.predict_regression(x3, S=2), cal)
    bad = copy.copy(cal)
    bad.scope = "joint"                                      # (its thresholds are Q x D, a joint calibration's Q x 1)
    with pytest.raises(ValueError, match="2 x 1 thresholds"):
        eng.conformal_intervals(res, bad)
    qres = eng.predict_quantiles(x, (0.05, 0.25, 0.75, 0.95), S=4, targets=t)
    calq = eng.conformal_calibrate_intervals(qres, t, levels=(0.9,), score="cqr")
    assert calq.probs == [(qres.probs[0], qres.probs[3])]
    with pytest.raises(ValueError, match=r"0\.05 and 0\.95"):       # a quantile result without the calibration's probabilities
        eng.conformal_intervals(eng.predict_quantiles(x, (0.1, 0.9), S=4), calq)
    bad = copy.copy(calq)
    bad.probs = [(qres.probs[1], qres.probs[2])]
    with pytest.raises(ValueError, match="probs"):
        eng.conformal_intervals(qres, bad)
    with pytest.raises(ValueError, match="QuantilePredictResult"):
        eng.conformal_intervals(res, calq)
    # into=: other levels, other outputs, a merged result, made without / with targets
    other = eng.conformal_intervals(res, eng.conformal_calibrate_intervals(res, t, levels=(0.8,)), targets=t)
    with pytest.raises(ValueError, match="same levels and outputs"):
        eng.conformal_intervals(res, cal, targets=t, into=other)
    with pytest.raises(ValueError, match="same levels and outputs"):
        eng.conformal_intervals(res, cal, targets=t, into=object())
    with pytest.raises(ValueError, match="merged"):
        eng.conformal_intervals(res, cal, targets=t, into=out.merge(out))
    blind = eng.conformal_intervals(res, cal)
    with pytest.raises(ValueError, match="made without targets"):
        eng.conformal_intervals(res, cal, targets=t, into=blind)
    with pytest.raises(ValueError, match="made with targets"):
        eng.conformal_intervals(res, cal, into=out)
    with pytest.raises(ValueError, match="keep_covered needs targets"):
        eng.conformal_intervals(res, cal, keep_covered=True)
    assert out.counts() == before and out.lo.shape[1] == R   # a refused call added nothing
    # tensors on the device of the wrong dtype, rank or shape; targets of another shape or on the host
    with pytest.raises(ValueError, match="float64"):
        eng.conformal_calibrate_intervals(Reg(res.mean.double(), res.var), t)
    with pytest.raises(ValueError, match="float64"):
        eng.conformal_calibrate_intervals(Reg(res.mean, res.var.double()), t)
    with pytest.raises(ValueError, match=r"got \(5,\)"):
        eng.conformal_calibrate_intervals(Reg(res.mean[0], res.var), t)
    with pytest.raises(ValueError, match=r"var is \(39, 5\), expected R x D = 40 x 5"):
        eng.conformal_calibrate_intervals(Reg(res.mean, res.var[:39]), t)
    with pytest.raises(ValueError, match=r"targets is \(40, 3\), expected R x D = 40 x 5"):
        eng.conformal_calibrate_intervals(res, t[:, :3])
    with pytest.raises(ValueError, match=r"targets is \(39, 5\)"):
        eng.conformal_intervals(res, cal, targets=t[:39])
    with pytest.raises(ValueError, match="on cpu"):
        eng.conformal_calibrate_intervals(res, t.cpu())
    with pytest.raises(ValueError, match="int32"):
        eng.conformal_calibrate_intervals(res, t.to(torch.int32))
    with pytest.raises(ValueError, match="differ in device or width"):
        eng.conformal_calibrate_intervals([res, Reg(res.mean[:, :3], res.var[:, :3])], [t, t[:, :3]])


@pytest.mark.parametrize("scope", ["per_output", "joint"])
def test_levels_whose_ranks_inside_the_set_are_not_neighbours(scope):
    """n = 5 with levels 0.5, 0.99, 0.6: k = 3, 6, 4 -- the middle one is past the set (+inf), the select's two thresholds go to
    rows 0 and 2 of the thresholds."""
    from vbnn_amd.conformal import _RowSlice
    from vbnn_amd.engine import FusedMLP
    eng = FusedMLP(opt_for("mse", 4))
    x, t = regression_set(5, 4)
    res = eng.predict_regression(x, S=3, targets=t, noise_var=0.25)
    cal, out = check_engine(eng, _RowSlice(res, 0, 5), t, (0.5, 0.99, 0.6), "scaled", scope, 0.25)
    assert cal.k == [3, 6, 4]
    q = np.array(cal.qhat, F32)
    assert np.isposinf(q[1]).all() and np.isfinite(q[[0, 2]]).all() and (q[0] <= q[2]).all()
    assert out.coverage[1] == 1.0


def test_an_over_confident_predictive_is_repaired():
    """One split, n = 999 calibration and m = 1000 test rows, a MAP-collapsed predictive with a small fixed noise: the nominal 90 %
    interval covers far less, the conformal one at least 0.9 - 5 sqrt(ab / ((a + b)^2 (a + b + 1)) + 0.09 / m) = 0.9 - 0.067
    (a = k = 900, b = n + 1 - k = 100: the Beta spread of the split plus the binomial spread of the test rows)."""
    from vbnn_amd.conformal import _RowSlice
    from vbnn_amd.engine import FusedMLP
    n, m, D = 999, 1000, 3
    x, t = regression_set(n + m, D, seed=11)
    eng = FusedMLP(opt_for("mse", D))
    res = eng.predict_quantiles(x, (0.05, 0.95), S=2, targets=t, noise_var=1e-3, map=True)
    test = eng.predict_quantiles(x[n:], (0.05, 0.95), S=2, targets=t[n:], noise_var=1e-3, map=True)
    nominal = test.interval(0.9)[2]
    a, b = 900, 100
    bound = 0.9 - 5 * (a * b / ((a + b) ** 2 * (a + b + 1)) + 0.09 / m) ** 0.5
    assert abs(bound - (0.9 - 0.067)) < 1e-3
    for score, scope, nv in (("scaled", "per_output", 1e-3), ("cqr", "per_output", None), ("scaled", "joint", 1e-3)):
        cal = eng.conformal_calibrate_intervals(_RowSlice(res, 0, n), t[:n], levels=(0.9,), score=score, scope=scope, noise_var=nv)
        assert cal.k == [conformal_rank(n, 0.9)] == [900]
        out = eng.conformal_intervals(_RowSlice(res, n, n + m), cal, targets=t[n:])
        cov = out.joint_coverage[0] if scope == "joint" else out.coverage[0]
        print(score, scope, "nominal", nominal, "conformal", cov, "bound", bound)
        assert nominal < cov and cov >= bound
        _, _, _, want = restated(res, t, (0.9,), score, scope, nv, cal_rows=slice(0, n))
        assert out.counts()[1] == int((want["covered"][0, n:] == 1).sum())


def test_trainer_series_appear_only_when_switched_on(tmp_path):
    from vbnn_amd.data import Dataset
    from vbnn_amd.train import Main, default_opt
    rng = np.random.default_rng(4)
    n, D = 128, 3
    ds = Dataset(inputs=rng.standard_normal((n, 4, 4)).astype(F32), targets=rng.standard_normal((n, D)).astype(F32))
    base = dict(hidden=[24], input_size=16, geometry=(4, 4), testBatchSize=32, testSize=n, batchSize=32, trainSize=n, testSamples=3,
                S=1, log=False, predictive=True, var_init=1e-2)
    for crit, extra, ci in (("mse", dict(noise_var=0.5), {}), ("gauss", {}, dict(conformal_interval_scope="joint")),
                            ("mse", dict(quantile_probs=[0.05, 0.1, 0.9, 0.95]), dict(conformal_interval_score="cqr")),
                            ("mse", dict(predictive="analytic"), dict(conformal_interval_score="absolute"))):
        kw = {**base, **dict(criterion=crit, n_classes=2 * D if crit == "gauss" else D), **extra}
        plain = Main(default_opt(conformal_levels=[0.9], **kw))             # (conformal_levels keeps ignoring regression engines)
        on = Main(default_opt(conformal_interval_levels=[0.8, 0.9], **ci, **kw))
        plain.test(ds)
        on.test(ds)
        new = {"dev_icov@0.8", "dev_icov@0.9", "dev_iwidth@0.8", "dev_iwidth@0.9"}
        assert not any(k.startswith(("dev_icov@", "dev_iwidth@", "dev_cov@")) for k in plain.predictive)
        assert set(on.predictive) == set(plain.predictive) | new
        for k, v in plain.predictive.items():                # the existing series: exactly what they were
            assert on.predictive[k] == v, k
        assert all(0.0 <= on.predictive[f"dev_icov@{l}"] <= 1.0 and on.predictive[f"dev_iwidth@{l}"] >= 0.0 for l in ("0.8", "0.9"))
        if ci.get("conformal_interval_score") != "cqr":      # one plane pair: a larger rank is a larger threshold on every output
            assert on.predictive["dev_icov@0.8"] <= on.predictive["dev_icov@0.9"]
            assert on.predictive["dev_iwidth@0.8"] <= on.predictive["dev_iwidth@0.9"]
        assert on.net.draw == plain.net.draw
    with pytest.raises(ValueError, match="0.05"):
        Main(default_opt(conformal_interval_levels=[0.9], conformal_interval_score="cqr", quantile_probs=[0.1, 0.95],
                         **{**base, "criterion": "mse", "n_classes": D})).test(ds)
    import os
    from vbnn_amd.logger import read_data
    d = str(tmp_path / "on")
    m = Main(default_opt(criterion="mse", n_classes=D, network_name=d, conformal_interval_levels=[0.9], **{**base, "log": True}))
    rec = m.run(ds, ds, epochs=1)[-1]
    m.log.close()
    for series in ("dev_icov@0.9", "dev_iwidth@0.9"):
        assert read_data(os.path.join(d, series)) == [pytest.approx(rec[series], rel=1e-6)]
