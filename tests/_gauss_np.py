"""Float64 NumPy restatements for the heteroscedastic Gaussian head's tests: the criterion vbnn_gauss_nll_forward computes
(loss without its 0.5 log 2 pi constant, the two gradient halves) and the moments vbnn_predict_gauss_moments forms, with the
bounds their tests hold them to. A row of y is { m[D], s[D] }, s the log of the noise variance; every function takes the fp32
inputs the kernel saw and evaluates in float64."""
import numpy as np

from tests._regress_np import EPS, mean_tol, moments64, var_tol

LOG_2PI = float(np.log(2.0 * np.pi))


def split(y):
    """(m, s) in float64 from y (.. x 2 D)."""
    D = y.shape[-1] // 2
    y = np.asarray(y, dtype=np.float64)
    return y[..., :D], y[..., D:]


def clamp(s, s_min, s_max):
    """min(max(s, s_min), s_max) with the fp32 clamp values; a NaN stays NaN."""
    return np.where(np.isnan(s), s, np.minimum(np.maximum(s, float(np.float32(s_min))), float(np.float32(s_max))))


def inside(s, s_min, s_max):
    """Where the clamp has a slope: not below s_min, not above s_max (a NaN counts as inside: it reaches its gradient)."""
    return ~((s < float(np.float32(s_min))) | (s > float(np.float32(s_max))))


def nll_terms(y, t, s_min, s_max):
    """Per element: (0.5 (s_c + d^2 w), its magnitude 0.5 (|s_c| + d^2 w), d^2 w, w) in float64."""
    m, s = split(y)
    sc = clamp(s, s_min, s_max)
    w = np.exp(-sc)
    d = np.asarray(t, dtype=np.float64) - m
    dw = d * d * w
    return 0.5 * (sc + dw), 0.5 * (np.abs(sc) + dw), dw, w


def criterion64(y, t, inv_nd, s_min, s_max):
    """The criterion on y (N x 2 D) and t (N x D): loss = inv_nd sum 0.5 (s_c + d^2 w), g_m = inv_nd (m - t) w,
    g_s = 0.5 inv_nd (1 - d^2 w) inside the clamp and 0 outside; and the magnitudes the bounds are stated against."""
    inv_nd = float(np.float32(inv_nd))
    m, s = split(y)
    e, mag, dw, w = nll_terms(y, t, s_min, s_max)
    g_m = inv_nd * (m - np.asarray(t, dtype=np.float64)) * w
    ins = inside(s, s_min, s_max)
    g_s = np.where(ins, 0.5 * inv_nd * (1.0 - dw), 0.0)
    return dict(loss=inv_nd * e.sum(), g_m=g_m, g_s=g_s, inside=ins, loss_mag=inv_nd * mag.sum(),
                g_s_mag=0.5 * inv_nd * (1.0 + dw))


def loss_only64(y, t, inv_nd, s_min, s_max):
    return criterion64(y, t, inv_nd, s_min, s_max)["loss"]


def check_criterion(loss, g, y, t, inv_nd, s_min, s_max, label=""):
    """loss (float) and g (N x 2 D fp32) of the kernel against criterion64 on the same fp32 inputs:
    |g_m - g_m64| <= 8 eps |g_m64|, |g_s - g_s64| <= 8 eps 0.5 inv_nd (1 + d^2 w), g_s == +0 bitwise outside the clamp,
    |loss - loss64| <= 8 eps inv_nd sum 0.5 (|s_c| + d^2 w) -- three or four fp32 roundings and a 1-ulp expf."""
    ref = criterion64(y, t, inv_nd, s_min, s_max)
    D = y.shape[1] // 2
    g_m, g_s = g[:, :D].astype(np.float64), g[:, D:].astype(np.float64)
    dm = np.abs(g_m - ref["g_m"]) / np.maximum(8 * EPS * np.abs(ref["g_m"]), 1e-300)
    ds = np.abs(g_s - ref["g_s"]) / (8 * EPS * ref["g_s_mag"])
    out = ~ref["inside"]
    print(f"{label}: g_m err/bound {dm.max():.3f}, g_s err/bound {ds.max():.3f}, clamped {int(out.sum())} of {out.size}")
    assert (np.abs(g_m - ref["g_m"]) <= 8 * EPS * np.abs(ref["g_m"])).all(), (label, float(dm.max()))
    assert (ds <= 1.0).all(), (label, float(ds.max()))
    assert not g[:, D:][out].view(np.uint32).any(), label              # exactly +0 outside the clamp
    if loss is not None:
        dl = abs(loss - ref["loss"]) / (8 * EPS * ref["loss_mag"])
        print(f"{label}: loss {loss!r} want {ref['loss']!r}, err/bound {dl:.3f}")
        assert dl <= 1.0, (label, loss, ref["loss"])
    return ref


def gauss_moments64(y, t=None, s_min=-20.0, s_max=20.0):
    """The float64 reference on fp32 inputs: y S x R x 2 D, t R x D. moments64 of the m half (mean, var, a, row_var and with t
    row_sq_err) plus noise_var = mean_s exp(s_c), row_noise_var, and with t: nll (S x R: 0.5 sum_d (s_c + d^2 w)), nll_mag
    (S x R: 0.5 sum_d (|s_c| + d^2 w)) and row_log_lik, the log density of the equal-weight mixture of N(m_s, diag exp(s_c))."""
    S, R, W = y.shape
    D = W // 2
    m, s = split(y)
    ref = moments64(m, t)
    ref["noise_var"] = np.exp(clamp(s, s_min, s_max)).mean(0)
    ref["row_noise_var"] = ref["noise_var"].mean(1)
    if t is not None:
        e, mag, _, _ = nll_terms(y, np.asarray(t, dtype=np.float64)[None], s_min, s_max)
        ref["nll"], ref["nll_mag"] = e.sum(2), mag.sum(2)
        a = -ref["nll"]
        top = a.max(0)
        ref["row_log_lik"] = top + np.log(np.exp(a - top).sum(0)) - np.log(S) - 0.5 * D * LOG_2PI
    return ref


def nll_bound(ref, D):
    """(D + 32) eps 0.5 sum_d (|s_c| + d^2 w): a D-term fp32 row sum of terms three roundings and a 1-ulp expf deep."""
    return (D + 32) * EPS * ref["nll_mag"]


def check_gauss_moments(got, y, t=None, s_min=-20.0, s_max=20.0, nll=None, extra_mean=0.0, extra_var=0.0, extra_noise=0.0,
                        label="", rows=True):
    """got: dict of NumPy arrays (mean, var, noise_var, row_var, row_noise_var and with t row_sq_err / row_log_lik / totals)
    against gauss_moments64(y, t). mean / var: tests/_regress_np.py's element bounds on the m half;
    |noise_var - v64| <= (S + 4) eps v64 (a 1-ulp expf per draw, S - 1 additions, one division) (+ extra_*: what the caller's y
    itself may be off by). nll (S x R, the kernel's own per-draw values where the caller has them): each within nll_bound.
    The row sums and their totals: relative (D + 16) eps against the float64 sum of the RETURNED fp32 terms, and against the
    all-float64 values with the terms' element bounds carried through the sum. row_log_lik: the row's largest nll bound plus
    (4 S + 16) eps max(|ll64|, 1) for the S logsumexp steps. totals[2] is the double sum of the returned rows."""
    S, R, W = y.shape
    D = W // 2
    ref = gauss_moments64(y, t, s_min, s_max)
    tm, tv = mean_tol(ref, S) + extra_mean, var_tol(ref) + extra_var
    tn = (S + 4) * EPS * ref["noise_var"] + extra_noise
    dm, dv, dn = np.abs(got["mean"] - ref["mean"]), np.abs(got["var"] - ref["var"]), np.abs(got["noise_var"] - ref["noise_var"])
    print(f"{label} S {S} R {R} D {D}: mean err/tol {np.max(dm / np.maximum(tm, 1e-300)):.3f}, var err/tol "
          f"{np.max(dv / np.maximum(tv, 1e-300)):.3f}, noise_var err/tol {np.max(dn / np.maximum(tn, 1e-300)):.3f}")
    assert (dm <= tm).all(), (label, float((dm - tm).max()))
    assert (dv <= tv).all(), (label, float((dv - tv).max()))
    assert (dn <= tn).all(), (label, float((dn - tn).max()))
    assert (got["var"] >= 0).all() and (got["noise_var"] > 0).all()
    if not rows:                                     # (y is a restatement of the forward, not the kernel's own input)
        return ref
    rel = (D + 16) * EPS
    g_mean, g_var, g_nv = (got[k].astype(np.float64) for k in ("mean", "var", "noise_var"))
    rv_terms, rn_terms = g_var.mean(1), g_nv.mean(1)
    assert (np.abs(got["row_var"] - rv_terms) <= rel * rv_terms).all(), label
    assert (np.abs(got["row_var"] - ref["row_var"]) <= rel * ref["row_var"] + tv.mean(1)).all(), label
    assert (np.abs(got["row_noise_var"] - rn_terms) <= rel * rn_terms).all(), label
    assert (np.abs(got["row_noise_var"] - ref["row_noise_var"]) <= rel * ref["row_noise_var"] + tn.mean(1)).all(), label
    if t is None:
        return ref
    t64 = t.astype(np.float64)
    sq_terms = ((t64 - g_mean) ** 2).sum(1)
    assert (np.abs(got["row_sq_err"] - sq_terms) <= rel * sq_terms).all(), label
    carried = (2 * np.abs(t64 - ref["mean"]) * tm + tm * tm).sum(1)
    assert (np.abs(got["row_sq_err"] - ref["row_sq_err"]) <= rel * ref["row_sq_err"] + carried).all(), label
    nb = nll_bound(ref, D)
    if nll is not None:
        d = np.abs(nll.astype(np.float64) - ref["nll"]) / np.maximum(nb, 1e-300)
        print(f"{label} per-draw nll: worst err/bound {d.max():.3f}")
        assert (d <= 1.0).all(), (label, float(d.max()))
    ll, want = got["row_log_lik"].astype(np.float64), ref["row_log_lik"]
    tl = nb.max(0) + (4 * S + 16) * EPS * np.maximum(np.abs(want), 1.0)
    d = np.abs(ll - want) / tl
    print(f"{label} log-lik: worst err/bound {d.max():.3f}")
    assert (d <= 1.0).all(), (label, float(d.max()))
    tot = got.get("totals")
    if tot is not None:
        assert len(tot) == 5
        want = {0: sq_terms.sum(), 3: g_var.sum(), 4: g_nv.sum()}
        for k, wv in want.items():
            print(f"{label} total {k}: {tot[k]!r} want {wv!r}")
            assert abs(tot[k] - wv) <= rel * abs(wv), (label, k, tot[k], wv)
        assert abs(tot[0] - ref["row_sq_err"].sum()) <= rel * ref["row_sq_err"].sum() + carried.sum(), label
        assert abs(tot[3] - ref["var"].sum()) <= rel * ref["var"].sum() + tv.sum(), label
        assert abs(tot[4] - ref["noise_var"].sum()) <= rel * ref["noise_var"].sum() + tn.sum(), label
        # sum_{r,s} nll_s: per row an fp32 running sum of S values, each within its bound
        t1 = nb.sum() + S * EPS * np.abs(ref["nll"]).sum()
        print(f"{label} total 1: {tot[1]!r} want {ref['nll'].sum()!r} (err/bound {abs(tot[1] - ref['nll'].sum()) / t1:.3f})")
        assert abs(tot[1] - ref["nll"].sum()) <= t1, (label, tot[1], ref["nll"].sum())
        assert abs(tot[2] - ll.sum()) <= 1e-12 * np.abs(ll).sum(), (label, tot[2], ll.sum())
    return ref
