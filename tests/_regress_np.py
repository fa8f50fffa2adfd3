"""Float64 NumPy restatements for the regression predictive's tests: the forward of one draw up to the final Linear's outputs
(tests/test_predict_gpu.py::oracle_draw without the softmax) and the moments vbnn_predict_moments forms, with the tolerances
its tests hold it to."""
import numpy as np

EPS = 2.0 ** -24
STREAM_EPS, STREAM_ZETA = 1, 2


def forward_draw(oracle, ps, w3, b3, mode, seed, x, draw, row0=0):
    """One draw's outputs y = h W3^T + b3 in float64 (LRT: the oracle's z per layer; WN: OracleVBLinear.sample's weights;
    draw None: the means) and, per row, the largest error of an output that fp32 GEMM accumulation can explain
    (|d| <= 4e-6 sum |a b| per fp32 GEMM, carried layer to layer by sum |w|). ps: [(means, lvars, bias)] in float64."""
    h, err = x.astype(np.float64), np.zeros((x.shape[0], 1))
    for li, (mu, lv, b) in enumerate(ps):
        O = mu.shape[0]
        if draw is None:
            y = h @ mu.T + b
            absprod = np.abs(h) @ np.abs(mu).T
            prop = err * np.abs(mu).sum(1)[None, :]
        elif mode == "lrt":
            z = oracle.fill_normal(h.shape[0], O, seed, STREAM_ZETA, li, draw, row0).astype(np.float64)
            var = np.exp(lv)
            m, v = h @ mu.T + b, (h * h) @ var.T
            y = m + np.sqrt(v) * z
            absprod = np.abs(h) @ np.abs(mu).T + np.sqrt(v) * np.abs(z)
            prop = (err * (np.abs(mu).sum(1)[None, :] + 2 * np.sqrt(var.max()) * np.abs(z) * np.sqrt(np.abs(h).sum(1, keepdims=True))))
        else:
            e = oracle.fill_normal(O, mu.shape[1], seed, STREAM_EPS, li, draw).astype(np.float64)
            w = mu + np.sqrt(np.exp(lv)) * e
            y = h @ w.T + b
            absprod = np.abs(h) @ np.abs(w).T
            prop = err * np.abs(w).sum(1)[None, :]
        err = 4e-6 * absprod + prop + 1e-6 * np.abs(y)
        h = np.maximum(y, 0.0)
        err = err.max(1, keepdims=True)
    y = h @ w3.T + b3
    yerr = 4e-6 * (np.abs(h) @ np.abs(w3).T).max(1, keepdims=True) + err * np.abs(w3).sum(1).max()
    return y, yerr[:, 0]


def moments64(y, t=None, noise_var=None):
    """The float64 reference on fp32 inputs: y S x R x D, t R x D. A dict of mean, var (population), a = max_s |y_s|, row_var,
    and with t: e (S x R), row_sq_err, and with noise_var: row_log_lik."""
    y = y.astype(np.float64)
    S, R, D = y.shape
    ref = dict(mean=y.mean(0), var=y.var(0), a=np.abs(y).max(0))
    ref["row_var"] = ref["var"].mean(1)
    if t is not None:
        t = t.astype(np.float64)
        ref["e"] = ((t[None] - y) ** 2).sum(2)
        ref["row_sq_err"] = ((t - ref["mean"]) ** 2).sum(1)
        if noise_var is not None:
            tau2 = float(np.float32(noise_var))
            a = -ref["e"] / (2.0 * tau2)
            m = a.max(0)
            ref["row_log_lik"] = m + np.log(np.exp(a - m).sum(0)) - np.log(S) - 0.5 * D * np.log(2.0 * np.pi * tau2)
    return ref


def mean_tol(ref, S):
    return max(4, S) * EPS * ref["a"]


def var_tol(ref):
    v, a = ref["var"], ref["a"]
    return 8 * EPS * (v + a * np.sqrt(v) + EPS * a * a)


def check_moments(got, y, t=None, noise_var=None, extra_mean=0.0, extra_var=0.0, label="", rows=True):
    """got: dict of NumPy arrays (mean, var, row_var, and with t row_sq_err / row_log_lik / totals) against moments64(y, t).
    The element bounds: |mean - mean64| <= max(4, S) eps a, |var - var64| <= 8 eps (var64 + a sqrt(var64) + eps a^2)
    (+ extra_*: what the caller's y itself may be off by). The row sums and totals are fp32 sums of D non-negative terms:
    relative (D + 16) eps against the float64 sum of THEIR terms -- (t - y_s)^2 from the inputs for e_s, and for row_sq_err and
    row_var the returned fp32 mean / var, whose own distance to float64 the element bounds above already hold (a sum cannot be
    closer to the float64 one than its terms: at y = 1000 + 1e-3 z the var bound is half of var). They are held against the
    all-float64 values too, with the terms' element bounds carried through the sum added to (D + 16) eps."""
    S, R, D = y.shape
    ref = moments64(y, t, noise_var)
    tm, tv = mean_tol(ref, S) + extra_mean, var_tol(ref) + extra_var
    dm, dv = np.abs(got["mean"] - ref["mean"]), np.abs(got["var"] - ref["var"])
    print(f"{label} S {S} R {R} D {D}: mean err/tol {np.max(dm / np.maximum(tm, 1e-300)):.3f}, var err/tol {np.max(dv / np.maximum(tv, 1e-300)):.3f}")
    assert (dm <= tm).all(), (label, float((dm - tm).max()))
    assert (dv <= tv).all(), (label, float((dv - tv).max()))
    assert (got["var"] >= 0).all()
    if not rows:                                     # (y is a restatement of the forward, not the kernel's own input)
        return ref
    rel = (D + 16) * EPS
    g_mean, g_var = got["mean"].astype(np.float64), got["var"].astype(np.float64)
    rv_terms = g_var.mean(1)
    assert (np.abs(got["row_var"] - rv_terms) <= rel * rv_terms).all(), label
    assert (np.abs(got["row_var"] - ref["row_var"]) <= rel * ref["row_var"] + tv.mean(1)).all(), label
    if t is None:
        return ref
    t64 = t.astype(np.float64)
    sq_terms = ((t64 - g_mean) ** 2).sum(1)
    assert (np.abs(got["row_sq_err"] - sq_terms) <= rel * sq_terms).all(), label
    carried = (2 * np.abs(t64 - ref["mean"]) * tm + tm * tm).sum(1)
    assert (np.abs(got["row_sq_err"] - ref["row_sq_err"]) <= rel * ref["row_sq_err"] + carried).all(), label
    tot = got.get("totals")
    if tot is not None:
        want = [sq_terms.sum(), ref["e"].sum(), 0.0, g_var.sum()]
        for k in (0, 1, 3):
            print(f"{label} total {k}: {tot[k]!r} want {want[k]!r}")
            assert abs(tot[k] - want[k]) <= rel * abs(want[k]), (label, k, tot[k], want[k])
        assert abs(tot[0] - ref["row_sq_err"].sum()) <= rel * ref["row_sq_err"].sum() + carried.sum(), label
        assert abs(tot[3] - ref["var"].sum()) <= rel * ref["var"].sum() + tv.sum(), label
    if noise_var is not None:
        ll, want = got["row_log_lik"].astype(np.float64), ref["row_log_lik"]
        scale = np.maximum(np.abs(want), 1.0)
        d = np.abs(ll - want) / scale
        print(f"{label} log-lik: worst {d.max() / EPS:.2f} eps, median {np.median(d) / EPS:.2f} eps (bounds {D + 4 * S + 16}, 16)")
        assert (d <= (D + 4 * S + 16) * EPS).all(), (label, float(d.max() / EPS))
        assert np.median(d) <= 16 * EPS, (label, float(np.median(d) / EPS))
        if tot is not None:
            # the third total is the double sum of the returned fp32 rows
            assert abs(tot[2] - ll.sum()) <= 1e-12 * np.abs(ll).sum(), (label, tot[2], ll.sum())
    elif tot is not None:
        assert tot[2] == 0.0
    return ref
