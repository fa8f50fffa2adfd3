"""tests/_sweeps_np.py held to the CPU oracle and to its own float64 definitions, on every input set tests/test_sweeps_gpu.py
uses; and how much of each derived bound the float32 restatement itself uses (recorded in _sweeps_np.BOUND_USED). No GPU."""
import numpy as np
import pytest

from tests import _sweeps_np as R
from tests._sweeps_np import F, f8

WS = [1, 2, 3, 5, 1023, 1025, 4096, 70000]
SEED = 20240229


@pytest.fixture(scope="module")
def oracle():
    from oracle import vbnn_oracle as vo
    vo.build()
    return vo


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sets():
    for W in WS:
        for kind in R.PARAM_SETS:
            yield W, kind, R.param_set(kind, W)


def test_input_sets_hold_what_they_promise():
    m, l = R.param_set("wide", 4096)
    assert l.min() >= -20 and l.max() <= 5 and l.min() < -19 and l.max() > 4
    assert set(R.MU_SPECIAL.tolist()) <= set(m.tolist())
    m, l = R.param_set("fresh", 1025)
    assert not m.any() and (l == l[0]).all()
    st = R.prior_f64(m, l)["stats"]
    assert F(st[2]) == R.exp32(l[:1])[0]                             # v == var_hat exactly, as the kernels see var_hat
    x = R.input_set(37, 70)
    assert not x[18].any() and np.signbit(x[x == 0]).any()
    up = np.abs(R.bf16_round(x)) >= 2.0 * 2.0 ** np.floor(np.log2(np.maximum(np.abs(x), 1e-30)))
    assert up.any(), "no value that bf16 rounds up into the next binade"
    a, _ = R.pack_set(5, 7)
    assert np.isnan(a[1, 0]) and a[1, 1] == np.inf and a[1, 2] == -np.inf and np.signbit(a[1, 3]) and a[1, 3] == 0


def test_prior_restatement_against_the_oracle_and_the_definition(oracle):
    used0 = used1 = 0.0
    for W, kind, (m, l) in _sets():
        got = R.prior_f32(m, l)
        vars_, stdv, mu_sqe, vh = oracle.compute_prior(m, l)
        assert R.exp_ok(vars_, l, "f32").all(), (W, kind)            # the oracle's libm expf, within the allowance of exp64
        assert (_bits(stdv) == _bits(np.sqrt(vars_))).all()
        assert (_bits(mu_sqe) == _bits(got["mu_sqe"])).all()
        assert (_bits(got["stdv"]) == _bits(np.sqrt(got["vars"]))).all()
        ref = R.prior_f64(m, l)
        b0, b1 = R.prior_sum_bound(m, l), R.lsum_bound(l)
        assert abs(vh - ref["stats"][2]) * W <= b0
        used0 = max(used0, abs(got["stats"][0] - ref["stats"][0]) / b0)
        if b1 > 0:
            used1 = max(used1, abs(got["stats"][1] - ref["stats"][1]) / b1)
        assert got["stats"][3] == W and got["stats"][2] == (1.0 / W) * got["stats"][0]
        assert np.abs(got["vars"].astype(f8) - ref["vars"]).max() <= R.U32 * ref["vars"].max()
    print(f"stats[0] uses {used0:.4f} of its bound, stats[1] {used1:.4f}")
    _record("stats0", used0)
    _record("stats1", used1)


def _record(name, used):
    assert used < 1.0, f"{name}: the restatement itself exceeds the derived bound ({used:.3f}): the derivation is wrong"
    rec = R.BOUND_USED[name]
    assert used <= rec and (used == 0.0 or rec <= 2.0 * used + 1e-3), f"{name}: measured {used:.4f}, recorded {rec}: update _sweeps_np.BOUND_USED"


def test_restatement_stays_inside_the_derived_bounds(oracle):
    """calc_lc: the float32 restatement and the oracle against the float64 definition, element by element and summed."""
    used_e = used_s = 0.0
    for W, kind, (m, l) in _sets():
        if W not in (1, 5, 1023, 1025, 70000):
            continue
        var_hat = R.prior_f64(m, l)["stats"][2]
        v32, q32 = R.exp32(l), m * m
        for B in (1e6, 50.0):
            for route, a in (("cached", (None, None, v32, q32)), ("derived", (m, l, None, None))):
                lc, s = R.calc_lc_f32(*a, var_hat, B)
                want, want_s = R.calc_lc_f64(*a, var_hat, B)
                bound = R.lc_bound(*a, var_hat, B)
                err = np.abs(lc.astype(f8) - want)
                assert (err <= bound).all(), (W, kind, B, route, float((err / bound).max()))
                used_e = max(used_e, float((err / bound).max()))
                sb = float(bound.sum()) + 1e-10 * float(np.abs(want).sum())
                used_s = max(used_s, abs(s - want_s) / sb)
            o_sum, o_lc = oracle.calc_lc(v32, q32, var_hat, B, want_elem=True)
            want, _ = R.calc_lc_f64(None, None, v32, q32, var_hat, B)
            assert (np.abs(o_lc.astype(f8) - want) <= R.lc_bound(None, None, v32, q32, var_hat, B)).all(), (W, kind, B)
            assert abs(o_sum - float(o_lc.astype(f8).sum())) <= 1e-10 * float(np.abs(o_lc.astype(f8)).sum()) + 1e-300
    print(f"lc elements use {used_e:.4f} of their bound, the sum {used_s:.4f}")
    _record("lc_elem", used_e)
    _record("lc_sum", used_s)


def test_lc_bound_is_absolute_where_the_halves_cancel():
    m, l = R.param_set("fresh", 1025)
    var_hat = R.prior_f64(m, l)["stats"][2]
    want, _ = R.calc_lc_f64(m, l, None, None, var_hat, 50.0)
    bound = R.lc_bound(m, l, None, None, var_hat, 50.0)
    assert np.abs(want).max() < 1e-12 and bound.min() > 1e-9 / 50.0 and bound.max() < 1e-5 / 50.0


def test_kl_gradients_against_the_oracle_and_the_definition(oracle):
    for W, kind, (m, l) in _sets():
        if W > 1025:
            continue
        var_hat = R.telling_var_hat(R.prior_f64(m, l)["stats"][2])
        assert F(1.0 / var_hat) != F(1.0) / F(var_hat)
        v, g = R.exp32(l), np.random.RandomState(W).standard_normal(W).astype(F)
        sd = np.sqrt(v)
        for B in (1.0, 1e6):
            for S in (1.0, 30.0):
                lcg, gw = R.mugrads_f32(m, var_hat, B, S, g)
                o_gw, o_lcg = oracle.compute_mugrads(m, var_hat, B, S, g.copy())
                assert (_bits(lcg) == _bits(o_lcg)).all() and (_bits(gw) == _bits(o_gw)).all()
                d_lcg, d_gw = R.mugrads_f64(m, var_hat, B, S, g)
                assert (np.abs(lcg - d_lcg) <= 2 * R.U32 * np.abs(d_lcg) + R.TINY).all()
                assert (np.abs(gw - d_gw) <= R.U32 * np.abs(d_gw)).all()
                lcg, gs = R.vargrads_f32(None, v, sd, var_hat, B, S, g)
                o_gs, o_lcg = oracle.compute_vargrads(v, sd, var_hat, B, S, g.copy())
                assert (_bits(lcg) == _bits(o_lcg)).all() and (_bits(gs) == _bits(o_gs)).all()
                d_lcg, d_gs = R.vargrads_f64(None, v, sd, var_hat, B, S, g)
                # the KL part cancels at v = var_hat: bounded by the roundings of its two terms, 1 / v and 1 / var_hat
                assert (np.abs(lcg - d_lcg) <= 4 * R.U32 * (np.abs(d_lcg) + (1.0 / v + 1.0 / var_hat) * v / (2.0 * B)) + R.TINY).all()
                assert (np.abs(gs - d_gs) <= 3 * R.U32 * np.abs(d_gs)).all()
                # the lvars-only route: every expf the allowance admits lies inside the envelope
                for k, pick in ((0, 0), (1, 0), (-1, 1), (0, 1)):
                    a, b = R.envelope(lambda exp: R.vargrads_f32(l, None, None, var_hat, B, S, g, exp=exp)[pick])
                    mid = R.vargrads_f32(l, None, None, var_hat, B, S, g, exp=R.exp_shifted(k))[pick]
                    assert ((a <= mid) & (mid <= b)).all()


def test_weight_draw_and_fill_against_the_oracle(oracle):
    for O, I in [(1, 1), (5, 7), (48, 64), (3, 130)]:
        e = R.wn_eps(O, I, SEED, 3, 11)
        assert (_bits(e) == _bits(oracle.fill_normal(O, I, SEED, oracle.STREAM_EPS, 3, 11, 0))).all()
        for kind in R.PARAM_SETS:
            m, l = R.param_set(kind, O * I)
            sd = np.sqrt(R.exp32(l))
            w = R.wn_sample_f32(m, sd, None, e.reshape(-1))
            assert (_bits(w) == _bits(oracle.sample(m, sd, e.reshape(-1).copy()))).all()
            d = R.wn_sample_f64(m, sd, None, e.reshape(-1))
            assert (np.abs(w - d) <= R.U32 * (np.abs(d) + np.abs(sd * e.reshape(-1)))).all()
            a, b = R.envelope(lambda exp: R.wn_sample_f32(m, None, l, e.reshape(-1), exp=exp))
            assert ((a <= w) & (w <= b)).all()
            d = R.wn_sample_f64(m, None, l, e.reshape(-1))
            assert (np.abs(w - d) <= 3 * R.U32 * (np.abs(d) + np.abs(sd * e.reshape(-1)))).all()
    for scale in (1.0, 0.05):
        z = R.fill_normal_f32(33, 130, SEED, 2, 2, 7, (1 << 32) - 16, scale)
        d = R.fill_normal_f64(33, 130, SEED, 2, 2, 7, (1 << 32) - 16, scale)
        assert (np.abs(z - d) <= R.U32 * np.abs(d)).all()
        assert (_bits(z[16:]) == _bits(R.fill_normal_f32(17, 130, SEED, 2, 2, 7, 0, scale))).all()      # the row word wraps


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_packers_against_their_definitions(dtype):
    u_t = 2.0 ** -8 if dtype == "bf16" else R.U32
    for rows, cols in [(1, 1), (5, 7), (65, 63)]:
        a, b = R.pack_set(rows, cols)
        fin = np.isfinite(a)
        for func in range(6):
            v32, v64 = R.pack_f32(func, a, b, dtype), R.pack_f64(func, a, b, dtype)
            assert (np.isnan(v32) == np.isnan(v64)).all()
            ok = fin & ~np.isnan(v64)
            assert (np.abs(v32[ok] - v64[ok]) <= R.U32 * np.abs(v64[ok])).all(), func
            st = R.values(R.stored(v32, dtype))
            assert (np.abs(st[ok] - v64[ok]) <= (u_t + R.U32) * np.abs(v64[ok])).all(), func
        relu = R.pack_f32(R.RELU, a, b, dtype)
        if rows >= 2:
            assert relu[1, 0] == 0 and relu[1, 1] == np.inf and relu[1, 2] == 0 and relu[1, 3] == 0      # NaN -> 0, -0.0 -> a zero
    for N, I in [(3, 7), (37, 70)]:
        x = R.input_set(N, I)
        for rpd in (0, 7):
            xs, x2 = R.pack_input_f32(x, N, rpd, dtype)
            d, d2 = R.pack_input_f64(x, N, rpd, dtype)
            rows = np.arange(N) % rpd if rpd else np.arange(N)
            assert (R.values(xs) == R.round_t(x[rows], dtype)).all()
            assert (np.abs(R.values(xs) - d) <= u_t * np.abs(d)).all()
            assert (np.abs(R.values(x2) - d2) <= u_t * d2).all()
            if dtype == "bf16":                                      # the square of a bf16 value is exact in float32
                assert (R.values(x2) == R.bf16_round(d2.astype(F))).all()
