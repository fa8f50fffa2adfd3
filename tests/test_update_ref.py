"""The NumPy restatement of the update (tests/_update_np.py) against what is independent of it: the oracle's C adam_step and
sgd_step bit for bit, its own float64 form within a derived bound, and OracleVBLinear.update's norm ratios. CPU only. The GPU
tests (test_update_gpu.py) then hold the kernels to the restatement."""
import numpy as np
import pytest

from tests import _update_np as U

F = np.float32
N = 100003


def _adam_inputs(zero_moments, seed=3):
    r = np.random.RandomState(seed)
    x = (0.1 * r.standard_normal(N)).astype(np.float32)
    g = (1e-2 * r.standard_normal(N)).astype(np.float32)
    g[::17] = 0.0                                                    # exact-zero gradients
    g[5::19] = 1e-25                                                 # gradients whose square underflows
    g[6::19] = -1e-25
    if zero_moments:
        m, v = np.zeros(N, np.float32), np.zeros(N, np.float32)
    else:
        m = (1e-3 * r.standard_normal(N)).astype(np.float32)
        v = (1e-5 * np.abs(r.standard_normal(N)) + 1e-7).astype(np.float32)
        m[::23] = 0.0
        v[::23] = 0.0
    return x, g, m, v


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("zero_moments", [False, True])
@pytest.mark.parametrize("lr", [1e-3, 5e-2])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_f32_is_the_oracles_adam_step_bit_for_bit(oracle, t, lr, zero_moments):
    x, g, m, v = _adam_inputs(zero_moments)
    cfg = U.adam_cfg(lr, t)                                          # lambda = 1: all the oracle has
    x2, m2, v2, up = U.adam_f32(x, g, None, m, v, cfg)
    ox, om, ov = x.copy(), m.copy(), v.copy()
    oup = oracle.adam_step(ox, g, om, ov, lr, 0.9, 0.999, 1e-8, t)
    for name, a, b in (("x", x2, ox), ("m", m2, om), ("v", v2, ov), ("update", up, oup)):
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert bad.size == 0, (name, bad.size, bad[:5])
    assert not _same(x2, x)


@pytest.mark.parametrize("zero_moments", [False, True])
@pytest.mark.parametrize("t,lam", [(1, 1.0), (2, 1.0), (1000, 1.0), (1000, 0.999)])
def test_adam_f32_stays_within_the_float64_bound(t, lam, zero_moments):
    x, g, m, v = _adam_inputs(zero_moments)
    g2 = (1e-3 * np.random.RandomState(9).standard_normal(N)).astype(np.float32)
    for second in (None, g2):
        cfg = U.adam_cfg(1e-3, t, lambda_=lam)
        x32 = U.adam_f32(x, g, second, m, v, cfg)[0]
        x64, _, v64, _ = U.adam_f64(x, g, second, m, v, cfg)
        gsum = g.astype(np.float64) + (0.0 if second is None else second.astype(np.float64))
        bound = U.adam_bound(x64, gsum, m, v64, cfg)
        err = np.abs(x32.astype(np.float64) - x64)
        worst = float(np.max(err / bound))
        print(f"t {t} lambda {lam} grad2 {second is not None}: worst |x32 - x64| / bound = {worst:.3f}")
        assert (err <= bound).all(), worst


def test_a_float64_learning_rate_is_not_the_kernels_step():
    """Why adam_consts rounds the hyper-parameters to float32 first: the double step size from lr = 1e-3 (not a float) rounds
    to another float than the one from float(1e-3) at some t, and x then differs in places."""
    import math
    differs = 0
    for t in range(1, 2001):
        bc1, bc2 = 1.0 - math.pow(float(F(0.9)), t), 1.0 - math.pow(float(F(0.999)), t)
        differs += F(1e-3 * math.sqrt(bc2) / bc1) != F(float(F(1e-3)) * math.sqrt(bc2) / bc1)
    assert differs > 0


def test_sgd_f32_is_the_oracles_sgd_step_bit_for_bit(oracle):
    r = np.random.RandomState(4)
    x = (0.1 * r.standard_normal(N)).astype(np.float32)
    g = (1e-2 * r.standard_normal(N)).astype(np.float32)
    g[::13] = 0.0
    for lr in (1e-2, 1e-3, 0.3):
        ox = x.copy()
        oracle.sgd_step(ox, g, lr)
        assert _same(U.sgd_f32(x, g, lr), ox), lr


def test_fma_f32_rounds_once():
    """A sum one part in 2^46 below a float32 tie: rounding to float64 first lands ON the tie and then goes to even (up)."""
    a, b, c = F(2.0 ** -12 * (1 + 2.0 ** -23)), F(2.0 ** -12 * (1 - 2.0 ** -23)), F(1 + 2.0 ** -23)
    naive = F(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive == F(1 + 2.0 ** -22)                                # the double rounding this guards against
    assert U.fma_f32(np.array([a, -a]), np.array([b, b]), np.array([c, -c])).tolist() == [float(c), -float(c)]
    x = np.array([3.0, -0.5, 1e-3], np.float32)
    assert _same(U.fma_f32(x, F(2.0), F(1.0)), F(2.0) * x + F(1.0))  # exact cases are left alone


def test_bf16_rounding_by_integer_arithmetic():
    x = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, np.inf, -np.inf,
                  3.4028234663852886e38, 1e-40, -1e-45], np.float32)
    want = np.array([0.0, -0.0, 1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, np.inf, -np.inf, np.inf, 1e-40, -0.0], np.float32)
    got = U.bf16_round(x)
    want[9] = U.bf16_to_f32(np.array([(np.array([1e-40], np.float32).view(np.uint32)[0] + 0x8000) >> 16], np.uint16))[0]
    assert _same(got, want), (got, want)
    assert np.isnan(U.bf16_round(np.array([np.nan], np.float32)))[0]
    b = np.arange(0, 0x10000, dtype=np.uint32).astype(np.uint16)
    b = b[~np.isnan(U.bf16_to_f32(b))]
    assert np.array_equal(U.bf16_bits(U.bf16_to_f32(b)), b)          # every bf16 value survives the round trip


# ------------------------------------------------------------------------------------------------ the layer restatement
STEPS = [(1, 1.0), (1000, 0.999)]
LAYERS = [(1, 1), (5, 7), (70, 50), (128, 192)]      # the small shapes of the GPU table: the distance depends on the count


def _cfgs(t, lam):
    return U.adam_cfg(1e-3, t, lambda_=lam), U.adam_cfg(5e-2, t, lambda_=lam)


def _distances(O, I, kl_add, t, lam, mask=None):
    st = U.make_state(O, I, zero_moments=(t == 1))
    a = U.update_layer_f32(st, *_cfgs(t, lam), 50.0, kl_add, mask)
    b = U.update_layer_f64(st, *_cfgs(t, lam), 50.0, kl_add, mask)
    d = np.abs(a["log14"] - b["log14"])
    return np.where(d == 0.0, 0.0, d / np.maximum(np.abs(b["log14"]), 1e-300)), a, b      # (the std of ONE weight is 0 in both)


def test_series_distance_between_the_float32_and_float64_restatements():
    """The relative distance of each of the 14 series between update_layer_f32 and update_layer_f64, worst over four small
    layers, both kl_add and two steps: what float32 arithmetic (and a half-ulp exp) does to the series. U.SERIES_DIST records
    it; the GPU tests allow the series whose terms hold the device's expf four times that."""
    worst = np.zeros(14)
    for O, I in LAYERS:
        for kl_add in (0.0, 1.0):
            for t, lam in STEPS:
                worst = np.maximum(worst, _distances(O, I, kl_add, t, lam)[0])
    print("measured:", " ".join(f"{d:.2e}" for d in worst))
    print("recorded:", " ".join(f"{d:.2e}" for d in U.SERIES_DIST))
    assert (worst <= U.SERIES_DIST).all() and (worst[7] == 0.0)
    assert (U.SERIES_DIST <= 2.0 * worst + 1e-300).all()             # the record is the measurement, not a loosened one


def test_the_float64_form_bounds_every_parameter():
    """Per weight, the new means and lvars of the restatement stay within adam_bound of the float64 form (kl_add = 0: the
    gradients enter as they are, no exp on the way to a parameter)."""
    for t, lam in STEPS:
        st = U.make_state(70, 50, zero_moments=(t == 1))
        cm, cl = _cfgs(t, lam)
        a, b = U.update_layer_f32(st, cm, cl, 50.0, 0.0), U.update_layer_f64(st, cm, cl, 50.0, 0.0)
        for x, g, m, v, cfg in (("means", "g_mu", "m_mu", "v_mu", cm), ("lvars", "g_lv", "m_lv", "v_lv", cl)):
            bound = U.adam_bound(b[x], st[g], st[m], b[v], cfg)
            err = np.abs(a[x].astype(np.float64) - b[x])
            assert (err <= bound).all(), (x, t, float(np.max(err / bound)))


def test_series_match_the_oracles_update(oracle):
    """OracleVBLinear.update on one small layer returns the two norm ratios, series 12 and 13. Two steps: the first from zero
    moments (t = 1), the second with the moments the oracle carries (t = 2). The restatement gets the oracle's own pre-update
    var_hat, moments and likelihood gradients and adds the KL part itself (kl_add = 1). The oracle forms the KL gradients by
    other float32 expressions (a division by float(B var_hat); (-1 / v + 1 / var_hat) / (2 B) v) and takes expf from the C
    library, so the ratios agree to float32 rounding, not to the bit: tolerance 4 x U.SERIES_DIST[12], [13] (relative), the
    measured float32-to-float64 distance of the restatement itself. The two wrong forms of _bitten must fail at t = 2."""
    O, I, Bk = 70, 50, 50.0
    opt = dict(var_init=1e-2, mu_init=1, B=Bk, S=1, mode="lrt", seed=3, state=dict(learningRate=1e-2),
               meanState=dict(learningRate=1e-3), varState=dict(learningRate=5e-2))
    lay = oracle.OracleVBLinear(I, O, opt)
    r = np.random.RandomState(8)
    lay.lvars += (0.6 * r.standard_normal((O, I))).astype(np.float32)
    zeros = np.zeros((O, I), np.float32)
    for t in (1, 2):
        lay.gradWeight[:] = (1e-2 * r.standard_normal((O, I))).astype(np.float32)
        lay.gradSum[:] = (1e-1 * r.standard_normal((O, I))).astype(np.float32)       # (update() rescales it in place)
        lay.gradBias[:] = (1e-2 * r.standard_normal(O)).astype(np.float32)
        bias0, gbias = lay.bias.copy(), lay.gradBias.copy()
        _, stdv, _, var_hat = oracle.compute_prior(lay.means, lay.lvars)
        os_ = getattr(lay, "_opt_state", None)
        mom = lambda key, which: zeros if os_ is None else os_[key][which].copy()
        st = dict(means=lay.means.copy(), lvars=lay.lvars.copy(), g_mu=lay.gradWeight.copy(), g_lv=(lay.gradSum / F(2.0)) * stdv,
                  m_mu=mom("mean", "m"), v_mu=mom("mean", "v"), m_lv=mom("var", "m"), v_lv=mom("var", "v"),
                  stats=np.array([0.0, 0.0, var_hat, O * I]))
        ratios = lay.update(opt)
        cm, cl = U.adam_cfg(1e-3, t), U.adam_cfg(5e-2, t)
        for bite in (None, "swap", "step") if t == 2 else (None,):
            ref = _bitten(bite)(st, cm, cl, Bk, 1.0)
            got = (ref["log14"][12], ref["log14"][13])
            rel = [abs(g - w) / abs(w) for g, w in zip(got, ratios)]
            print(f"t {t} {bite or 'restatement'}: norm ratios {got} | oracle {ratios} | relative {rel[0]:.2e} {rel[1]:.2e} "
                  f"| allowed {4 * U.SERIES_DIST[12]:.2e} {4 * U.SERIES_DIST[13]:.2e}")
            ok = rel[0] <= 4 * U.SERIES_DIST[12] and rel[1] <= 4 * U.SERIES_DIST[13]
            assert ok == (bite is None), (t, bite, rel)
            # the new parameters against the oracle's: a few float32 roundings of the KL gradient apart, far less than a step
            far = [float(np.abs(ref[k].astype(np.float64) - getattr(lay, k)).max()) / float(F(c["lr"]))
                   for k, c in (("means", cm), ("lvars", cl))]
            assert all(f <= 1e-4 for f in far) == (bite is None), (t, bite, far)      # (a NaN is far)
        assert np.array_equal(U.sgd_f32(bias0, gbias, 1e-2).view(np.uint32), lay.bias.view(np.uint32))


def _bitten(kind):
    """update_layer_f32, or a deliberately wrong form of it: `swap` feeds m_lv and v_lv crossed over, `step` takes the lvars'
    step size from the means' configuration. Both must FAIL the cross-checks that the true restatement passes: the reference
    bites."""
    if kind is None:
        return U.update_layer_f32
    if kind == "swap":
        def f(st, cm, cl, B, kl_add, mask=None):
            with np.errstate(invalid="ignore"):                      # (the root of a negative "second moment")
                out = U.update_layer_f32(dict(st, m_lv=st["v_lv"], v_lv=st["m_lv"]), cm, cl, B, kl_add, mask)
            out["m_lv"], out["v_lv"] = out["v_lv"], out["m_lv"]
            return out
        return f

    def f(st, cm, cl, B, kl_add, mask=None):
        return U.update_layer_f32(st, cm, dict(cl, lr=cm["lr"]), B, kl_add, mask)
    return f


@pytest.mark.parametrize("bite", [None, "swap", "step"])
def test_the_float64_cross_check_bites(bite):
    """With non-zero moments (t = 1000) a crossed m_lv / v_lv or a step_lv from the means' configuration leaves the lvars far
    outside adam_bound of the float64 form; the true restatement is inside."""
    st = U.make_state(70, 50)
    cm, cl = _cfgs(1000, 0.999)
    a, b = _bitten(bite)(st, cm, cl, 50.0, 0.0), U.update_layer_f64(st, cm, cl, 50.0, 0.0)
    bound = U.adam_bound(b["lvars"], b["g_lv_total"], st["m_lv"], b["v_lv"], cl)
    inside = bool((np.abs(a["lvars"].astype(np.float64) - b["lvars"]) <= bound).all())
    assert inside == (bite is None)


def test_masked_restatement_freezes_and_counts():
    O, I = 70, 50
    st = U.make_state(O, I)
    mask = (np.random.RandomState(2).rand(O, I) < 0.5).astype(np.uint8)
    st["stats"] = U.prior_stats(st["means"], st["lvars"], keep=mask == 0)
    cm, cl = _cfgs(2, 1.0)
    a = U.update_layer_f32(st, cm, cl, 50.0, 1.0, mask)
    full = U.update_layer_f32(st, cm, cl, 50.0, 1.0)
    keep = mask == 0
    for k in U.FIELDS:
        assert _same(a[k][keep], full[k][keep]) and _same(a[k][~keep], st[k][~keep]), k
    assert not a["mu_s"][~keep].view(np.uint32).any() and not a["var_s"][~keep].view(np.uint32).any()
    assert a["stats"][3] == keep.sum() and a["stats"][2] == a["stats"][0] / keep.sum()
    assert a["log14"][8] == a["tot"][11] / keep.sum()
    none = U.update_layer_f32(st, cm, cl, 50.0, 1.0, np.zeros((O, I), np.uint8))
    assert np.array_equal(none["stats"], full["stats"]) and np.array_equal(none["log14"], full["log14"])
