"""tests/_step_np.py (the float64 restatement of one engine step for every head kind) held on the CPU: against
oracle.ref_numpy.emulate_lrt_step and OracleMLP.run where those know the criterion (`nll`, `mse`), against central finite
differences of its own objective where they do not (`gauss`, `bce`, 20-class `nll`), and the margins the step matrix's cases
(tests/test_step_matrix_gpu.py) need in their float64 logits."""
import numpy as np
import pytest

from tests import _step_np as R

OPT = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", seed=3, type="vb")


def _net(oracle, crit, Cn, I0=20, hidden=(16, 12), N=9, S=2, seed=11):
    opt = dict(OPT, input_size=I0, hidden=list(hidden), n_classes=Cn, criterion=crit, S=S)
    onet = oracle.OracleMLP(opt)
    rng = np.random.default_rng(seed)
    for om in onet.vb:
        om.means[:] = om.weight
        om.lvars[:] = rng.normal(np.log(1e-3), 0.3, om.lvars.shape).astype(np.float32)
        om.bias[:] = rng.normal(0, 0.1, om.bias.shape).astype(np.float32)
        om.compute_prior()
    onet.last.bias[:] = rng.normal(0, 0.1, Cn).astype(np.float32)
    x = oracle.fill_normal(N, I0, 3, oracle.STREAM_DATA, 0, 0)
    t = (np.arange(N) * 3 % Cn).astype(np.int32) if crit == "nll" else rng.normal(0, 1, (N, Cn)).astype(np.float32)
    layers = [dict(means=om.means, lvars=om.lvars, bias=om.bias) for om in onet.vb]
    zetas = [[oracle.fill_normal(N, om.O, 3, oracle.STREAM_ZETA, k, s + 1, 0).astype(np.float64) for k, om in enumerate(onet.vb)]
             for s in range(S)]
    return opt, onet, layers, x, t, zetas


@pytest.mark.parametrize("crit,Cn", [("nll", 10), ("mse", 7)])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_step_is_emulate_lrt_step_draw_by_draw(oracle, crit, Cn, bf16):
    """S = 2 draws against the sums of two emulate_lrt_step calls, to float64 rounding (1e-12 of each region's largest value),
    with and without bf16 operand rounding and shadow KL terms."""
    from oracle.ref_numpy import bf16_round, emulate_lrt_step
    opt, onet, layers, x, t, zetas = _net(oracle, crit, Cn)
    rnd = bf16_round if bf16 else (lambda a: a)
    S = len(zetas)
    got = R.step(layers, onet.last.weight, onet.last.bias, x, t, zetas, crit, rnd, B=opt["B"], kl_shadows=bf16)
    parts = [emulate_lrt_step(layers, onet.last.weight, onet.last.bias, x, t, zs, rnd, S=1.0, B=opt["B"], kl_shadows=bf16,
                              criterion=crit) for zs in zetas]
    # emulate_lrt_step's grad_mu = gw + KL for one draw with S = 1: the S-draw total is mean(gw) + KL
    one = emulate_lrt_step(layers, onet.last.weight, onet.last.bias, x, t, zetas[0], rnd, S=1.0, B=opt["B"], kl_shadows=bf16,
                           criterion=crit, kl_scale=0.0)
    want = {"final.weight": sum(p[2] for p in parts), "final.bias": sum(p[3] for p in parts)}
    for k in range(len(layers)):
        kl_mu = parts[0][1][k]["grad_mu"] - one[1][k]["grad_mu"]
        kl_lv = parts[0][1][k]["grad_lv"] - one[1][k]["grad_lv"]
        like_mu = sum(p[1][k]["grad_mu"] for p in parts) - S * kl_mu
        like_lv = sum(p[1][k]["grad_lv"] for p in parts) - S * kl_lv
        want[f"{k}.mu"], want[f"{k}.lv"] = like_mu / S + kl_mu, like_lv / S + kl_lv
        want[f"{k}.bias"] = sum(p[1][k]["gradBias"] for p in parts)
    assert abs(got["loss"] - sum(p[0] for p in parts)) <= 1e-14 * abs(got["loss"])
    assert sorted(want) == sorted(got["regions"]) == sorted(R.region_names(len(layers)))
    for name, w in want.items():
        assert np.abs(got["regions"][name] - w).max() <= 1e-12 * np.abs(w).max(), name


@pytest.mark.parametrize("crit,Cn", [("nll", 10), ("mse", 7)])
def test_step_is_the_oracle_network(oracle, crit, Cn):
    """Against OracleMLP.run (C kernels, fp32, module by module) over S = 2 draws, with the tolerances of
    test_mlp_step_against_independent_float64_derivation; the hit count exactly."""
    opt, onet, layers, x, t, zetas = _net(oracle, crit, Cn)
    got = R.step(layers, onet.last.weight, onet.last.bias, x, t, zetas, crit, B=opt["B"])
    onet.resetGradients()
    err = hits = 0.0
    for _ in zetas:
        onet.sample()
        e, acc = onet.run(x, t)
        err += e
        hits += acc * x.shape[0] / 100.0
    assert abs(got["loss"] - err) <= 1e-5 * abs(err)
    assert got["hits"] == round(hits)
    reg = got["regions"]
    for k, om in enumerate(onet.vb):
        mle, mlc = om.compute_mugrads(opt)
        vle, vlc = om.compute_vargrads(opt)
        np.testing.assert_allclose(mle + mlc, reg[f"{k}.mu"], rtol=0, atol=2e-5 * np.abs(reg[f"{k}.mu"]).max())
        np.testing.assert_allclose(vle + vlc, reg[f"{k}.lv"], rtol=0, atol=5e-5 * np.abs(reg[f"{k}.lv"]).max())
        np.testing.assert_allclose(om.gradBias, reg[f"{k}.bias"], rtol=0, atol=2e-5 * np.abs(reg[f"{k}.bias"]).max())
    np.testing.assert_allclose(onet.last.gradWeight, reg["final.weight"], rtol=0, atol=2e-5 * np.abs(reg["final.weight"]).max())
    np.testing.assert_allclose(onet.last.gradBias, reg["final.bias"], rtol=0, atol=2e-5 * np.abs(reg["final.bias"]).max())


@pytest.mark.parametrize("crit,Cn", [("gauss", 6), ("bce", 5), ("nll", 20)])
def test_step_gradients_by_finite_differences(oracle, crit, Cn):
    """A 7-5-4 network, S = 2 draws, B = 10 (so that the KL terms weigh in): every region of step() against central differences
    of step()'s own objective = loss / S + KL cost, all in float64 (acc = np.float64), with test_kl_gradients_by_finite_differences'
    step and tolerance (eps = 1e-4; 2e-3 relative + 1e-7). d/dmeans and d/dlvars are the objective's derivatives; the bias and
    final Linear regions hold the draws' sum, S times them."""
    B = 10.0
    opt, onet, layers, x, t, zetas = _net(oracle, crit, Cn, I0=7, hidden=(5, 4), N=6, S=2, seed=5)
    rng = np.random.default_rng(8)
    if crit == "gauss":
        t = rng.normal(0, 1, (6, Cn // 2)).astype(np.float32)
    elif crit == "bce":
        t = (rng.random((6, Cn)) < 0.4).astype(np.float32)
    S = len(zetas)
    w3, b3 = onet.last.weight.astype(np.float64), onet.last.bias.astype(np.float64)
    layers = [{k: v.astype(np.float64) for k, v in lay.items()} for lay in layers]

    def objective():
        return R.step(layers, w3, b3, x.astype(np.float64), t, zetas, crit, B=B, acc=np.float64)["objective"]

    reg = R.step(layers, w3, b3, x.astype(np.float64), t, zetas, crit, B=B, acc=np.float64)["regions"]
    eps = 1e-4
    targets = [(f"{k}.mu", lay["means"], 1.0) for k, lay in enumerate(layers)] + \
              [(f"{k}.lv", lay["lvars"], 1.0) for k, lay in enumerate(layers)] + \
              [(f"{k}.bias", lay["bias"], float(S)) for k, lay in enumerate(layers)] + \
              [("final.weight", w3, float(S)), ("final.bias", b3, float(S))]
    checked = 0
    for name, arr, mult in targets:
        flat = arr.reshape(-1)                                       # a view: the step reads the perturbed parameter
        for i in sorted(set(int(j) for j in rng.integers(0, flat.size, 4)) | {0, flat.size - 1}):
            keep = flat[i]
            flat[i] = keep + eps
            up = objective()
            flat[i] = keep - eps
            dn = objective()
            flat[i] = keep
            fd = mult * (up - dn) / (2 * eps)
            an = reg[name].reshape(-1)[i]
            assert abs(fd - an) <= 2e-3 * abs(an) + 1e-7, (name, i, fd, an)
            checked += 1
    assert checked >= 5 * len(targets) // 2


@pytest.mark.parametrize("head", list(R.HEADS))
@pytest.mark.parametrize("tier", list(R.TIERS))
def test_matrix_cases_keep_their_margins(oracle, tier, head):
    """The seeds of the step matrix's cases: in the float64 reference no `bce` logit lies within 1e-3 max|z| of 0, no top-two
    gap of an `nll` row is below 1e-3 max|z|, no `gauss` s within 1 of the clamp -- so the hit counts and the clamp's slope
    cannot turn on a rounding."""
    case = R.make_case(oracle, tier, head, draws=3 if tier == "small-f32" else None)      # (small-f32: its stacked cases' three draws)
    ref = R.reference(case)
    ok, have, need = R.margins(case, ref)
    print(f"{tier} {head}: seed {case['seed']}, margin {have:.4e} against {need:.4e}")
    assert ok, (tier, head, have, need)
    assert np.isfinite(ref["loss"]) and all(np.isfinite(v).all() for v in ref["regions"].values())
