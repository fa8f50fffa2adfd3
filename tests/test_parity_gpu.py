"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs. Tolerances are stated per test. fp32 GEMM outputs: |d| <= 2e-6 * sum_k|a_k b_k| + 1e-7
(fp32 MFMA is an exact fma chain; the K order inside a 16-wide step is permuted).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def gemm_tol(absprod, rel=2e-6, abs_=1e-7):
    return rel * absprod + abs_


def assert_close(got, want, tol, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = err > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} off, max err {err.max():.3e} (tol at worst {np.max(tol):.3e})"


GEMM_KERNELS = {0: "none", 1: "latency", 2: "latency pair", 3: "general", 4: "general pair", 5: "pipelined", 6: "two-pass", 7: "two-pass split"}


def gemm_form():
    """VBNN_DEBUG_LAST_GEMM_FORM (include/vbnn_hip.h) of the last GEMM launch: (kernel, A K-major, family 1 FWD / 2 DX / 3 DW, value)"""
    from vbnn_amd import _lib as L
    f = L.lib().vbnn_debug_get(13)
    return f & 15, (f >> 12) & 1, (f >> 20) & 3, f


def check_forced_kernel(forced, what):
    """After a launch of the MODULE path under VBNN_DEBUG_GEMM_KERNEL = forced: 1 and 2 take every bf16 launch (packed pitches are
    multiples of 64), asserted. 3 means "the two-pass kernel whenever the shape and outputs allow it": whole 256 x 256 tiles AND
    the fused outputs alone -- the module path asks for y / gx / gradWeight in fp32, so today it runs another kernel there, and
    this says which. (The two-pass kernel's own cases: tests/test_gemm_forms_gpu.py.)"""
    k, _, _, f = gemm_form()
    if forced == 1:
        assert k == 3, f"{what}: forced the general kernel, ran the {GEMM_KERNELS[k]} kernel"
    elif forced == 2:
        assert k == 5, f"{what}: forced the pipelined kernel, ran the {GEMM_KERNELS[k]} kernel"
    else:
        assert k in (3, 5, 6), f"{what}: ran the {GEMM_KERNELS[k]} kernel (form {f:#x})"
        if k != 6:
            print(f"{what}: VBNN_DEBUG_GEMM_KERNEL = {forced} did not take this launch, the {GEMM_KERNELS[k]} kernel ran (form {f:#x})")


@pytest.fixture(scope="module")
def nnmod():
    from vbnn_amd import nn
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return nn


def opt_for(mode, dtype="f32", **kw):
    o = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode=mode, dtype=dtype, seed=SEED, keep_e=True,
             input_size=784, hidden=[400, 400], n_classes=10, type="vb", testSamples=2)
    o.update(kw)
    return o


# ------------------------------------------------------------------------------------------- RNG
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 7), (5, 64), (33, 130)])
def test_fill_normal_bit_exact(nnmod, oracle, rows, cols):
    """device Philox4x32-10 + Box-Muller == oracle, bit for bit (include/vbnn_philox.h)."""
    from vbnn_amd import _lib as L
    for stream, layer, draw, row0 in [(L.STREAM_EPS, 0, 1, 0), (L.STREAM_ZETA, 2, 7, 1000)]:
        t = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
        nnmod.fill_normal(t, SEED, stream, layer, draw, row0=row0)
        want = oracle.fill_normal(rows, cols, SEED, stream, layer, draw, row0)
        got = host(t)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_hardware_form_of_the_normals_stays_within_2e6_of_the_contract(nnmod, oracle):
    """What the bf16 forward draws (vbnn_normal4_hw: the contract's Philox words, Box-Muller by v_log / v_sqrt / v_sin / v_cos)
    against the bit-exact contract on 2^22 normals: max |dz| < 2e-6 absolute (bf16 rounds what is made of them at 4e-3
    relative), same mean / variance to 1e-6, and the largest |z| -- the u1 -> 0 tail, where log2 is steepest -- included."""
    from vbnn_amd import _lib as L
    rows, cols = 2048, 2048
    a = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
    b = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(a, SEED, L.STREAM_ZETA, 1, 5, row0=4096)
    nnmod.fill_normal(b, SEED, L.STREAM_ZETA, 1, 5, row0=4096, hw=True)
    want = oracle.fill_normal(4, 64, SEED, L.STREAM_ZETA, 1, 5, 4096)
    assert np.array_equal(host(a[:4, :64]).view(np.uint32), want.view(np.uint32))     # `a` IS the contract
    d = (a.double() - b.double()).abs()
    assert float(d.max()) < 2e-6, float(d.max())
    assert abs(float(a.double().mean() - b.double().mean())) < 1e-6
    assert abs(float(a.double().var() - b.double().var())) < 1e-6
    i = int(a.abs().argmax())
    assert abs(float(a.view(-1)[i] - b.view(-1)[i])) < 2e-6 and float(a.abs().max()) > 4.5


def test_hardware_form_error_model_over_all_radii_all_angles_and_eight_windows(nnmod, oracle, tmp_path):
    """the bf16 forward's normals (v_log / v_sqrt / v_sin / v_cos Box-Muller) against the contract, as an ERROR
    MODEL rather than one window. With vbnn_box_muller_forms both forms are evaluated on GIVEN Philox words:
      (A) ALL 2^24 radii (u1 = (k + 1) 2^-24, k = 0 .. 2^24 - 1: u1 -> 0 included) at the angles 0 and 1/8 turn;
      (B) ALL 2^24 angles (every octant edge, every zero crossing) at the LARGEST radius (u1 = 2^-24, r = 5.768) and at r ~ 1;
      (C) eight (layer, draw, row0) windows of 2^20 normals addressed through the counter, as the forward addresses them.
    Bounds: |z_hw - z_contract| < 2e-6 everywhere, and both forms within 2.5e-6 of float64 Box-Muller on the same words (the
    contract's own polynomial log / sincos are not exact either). The measured maxima are written to gpurun_out/ and held against
    tests/golden/normals_hw_error.json (taken on an MI355X of this pool): a box whose transcendental microcode answers
    differently by more than a quarter shows up here."""
    import ctypes as C
    import json
    from vbnn_amd import _lib as L
    from tests import _philox_np as P
    lib, ctx = L.lib(), nnmod.Context.get()
    n = 1 << 24
    ks = torch.arange(n, device="cuda", dtype=torch.int64)

    def forms(x0, x1):
        x0, x1 = x0.to(torch.int32).contiguous(), x1.to(torch.int32).contiguous()
        ze = torch.empty(2 * x0.numel(), dtype=torch.float32, device="cuda")
        zh = torch.empty_like(ze)
        L.check(lib.vbnn_box_muller_forms(ctx.h, C.c_void_p(x0.data_ptr()), C.c_void_p(x1.data_ptr()), C.c_void_p(ze.data_ptr()),
                                          C.c_void_p(zh.data_ptr()), x0.numel()))
        return ze.view(-1, 2).double(), zh.view(-1, 2).double()

    def words(k):                                            # 24-bit field k -> the 32-bit word whose top 24 bits are k (as int32 bits)
        w = (k << 8) & 0xFFFFFFFF
        return torch.where(w >= (1 << 31), w - (1 << 32), w)

    rec = {}
    # (A) all radii, at angle 0 (z0 = r) and at 1/8 turn (z0 = z1 = r / sqrt 2)
    u1 = (ks.double() + 1.0) * 2.0 ** -24
    r_ideal = torch.sqrt(-2.0 * torch.log(u1))
    for name, tk in (("angle_0", 0), ("angle_1_8", 1 << 21)):
        ze, zh = forms(words(ks), words(torch.full_like(ks, tk)))
        c, s_ = np.cos(2 * np.pi * tk / 2 ** 24), np.sin(2 * np.pi * tk / 2 ** 24)
        ideal = torch.stack([r_ideal * c, r_ideal * s_], -1)
        rec[f"all_radii_{name}"] = {"hw_vs_contract": float((zh - ze).abs().max()), "hw_vs_float64": float((zh - ideal).abs().max()),
                                    "contract_vs_float64": float((ze - ideal).abs().max()),
                                    "hw_vs_contract_at_u1_min": float((zh[0] - ze[0]).abs().max()), "r_max": float(ze[0].abs().max())}
    # (B) all angles, at the largest radius (k = 0) and at r ~ 1 (u1 = exp(-1/2))
    t = ks.double() * 2.0 ** -24
    for name, rk in (("r_max", 0), ("r_1", int(round(2 ** 24 * np.exp(-0.5))) - 1)):
        ze, zh = forms(words(torch.full_like(ks, rk)), words(ks))
        r = float(np.sqrt(-2.0 * np.log((rk + 1) * 2.0 ** -24)))
        ideal = torch.stack([r * torch.cos(2 * np.pi * t), r * torch.sin(2 * np.pi * t)], -1)
        d = (zh - ze).abs().max(dim=1).values
        edges = torch.arange(0, n, n // 8, device="cuda")                      # the octant edges themselves
        rec[f"all_angles_{name}"] = {"r": r, "hw_vs_contract": float(d.max()), "hw_vs_float64": float((zh - ideal).abs().max()),
                                     "contract_vs_float64": float((ze - ideal).abs().max()),
                                     "hw_vs_contract_at_octant_edges": float(d[edges].max()),
                                     "hw_vs_contract_within_4_steps_of_an_edge": float(torch.stack([d[(edges + o) % n] for o in range(-4, 5)]).max())}
    # (C) eight windows through the counter
    rows, cols = 512, 2048
    a = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    for layer, draw, row0 in ((0, 1, 0), (1, 5, 4096), (2, 2, 1 << 20), (3, 1000, 28672), (4, 7, (1 << 31) - 512), (5, 1 << 30, 12345),
                              (6, 3, 1 << 24), (7, (1 << 32) - 1, 65536)):
        nnmod.fill_normal(a, SEED, L.STREAM_ZETA, layer, draw, row0=row0)
        nnmod.fill_normal(b, SEED, L.STREAM_ZETA, layer, draw, row0=row0, hw=True)
        x0, x1 = P.window_words(rows, cols, SEED, L.STREAM_ZETA, layer, draw, row0)
        z0, z1, r = P.ideal_box_muller(x0, x1)
        ideal = np.stack([z0, z1], -1).reshape(rows, cols)
        ha, hb = host(a).astype(np.float64), host(b).astype(np.float64)
        d = np.abs(hb - ha)
        i = int(np.argmax(r))                                                  # the pair with the smallest u1 of the window
        rec[f"window_layer{layer}_draw{draw}_row{row0}"] = {
            "hw_vs_contract": float(d.max()), "hw_vs_float64": float(np.abs(hb - ideal).max()), "contract_vs_float64": float(np.abs(ha - ideal).max()),
            "z_min": float(ha.min()), "z_max": float(ha.max()), "r_max_in_window": float(r.max()),
            "hw_vs_contract_at_r_max": float(d.reshape(rows, cols // 2, 2)[i // (cols // 2), i % (cols // 2)].max()),
            "mean_hw_minus_contract": float((hb - ha).mean())}
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "normals_hw_error_measured.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    for name, v in rec.items():
        assert v["hw_vs_contract"] < 2e-6, (name, v)
        assert v["hw_vs_float64"] < 2.5e-6 and v["contract_vs_float64"] < 2.5e-6, (name, v)
    gold_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normals_hw_error.json")
    if os.path.exists(gold_path):
        gold = json.load(open(gold_path))
        assert sorted(gold) == sorted(rec), "the recorded windows are not the measured ones: regenerate tests/golden/normals_hw_error.json"
        for name, v in rec.items():
            for k in ("hw_vs_contract", "hw_vs_float64"):
                assert v[k] <= 1.25 * gold[name][k] + 1e-8, f"{name} {k}: {v[k]:.3e} measured, {gold[name][k]:.3e} recorded"


# ------------------------------------------------------------------------------------------- prior / KL
@pytest.mark.parametrize("O,I", [(5, 7), (48, 64), (400, 784)])
def test_compute_prior_and_kl(nnmod, oracle, O, I):
    opt = opt_for("wn")
    m = nnmod.VBLinear(I, O, opt)
    rng = np.random.default_rng(0)
    means = rng.normal(0, 0.05, (O, I)).astype(np.float32)
    lvars = rng.normal(np.log(1e-3), 0.5, (O, I)).astype(np.float32)
    m.means.copy_(dev(means)); m.lvars.copy_(dev(lvars))
    _, var_hat = m.compute_prior()
    vars_, stdv, mu_sqe, vh = oracle.compute_prior(means, lvars)
    assert abs(var_hat - vh) <= 1e-6 * vh
    np.testing.assert_allclose(host(m.vars), vars_, rtol=1e-5, atol=0)
    np.testing.assert_allclose(host(m.stdv), stdv, rtol=1e-5, atol=0)
    np.testing.assert_allclose(host(m.mu_sqe), mu_sqe, rtol=1e-6, atol=0)
    # calc_lc (VBLinear.lua:99-103) on the cached statistics
    lc, lc_elem = m.calc_lc(opt, elementwise=True)
    want_sum, want_elem = oracle.calc_lc(vars_, mu_sqe, vh, opt["B"], want_elem=True)
    np.testing.assert_allclose(host(lc_elem), want_elem, rtol=2e-4, atol=1e-11)
    assert abs(float(lc.item()) - want_sum) <= 2e-4 * abs(want_sum) + 1e-9
    # compute_mugrads / compute_vargrads (VBLinear.lua:90-98), in-place semantics included
    gw = rng.normal(0, 1, (O, I)).astype(np.float32)
    gs = rng.normal(0, 1, (O, I)).astype(np.float32)
    m.gradWeight.copy_(dev(gw)); m.gradSum.copy_(dev(gs))
    o2 = dict(opt, S=30)
    mle, mlc = m.compute_mugrads(o2)
    vle, vlc = m.compute_vargrads(o2)
    w_mle, w_mlc = oracle.compute_mugrads(means, vh, o2["B"], o2["S"], gw.copy())
    w_vle, w_vlc = oracle.compute_vargrads(vars_, stdv, vh, o2["B"], o2["S"], gs.copy())
    np.testing.assert_allclose(host(mle), w_mle, rtol=1e-6, atol=0)
    np.testing.assert_allclose(host(mlc), w_mlc, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(host(vle), w_vle, rtol=1e-5, atol=0)
    np.testing.assert_allclose(host(vlc), w_vlc, rtol=1e-4, atol=1e-11)
    assert mle.data_ptr() == m.gradWeight.data_ptr() and vle.data_ptr() == m.gradSum.data_ptr()


def test_fresh_layer_known_answers(nnmod):
    """SURVEY 8c KAT 1-2: mu_init = 0 => var_hat == var_init, LC == 0, KL grads == 0; msr_init => 2/I."""
    opt = opt_for("wn", mu_init=0)
    m = nnmod.VBLinear(64, 48, opt)
    assert abs(m.var_hat - 1e-3) <= 1e-9
    lc = float(m.calc_lc(opt).item())
    assert abs(lc) < 1e-9
    _, mlc = m.compute_mugrads(opt)
    _, vlc = m.compute_vargrads(opt)
    assert float(mlc.abs().max()) == 0.0
    assert float(vlc.abs().max()) < 1e-12
    m2 = nnmod.VBLinear(50, 20, opt_for("wn", mu_init=0, msr_init=True))
    assert abs(m2.var_init - 2.0 / 50) < 1e-12
    np.testing.assert_allclose(host(m2.lvars), np.full((20, 50), np.log(2.0 / 50), np.float32), rtol=1e-6)


# ------------------------------------------------------------------------------------------- single layer
def _layer_pair(nnmod, oracle, mode, I, O, dtype="f32"):
    opt = opt_for(mode, dtype)
    m = nnmod.VBLinear(I, O, opt)
    om = oracle.OracleVBLinear(I, O, opt, layer_id=0)
    rng = np.random.default_rng(1)
    means = rng.normal(0, np.sqrt(2.0 / I), (O, I)).astype(np.float32)
    lvars = rng.normal(np.log(1e-3), 0.3, (O, I)).astype(np.float32)
    bias = rng.normal(0, 0.1, O).astype(np.float32)
    m.means.copy_(dev(means)); m.lvars.copy_(dev(lvars)); m.bias.copy_(dev(bias))
    om.means[:] = means; om.lvars[:] = lvars; om.bias[:] = bias
    m.compute_prior(); om.compute_prior()
    return opt, m, om


@pytest.mark.parametrize("N,I,O", [(1, 4, 4), (3, 7, 5), (32, 64, 48), (100, 130, 70), (256, 784, 400),
                                   (64, 256, 100), (64, 100, 10),       # these two: convnet.lua:24,30
                                   (8, 3001, 24), (17, 1, 3)])          # a long ragged K walk and K = 1 (the latency kernel's ring and tail)
@pytest.mark.parametrize("mode", ["wn", "lrt"])
def test_layer_forward_backward_f32(nnmod, oracle, mode, N, I, O):
    """T1 (wn) / T2 (lrt): output, gradInput, gradWeight, gradSum, gradBias sample-exact vs the oracle."""
    opt, m, om = _layer_pair(nnmod, oracle, mode, I, O)
    rng = np.random.default_rng(2)
    x = rng.normal(0, 1, (N, I)).astype(np.float32)
    x[0, :] = 0.0 if N > 1 else x[0, :]          # a zero row: v == 0 -> r must be 0, not NaN
    g = rng.normal(0, 1.0 / N, (N, O)).astype(np.float32)
    for draw in range(2):                         # two draws: accumulation across draws (main.lua:32-37)
        m.sample(); om.sample()
        if mode == "wn":
            np.testing.assert_allclose(host(m.weight), om.weight, rtol=0, atol=2e-7 * np.abs(om.weight).max())
            assert np.array_equal(host(m.e).view(np.uint32), om.e.view(np.uint32))
            # and bit for bit from the device's own cached stdv (the oracle's differs by its libm's expf): two fp32 roundings
            assert np.array_equal(host(m.weight).view(np.uint32), (host(m.means) + host(m.stdv) * host(m.e)).view(np.uint32))
        y = m.updateOutput(dev(x))
        want_y = om.updateOutput(x)
        w_eff = np.abs(om.weight) if mode == "wn" else np.abs(om.means)
        absprod = np.abs(x) @ w_eff.T + np.abs(om.bias)
        if mode == "lrt":
            absprod = absprod + np.abs(np.sqrt(om.v) * oracle.fill_normal(N, O, SEED, 2, 0, om.draw, 0))
        assert_close(host(y), want_y, gemm_tol(absprod, 4e-6), f"output draw {draw}")
        if mode == "lrt":
            assert np.isfinite(host(m.r)).all()
            np.testing.assert_allclose(host(m.r), om.r, rtol=2e-5, atol=1e-6)
        gx = m.backward(dev(x), dev(g), 0.5)
        want_gx = om.backward(x, g, 0.5)
        if mode == "wn":
            absg = np.abs(g) @ np.abs(om.weight)
        else:
            absg = np.abs(g) @ np.abs(om.means) + 2 * np.abs(x) * (np.abs(g * om.r) @ om.vars)
        assert_close(host(gx), want_gx, gemm_tol(absg, 1e-5, 1e-7), f"gradInput draw {draw}")
    absw = np.abs(g).T @ np.abs(x)
    assert_close(host(m.gradWeight), om.gradWeight, 2 * gemm_tol(absw, 4e-6), "gradWeight")
    np.testing.assert_allclose(host(m.gradBias), om.gradBias, rtol=1e-5, atol=1e-6)
    if mode == "wn":
        asum = 2 * (absw * 5.0)
    else:
        asum = 2 * 2 * (np.abs(g * om.r).T @ (x * x)) * om.stdv
    assert_close(host(m.gradSum), om.gradSum, gemm_tol(asum, 2e-5, 1e-6), "gradSum")


def test_map_forward_equals_plain_linear(nnmod, oracle):
    """SURVEY 8c KAT 3: clamp_to_map then forward == Linear with weight = means (both modes)."""
    for mode in ("wn", "lrt"):
        opt, m, om = _layer_pair(nnmod, oracle, mode, 64, 48)
        x = np.random.default_rng(3).normal(0, 1, (16, 64)).astype(np.float32)
        m.clamp_to_map()
        y = host(m.updateOutput(dev(x)))
        want = oracle.linear_forward(x, om.means, om.bias)
        assert_close(y, want, gemm_tol(np.abs(x) @ np.abs(om.means).T + 1.0, 4e-6), "MAP output")


def test_lrt_forward_moments(nnmod, oracle):
    """SURVEY 8c KAT 8 (statistical, fixed seeds): over draws, LRT y has mean x mu^T + b and variance
    (x.x)(sigma^2)^T. 400 draws of a 64 x 32 output block: the mean of z is within 5 sigma / sqrt(n)."""
    opt, m, om = _layer_pair(nnmod, oracle, "lrt", 64, 32)
    x = np.random.default_rng(4).normal(0, 1, (64, 64)).astype(np.float32)
    mean_want = oracle.linear_forward(x, om.means, om.bias)
    var_want = (x * x) @ om.vars.T
    zs = []
    for _ in range(400):
        m.sample()
        zs.append((host(m.updateOutput(dev(x))) - mean_want) / np.sqrt(var_want))
    zs = np.stack(zs)
    assert abs(zs.mean()) < 5.0 / np.sqrt(zs.size)
    assert abs(zs.var() - 1.0) < 5.0 * np.sqrt(2.0 / zs.size)
    assert np.abs(zs.mean(axis=0)).max() < 6.0 / np.sqrt(400)


def test_lrt_rows_independent_of_sharding(nnmod, oracle):
    """Data-parallel invariance: rows [r0, r0+n) computed with row0 = r0 equal the same rows of the full batch."""
    opt, m, om = _layer_pair(nnmod, oracle, "lrt", 64, 48)
    x = np.random.default_rng(5).normal(0, 1, (32, 64)).astype(np.float32)
    m.sample()
    full = host(m.updateOutput(dev(x))).copy()
    m.row0 = 16
    part = host(m.updateOutput(dev(x[16:]))).copy()
    m.row0 = 0
    assert np.array_equal(full[16:], part)


# ------------------------------------------------------------------------------------------- whole MLP
@pytest.mark.parametrize("mode", ["wn", "lrt"])
def test_mlp_step_matches_oracle_f32(nnmod, oracle, mode):
    """BASELINE config 2: 784-400-400-10, batch 256, fp32, fixed RNG counter. mlp.lua call order:
    resetGradients, S x (sample, run), then the KL readout."""
    from vbnn_amd import mlp
    opt = opt_for(mode, S=2)
    net = mlp.buildModel(opt)
    onet = oracle.OracleMLP(opt)
    # identical parameters: take the oracle's (Philox-initialised) ones; means <- He weights so the net is not degenerate
    for k, i in enumerate(net.vb_indices):
        mod, om = net.model.get(i), onet.vb[k]
        np.testing.assert_array_equal(host(mod.weight).view(np.uint32), om.weight.view(np.uint32))
        om.means[:] = om.weight
        mod.means.copy_(mod.weight)
        mod.compute_prior(); om.compute_prior()
    last = net.model.get(2 * (len(opt["hidden"]) + 1))
    np.testing.assert_array_equal(host(last.weight).view(np.uint32), onet.last.weight.view(np.uint32))
    N = 256
    x = oracle.fill_normal(N, 784, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    net.resetGradients(); onet.resetGradients()
    for s in range(opt["S"]):
        net.sample(); onet.sample()
        err, acc = net.run(dev(x.reshape(N, 1, 28, 28)), dev(t))
        werr, wacc = onet.run(x.reshape(N, 1, 28, 28), t)
        assert abs(err - werr) <= 2e-5 * abs(werr) + 1e-6, (err, werr)
        assert abs(acc - wacc) <= 100.0 * 2 / N
        np.testing.assert_allclose(host(net.model.output), onet.outputs, rtol=0, atol=5e-5)
    for k, i in enumerate(net.vb_indices):
        mod, om = net.model.get(i), onet.vb[k]
        scale = np.abs(om.gradWeight).max()
        np.testing.assert_allclose(host(mod.gradWeight), om.gradWeight, rtol=0, atol=2e-5 * scale + 1e-9)
        np.testing.assert_allclose(host(mod.gradBias), om.gradBias, rtol=0, atol=2e-5 * np.abs(om.gradBias).max() + 1e-9)
        sscale = np.abs(om.gradSum).max()
        np.testing.assert_allclose(host(mod.gradSum), om.gradSum, rtol=0, atol=1e-4 * sscale + 1e-9)
    np.testing.assert_allclose(host(last.gradWeight), onet.last.gradWeight, rtol=0,
                               atol=2e-5 * np.abs(onet.last.gradWeight).max())
    lc, wlc = net.calc_lc(), onet.calc_lc()
    assert abs(lc - wlc) <= 2e-4 * abs(wlc) + 1e-9


# ------------------------------------------------------------------------------------------- fused engine
def _engine_pair(oracle, mode, dtype, hidden, I0, fuse_kl, S=2):
    from vbnn_amd.engine import FusedMLP
    opt = opt_for(mode, dtype, input_size=I0, hidden=hidden, S=S, fuse_kl=fuse_kl)
    eng = FusedMLP(opt)
    onet = oracle.OracleMLP(opt)
    rng = np.random.default_rng(7)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        np.testing.assert_array_equal(host(v.means).view(np.uint32), om.weight.view(np.uint32))   # same He stream
        lv = rng.normal(np.log(1e-3), 0.3, om.lvars.shape).astype(np.float32)
        b = rng.normal(0, 0.05, om.bias.shape).astype(np.float32)
        om.means[:] = om.weight; om.lvars[:] = lv; om.bias[:] = b
        v.lvars.copy_(dev(lv)); v.bias.copy_(dev(b))
        om.compute_prior()
    np.testing.assert_array_equal(host(eng.weight3).view(np.uint32), onet.last.weight.view(np.uint32))
    return opt, eng, onet


def _run_pair(opt, eng, onet, oracle, N, I0):
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    eng.resetGradients(); eng.prepare(); onet.resetGradients()
    werr = 0.0
    for _ in range(int(opt["S"])):
        eng.sample(); onet.sample()
        eng.run(dev(x), dev(t))
        e, _ = onet.run(x, t)
        werr += e
    loss, correct = eng.loss_and_accuracy()
    return loss, werr


@pytest.mark.parametrize("mode", ["lrt", "wn"])
@pytest.mark.parametrize("fuse_kl", [False, True])
def test_engine_matches_oracle_f32(oracle, nnmod, mode, fuse_kl):
    """The fused whole-step engine (epilogue-fused ReLU / packing / dv hand-off / KL gradients) computes
    what the module-by-module reference sequence computes. Shapes deliberately ragged (not multiples of
    the tile or of 4) plus BASELINE config 2."""
    for hidden, I0, N in ([[50, 34], 70, 37], [[400, 400], 784, 256]):
        opt, eng, onet = _engine_pair(oracle, mode, "f32", hidden, I0, fuse_kl)
        loss, werr = _run_pair(opt, eng, onet, oracle, N, I0)
        assert abs(loss - werr) <= 3e-5 * abs(werr) + 1e-6, (loss, werr)
        for k, v in enumerate(eng.vb):
            om = onet.vb[k]
            if fuse_kl:
                mle, mlc = om.compute_mugrads(opt)      # VBLinear.lua:131-134: mugrad = mleg + mlcg, vgrad = vleg + vlcg
                vle, vlc = om.compute_vargrads(opt)
                want_mu, want_lv = mle + mlc, vle + vlc
            else:
                want_mu, want_lv = om.gradWeight, om.gradSum
            np.testing.assert_allclose(host(v.gradWeight), want_mu, rtol=0, atol=3e-5 * np.abs(want_mu).max() + 1e-10)
            np.testing.assert_allclose(host(v.gradSum), want_lv, rtol=0, atol=2e-4 * np.abs(want_lv).max() + 1e-10)
            np.testing.assert_allclose(host(v.gradBias), om.gradBias, rtol=0, atol=3e-5 * np.abs(om.gradBias).max() + 1e-10)
        np.testing.assert_allclose(host(eng.gradWeight3), onet.last.gradWeight, rtol=0,
                                   atol=3e-5 * np.abs(onet.last.gradWeight).max())
        np.testing.assert_allclose(host(eng.gradBias3), onet.last.gradBias, rtol=0,
                                   atol=3e-5 * np.abs(onet.last.gradBias).max() + 1e-9)
        assert abs(eng.calc_lc() - onet.calc_lc()) <= 2e-4 * abs(onet.calc_lc()) + 1e-9


def _fuzz_nets():
    rng = np.random.default_rng(424242)
    nets = []
    for classes in (2, 7, 10, 13, 16, 20):                # <= 16: the fused classifier head; 20: the generic GEMM head
        depth = int(rng.integers(1, 4))
        nets.append(([int(rng.integers(1, 150)) for _ in range(depth)], int(rng.integers(1, 200)), int(rng.integers(1, 100)), classes))
    nets.append(([64, 128], 256, 64, 10))                 # whole tiles everywhere: every unguarded fast path
    nets.append(([1], 1, 1, 2))                           # the smallest network there is
    return nets


@pytest.mark.parametrize("hidden,I0,N,classes", _fuzz_nets())
@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_engine_matches_oracle_on_random_networks(oracle, nnmod, mode, hidden, I0, N, classes):
    """test_engine_matches_oracle_f32 on seeded random depths / widths / batch sizes / class counts (fp32, total
    gradients from the fused epilogue, S = 2): ragged everything, including the classifier head's class padding."""
    from vbnn_amd.engine import FusedMLP
    opt = opt_for(mode, "f32", input_size=I0, hidden=hidden, S=2, fuse_kl=True, n_classes=classes)
    eng, onet = FusedMLP(opt), oracle.OracleMLP(opt)
    rng = np.random.default_rng(9)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        lv = rng.normal(np.log(1e-3), 0.3, om.lvars.shape).astype(np.float32)
        b = rng.normal(0, 0.05, om.bias.shape).astype(np.float32)
        om.means[:] = om.weight; om.lvars[:] = lv; om.bias[:] = b
        v.lvars.copy_(dev(lv)); v.bias.copy_(dev(b))
        om.compute_prior()
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % classes).astype(np.int32)
    eng.resetGradients(); eng.prepare(); onet.resetGradients()
    werr = 0.0
    for _ in range(2):
        eng.sample(); onet.sample()
        eng.run(dev(x), dev(t))
        werr += onet.run(x, t)[0]
    loss, _ = eng.loss_and_accuracy()
    assert abs(loss - werr) <= 3e-5 * abs(werr) + 1e-6, (loss, werr)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        mle, mlc = om.compute_mugrads(opt)
        vle, vlc = om.compute_vargrads(opt)
        want_mu, want_lv = mle + mlc, vle + vlc
        np.testing.assert_allclose(host(v.gradWeight), want_mu, rtol=0, atol=3e-5 * np.abs(want_mu).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradSum), want_lv, rtol=0, atol=2e-4 * np.abs(want_lv).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradBias), om.gradBias, rtol=0, atol=3e-5 * np.abs(om.gradBias).max() + 1e-10)
    np.testing.assert_allclose(host(eng.gradWeight3), onet.last.gradWeight, rtol=0, atol=3e-5 * np.abs(onet.last.gradWeight).max() + 1e-10)
    np.testing.assert_allclose(host(eng.gradBias3), onet.last.gradBias, rtol=0, atol=3e-5 * np.abs(onet.last.gradBias).max() + 1e-9)


def _engine_masks(eng):
    """The ReLU on/off pattern the engine took: the stored (packed) activation of every VB layer is > 0."""
    acts = [v.x_s.t for v in eng.vb[1:]] + [eng.h_s.t]
    return [host(a[:, :v.O].float() > 0) for a, v in zip(acts, eng.vb)]


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_engine_bf16_close_to_f32_oracle(oracle, nnmod, gemm_kernel, mode):
    """bf16 operands / fp32 accumulate against the fp32 oracle on UNROUNDED operands, SURVEY 8c T2: 2e-2 relative.
    A bf16 rounding flips a fraction of a percent of the ReLU units on / off, and every flip moves a whole row's
    contribution in or out of a gradient sum -- a discontinuity, not an error of the arithmetic. The comparison is
    therefore mask-aware: the oracle takes the ReLU pattern the engine took (OracleMLP.run(masks=...)), what remains is
    rounding, held to 2e-2 (Frobenius; 2e-2 on the loss); the flip fraction itself is measured against the oracle's own
    pattern and bounded."""
    opt, eng, onet = _engine_pair(oracle, mode, "bf16", [400, 400], 784, False, S=1)
    N, I0 = 256, 784
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    eng.resetGradients(); eng.prepare(); eng.sample()
    eng.run(dev(x), dev(t))
    loss, _ = eng.loss_and_accuracy()
    masks = _engine_masks(eng)
    onet.resetGradients(); onet.sample()
    onet.run(x, t)                                            # the oracle's own pattern: how many units flipped?
    own = [om.output > 0 for om in onet.vb]
    flips = [float(np.mean(a != b)) for a, b in zip(masks, own)]
    assert max(flips) <= 1e-2, flips
    onet.resetGradients()
    for om in onet.vb:
        om.draw -= 1                                          # the same draw again
    onet.sample()
    werr, _ = onet.run(x, t, masks=masks)
    assert abs(loss - werr) <= 2e-2 * abs(werr), (loss, werr)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        for got, want, what in ((v.gradWeight, om.gradWeight, "gradWeight"), (v.gradSum, om.gradSum, "gradSum"),
                                (v.gradBias, om.gradBias, "gradBias")):
            rel_fro = np.linalg.norm(host(got) - want) / np.linalg.norm(want)
            assert rel_fro <= 2e-2, f"layer {k} {what}: relative Frobenius error {rel_fro:.3e} (flip fractions {flips})"


def _check_bf16_step_against_emulation(oracle, hidden, I0, N, fuse_kl, loss_tol=1e-4, fro_tol=2e-3, max_tol=2e-2, tgt=None):
    """The bf16 fused step against float64 math that rounds to bf16 at exactly the engine's rounding points
    (oracle/ref_numpy.emulate_lrt_step): identical ReLU masks, so what remains is fp32 accumulation order."""
    from oracle.ref_numpy import bf16_round, emulate_lrt_step
    opt, eng, onet = _engine_pair(oracle, "lrt", "bf16", hidden, I0, fuse_kl, S=1)
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32) if tgt is None else tgt
    eng.resetGradients(); eng.prepare(); eng.sample()
    eng.run(dev(x), dev(t))
    loss, _ = eng.loss_and_accuracy()
    layers = [dict(means=om.means, lvars=om.lvars, bias=om.bias) for om in onet.vb]
    zetas = [oracle.fill_normal(N, om.O, SEED, 2, k, 1, 0).astype(np.float64) for k, om in enumerate(onet.vb)]
    wloss, res, gw3, gb3 = emulate_lrt_step(layers, onet.last.weight, onet.last.bias, x, t, zetas, bf16_round,
                                            S=1.0, B=opt["B"], kl_shadows=eng.kl_from_shadows,
                                            kl_scale=0.0 if eng.kl_in_update else 1.0)
    assert abs(loss - wloss) <= loss_tol * abs(wloss), (loss, wloss)

    def close(got, want, what):
        got = host(got).astype(np.float64)
        fro = np.linalg.norm(got - want) / np.linalg.norm(want)
        mx = np.abs(got - want).max() / np.abs(want).max()
        assert fro <= fro_tol and mx <= max_tol, f"{what}: Frobenius {fro:.3e}, max {mx:.3e}"

    for k, v in enumerate(eng.vb):
        close(v.gradWeight, res[k]["grad_mu" if fuse_kl else "gradWeight"], f"layer {k} d/dmeans")
        close(v.gradSum, res[k]["grad_lv" if fuse_kl else "gradSum"], f"layer {k} d/dlvars")
        close(v.gradBias, res[k]["gradBias"], f"layer {k} gradBias")
    close(eng.gradWeight3, gw3, "final gradWeight")
    close(eng.gradBias3, gb3, "final gradBias")
    return eng


@pytest.mark.parametrize("hidden,I0,N", [([50, 34], 70, 37), ([400, 400], 784, 256), ([512, 384], 320, 640),
                                         ([512, 256], 256, 512),      # whole 256 x 256 tiles (gemm_v3.h)
                                         ([256, 256], 64, 256), ([256, 512], 128, 256), ([512, 256], 192, 256)])
                                         # the last three: 1, 2 and 3 K steps in the first forward (gemm_v3's peeled pipeline)
@pytest.mark.parametrize("fuse_kl", [False, True])
def test_engine_bf16_against_rounding_emulation(oracle, nnmod, gemm_kernel, hidden, I0, N, fuse_kl):
    """Bounds: loss 1e-4 relative; gradients 2e-3 Frobenius, 2e-2 of the largest entry."""
    _check_bf16_step_against_emulation(oracle, hidden, I0, N, fuse_kl)


@pytest.mark.parametrize("hidden,I0,N", [([256, 512], 100, 256),      # layer 1: ragged M with the ones row (101 of 256); layer 2: whole tiles
                                         ([512, 256], 260, 384),      # two M tiles, the second ragged (261 of 512); 3 K steps per half
                                         ([256, 256], 252, 128),      # the ones row is the LAST row of the quad before a tile edge
                                         ([256, 256], 100, 64), ([256, 256], 100, 192), ([256, 512], 100, 320)])
                                         # the last three: 1, 3 and 5 K steps (r04: the alternating half-height step's fill and its guarded last three steps)
def test_split_two_pass_gradient_against_rounding_emulation(oracle, nnmod, hidden, I0, N):
    """accGradParameters on gemm_v3's pair-split HALF-HEIGHT launch (forced: debug key 8), the launch of the 784 x 4096 gradient:
    128-row tiles, every workgroup walks all of K; ragged output rows, the bias gradient from the ones row."""
    from vbnn_amd import _lib as L
    L.check(L.lib().vbnn_debug_set(8, 1))
    try:
        eng = _check_bf16_step_against_emulation(oracle, hidden, I0, N, True)
        assert all(v.dw_km for v in eng.vb) and eng.vb[0].x_pad256
        g1 = eng.grads.clone()
        for _ in range(3):
            eng.resetGradients(); eng.run(eng_x(eng, oracle, N, I0), eng_t(N))
            assert torch.equal(eng.grads, g1)
        k, ak, fam, f = gemm_form()                      # the step's last GEMM: an accGradParameters on the split launch
        assert k == 7 and ak and fam == 3, f"the last launch was the {GEMM_KERNELS[k]} kernel (form {f:#x}), not the split launch"
    finally:
        L.check(L.lib().vbnn_debug_set(8, -1))


def test_nan_in_the_backward_shows_in_the_loss_and_the_layers_gradients_but_not_below_the_two_pass_gradinput(nnmod):
    """The one place where the bf16 path is NOT NaN-transparent, pinned. gemm_v3's
    updateGradInput carries the ReLU mask of the module in between through its second pass as a quiet NaN in the accumulator and
    reads it back as `a != a` (csrc/epilogues.h, EpiDx::fold / apply_folded): a GENUINE NaN arriving in gradOutput -- a diverged
    run -- is zeroed in g_prev with it, where the reference's model:backward (mlp.lua:79) would carry it into every layer below.
    What still shows it, and what a host must therefore look at before update(): the loss, and the gradients of the layer the
    NaN arrived at. Here: one NaN planted in the final Linear's weight -> NaN logits for every row -> the loss is NaN, the last
    VB layer's d/dmeans and the final Linear's gradWeight are NaN; below the two-pass gradInput launch g / gv are finite (zeros)
    and the first layer's gradients are finite. (train.py raises on the non-finite loss; INTEGRATION.md, error behaviour.)"""
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP
    I0, N, hidden = 64, 256, [256, 256]
    L.check(L.lib().vbnn_debug_set(0, 3))                # the two-pass 256 x 256 kernel wherever the shape allows (the wide configuration's kernel)
    try:
        opt = opt_for("lrt", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True)
        eng = FusedMLP(opt)
        x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
        nnmod.fill_normal(x, SEED, 4, 0, 0)
        t = eng_t(N)
        eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t)
        loss0, _ = eng.loss_and_accuracy()
        assert eng.vb[1].dx_km, "layer 2's gradInput must run on the two-pass kernel for this test to test anything"
        assert np.isfinite(loss0) and bool(torch.isfinite(eng.grads).all())
        assert float(eng.vb[0].g_s.t.float().abs().max()) > 0.0
        eng.weight3[3, 17] = float("nan")
        eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t)
        loss, _ = eng.loss_and_accuracy()
        assert np.isnan(loss), loss                                                     # the criterion shows it
        assert bool(torch.isnan(eng.gradWeight3).any()) and bool(torch.isnan(eng.vb[1].gradWeight).any())   # and so do the gradients above
        g_below = eng.vb[0].g_s.t.float()
        assert bool(torch.isfinite(g_below).all()) and float(g_below.abs().max()) == 0.0, "the quirk: g below the two-pass gradInput is zeroed, not NaN"
        assert bool(torch.isfinite(eng.vb[0].gradWeight).all()) and bool(torch.isfinite(eng.vb[0].gradSum).all())
    finally:
        L.check(L.lib().vbnn_debug_set(0, 0))


def test_wide_training_steps_repeat_bit_for_bit(nnmod):
    """The race screen of the pipelined kernels at bench size: two engines from the same seed run the same three training steps of the
    wide configuration (every timed launch: two-pass 256 x 256 forward / gradInput / accGradParameters with their alternating K steps,
    the half-height launch, the fused head, the update sweep) and must leave the same bits in the gradient arena, the operand shadows
    and the loss after every step (tools/step_bits.py: the same hashes also compare two BUILDS of the library)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("step_bits", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "step_bits.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    reps = sb.run("wide", 3, 2, out=lambda *a, **k: None)
    assert reps[0] == reps[1] and len(reps[0]) == 3
    assert len({line.split()[3] for line in reps[0]}) == 3          # the gradients do change from step to step


def eng_x(eng, oracle, N, I0):
    return dev(oracle.fill_normal(N, I0, SEED, 4, 0, 0))


def eng_t(N):
    return dev((np.arange(N) * 7 % 10).astype(np.int32))


def test_full_size_wide_step_against_rounding_emulation(oracle, nnmod):
    """BASELINE.json's headline configuration -- 784-4096-4096-10, batch 4096, bf16, LRT, S = 1, exactly the launches
    bench.py times (two-pass 256 x 256 forward / gradInput / accGradParameters with K-major operands and the fused KL
    epilogue at N = I = O = 4096; the split launch for the 784 x 4096 gradient) -- against float64 BLAS on identically
    rounded operands (VBLinear.lua:90-98,112-118 restated in oracle/ref_numpy.emulate_lrt_step). Loss 1e-4, gradients
    2e-3 Frobenius / 2e-2 of the largest entry, as the small cases."""
    eng = _check_bf16_step_against_emulation(oracle, [4096, 4096], 784, 4096, True)
    assert eng.vb[1].dw_km and eng.vb[1].dx_km and eng.vb[0].dw_km      # the K-major launches were the ones checked
    k, ak, fam, f = gemm_form()                                         # the step's last GEMM: a K-major accGradParameters
    assert k in (6, 7) and ak and fam == 3, f"the last launch was the {GEMM_KERNELS[k]} kernel (form {f:#x})"


def test_full_size_layer2_backward_launches_against_float64(oracle, nnmod):
    """The two timed backward launches of the widest layer on their own, at N = I = O = 4096, from GIVEN operands:
    vbnn_grad_input (K-major mu / sigma^2, fold 2 x . (gv sigma^2), ReLU mask, x r hand-off) and
    vbnn_acc_grad_parameters (K-major x / g, d/dlvars finished between the passes, fused KL gradient) against
    float64 BLAS on the same bf16 values. Per-element bound from the operands' absolute products."""
    import ctypes as C
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP, _p
    from oracle.ref_numpy import bf16_round
    N = I = O = 4096
    opt = opt_for("lrt", "bf16", input_size=I, hidden=[I, O], S=1, fuse_kl=True)
    eng = FusedMLP(opt)
    rng = np.random.default_rng(11)
    v, p = eng.vb[1], eng.vb[0]
    lv = rng.normal(np.log(1e-3), 0.3, (O, I)).astype(np.float32)
    v.lvars.copy_(dev(lv))
    eng._alloc_batch(N)
    eng.prepare()
    torch.cuda.synchronize()
    assert v.dw_km and v.dx_km
    f8 = np.float64
    # operands as the forward / head would have left them (any bf16 values do): x >= 0 with zeros (a ReLU output)
    x = bf16_round(np.maximum(rng.normal(0, 1, (N, I)), 0).astype(np.float32))
    g = bf16_round(rng.normal(0, 1e-3, (N, O)).astype(np.float32))
    gv = bf16_round((g * rng.normal(0, 3.0, (N, O))).astype(np.float32))
    rp = bf16_round(rng.normal(0, 3.0, (N, I)).astype(np.float32))
    v.x_s.t[:, :I].copy_(dev(x)); v.x2_s.t[:, :I].copy_(dev(bf16_round(x * x)))
    v.g_s.t[:, :O].copy_(dev(g)); v.gv_s.t[:, :O].copy_(dev(gv))
    p.r[:, :I].copy_(dev(rp))
    x2 = host(v.x2_s.t[:, :I].float()).astype(f8)
    mu, var = host(v.mu_s.t[:, :I].float()).astype(f8), host(v.var_s.t[:, :I].float()).astype(f8)
    lib, ctx = L.lib(), eng.ctx.h
    # ---- updateGradInput
    L.check(lib.vbnn_grad_input(ctx, eng.code, C.byref(eng._dx_args(1, N))))
    k, ak, fam, f = gemm_form()
    assert k == 6 and ak and fam == 2, f"gradInput ran the {GEMM_KERNELS[k]} kernel (form {f:#x}), not the K-major two-pass launch"
    t1 = g.astype(f8) @ mu
    t2 = 2 * x.astype(f8) * (gv.astype(f8) @ var)
    want = np.where(x > 0, t1 + t2, 0.0)
    tol = 4e-6 * (np.abs(g).astype(f8) @ np.abs(mu) + 2 * x * (np.abs(gv).astype(f8) @ var)) + 1e-12
    got_g = host(p.g_s.t[:, :I].float()).astype(f8)
    err = np.abs(got_g - want)
    assert (err <= tol + 2.0 ** -8 * np.abs(want)).all(), f"g_prev: {(err > tol + 2.0 ** -8 * np.abs(want)).sum()} off, max {err.max():.3e}"
    got_gv = host(p.gv_s.t[:, :I].float()).astype(f8)
    want_gv = want * rp
    assert (np.abs(got_gv - want_gv) <= (tol + 2.0 ** -8 * np.abs(want)) * np.abs(rp) + 2.0 ** -8 * np.abs(want_gv)).all()
    # ---- accGradParameters with the fused KL gradient
    L.check(lib.vbnn_acc_grad_parameters(ctx, eng.code, C.byref(eng._dw_args(1, N, 0))))
    k, ak, fam, f = gemm_form()
    assert k == 6 and ak and fam == 3, f"accGradParameters ran the {GEMM_KERNELS[k]} kernel (form {f:#x}), not the K-major two-pass launch"
    gw = g.astype(f8).T @ x.astype(f8)
    gs2 = gv.astype(f8).T @ x2
    var32 = np.exp(lv).astype(f8)
    means = host(v.means).astype(f8)
    vh = float(np.sum(var32 + means ** 2) / means.size)
    B = opt["B"]
    assert eng.kl_from_shadows                                # the epilogue reads the bf16 shadows (vbnn_dw_args.mu_s / var_s)
    klk = 0.0 if eng.kl_in_update else 1.0                     # (default: the arena holds the likelihood parts, update() adds the KL)
    want_mu = gw + klk * mu / (B * vh)
    want_lv = gs2 * var + klk * (var / vh - 1.0) / (2 * B)
    var32 = var
    tol_mu = 4e-6 * (np.abs(g).astype(f8).T @ np.abs(x).astype(f8)) + 1e-12
    tol_lv = 4e-6 * (np.abs(gv).astype(f8).T @ x2) * var32 * 1.001 + 1e-5 * np.abs(want_lv) + 1e-12
    e_mu, e_lv = np.abs(host(v.gradWeight) - want_mu), np.abs(host(v.gradSum) - want_lv)
    assert (e_mu <= tol_mu).all(), f"d/dmeans: {(e_mu > tol_mu).sum()} off, max {e_mu.max():.3e}"
    assert (e_lv <= tol_lv).all(), f"d/dlvars: {(e_lv > tol_lv).sum()} off, max {e_lv.max():.3e}"


def test_committed_golden_vectors_on_the_gpu(nnmod):
    """tests/golden/vblinear_small.npz (inputs + expected outputs, made by tests/golden/make_golden.py) through the HIP
    path: no oracle at run time. fp32 modules, both modes, two draws with scale 0.5, S = 2 KL gradients."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vblinear_small.npz"))
    np.testing.assert_array_equal(host(_filled(nnmod, 5, 7, 1, 1, 1, 0)).view(np.uint32), gold["normal_eps_5x7"].view(np.uint32))
    np.testing.assert_array_equal(host(_filled(nnmod, 3, 5, 2, 2, 7, 1000)).view(np.uint32),
                                  gold["normal_zeta_3x5_row1000"].view(np.uint32))
    for mode in ("wn", "lrt"):
        for N, I, O in ((3, 7, 5), (32, 64, 48)):
            k = f"{mode}_{N}x{I}x{O}"
            opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=2, mode=mode, seed=3, dtype="f32", keep_e=True)
            m = nnmod.VBLinear(I, O, opt)
            m.set_layer_id(1)
            m.means.copy_(dev(gold[k + "_in_means"])); m.lvars.copy_(dev(gold[k + "_in_lvars"])); m.bias.copy_(dev(gold[k + "_in_bias"]))
            m.compute_prior()
            x, g = gold[k + "_in_x"], gold[k + "_in_g"]
            sc = lambda a: 1e-5 * np.abs(a).max() + 1e-7
            for d in range(2):
                m.sample()
                np.testing.assert_allclose(host(m.updateOutput(dev(x))), gold[f"{k}_out_output{d}"], rtol=0, atol=sc(gold[f"{k}_out_output{d}"]))
                np.testing.assert_allclose(host(m.backward(dev(x), dev(g), 0.5)), gold[f"{k}_out_gradInput{d}"], rtol=0,
                                           atol=sc(gold[f"{k}_out_gradInput{d}"]))
            for name, got in (("gradWeight", m.gradWeight), ("gradSum", m.gradSum), ("gradBias", m.gradBias)):
                np.testing.assert_allclose(host(got), gold[f"{k}_out_{name}"], rtol=0, atol=4 * sc(gold[f"{k}_out_{name}"]))
            assert abs(m.var_hat - float(gold[k + "_out_var_hat"])) <= 1e-6 * float(gold[k + "_out_var_hat"])
            assert abs(float(m.calc_lc(opt).item()) - float(gold[k + "_out_lc"])) <= 2e-4 * abs(float(gold[k + "_out_lc"])) + 1e-9
            mle, mlc = m.compute_mugrads(opt)
            vle, vlc = m.compute_vargrads(opt)
            for name, got in (("mugrad_le", mle), ("mugrad_lc", mlc), ("vargrad_le", vle), ("vargrad_lc", vlc)):
                np.testing.assert_allclose(host(got), gold[f"{k}_out_{name}"], rtol=1e-4, atol=4 * sc(gold[f"{k}_out_{name}"]))


def _filled(nnmod, rows, cols, stream, layer, draw, row0):
    t = torch.empty(rows, cols, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(t, SEED, stream, layer, draw, row0=row0)
    return t


@pytest.fixture(params=[(1, 0, 0), (2, 256, 0), (2, 128, 0), (2, 64, 0), (3, 0, -1), (2, 256, 1)],
                ids=["general-kernel", "pipelined-256x128", "pipelined-128x128", "pipelined-128x128-pairs",
                     "two-pass-256x256", "pipelined-256x128-pairsplit"])
def gemm_kernel(request, nnmod):
    """Run a bf16 test once per SETTING of the kernel keys (gemm_v1.h / gemm_v2.h in its block tiles and with the pair split /
    gemm_v3.h), whatever the shape heuristics say. Settings 1 and 2 take every launch of the module path; the last setting,
    "two-pass-256x256", only asks for gemm_v3.h where shape and outputs allow it, and the module path's fp32 outputs never do:
    those cases run the general or the pipelined kernel (check_forced_kernel prints which). The two-pass kernel is held by
    tests/test_gemm_forms_gpu.py and by the engine tests."""
    from vbnn_amd import _lib as L
    kernel, tile, psplit = request.param
    L.check(L.lib().vbnn_debug_set(0, kernel))
    L.check(L.lib().vbnn_debug_set(2, tile))
    L.check(L.lib().vbnn_debug_set(5, psplit))
    yield request.param
    L.check(L.lib().vbnn_debug_set(0, 0))
    L.check(L.lib().vbnn_debug_set(2, 0))
    L.check(L.lib().vbnn_debug_set(5, -1))


@pytest.mark.parametrize("N,I,O", [(1, 8, 8), (37, 70, 50), (300, 200, 260), (512, 448, 384), (200, 4096, 130),
                                   (512, 256, 768)])
def test_bf16_gemm_exact_on_integers(nnmod, gemm_kernel, N, I, O):
    """Layout / race screen: small-integer operands are exact in bf16 and their sums exact in fp32, so
    y = x W^T + b, gradInput = g W and gradWeight = g^T x must equal the integer results EXACTLY, for both
    bf16 kernels, on ragged shapes (asymmetric operands, so a transposed or permuted tile cannot pass)."""
    rng = np.random.default_rng(N * 1000 + I)
    W = rng.integers(-3, 4, (O, I)).astype(np.float32)
    b = rng.integers(-5, 6, O).astype(np.float32)
    x = rng.integers(-3, 4, (N, I)).astype(np.float32)
    g = rng.integers(-2, 3, (N, O)).astype(np.float32)
    m = nnmod.Linear(I, O, dict(dtype="bf16"))
    m.weight.copy_(dev(W)); m.bias.copy_(dev(b))
    for it in range(3):                                  # repeated launches: a race would not repeat exactly
        y = host(m.updateOutput(dev(x)))
        if it == 0:
            check_forced_kernel(gemm_kernel[0], f"forward {N}x{I}x{O}")
        assert np.array_equal(y, x @ W.T + b)
        m.gradWeight.zero_(); m.gradBias.zero_()
        gx = host(m.backward(dev(x), dev(g), 1.0))
        assert np.array_equal(gx, g @ W)
        assert np.array_equal(host(m.gradWeight), g.T @ x)
        assert np.array_equal(host(m.gradBias), g.sum(axis=0))


@pytest.mark.parametrize("N,I,O", [(256, 64, 256), (256, 128, 512), (512, 192, 256), (256, 256, 256), (512, 320, 256)])
def test_two_pass_kernel_short_k(nnmod, N, I, O):
    """nn.Linear at whole 256 x 256 tiles and 1, 2, 3, 4 and 5 K steps under debug key 0 = 3. Written for gemm_v3's peeled pipeline
    (prologue of two steps, unguarded main loop, guarded last two steps) -- but the module path's fp32 outputs keep these launches
    off the two-pass kernel (check_forced_kernel prints which kernel ran): what this holds is the fall-back of key 3. The peeled
    pipeline at these K in each of its three roles is run by tests/test_gemm_forms_gpu.py::test_two_pass_kernel."""
    from vbnn_amd import _lib as L
    L.check(L.lib().vbnn_debug_set(0, 3))
    try:
        rng = np.random.default_rng(N + I + O)
        W = rng.integers(-3, 4, (O, I)).astype(np.float32)
        b = rng.integers(-5, 6, O).astype(np.float32)
        x = rng.integers(-3, 4, (N, I)).astype(np.float32)
        g = rng.integers(-2, 3, (N, O)).astype(np.float32)
        m = nnmod.Linear(I, O, dict(dtype="bf16"))
        m.weight.copy_(dev(W)); m.bias.copy_(dev(b))
        for it in range(2):
            y = host(m.updateOutput(dev(x)))
            if it == 0:
                check_forced_kernel(3, f"forward {N}x{I}x{O}")
            assert np.array_equal(y, x @ W.T + b)
            m.gradWeight.zero_(); m.gradBias.zero_()
            assert np.array_equal(host(m.backward(dev(x), dev(g), 1.0)), g @ W)
            assert np.array_equal(host(m.gradWeight), g.T @ x)
    finally:
        L.check(L.lib().vbnn_debug_set(0, 0))


def _fuzz_shapes():
    rng = np.random.default_rng(20260401)
    shapes = [(int(rng.integers(1, 700)), int(rng.integers(1, 900)), int(rng.integers(1, 700))) for _ in range(10)]
    # tile-boundary neighbours of the three kernels' block tiles (32 / 64 / 128 / 256) and of the 64-element K step
    shapes += [(255, 64, 257), (256, 63, 256), (257, 65, 255), (129, 128, 127), (1024, 192, 1280), (768, 1088, 1025)]
    return shapes


@pytest.mark.parametrize("N,I,O", _fuzz_shapes())
def test_bf16_gemm_exact_on_random_shapes(nnmod, N, I, O):
    """The same exactness screen as test_bf16_gemm_exact_on_integers on seeded random and tile-boundary shapes, with the
    library's OWN kernel choice per shape (no debug key): whatever the heuristics pick must be exact on ragged edges."""
    rng = np.random.default_rng(N * 7919 + I * 31 + O)
    W = rng.integers(-3, 4, (O, I)).astype(np.float32)
    b = rng.integers(-5, 6, O).astype(np.float32)
    x = rng.integers(-3, 4, (N, I)).astype(np.float32)
    g = rng.integers(-2, 3, (N, O)).astype(np.float32)
    m = nnmod.Linear(I, O, dict(dtype="bf16"))
    m.weight.copy_(dev(W)); m.bias.copy_(dev(b))
    for _ in range(2):
        assert np.array_equal(host(m.updateOutput(dev(x))), x @ W.T + b)
        m.gradWeight.zero_(); m.gradBias.zero_()
        assert np.array_equal(host(m.backward(dev(x), dev(g), 1.0)), g @ W)
        assert np.array_equal(host(m.gradWeight), g.T @ x)
        assert np.array_equal(host(m.gradBias), g.sum(axis=0))


@pytest.mark.parametrize("N,I,O", [(3, 7, 5), (100, 130, 70), (256, 784, 400)])
def test_layer_bf16_against_rounded_operands(nnmod, oracle, gemm_kernel, N, I, O):
    """bf16 MFMA path of one VBLinear (LRT) against float64 math on the SAME bf16-rounded operands
    (oracle/ref_numpy.py): only the fp32 accumulation order differs. atol 1e-3 * max|.|, as SURVEY 8c T2."""
    from oracle.ref_numpy import bf16_round as rb
    opt, m, om = _layer_pair(nnmod, oracle, "lrt", I, O, dtype="bf16")
    rng = np.random.default_rng(11)
    x = rng.normal(0, 1, (N, I)).astype(np.float32)
    g = rng.normal(0, 1.0 / N, (N, O)).astype(np.float32)
    m.sample()
    y = host(m.updateOutput(dev(x))).astype(np.float64)
    check_forced_kernel(gemm_kernel[0], f"LRT forward {N}x{I}x{O}")
    zeta = oracle.fill_normal(N, O, SEED, 2, 0, m.draw, 0).astype(np.float64)
    xr, mur = rb(x).astype(np.float64), rb(om.means).astype(np.float64)
    x2r = rb(rb(x) * rb(x)).astype(np.float64)
    varr = rb(np.exp(om.lvars)).astype(np.float64)
    v = x2r @ varr.T
    want_y = xr @ mur.T + om.bias + np.sqrt(v) * zeta
    assert np.abs(y - want_y).max() <= 1e-3 * np.abs(want_y).max()
    r = zeta / (2 * np.sqrt(v))
    np.testing.assert_allclose(host(m.r), r, rtol=1e-3, atol=1e-6)
    gx = host(m.backward(dev(x), dev(g), 1.0)).astype(np.float64)
    r32 = host(m.r)
    gr = rb(g).astype(np.float64)
    gvr = rb(g * r32).astype(np.float64)
    want_gx = gr @ mur + 2 * xr * (gvr @ varr)
    assert np.abs(gx - want_gx).max() <= 1e-3 * np.abs(want_gx).max()
    want_gw = gr.T @ xr
    assert np.abs(host(m.gradWeight) - want_gw).max() <= 1e-3 * np.abs(want_gw).max()
    want_gs = 2 * (gvr.T @ x2r) * np.sqrt(np.exp(om.lvars.astype(np.float64)))
    assert np.abs(host(m.gradSum) - want_gs).max() <= 1e-3 * np.abs(want_gs).max()


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_engine_deep_stack_matches_oracle(oracle, nnmod, mode):
    """BASELINE configs[4]'s structure (a deep stack of VB layers) at test scale: five VB layers, three draws
    accumulated with the fused KL epilogue (the gradInput hand-off chain runs through four ReLUs)."""
    hidden, I0, N = [48, 40, 36, 32, 28], 44, 33
    opt, eng, onet = _engine_pair(oracle, mode, "f32", hidden, I0, True, S=3)
    loss, werr = _run_pair(opt, eng, onet, oracle, N, I0)
    assert abs(loss - werr) <= 5e-5 * abs(werr) + 1e-6, (loss, werr)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        mle, mlc = om.compute_mugrads(opt)
        vle, vlc = om.compute_vargrads(opt)
        want_mu, want_lv = mle + mlc, vle + vlc
        np.testing.assert_allclose(host(v.gradWeight), want_mu, rtol=0, atol=5e-5 * np.abs(want_mu).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradSum), want_lv, rtol=0, atol=3e-4 * np.abs(want_lv).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradBias), om.gradBias, rtol=0, atol=5e-5 * np.abs(om.gradBias).max() + 1e-10)


# ------------------------------------------------------------------------------------------- BASELINE.json's full sizes
def test_full_size_bf16_layer_exact_on_integers(nnmod):
    """The 4096 x 4096 layer at batch 4096 (BASELINE configs[2]) on integer operands: forward, gradInput and
    gradWeight of the pipelined kernel must equal the integer results exactly (fp32 sgemm on the host is exact
    here too: every partial sum stays below 2^24)."""
    N = I = O = 4096
    rng = np.random.default_rng(4096)
    W = rng.integers(-3, 4, (O, I)).astype(np.float32)
    b = rng.integers(-5, 6, O).astype(np.float32)
    x = rng.integers(-3, 4, (N, I)).astype(np.float32)
    g = rng.integers(-2, 3, (N, O)).astype(np.float32)
    m = nnmod.Linear(I, O, dict(dtype="bf16"))
    m.weight.copy_(dev(W)); m.bias.copy_(dev(b))
    y = host(m.updateOutput(dev(x)))
    assert np.array_equal(y, x @ W.T + b)
    m.gradWeight.zero_(); m.gradBias.zero_()
    gx = host(m.backward(dev(x), dev(g), 1.0))
    assert np.array_equal(gx, g @ W)
    assert np.array_equal(host(m.gradWeight), g.T @ x)
    assert np.array_equal(host(m.gradBias), g.sum(axis=0))


def test_full_size_lrt_forward_against_rounded_operands(nnmod, oracle):
    """The wide configuration's second VB layer (4096 -> 4096, batch 4096, bf16, LRT): y against float64 BLAS on
    identically rounded operands (oracle/ref_numpy.lrt_forward), 1e-3 of max|y|; the noise is the oracle's Philox
    stream for global rows, and an all-zero input row must come out finite with r = 0."""
    from oracle.ref_numpy import bf16_round, lrt_forward
    N = I = O = 4096
    opt, m, om = _layer_pair(nnmod, oracle, "lrt", I, O, dtype="bf16")
    x = oracle.fill_normal(N, I, SEED, 4, 9, 0)
    x[17, :] = 0.0
    m.sample(); m.row0 = 8192
    y = host(m.updateOutput(dev(x))).astype(np.float64)
    zeta = oracle.fill_normal(N, O, SEED, 2, 0, m.draw, 8192).astype(np.float64)
    want, v = lrt_forward(x, om.means, om.lvars, om.bias.astype(np.float64), zeta, bf16_round)
    assert np.abs(y - want).max() <= 1e-3 * np.abs(want).max()
    r = host(m.r)
    assert np.isfinite(r).all() and np.all(r[17] == 0.0)
    m.row0 = 0


def test_empty_batch_is_an_error_not_a_crash(nnmod):
    from vbnn_amd import _lib as L
    m = nnmod.Linear(8, 4)
    with pytest.raises(L.VbnnError):
        m.updateOutput(torch.zeros(0, 8, device="cuda"))


# ------------------------------------------------------------------------------------------- MC loop / test path
@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_engine_test_path_matches_oracle(oracle, nnmod, mode):
    """mlp:test (mlp.lua:86-107): quicktest = clamp_to_map + one pass; otherwise the mean over testSamples draws."""
    N, I0 = 37, 70
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    for quick in (True, False):
        opt, eng, onet = _engine_pair(oracle, mode, "f32", [50, 34], I0, True, S=1)
        opt["quicktest"] = quick
        opt["testSamples"] = 3
        err, acc = eng.test(dev(x), dev(t))
        if quick:
            for om in onet.vb:
                om.clamp_to_map()
            werr, wacc = onet.run(x, t)
        else:
            werr = wacc = 0.0
            for _ in range(3):
                onet.sample()
                e, a = onet.run(x, t)
                werr += e / 3; wacc += a / 3
        assert abs(err - werr) <= 3e-5 * abs(werr) + 1e-6, (quick, err, werr)
        assert abs(acc - wacc) <= 100.0 * 1.01 / N


def test_head_logits_from_the_forward_tiles_equal_the_heads_own_pass_over_h(oracle, nnmod):
    """vbnn_fwd_args.head_slots (r04): the last VB layer's forward forms the final Linear's logits from its output tiles while
    they are in registers -- [2 x 16 tiles of m][N][16] fp32 partials in fixed slots, added in order by the head. Against (1) a
    float64 product of the stored h and the packed final weight (per-element fp32 accumulation bound), (2) an engine whose head
    reads h itself (opt.head_from_h: the same numbers in another summation order), (3) itself, bitwise, on a second run; and the
    whole step's gradients agree with the head_from_h engine's to fp32 rounding. MAP passes (single GEMM) carry the logits too."""
    from vbnn_amd.engine import FusedMLP
    I0, N, hidden = 256, 4096, [1024, 4096]
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    res = {}
    for name, extra in (("slots", {}), ("from_h", dict(head_from_h=True))):
        opt = opt_for("lrt", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True, **extra)
        eng = FusedMLP(opt)
        eng.bias3.copy_(torch.linspace(-0.5, 0.5, 10, device="cuda"))
        # NON-ZERO VB biases: what every layer holds after its first SGD step. The single-GEMM launch of a
        # MAP / weight-noise pass has W x in its accumulators, not W x + b: with the biases at their initial zero the logits
        # taken from relu(W x) passed this test.
        for v in eng.vb:
            v.bias.copy_(torch.linspace(-0.4, 0.6, v.O, device="cuda"))
        runs = []
        for rep in range(2):
            eng.draw = 0
            eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t)
            loss, hits = eng.loss_and_accuracy()
            runs.append((loss, hits, host(eng.logits).copy(), host(eng.grads).copy()))
        assert (eng.n_head_slots > 0) == (name == "slots"), (name, eng.n_head_slots)
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32))
        assert np.array_equal(runs[0][3].view(np.uint32), runs[1][3].view(np.uint32)), f"{name}: gradients differ between two runs"
        h = host(eng.h_s.t[:, :hidden[-1]].float()).astype(np.float64)
        w3 = host(eng.w3_s.t[:, :hidden[-1]].float()).astype(np.float64)
        want = h @ w3.T + host(eng.bias3).astype(np.float64)
        bound = 4e-6 * (np.abs(h) @ np.abs(w3).T) + 1e-6
        err = np.abs(runs[0][2] - want)
        assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} logits off, max {err.max():.3e}"
        # MAP pass, forward only (mlp.lua:88-92): the single-GEMM launch carries the logits as well
        eng.resetGradients(); eng.clamp_to_map(); eng.run(x, t, backward=False)
        lm, _ = eng.loss_and_accuracy()
        hm = host(eng.h_s.t[:, :hidden[-1]].float()).astype(np.float64)
        wantm = hm @ w3.T + host(eng.bias3).astype(np.float64)
        errm = np.abs(host(eng.logits) - wantm)
        assert (errm <= 4e-6 * (np.abs(hm) @ np.abs(w3).T) + 1e-6).all(), f"{name} MAP: max {errm.max():.3e}"
        res[name] = runs[0] + (lm,)
    a, b = res["slots"], res["from_h"]
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2, (a[0], b[0], a[1], b[1])
    assert abs(a[4] - b[4]) <= 1e-6 * abs(b[4])
    rel = np.linalg.norm(a[3] - b[3]) / np.linalg.norm(b[3])
    assert rel <= 1e-4, f"gradient arenas of the two head forms: relative Frobenius {rel:.3e}"
    # weight-noise mode (the reference's own estimator, VBLinear.lua:49-64): every forward is the single-GEMM launch, with backward
    wn = {}
    for name, extra in (("slots", {}), ("from_h", dict(head_from_h=True))):
        opt = opt_for("wn", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True, **extra)
        eng = FusedMLP(opt)
        eng.bias3.copy_(torch.linspace(-0.5, 0.5, 10, device="cuda"))
        for v in eng.vb:
            v.bias.copy_(torch.linspace(-0.4, 0.6, v.O, device="cuda"))
        eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t)
        loss, hits = eng.loss_and_accuracy()
        assert (eng.n_head_slots > 0) == (name == "slots"), (name, eng.n_head_slots)
        h = host(eng.h_s.t[:, :hidden[-1]].float()).astype(np.float64)
        w3 = host(eng.w3_s.t[:, :hidden[-1]].float()).astype(np.float64)
        want = h @ w3.T + host(eng.bias3).astype(np.float64)
        err = np.abs(host(eng.logits) - want)
        assert (err <= 4e-6 * (np.abs(h) @ np.abs(w3).T) + 1e-6).all(), f"wn {name}: max {err.max():.3e}"
        wn[name] = (loss, hits, host(eng.grads).copy())
    a, b = wn["slots"], wn["from_h"]
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2, (a[0], b[0], a[1], b[1])
    rel = np.linalg.norm(a[2] - b[2]) / np.linalg.norm(b[2])
    assert rel <= 1e-4, f"weight-noise gradient arenas of the two head forms: relative Frobenius {rel:.3e}"


@pytest.mark.parametrize("N,H,C,with_r", [(4096, 4096, 10, True), (512, 256, 10, True), (320, 384, 3, True), (64, 128, 12, False), (1024, 1024, 1, True)])
def test_streaming_head_backward_agrees_with_the_tile_form_and_with_float64(nnmod, N, H, C, with_r):
    """The fused head's backward in its STREAMING form (r05, k_head_backward_stream: no LDS in the loop, four waves per SIMD,
    d(loss)/d(logits) as scalar operands of v_dot2c_f32_bf16) against the tile form (k_head_backward: MFMA sums over LDS tiles), forced
    one after the other through vbnn_debug_set(VBNN_DEBUG_HEAD_BACKWARD), and both against float64 on the same bf16 operands:
    g_prev = (round_bf16(g) W3) . [h > 0], gv_prev = g_prev . r (bf16 outputs: equal up to one bf16 ulp where the fp32 sums round
    differently), gradWeight = round_bf16(g)^T h, the layer below's bias gradient = column sums of the ROUNDED g_prev, the final
    bias gradient = column sums of the unrounded g; with accumulate = 1 on top of what is there. Ragged class counts (1, 3, 12),
    a net without r (weight-noise mode), sizes whose partial sums the tile form would finish in-launch."""
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context, _Packed, _p
    lib, ctx = L.lib(), Context.get(torch.device("cuda", 0))
    gen = torch.Generator(device="cuda").manual_seed(N + H + C)
    bf = torch.bfloat16
    hs, rs, w3 = _Packed(N, H, bf, "cuda"), _Packed(N, H, bf, "cuda"), _Packed(C, H, bf, "cuda")
    hs.t[:, :H] = torch.relu(torch.randn(N, H, device="cuda", generator=gen)).to(bf)
    rs.t[:, :H] = (0.5 * torch.randn(N, H, device="cuda", generator=gen)).to(bf)
    w3.t[:, :H] = (torch.randn(C, H, device="cuda", generator=gen) / 8).to(bf)
    g = (torch.randn(N, C, device="cuda", generator=gen) / N).contiguous()
    base = {k: torch.randn(*shape, device="cuda", generator=gen) for k, shape in (("gw", (C, H)), ("gb", (C,)), ("gbp", (H,)))}
    res = {}
    try:
        for form in (0, 1):
            L.check(lib.vbnn_debug_set(10, form))
            outs = []
            for accumulate in (0, 1):
                gw, gb, gbp = base["gw"].clone(), base["gb"].clone(), base["gbp"].clone()
                gp, gvp = _Packed(N, H, bf, "cuda"), _Packed(N, H, bf, "cuda")
                L.check(lib.vbnn_head_backward(ctx.h, L.BF16, hs.ptr, hs.ld, w3.ptr, w3.ld, _p(g), N, H, C, accumulate, _p(gw), _p(gb), _p(gbp), 1,
                                               rs.ptr if with_r else None, rs.ld, 1, gp.ptr, gvp.ptr if with_r else None, gp.ld, None, None, 0))
                torch.cuda.synchronize()
                outs.append(dict(gw=gw, gb=gb, gbp=gbp, gp=gp.t[:, :H].float(), gvp=gvp.t[:, :H].float()))
            res[form] = outs
    finally:
        L.check(lib.vbnn_debug_set(10, -1))
    h64, r64, w64 = hs.t[:, :H].double(), rs.t[:, :H].double(), w3.t[:, :H].double()
    g64 = g.to(bf).double()
    gx = (g64 @ w64) * (h64 > 0)
    for form in (0, 1):
        for accumulate in (0, 1):
            o = res[form][accumulate]
            tag = f"form {form} accumulate {accumulate}"
            # bf16 outputs against float64: within one bf16 rounding of the exact value (2^-8 relative) plus the fp32 sum's own rounding
            assert float((o["gp"].double() - gx).abs().max()) <= 2.0 ** -8 * float(gx.abs().max()) + 1e-12, tag
            if with_r:
                # (gv_prev = bf16(g_prev before ITS rounding x r): half an ulp from each of the two roundings)
                assert float((o["gvp"].double() - o["gp"].double() * r64).abs().max()) <= 2.0 ** -7 * float((gx * r64).abs().max()) + 1e-12, tag
            want_w = g64.T @ h64 + (base["gw"].double() if accumulate else 0)
            want_bp = o["gp"].double().sum(0) + (base["gbp"].double() if accumulate else 0)          # of the ROUNDED g_prev this form stored
            want_b = g.double().sum(0) + (base["gb"].double() if accumulate else 0)
            assert float((o["gw"].double() - want_w).abs().max()) <= 2e-6 * float((g64.abs().T @ h64).max()) + 1e-6 * float(base["gw"].abs().max()) * accumulate + 1e-12, tag
            assert float((o["gbp"].double() - want_bp).abs().max()) <= 2e-6 * float(o["gp"].double().abs().sum(0).max()) + 1e-6 * float(base["gbp"].abs().max()) * accumulate + 1e-12, tag
            assert float((o["gb"].double() - want_b).abs().max()) <= 2e-6 * float(g.double().abs().sum(0).max()) + 1e-6 * float(base["gb"].abs().max()) * accumulate + 1e-12, tag
    # the two forms against each other: the bf16 outputs differ, if at all, by one bf16 ulp in a small fraction of places
    a, b = res[0][0], res[1][0]
    d = (a["gp"] - b["gp"]).abs()
    assert float(d.max()) <= 2.0 ** -7 * float(a["gp"].abs().max()) and float((d > 0).float().mean()) < 0.02, (float(d.max()), float((d > 0).float().mean()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_engine_alternates_sampled_and_map_passes_at_one_batch_size(oracle, nnmod, dtype):
    """the kept argument blocks bake in the LRT / MAP operand set, and their cache key did not say which.
    ONE engine, one batch size: a sampled training run, then clamp_to_map() + a forward-only run -- which must be the plain
    Linear on the means (no noise: two MAP runs are bitwise equal and equal the oracle's clamped pass) --, then a sampled
    run again, which must draw THIS draw's noise (the oracle's third draw) and back-propagate through it."""
    N, I0 = 37, 70
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    opt, eng, onet = _engine_pair(oracle, "lrt", dtype, [50, 34], I0, True, S=1)
    tol = 3e-5 if dtype == "f32" else 3e-2
    # 1. sampled, with backward
    eng.resetGradients(); eng.prepare(); eng.sample(); onet.resetGradients(); onet.sample()
    eng.run(dev(x), dev(t)); w1, _ = onet.run(x, t)
    l1, _ = eng.loss_and_accuracy()
    assert abs(l1 - w1) <= tol * abs(w1) + 1e-6, (l1, w1)
    # 2. MAP, forward only, same N (the reference's quicktest, mlp.lua:88-92)
    outs = []
    for _ in range(2):
        eng.resetGradients(); eng.clamp_to_map()
        eng.run(dev(x), dev(t), backward=False)
        lm, _ = eng.loss_and_accuracy()
        outs.append((lm, host(eng.out).copy()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32)), "a MAP pass drew noise"
    for om in onet.vb:
        om.clamp_to_map()
    wm, _ = onet.run(x, t)
    assert abs(outs[0][0] - wm) <= tol * abs(wm) + 1e-6, (outs[0][0], wm)
    assert abs(outs[0][0] - l1) > 1e-6 * abs(l1), "the MAP loss equals the sampled loss: the cached LRT block ran"
    # 3. sampled again: the second draw's noise, and a backward that uses this run's r
    eng.resetGradients(); eng.sample(); onet.resetGradients(); onet.sample()
    eng.run(dev(x), dev(t)); w3, _ = onet.run(x, t)
    l3, _ = eng.loss_and_accuracy()
    assert abs(l3 - w3) <= tol * abs(w3) + 1e-6, (l3, w3)
    assert abs(l3 - l1) > 1e-7 * abs(l1), "the second draw repeated the first draw's noise"
    if dtype == "f32":
        mle, mlc = onet.vb[0].compute_mugrads(opt)
        want = mle + mlc
        np.testing.assert_allclose(host(eng.vb[0].gradWeight), want, rtol=0, atol=3e-5 * np.abs(want).max() + 1e-10)
        vle, vlc = onet.vb[0].compute_vargrads(opt)
        want = vle + vlc
        np.testing.assert_allclose(host(eng.vb[0].gradSum), want, rtol=0, atol=3e-5 * np.abs(want).max() + 1e-10)


def test_engine_on_its_own_stream_orders_itself_behind_the_callers_stream(oracle, nnmod):
    """with stream= the library launches on the engine's stream while the caller's copies and torch's fills
    go to torch's current stream. The engine orders itself (FusedMLP._on_stream): constructed OUTSIDE any stream context,
    fed a minibatch that a slow copy chain on the caller's stream is still producing when run() is issued, it computes
    bitwise what an engine on the default stream computes."""
    from vbnn_amd.engine import FusedMLP
    N, I0 = 256, 784
    opt = opt_for("lrt", "bf16", input_size=I0, hidden=[512, 256], S=1, fuse_kl=True)
    x0 = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x0, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    ref = FusedMLP(opt)
    ref.resetGradients(); ref.prepare(); ref.sample(); ref.run(x0, t)
    want_loss, _ = ref.loss_and_accuracy()
    want = host(ref.grads).copy()
    s = torch.cuda.Stream()
    eng = FusedMLP(opt, stream=s)                          # NOT under torch.cuda.stream(s): allocation + init are the engine's job
    big = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    for rep in range(2):
        xin = torch.zeros_like(x0)
        for _ in range(8):                                  # ~2 GB of fills on the caller's stream, then the minibatch lands
            big.add_(1.0)
        xin.copy_(x0)
        eng.resetGradients()
        if rep == 0:
            eng.prepare()
        eng.sample(); eng.run(xin, t)                       # issued while the copy chain above is still in flight
        got_loss, _ = eng.loss_and_accuracy()
        if rep == 0:
            assert got_loss == want_loss, (got_loss, want_loss)
            assert np.array_equal(host(eng.grads).view(np.uint32), want.view(np.uint32))
    assert np.isfinite(host(eng.grads)).all()


def test_update_refuses_an_exchange_that_cannot_vouch_for_its_sums(oracle, nnmod):
    """FusedMLP.update() asks the exchange BEFORE a parameter is touched (check_exchange): a p2p barrier
    that gave up makes it raise, with means / lvars / Adam state as they were. (The exchange object here is a stand-in that
    reports a given-up barrier; the real give-up path is tests/test_dist_gpu.py's delayed-rank case.)"""
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", "f32", input_size=70, hidden=[50, 34], S=1, fuse_kl=True, **OPT_STATES)
    eng = FusedMLP(opt)
    x = torch.empty(37, 70, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(37, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t)
    before = [host(v.means).copy() for v in eng.vb] + [host(eng.weight3).copy()]

    class GaveUp:
        backend = "stand-in"

        def finish(self):
            pass

        def check(self):
            raise RuntimeError("vbnn_p2p: barrier 7 of rank 0 gave up waiting for a peer rank")
    eng._exchange = GaveUp()
    with pytest.raises(RuntimeError, match="gave up"):
        eng.update(opt)
    with pytest.raises(RuntimeError, match="gave up"):
        eng.loss_and_accuracy()
    after = [host(v.means) for v in eng.vb] + [host(eng.weight3)]
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "update() touched parameters before it checked the exchange"


def test_cu_budget_is_a_property_of_the_context_not_of_the_process(nnmod):
    """a budgeted context plans for its budget, a full-device context in the same process for the device --
    whatever order they were made or destroyed in."""
    import ctypes as C
    from vbnn_amd import _lib as L
    lib = L.lib()
    full = nnmod.Context.get()
    n = C.c_int()
    L.check(lib.vbnn_ctx_stream(full.h, None, C.byref(n)))
    total = n.value
    assert total >= 64
    a = nnmod.Context.with_cu_budget(0, total // 2)
    b = nnmod.Context.with_cu_budget(0, total // 2)
    assert a.cu_budget == total // 2
    L.check(lib.vbnn_ctx_stream(full.h, None, C.byref(n)))
    assert n.value == total, "a full-device context plans for the budget of another context"
    # 4096^3 fills 256 CUs with 256 two-pass tiles; on half the CUs the shape heuristic answers differently from the device's
    full_says = lib.vbnn_ctx_kmajor_supported(full.h, 4096, 4096, 4096)
    assert full_says == lib.vbnn_kmajor_supported(4096, 4096, 4096) == 1
    L.check(lib.vbnn_ctx_destroy(a.h))
    L.check(lib.vbnn_ctx_stream(b.h, None, C.byref(n)))
    assert n.value == total // 2, "destroying one budgeted context reset the survivor's plan"
    L.check(lib.vbnn_ctx_destroy(b.h))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_is_bitwise_reproducible_and_handles_tiny_batches(oracle, nnmod, dtype):
    """No float atomics feed a gradient: two engines with the same seed produce bit-identical gradient arenas.
    Batches of 1 and 5 rows (below every tile and vector width) run and, in fp32, match the oracle."""
    for N in (1, 5, 37):
        arenas = []
        for rep in range(2):
            opt, eng, onet = _engine_pair(oracle, "lrt", dtype, [50, 34], 70, True, S=2)
            loss, werr = _run_pair(opt, eng, onet, oracle, N, 70)
            arenas.append(host(eng.grads).copy())
            if dtype == "f32":
                assert abs(loss - werr) <= 3e-5 * abs(werr) + 1e-6, (N, loss, werr)
                mle, mlc = onet.vb[0].compute_mugrads(opt)
                want = mle + mlc
                np.testing.assert_allclose(host(eng.vb[0].gradWeight), want, rtol=0, atol=3e-5 * np.abs(want).max() + 1e-10)
        assert np.array_equal(arenas[0].view(np.uint32), arenas[1].view(np.uint32)), f"N={N}: gradients differ between runs"
        assert np.isfinite(arenas[0]).all()


def test_engine_two_stream_backward_is_identical(oracle, nnmod):
    """opt.overlap = True (accGradParameters on a second HIP stream) changes scheduling only: the gradient arena
    is bit-identical to the single-stream run, draw after draw."""
    from vbnn_amd.engine import FusedMLP
    x = oracle.fill_normal(64, 70, SEED, 4, 0, 0)
    t = (np.arange(64) * 7 % 10).astype(np.int32)
    arenas = []
    for overlap in (False, True):
        opt = opt_for("lrt", "bf16", input_size=70, hidden=[50, 34, 30], S=2, fuse_kl=True, overlap=overlap)
        eng = FusedMLP(opt)
        for step in range(3):
            eng.resetGradients(); eng.prepare()
            for _ in range(2):
                eng.sample(); eng.run(dev(x), dev(t))
            eng.finish()
        arenas.append(host(eng.grads).copy())
    assert np.array_equal(arenas[0].view(np.uint32), arenas[1].view(np.uint32))


def test_two_engines_on_two_streams_compute_what_each_computes_alone(nnmod):
    """The product's real concurrency, in one process: two FusedMLP engines on two HIP streams computing at the same time
    (their kernels share the CUs, the LDS and the texture path), one of them with the one-rank RCCL exchange running on the
    communicator's own high-priority stream beside its backward. Shape = the shard of the two-rank rehearsal (512 rows of
    784-4096-4096-10), whose GEMMs take the DUAL SCHED-0 instantiations of gemm_nt_v2 in which r02's late LDS-DMA piece
    lived (gemm_v2.h, v2_wait_barrier). Activations and gradient arenas must be BITWISE what each engine computes with the
    device to itself."""
    from vbnn_amd.engine import FusedMLP
    I0, N = 784, 512
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    engs = []
    for r, s in enumerate(streams):
        opt = opt_for("lrt", "bf16", input_size=I0, hidden=[4096, 4096], fuse_kl=True)
        e = FusedMLP(opt, stream=s, force_reduce=(r == 0))
        x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
        nnmod.fill_normal(x, SEED, 4, 0, 0, row0=r * N)
        t = ((torch.arange(N, device="cuda", dtype=torch.int64) + r * N) * 7 % 10).to(torch.int32)
        engs.append((e, x, t, s))
    torch.cuda.synchronize()

    def step(e, x, t, s):
        with torch.cuda.stream(s):
            e.draw = 0                                          # the same noise every time
            e.resetGradients(); e.sample(); e.run(x, t); e.finish()

    ref = []
    for e, x, t, s in engs:                                     # each engine alone on the device
        with torch.cuda.stream(s):
            e.prepare()
        step(e, x, t, s)
        torch.cuda.synchronize()
        step(e, x, t, s)                                        # (second step: every buffer reused)
        torch.cuda.synchronize()
        ref.append((e.h_s.t.clone(), e.vb[1].x_s.t.clone(), e.grads.clone()))
    assert engs[0][0].comm_backend() == "vbnn_comm/rccl"
    for rep in range(8):                                        # both at once: nothing between the two enqueues
        for k in range(3):
            for e, x, t, s in engs:
                step(e, x, t, s)
        torch.cuda.synchronize()
        for (e, _, _, _), (h, x1, g) in zip(engs, ref):
            assert torch.equal(e.vb[1].x_s.t, x1), f"round {rep}: layer-1 output differs under concurrency"
            assert torch.equal(e.h_s.t, h), f"round {rep}: layer-2 output differs under concurrency"
            assert torch.equal(e.grads, g), f"round {rep}: gradient arena differs under concurrency"
    # the two engines did compute different things (different rows), i.e. the comparison is not vacuous
    assert not torch.equal(ref[0][0], ref[1][0])


@pytest.mark.parametrize("N,S,stack", [(256, 1, False), (1, 30, True), (100, 3, False)], ids=["batch256", "batch1-S30-stacked", "batch100-S3"])
def test_captured_step_is_bitwise_the_launched_step(nnmod, N, S, stack):
    """BASELINE configs[1] (784-400-400-10, fp32) as ONE graph launch: the draw counter lives in device memory
    (vbnn_fwd_args.draw_dev, vbnn_sample), the step's launches are captured once (vbnn_capture_*) and replayed. Every replay
    must be bit for bit the same step issued launch by launch -- its own noise included (the counter advances inside the
    graph) -- for the batch-256 step, for the reference's own operating point (batch 1, S = 30, config.lua:11,32, draws
    stacked as rows) and for S sequential draws accumulating (main.lua:32-37)."""
    from vbnn_amd.engine import FusedMLP
    I0 = 784
    opt = opt_for("lrt", "f32", input_size=I0, hidden=[400, 400], S=S, fuse_kl=True, device_draw=True)
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    torch.cuda.synchronize()

    def make():
        s = torch.cuda.Stream()
        e = FusedMLP(opt, stream=s)

        def issue():
            e.resetGradients()
            if stack:
                e.run_draws(x, t, S)
            else:
                for _ in range(S):
                    e.sample(); e.run(x, t)
            e.finish()
        with torch.cuda.stream(s):
            e.prepare()
        return e, s, issue

    ea, sa, issue_a = make()
    want = []
    for step in range(4):                                       # launch by launch
        with torch.cuda.stream(sa):
            issue_a()
        loss, _ = ea.loss_and_accuracy()
        want.append((ea.grads.clone(), loss, ea.vb[0].r.clone()))
    assert not torch.equal(want[1][2], want[2][2])              # each step drew its own noise

    eb, sb, issue_b = make()
    with torch.cuda.stream(sb):
        issue_b()                                               # step 1 un-captured: allocations, first-launch configuration
    loss, _ = eb.loss_and_accuracy()
    assert torch.equal(eb.grads, want[0][0]) and loss == want[0][1]
    g = eb.capture_step(issue_b)
    # fp32: no packing launch, no finish launch -- sample, 2 forwards, 2 head kernels, gradInput, 2 accGradParameters (+ one
    # more sample for the stacked draws)
    # sample, two forwards, two head kernels, the layer-2 accGradParameters + updateGradInput PAIR launch, layer 1's
    # accGradParameters; stacked draws: + the packer (row n % rows_per_draw) and the closing sample(S - 1)
    # (r03 late: the head's forward + backward are one launch as well, vbnn_head_forward_backward)
    want_nodes = 8 if stack else 6 * S
    assert g.kernel_nodes == g.nodes == want_nodes, (g.kernel_nodes, g.nodes, want_nodes)
    print(f"captured step: {g.kernel_nodes} kernel nodes")
    for step in range(1, 4):                                    # steps 2..4 as graph replays
        g.launch()
        loss, _ = eb.loss_and_accuracy()
        assert torch.equal(eb.vb[0].r, want[step][2]), f"replay {step}: the noise differs"
        assert torch.equal(eb.grads, want[step][0]) and loss == want[step][1], f"replay {step}: gradients / loss differ"
    assert eb.draw == ea.draw
    g.close()


def test_cu_budget_stream_computes_the_same_gradients(nnmod):
    """opt.cu_budget: the engine on a CU-masked stream of the library's own (vbnn_ctx_create_cu_budget) -- the compute
    stream of a data-parallel rank, beside RCCL's channels. The mask changes where workgroups run and how many rounds a
    launch takes, never what they compute: the gradient arena is bitwise the unmasked engine's, for a budget that keeps
    the same kernels (the plan is per process: checked in a child process so that this one's stays unmasked)."""
    import subprocess, sys, os
    code = r"""
import sys, torch, numpy as np
sys.path.insert(0, %r)
from vbnn_amd.engine import FusedMLP
from vbnn_amd.nn import fill_normal
budget = int(sys.argv[1])
opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=256, hidden=[512, 256], n_classes=10, fuse_kl=True)
if budget: opt["cu_budget"] = budget
eng = FusedMLP(opt)
s = eng.ctx.torch_stream if budget else torch.cuda.current_stream()
with torch.cuda.stream(s):
    x = torch.empty(512, 256, dtype=torch.float32, device="cuda"); fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(512, device="cuda", dtype=torch.int64) * 7 %% 10).to(torch.int32)
    torch.cuda.synchronize()
    for _ in range(2):
        eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t); eng.finish()
    loss, _ = eng.loss_and_accuracy()
np.save(sys.argv[2], eng.grads.cpu().numpy())
print("budget", budget, "cus", getattr(eng.ctx, "cu_budget", None), "loss", repr(loss))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for budget in (0, 192):
            out = os.path.join(d, f"g{budget}.npy")
            res = subprocess.run([sys.executable, "-c", code, str(budget), out], capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
            print(res.stdout.strip())
            outs.append(np.load(out))
        assert "cus 192" in res.stdout
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("hidden,I0,N", [([400, 400], 784, 256), ([50, 34], 70, 37), ([64, 48, 40], 128, 100), ([256, 48, 40], 64, 33)])
def test_backward_pair_launch_is_bitwise_the_two_launches(nnmod, hidden, I0, N):
    """vbnn_backward_pair (accGradParameters + updateGradInput of a layer as ONE launch on the fp32 path) against the same engine
    with the two calls issued separately (opt.keep_transposes: the packed / transposed operand path of r02, separate launches):
    the K order of every accumulation chain is the same, so gradients and loss are bitwise equal -- ragged shapes included."""
    from vbnn_amd.engine import FusedMLP
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    res = []
    for keep in (False, True):
        # (head_step = False: the head as its two launches in both engines -- its one-launch form does not write the transposed
        # copies the r02 path wants, and sums gradWeight3 in another order)
        eng = FusedMLP(opt_for("lrt", "f32", input_size=I0, hidden=hidden, S=1, fuse_kl=True, keep_transposes=keep, head_step=False))
        for _ in range(2):
            eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t); eng.finish()
        loss, _ = eng.loss_and_accuracy()
        assert eng.f32_direct == (not keep)
        res.append((eng.grads.clone(), loss))
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][0], res[1][0])


@pytest.mark.parametrize("hidden,I0,N", [([400, 400], 784, 256), ([50, 34], 70, 37), ([64, 48, 40], 128, 100), ([256, 48, 40], 64, 33)])
def test_latency_kernel_agrees_with_the_general_kernel(nnmod, hidden, I0, N):
    """The fp32 step on the latency kernel (csrc/gemm_v0.h: 16-row tiles, K split over the workgroup's waves, fragments straight
    from global memory) against the same step on gemm_v1's LDS-staged 32 x 32 tile (vbnn_debug_set(VBNN_DEBUG_V0, 0)): the two
    differ in summation order only -- the same Philox draws, the same operands -- so loss and gradients agree to rounding. (Each
    is compared with the oracle by the parity tests of this file under the default, the latency kernel.)"""
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    res = []
    try:
        for v0 in (1, 0):
            L.check(L.lib().vbnn_debug_set(9, v0))
            eng = FusedMLP(opt_for("lrt", "f32", input_size=I0, hidden=hidden, S=1, fuse_kl=True))
            for _ in range(2):
                eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t); eng.finish()
            loss, _ = eng.loss_and_accuracy()
            res.append((eng.grads.clone(), loss))
    finally:
        L.check(L.lib().vbnn_debug_set(9, 1))
    assert abs(res[0][1] - res[1][1]) <= 2e-6 * abs(res[1][1])
    assert not torch.equal(res[0][0], res[1][0]), "the debug key selected nothing"
    scale = float(res[1][0].abs().max())
    assert float((res[0][0] - res[1][0]).abs().max()) <= 2e-5 * scale


@pytest.mark.parametrize("hidden,I0,N,S", [([400, 400], 784, 256, 1), ([50, 34], 70, 37, 2), ([64, 48, 40], 128, 100, 1), ([48, 130], 64, 16, 3)])
def test_head_as_one_launch_agrees_with_its_two_launches(nnmod, hidden, I0, N, S):
    """vbnn_head_forward_backward (mlp.lua:77-83 for the fused head in one call; fp32 at launch-bound sizes: ONE launch that
    recomputes the logits per workgroup) against vbnn_head_forward + vbnn_head_backward (opt.head_step = False): logits, output,
    d(loss)/d(logits) and the loss bit for bit (the same K split and MFMA order), the gradients to summation-order rounding --
    ragged shapes, S accumulated draws."""
    from vbnn_amd.engine import FusedMLP
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    res = []
    for one in (True, False):
        eng = FusedMLP(opt_for("lrt", "f32", input_size=I0, hidden=hidden, S=S, fuse_kl=True, head_step=one))
        eng.resetGradients(); eng.prepare()
        for _ in range(S):
            eng.sample(); eng.run(x, t)
        eng.finish()
        loss, acc = eng.loss_and_accuracy()
        res.append((eng.grads.clone(), loss, acc, eng.logits.clone(), eng.out.clone(), eng.g_logits.clone()))
    a, b = res
    assert a[1] == b[1] and a[2] == b[2]
    for k in (3, 4, 5):
        assert torch.equal(a[k], b[k])
    scale = float(b[0].abs().max())
    assert float((a[0] - b[0]).abs().max()) <= 2e-6 * scale


# ------------------------------------------------------------------------------------------- update
OPT_STATES = dict(state=dict(learningRate=1e-3), meanState=dict(learningRate=1e-4), varState=dict(learningRate=5e-2))


@pytest.mark.parametrize("mode", ["wn", "lrt"])
def test_module_update_matches_oracle(nnmod, oracle, mode):
    """mlp:update / VBLinear:update (mlp.lua:117-142, VBLinear.lua:124-166) after a two-draw minibatch, twice
    (Adam state carried across): parameters, Adam-visible ratios and the next step's loss."""
    from vbnn_amd import mlp
    opt = opt_for(mode, S=2, input_size=70, hidden=[50, 34], **OPT_STATES)
    net, onet = mlp.buildModel(opt), oracle.OracleMLP(opt)
    for k, i in enumerate(net.vb_indices):
        mod, om = net.model.get(i), onet.vb[k]
        om.means[:] = om.weight; mod.means.copy_(mod.weight)
        mod.compute_prior(); om.compute_prior()
    N = 37
    x = oracle.fill_normal(N, 70, SEED, 4, 0, 0)
    t = (np.arange(N) * 7 % 10).astype(np.int32)
    for it in range(2):
        net.resetGradients(); onet.resetGradients()
        for _ in range(2):
            net.sample(); onet.sample()
            err, _ = net.run(dev(x), dev(t))
            werr, _ = onet.run(x, t)
            assert abs(err - werr) <= 5e-5 * abs(werr) + 1e-6, (it, err, werr)
        ratios, wratios = net.update(opt), onet.update(opt)
        for k, i in enumerate(net.vb_indices):
            mod, om = net.model.get(i), onet.vb[k]
            # Adam's first steps move every weight by ~lr whatever the gradient scale, so compare absolutely
            np.testing.assert_allclose(host(mod.means), om.means, rtol=0, atol=2e-3 * 1e-4 + 1e-7 * np.abs(om.means).max())
            np.testing.assert_allclose(host(mod.lvars), om.lvars, rtol=0, atol=2e-3 * 5e-2)
            np.testing.assert_allclose(host(mod.bias), om.bias, rtol=0, atol=1e-8 + 1e-5 * np.abs(om.bias).max())
            for a, b in zip(ratios[k], wratios[k]):
                assert abs(a - b) <= 2e-3 * b
        last = net.model.get(2 * (len(opt["hidden"]) + 1))
        np.testing.assert_allclose(host(last.weight), onet.last.weight, rtol=0, atol=1e-7 * np.abs(onet.last.weight).max() + 1e-9)


@pytest.mark.parametrize("dtype,hidden,I0,N", [("f32", [50, 34], 70, 64), ("bf16", [512, 256], 256, 512)])
def test_engine_two_rank_shards_sum_to_the_single_process_step(oracle, nnmod, dtype, hidden, I0, N):
    """The data-parallel recipe on the REAL kernels, without a process group: two engines built as ranks 0 and 1 of a
    world of 2 (their all-reduce switched off) each take half the rows; the sum of their gradient arenas must equal
    the arena of one engine on the whole batch (criterion / global batch, KL gradient x 1/world, z by GLOBAL row),
    and their losses must add up. fp32: summation-order tolerance; bf16: the same plus the operand rounding of the
    per-half column sums."""
    import torch
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", dtype, input_size=I0, hidden=hidden, S=1, fuse_kl=True)
    x = dev(oracle.fill_normal(N, I0, SEED, 4, 0, 0))
    t = dev((np.arange(N) * 7 % 10).astype(np.int32))

    def one(world, rank, xs, ts):
        eng = FusedMLP(opt, world_size=world, rank=rank)
        eng.reduce = False                                    # the exchange itself is torch.distributed's job
        eng.resetGradients(); eng.prepare(); eng.sample()
        eng.run(xs, ts)
        loss, _ = eng.loss_and_accuracy()
        return eng.grads.clone(), loss

    g_full, loss_full = one(1, 0, x, t)
    g0, l0 = one(2, 0, x[: N // 2].contiguous(), t[: N // 2].contiguous())
    g1, l1 = one(2, 1, x[N // 2:].contiguous(), t[N // 2:].contiguous())
    assert abs((l0 + l1) - loss_full) <= 1e-5 * abs(loss_full)
    got, want = host(g0 + g1), host(g_full)
    tol = 2e-5 if dtype == "f32" else 2e-3
    assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want), np.linalg.norm(got - want) / np.linalg.norm(want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prepare_equals_per_layer_sweeps(nnmod, dtype):
    """vbnn_prepare (all layers + the final weight in one call, one finish kernel) must leave exactly what
    n x vbnn_prep_layer + vbnn_pack leave: bitwise equal shadows, transposes, statistics and packed final weight."""
    import ctypes as C
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP, _p
    opt = opt_for("lrt", dtype, input_size=70, hidden=[130, 64, 50], fuse_kl=True)
    eng = FusedMLP(opt)
    for v in eng.vb:                                       # non-trivial parameters
        v.lvars.uniform_(-9.0, -5.0)
    lib = L.lib()
    eng.prepare()                                          # the one-call form
    torch.cuda.synchronize()
    got = [(v.mu_s.t.clone(), v.var_s.t.clone(), v.muT_s.t.clone() if v.muT_s else None,
            v.varT_s.t.clone() if v.varT_s else None, v.stats.clone()) for v in eng.vb]
    got_w3, got_w3T = eng.w3_s.t.clone(), eng.w3T_s.t.clone()
    for v in eng.vb:
        for buf in (v.mu_s, v.var_s, v.muT_s, v.varT_s):
            if buf is not None:
                buf.t.zero_()
        v.stats.zero_()
        L.check(lib.vbnn_prep_layer(eng.ctx.h, eng.code, _p(v.means), _p(v.lvars), v.O, v.I, v.mu_s.ptr, v.var_s.ptr, v.mu_s.ld,
                                    v.muT_s.ptr if v.muT_s else None, v.varT_s.ptr if v.varT_s else None,
                                    v.muT_s.ld if v.muT_s else 0, _p(v.stats)))
    eng.w3_s.t.zero_(); eng.w3T_s.t.zero_()
    L.check(lib.vbnn_pack(eng.ctx.h, eng.code, L.PACK_COPY, _p(eng.weight3), None, eng.sizes[-1], eng.n_classes, eng.sizes[-1],
                          eng.w3_s.ptr, eng.w3_s.ld, eng.w3T_s.ptr, eng.w3T_s.ld))
    torch.cuda.synchronize()
    for v, (mu, var, muT, varT, st) in zip(eng.vb, got):
        assert torch.equal(mu, v.mu_s.t) and torch.equal(var, v.var_s.t)
        if muT is not None:
            assert torch.equal(muT, v.muT_s.t) and torch.equal(varT, v.varT_s.t)
        assert torch.equal(st, v.stats)
    assert torch.equal(got_w3, eng.w3_s.t) and torch.equal(got_w3T, eng.w3T_s.t)


def test_engine_update_matches_oracle(oracle, nnmod):
    """FusedMLP.update (total gradients straight from the dW epilogue) == the reference's update sequence."""
    opt, eng, onet = _engine_pair(oracle, "lrt", "f32", [50, 34], 70, True, S=1)
    opt.update(OPT_STATES)
    for it in range(2):
        loss, werr = _run_pair(opt, eng, onet, oracle, 37, 70)
        assert abs(loss - werr) <= 5e-5 * abs(werr) + 1e-6, (it, loss, werr)
        eng.update(opt); onet.update(opt)
        for k, v in enumerate(eng.vb):
            om = onet.vb[k]
            np.testing.assert_allclose(host(v.means), om.means, rtol=0, atol=2e-3 * 1e-4 + 1e-7 * np.abs(om.means).max())
            np.testing.assert_allclose(host(v.lvars), om.lvars, rtol=0, atol=2e-3 * 5e-2)
            np.testing.assert_allclose(host(v.bias), om.bias, rtol=0, atol=1e-8 + 1e-5 * np.abs(om.bias).max())
        np.testing.assert_allclose(host(eng.weight3), onet.last.weight, rtol=0, atol=1e-7 * np.abs(onet.last.weight).max() + 1e-9)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kl_gradient_added_in_the_update_is_the_fp32_form(oracle, nnmod, dtype):
    """opt.kl_in_update: the arena carries the likelihood parts only (vbnn_dw_args.kl_scale = 0) and vbnn_update adds the KL
    gradient from the fp32 means / lvars (vbnn_update_desc.kl_add) -- VBLinear.lua:91,96 exactly. (1) arena + the KL gradient
    formed here in float64 from the fp32 parameters = the total gradients of an engine whose epilogue added the fp32 KL terms
    (kl_from_shadows = False). (2) After TWO steps with updates (the second Adam step depends on the gradients' values, not
    just their signs) the parameters of the two engines agree to fp32 rounding; in bf16 the default shadow form --
    bf16(s2) / var_hat - 1 -- is measurably further away."""
    from vbnn_amd.engine import FusedMLP
    I0, N, hidden, B = 256, 512, [512, 256], 50.0
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    out = {}
    for name, extra in (("in_update", dict(kl_in_update=True)), ("fp32_epilogue", dict(kl_from_shadows=False)),
                        ("shadows", dict(kl_in_update=False))):       # (the A/B form: in-update is the bf16 default since r04)
        opt = opt_for("lrt", dtype, input_size=I0, hidden=hidden, S=1, fuse_kl=True, B=B, **OPT_STATES, **extra)   # small B: the KL part matters
        eng = FusedMLP(opt)
        for v in eng.vb:                                    # posterior variances away from the prior's: a KL gradient that is not ~0
            v.lvars.add_(0.7 * torch.sin(torch.arange(v.lvars.numel(), device="cuda", dtype=torch.float32)).view_as(v.lvars))
        eng.prepare()
        first = None
        for step in range(2):
            eng.resetGradients(); eng.sample(); eng.run(x, t); eng.finish()
            if step == 0:
                kl, kls = [], []
                for v in eng.vb:                            # VBLinear.lua:91,96 in float64 from the fp32 parameters ...
                    mu, lv = v.means.double(), v.lvars.double()
                    var_hat = float((lv.exp() + mu * mu).mean().item())
                    kl.append(((lv.exp() / var_hat - 1.0) / (2.0 * B), mu / (B * var_hat)))
                    # ... and as the shadow form has them: from the operand shadows (bf16 mu, bf16 exp(lvars))
                    ms, vs = v.mu_s.t[:, :v.I].double(), v.var_s.t[:, :v.I].double()
                    kls.append(((vs / var_hat - 1.0) / (2.0 * B), ms / (B * var_hat)))
                first = ([v.gradSum.double().clone() for v in eng.vb], [v.gradWeight.double().clone() for v in eng.vb], kl, kls)
            eng.update(opt)
        torch.cuda.synchronize()
        out[name] = (first, [v.lvars.clone() for v in eng.vb], [v.means.clone() for v in eng.vb])
    for k in range(2):
        # (1) the arena of the in-update engine IS the likelihood part: + the KL gradient = another engine's totals. fp32: + the
        # exact KL = the fp32-epilogue engine's. bf16: the likelihood factor of d/dlvars is the bf16 sigma^2 the forward multiplied
        # by (in both shadow engines; the fp32-epilogue engine uses exp(lvars) there), so the like-for-like check is
        # + the KL gradient as the shadow form has it = the shadow engine's totals.
        glv_lik, gmu_lik, kl, kls = (out["in_update"][0][j][k] for j in range(4))
        ref, klr = ("fp32_epilogue", kl) if dtype == "f32" else ("shadows", kls)
        glv_tot, gmu_tot = out[ref][0][0][k], out[ref][0][1][k]
        e_lv = float(((glv_lik + klr[0]) - glv_tot).abs().max() / glv_tot.abs().max())
        e_mu = float(((gmu_lik + klr[1]) - gmu_tot).abs().max() / gmu_tot.abs().max())
        assert e_lv <= 2e-6 and e_mu <= 2e-6, (k, ref, e_lv, e_mu)
        assert float(kl[0].abs().max()) > 1e-2 * float(glv_tot.abs().max())          # the KL part is not negligible here
        # what the shadow form loses: its KL gradient against the exact one (bf16: ~2^-9 absolute in the bracket)
        kl_err = float((kls[0] - kl[0]).abs().max() / kl[0].abs().max())
        # (2) parameters after two updates (the second Adam step depends on the gradients' values)
        a, b, c = out["in_update"][1][k], out["fp32_epilogue"][1][k], out["shadows"][1][k]
        d_exact, d_shadow = float((a - b).abs().max()), float((c - b).abs().max())
        m_exact = float((out["in_update"][2][k] - out["fp32_epilogue"][2][k]).abs().max())
        print(f"layer {k}: shadow-form KL gradient off by {kl_err:.2e} of its max; lvars after two updates: |in-update - fp32 epilogue| "
              f"{d_exact:.3e}, |shadows - fp32 epilogue| {d_shadow:.3e}; means {m_exact:.3e}")
        if dtype == "f32":
            assert d_exact <= 2e-5 and m_exact <= 2e-6, (k, d_exact, m_exact)
            assert kl_err <= 1e-6                              # (fp32 "shadows" are the parameters themselves)
        else:
            assert kl_err > 1e-4                               # the deviation ADVICE r02 described is real ...
            assert d_exact <= d_shadow + 1e-7, (k, d_exact, d_shadow)      # ... and the in-update form does not have it


def test_update_leaves_what_prepare_would_and_logs_the_14_series(oracle, nnmod):
    """vbnn_update = VBLinear:update + the next minibatch's parameter sweep in one pass. After two minibatches with
    updates (Adam state carried): (1) the operand shadows it wrote are BITWISE what vbnn_prepare writes from the updated
    parameters, the statistics agree to 1e-12; (2) the next step run WITHOUT prepare() gives bitwise the gradients of a
    step run after prepare(); (3) the 14 logged series (VBLinear.lua:149-164) match float64 NumPy on the oracle's
    update quantities."""
    for dtype, hidden, I0, N in (("f32", [50, 34], 70, 37), ("bf16", [512, 256], 256, 512)):
        opt, eng, onet = _engine_pair(oracle, "lrt", dtype, hidden, I0, True, S=1)
        opt.update(OPT_STATES)
        x = dev(oracle.fill_normal(N, I0, SEED, 4, 0, 0))
        t = dev((np.arange(N) * 7 % 10).astype(np.int32))
        eng.prepare()
        for it in range(2):
            eng.resetGradients(); eng.sample(); eng.run(x, t)
            before = [(host(v.means).astype(np.float64), host(v.lvars).astype(np.float64), host(v.gradWeight).astype(np.float64),
                       host(v.gradSum).astype(np.float64), float(host(v.stats)[2])) for v in eng.vb]
            eng.update(opt, log=True)
            torch.cuda.synchronize()
            B = opt["B"]
            for k, v in enumerate(eng.vb):                     # (3)
                mu0, lv0, gmu, glv, vh = before[k]
                mu1, lv1 = host(v.means).astype(np.float64), host(v.lvars).astype(np.float64)
                mlc, vlc = mu0 / (B * vh), (np.exp(lv0) / vh - 1.0) / (2 * B)
                # (the arena holds the totals -- or, with kl_in_update, the bf16 default, the likelihood parts themselves)
                mle, vle = (gmu, glv) if eng.kl_in_update else (gmu - mlc, glv - vlc)
                nl, nm = np.linalg.norm(lv1), np.linalg.norm(mu1)
                var1 = np.exp(lv1)
                want = [np.linalg.norm(vlc) / nl, np.linalg.norm(vle) / nl, np.linalg.norm(mlc) / nm, np.linalg.norm(mle) / nm,
                        var1.min(), var1.max(), var1.mean(), vh, mu1.mean(), mu1.std(ddof=1), mu1.min(), mu1.max(),
                        np.linalg.norm(mu1 - mu0) / nm, np.linalg.norm(lv1 - lv0) / nl]
                got = host(eng.update_log[k])
                np.testing.assert_allclose(got, want, rtol=2e-4, atol=1e-12, err_msg=f"{dtype} layer {k} step {it}")
        got = [(v.mu_s.t.clone(), v.var_s.t.clone(), v.muT_s.t.clone() if v.muT_s is not None else None,
                v.varT_s.t.clone() if v.varT_s is not None else None, v.stats.clone()) for v in eng.vb]
        got_w3 = eng.w3_s.t.clone()
        eng.resetGradients(); eng.sample(); eng.run(x, t)          # no prepare(): shadows + statistics from vbnn_update
        g_a = eng.grads.clone()
        eng.draw -= 1
        eng.prepare()
        torch.cuda.synchronize()
        for v, (mu, var, muT, varT, st) in zip(eng.vb, got):       # (1)
            assert torch.equal(mu, v.mu_s.t) and torch.equal(var, v.var_s.t)
            if muT is not None and getattr(v, "use_muT", True):
                assert torch.equal(muT, v.muT_s.t) and torch.equal(varT, v.varT_s.t)
            np.testing.assert_allclose(host(st), host(v.stats), rtol=1e-12, atol=0)
        assert torch.equal(got_w3, eng.w3_s.t)
        eng.resetGradients(); eng.sample(); eng.run(x, t)
        rel = float((eng.grads - g_a).norm() / g_a.norm())         # (2): bitwise unless the statistics moved in their last bit
        assert rel <= 1e-7, rel


def test_rccl_exchange_through_the_c_abi_one_rank(nnmod):
    """vbnn_comm_* (RCCL bound with dlopen behind the C ABI) with a world of one -- all a one-GPU box can host: the
    communicator comes up, an in-place SUM all-reduce of an arena-sized bucket leaves it unchanged, it is ordered after
    the compute stream's producer and finish() orders the consumer after it, and the gather proves the rank count."""
    from vbnn_amd.comm import RcclExchange
    ctx = nnmod.Context.get()
    ex = RcclExchange(ctx, 0, 1)
    assert ex.backend == "vbnn_comm/rccl"
    buf = torch.empty(6_000_000, dtype=torch.float32, device="cuda")
    for rep in range(3):
        buf.normal_()                                             # producer on the compute stream
        want = buf.clone()
        ex.allreduce(buf)
        ex.finish()
        got = buf * 1.0                                            # consumer on the compute stream
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert ex.gather_u64(0x1234567890ABCDEF) == [0x1234567890ABCDEF]
    ex.close()


def test_p2p_exchange_with_one_rank_and_engine_arena(nnmod):
    """vbnn_p2p_* with a world of one (all an in-process test can host; tests/test_dist_gpu.py runs 2 and 3 ranks): the arena is
    the exchange's own allocation wrapped as a tensor without a copy, an all-reduce leaves it unchanged and is ordered between
    producer and consumer on the compute stream, and an engine with opt.exchange = "p2p" keeps its gradients in that arena and
    computes bitwise what the plain engine computes."""
    from vbnn_amd.comm import P2PExchange
    from vbnn_amd.engine import FusedMLP
    ctx = nnmod.Context.get()
    ex = P2PExchange(ctx, 0, 1, 1_000_003)
    assert ex.backend == "vbnn_p2p/ipc" and ex.arena.numel() == 1_000_003 and float(ex.arena.abs().sum()) == 0.0
    for rep in range(2):
        ex.arena.normal_()
        want = ex.arena.clone()
        ex.allreduce(ex.arena[5:900_000])
        ex.finish()
        got = ex.arena * 1.0
        torch.cuda.synchronize()
        assert torch.equal(got, want) and ex.gave_up() == 0
    ex.close()
    x = torch.empty(64, 70, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = (torch.arange(64, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    arenas = []
    for kind in ("", "p2p"):
        eng = FusedMLP(opt_for("lrt", "bf16", input_size=70, hidden=[50, 34], fuse_kl=True, exchange=kind), force_reduce=bool(kind))
        for _ in range(2):
            eng.resetGradients(); eng.prepare(); eng.sample(); eng.run(x, t); eng.finish()
        torch.cuda.synchronize()
        if kind:
            assert eng.comm_backend() == "vbnn_p2p/ipc" and eng.exchange().gave_up() == 0
        arenas.append(eng.grads.clone())
    assert torch.equal(arenas[0], arenas[1])


@pytest.mark.parametrize("hidden,I0,N", [([50, 34], 70, 64), ([512, 256], 256, 512)])
def test_bf16_exchange_option_with_one_rank(nnmod, hidden, I0, N):
    """opt.exchange_dtype = "bf16" (the optional half-size exchange) through RCCL with a world of one: every bucket is
    rounded to bf16 (RNE), all-reduced in place on the staging arena, and widened back behind the exchange -- so the arena
    must hold EXACTLY bf16(gradients of the same step without the option); the default engine's gradients are untouched
    by the option's existence. Odd bucket offsets (the 50-34 net) take the cast kernel's scalar path."""
    from vbnn_amd.engine import FusedMLP
    from vbnn_amd.nn import fill_normal
    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=3, input_size=I0, hidden=hidden,
               n_classes=10, fuse_kl=True)
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    fill_normal(x, 3, 4, 0, 0)
    t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % 10).to(torch.int32)
    grads = {}
    for name, extra in (("plain", {}), ("f32", dict(force=True)), ("bf16", dict(force=True, exchange_dtype="bf16"))):
        eng = FusedMLP(dict(opt, **{k: v for k, v in extra.items() if k != "force"}), force_reduce=extra.get("force", False))
        for _ in range(2):
            eng.resetGradients(); eng.prepare(); eng.sample()
            eng.run(x, t)
            eng.finish()
        torch.cuda.synchronize()
        if extra.get("force"):
            assert eng.comm_backend() == "vbnn_comm/rccl", eng.comm_backend()
        grads[name] = eng.grads.clone()
    assert torch.equal(grads["plain"], grads["f32"])
    assert torch.equal(grads["bf16"], grads["plain"].to(torch.bfloat16).float())
    assert not torch.equal(grads["bf16"], grads["plain"])


# ------------------------------------------------------------------------------------------- MSE head (BASELINE configs[4])
@pytest.mark.parametrize("N,D", [(1, 1), (37, 70), (64, 256)])
def test_mse_criterion_matches_oracle(nnmod, oracle, N, D):
    """vbnn_mse_forward / _backward == nn.MSECriterion restated (oracle vbo_mse_*): loss 1e-6, gradient 1e-6 relative;
    the loss accumulates over draws and is bitwise reproducible."""
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import _p
    rng = np.random.default_rng(N * 100 + D)
    y = rng.normal(0, 1, (N, D)).astype(np.float32)
    t = rng.normal(0, 1, (N, D)).astype(np.float32)
    ctx = nnmod.Context.get()
    yd, td = dev(y), dev(t)
    g = torch.zeros(N, D, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    inv = 1.0 / (N * D)
    L.check(L.lib().vbnn_mse_forward(ctx.h, _p(yd), D, _p(td), D, N, D, inv, _p(g), D, 0, _p(loss)))
    l1 = float(host(loss)[0])
    want = oracle.mse_forward(y, t)
    assert abs(l1 - want) <= 1e-6 * abs(want) + 1e-12
    np.testing.assert_allclose(host(g), oracle.mse_backward(y, t), rtol=1e-6, atol=1e-9)
    L.check(L.lib().vbnn_mse_forward(ctx.h, _p(yd), D, _p(td), D, N, D, inv, None, 0, 1, _p(loss)))
    assert abs(float(host(loss)[0]) - 2 * l1) <= 1e-12 * abs(l1)
    g2 = torch.zeros_like(g)
    L.check(L.lib().vbnn_mse_backward(ctx.h, _p(yd), D, _p(td), D, N, D, inv, _p(g2), D))
    assert torch.equal(g, g2)


@pytest.mark.parametrize("mode", ["lrt", "wn"])
def test_engine_regression_head_matches_oracle_f32(oracle, nnmod, mode):
    """The fused engine with the regression head (final Linear to D outputs + MSE, the criterion of BASELINE configs[4])
    against the module-by-module oracle with the same criterion: fp32, ragged shapes, two draws."""
    from vbnn_amd.engine import FusedMLP
    hidden, I0, N, D = [50, 34], 70, 37, 24
    opt = opt_for(mode, "f32", input_size=I0, hidden=hidden, S=2, fuse_kl=True, n_classes=D, criterion="mse")
    eng, onet = FusedMLP(opt), oracle.OracleMLP(opt)
    rng = np.random.default_rng(9)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        lv = rng.normal(np.log(1e-3), 0.3, om.lvars.shape).astype(np.float32)
        om.means[:] = om.weight; om.lvars[:] = lv
        v.lvars.copy_(dev(lv))
        om.compute_prior()
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    t = rng.normal(0, 1, (N, D)).astype(np.float32)
    eng.resetGradients(); eng.prepare(); onet.resetGradients()
    werr = 0.0
    for _ in range(2):
        eng.sample(); onet.sample()
        eng.run(dev(x), dev(t))
        werr += onet.run(x, t)[0]
    loss, _ = eng.loss_and_accuracy()
    assert abs(loss - werr) <= 3e-5 * abs(werr) + 1e-6, (loss, werr)
    for k, v in enumerate(eng.vb):
        om = onet.vb[k]
        mle, mlc = om.compute_mugrads(opt)
        vle, vlc = om.compute_vargrads(opt)
        np.testing.assert_allclose(host(v.gradWeight), mle + mlc, rtol=0, atol=3e-5 * np.abs(mle + mlc).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradSum), vle + vlc, rtol=0, atol=2e-4 * np.abs(vle + vlc).max() + 1e-10)
        np.testing.assert_allclose(host(v.gradBias), om.gradBias, rtol=0, atol=3e-5 * np.abs(om.gradBias).max() + 1e-10)
    np.testing.assert_allclose(host(eng.gradWeight3), onet.last.gradWeight, rtol=0, atol=3e-5 * np.abs(onet.last.gradWeight).max() + 1e-10)
    np.testing.assert_allclose(host(eng.gradBias3), onet.last.gradBias, rtol=0, atol=3e-5 * np.abs(onet.last.gradBias).max() + 1e-9)


def test_engine_regression_head_bf16_against_rounding_emulation(oracle, nnmod):
    """configs[4]'s head in bf16 (final Linear 256 -> 256 on the GEMM kernels, MSE) against the float64 emulation."""
    from oracle.ref_numpy import bf16_round, emulate_lrt_step
    from vbnn_amd.engine import FusedMLP
    hidden, I0, N, D = [512, 256], 256, 512, 256
    opt = opt_for("lrt", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True, n_classes=D, criterion="mse")
    eng, onet = FusedMLP(opt), oracle.OracleMLP(opt)
    for k, v in enumerate(eng.vb):
        onet.vb[k].means[:] = onet.vb[k].weight
    x = oracle.fill_normal(N, I0, SEED, 4, 0, 0)
    xt = dev(x)
    t = eng.synthetic_targets(xt)
    eng.resetGradients(); eng.prepare(); eng.sample()
    eng.run(xt, t)
    loss, _ = eng.loss_and_accuracy()
    layers = [dict(means=om.means, lvars=om.lvars, bias=om.bias) for om in onet.vb]
    zetas = [oracle.fill_normal(N, om.O, SEED, 2, k, 1, 0).astype(np.float64) for k, om in enumerate(onet.vb)]
    wloss, res, gw3, gb3 = emulate_lrt_step(layers, onet.last.weight, onet.last.bias, x, host(t), zetas, bf16_round, S=1.0, B=opt["B"],
                                            kl_shadows=eng.kl_from_shadows, criterion="mse", kl_scale=0.0 if eng.kl_in_update else 1.0)
    assert abs(loss - wloss) <= 1e-4 * abs(wloss), (loss, wloss)
    for k, v in enumerate(eng.vb):
        for got, want, what in ((v.gradWeight, res[k]["grad_mu"], "d/dmeans"), (v.gradSum, res[k]["grad_lv"], "d/dlvars"), (v.gradBias, res[k]["gradBias"], "gradBias")):
            fro = np.linalg.norm(host(got) - want) / np.linalg.norm(want)
            assert fro <= 2e-3, f"layer {k} {what}: {fro:.3e}"
    assert np.linalg.norm(host(eng.gradWeight3) - gw3) <= 2e-3 * np.linalg.norm(gw3)
    assert np.linalg.norm(host(eng.gradBias3) - gb3) <= 2e-3 * np.linalg.norm(gb3)


@pytest.mark.parametrize("dtype,hidden,I0,N", [("f32", [50, 34], 70, 37), ("bf16", [512, 256], 256, 512), ("bf16", [4096, 4096], 784, 4096)])
def test_early_dlvars_message_is_bitwise_the_fused_launch(oracle, nnmod, dtype, hidden, I0, N):
    """The data-parallel overlap lever: accGradParameters as TWO launches (vbnn_dw_args.part = 2, then 1),
    so that the exchange of the finished d/dlvars starts while the d/dmeans GEMM still runs. Every output depends on one
    accumulator of the pair, so the gradients must equal the single launch's BIT FOR BIT (general kernel, pipelined kernel
    and the two-pass kernel at the bench's size); with a world of one the RCCL exchange runs between the launches."""
    from vbnn_amd.engine import FusedMLP
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    arenas = []
    for early, reduce in ((False, False), (True, False), (True, True)):
        # (head_step = False: the fp32 head as its two launches in all three -- its one-launch form, taken only without transposed
        # copies, sums the head's gradients in another order)
        opt = opt_for("lrt", dtype, input_size=I0, hidden=hidden, S=1, fuse_kl=True, early_lv=early, head_step=False)
        eng = FusedMLP(opt, force_reduce=reduce)
        assert eng.early_lv == [early] * len(hidden)
        t = eng.synthetic_targets(x)
        eng.prepare(); eng.resetGradients(); eng.sample()
        eng.run(x, t)
        eng.finish()
        loss, _ = eng.loss_and_accuracy()
        if reduce:
            assert eng.comm_backend() == "vbnn_comm/rccl" and len(eng.buckets()) == len(hidden) + sum(eng._early(v) for v in eng.vb)
            assert eng._early(eng.vb[-1])
        arenas.append((eng.grads.clone(), loss))
        del eng
    for g, l in arenas[1:]:
        assert torch.equal(g, arenas[0][0]) and l == arenas[0][1]


@pytest.mark.parametrize("dtype,hidden,I0,N,S", [("f32", [50, 34], 70, 1, 30), ("f32", [400, 400], 784, 100, 5), ("bf16", [512, 256], 256, 128, 4)])
def test_stacked_draws_equal_sequential_draws(oracle, nnmod, dtype, hidden, I0, N, S):
    """FusedMLP.run_draws -- the S Monte-Carlo draws of a minibatch (main.lua:32-37) as rows of ONE pass, noise addressed by
    (draw, minibatch row) -- against S sequential sample() / run() calls with in-place accumulation: the noise-dependent
    residual r of every draw BITWISE (same z, same GEMM chain per output), loss and gradients to fp32 summation order.
    The first case is the reference's own operating point: batchSize 1, S = 30 (config.lua:11,32)."""
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", dtype, input_size=I0, hidden=hidden, S=S, fuse_kl=True)
    x = dev(oracle.fill_normal(N, I0, SEED, 4, 0, 0))
    t = dev((np.arange(N) * 7 % 10).astype(np.int32))
    seq, stk = FusedMLP(opt), FusedMLP(opt)
    seq.prepare(); seq.resetGradients()
    rs = []
    for _ in range(S):
        seq.sample(); seq.run(x, t)
        rs.append([v.r[:N].clone() for v in seq.vb])
    loss_a, corr_a = seq.loss_and_accuracy()
    stk.prepare(); stk.resetGradients()
    stk.run_draws(x, t, S)
    loss_b, corr_b = stk.loss_and_accuracy()
    assert stk.draw == seq.draw == S
    for s_ in range(S):
        for k, v in enumerate(stk.vb):
            assert torch.equal(v.r[s_ * N:(s_ + 1) * N], rs[s_][k]), (s_, k)
    assert abs(loss_a - loss_b) <= 2e-6 * abs(loss_a) and corr_a == corr_b
    tol = 2e-5 if dtype == "f32" else 2e-3
    rel = float((stk.grads - seq.grads).norm() / seq.grads.norm())
    assert rel <= tol, rel


@pytest.mark.parametrize("hidden,I0,N", [([4096, 4096], 784, 1024), ([4096, 4096], 784, 4096), ([512, 256], 256, 512)])
def test_staged_stores_stay_inside_their_tensors(oracle, nnmod, hidden, I0, N):
    """Guard-band screen of the kernels that address their outputs by hand (the fold's staged stores of r and d/dlvars, the
    split launch's slabs and ragged epilogue): every output tensor of a step is re-pointed into the middle of a larger
    sentinel-filled allocation; after two steps the sentinels on both sides must be untouched."""
    from vbnn_amd.engine import FusedMLP
    opt = opt_for("lrt", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True)
    eng = FusedMLP(opt)
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = eng.synthetic_targets(x)
    eng.prepare(); eng.resetGradients(); eng.sample(); eng.run(x, t)          # allocates the batch buffers
    GUARD = 1 << 16
    guards = []

    def guarded(tensor, sentinel):
        flat = tensor.reshape(-1)
        big = torch.full((flat.numel() + 2 * GUARD,), sentinel, dtype=tensor.dtype, device="cuda")
        big[GUARD:GUARD + flat.numel()] = flat
        guards.append((big, flat.numel(), sentinel))
        return big[GUARD:GUARD + flat.numel()].view(tensor.shape)

    # the gradient arena (d/dlvars, d/dmeans, bias gradients are views into it) and every layer's r
    arena = guarded(eng.grads, 12345.0)
    eng.grads = arena
    lay = eng._lay
    for li, v in enumerate(eng.vb):
        v.gradSum = arena[lay[li]["lv"][0]:lay[li]["lv"][0] + lay[li]["lv"][1]].view(v.O, v.I)
        v.gradWeight = arena[lay[li]["mu"][0]:lay[li]["mu"][0] + lay[li]["mu"][1]].view(v.O, v.I)
        v.gradBias = arena[lay[li]["bias"][0]:lay[li]["bias"][0] + lay[li]["bias"][1]]
        v.r = guarded(v.r, 77.0)
    off = lay[-1]["bucket"][1]
    H, Cn = eng.sizes[-1], eng.n_classes
    eng.gradWeight3 = arena[off:off + Cn * H].view(Cn, H)
    eng.gradBias3 = arena[off + Cn * H:off + Cn * H + Cn]
    eng._acc = guarded(eng._acc, 3.0e300)
    eng._argcache.clear()                     # the engine keeps its argument blocks: rebuild them around the guarded tensors
    for _ in range(2):
        eng.resetGradients(); eng.sample(); eng.run(x, t)
    loss, _ = eng.loss_and_accuracy()
    torch.cuda.synchronize()
    assert np.isfinite(loss) and 0.0 < loss < 1e3
    for big, n, sentinel in guards:
        lo, hi = big[:GUARD], big[GUARD + n:]
        assert bool((lo == sentinel).all()) and bool((hi == sentinel).all()), "a kernel wrote outside its output tensor"


# ------------------------------------------------------------------------------------------- errors
def test_box_calibration_reports_a_plausible_box(nnmod):
    """vbnn_box_calibrate (bench.py's `box` block): the register-only MFMA probe holds a clock between 1.2 and 2.6 GHz and reaches
    at least 85 % of what 2.5 PFLOP/s scales to at that clock (1024 SIMDs x 1024 flop per cycle); the stream copy moves its 1 GiB at
    2 ... 8 TB/s; two calls agree to 5 %."""
    import ctypes as C
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    ctx = Context.get(torch.device("cuda", 0))
    got = []
    for _ in range(2):
        info = L.BoxInfo()
        L.check(L.lib().vbnn_box_calibrate(ctx.h, C.byref(info)))
        assert info.cus >= 64 and info.hbm_bytes == 1 << 30
        assert 1.2 <= info.mfma_clock_ghz <= 2.6, info.mfma_clock_ghz
        ceiling = info.cus * 4 * 1024 * info.mfma_clock_ghz * 1e9 / 1e12
        assert 0.85 * ceiling <= info.mfma_tflops <= 1.02 * ceiling, (info.mfma_tflops, ceiling)
        assert 2.0 <= info.hbm_TBps <= 8.0, info.hbm_TBps
        got.append((info.mfma_clock_ghz, info.mfma_tflops, info.hbm_TBps))
    for a, b in zip(*got):
        assert abs(a - b) <= 0.05 * max(a, b), got


def test_p2p_stand_in_runs_what_a_rank_of_eight_runs_and_switches_off(nnmod):
    """vbnn_p2p_standin (LAB, one rank): with the stand-in on, an all-reduce launches the barrier / reduce-scatter / barrier /
    all-gather chain of an 8-rank exchange against this arena -- its values are garbage afterwards by design, its status word
    stays clear, the compute stream is ordered behind it by finish() -- and with it off the world-of-one exchange leaves the
    arena alone again; paced and unpaced, default and tiny grids; a region that is shorter than the world."""
    from vbnn_amd.comm import P2PExchange
    from vbnn_amd.nn import Context
    ctx = Context.get(torch.device("cuda", 0))
    n = 1_000_003
    ex = P2PExchange(ctx, 0, 1, n)
    try:
        ref = torch.randn(n, device="cuda")
        for gbps, grid in ((0.0, (0, 0)), (770.0, (0, 0)), (0.0, (2, 1))):
            ex.arena.copy_(ref)
            ex.set_grid(*grid)
            ex.standin(8, gbps)
            for off, cnt in ((0, 500_000), (500_000, 500_003), (16, 5)):
                ex.allreduce(ex.arena[off:off + cnt])
            ex.finish()
            torch.cuda.synchronize()
            assert ex.gave_up() == 0
            assert not torch.equal(ex.arena, ref), "the stand-in's kernels did not run"
            # the EIGHT-way reduce-scatter's arithmetic, bitwise (a world above four takes a second batch of peer loads; the box's
            # process limit keeps the multi-process tests at four ranks): the stand-in's peers are this arena's own chunks, so its
            # chunk 0 must hold ((((c0 + c1) + c2) + ...) + c7) of the ORIGINAL chunks in rank order -- and chunk 1, gathered from
            # "peer 0", that same sum
            ex.arena.copy_(ref)
            ex.standin(8, gbps)
            ex.allreduce(ex.arena[:800_000]); ex.finish()
            torch.cuda.synchronize()
            cs = 100_000
            want = ref[:cs].clone()
            for q in range(1, 8):
                want += ref[q * cs:(q + 1) * cs]
            assert torch.equal(ex.arena[:cs].view(torch.int32), want.view(torch.int32)), "the 8-way reduce-scatter's sum is not the rank-ordered fp32 sum"
            assert torch.equal(ex.arena[cs:2 * cs].view(torch.int32), want.view(torch.int32)), "the all-gather did not deliver the reduced chunk"
            ex.standin(0)
            ex.arena.copy_(ref)
            ex.allreduce(ex.arena[:n]); ex.finish()
            torch.cuda.synchronize()
            assert torch.equal(ex.arena, ref)
    finally:
        ex.close()


def test_error_convention(nnmod):
    """Non-zero status + message instead of a crash (SURVEY 8b error convention)."""
    from vbnn_amd import _lib as L
    m = nnmod.Linear(8, 4)
    with pytest.raises(ValueError):
        m.updateOutput(torch.zeros(8, device="cuda"))          # 1-D input: the reference fails too (VBLinear.lua:114)
    ctx = nnmod.Context.get()
    st = L.lib().vbnn_pack(ctx.h, 7, 0, None, None, 0, 0, 0, None, 0, None, 0)
    assert st != 0 and len(L.lib().vbnn_last_error()) > 0


# --------------------------------------------------------------------- the benchmark configurations, whole step
@pytest.mark.parametrize("hidden,I0,crit", [([4096, 4096], 784, "nll"), ([4096] * 8, 4096, "nll"), ([4096] * 8, 4096, "mse")],
                         ids=["wide", "deep", "deep-mse"])
def test_full_size_step_properties(oracle, nnmod, hidden, I0, crit):
    """BASELINE.json's measured configurations (batch 4096, bf16, LRT, S = 1) are beyond what the oracle finishes in
    seconds, so the WHOLE fused step is held to size-independent properties instead:
      1. two fresh engines produce bit-identical gradient arenas (no atomics, no arrival-order sums);
      2. the launch with K-major operands (gemm_v3 AK/BK, gemm_v2 pair split KM) and the launch with the transposed
         copies (debug key 6 = 0) are different kernels over different buffers: their gradients must agree to bf16
         operand rounding of the bias column sums, far below any layout or indexing error;
      3. two half-batch ranks of a world of 2 sum to the single-process gradients and loss (wide only: memory);
      4. softmax-gradient identities: the final Linear's bias gradient sums to zero over classes; every gradient finite.
    "deep-mse" is BASELINE configs[4] exactly as bench.py --config deep runs it: 8 x 4096 + Linear 4096 -> 4096 + nn.MSECriterion
    on the synthetic regression target. Its form of 4: the criterion's two outputs bind each other (loss = sum g^2 / (4 inv_nd)
    with g = 2 inv_nd (y - t)) and the final Linear's bias gradient is the column sum of g."""
    import torch
    from vbnn_amd import _lib as L
    from vbnn_amd.engine import FusedMLP
    N = 4096
    mse = crit == "mse"
    opt = opt_for("lrt", "bf16", input_size=I0, hidden=hidden, S=1, fuse_kl=True, criterion=crit, n_classes=4096 if mse else 10)
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nnmod.fill_normal(x, SEED, 4, 0, 0)
    t = ((torch.arange(N, device="cuda", dtype=torch.int64) * 2654435761) % 10).to(torch.int32)
    if mse:
        probe = FusedMLP(opt)
        t = probe.synthetic_targets(x)                              # y* = x R / sqrt(I): bench.py's regression target
        del probe
    checks = {}

    def one(world=1, rank=0, xs=x, ts=t, **over):
        eng = FusedMLP(dict(opt, **over), world_size=world, rank=rank)
        eng.reduce = False
        eng.resetGradients(); eng.prepare(); eng.sample()
        eng.run(xs, ts)
        loss, correct = eng.loss_and_accuracy()
        g = eng.grads.clone()
        gb3 = eng.gradBias3.clone()
        if mse and not checks:
            gl = eng.g_logits.double()
            checks["loss_from_g"] = float((gl * gl).sum().item()) * (xs.shape[0] * world * 4096) / 4.0
            checks["gb3_from_g"] = gl.sum(dim=0)
        del eng
        return g, loss, gb3

    g_a, loss_a, gb3 = one()
    g_b, loss_b, _ = one()
    assert torch.equal(g_a, g_b) and loss_a == loss_b                                   # 1
    assert bool(torch.isfinite(g_a).all()) and np.isfinite(loss_a)
    if mse:
        assert loss_a > 0.1                                                             # untrained regression: O(1) squared error
        assert abs(checks["loss_from_g"] - loss_a) <= 1e-5 * loss_a, (checks["loss_from_g"], loss_a)   # 4 (criterion identities)
        err = float((gb3.double() - checks["gb3_from_g"]).abs().max())
        assert err <= 1e-5 * float(checks["gb3_from_g"].abs().max()) + 1e-9, err
    else:
        assert loss_a > 1.0                                                             # untrained: worse than chance's log 10
        assert abs(float(gb3.sum())) <= 1e-5 * float(gb3.abs().sum() + 1e-12)           # 4
    L.check(L.lib().vbnn_debug_set(6, 0))
    try:
        g_t, loss_t, _ = one()
    finally:
        L.check(L.lib().vbnn_debug_set(6, 1))
    assert abs(loss_t - loss_a) <= 1e-6 * abs(loss_a)
    rel = float((g_t - g_a).norm() / g_a.norm())
    assert rel <= 2e-3, rel                                                             # 2
    del g_t, g_b
    if len(hidden) == 2:
        g0, l0, _ = one(2, 0, x[: N // 2].contiguous(), t[: N // 2].contiguous())
        g1, l1, _ = one(2, 1, x[N // 2:].contiguous(), t[N // 2:].contiguous())
        assert abs((l0 + l1) - loss_a) <= 1e-5 * abs(loss_a)
        rel = float((g0 + g1 - g_a).norm() / g_a.norm())
        assert rel <= 2e-3, rel                                                         # 3
