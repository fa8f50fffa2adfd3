"""The step matrix: every backward schedule of FusedMLP.run, the stacked draws of run_draws and capture_step, for every head
kind -- the fused 10-class head (the control) and the generic head's four criteria (20-class `nll`, `mse`, `gauss`, `bce`).

  (a) anchor: the baseline schedule of every head on the small tiers against the float64 step (tests/_step_np.py);
  (b) schedules: gradient arena, loss and hit count of every other schedule BITWISE the baseline's -- the engine's own claims
      (the comments in FusedMLP.run) -- or, where a schedule takes other kernels by design, held to the float64 step;
  (c) stacked draws against sequential draws and against the float64 step;
  (d) a captured step against the same steps issued launch by launch, the targets changing between replays;
  (e) a step allocates nothing.
Tolerances are the engine-level ones of tests/test_parity_gpu.py (test_engine_regression_head_matches_oracle_f32: loss 3e-5
relative + 1e-6, regions 3e-5 of their largest value, d/dlvars 2e-4; ..._bf16_against_rounding_emulation: loss 1e-4 relative,
regions 2e-3 relative Frobenius; test_stacked_draws_equal_sequential_draws: loss 2e-6, arena 2e-5 relative Frobenius;
test_full_size_step_properties: K-major against transposed operands 2e-3, loss 1e-6). Every comparison prints the share of its
tolerance in use (profiles/step_matrix_bounds.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _step_np as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HEADS = list(R.HEADS)
GENERIC = [h for h in HEADS if h != "nll10"]
BASELINE = dict(dx_first=False, chain_backward=False)
# name: (engine options over the baseline's, force_reduce)
BITWISE_BF16 = {
    "dx_first": (dict(dx_first=True), False),
    "chain-dx": (dict(chain_backward="dx"), False),
    "chain-dw": (dict(chain_backward="dw"), False),
    "overlap": (dict(overlap=True), False),
    "exchange": (dict(early_lv=False), True),
    "exchange-early-lv": (dict(early_lv=True), True),
}
WIDE_HEADS = {"nll20": ("nll", 20), "mse256": ("mse", 256)}
WIDE = dict(I0=784, hidden=[4096, 3072], N=3072)             # test_backward_chain_gpu.py's SHAPES[0] engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _close(eng):
    ex = getattr(eng, "_exchange", None)
    if ex is not None and hasattr(ex, "close"):
        ex.finish()
        torch.cuda.synchronize()
        ex.close()
        eng._exchange = None


# ------------------------------------------------------------------------------------------------ cases, engines, references
@functools.lru_cache(maxsize=None)
def _case(tier, head, draws=None):
    from oracle import vbnn_oracle as vo
    vo.build()
    vo.lib()
    return R.make_case(vo, tier, head, draws=draws)


@functools.lru_cache(maxsize=None)
def _reference(tier, head, draws=None):
    """the float64 step of the case, computed once and shared (bf16: the engine's defaults -- the KL terms live in update())"""
    bf16 = R.TIERS[tier][0] == "bf16"
    return R.reference(_case(tier, head, draws), kl_shadows=bf16, kl_scale=0.0 if bf16 else 1.0)


def _engine(case, draws=None, stream=None, force_reduce=False, **over):
    from vbnn_amd.engine import FusedMLP
    opt = R.engine_opt(case["tier"], case["head"], S=draws or case["S"], **dict(BASELINE, **over))
    eng = FusedMLP(opt, stream=stream, force_reduce=force_reduce)
    with eng._on_stream():
        for v, lay in zip(eng.vb, case["layers"]):
            v.means.copy_(dev(lay["means"])); v.lvars.copy_(dev(lay["lvars"])); v.bias.copy_(dev(lay["bias"]))
        eng.weight3.copy_(dev(case["w3"])); eng.bias3.copy_(dev(case["b3"]))
    return eng


def _issue(eng, x, t, S, stacked=False):
    eng.resetGradients()
    if stacked:
        eng.run_draws(x, t, S)
    else:
        for _ in range(S):
            eng.sample(); eng.run(x, t)
    eng.finish()


def _step(eng, x, t, S, stacked=False):
    eng.prepare()
    _issue(eng, x, t, S, stacked)
    loss, hits = eng.loss_and_accuracy()
    return eng.grads.clone(), loss, hits


def _run_case(tier, head, force_reduce=False, **over):
    case = _case(tier, head)
    eng = _engine(case, force_reduce=force_reduce, **over)
    try:
        res = _step(eng, dev(case["x"]), dev(case["t"]), case["S"])
        if force_reduce:
            assert eng.comm_backend() == "vbnn_comm/rccl", eng.comm_backend()
    finally:
        _close(eng)
    return res, eng


@functools.lru_cache(maxsize=None)
def _baseline(tier, head):
    res, eng = _run_case(tier, head)
    bf16 = R.TIERS[tier][0] == "bf16"
    assert eng.kl_from_shadows == bf16 and eng.kl_in_update == bf16 and eng.f32_direct == (not bf16)
    assert not eng.chain_backward and not eng.dx_first and not eng.overlap and not eng.reduce
    return res


def _check_margins(tier, head, draws=None):
    """the seeds' promise (tests/_step_np.margins), asserted: the hit count cannot turn on a rounding"""
    ok, have, need = R.margins(_case(tier, head, draws), _reference(tier, head, draws))
    assert ok, f"{tier} {head}: the float64 logits' margin {have:.3e} is below {need:.3e}: choose another seed"


def _hold_to_float64(tier, head, got, what, draws=None):
    """(a): loss, hit count and every arena region of `got` against the float64 step, at the tier's engine-level tolerances"""
    grads, loss, hits = got
    case, ref = _case(tier, head, draws), _reference(tier, head, draws)
    _check_margins(tier, head, draws)
    regions = R.arena_regions(host(grads).astype(np.float64), case["sizes"], case["n_classes"])
    f32 = case["dtype"] == "f32"
    tol_loss = 3e-5 * abs(ref["loss"]) + 1e-6 if f32 else 1e-4 * abs(ref["loss"])
    shares = {"loss": abs(loss - ref["loss"]) / tol_loss}
    for name in R.region_names(len(case["layers"])):
        want, have = ref["regions"][name], regions[name]
        assert np.isfinite(have).all() and np.abs(want).max() > 0, name
        if f32:
            tol = (2e-4 if name.endswith(".lv") else 3e-5) * np.abs(want).max() + (1e-9 if name == "final.bias" else 1e-10)
            shares[name] = float(np.abs(have - want).max() / tol)
        else:
            shares[name] = float(np.linalg.norm(have - want) / np.linalg.norm(want) / 2e-3)
    worst = max(shares, key=shares.get)
    print(f"STEP-MATRIX float64 | {tier} | {head} | {what} | loss share {shares['loss']:.3f} | worst region {worst} "
          f"{shares[worst]:.3f} | d/dlvars {max(v for k, v in shares.items() if k.endswith('.lv')):.3f} | hits {hits}")
    assert hits == ref["hits"], (tier, head, what, hits, ref["hits"])
    bad = {k: round(v, 3) for k, v in shares.items() if not v <= 1.0}
    assert not bad, f"{tier} {head} {what}: shares of the tolerance above 1: {bad}"


def _same_bits(got, want, what):
    assert got[1] == want[1] and got[2] == want[2], (what, got[1:], want[1:])
    assert bool(torch.isfinite(want[0]).all()) and float(want[0].abs().max()) > 0.0
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), f"{what}: the gradient arena differs from the baseline's"


# ------------------------------------------------------------------------------------------------ (a) the anchor
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("tier", list(R.TIERS))
def test_baseline_schedule_is_the_float64_step(tier, head):
    """Every head on the baseline schedule (dx_first = False, chain_backward = False, no overlap, no exchange), S = 2 sequential
    draws: loss, hit count (exactly) and every arena region against tests/_step_np.py."""
    _hold_to_float64(tier, head, _baseline(tier, head), "baseline")


# ------------------------------------------------------------------------------------------------ (b) the schedules
@pytest.mark.parametrize("schedule", list(BITWISE_BF16))
@pytest.mark.parametrize("head", HEADS)
def test_bf16_schedules_are_bitwise_the_baseline(head, schedule):
    """small-bf16 (256-[512, 256], 512 rows, S = 2): dx_first, the chained backward in both orders (at this size the two-call
    fallback: VBNN_DEBUG_LAST_CHAINED == 0), the second stream, and the one-rank RCCL exchange with and without the early
    d/dlvars message issue the same tiles on the same operands: arena, loss and hit count bitwise the baseline's."""
    from vbnn_amd import _lib as L
    over, reduce = BITWISE_BF16[schedule]
    got, eng = _run_case("small-bf16", head, force_reduce=reduce, **over)
    if schedule.startswith("chain"):
        assert eng.chain_backward == schedule[-2:] and L.lib().vbnn_debug_get(L.DEBUG_LAST_CHAINED) == 0
    if schedule == "dx_first":
        assert eng.dx_first and not eng.chain_backward
    if schedule == "exchange-early-lv":
        assert eng.early_lv == [True, True]
        print(f"{head}: early d/dlvars message per layer: {[bool(eng._early(v)) for v in eng.vb]}")
    _same_bits(got, _baseline("small-bf16", head), f"small-bf16 {head} {schedule}")


@pytest.mark.parametrize("head", HEADS)
def test_f32_second_stream_is_bitwise_the_pair_launch_step(head):
    """small-f32 (70-[50, 34], 37 rows, S = 2): opt.overlap issues accGradParameters and updateGradInput as their own launches on
    two streams where the default step issues vbnn_backward_pair -- each tile bitwise what its own launch computes."""
    got, eng = _run_case("small-f32", head, overlap=True)
    assert eng.overlap and eng.f32_direct
    _same_bits(got, _baseline("small-f32", head), f"small-f32 {head} overlap")


@pytest.mark.parametrize("schedule", ["exchange", "exchange-early-lv", "keep_transposes"])
@pytest.mark.parametrize("head", HEADS)
def test_f32_other_kernels_hold_the_float64_step(head, schedule):
    """small-f32 schedules that take other kernels than the baseline BY DESIGN, held to the float64 step instead of bitwise: with
    an exchange the fp32 step leaves the direct forms (FusedMLP._alloc_batch: f32_direct needs `not self.reduce` -- packed
    operands, x.x as an operand of the two-launch accGradParameters); keep_transposes is the packed / transposed operand path
    (the same line: f32_direct needs `not keep_transposes`)."""
    over, reduce = {"exchange": (dict(early_lv=False), True), "exchange-early-lv": (dict(early_lv=True), True),
                    "keep_transposes": (dict(keep_transposes=True), False)}[schedule]
    got, eng = _run_case("small-f32", head, force_reduce=reduce, **over)
    assert not eng.f32_direct
    _hold_to_float64("small-f32", head, got, schedule)


@pytest.mark.parametrize("head", HEADS)
def test_bf16_transposed_operands_hold_the_float64_step(head):
    """small-bf16 with keep_transposes: the transposed copies instead of K-major operands wherever the baseline reads K-major
    (other kernels by design, FusedMLP._alloc_batch: km_ok), held to the float64 step."""
    got, eng = _run_case("small-bf16", head, keep_transposes=True)
    assert not any(v.dw_km or v.dx_km for v in eng.vb)
    _hold_to_float64("small-bf16", head, got, "keep_transposes")


# ---- wide-bf16: 784-[4096, 3072] on 3072 rows, S = 1 -- where the chained launch, the K-major two-pass kernels and dx_first live
def _need_256_cus():
    from vbnn_amd import _lib as L
    from vbnn_amd import nn
    sp, n = C.c_void_p(), C.c_int()
    L.check(L.lib().vbnn_ctx_stream(nn.Context.get().h, C.byref(sp), C.byref(n)))
    if n.value != 256:
        pytest.skip(f"the shapes are the smallest that take the two-pass kernel on 256 CUs; this context plans for {n.value}")


@functools.lru_cache(maxsize=None)
def _wide_data(head):
    from vbnn_amd import nn
    crit, Cn = WIDE_HEADS[head]
    N, I0 = WIDE["N"], WIDE["I0"]
    x = torch.empty(N, I0, dtype=torch.float32, device="cuda")
    nn.fill_normal(x, R.SEED, R.STREAM_DATA, 0, 0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    if crit == "nll":
        t = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 % Cn).to(torch.int32)
    else:
        t = torch.randn((N, Cn), generator=gen, device="cuda", dtype=torch.float32)
    sizes = [I0] + WIDE["hidden"]
    lvars = [float(np.log(1e-3)) + 0.3 * torch.randn((sizes[k + 1], sizes[k]), generator=gen, device="cuda", dtype=torch.float32)
             for k in range(len(WIDE["hidden"]))]
    return x, t, lvars


def _wide_step(head, force_reduce=False, **over):
    from vbnn_amd.engine import FusedMLP
    crit, Cn = WIDE_HEADS[head]
    x, t, lvars = _wide_data(head)
    opt = dict(var_init=1e-3, mu_init=1, B=1e6, S=1, mode="lrt", dtype="bf16", seed=R.SEED, keep_e=True, input_size=WIDE["I0"],
               hidden=list(WIDE["hidden"]), n_classes=Cn, criterion=crit, type="vb", testSamples=2, fuse_kl=True)
    eng = FusedMLP(dict(opt, **dict(BASELINE, **over)), force_reduce=force_reduce)
    try:
        for v, lv in zip(eng.vb, lvars):
            v.lvars.copy_(lv)
        res = _step(eng, x, t, 1)
        if force_reduce:
            assert eng.comm_backend() == "vbnn_comm/rccl"
    finally:
        _close(eng)
    return res, eng


@functools.lru_cache(maxsize=None)
def _wide_baseline(head):
    res, eng = _wide_step(head)
    assert not eng.chain_backward and not eng.dx_first and not eng.overlap and not eng.reduce
    return res


@pytest.mark.parametrize("head", list(WIDE_HEADS))
def test_wide_baseline_kmajor_against_transposed_operands(head):
    """wide-bf16 has no float64 run (minutes); its baseline is anchored as test_full_size_step_properties anchors the benchmark
    step: the launches with the transposed copies (debug key 6 = 0) are other kernels over other buffers and must agree within
    2e-3 relative Frobenius per region, the loss within 1e-6."""
    _need_256_cus()
    from vbnn_amd import _lib as L
    base = _wide_baseline(head)
    L.check(L.lib().vbnn_debug_set(6, 0))
    try:
        (g_t, loss_t, hits_t), eng_t = _wide_step(head)
    finally:
        L.check(L.lib().vbnn_debug_set(6, 1))
    _, eng_k = _wide_step(head)                        # (the baseline again, for its operand forms: the two runs did differ)
    forms = [(bool(v.dw_km), bool(v.dx_km)) for v in eng_k.vb]
    print(f"wide-bf16 {head}: K-major (accGradParameters, updateGradInput) per layer {forms}")
    assert any(a or b for a, b in forms) and not any(v.dw_km or v.dx_km for v in eng_t.vb)
    Cn = WIDE_HEADS[head][1]
    sizes = [WIDE["I0"]] + WIDE["hidden"]
    a, b = R.arena_regions(host(base[0]), sizes, Cn), R.arena_regions(host(g_t), sizes, Cn)
    shares = {}
    for k in a:
        want = a[k].astype(np.float64)
        shares[k] = float(np.linalg.norm(b[k] - want) / np.linalg.norm(want)) / 2e-3
    share_loss = abs(loss_t - base[1]) / (1e-6 * abs(base[1]))
    worst = max(shares, key=shares.get)
    print(f"STEP-MATRIX kmajor-off | wide-bf16 | {head} | baseline | loss share {share_loss:.2e} | worst region {worst} {shares[worst]:.2e}")
    assert np.isfinite(base[1]) and share_loss <= 1.0
    assert all(v <= 1.0 for v in shares.values()), shares


@pytest.mark.parametrize("schedule", list(BITWISE_BF16))
@pytest.mark.parametrize("head", list(WIDE_HEADS))
def test_wide_schedules_are_bitwise_the_baseline(head, schedule):
    """wide-bf16: the schedules of the small tier where the second layer's pair runs on the two-pass 256 x 256 kernel -- the
    chained cases must have chained (VBNN_DEBUG_LAST_CHAINED == 1)."""
    _need_256_cus()
    from vbnn_amd import _lib as L
    over, reduce = BITWISE_BF16[schedule]
    base = _wide_baseline(head)
    got, eng = _wide_step(head, force_reduce=reduce, **over)
    if schedule.startswith("chain"):
        assert eng.chain_backward == schedule[-2:] and L.lib().vbnn_debug_get(L.DEBUG_LAST_CHAINED) == 1, "the second layer's pair must chain"
    _same_bits(got, base, f"wide-bf16 {head} {schedule}")


# ------------------------------------------------------------------------------------------------ (c) stacked draws
@pytest.mark.parametrize("head", GENERIC)
def test_stacked_draws_of_the_generic_heads(head):
    """small-f32, S = 3: run_draws against three sequential draws (loss 2e-6 relative, the hit count exactly, the arena 2e-5
    relative Frobenius: test_stacked_draws_equal_sequential_draws' bounds for fp32) and against the float64 step."""
    S = 3
    case = _case("small-f32", head, S)
    x, t = dev(case["x"]), dev(case["t"])
    seq, stk = _engine(case, S), _engine(case, S)
    g_a, loss_a, hits_a = _step(seq, x, t, S)
    g_b, loss_b, hits_b = _step(stk, x, t, S, stacked=True)
    assert stk.draw == seq.draw == S
    rel = float((g_b - g_a).norm() / g_a.norm())
    print(f"STEP-MATRIX stacked-vs-sequential | small-f32 | {head} | S=3 | loss share {abs(loss_a - loss_b) / (2e-6 * abs(loss_a)):.3f} "
          f"| arena share {rel / 2e-5:.3f}")
    assert abs(loss_a - loss_b) <= 2e-6 * abs(loss_a) and hits_a == hits_b
    assert rel <= 2e-5, rel
    _hold_to_float64("small-f32", head, (g_a, loss_a, hits_a), "sequential S=3", draws=S)
    _hold_to_float64("small-f32", head, (g_b, loss_b, hits_b), "stacked S=3", draws=S)


# ------------------------------------------------------------------------------------------------ (d) capture
def _target_variants(case, n):
    """the targets of n successive steps: each differs from the last in every row"""
    t = case["t"]
    if case["criterion"] == "nll":
        return [dev(((t.astype(np.int64) + 3 * k) % case["n_classes"]).astype(np.int32)) for k in range(n)]
    if case["criterion"] == "bce":
        return [dev(t if k % 2 == 0 else (1.0 - t).astype(np.float32)) for k in range(n)]
    return [dev((t + np.float32(0.5 * k)).astype(np.float32)) for k in range(n)]


def _host_loss(eng, case, t_now, S, stacked):
    """the loss of the step the engine just ran, from its own logits and the targets it should have read (float64 criterion)"""
    N = case["N"]
    logits = host(eng.logits)
    if not stacked:                                       # sequential draws: the logits of the last draw only
        return None
    inv_n = 1.0 / N
    return sum(R.criterion(case["criterion"], logits[s * N:(s + 1) * N], t_now, inv_n, logvar_clamp=eng.logvar_clamp)[0] for s in range(S))


@pytest.mark.parametrize("S,stacked", [(2, False), (3, True)], ids=["S2-sequential", "S3-stacked"])
@pytest.mark.parametrize("head", HEADS)
def test_captured_step_is_bitwise_the_launched_step(head, S, stacked):
    """small-f32, opt.device_draw, an engine stream: one un-captured issue, capture_step, three replays -- each bitwise (arena,
    loss, hit count) the same step issued launch by launch on a twin engine. Before every step new target VALUES are copied into
    the callers' target tensors: a replay re-reads them (the stacked generic head through the engine's own stacked-target buffer,
    whose fill is part of the recorded step) -- checked against the twin and, for the stacked draws, against the criterion
    evaluated on the host from the replay's own logits and the NEW targets."""
    case = _case("small-f32", head, S)
    variants = _target_variants(case, 4)
    x = dev(case["x"])
    torch.cuda.synchronize()

    def make():
        s = torch.cuda.Stream()
        e = _engine(case, S, stream=s, device_draw=True)
        t = variants[0].clone()
        with torch.cuda.stream(s):
            e.prepare()
        torch.cuda.synchronize()
        return e, s, t, (lambda: _issue(e, x, t, S, stacked))

    ea, sa, ta, issue_a = make()
    want = []
    for step in range(4):                                        # launch by launch
        ta.copy_(variants[step])
        torch.cuda.synchronize()                                 # (the copy ran on the caller's stream)
        with torch.cuda.stream(sa):
            issue_a()
        loss, hits = ea.loss_and_accuracy()
        want.append((ea.grads.clone(), loss, hits))
    assert want[1][1] != want[2][1] and not torch.equal(want[1][0], want[2][0])

    eb, sb, tb, issue_b = make()
    with torch.cuda.stream(sb):
        issue_b()                                                # step 1 un-captured: allocations, first-launch configuration
    loss, hits = eb.loss_and_accuracy()
    _same_bits((eb.grads, loss, hits), want[0], f"{head}: the un-captured step")
    g = eb.capture_step(issue_b)
    try:
        assert g.nodes >= g.kernel_nodes > 0
        print(f"{head} {'stacked' if stacked else 'sequential'}: {g.kernel_nodes} kernel nodes of {g.nodes}")
        for step in range(1, 4):                                 # steps 2..4 as graph replays
            tb.copy_(variants[step])
            g.launch()
            loss, hits = eb.loss_and_accuracy()
            _same_bits((eb.grads, loss, hits), want[step], f"{head}: replay {step}")
            lh = _host_loss(eb, case, host(variants[step]), S, stacked)
            if lh is not None:
                assert abs(loss - lh) <= 3e-5 * abs(lh) + 1e-6, (head, step, loss, lh)      # (a)'s fp32 loss tolerance
                stale = _host_loss(eb, case, host(variants[step - 1]), S, stacked)
                assert abs(loss - stale) > 4 * (3e-5 * abs(lh) + 1e-6), "the test's targets do not move the loss"
        assert eb.draw == ea.draw
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ (e) no allocation in a step
@pytest.mark.parametrize("S,stacked", [(2, False), (3, True)], ids=["S2-sequential", "S3-stacked"])
@pytest.mark.parametrize("head", HEADS)
def test_a_step_allocates_nothing(head, S, stacked):
    """After one warm-up issue a second issue of the same step leaves torch's count of allocations where it was: a step that a
    graph may replay cannot own memory the allocator can give away (a temporary made inside run() is such memory)."""
    case = _case("small-f32", head, S)
    eng = _engine(case, S)
    x, t = dev(case["x"]), dev(case["t"])
    eng.prepare()
    _issue(eng, x, t, S, stacked)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    _issue(eng, x, t, S, stacked)
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats()["allocation.all.allocated"]
    assert after - before == 0, f"{head}: {after - before} allocations inside one step"
