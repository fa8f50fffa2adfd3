"""Every grid-stride loop and every finish loop taken round a second time, against the references of the family's own test file.

The streaming kernels launch a capped grid (about eight workgroups a compute unit) and walk the rest of their input in a
grid-stride loop; the kernels that add workgroup partials stride by 256. At a few dozen rows neither loop iterates twice, so
the family files never reach what a second trip newly runs: the LDS buffers and per-thread totals carried from row to row, the
`continue` of a ragged last trip, the barrier before the next tile's fill. The cases here take the runners, inputs and checks
of the family files by name and only choose the size and, where the cap follows the context's compute units, the context:

  * default context, more than 2 x 256 workgroups: the finish of the partials loops a third time;
  * a context of cus // 64 compute units (the cap shrinks with it): every workgroup takes four trips or more. Per row and per
    element the outputs are bit for bit those of the default context -- only the partition of the rows over workgroups differs,
    and a row's sum order depends on its width alone -- while the totals, whose partials group differently, keep their bound.

Each case first ASSERTS, from the cap expression mirrored beside the source line that states it and the compute-unit count
vbnn_ctx_stream reports, that its launch takes the trips it is there for, with a factor of four over the cap so that a retuned
cap fails the assertion before it silently makes the case a one-trip test. Outputs start as NaN or a sentinel in every runner,
so a row no trip visited shows. The small context is safe for these kernels: none of them waits on another workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _conformal_np as CF
from tests import _gauss_np as G
from tests import _labels_np as B
from tests import _quantiles_np as Q
from tests import test_conformal_gpu as TC
from tests import test_gauss_gpu as TG
from tests import test_labels_gpu as TL
from tests import test_predict_classes_gpu as TK
from tests import test_predict_regression_gpu as TR
from tests import test_propagate_gpu as TP
from tests import test_quantiles_gpu as TQ
from tests._classes_np import check_classes
from tests._regress_np import check_moments

pytestmark = pytest.mark.gpu

FINISH_STRIDE = 256                     # k_moments_finish (moments_common.h:103) and the *_finish kernels of elementwise.hip
FACTOR = 4                              # every size is at least this many times what one trip of the capped grid holds


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lib():
    from vbnn_amd import _lib as L
    from vbnn_amd.nn import Context
    return L, L.lib(), Context.get().h


def cus_of(h=None):
    """The compute units the launches of context h (default: the default context) are tiled for."""
    L, lib, own = _lib()
    sp, n = C.c_void_p(), C.c_int()
    L.check(lib.vbnn_ctx_stream(h or own, C.byref(sp), C.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def small():
    """A context of cus // 64 compute units on a stream of its own, destroyed when the module's cases are done."""
    from vbnn_amd import nn
    L, lib, _ = _lib()
    cus = cus_of()
    ctx = nn.Context.with_cu_budget(0, max(1, cus // 64))
    try:
        assert cus_of(ctx.h) == ctx.cu_budget == max(1, cus // 64) < cus
        yield ctx
    finally:
        torch.cuda.synchronize()
        L.check(lib.vbnn_ctx_destroy(ctx.h))


def assert_trips(items, per_workgroup, cap, what):
    """`items` over a grid capped at `cap` workgroups of `per_workgroup` items each: the cap binds, every workgroup takes a
    second trip and the size keeps FACTOR over the cap. Returns (workgroups, trips of the busiest workgroup)."""
    per_trip = per_workgroup * cap
    assert items > 2 * per_trip and items >= FACTOR * per_trip, f"{what}: {items} items, {per_trip} a trip -- no longer a several-trip case"
    return cap, -(-items // per_trip)


# ================================================================================================ the moments family
def mom_plan(R, width, cus):
    """MomPlan (moments_common.h:127-128): (workgroups, rows a workgroup works per trip)."""
    rows = 4 if width <= 256 else 1                                    # one wave per row, four rows a workgroup; else a workgroup per row
    return min(-(-R // rows), 8 * cus), rows


MOMENT_SHAPES = [(2051, 5, 3), (517, 260, 2)]                          # (R, D or C, S): wave per row (513 workgroups, a ragged last); workgroup per row


class Regress:
    per_row = ("mean", "var", "row_var", "row_sq_err", "row_log_lik")

    def __init__(self, R, D, S):
        self.y, self.t = TR.normal((S, R, D), 11), TR.normal((R, D), 12)

    def run(self, form, ctx=None):
        return TR.run_moments(self.y, self.t, form, 0.5, ctx=ctx)

    def check(self, got, label):
        check_moments(got, self.y, self.t, 0.5, label=label)

    same = staticmethod(TR.assert_same_outputs)


class Gauss:
    per_row = TG.OUT_KEYS

    def __init__(self, R, D, S):
        self.y, self.t = TG.moments_data(R, D, S, scale=4.0)
        self.nll = None

    def run(self, form, ctx=None):
        from vbnn_amd import _lib as L
        first = self.nll is None and form == L.MOMENTS_ACCUMULATE and ctx is None
        got = TG.run_gmoments(self.y, self.t, form, draw_nll=first, ctx=ctx)
        if first:
            self.nll = got.pop("nll")                                  # every draw's nll_s as the device leaves it: check_gauss_moments holds it too
        return got

    def check(self, got, label):
        G.check_gauss_moments(got, self.y, self.t, TG.S_MIN, TG.S_MAX, nll=self.nll, label=label)

    same = staticmethod(TG.assert_same_outputs)


class Classes:
    per_row = ("entropy", "expected_entropy", "mutual_info", "pred", "probs", "log_probs", "topk_idx", "topk_prob")

    def __init__(self, R, Cn, S):
        self.y = (np.float32(2.0) * np.random.default_rng(11).standard_normal((S, R, Cn)).astype(np.float32)).astype(np.float32)
        self.t = np.random.default_rng(12).integers(0, Cn, R).astype(np.int32)
        self.K = min(5, Cn)
        self.rows = None

    def run(self, form, ctx=None):
        got = TK.run_classes(self.y, self.t, form, self.K, ctx=ctx)
        if "rows" in got and self.rows is None:
            self.rows = got["rows"]                                    # the ACCUMULATE state's row values; STACKED equals them bitwise
        return got

    def check(self, got, label):
        check_classes(dict(got, rows=got.get("rows", self.rows)), self.y, self.t, self.K, label=label)

    @staticmethod
    def same(a, b, what):
        TK.assert_same_outputs(a, b, what)


class Labels:
    per_row = TL.ELEM_KEYS + TL.ROW_KEYS

    def __init__(self, R, D, S):
        self.y, self.t = TL.moments_data(R, D, S)
        # check_label_moments wants inputs free of near ties (a mean probability within rounding of 1/2): at 10^5 elements a
        # few are, and their first draw's logit moves away
        ref = B.label_moments64(self.y, self.t)
        near = B.tie_margin(ref, S) <= 4.0
        self.y[0][near] += np.float32(1.0)
        assert (B.tie_margin(B.label_moments64(self.y, self.t), S) > 4.0).all()

    def run(self, form, ctx=None):
        return TL.run_lmoments(self.y, self.t, form, ctx=ctx)

    def check(self, got, label):
        B.check_label_moments(got, self.y, self.t, label=label)

    same = staticmethod(TL.assert_same_outputs)


FAMILIES = {"vbnn_predict_moments": Regress, "vbnn_predict_gauss_moments": Gauss, "vbnn_predict_class_moments": Classes,
            "vbnn_predict_label_moments": Labels}
_MOMENTS = {}


def moments_on_the_default_context(family, R, D, S):
    """(the family's inputs, {form: outputs}) of the default context, each form held to float64 and the two to each other bit
    for bit; computed once per shape and shared by the cases below."""
    from vbnn_amd import _lib as L
    key = (family, R, D, S)
    if key not in _MOMENTS:
        fam = FAMILIES[family](R, D, S)
        acc = fam.run(L.MOMENTS_ACCUMULATE)
        stk = fam.run(L.MOMENTS_STACKED)
        fam.check(acc, f"{family} {R}x{D}x{S} accumulate")
        fam.check(stk, f"{family} {R}x{D}x{S} stacked")
        fam.same(stk, acc, f"{family} {R}x{D}x{S}: the forms agree bitwise")
        _MOMENTS[key] = fam, {L.MOMENTS_ACCUMULATE: acc, L.MOMENTS_STACKED: stk}
    return _MOMENTS[key]


@pytest.mark.parametrize("R,D,S", MOMENT_SHAPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_moments_finish_adds_more_partials_than_its_stride(family, R, D, S):
    nb, rows = mom_plan(R, D, cus_of())
    assert nb > 2 * FINISH_STRIDE, f"{nb} partials: k_moments_finish no longer takes a third trip"
    assert nb == -(-R // rows) and (rows == 1 or R % rows), "every row in one trip, the last workgroup ragged"
    fam, got = moments_on_the_default_context(family, R, D, S)
    assert all("totals" in g and np.isfinite(g["totals"]).all() for g in got.values())
    print(f"{family} R {R} D {D}: {nb} workgroups of {rows} rows, {nb} partials, {-(-nb // FINISH_STRIDE)} trips of the finish")


@pytest.mark.parametrize("R,D,S", MOMENT_SHAPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_moments_rows_take_several_trips_on_a_small_grid(family, R, D, S, small):
    from vbnn_amd import _lib as L
    nb, rows = mom_plan(R, D, small.cu_budget)
    _, trips = assert_trips(R, rows, 8 * small.cu_budget, family)       # MomPlan's cap, moments_common.h:128
    assert nb == 8 * small.cu_budget and R % (rows * nb), "the cap binds and the last trip is partial"
    fam, base = moments_on_the_default_context(family, R, D, S)
    got = {}
    for form in (L.MOMENTS_ACCUMULATE, L.MOMENTS_STACKED):
        got[form] = fam.run(form, ctx=small.h)
        fam.check(got[form], f"{family} {R}x{D}x{S} form {form} on {small.cu_budget} CUs")       # (a) and (c): float64, totals included
        for k in fam.per_row:                                                                   # (b): the default context's bits
            assert same_bits(got[form][k], base[form][k]), (family, form, k, "differs from the default context's output")
    fam.same(got[L.MOMENTS_STACKED], got[L.MOMENTS_ACCUMULATE], f"{family} on the small grid: the forms agree bitwise")
    print(f"{family} R {R} D {D}: {nb} workgroups of {rows} rows, {trips} trips each")


# ================================================================================================ vbnn_predict_quantiles
def quant_tile(S, kind):
    """The tile of k_quantiles (quantiles.hip:302-304): T elements whose S draws (GAUSS: two planes) fit the tile's LDS share."""
    T = 256
    while S * (2 if kind == Q.GAUSS else 1) * T * 4 > 65536 - 256:
        T >>= 1
    return T


QUANT_KINDS = {"empirical": Q.EMPIRICAL, "fixed_noise": Q.FIXED_NOISE, "gauss": Q.GAUSS}
QUANT_LAYOUTS = {"16-byte loads": {}, "4-byte loads": dict(y_offset=1)}  # the first fills other threads' columns: the barrier branch
_QUANT = {}


def quantiles_on_the_default_context(name):
    """(y, t, kind, p, kwargs, verify, outputs) of the 200 x 200 x 30 case of a kind on the default context. verify(got) holds
    outputs to the kind's restatement (EMPIRICAL: bit for bit; the mixtures: the bracket criterion against float64) with pit,
    row_le and count_le; the default context's have passed it."""
    if name not in _QUANT:
        kind = QUANT_KINDS[name]
        if kind == Q.EMPIRICAL:
            y, t = TQ.empirical_data(200, 200, 30, 41)
            p, kw = tuple(float(np.float32(v)) for v in Q.P3), {}
        else:
            y, t, _, p, kw = Q.mixture_case("gauss-calibration" if kind == Q.GAUSS else "fixed-calibration")
        if kind == Q.EMPIRICAL:
            q_ref, pit_ref = Q.empirical32(y, p, t)
            row_ref, count_ref = TQ.counts_of(q_ref, t)

            def verify(got):
                assert same_bits(got["q"], q_ref) and same_bits(got["pit"], pit_ref)
                assert np.array_equal(got["row_le"], row_ref) and np.array_equal(got["count_le"], count_ref)
                assert (got["q_pads"] == TQ.SENTINEL).all()
        else:
            def verify(got):
                TQ.check_mixture(name, got, y, t, kind, p, kw)          # (the counts: exact, from the kernel's own q)
                assert (got["q_pads"] == TQ.SENTINEL).all()
        st, got = TQ.run_quantiles(y, p, kind, t, **kw)
        TQ.ok(st)
        verify(got)
        _QUANT[name] = y, t, kind, p, kw, verify, got
    return _QUANT[name]


@pytest.mark.parametrize("layout", list(QUANT_LAYOUTS))
@pytest.mark.parametrize("name", list(QUANT_KINDS))
def test_quantile_tiles_take_several_trips_on_a_small_grid(name, layout, small):
    y, t, kind, p, kw, verify, base = quantiles_on_the_default_context(name)
    S, R, W = y.shape
    D = W // 2 if kind == Q.GAUSS else W
    T = quant_tile(S, kind)
    tiles = -(-R * D // T)
    _, trips = assert_trips(tiles, 1, 8 * small.cu_budget, name)        # nb = min(tiles, 8 CUs), quantiles.hip:308
    assert (R * D) % T, "the last tile is partial"
    st, got = TQ.run_quantiles(y, p, kind, t, ctx=small.h, **QUANT_LAYOUTS[layout], **kw)
    TQ.ok(st)
    verify(got)                                                         # (a) the restatement
    for k in ("q", "pit", "row_le", "count_le"):                        # (b) the default context's bits; the layout never changes one
        assert same_bits(got[k], base[k]), (name, layout, k)
    print(f"vbnn_predict_quantiles {name} {layout}: {tiles} tiles of {T}, {8 * small.cu_budget} workgroups, {trips} trips")


# ================================================================================================ vbnn_conformal
def conf_rows_per_workgroup(Cn):
    """(threads, rows a workgroup works per trip) of k_conformal (conformal.hip:31, 372-375): C <= 256 a wave works 64 / G rows,
    G the row's quads rounded up to a power of two; above, 512 threads and a row per wave."""
    if Cn > 256:
        return 512, 512 // 64
    g = 1
    while g < (Cn + 3) // 4:
        g <<= 1
    return 1024, (1024 // 64) * (64 // g)


# (C, R): sixteen, two and one row a wave of the 1024-thread kernel, then the 512-thread tiles NK = 1, 4 and 0
CONF_SHAPES = [(10, 4099), (100, 517), (257, 517), (1030, 261), (4100, 261)]


@pytest.mark.parametrize("kind", [CF.LAC, CF.APS])
@pytest.mark.parametrize("Cn,R", CONF_SHAPES)
def test_conformal_rows_take_several_trips_on_a_small_grid(Cn, R, kind, small):
    threads, rows = conf_rows_per_workgroup(Cn)
    cap = small.cu_budget * (1024 // threads)                           # conformal.hip:341
    _, trips = assert_trips(R, rows, cap, f"vbnn_conformal C {Cn}")
    assert R % (rows * cap), "the last trip is partial"
    probs, target = TC.case(R, Cn, seed=Cn + R)
    qhat = TC.thresholds(probs, target, kind, 3, seed=R)
    want = CF.conformal32(probs, target, kind, qhat)
    base = TC.run_conformal(probs, target, kind, qhat)
    got = TC.run_conformal(probs, target, kind, qhat, ctx=small.h)
    TC.assert_equals_restatement(base, want, (Cn, R, "default context"))
    TC.assert_equals_restatement(got, want, (Cn, R, f"{small.cu_budget} CUs"))         # (a) bit for bit, acc included
    for k in got:
        assert same_bits(got[k], base[k]), (Cn, R, k)                                   # (b)
    TC.assert_invariants(got, probs, target, qhat, want)
    assert int(got["acc"][0]) == R
    print(f"vbnn_conformal C {Cn} R {R}: {cap} workgroups of {rows} rows, {trips} trips")


# ================================================================================================ propagate.hip
def prop_cap(cus):
    return 8 * cus                                                      # prop_grid, propagate.hip:11-13: workgroups of 256 items


PROP_N, PROP_O = 523, 517


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_relu_moments_take_several_trips_on_a_small_grid(dtype, small):
    N, O = PROP_N, PROP_O
    group = 4 if dtype == "f32" else 8                                  # G = 16 / sizeof(T), propagate.hip:101, 108
    _, trips = assert_trips(N * -(-O // group), 256, prop_cap(small.cu_budget), "vbnn_relu_moments")
    m, v1, v2 = TP.relu_inputs(N, O)
    kw = TP.PATHS["vector"](O)
    base = TP.run_relu(m, v1, v2, dtype, **kw)
    got = TP.run_relu(m, v1, v2, dtype, ctx=small.h, **kw)
    TP.check_relu(base, m, v1, v2, dtype)
    TP.check_relu(got, m, v1, v2, dtype)
    assert all(same_bits(got[k], base[k]) for k in got)
    print(f"vbnn_relu_moments {dtype} {N}x{O}: {prop_cap(small.cu_budget)} workgroups, {trips} trips")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_square_shadow_takes_several_trips_on_a_small_grid(dtype, small):
    rows, cols = PROP_N, PROP_O
    group = 4 if dtype == "f32" else 8                                  # propagate.hip:176, 180
    _, trips = assert_trips(rows * -(-cols // group), 256, prop_cap(small.cu_budget), "vbnn_square_shadow")
    base = TP.check_square_shadow(rows, cols, dtype, 0)
    got = TP.check_square_shadow(rows, cols, dtype, 0, ctx=small.h)
    assert same_bits(got, base)
    print(f"vbnn_square_shadow {dtype} {rows}x{cols}: {prop_cap(small.cu_budget)} workgroups, {trips} trips")


def test_logit_draws_take_several_trips_on_a_small_grid(small):
    R, Cn, S, layer, draw, row0 = PROP_N, 85, 3, 2, 5, 11
    _, trips = assert_trips(S * R * -(-Cn // 4), 256, prop_cap(small.cu_budget), "vbnn_logit_draws")     # propagate.hip:225
    g = np.random.default_rng(R * 100 + Cn)
    m = g.standard_normal((R, Cn)).astype(np.float32)
    v = (10.0 ** g.uniform(-3, 1, (R, Cn))).astype(np.float32)
    want = TP.restated_draws(m, v, S, layer, draw, row0)
    base = TP.run_draws(m, v, S, layer, draw, row0)
    assert same_bits(base, want)
    for kw in ({}, dict(ld_y=Cn + 3, stride=R * (Cn + 3) + 5, off=1), dict(ld_y=(Cn + 3) // 4 * 4 + 4)):
        assert same_bits(TP.run_draws(m, v, S, layer, draw, row0, ctx=small.h, **kw), want), kw
    print(f"vbnn_logit_draws {S}x{R}x{Cn}: {prop_cap(small.cu_budget)} workgroups, {trips} trips")


# ================================================================================================ the fixed caps, default context
# elementwise.hip's grid_for (lines 8-13) and vbnn_sgd_step cap the grid at 2048 workgroups whatever the device; the packers at
# 4096 tiles, the layer preparation at 2048. Each entry point gets the smallest shape that sends EVERY workgroup round twice with
# a ragged third trip, through the case function or runner of its family's file and so against that file's restatement and
# bounds. The criteria, the prior and KL sweeps end in a finish kernel over the 2048 partials: eight trips of its 256 threads.
GRID = 2048                                                             # grid_for, elementwise.hip:11
TWICE = 2 * GRID * 256 + 3                                              # items of a 256-a-workgroup launch: two trips and a tail of three


def fixed_trips(items, per_workgroup, what, cap=GRID):
    """The cap binds with every workgroup in a second trip and a ragged last one; with partials, the finish loops too."""
    per_trip = per_workgroup * cap
    assert items > 2 * per_trip and items % per_trip, f"{what}: {items} items, {per_trip} a trip"
    assert cap > FINISH_STRIDE
    print(f"{what}: {items} items, {cap} workgroups of {per_workgroup}, {-(-items // per_trip)} trips, finish {-(-cap // FINISH_STRIDE)} trips over {cap} partials")


def test_relu_forward_and_backward_every_workgroup_twice():
    from tests import test_head_gpu as TH
    fixed_trips(TWICE, 256, "vbnn_relu_forward / _backward (elementwise.hip:494-509)")
    TH.test_relu_forward_and_backward(TWICE)


def test_sgd_step_every_workgroup_twice():
    from tests import test_update_gpu as TU
    fixed_trips(TWICE, 256, "vbnn_sgd_step (optim.hip:73)")
    TU.test_sgd_step_is_the_restatement_bit_for_bit(TWICE)


# (N, C): vbnn_nll_forward strides rows by 256, vbnn_nll_backward elements by 256, vbnn_logsoftmax_backward rows by four
@pytest.mark.parametrize("N,Cn,what,items,per", [
    (TWICE, 2, "vbnn_nll_forward (elementwise.hip:851)", TWICE, 256),
    (349527, 3, "vbnn_nll_backward (elementwise.hip:860)", 349527 * 3, 256),
    (2 * GRID * 4 + 3, 3, "vbnn_logsoftmax_backward (elementwise.hip:868)", 2 * GRID * 4 + 3, 4),
    (2 * GRID * 4 + 3, 17, "vbnn_logsoftmax_backward (elementwise.hip:868)", 2 * GRID * 4 + 3, 4)])
def test_separate_criterion_modules_every_workgroup_twice(N, Cn, what, items, per):
    from tests import test_head_gpu as TH
    fixed_trips(items, per, what)
    TH.test_separate_criterion_modules(N, Cn)


@pytest.mark.parametrize("Cn", [3, 17])
def test_logsoftmax_nll_every_workgroup_twice(Cn):
    from tests import test_head_gpu as TH
    N = 2 * GRID * 4 + 3
    fixed_trips(N, 4, "vbnn_logsoftmax_nll (elementwise.hip:561)")
    rng = np.random.default_rng(N + Cn)
    lg = (rng.standard_normal((N, Cn)) * 3).astype(np.float32)
    target = rng.integers(0, Cn, N).astype(np.int32)
    inv_n = np.float32(1.0 / N)
    TH.check_rows(TH.logsoftmax_nll(lg, target, inv_n), lg, target, inv_n, "a")


# the criteria work 1024 quads of a row's ceil(D / 4) a workgroup: D = 1 is the least memory, D = 5 has a partial second quad
QUADS = 2 * GRID * 1024 + 3
CRIT_SHAPES = [(QUADS, 1), (-(-QUADS // 2), 5)]


@pytest.mark.parametrize("N,D", CRIT_SHAPES)
def test_mse_criterion_every_workgroup_twice(oracle, N, D):
    from vbnn_amd import nn
    from tests import test_parity_gpu as TPAR
    fixed_trips(N * -(-D // 4), 1024, "vbnn_mse_forward / _backward (elementwise.hip:605)")
    TPAR.test_mse_criterion_matches_oracle(nn, oracle, N, D)


@pytest.mark.parametrize("N,D", CRIT_SHAPES)
def test_gauss_criterion_every_workgroup_twice(N, D):
    fixed_trips(N * -(-D // 4), 1024, "vbnn_gauss_nll_forward / _backward (elementwise.hip:682)")
    inv_nd = float(np.float32(1.0 / (N * D)))
    y, t = TG.criterion_data(N, D, 4.0, seed=35)
    loss, g, pads = TG.run_criterion(y, t, inv_nd)
    G.check_criterion(loss, g, y, t, inv_nd, TG.S_MIN, TG.S_MAX, label=f"{N}x{D}")
    assert pads.size == 0
    _, g3, _ = TG.run_criterion(y, t, inv_nd, backward=True)
    assert same_bits(g3, g)


@pytest.mark.parametrize("N,D", CRIT_SHAPES)
def test_bce_criterion_every_workgroup_twice(N, D):
    fixed_trips(N * -(-D // 4), 1024, "vbnn_bce_forward / _backward (elementwise.hip:781)")
    inv_nd = float(np.float32(1.0 / (N * D)))
    z, t = TL.criterion_data(N, D, 4.0, True, seed=35)
    loss, g, pads, hits = TL.run_criterion(z, t, inv_nd)
    B.check_criterion(loss, g, hits, z, t, inv_nd, label=f"{N}x{D}")       # (hits: exact)
    assert pads.size == 0
    _, g3, _, _ = TL.run_criterion(z, t, inv_nd, backward=True)
    assert same_bits(g3, g)


@pytest.mark.parametrize("hw", [False, True], ids=["contract", "hw"])
def test_fill_normal_every_workgroup_twice(hw):
    from tests import test_sweeps_gpu as TS
    rows, cols = 1030, 4100
    fixed_trips(rows * -(-cols // 4), 256, "vbnn_fill_normal / _hw (elementwise.hip:38, 50)")
    TS._fill_case(rows, cols, cols, 0, 0.05, hw, 0)


def test_wn_sample_every_workgroup_twice():
    from tests import test_sweeps_gpu as TS
    O, I = 1040, 4100
    fixed_trips(O * -(-I // 4), 256, "vbnn_wn_sample (elementwise.hip:224)")
    TS._wn_case(O, I, "lvars", False, 0)                                # the route the engine takes
    TS._wn_case(O, I, "stdv", True, 0)


def test_compute_prior_every_workgroup_twice():
    from tests import test_sweeps_gpu as TS
    W = 4 * (2 * GRID * 256 + 3) + 3
    fixed_trips(W // 4 + 1, 256, "vbnn_compute_prior (elementwise.hip:182)")
    TS._prior_case(W, TS.CACHES[0], 0, "trained")
    TS._prior_case(W, (), 0, "wide")


def test_kl_gradients_every_workgroup_twice():
    from tests import test_sweeps_gpu as TS
    fixed_trips(TWICE, 256, "vbnn_compute_mugrads / _vargrads (elementwise.hip:337, 347)")
    TS.test_compute_mugrads(TWICE, 1e6, 30.0)
    for route in ("given", "lvars"):
        TS.test_compute_vargrads(TWICE, 1e6, 30.0, route)


@pytest.mark.parametrize("route", ["cached", "derived"])
def test_calc_lc_every_workgroup_twice(route):
    from tests import test_sweeps_gpu as TS
    fixed_trips(QUADS, 1024, "vbnn_calc_lc (elementwise.hip:400)")
    TS._lc_case(QUADS, route, "trained", 1e6)


def test_calc_lc_masked_every_workgroup_twice():
    from tests import test_finetune_gpu as TF
    O, I = 2049, 2048
    fixed_trips(O * I, 1024, "vbnn_calc_lc_masked (elementwise.hip:416)")
    TF.test_calc_lc_masked(O, I, False, TF.MASKS[0])


PACK_ROWS, PACK_COLS = 2, 64 * 2 * 4096 + 7                            # 8193 tiles of 64 x 64, a ragged edge either way


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fname", ["copy", "exp", "square", "mul", "relu", "relu_square"])
def test_pack_every_workgroup_twice(fname, dtype):
    from tests import test_sweeps_gpu as TS
    fixed_trips(-(-PACK_ROWS // 64) * -(-PACK_COLS // 64), 1, "vbnn_pack (elementwise.hip:296-297)", cap=4096)
    # the transposed output is PACK_COLS rows of a whole pad each: once per dtype
    TS._pack_case(PACK_ROWS, PACK_COLS, fname, dtype, "dt" if fname == "mul" else "d")


def test_pack_input_every_workgroup_twice():
    from tests import test_sweeps_gpu as TS
    fixed_trips(-(-PACK_ROWS // 64) * -(-PACK_COLS // 64), 1, "vbnn_pack_input (elementwise.hip:1545-1546)", cap=4096)
    TS._pack_input_case(PACK_ROWS, PACK_COLS, "bf16", TS.OUTS[0], 0)


def test_prep_layer_every_workgroup_twice():
    from tests import test_sweeps_gpu as TS
    O, I = 2, 64 * 2 * GRID + 1
    fixed_trips(-(-O // 64) * -(-I // 64), 1, "vbnn_prep_layer, the tile form (elementwise.hip:994-995)")
    TS._prep_both_entries(O, I, True, "f32", "trained")
    O, I = 33, 131072                                                   # FLAT: 2048 workgroups stride by 1024 elements each
    assert -(-O // 64) * -(-I // 64) >= GRID
    fixed_trips(O * I, 1024, "vbnn_prep_layer, the flat form (elementwise.hip:901-904)")
    TS._prep_both_entries(O, I, False, "f32", "wide")


def test_digest_takes_the_unrolled_loop_round_twice():
    """k_digest's body loop (digest.hip:45) takes two 16-byte loads a trip; the family's largest size ends after one trip with a
    single quad left over. Here every thread takes two trips, five take a third, the rest one single load, then a tail of three."""
    from tests import _digest_np as D
    from tests import test_checkpoint_gpu as TCK
    stride = GRID * 256                                                 # DIGEST_MAX_BLOCKS x DIGEST_THREADS, digest.hip:14-16
    quads = 5 * stride + 5
    assert quads > 2 * 2 * stride and TCK.GRID_PASS == 2 * 4 * stride
    n = 4 * quads + 3
    host = np.random.RandomState(22).randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    dev = torch.from_numpy(host.view(np.int32)).cuda()
    assert dev.data_ptr() % 16 == 0
    st, out = TCK._digest(dev, n, index0=3)
    assert st == 0 and TCK._value(out) == D.digest(host, 3)
