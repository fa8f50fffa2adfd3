"""vbnn_head_predict (k_head_predict, head.hip) through direct C ABI calls with operands of its own, against the float64
reference of tests/_predict_np.py (held on the CPU by tests/test_predict_ref.py).

One runner (run_predict) packs h (S R rows; ACCUMULATE is given draw s as the R rows at row s R) and w3 with zero pads, gives
every output a sentinel fill with guard rows behind it, pre-fills `state` with NaN before the `first` call, and returns every
output, the totals and, for ACCUMULATE, the state after each call.

What is compared how:
  bit for bit   STACKED against ACCUMULATE; S = 1 log_probs and the state's L of a first call against vbnn_head_forward's out on
                the same operands; S = 1 entropies; pred against the returned log_probs; exact ties of the average; clamped
                targets; the integer totals; skipped optional arguments; the totals of two calls in a row.
  the bounds    _predict_np.check_predict / check_states (derived in that module's docstring) on exact integer logits -- every
                class count, the log-softmax extremes per draw, rotating peaks, uniform draws -- and, for real operands, on the
                device's own logits (vbnn_head_forward's `logits` of the stacked rows, bitwise the predict kernel's by the
                identity test). Every err / tol ratio is printed; the last test prints the largest per quantity.
  the contract  a NaN in any draw of a row (include/vbnn_hip.h), and every refusal with its message, before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _head_np as R
from tests import _predict_np as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_head_gpu import _code, _ctx, _p, bitwise, dev, head_forward, packed  # noqa: E402

F = np.float32
SENT = 7.0
DTYPES = ("f32", "bf16")
FORMS = ("stacked", "accumulate")
FLOAT_OUT = ("probs", "log_probs", "entropy", "expected_entropy", "mutual_info")
OUTPUTS = FLOAT_OUT + ("pred",)
USED = {}                                                  # quantity -> largest err / tol ratio of this module's cases


def record(ratios):
    for k, v in ratios.items():
        USED[k] = max(USED.get(k, 0.0), v)


def run_predict(dtype, op, form, skip=(), bias=True, target=True, totals=True, n_calls=None, repeat=1):
    """vbnn_head_predict on an operand set of _predict_np (h: S R x H, w3: C x H, values the type holds exactly). skip: outputs
    passed as NULL; n_calls: ACCUMULATE runs only that many draws; repeat: the whole prediction is issued that many times into
    the same buffers (the last one's results are returned). Guards are checked here."""
    L, lib, ctx = _ctx()
    S, N, Cn, H = op["S"], op["R"], op["C"], op["H"]
    ld, W = L.pad_ld(H), Cn + 3
    th, tw = packed(op["h"], dtype, ld), packed(op["w3"], dtype, ld)
    tb = dev(np.asarray(op["bias"], F)) if bias and op["bias"] is not None else None
    tt = dev(np.asarray(op["target"], np.int32)) if target else None
    f32 = dict(dtype=torch.float32, device="cuda")
    bufs = {k: torch.full((N + 2, Cn), SENT, **f32) for k in ("probs", "log_probs")}
    bufs.update({k: torch.full((N + 16,), SENT, **f32) for k in ("entropy", "expected_entropy", "mutual_info")})
    bufs["pred"] = torch.full((N + 16,), -7, dtype=torch.int32, device="cuda")
    tot = torch.full((6,), SENT, dtype=torch.float64, device="cuda") if totals and target else None
    accumulate = form == "accumulate"
    state = torch.full((N + 2, W), float("nan"), **f32) if accumulate else None
    a = L.PredictArgs(h=_p(th), ld_h=ld, w3=_p(tw), ld_w=ld, bias=_p(tb), target=_p(tt), R=N, H=H, C=Cn, S=S,
                      form=L.PREDICT_ACCUMULATE if accumulate else L.PREDICT_STACKED, first=1, final=1, state=_p(state),
                      totals=_p(tot), **{k: _p(bufs[k]) for k in OUTPUTS if k not in skip})
    states = []
    for _ in range(repeat):
        if not accumulate:
            L.check(lib.vbnn_head_predict(ctx, _code(dtype), C.byref(a)))
            continue
        # the final call writes the outputs and leaves the state alone: a first pass without it shows the state after EVERY
        # draw (and must write no output), the second is the prediction itself
        for finish in (False, True):
            if (finish and n_calls is not None and n_calls < S) or (not finish and states):
                continue
            state.fill_(float("nan"))
            for s in range(S if n_calls is None else n_calls):
                a.h = C.c_void_p(th.data_ptr() + s * N * ld * th.element_size())
                a.first, a.final = int(s == 0), int(finish and s == S - 1)
                L.check(lib.vbnn_head_predict(ctx, _code(dtype), C.byref(a)))
                if not finish:
                    torch.cuda.synchronize()
                    st = state.cpu().numpy()
                    assert np.isnan(st[N:]).all(), "state: a row >= R was written"
                    states.append(st[:N].copy())
            if not finish:
                for k, v in bufs.items():
                    assert bool((v == (-7 if k == "pred" else SENT)).all()), f"{k}: written before the final call"
                assert tot is None or bool((tot == SENT).all()), "totals: written before the final call"
    torch.cuda.synchronize()
    assert state is None or bool(torch.isnan(state[N:]).all()), "state: a row >= R was written"
    got = {}
    for k in OUTPUTS:
        v = bufs[k].cpu().numpy()
        fill = -7 if k == "pred" else SENT
        if k in skip:
            assert (v == fill).all(), f"{k}: written though NULL was passed"
            continue
        if n_calls is not None and n_calls < S:
            assert (v == fill).all(), f"{k}: written before the final call"
            continue
        assert (v[N:] == fill).all(), f"{k}: written behind its end"
        got[k] = v[:N].copy()
    if tot is not None:
        v = tot.cpu().numpy()
        assert (v[4:] == SENT).all(), "totals: written behind the four sums"
        got["totals"] = v[:4].tolist()
    if accumulate:
        got["states"] = states
        if tt is not None and states:
            got["rows"] = states[-1][:, Cn:].copy()
    return got


def same_outputs(a, b, what, keys=None):
    keys = (set(a) & set(b)) - {"states", "rows"} if keys is None else keys
    for k in sorted(keys):
        if k == "totals":
            assert np.array_equal(np.array(a[k]).view(np.uint64), np.array(b[k]).view(np.uint64)), (what, k, a[k], b[k])
        else:
            bitwise(f"{what}: {k}", a[k], b[k])


def device_logits(dtype, op):
    """The device's own logits of every stacked row (vbnn_head_forward's `logits`), S x R x C, and its `out`."""
    t = np.tile(np.clip(op["target"], 0, op["C"] - 1).astype(np.int32), op["S"])
    res = head_forward(dtype, op["h"], op["w3"], op["bias"], t, F(1.0), op["C"])
    shape = (op["S"], op["R"], op["C"])
    return res["logits"].reshape(shape), res["out"].reshape(shape)


def check(got, lg, op, label, target=True):
    t = op["target"] if target else None
    ref, ratios = P.check_predict(got, lg, t, label=label)
    if got.get("states"):
        ratios.update(P.check_states(got["states"], lg, t, label=label + " state"))
    record(ratios)
    return ref


def both_forms(dtype, op, lg, label):
    """Both forms on one operand set: each inside the bounds, every output and total equal bit for bit."""
    st = run_predict(dtype, op, "stacked")
    ac = run_predict(dtype, op, "accumulate")
    same_outputs(st, ac, label + ", STACKED against ACCUMULATE", set(OUTPUTS) | {"totals"})
    ref = check(ac, lg, op, f"{label} {dtype} accumulate")
    check(dict(st, rows=ac["rows"]), lg, op, f"{label} {dtype} stacked")
    return st, ac, ref


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", P.FORM_R)
@pytest.mark.parametrize("S", P.FORM_S)
def test_stacked_equals_accumulate(S, N, dtype):
    """Distinct draws of real operands: whole blocks, a ragged last block, a single row. Reading draw s at a wrong row offset
    would show in either form against the device's own logits of those rows."""
    op = P.real_set(S, N, 70, 10, 50 + S, dtype)
    lg, out = device_logits(dtype, op)
    st, ac, _ = both_forms(dtype, op, lg, f"real S{S} R{N}")
    if S == 1:
        bitwise("S = 1: log_probs is the forward's out", st["log_probs"], out[0])
        bitwise("S = 1: entropy and expected_entropy", st["entropy"], st["expected_entropy"])
        assert (st["mutual_info"] == 0).all()
        assert st["totals"][0] == st["totals"][2] and st["totals"][1] == st["totals"][3]


def logit_identity(dtype, op):
    _, out = device_logits(dtype, op)
    one = run_predict(dtype, op, "stacked")
    bitwise("log_probs against vbnn_head_forward's out", one["log_probs"], out[0])
    bitwise("entropy against expected_entropy", one["entropy"], one["expected_entropy"])
    assert (one["mutual_info"] == 0).all() and not np.signbit(one["mutual_info"]).any()
    first = run_predict(dtype, dict(op, S=5, h=np.tile(op["h"], (5, 1))), "accumulate", n_calls=1)      # a non-final first call
    bitwise("the state's L after the first call against out", first["states"][0][:, :op["C"]], out[0])
    assert np.isfinite(out).all()


@pytest.mark.parametrize("dtype,H", [("f32", 3456), ("bf16", 6912)])
def test_logits_are_the_forwards_with_all_four_unrolled_k_loops(dtype, H):
    """27 K steps per wave: 16 + 8 + 2 + 1 (test_head_gpu holds the forward's logits at this width)."""
    logit_identity(dtype, P.real_set(1, 17, H, 10, 61, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 31, 33, 130])
def test_logits_are_the_forwards_where_some_waves_have_no_k_step(dtype, H):
    logit_identity(dtype, P.real_set(1, 17, H, 10, 62, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cn", [1, 2, 5, 16])
def test_one_draw_has_no_epistemic_part_at_any_class_count(Cn, dtype):
    """S = 1 at the class counts' edges. With one class the entropy is a zero whose sign the kernel's negated sum sets: a first
    draw that were ADDED to a state of zeros instead of starting it would leave expected_entropy with the other sign -- the one
    place where that edit shows, since logaddexp(-inf, o) is o bit for bit."""
    logit_identity(dtype, P.class_count_set(Cn, S=1))


def assert_tie(got, a, b, label):
    lp = got["log_probs"]
    bitwise(f"{label}: log_probs of the tied classes", lp[:, a], lp[:, b])
    bitwise(f"{label}: probs of the tied classes", got["probs"][:, a], got["probs"][:, b])
    assert (got["pred"] == min(a, b)).all(), (label, got["pred"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", P.TIE_KINDS)
def test_a_tie_in_every_draw_goes_to_the_first_class(kind, dtype):
    for Cn in P.EXTREME_CLASSES:
        a, b = (min(int(k), Cn - 1) for k in kind.split("_")[1:])
        op = P.extreme_set(kind, Cn)
        st, ac, _ = both_forms(dtype, op, P.stacked_logits(op), f"{kind} C{Cn}")
        assert_tie(st, a, b, f"{kind} C{Cn}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a,b", P.TIE_PAIRS)
def test_a_tie_of_two_swapped_draws_goes_to_the_first_class(a, b, dtype):
    op = P.swapped_tie_set(a, b)
    st, ac, _ = both_forms(dtype, op, P.stacked_logits(op), f"swapped tie {a} {b}")
    assert_tie(st, a, b, f"swapped tie {a} {b}")
    t = op["target"]
    assert st["totals"][1] == float((t == min(a, b)).sum()) and st["totals"][3] == float((t == a).sum() + (t == b).sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["target_low", "target_high"])
def test_out_of_range_targets_are_clamped(kind, dtype):
    op = P.extreme_set(kind, 10)
    assert ((op["target"] < 0) | (op["target"] > 9)).any()
    clamped = dict(op, target=np.clip(op["target"], 0, 9).astype(np.int32))
    for form in FORMS:
        got, want = run_predict(dtype, op, form), run_predict(dtype, clamped, form)
        same_outputs(got, want, f"{kind} {form}", set(OUTPUTS) | {"totals"})
        check(got, P.stacked_logits(op), op, f"{kind} {dtype} {form}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_optional_arguments(form, dtype):
    """bias = NULL; target = NULL with totals = NULL; totals = NULL alone; each output NULL on its own: the remaining outputs
    keep their bits, nothing is written behind an output, into a skipped one or into rows >= R of the state (run_predict)."""
    op = P.class_count_set(10, N=19)
    lg = P.stacked_logits(op)
    full = run_predict(dtype, op, form)
    check(full, lg, op, f"optional: all {dtype} {form}")
    nobias = dict(op, bias=None)
    got = run_predict(dtype, nobias, form)
    check(got, P.stacked_logits(nobias), nobias, f"optional: no bias {dtype} {form}")
    assert not np.array_equal(got["log_probs"], full["log_probs"])
    bare = run_predict(dtype, op, form, target=False)
    assert "totals" not in bare
    same_outputs(bare, full, "no target", set(OUTPUTS))
    check(bare, lg, op, f"optional: no target {dtype} {form}", target=False)
    same_outputs(run_predict(dtype, op, form, totals=False), full, "no totals", set(OUTPUTS))
    for k in OUTPUTS:
        got = run_predict(dtype, op, form, skip=(k,))
        assert k not in got
        same_outputs(got, full, f"{k} = NULL", (set(OUTPUTS) | {"totals"}) - {k})
        if form == "accumulate":
            for s in range(op["S"]):
                bitwise(f"{k} = NULL: the state after draw {s}", got["states"][s], full["states"][s])


@pytest.mark.parametrize("dtype", DTYPES)
def test_totals_of_two_calls_in_a_row(dtype):
    op = P.class_count_set(10, N=47)
    for form in FORMS:
        once, twice = run_predict(dtype, op, form), run_predict(dtype, op, form, repeat=2)
        same_outputs(once, twice, f"two calls {form}", set(OUTPUTS) | {"totals"})


def test_totals_over_more_workgroups_than_finish_threads():
    """514 workgroups: the finish block's 512 threads go round their loop a second time."""
    op = P.many_workgroups_set()
    lg = P.stacked_logits(op)
    got = run_predict("f32", op, "stacked", repeat=2)
    ref = check(got, lg, op, "514 workgroups")
    rows, t = np.arange(op["R"]), op["target"]
    want = (-got["log_probs"][rows, t]).astype(np.float64).sum()
    tot = got["totals"]
    assert abs(tot[0] - want) <= 1e-12 * abs(want) and abs(tot[2] - want) <= 1e-12 * abs(want), (tot, want)    # S = 1: sum -o[t] is -log p[t]
    assert tot[1] == float((got["pred"] == t).sum()) == tot[3] == float(ref["hit"].sum()) and tot[1] > 0
    same_outputs(run_predict("f32", op, "accumulate"), got, "514 workgroups, ACCUMULATE", set(OUTPUTS) | {"totals"})


# ------------------------------------------------------------------------------------------------ bounded
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cn", range(1, 17))
def test_every_class_count(Cn, dtype):
    op = P.class_count_set(Cn)
    st, ac, _ = both_forms(dtype, op, P.stacked_logits(op), f"int C{Cn}")
    if Cn == 1:
        assert (st["pred"] == 0).all() and st["totals"][1] == st["totals"][3] / op["S"] == float(op["R"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [k for k in R.EXTREME_KINDS if not k.startswith(("tie_", "target_"))])
def test_log_softmax_extremes_per_draw(kind, dtype):
    """(the tie and target kinds: the exact tests above, which hold them to the bounds too)"""
    for Cn in P.EXTREME_CLASSES:
        op = P.extreme_set(kind, Cn)
        st, ac, ref = both_forms(dtype, op, P.stacked_logits(op), f"{kind} C{Cn}")
        assert np.isfinite(st["log_probs"]).all()
        if kind == "all_equal":                              # uniform draws: log p = -log C
            assert (np.abs(st["log_probs"] + math.log(Cn)) <= P.logp_tol(ref, P.stacked_logits(op))).all()
        if kind in ("peak120", "target100") and Cn > 1:
            assert (ref["probs"] < P.TINY).any(), "no probability of this set underflows"


@pytest.mark.parametrize("dtype", DTYPES)
def test_rotating_peaks_keep_their_logs(dtype):
    """Each draw peaks 120 above the rest at another class: exp(o) is 0 in fp32 for every class but the peak, in every draw."""
    op = P.rotating_peak_set()
    st, ac, ref = both_forms(dtype, op, P.stacked_logits(op), "rotating peaks")
    lp = st["log_probs"]
    peaked = np.zeros(lp.shape, bool)
    for s in range(op["S"]):
        peaked[np.arange(op["R"]), (np.arange(op["R"]) + 3 * s) % op["C"]] = True
    assert np.isfinite(lp).all()
    assert (np.abs(lp[peaked] + math.log(op["S"])) <= 1e-6).all()
    assert (np.abs(lp[~peaked] + 120) <= 10).all()
    assert (st["probs"][~peaked] < P.TINY).all() and (np.abs(st["probs"][peaked] - 1 / 3) <= 1e-6).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_draws_carry_no_information(dtype):
    op = P.identical_draws_set(dtype=dtype)
    lg, out = device_logits(dtype, op)
    st, ac, ref = both_forms(dtype, op, lg, "identical draws")
    one = P.predict64(lg[:1])
    d = np.abs(st["log_probs"] - one["log_probs"])
    assert (d <= P.logp_tol(ref, lg)).all(), float((d / P.logp_tol(ref, lg)).max())
    d = np.abs(st["log_probs"].astype(np.float64) - out[0])
    assert (d <= P.logp_tol(ref, lg) + P.logp_tol(one, lg[:1])).all()
    tol = P.entropy_tol(ref, lg) + P.expected_entropy_tol(ref, lg)
    assert (np.abs(st["mutual_info"]) <= tol).all(), float((np.abs(st["mutual_info"]) / tol).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_operands_with_a_wide_spread(dtype):
    op = P.real_set(3, 37, 70, 10, 43, dtype, scale=8.0)
    lg, _ = device_logits(dtype, op)
    exact = op["h"].astype(np.float64) @ op["w3"].astype(np.float64).T + op["bias"]
    bound = 4e-6 * (np.abs(op["h"]).astype(np.float64) @ np.abs(op["w3"]).astype(np.float64).T) + 1e-6       # test_head_gpu's logit bound
    assert (np.abs(lg.reshape(exact.shape) - exact) <= bound).all()
    both_forms(dtype, op, lg, "real spread x8")


# ------------------------------------------------------------------------------------------------ the NaN contract
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("s_nan", [0, 1, 2])
def test_a_nan_in_any_draw_makes_its_row_nan_and_no_other(s_nan, form, dtype):
    """One NaN element of h in row 5 of 19, draw s_nan of 3, in a hidden unit that no class reads (NaN x 0): every float output of
    the row is NaN, totals [0] and [2] are NaN, the row is no hit in [1] and its NaN draw none in [3], pred stays inside
    [0, C), and every other row keeps its bits."""
    S, N, Cn, row = 3, 19, 10, 5
    lg = np.stack([R.extreme_logits("peak120", N, Cn, seed=11 + s)[0] for s in range(S)])
    target = R.extreme_logits("peak120", N, Cn)[2].copy()
    target[row] = row % Cn                                   # the row's peak in every draw: a hit in the clean call, draw by draw
    op = P.from_logits(lg, np.zeros(Cn, F), target)
    clean = run_predict(dtype, op, form)
    ref = check(clean, P.stacked_logits(op), op, f"NaN test, clean {dtype} {form}")
    assert clean["pred"][row] == target[row] and ref["hit"][:, row].all()
    h = op["h"].copy()
    h[s_nan * N + row, 20] = np.nan
    got = run_predict(dtype, dict(op, h=h), form)
    for k in FLOAT_OUT:
        assert np.isnan(got[k][row]).all(), f"{k} of the NaN row: {got[k][row]}"
    assert 0 <= got["pred"][row] < Cn
    others = np.arange(N) != row
    for k in OUTPUTS:
        bitwise(f"{k} of the other rows", got[k][others], clean[k][others])
    tot, want = got["totals"], clean["totals"]
    assert math.isnan(tot[0]) and math.isnan(tot[2]), tot
    assert tot[1] == want[1] - 1 and tot[3] == want[3] - 1, (tot, want)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch():
    L, lib, ctx = _ctx()
    N, H, Cn, S = 4, 32, 10, 3
    f32 = dict(dtype=torch.float32, device="cuda")
    h, w3 = torch.zeros(S * N + 1, 64, **f32), torch.zeros(Cn, 64, **f32)
    t = torch.zeros(N, dtype=torch.int32, device="cuda")
    tot = torch.full((4,), SENT, dtype=torch.float64, device="cuda")
    state = torch.full((N, Cn + 3), SENT, **f32)
    lp = torch.full((N, Cn), SENT, **f32)

    def args(**kw):
        base = dict(h=_p(h), ld_h=64, w3=_p(w3), ld_w=64, target=_p(t), R=N, H=H, C=Cn, S=S, form=L.PREDICT_STACKED,
                    log_probs=_p(lp), totals=_p(tot))
        base.update(kw)
        return L.PredictArgs(**base)

    def refused(a, match, code=L.F32, ctx=ctx):
        st = lib.vbnn_head_predict(ctx, code, C.byref(a) if a is not None else None)
        assert st != 0
        with pytest.raises(L.VbnnError, match=match):
            L.check(st)

    acc = dict(form=L.PREDICT_ACCUMULATE, state=_p(state))
    refused(None, "null argument")
    refused(args(), "null argument", ctx=None)
    refused(args(w3=None), "null argument")
    for Cbad in (0, 17):
        refused(args(C=Cbad), "shape")
    for k in ("R", "H"):
        refused(args(**{k: 0}), "shape")
    refused(args(S=0), "draws S >= 1")
    for form in (2, -1):
        refused(args(form=form), r"invalid argument: form")
    for k in ("ld_h", "ld_w"):
        refused(args(**{k: 96}), "packed operands")          # no multiple of 64
        refused(args(H=100, **{k: 64}), "packed operands")   # below H
    refused(args(h=C.c_void_p(h.data_ptr() + 4)), "16-byte aligned")
    refused(args(w3=C.c_void_p(w3.data_ptr() + 4)), "16-byte aligned")
    refused(args(target=None), "totals need targets")
    for first, final in ((1, 0), (0, 1), (0, 0)):
        refused(args(form=L.PREDICT_ACCUMULATE, first=first, final=final), "running state")
    refused(args(), "unsupported dtype", code=99)
    # R above the reduction scratch ((R + 15) / 16 * 4 > 2^21 doubles): refused before the small buffers above are touched
    refused(args(R=16 * (1 << 19) + 1), "reduction scratch")
    refused(args(R=16 * (1 << 19) + 1, first=1, final=1, **acc), "reduction scratch")
    torch.cuda.synchronize()
    assert (lp.cpu().numpy() == SENT).all() and (tot.cpu().numpy() == SENT).all() and (state.cpu().numpy() == SENT).all()
    # ... and what is allowed: ACCUMULATE without a state when the one call is first and final
    L.check(lib.vbnn_head_predict(ctx, L.F32, C.byref(args(S=1, form=L.PREDICT_ACCUMULATE, first=1, final=1))))
    torch.cuda.synchronize()
    got = lp.cpu().numpy()                                  # zero operands: uniform (logf within its ulp), class 0 wins
    assert (got == got[0, 0]).all() and abs(got[0, 0] + math.log(Cn)) <= 2 * R.ULP * math.log(Cn)
    assert tot.cpu().numpy().tolist()[1::2] == [float(N), float(N)]


def test_the_largest_share_of_each_bound_the_device_used():
    """Prints, per quantity, the largest err / tol ratio over the cases of this module that ran before it; each was asserted <= 1
    where it was measured. tests/_predict_np.BOUND_USED records what an fp32 restatement uses on the CPU."""
    print("vbnn_head_predict, largest err / tol per quantity: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(USED.items())))
    print("fp32 restatement on the CPU (BOUND_USED):          " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(P.BOUND_USED.items())))
    assert all(v <= 1.0 for v in USED.values())
