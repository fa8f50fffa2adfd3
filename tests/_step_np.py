"""Float64 restatement of one FusedMLP step for every head kind (tests/test_step_ref.py holds it on the CPU,
tests/test_step_matrix_gpu.py holds the engine to it). It generalises oracle.ref_numpy.emulate_lrt_step -- whose `nll` and `mse`
arithmetic it repeats operation for operation, so that the two agree to float64 rounding -- to the `gauss` and `bce` criteria
(tests/_gauss_np.criterion64, tests/_labels_np.criterion64: the criteria are NOT restated here), to S draws accumulating in the
arena, to the hit count, and to the arena's own region names (vbnn_amd.partition.arena_layout).

Rounding points: `rnd` wherever the engine stores a GEMM operand (identity for f32, oracle.ref_numpy.bf16_round for bf16), `acc`
wherever it stores an fp32 accumulator (the pre-activations, r, the logits, the criterion's gradient, the masked gradient).
acc = np.float64 makes the step a smooth float64 function of its parameters, which is what the finite differences need."""
import numpy as np

from oracle.ref_numpy import log_softmax as _log_softmax32
from tests import _gauss_np, _labels_np
from vbnn_amd import partition

F8 = np.float64


def _ident(a):
    return a


def _log_softmax(z, acc):
    if acc is np.float32:
        return _log_softmax32(z)                              # emulate_lrt_step's own, rounding for rounding
    mx = z.max(axis=1, keepdims=True)
    return z - (mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True)))


def criterion(kind, logits, t, inv_n, acc=np.float32, logvar_clamp=(-20.0, 20.0)):
    """(loss, hits, g) of one draw on the stored logits (N x C, dtype acc). inv_n = 1 / (global rows); the regression and label
    criteria divide by their D as the engine does (inv_n / D as an fp32 argument of the criterion kernel)."""
    N, Cn = logits.shape
    if kind == "nll":
        out = _log_softmax(logits, acc)
        rows = np.arange(N)
        loss = float(-out[rows, t].sum() * inv_n)
        onehot = np.zeros_like(out)
        onehot[rows, t] = 1.0
        g = ((np.exp(out) - onehot) * acc(inv_n)).astype(acc)
        return loss, int((logits.argmax(axis=1) == t).sum()), g          # (argmax: the first of equal maxima, as the kernels)
    if kind == "mse":
        diff = logits.astype(F8) - t.astype(F8)
        loss = float((diff * diff).sum() * inv_n / Cn)
        g = (2.0 * (logits - t.astype(acc)) * acc(inv_n / Cn)).astype(acc)
        return loss, 0, g
    if kind == "gauss":
        D = Cn // 2
        ref = _gauss_np.criterion64(logits, t, inv_n / D, *logvar_clamp)
        return float(ref["loss"]), 0, np.concatenate([ref["g_m"], ref["g_s"]], axis=1).astype(acc)
    if kind == "bce":
        ref = _labels_np.criterion64(logits, t, inv_n / Cn)
        return float(ref["loss"]), ref["hits"], ref["g"].astype(acc)
    raise ValueError(kind)


def forward(layers, w3, b3, x, zetas, rnd=_ident, acc=np.float32):
    """One draw's forward: the stored operands xs / x2s, the stored residuals rs, and the stored logits."""
    xs, x2s, rs = [rnd(x).astype(F8)], [rnd(rnd(x) * rnd(x)).astype(F8)], []
    for lay, z in zip(layers, zetas):
        mu, var = rnd(lay["means"]).astype(F8), rnd(np.exp(lay["lvars"])).astype(F8)
        m = xs[-1] @ mu.T + lay["bias"].astype(F8)
        v = x2s[-1] @ var.T
        y = (m + np.sqrt(v) * z).astype(acc)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(v > 0, z / (2 * np.sqrt(v)), 0.0).astype(acc)
        h = rnd(np.maximum(y, 0))
        rs.append(rnd(r))
        xs.append(h.astype(F8))
        x2s.append(rnd(h * h).astype(F8))
    logits = (xs[-1] @ rnd(w3).astype(F8).T + b3).astype(acc)
    return xs, x2s, rs, logits


def kl_cost(layers, B):
    """sum over the VB layers of LC = sum_w 0.5 log(var_hat / sigma^2) + (mu^2 + sigma^2 - var_hat) / (2 var_hat), over B
    (var_hat = mean(sigma^2 + mu^2), its stationary point: the partial and the total derivative agree)."""
    lc = 0.0
    for lay in layers:
        v, q = np.exp(lay["lvars"].astype(F8)), lay["means"].astype(F8) ** 2
        vh = (v + q).mean()
        lc += float(((0.5 * np.log(vh) - 0.5 * np.log(v)) + (q + v - vh) / (2 * vh)).sum() / B)
    return lc


def step(layers, w3, b3, x, t, zetas, criterion_kind="nll", rnd=_ident, B=1e6, kl_shadows=False, kl_scale=1.0, inv_n=None,
         acc=np.float32, logvar_clamp=(-20.0, 20.0)):
    """S = len(zetas) draws of one minibatch accumulating, as resetGradients(); S x { sample(); run(x, t) } leaves them.
    layers: dicts(means, lvars, bias); zetas[s][k]: draw s's N x O_k normals of layer k (oracle.fill_normal, the zeta stream).
    kl_shadows / kl_scale: emulate_lrt_step's (vbnn_dw_args.mu_s / var_s, vbnn_dw_args.kl_scale).
    Returns dict(loss = the draws' losses summed, hits = their hit counts summed, regions = {name: float64 array} with the names
    of region_names(), logits = [S] float64 N x C, objective = loss / S + KL cost: what `regions` differentiates -- d/dmeans
    and d/dlvars are its total derivatives, the bias and final Linear gradients S times theirs)."""
    S = len(zetas)
    N = x.shape[0]
    inv_n = 1.0 / N if inv_n is None else inv_n
    nl = len(layers)
    gw = [0.0] * nl
    gs2 = [0.0] * nl
    gb = [0.0] * nl
    gw3 = gb3 = 0.0
    loss, hits, all_logits = 0.0, 0, []
    for zs in zetas:
        xs, x2s, rs, logits = forward(layers, w3, b3, x, zs, rnd, acc)
        all_logits.append(logits.astype(F8))
        l, h, g3 = criterion(criterion_kind, logits, t, inv_n, acc, logvar_clamp)
        loss += l
        hits += h
        g3r = rnd(g3).astype(F8)
        gw3 = gw3 + g3r.T @ xs[-1]
        gb3 = gb3 + g3.astype(F8).sum(axis=0)
        gx = g3r @ rnd(w3).astype(F8)
        for k in range(nl - 1, -1, -1):
            lay = layers[k]
            gp = np.where(xs[k + 1] > 0, gx, 0.0).astype(acc)          # the ReLU mask on the stored activation
            g = rnd(gp).astype(F8)
            gv = rnd(gp * rs[k]).astype(F8)
            gw[k] = gw[k] + g.T @ xs[k]
            gs2[k] = gs2[k] + gv.T @ x2s[k]
            gb[k] = gb[k] + g.sum(axis=0)
            if k > 0:
                mu, var = rnd(lay["means"]).astype(F8), rnd(np.exp(lay["lvars"])).astype(F8)
                gx = g @ mu + 2 * xs[k] * (gv @ var)
    regions = {}
    for k, lay in enumerate(layers):
        var32 = np.exp(lay["lvars"])
        vh = float(np.sum(var32.astype(F8) + lay["means"].astype(F8) ** 2) / lay["means"].size)
        mu_e = rnd(lay["means"]).astype(F8) if kl_shadows else lay["means"].astype(F8)
        var_e = rnd(var32).astype(F8) if kl_shadows else var32.astype(F8)
        regions[f"{k}.lv"] = gs2[k] * var_e / S + kl_scale * (var_e / vh - 1.0) / (2 * B)
        regions[f"{k}.mu"] = gw[k] / S + kl_scale * mu_e / (B * vh)
        regions[f"{k}.bias"] = gb[k]
    regions["final.weight"], regions["final.bias"] = gw3, gb3
    return dict(loss=loss, hits=hits, regions=regions, logits=all_logits, objective=loss / S + kl_scale * kl_cost(layers, B))


def region_names(n_layers):
    return [f"{k}.{part}" for k in range(n_layers) for part in ("lv", "mu", "bias")] + ["final.weight", "final.bias"]


def arena_regions(arena, sizes, n_classes):
    """A flat gradient arena (NumPy) cut into step()'s regions by partition.arena_layout."""
    lay, fin, total, _ = partition.arena_layout(sizes, n_classes)
    assert arena.size == total
    out = {}
    for k, d in enumerate(lay):
        for part in ("lv", "mu"):
            out[f"{k}.{part}"] = arena[d[part][0]:d[part][0] + d[part][1]].reshape(d["O"], d["I"])
        out[f"{k}.bias"] = arena[d["bias"][0]:d["bias"][0] + d["bias"][1]]
    out["final.weight"] = arena[fin["weight"][0]:fin["weight"][0] + fin["weight"][1]].reshape(n_classes, sizes[-1])
    out["final.bias"] = arena[fin["bias"][0]:fin["bias"][0] + fin["bias"][1]]
    return out


# ------------------------------------------------------------------------------------------------ the step matrix's cases
SEED = 3
STREAM_ZETA, STREAM_DATA, STREAM_HEINIT = 2, 4, 5            # oracle.vbnn_oracle's stream ids
HEADS = {                       # name: (criterion, n_classes)
    "nll10": ("nll", 10),       # the fused head: the control
    "nll20": ("nll", 20),
    "mse24": ("mse", 24),
    "gauss12": ("gauss", 12),
    "bce5": ("bce", 5),
}
TIERS = {                       # name: (dtype, input size, hidden, rows, sequential draws)
    "small-f32": ("f32", 70, [50, 34], 37, 2),
    "small-bf16": ("bf16", 256, [512, 256], 512, 2),
}
# (tier, head): the seed of the case's random parameters and targets, chosen on the CPU so that margins() holds
CASE_SEEDS = {                  # (the first seed from 9 up that holds them; small-f32: for three draws, its stacked cases' count)
    ("small-f32", "nll20"): 10,
    ("small-bf16", "nll10"): 238,
    ("small-bf16", "nll20"): 1849,
    ("small-bf16", "bce5"): 49,
}


def engine_opt(tier, head, **over):
    dtype, I0, hidden, _, S = TIERS[tier]
    crit, Cn = HEADS[head]
    o = dict(var_init=1e-3, mu_init=1, B=1e6, S=S, mode="lrt", dtype=dtype, seed=SEED, keep_e=True, input_size=I0,
             hidden=list(hidden), n_classes=Cn, criterion=crit, type="vb", testSamples=2, fuse_kl=True)
    o.update(over)
    return o


def make_case(oracle, tier, head, draws=None, seed=None):
    """The NumPy side of one (tier, head) cell: He-rule means and final weight from the library's own streams, lvars
    randomised as test_engine_regression_head_matches_oracle_f32 does, small random biases, the input from fill_normal, the
    targets as the head's family tests make them, and the zeta normals of `draws` draws (default: the tier's)."""
    dtype, I0, hidden, N, S = TIERS[tier]
    crit, Cn = HEADS[head]
    S = draws or S
    seed = CASE_SEEDS.get((tier, head), 9) if seed is None else seed
    rng = np.random.default_rng(seed)
    sizes = [I0] + list(hidden)
    layers = []
    for k in range(len(hidden)):
        I, O = sizes[k], sizes[k + 1]
        layers.append(dict(means=oracle.fill_normal(O, I, SEED, STREAM_HEINIT, k, 0) * np.float32(np.sqrt(2.0 / I)),
                           lvars=rng.normal(np.log(1e-3), 0.3, (O, I)).astype(np.float32),
                           bias=rng.normal(0, 0.1, O).astype(np.float32)))
    H = sizes[-1]
    w3 = oracle.fill_normal(Cn, H, SEED, STREAM_HEINIT, len(hidden), 0) * np.float32(np.sqrt(2.0 / H))
    b3 = rng.normal(0, 0.1, Cn).astype(np.float32)
    if crit == "bce":
        # one logit in a thousand lies within 1e-3 max|z| of 0 when the logits are centred there, and a tier has thousands: the
        # labels' logits get offsets of two of their standard deviations, either sign (margins() still has to hold)
        b3 = (np.where(np.arange(Cn) % 2 == 0, 2.0, -2.0) * np.sqrt(2.0)).astype(np.float32)
    x = oracle.fill_normal(N, I0, SEED, STREAM_DATA, 0, 0)
    if crit == "nll":
        t = (np.arange(N) * 7 % Cn).astype(np.int32)
    elif crit == "bce":
        t = (rng.random((N, Cn)) < 0.4).astype(np.float32)
    else:
        t = rng.normal(0, 1, (N, Cn // 2 if crit == "gauss" else Cn)).astype(np.float32)
    zetas = [[oracle.fill_normal(N, sizes[k + 1], SEED, STREAM_ZETA, k, s + 1, 0).astype(F8) for k in range(len(hidden))]
             for s in range(S)]
    return dict(tier=tier, head=head, dtype=dtype, criterion=crit, n_classes=Cn, sizes=sizes, N=N, S=S, layers=layers, w3=w3,
                b3=b3, x=x, t=t, zetas=zetas, seed=seed)


def reference(case, kl_shadows=False, kl_scale=1.0, B=1e6):
    from oracle.ref_numpy import bf16_round
    rnd = bf16_round if case["dtype"] == "bf16" else _ident
    return step(case["layers"], case["w3"], case["b3"], case["x"], case["t"], case["zetas"], case["criterion"], rnd, B=B,
                kl_shadows=kl_shadows, kl_scale=kl_scale)


def margins(case, ref, logvar_clamp=(-20.0, 20.0)):
    """What makes the hit count and the clamp's slope immune to rounding, in the float64 reference's logits: no `bce` logit
    within 1e-3 max|z| of 0, no top-two gap of an `nll` row below 1e-3 max|z|, no `gauss` s within 1 of the clamp.
    Returns (holds, the margin in use, the margin required)."""
    z = np.stack(ref["logits"])
    top = float(np.abs(z).max())
    if case["criterion"] == "bce":
        return bool(np.abs(z).min() >= 1e-3 * top), float(np.abs(z).min()), 1e-3 * top
    if case["criterion"] == "nll":
        srt = np.sort(z, axis=-1)
        gap = float((srt[..., -1] - srt[..., -2]).min())
        return bool(gap >= 1e-3 * top), gap, 1e-3 * top
    if case["criterion"] == "gauss":
        s = z[..., case["n_classes"] // 2:]
        room = float(min((s - logvar_clamp[0]).min(), (logvar_clamp[1] - s).min()))
        return bool(room >= 1.0), room, 1.0
    return True, float("inf"), 0.0
