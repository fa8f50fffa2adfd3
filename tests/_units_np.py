"""A float64 / NumPy restatement of structured (unit-level) signal-to-noise pruning, for the tests of vbnn_unit_* and of
FusedMLP.prune_units / compact: the key of a unit, the exact k-th order statistic over keys, the kept-set rule (threshold, the
`multiple` rounding, ties, NaN, the layer that would lose everything) and the compaction of a network by fancy indexing."""
import numpy as np

NAN_BITS = np.uint32(0x7fc00000)


def unit_key64(means, lvars):
    """||mu_o||_2 / ||sigma_o||_2 per output row, in float64 (0 / 0 and NaN parameters give NaN)."""
    m, l = np.asarray(means, np.float64), np.asarray(lvars, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt((m * m).sum(1)) / np.sqrt(np.exp(l).sum(1))


def code(keys):
    """The total order of the fp32 keys as integers: non-negative floats order as their bits, every NaN above +inf."""
    k = np.ascontiguousarray(np.asarray(keys, np.float32))
    return np.where(np.isnan(k), NAN_BITS, k.view(np.uint32)).astype(np.uint32)


def kth(keys, k):
    """The k-th smallest (0-based) of the fp32 keys in that order, as a float32 scalar (the canonical NaN if it is one)."""
    c = code(np.asarray(keys, np.float32).ravel())
    assert 0 <= k < c.size
    return np.partition(c, k)[k:k + 1].view(np.float32)[0]


def kept(keys, tau, multiple=1):
    """The kept units of one layer, ascending: n0 = #{!(key < tau)}, n = min(O, m ceil(max(n0, 1) / m)), the first n units in
    the order (larger key first, NaN above all numbers, the lower index first on equal keys)."""
    keys = np.asarray(keys, np.float32)
    O, m = keys.size, int(multiple)
    assert m >= 1 and O >= 1
    with np.errstate(invalid="ignore"):
        n0 = int((~(keys < np.float32(tau))).sum())
    n = min(O, m * -(-max(n0, 1) // m))
    order = np.argsort(-code(keys).astype(np.int64), kind="stable")           # stable: equal keys stay in index order
    return np.sort(order[:n]).astype(np.uint32)


def prune_units(keys, fraction=None, threshold=None, scope="global", multiple=1):
    """keys: one fp32 array per layer. Returns (tau per layer as float32, kept list per layer), as FusedMLP.prune_units."""
    assert (fraction is None) != (threshold is None)
    nl = len(keys)
    groups = [list(range(nl))] if scope == "global" else [[li] for li in range(nl)]
    tau = [np.float32(threshold if threshold is not None else np.inf)] * nl
    for g in groups:
        pool = np.concatenate([np.asarray(keys[li], np.float32) for li in g])
        k = int(np.floor(float(fraction) * pool.size)) if fraction is not None else pool.size
        if k < pool.size:
            for li in g:
                tau[li] = kth(pool, k)
    return tau, [kept(keys[li], tau[li], multiple) for li in range(nl)]


def compact(layers, weight3, keep):
    """layers: (means, lvars, bias) per VB layer; keep: the kept list per layer. The compact network's parameters: a layer's
    rows by its own list, its columns by the previous layer's (the first layer keeps every input); weight3 by columns."""
    out, cols = [], None
    for (means, lvars, bias), rows in zip(layers, keep):
        rows = np.asarray(rows, np.int64)
        sel = (lambda a: a[rows]) if cols is None else (lambda a: a[rows][:, cols])
        out.append((sel(np.asarray(means)), sel(np.asarray(lvars)), np.asarray(bias)[rows]))
        cols = rows
    return out, np.asarray(weight3)[:, cols]


def n_weights(sizes, n_classes):
    return sum(sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1)) + sizes[-1] * n_classes
