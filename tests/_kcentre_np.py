"""vbnn_kcentre restated in NumPy fp32 (include/vbnn_hip.h: DISTANCE, VOID, MINIMUM, CANDIDATES, KEY), operation by
operation: the summation order that depends on D alone, the key, the ties, the void rows and resume. The GPU tests hold the
kernel to this bit for bit; tests/test_kcentre_ref.py holds this to a plain float64 greedy."""
import numpy as np

QNAN = np.uint32(0x7fc00000).view(np.float32)
MAX_K, MAX_D = 4096, 8192


def block(D):
    """initial centres per pass over the features (the header's SHAPE; the result does not depend on it)"""
    return max(1, min(8, 32768 // (4 * ((D + 3) // 4))))


def threads(D):
    """the threads that share a row: a wave up to D = 1024, a workgroup of four waves above"""
    return 64 if D <= 1024 else 256


def row_sums(p):
    """The header's sum of the per-column terms p (n x D fp32, already rounded): T threads share a row, thread i adds the
    columns of quads i, i + T, ... in ascending order from +0; a wave's 64 partials by the xor butterfly; four waves as
    ((w0 + w1) + w2) + w3. Returns n fp32 sums."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    n, D = p.shape
    T = threads(D)
    nq = (D + 3) // 4
    per = (nq + T - 1) // T                                         # quads per thread
    pad = np.zeros((n, per * T * 4), dtype=np.float32)
    pad[:, :D] = p
    pad = pad.reshape(n, per, T, 4)
    acc = np.zeros((n, T), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(per):
            for e in range(4):
                acc = acc + pad[:, k, :, e]
        v = acc.reshape(n, T // 64, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lanes ^ off]
        w = v[:, :, 0]
        out = w[:, 0]
        for i in range(1, T // 64):
            out = out + w[:, i]
    return out.astype(np.float32)


def sq_norms(F):
    F = np.asarray(F, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return row_sums(F * F)


def sq_dists(F, c):
    """d(r, c) for every row r"""
    F = np.asarray(F, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = F - F[c][None, :]
        return row_sums(t * t)


def order_word(key):
    b = np.asarray(key, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xffffffff, b ^ 0x80000000).astype(np.uint64)


def keys_of(m, weight):
    """the key of every row from its minimum (void rows: whatever; the caller masks them)"""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if weight is None:
            key = m.copy()
        else:
            key = np.where(np.isinf(m), weight, (m * weight).astype(np.float32)).astype(np.float32)
    key[np.isnan(key)] = np.float32(0.0)
    return key


def kcentre(F, k, weight=None, exclude=None, centres=(), resume=False, min_dist=None):
    """Returns dict(index int32[k], key f32[k], dist f32[k], min_dist f32[R], counts [n_selected, n_candidates, n_void,
    n_excluded], ignored)."""
    F = np.asarray(F, dtype=np.float32)
    R, D = F.shape
    w = None if weight is None else np.asarray(weight, dtype=np.float32)
    ex = np.zeros(R, dtype=bool) if exclude is None else np.asarray(exclude) != 0
    if resume:
        m = np.array(min_dist, dtype=np.float32)
        void = np.isnan(m)
    else:
        void = ~np.isfinite(sq_norms(F))
        m = np.full(R, np.inf, dtype=np.float32)
    m[void] = QNAN
    w_void = np.zeros(R, dtype=bool) if w is None else (np.isnan(w) | (w < 0))
    standing = ex | void | w_void                                   # True: no candidate
    counts = [0, int((~standing).sum()), int((~ex & (void | w_void)).sum()), int(ex.sum())]
    ignored = 0

    def apply(c):
        nonlocal m
        d = sq_dists(F, c)
        live = ~void
        m = np.where(live & (d < m), d, m).astype(np.float32)

    for c in centres:
        c = int(c)
        if c < 0 or c >= R:
            ignored += 1
        elif not void[c]:
            apply(c)
    index = np.full(k, -1, dtype=np.int32)
    key = np.full(k, QNAN, dtype=np.float32)
    dist = np.full(k, QNAN, dtype=np.float32)
    for t in range(k):
        cand = np.nonzero(~standing)[0]
        if cand.size == 0:
            break
        kk = keys_of(m[cand], None if w is None else w[cand])
        ow = order_word(kk)
        best = cand[np.nonzero(ow == ow.max())[0][0]]              # ties: the lower row
        index[t], key[t], dist[t] = best, kk[np.nonzero(cand == best)[0][0]], m[best]
        standing[best] = True
        counts[0] += 1
        apply(best)
    return dict(index=index, key=key, dist=dist, min_dist=m, counts=counts, ignored=ignored)


def greedy64(F, k, weight=None, exclude=None, centres=()):
    """The plain float64 greedy the restatement is held to (finite features and weights >= 0 only): returns index, key, dist
    (float64), the final minimum and per step the gap between the best and the second-best key (inf with one candidate)."""
    F = np.asarray(F, dtype=np.float64)
    R = F.shape[0]
    w = None if weight is None else np.asarray(weight, dtype=np.float64)
    gone = np.zeros(R, dtype=bool) if exclude is None else (np.asarray(exclude) != 0).copy()
    m = np.full(R, np.inf)
    for c in centres:
        m = np.minimum(m, ((F - F[int(c)]) ** 2).sum(1))
    index, key, dist, gaps = [], [], [], []
    for _ in range(k):
        cand = np.nonzero(~gone)[0]
        if cand.size == 0:
            break
        mk = m[cand]
        with np.errstate(invalid="ignore"):
            kk = mk if w is None else np.where(np.isinf(mk), w[cand], mk * w[cand])
        srt = np.sort(kk)[::-1]
        best = cand[np.nonzero(kk == srt[0])[0][0]]
        gaps.append(srt[0] - srt[1] if srt.size > 1 and np.isfinite(srt[0]) else np.inf)
        index.append(best)
        key.append(srt[0])
        dist.append(m[best])
        gone[best] = True
        m = np.minimum(m, ((F - F[best]) ** 2).sum(1))
    return np.array(index), np.array(key), np.array(dist), m, np.array(gaps)
