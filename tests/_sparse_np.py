"""Float64 / NumPy restatements of the compressed pruned form (include/vbnn_hip.h: vbnn_sparse_desc) and of the forward on it
(vbnn_forward_sparse) -- test infrastructure for tests/test_sparse_abi.py and tests/test_sparse_gpu.py.

The format: per layer CSR over output rows. An entry is a KEPT weight, kept = not (key < tau) -- so a NaN key is kept, a key equal
to tau is kept -- columns ascend within a row, a kept weight whose value is zero is still an entry."""
import numpy as np


def csr_build(keys, tau, mu, var=None):
    """keys, mu, var: O x I arrays (values of any dtype: they are copied, not converted). Returns dict(row_ptr uint32 O + 1,
    cols int64 nnz, mu_v, var_v (or None), nnz)."""
    keys = np.asarray(keys)
    with np.errstate(invalid="ignore"):
        kept = ~(keys < np.float32(tau))
    counts = kept.sum(1)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    rows, cols = np.nonzero(kept)                                   # row-major: columns ascend within a row
    return dict(row_ptr=row_ptr, cols=cols.astype(np.int64), mu_v=np.asarray(mu)[rows, cols],
                var_v=None if var is None else np.asarray(var)[rows, cols], nnz=int(counts.sum()))


def csr_check(csr, O, I):
    """The structural invariants of the format."""
    rp = csr["row_ptr"].astype(np.int64)
    assert rp.shape == (O + 1,) and rp[0] == 0 and rp[-1] == csr["nnz"] and np.all(np.diff(rp) >= 0)
    cols = csr["cols"][:csr["nnz"]]
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < I)
    inner = np.ones(max(cols.size - 1, 0), dtype=bool)
    starts = rp[1:-1]
    inner[starts[(starts > 0) & (starts < cols.size)] - 1] = False      # pairs that straddle a row boundary
    assert np.all(np.diff(cols)[inner] > 0), "columns do not ascend within a row"


def csr_to_dense(csr, O, I, ld=None, which="mu_v"):
    """The dense pruned shadow the entries stand for: O x ld (default I), zero (+0) wherever no entry is; dtype of the values."""
    vals = csr[which][:csr["nnz"]]
    rp = csr["row_ptr"].astype(np.int64)
    out = np.zeros((O, ld or I), dtype=vals.dtype)
    rows = np.repeat(np.arange(O), np.diff(rp))
    out[rows, csr["cols"][:csr["nnz"]]] = vals
    return out


def forward64(csr, O, x, x2=None, bias=None, z=None, relu=True):
    """vbnn_forward_sparse in float64, entry by entry: x, x2 (N x I; x2 None: x * x) are the operand VALUES the kernel reads,
    z (N x O) the noise; var_v None or z None: the MAP form. Returns (y, h, absprod) with absprod = sum |a b| of the terms of y --
    |x| |mu|^T + |b| + sqrt(v) |z|, the scale of the fp32 accumulation bound."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    x2 = x * x if x2 is None else np.asarray(x2, dtype=np.float64)
    rp = csr["row_ptr"].astype(np.int64)
    cols = csr["cols"]
    mu_v = np.asarray(csr["mu_v"], dtype=np.float64)
    lrt = csr["var_v"] is not None and z is not None
    var_v = np.asarray(csr["var_v"], dtype=np.float64) if lrt else None
    m, v, am = np.zeros((N, O)), np.zeros((N, O)), np.zeros((N, O))
    for o in range(O):
        s, e = rp[o], rp[o + 1]
        if e == s:
            continue
        c = cols[s:e]
        m[:, o] = x[:, c] @ mu_v[s:e]
        am[:, o] = np.abs(x[:, c]) @ np.abs(mu_v[s:e])
        if lrt:
            v[:, o] = x2[:, c] @ var_v[s:e]
    b = np.zeros(O) if bias is None else np.asarray(bias, dtype=np.float64)
    y = m + b
    absprod = am + np.abs(b)
    if lrt:
        y = y + np.sqrt(v) * z
        absprod = absprod + np.sqrt(v) * np.abs(z)
    return y, (np.maximum(y, 0.0) if relu else y), absprod
