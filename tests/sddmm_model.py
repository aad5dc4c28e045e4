"""The definition of mspmv_sddmm_* (include/mspmv.h) in numpy: for every stored entry e of a CSR pattern, in row r and column c,

    s = +0.0;  for t = 0 .. k-1:  s = s + U[r, t] * V[c, t]          (left to right)
    C[e] = alpha * s + (beta == 0 ? +0.0 : beta * C[e])

in the compute dtype, one vectorised multiply and one vectorised add per t: numpy rounds each on its own (no fused multiply-add)
and flushes nothing.  bf16 inputs are uint16 arrays holding the upper half of an fp32; they are widened by a bit shift first."""
import numpy as np


def widen_bf16(a):
    """uint16 (the upper 16 bits of an fp32) -> float32, exactly"""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow_bf16(a):
    """float32 -> uint16 by truncation (test inputs only: the values the tests use are made representable first)"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def entry_rows(row_offsets, nnz):
    """the row of every stored entry"""
    off = np.asarray(row_offsets, dtype=np.int64)
    return np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))[:nnz]


def sddmm_model(row_offsets, column_indices, U, V, alpha=1.0, beta=0.0, C=None, dtype=None):
    """U: [rows, k], V: [cols, k] (uint16 = bf16, widened to float32).  Returns the nnz values in the compute dtype."""
    if U.dtype == np.uint16:
        U, V = widen_bf16(U).reshape(U.shape), widen_bf16(V).reshape(V.shape)
    dtype = np.dtype(dtype or U.dtype)
    assert U.dtype == dtype and V.dtype == dtype
    cols = np.asarray(column_indices, dtype=np.int64)
    rows = entry_rows(row_offsets, cols.size)
    assert rows.size == cols.size
    k = U.shape[1]
    t = dtype.type
    with np.errstate(all="ignore"):
        s = np.zeros(cols.size, dtype=dtype)
        for j in range(k):
            p = U[rows, j] * V[cols, j]
            s = s + p
        a = t(alpha) * s
        if t(beta) == 0:
            b = np.zeros(cols.size, dtype=dtype)
        else:
            b = t(beta) * np.asarray(C, dtype=dtype)
        out = a + b
    assert out.dtype == dtype
    return out
