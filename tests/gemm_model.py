"""Host restatements of C = A * B for two CSR matrices (include/mspmv.h: mspmv_csr_gemm_*) for tests/test_csr_gemm.py.  A matrix is (row_offsets, column_indices, values or None); any valid CSR: rows need not be
sorted and a column may repeat.

gemm_by_rows is THE model: per row of A, walk its entries in order, walk the row of B in order, append t(a) * t(b) to a list keyed
by the column, add each list left to right in the value type, emit the columns sorted.  host_gemm is the same computation in numpy
(expand in that order, stable sort by (row, column), add every run left to right) for the sizes the GPU tests use; the tests pin it
to gemm_by_rows, and gemm_by_rows to hand-written cases."""
import numpy as np


def count_products(a, b):
    """the number of scalar products: the sum over A's entries of the length of B's row"""
    lens = np.diff(np.asarray(b[0], np.int64))
    return int(lens[np.asarray(a[1], np.int64)].sum()) if len(a[1]) else 0


def gemm_by_rows(rows, a, b, dtype=None):
    (oa, ca, va), (ob, cb, vb) = a, b
    t = None if va is None else np.dtype(dtype).type
    off, col, val = [0], [], []
    for r in range(rows):
        lists = {}
        for e in range(oa[r], oa[r + 1]):
            k = int(ca[e])
            for j in range(ob[k], ob[k + 1]):
                lists.setdefault(int(cb[j]), []).append(None if t is None else t(va[e]) * t(vb[j]))
        for c in sorted(lists):
            col.append(c)
            if t is not None:
                s = lists[c][0]                                  # the first product starts the sum
                for p in lists[c][1:]:
                    s = t(s + p)
                val.append(s)
        off.append(len(col))
    return (np.asarray(off, np.int32), np.asarray(col, np.int32).reshape(-1),
            None if t is None else np.asarray(val, dtype).reshape(-1))


def host_gemm(rows, cols, a, b, dtype=None):
    (oa, ca, va), (ob, cb, vb) = a, b
    oa, ca, ob, cb = (np.asarray(x, np.int64) for x in (oa, ca, ob, cb))
    lens = np.diff(ob)[ca] if len(ca) else np.zeros(0, np.int64)
    n = int(lens.sum())
    start = np.zeros(len(ca) + 1, np.int64)
    np.cumsum(lens, out=start[1:])
    e = np.repeat(np.arange(len(ca), dtype=np.int64), lens)      # A's entry of every product, in expansion order
    j = ob[ca][e] + (np.arange(n, dtype=np.int64) - start[e]) if n else np.zeros(0, np.int64)
    row = np.repeat(np.repeat(np.arange(rows, dtype=np.int64), np.diff(oa)), lens)
    key = row * max(cols, 1) + (cb[j] if n else np.zeros(0, np.int64))
    order = np.argsort(key, kind="stable")
    key = key[order]
    head = np.ones(n, bool)
    head[1:] = key[1:] != key[:-1]
    heads = np.flatnonzero(head)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(key[heads] // max(cols, 1), minlength=rows), out=off[1:])
    col = (key[heads] % max(cols, 1)).astype(np.int32)
    if va is None:
        return off.astype(np.int32), col, None
    prod = (np.asarray(va, dtype)[e] * np.asarray(vb, dtype)[j])[order]          # each product rounded on its own
    run_len = np.diff(np.append(heads, n))
    val = prod[heads].copy()
    for k in range(1, int(run_len.max()) if n else 0):           # left to right: the k-th product of every run that has one
        live = np.flatnonzero(run_len > k)
        val[live] = val[live] + prod[heads[live] + k]
    return off.astype(np.int32), col, val.astype(dtype)
