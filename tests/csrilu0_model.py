"""numpy model of ILU(0) as include/mspmv.h defines it (mspmv_csrilu0_*): the row-wise elimination on A's own pattern, every divide,
multiply and subtract rounded on its own in the value type (plain numpy scalar arithmetic), rows in ascending order (a dependency
order).  Rows are sorted by column with no column twice.  Nothing here calls the library."""
import numpy as np


def ilu0(off, col, val):
    """(lu_values, pivot): for row i, for every stored entry e with k = col[e] < i in stored order: a[e] = a[e] / piv(k), piv(k) the
    final diagonal of row k (+0.0 if row k stores none); for every stored f of row k with j = col[f] > k that row i stores at g:
    a[g] = a[g] - a[e] * a[f].  pivot: the smallest row whose diagonal is missing or compares == 0, else -1."""
    dtype = val.dtype.type
    rows = len(off) - 1
    a = val.copy()
    diag = np.full(rows, -1, np.int64)
    for r in range(rows):
        for e in range(off[r], off[r + 1]):
            if int(col[e]) == r:
                diag[r] = e
    with np.errstate(all="ignore"):
        for i in range(rows):
            where = {int(col[g]): g for g in range(off[i], off[i + 1])}
            for e in range(off[i], off[i + 1]):
                k = int(col[e])
                if k >= i:
                    break
                piv = a[diag[k]] if diag[k] >= 0 else dtype(0.0)
                a[e] = dtype(a[e] / piv)
                for f in range(off[k], off[k + 1]):
                    j = int(col[f])
                    if j > k and j in where:
                        g = where[j]
                        p = dtype(a[e] * a[f])
                        a[g] = dtype(a[g] - p)
    pivot = -1
    for r in range(rows):
        if diag[r] < 0 or a[diag[r]] == 0:
            pivot = r
            break
    return a, pivot


def group(rows, nnz):
    """G as the header states it: the smallest power of two >= the mean row length (rounded up), within [1, 64]"""
    if rows <= 0:
        return 1
    mean = -(-nnz // rows)
    g = 1
    while g < 64 and g < mean:
        g *= 2
    return g
