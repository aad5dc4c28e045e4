"""numpy model of IC(0) as include/mspmv.h defines it (mspmv_csric0_*): the row-wise incomplete Cholesky on the pattern of A's lower
triangle, every divide, multiply, subtract and root rounded on its own in the value type (plain numpy scalar arithmetic), rows in
ascending order (a dependency order).  Rows are sorted by column with no column twice.  Nothing here calls the library."""
import numpy as np


def ic0(off, col, val, mirror=False):
    """(l_values, pivot): for row i, for every stored entry e with j = col[e] < i in stored order: a[e] = a[e] / piv(j), piv(j) the
    final (rooted) diagonal of row j (+0.0 if row j stores none); for every stored g of row i behind e with k = col[g], j < k < i,
    for which row k stores column j at f: a[g] = a[g] - a[e] * a[f]; the diagonal, if stored: a[d] = a[d] - a[e] * a[e].  Then
    a[d] = sqrt(a[d]).  pivot: the smallest row whose diagonal is missing or whose value under the root compares <= 0, else -1.
    Entries behind the diagonal: unchanged, or with `mirror` the final entry (j, i) of L (+0.0 if row j does not store column i)."""
    dtype = val.dtype.type
    rows = len(off) - 1
    a = val.copy()
    where = [{int(col[e]): e for e in range(off[r], off[r + 1])} for r in range(rows)]
    pivot = -1
    with np.errstate(all="ignore"):
        for i in range(rows):
            for e in range(off[i], off[i + 1]):
                j = int(col[e])
                if j >= i:
                    break
                piv = a[where[j][j]] if j in where[j] else dtype(0.0)
                a[e] = dtype(a[e] / piv)
                for g in range(e + 1, off[i + 1]):
                    k = int(col[g])
                    if k > i:
                        break
                    if k == i:
                        p = dtype(a[e] * a[e])
                        a[g] = dtype(a[g] - p)
                    elif j in where[k]:
                        p = dtype(a[e] * a[where[k][j]])
                        a[g] = dtype(a[g] - p)
            if i in where[i]:
                d = where[i][i]
                if a[d] <= 0 and pivot < 0:
                    pivot = i
                a[d] = dtype(np.sqrt(a[d]))
            elif pivot < 0:
                pivot = i
        if mirror:
            for i in range(rows):
                for g in range(off[i], off[i + 1]):
                    j = int(col[g])
                    if j > i:
                        a[g] = a[where[j][i]] if i in where[j] else dtype(0.0)
    return a, pivot


def group(rows, nnz):
    """G as the header states it: the smallest power of two >= ceil((nnz + rows) / (2 rows)), the mean length of a row's
    lower-plus-diagonal part under a symmetric pattern, within [1, 64]"""
    if rows <= 0:
        return 1
    mean = -(-(nnz + rows) // (2 * rows))
    g = 1
    while g < 64 and g < mean:
        g *= 2
    return g
