"""numpy model of the level-scheduled triangular solve (include/mspmv.h: mspmv_csrsv_*): the levels, the order, the level offsets,
the segments (launches) given W, the figures of the plan, and the solve with every operation rounded on its own in the value type
(plain numpy scalar arithmetic, row by row).  Nothing here calls the library."""
import numpy as np


def in_triangle(r, c, lower):
    return c < r if lower else c > r


def levels(off, col, lower=True):
    """level[r] = 0 for a row without strict-triangle entries, else 1 + max(level[c]) over them"""
    rows = len(off) - 1
    level = np.zeros(rows, np.int64)
    for r in (range(rows) if lower else range(rows - 1, -1, -1)):
        deps = [int(c) for c in col[off[r]:off[r + 1]] if in_triangle(r, int(c), lower)]
        level[r] = 1 + max(int(level[c]) for c in deps) if deps else 0
    return level


def schedule(level):
    """(order, level_offsets): the rows sorted stably by level (ascending row inside a level), and where each level starts"""
    rows = len(level)
    order = np.argsort(level, kind="stable").astype(np.int32)
    n = int(level.max()) + 1 if rows else 0
    lo = np.zeros(n + 1, np.int32)
    if rows:
        np.cumsum(np.bincount(level, minlength=n), out=lo[1:])
    return order, lo


def segments(level_offsets, W):
    """[(first level, one past the last, narrow)]: a maximal run of levels of at most W rows is one launch, every other level its own"""
    sizes = np.diff(np.asarray(level_offsets, np.int64))
    out, l = [], 0
    while l < len(sizes):
        if sizes[l] <= W:
            m = l
            while m < len(sizes) and sizes[m] <= W:
                m += 1
            out.append((l, m, True))
            l = m
        else:
            out.append((l, l + 1, False))
            l += 1
    return out


def bad_diagonal_row(off, col, unit=False):
    """NON_UNIT: the smallest row with no or more than one stored diagonal entry, else -1"""
    if unit:
        return -1
    for r in range(len(off) - 1):
        if sum(1 for c in col[off[r]:off[r + 1]] if int(c) == r) != 1:
            return r
    return -1


def used_entries(off, col, lower=True):
    return sum(1 for r in range(len(off) - 1) for c in col[off[r]:off[r + 1]] if in_triangle(r, int(c), lower))


def plan_info(off, col, lower, unit, W):
    rows = len(off) - 1
    order, lo = schedule(levels(off, col, lower))
    return dict(rows=rows, nnz=len(col), uplo=0 if lower else 1, diag=1 if unit else 0, levels=len(lo) - 1,
                launches=len(segments(lo, W)), narrow_rows=W, max_level_rows=int(np.diff(lo).max()) if rows else 0,
                bad_diagonal_row=bad_diagonal_row(off, col, unit), used_entries=used_entries(off, col, lower)), order, lo


def solve(off, col, val, b, alpha=1.0, lower=True, unit=False):
    """s = +0; s = s + a[e] * x[c] over the row's strict-triangle entries in stored order; t = alpha * b[r];
    x[r] = (t - s) / d (d = the row's stored diagonal) or t - s (unit): every operation rounded in b's dtype"""
    dtype = b.dtype.type
    rows = len(off) - 1
    x = np.zeros(rows, dtype)
    alpha = dtype(alpha)
    with np.errstate(all="ignore"):
        for r in (range(rows) if lower else range(rows - 1, -1, -1)):
            s, d = dtype(0.0), dtype(1.0)
            for e in range(off[r], off[r + 1]):
                c = int(col[e])
                if in_triangle(r, c, lower):
                    p = dtype(val[e]) * x[c]
                    s = dtype(s + p)
                elif c == r:
                    d = dtype(val[e])
            t = dtype(alpha * dtype(b[r]))
            v = dtype(t - s)
            x[r] = v if unit else dtype(v / d)
    return x
