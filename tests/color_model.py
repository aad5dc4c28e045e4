"""numpy model of the multicolour ordering (include/mspmv.h: mspmv_csr_color_*, mspmv_csr_permute_*), stating the definitions
literally: fmix32 and the key, greedy colouring in descending key order over the symmetrised neighbour sets, the order, its inverse
and the colour offsets, and the permutation of a CSR as a stable sort of its triples.  Nothing here calls the library."""
import numpy as np


def fmix32(v):
    """the 32-bit finaliser: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 (mod 2^32)"""
    h = np.asarray(v, np.uint64) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h


def keys(rows, priorities=None):
    """key(v) = prio(v) << 32 | v, prio(v) = priorities[v] (its 32 bits read as unsigned) or fmix32(v)"""
    v = np.arange(rows, dtype=np.uint64)
    prio = fmix32(v) if priorities is None else np.asarray(priorities).astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)
    return (prio << np.uint64(32)) | v


def neighbours(off, col):
    """the symmetrised neighbour sets: u in N(v) when u != v and A[u,v] or A[v,u] is stored"""
    rows = len(off) - 1
    nb = [set() for _ in range(rows)]
    for r in range(rows):
        for c in col[off[r]:off[r + 1]]:
            c = int(c)
            if c != r:
                nb[r].add(c)
                nb[c].add(r)
    return nb


def edges(off, col):
    """stored off-diagonal entries, duplicates counted"""
    return sum(1 for r in range(len(off) - 1) for c in col[off[r]:off[r + 1]] if int(c) != r)


def colors(off, col, priorities=None):
    """color[v] = the smallest non-negative integer that no neighbour of larger key holds: greedy, in descending key order"""
    rows = len(off) - 1
    key = keys(rows, priorities)
    nb = neighbours(off, col)
    color = np.full(rows, -1, np.int32)
    for v in np.argsort(key)[::-1]:                               # (keys are distinct: the low word is the vertex)
        taken = {int(color[u]) for u in nb[v] if key[u] > key[v]}
        c = 0
        while c in taken:
            c += 1
        color[v] = c
    return color


def schedule(color):
    """(order, inverse, offsets): the vertices sorted stably by colour, inverse[order[i]] = i, colours + 1 offsets"""
    rows = len(color)
    order = np.argsort(color, kind="stable").astype(np.int32)
    inverse = np.empty(rows, np.int32)
    inverse[order] = np.arange(rows, dtype=np.int32)
    n = int(color.max()) + 1 if rows else 0
    offsets = np.zeros(n + 1, np.int32)
    if rows:
        np.cumsum(np.bincount(color, minlength=n), out=offsets[1:])
    return order, inverse, offsets


def coloring(off, col, priorities=None):
    color = colors(off, col, priorities)
    order, inverse, offsets = schedule(color)
    rows = len(off) - 1
    return dict(colors=color, order=order, inverse=inverse, offsets=offsets, num_colors=len(offsets) - 1,
                max_color_rows=int(np.diff(offsets).max()) if rows else 0, edges=edges(off, col))


def permute(off, col, val, cols, row_perm=None, col_map=None):
    """(off_b, col_b, val_b, permutation): the triples (inverse_row(r), col_map[c], v) in A's stored order, sorted stably by (new row,
    new column); B entry j is A entry permutation[j] and its value is moved as it is"""
    rows, nnz = len(off) - 1, len(col)
    row_perm = np.arange(rows) if row_perm is None else np.asarray(row_perm, np.int64)
    col_map = np.arange(cols) if col_map is None else np.asarray(col_map, np.int64)
    inv = np.empty(rows, np.int64)
    inv[row_perm] = np.arange(rows)
    new_row = inv[np.repeat(np.arange(rows), np.diff(off))] if nnz else np.zeros(0, np.int64)
    new_col = col_map[np.asarray(col, np.int64)] if nnz else np.zeros(0, np.int64)
    perm = np.argsort(new_row * max(cols, 1) + new_col, kind="stable").astype(np.int32)
    off_b = np.zeros(rows + 1, np.int32)
    if rows:
        np.cumsum(np.bincount(new_row, minlength=rows), out=off_b[1:])
    return off_b, new_col[perm].astype(np.int32), (None if val is None else np.asarray(val)[perm]), perm
