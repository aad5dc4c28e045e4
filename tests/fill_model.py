"""Model of the level-of-fill pattern as include/mspmv_fill.h defines it (mspmv_csr_fill_*): the CLASSICAL row-by-row symbolic ILU(p),
in plain Python over numpy arrays.  Row i takes its entries k < i in ascending order, fill included, and merges row k's entries j > k
at level lev(i, k) + lev(k, j) + 1, keeping the minimum and dropping levels above p.  The device runs another algorithm (one levelled
product per level); two different algorithms agreeing is the point.  Also here: that product form restated as a fixed point
(`fill_product`), the patterns the tests share, and the scatter of values.  Nothing here calls the library."""
import heapq

import numpy as np


def fill(off, col, p):
    """(off, col, levels, source) of F_p: int32 arrays; source[e] = the entry's index in the given arrays, -1 for a fill entry"""
    rows = len(off) - 1
    lev_rows, src_rows = [], []              # per finished row: {column: level}, {column: source}
    upper = []                               # per finished row: its entries right of the diagonal, [(column, level)] ascending
    for i in range(rows):
        lev = {int(col[e]): 0 for e in range(off[i], off[i + 1])}
        src = {int(col[e]): e for e in range(off[i], off[i + 1])}
        todo = [k for k in lev if k < i]
        heapq.heapify(todo)
        done = set()
        while todo:
            k = heapq.heappop(todo)          # ascending; an entry entered while the row is worked is taken in its turn
            if k in done:
                continue
            done.add(k)
            for j, b in upper[k]:
                l = lev[k] + b + 1
                if l > p:
                    continue
                if j not in lev:
                    lev[j] = l
                    if j < i:
                        heapq.heappush(todo, j)
                elif l < lev[j]:
                    lev[j] = l               # (j > k: not worked yet, so its level is still free to fall)
        lev_rows.append(lev); src_rows.append(src)
        upper.append(sorted((j, l) for j, l in lev.items() if j > i))
    out_off = np.zeros(rows + 1, np.int32)
    out_col, out_lev, out_src = [], [], []
    for i in range(rows):
        for j in sorted(lev_rows[i]):
            out_col.append(j); out_lev.append(lev_rows[i][j]); out_src.append(src_rows[i].get(j, -1))
        out_off[i + 1] = len(out_col)
    return out_off, np.array(out_col, np.int32), np.array(out_lev, np.int32), np.array(out_src, np.int32)


def fill_product(off, col, p):
    """{(i, j): level} of F_p as the fixed point of the levelled product: S <- S u (strict lower part of S) x (strict upper part of S),
    a pair (i, m), (m, j) giving level a + b + 1, the minimum kept per position and levels above p dropped, until nothing changes"""
    rows = len(off) - 1
    s = {(i, int(col[e])): 0 for i in range(rows) for e in range(off[i], off[i + 1])}
    while True:
        by_row = {}
        for (m, j), b in s.items():
            if j > m:
                by_row.setdefault(m, []).append((j, b))
        new = dict(s)
        for (i, m), a in s.items():
            if m < i:
                for j, b in by_row.get(m, ()):
                    l = a + b + 1
                    if l <= p and l < new.get((i, j), p + 1):
                        new[(i, j)] = l
        if new == s:
            return s
        s = new


def as_dict(off, col, lev):
    return {(i, int(col[e])): int(lev[e]) for i in range(len(off) - 1) for e in range(off[i], off[i + 1])}


def scatter(values, source):
    """values of the given pattern moved into the filled one, +0.0 at fill entries"""
    out = np.zeros(len(source), values.dtype)
    keep = source >= 0
    out[keep] = values[source[keep]]
    return out


# ---- the patterns the tests share: (off, col) int32, canonical ---------------------------------------------------------------------
def from_pairs(n, pairs):
    pairs = sorted(set((int(i), int(j)) for i, j in pairs))
    off = np.zeros(n + 1, np.int32)
    for i, _ in pairs:
        off[i + 1] += 1
    return np.cumsum(off).astype(np.int32), np.array([j for _, j in pairs], np.int32)


def grid2d(w, h=None, order=None):
    """the 5-point stencil of a w x h grid with its diagonal; order: a permutation, new index -> old vertex"""
    h = w if h is None else h
    n = w * h
    new = np.arange(n) if order is None else np.argsort(np.asarray(order))
    pairs = []
    for y in range(h):
        for x in range(w):
            v = y * w + x
            for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < w and 0 <= y + dy < h:
                    pairs.append((new[v], new[(y + dy) * w + x + dx]))
    return from_pairs(n, pairs)


def red_black(w, h=None):
    """the order that numbers the red vertices (x + y even) of a w x h grid first, each colour in natural order"""
    h = w if h is None else h
    v = np.arange(w * h)
    return np.concatenate([v[(v % w + v // w) % 2 == 0], v[(v % w + v // w) % 2 == 1]])


def grid3d(w):
    n = w ** 3
    pairs = []
    for z in range(w):
        for y in range(w):
            for x in range(w):
                v = (z * w + y) * w + x
                pairs.append((v, v))
                for d, c in ((1, x), (w, y), (w * w, z)):
                    if c + 1 < w:
                        pairs += [(v, v + d), (v + d, v)]
    return from_pairs(n, pairs)


def cycle(n):
    return from_pairs(n, [(i, (i + d) % n) for i in range(n) for d in (-1, 0, 1)])


def arrow(n, first=True):
    """the diagonal and a dense first (or last) row and column"""
    hub = 0 if first else n - 1
    return from_pairs(n, [(i, i) for i in range(n)] + [(hub, i) for i in range(n)] + [(i, hub) for i in range(n)])


def diagonal(n):
    return from_pairs(n, [(i, i) for i in range(n)])


def empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32)


def random_pattern(rng, n, density, missing=0.15, symmetric=False):
    """a random pattern with most of its diagonal: each off-diagonal position stored with probability `density`, each diagonal with
    probability 1 - missing"""
    m = rng.random((n, n)) < density
    if symmetric:
        m = m | m.T
    np.fill_diagonal(m, rng.random(n) >= missing)
    return from_pairs(n, zip(*np.nonzero(m)))
