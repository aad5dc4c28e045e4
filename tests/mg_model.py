"""A model of the partitioned (multi-GPU) CsrMV for tests/test_mg_model.py and tests/test_mg_exact.py (numpy only: no GPU, no library).

It restates include/mspmv.h (mspmv_mg_partition, mspmv_mg_local_offsets, mspmv_mg_apply_carries, mspmv_mg_plan_*):
  * the merge path of rows + nnz items is cut at `parts` equally spaced diagonals; part g owns the rows ENDING in its swath,
    [row_split[g], row_split[g+1]), and the nonzeros [nz_split[g], nz_split[g+1]);
  * seen locally a part is a CSR matrix of owned + 1 rows: its first row may be the tail of a row begun earlier, its extra LAST row
    is the open row cut by its right boundary, whose y is the part's carry for global row row_split[g+1];
  * a part that owns at least one row adds to its first entry the carries of the earlier parts j whose key row_split[j+1] equals
    row_split[g], in part order.  Parts that own nothing take nothing.
y of the whole operator = the single-GPU y of every part + that fold: fold() below, in the compute type, one rounding per add.
"""
from __future__ import annotations

import numpy as np

from axpby_model import Csr

PARTS = [1, 2, 3, 8, 64]


# ------------------------------------------------------------------------------------------------------------ the partition

def partition(off_i64, parts):
    """(row_split[parts+1], nz_split[parts+1]).  Diagonal d_g = min(ceil((rows+nnz)/parts) * g, rows+nnz); row i is consumed at
    diagonal d iff off[i+1] + i + 1 <= d (its nonzeros and its row end lie before d)."""
    off = np.asarray(off_i64, np.int64)
    rows = off.size - 1
    total = rows + int(off[-1])
    per = -(-total // int(parts))
    d = np.minimum(per * np.arange(parts + 1, dtype=np.int64), total)
    key = off[1:] + np.arange(1, rows + 1, dtype=np.int64)          # strictly increasing
    row_split = np.searchsorted(key, d, side="right").astype(np.int64)
    return row_split, d - row_split


def local_csr(csr, row_split, nz_split, g) -> Csr:
    """part g's local CSR: owned + 1 rows, offsets rebased by -nz_split[g], first offset 0, the open last row ends at the part's nnz"""
    off = csr.row_offsets.astype(np.int64)
    rb, re, a, b = int(row_split[g]), int(row_split[g + 1]), int(nz_split[g]), int(nz_split[g + 1])
    lo = np.concatenate([[0], off[rb + 1: re + 1] - a, [b - a]]).astype(np.int32)
    return Csr(re - rb + 1, csr.cols, lo, csr.column_indices[a:b].copy(), csr.values[a:b].copy())


def sources(row_split):
    """for every part: the earlier parts whose open row is this part's first owned row, ascending; [] for a part that owns no row"""
    rs = [int(v) for v in row_split]
    parts = len(rs) - 1
    return [[j for j in range(g) if rs[j + 1] == rs[g]] if rs[g + 1] > rs[g] else [] for g in range(parts)]


def fold(y_locals, row_split, dtype):
    """(global y, open-row entries): every part's owned entries, the first of an owner being (((y_local[0] + c_s1) + c_s2) + ...) in
    `dtype` over its sources in ascending part order, c_s = source s's open-row entry (its last local entry)."""
    dtype = np.dtype(dtype)
    parts = len(y_locals)
    rows = int(row_split[-1])
    y = np.zeros(rows, dtype)
    opens = np.array([np.asarray(yl, dtype)[-1] for yl in y_locals], dtype)
    for g, src in enumerate(sources(row_split)):
        rb, re = int(row_split[g]), int(row_split[g + 1])
        yl = np.asarray(y_locals[g], dtype)
        assert yl.size == re - rb + 1, (g, yl.size, re - rb + 1)
        if re == rb:
            continue
        seg = yl[: re - rb].copy()
        acc = seg[0]
        for s in src:
            acc = dtype.type(acc + opens[s])           # one IEEE add in the compute type per source
        seg[0] = acc
        y[rb:re] = seg
    assert len(y_locals) == parts
    return y, opens


# ------------------------------------------------------------------------------------------------------------ the problems

def _lens_giant_middle(rng):
    lens = rng.integers(0, 7, 4000); lens[2000] = 200_000
    return lens


def _lens_giant_first(rng):
    lens = rng.integers(0, 3, 3000); lens[0] = 60_000
    return lens


def _lens_giant_last(rng):
    lens = rng.integers(0, 3, 3000); lens[-1] = 60_000
    return lens


def _lens_giant_then_empty_rows(rng):
    lens = np.zeros(3000, np.int64); lens[10] = 150_000
    return lens


def _lens_empty_runs(rng):
    lens = np.zeros(20_000, np.int64); lens[::97] = 300
    return lens


def _lens_power_law(rng):
    return np.minimum((rng.pareto(1.1, 20_000) * 2).astype(np.int64), 60_000)


# name -> (row lengths, square): fixed seeds; every one a shape where the routing of the carries can go wrong
_BUILDERS = {
    "giant_middle": (_lens_giant_middle, True),                      # a row spanning most parts: owners with many sources, parts that own nothing
    "giant_first": (_lens_giant_first, False),
    "giant_last": (_lens_giant_last, False),
    "giant_then_empty_rows": (_lens_giant_then_empty_rows, False),   # the trailing parts' open row lies beyond the last nonzero
    "empty_runs": (_lens_empty_runs, True),
    "all_empty": (lambda rng: np.zeros(64, np.int64), True),
    "single_row": (lambda rng: np.array([77_777]), False),
    "fewer_items_than_parts": (lambda rng: np.array([2, 0, 1, 0, 0]), False),      # parts with no row and no nonzero
    "short": (lambda rng: rng.integers(0, 12, 20_000), True),
    "power_law": (_lens_power_law, False),
    "cuts_on_row_ends": (lambda rng: np.full(3200, 7, np.int64), True),             # 8 merge items per row: every cut at 2, 8, 64 parts on a row end
}
NONSQUARE_COLS = 1234


def _seed(name):
    return 1000 + sum(map(ord, name))


PROBLEMS = {name: (np.asarray(build(np.random.default_rng(_seed(name))), np.int64), square) for name, (build, square) in _BUILDERS.items()}


def shape(name):
    """(rows, cols, lens)"""
    lens, square = PROBLEMS[name]
    return lens.size, (lens.size if square else NONSQUARE_COLS), lens


def offsets(name):
    lens = PROBLEMS[name][0]
    off = np.zeros(lens.size + 1, np.int64); np.cumsum(lens, out=off[1:])
    return off


def integer_problem(name, dtype):
    """(csr, x): values from +-{1,2}, x from +-{1..3} (axpby_model.integer_problem): every sum exact in `dtype`"""
    import axpby_model as AM
    rows, cols, lens = shape(name)
    csr, x, _ = AM.integer_problem(np.random.default_rng(_seed(name) + 1), rows, cols, lens, dtype)
    return csr, x


WIDE_PARTS = [2, 7, 64]
# the shapes the wide draw runs on: a boundary row shared by several parts (the giants, single_row), rows cut by most boundaries
# (short, power_law), and every cut on a row end
WIDE_NAMES = ["giant_middle", "giant_first", "giant_last", "giant_then_empty_rows", "single_row", "short", "power_law", "cuts_on_row_ends"]


def wide_problem(name, dtype):
    """(csr, x): axpby_model.wide_problem -- odd integers that fill the exactness budget, so that every part's sums, its open-row
    entry and the folded carries hold bits in both halves of a double (in the low 16 bits of a float)"""
    import axpby_model as AM
    rows, cols, lens = shape(name)
    csr, x, _ = AM.wide_problem(np.random.default_rng(_seed(name) + 3), rows, cols, lens, dtype)
    return csr, x


IPC_ROWS, IPC_GIANT = 30000, 200_000


def ipc_wide_problem(dtype):
    """(lens, csr, x) of kind `wide` of tests/mg_ipc_worker.py: the shape of its kind `exact` -- rows of 0 .. 3 entries and one row
    of 200 000 in the middle, which spans every rank -- on axpby_model.wide_problem.  Here, not in the worker, so that
    tests/test_mg_model.py can check the data on the CPU."""
    import axpby_model as AM
    lens = np.random.default_rng(1234).integers(0, 4, IPC_ROWS); lens[IPC_ROWS // 2] = IPC_GIANT      # (the worker's first draw)
    csr, x, _ = AM.wide_problem(np.random.default_rng(1235), IPC_ROWS, IPC_ROWS, lens, dtype)
    return lens, csr, x


def wide_open_row_share(csr, x, parts):
    """(the open-row entries that are not zero, the share of them with a non-zero low half): what the fold adds"""
    import axpby_model as AM
    row_split, nz_split = partition(csr.row_offsets.astype(np.int64), parts)
    opens = np.array([AM.row_sums(local_csr(csr, row_split, nz_split, g), x)[0][-1] for g in range(parts)], np.int64)
    opens = opens[opens != 0].astype(csr.values.dtype)
    return opens.size, (float((AM.low_half(opens) != 0).mean()) if opens.size else 1.0)


def float_problem(name, dtype, scale=1.0):
    """(csr, x): values and x uniform in (-1, 1) (values times `scale`): sums round, the association matters"""
    rows, cols, lens = shape(name)
    rng = np.random.default_rng(_seed(name) + 2)
    off = offsets(name)
    nnz = int(off[-1])
    col = rng.integers(0, cols, nnz).astype(np.int32)
    col = col[np.lexsort((col, np.repeat(np.arange(rows), lens)))]
    val = (rng.uniform(-1, 1, nnz) * scale).astype(dtype)
    return Csr(rows, cols, off.astype(np.int32), col, val), rng.uniform(-1, 1, cols).astype(dtype)


def census(name, parts):
    """what a problem exercises at a part count, from the model alone"""
    off = offsets(name)
    row_split, nz_split = partition(off, parts)
    src = sources(row_split)
    owned = np.diff(row_split)
    nnz = np.diff(nz_split)
    rows = off.size - 1
    # the nonzeros of a part's open row (its share of global row row_split[g+1])
    open_nnz = np.array([int(nz_split[g + 1]) - max(int(off[min(int(row_split[g + 1]), rows)]), int(nz_split[g])) for g in range(parts)])
    taken = sorted({s for lst in src for s in lst})
    return {"zero_owned": int((owned == 0).sum()), "max_sources": max((len(s) for s in src), default=0),
            "takers": sum(1 for s in src if s), "empty_parts": int(((owned == 0) & (nnz == 0)).sum()),
            "taken": len(taken), "taken_empty": sum(1 for s in taken if open_nnz[s] == 0), "open_nnz": open_nnz}
