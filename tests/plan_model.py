"""Plain models of what tests/test_plan_exact.py and tests/test_hotcols_skew.py compare the device with, and the integer-valued
cases whose product is one bit pattern whatever order a kernel adds in.  numpy only, int64 and float64 only; written from what
include/mspmv.h documents about mspmv_csrmv_plan_* and mspmv_csrmv_hotcols_skew, nothing of the C++ is imported or transcribed.

  stack       the band-major plan's stacked matrix A' = [A_0; ...; A_{B-1}]: band_width = max(1, ceil(cols / B)), entry j of row r
              lies in group (column // band_width) * rows + r, the entries of a group keep the order they have in A;
  skew        the hot-column probe: 512 windows of 2048 consecutive nonzeros at w * (nnz - 2048) // 511, the distinct 128-byte lines
              of x over all of them against L * (1 - exp(-n / L)), the windows whose max - min column spans >= 3/4 of the columns;
  exact_case  integer values, x and y over a given sparsity structure, small enough that every partial sum in any association is
              an exact fp32 number.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import axpby_model as AM

ALPHA_BETA = ((1.0, 0.0), (-2.0, 0.0), (-0.5, 3.0), (0.0, 2.0))
EXACT_BOUND = 1 << 22
SKEW_WINDOWS, SKEW_WINDOW = 512, 2048


@dataclass
class Csr:
    rows: int
    cols: int
    row_offsets: np.ndarray          # int64 [rows + 1]
    column_indices: np.ndarray       # int64 [nnz]
    values: np.ndarray               # [nnz], any dtype

    @property
    def nnz(self) -> int:
        return int(self.row_offsets[-1])

    def row_of_entry(self) -> np.ndarray:
        return np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.row_offsets))


def csr(rows, cols, lens, column_indices, values=None) -> Csr:
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    column_indices = np.asarray(column_indices, np.int64)
    assert column_indices.size == off[-1] and (column_indices.size == 0 or (column_indices.min() >= 0 and column_indices.max() < cols))
    return Csr(int(rows), int(cols), off, column_indices, np.zeros(column_indices.size) if values is None else np.asarray(values))


def band_width(cols: int, bands: int) -> int:
    return max(1, -(-cols // bands))


def stack(a: Csr, bands: int) -> Csr:
    """the stacked matrix of bands * rows rows; `.order` = for every stacked entry, its position in A"""
    w = band_width(a.cols, bands)
    key = (a.column_indices // w) * a.rows + a.row_of_entry()
    assert key.size == 0 or key.max() < bands * a.rows
    order = np.argsort(key, kind="stable")
    off = np.zeros(bands * a.rows + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=bands * a.rows), out=off[1:])
    s = Csr(bands * a.rows, a.cols, off, a.column_indices[order], a.values[order])
    s.order = order
    return s


def product_int(a: Csr, x) -> np.ndarray:
    """A x in int64, for integer-valued values and x"""
    v, xi = np.asarray(a.values).astype(np.int64), np.asarray(x).astype(np.int64)
    assert np.array_equal(v, a.values) and np.array_equal(xi, x)
    y = np.zeros(a.rows, np.int64)
    np.add.at(y, a.row_of_entry(), v * xi[a.column_indices])
    return y


def fold(ypart: np.ndarray, rows: int, bands: int) -> np.ndarray:
    """y'[0 : rows] + y'[rows : 2 rows] + ..., bands added in order, in ypart's own type"""
    s = ypart[:rows].copy()
    for b in range(1, bands):
        s = s + ypart[b * rows:(b + 1) * rows]
    return s


def skew(column_indices, cols: int, value_bytes: int):
    """(distinct_lines, wide_windows, samples, permille, ratio_x1000): what mspmv_csrmv_hotcols_skew reports (permille, wide_windows)
    and the numbers behind it; permille = -1 and 0 wide windows for fewer than 2048 nonzeros or no columns"""
    c = np.asarray(column_indices)
    nnz = c.size
    if nnz < SKEW_WINDOW or cols < 1:
        return 0, 0, 0, -1, float("nan")
    shift = {4: 5, 8: 4}[value_bytes]                      # 128-byte lines of x
    lines = ((cols - 1) >> shift) + 1
    starts = np.arange(SKEW_WINDOWS, dtype=np.int64) * (nnz - SKEW_WINDOW) // (SKEW_WINDOWS - 1)
    win = c[starts[:, None] + np.arange(SKEW_WINDOW, dtype=np.int64)[None, :]].astype(np.int64)
    distinct = int(np.unique(win >> shift).size)
    wide = int(np.count_nonzero(4 * (win.max(axis=1) - win.min(axis=1)) >= 3 * cols))
    samples = SKEW_WINDOWS * SKEW_WINDOW
    expect = lines * (1.0 - math.exp(-samples / lines))
    ratio = 1000.0 * distinct / expect
    return distinct, wide, samples, int(math.floor(ratio + 0.5)), ratio


@dataclass
class ExactCase:
    a: Csr                    # values: integers in float64
    x: np.ndarray             # int64 [cols]
    y0: np.ndarray            # int64 [rows]
    ax: np.ndarray            # int64 [rows]: A x

    def want(self, alpha: float, beta: float) -> np.ndarray:
        """alpha * A x + beta * y0, exact in float64 (and in float32: the bound of exact_case); every zero is +0.0"""
        return (alpha * self.ax.astype(np.float64) + beta * self.y0.astype(np.float64)) + 0.0


def exact_case(rng, structure: Csr, cap: int = 4) -> ExactCase:
    """Values in {-cap .. cap} without 0, x in {-8 .. 8}, y0 in {-16 .. 16} over `structure`.  Asserts, for every (alpha, beta) of
    ALPHA_BETA and every row, max(1, |alpha|) * sum |a_ij x_j| + |beta| |y0_i| <= 2^22: every sum of products in any association,
    its multiple by alpha and the result are then integers or half-integers below 2^24 in magnitude, i.e. exact in fp32."""
    n = structure.nnz
    mag = rng.integers(1, cap + 1, n)
    val = np.where(rng.integers(0, 2, n) == 1, mag, -mag).astype(np.int64)
    x = rng.integers(-8, 9, structure.cols).astype(np.int64)
    y0 = rng.integers(-16, 17, structure.rows).astype(np.int64)
    a = Csr(structure.rows, structure.cols, structure.row_offsets, structure.column_indices, val.astype(np.float64))
    s_abs = np.zeros(a.rows, np.int64)
    np.add.at(s_abs, a.row_of_entry(), np.abs(val * x[a.column_indices]))
    for alpha, beta in ALPHA_BETA:
        worst = max(1.0, abs(alpha)) * s_abs + abs(beta) * np.abs(y0)
        assert worst.size == 0 or worst.max() <= EXACT_BOUND, (alpha, beta, float(worst.max()))
    return ExactCase(a, x, y0, product_int(a, x))


# the wide rule is tests/axpby_model.py's: its limits, its cap on x, its budget, its odd draw and its scalars, by precision name
NPDT = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64)}
WIDE_LIMIT = {p: AM.LIMIT[d] for p, d in NPDT.items()}
# alpha, beta that fill the significand: no number here is an fp32 number (f64) / a bf16 or fp16 number (f32); granule 2^-30 (2^-12)
WIDE_SCALARS = {p: tuple((float(a), float(b)) for a, b in AM.WIDE_PAIRS[d]) for p, d in NPDT.items()}


def fits_wide_scalars(case: ExactCase, prec: str) -> bool:
    """whether y = alpha A x + beta y0 is exact in any association for the pairs of WIDE_SCALARS[prec]: in granules,
    |alpha| sum |a x| + |beta| |y0| < 2^24 (2^53) on every row (then ExactCase.want, computed in float64, is exact as well)"""
    v = np.asarray(case.a.values).astype(np.int64)
    s_abs = np.zeros(case.a.rows, np.int64)
    np.add.at(s_abs, case.a.row_of_entry(), np.abs(v * case.x[case.a.column_indices]))
    g = 1 << (30 if prec == "f64" else 12)
    worst = (g + 2) * s_abs + (g + 1) * np.abs(case.y0)
    return bool(worst.size == 0 or worst.max() < WIDE_LIMIT[prec])


def wide_case(rng, structure: Csr, prec: str) -> ExactCase:
    """exact_case with magnitudes that FILL the exactness budget of the precision instead of sitting at its bottom, drawn by
    tests/axpby_model.wide_problem (B = 2^24 (2^53) // 2 // 8; x odd integers up to xmax = min(2^8 (2^20), isqrt(B // longest row)),
    the values of a row of n entries odd integers up to max(1, B // (n * xmax)), three products in four positive, y0 odd integers
    up to B) and laid over `structure`.  Every number has a one in its lowest used bit, and sums, every band's partial sums and results carry
    bits in both halves of a double.  Asserts |alpha| / g * sum |a x| + |beta| / g * |y0| < 2^24 (2^53) per row for ALPHA_BETA, g the
    granule 1/2 of alpha = -0.5."""
    lens = np.diff(structure.row_offsets)
    col = structure.column_indices
    # (wide_problem draws a structure of its own first; its values follow that structure's row lengths, and are signed here by the
    #  x of THIS structure's columns)
    drawn, x, y0 = AM.wide_problem(rng, structure.rows, structure.cols, lens, NPDT[prec])
    x, y0 = x.astype(np.int64), y0.astype(np.int64)
    val = np.abs(drawn.values.astype(np.int64)) * np.sign(x)[col] * np.where(rng.random(col.size) < 0.75, 1, -1)
    a = Csr(structure.rows, structure.cols, structure.row_offsets, col, val.astype(np.float64))
    s_abs = np.zeros(a.rows, np.int64)
    np.add.at(s_abs, a.row_of_entry(), np.abs(val * x[col]))
    for alpha, beta in ALPHA_BETA:
        worst = int(2 * abs(alpha)) * s_abs + int(2 * abs(beta)) * np.abs(y0)              # in halves
        assert worst.size == 0 or worst.max() < WIDE_LIMIT[prec], (alpha, beta, int(worst.max()))
    return ExactCase(a, x.astype(np.int64), y0.astype(np.int64), product_int(a, x))


def low_half_share(numbers, prec: str, among=None) -> float:
    """the share of `numbers` (integers, exact in the precision) whose bit pattern in the precision has a non-zero low half (low 32
    bits of a double, low 16 of a float); among: a mask of the ones that count (1.0 when none does)"""
    f = np.asarray(numbers).astype(np.float32 if prec == "f32" else np.float64)
    assert np.array_equal(f.astype(np.float64), np.asarray(numbers, np.float64))
    low = AM.low_half(f)
    low = low if among is None else low[among]
    return float((low != 0).mean()) if low.size else 1.0


# ---- the sparsity structures of tests/test_plan_exact.py (sorted rows; some depend on the band count) ----
BANDS = (1, 2, 3, 8, 24, 64)


def sorted_rows(rng, rows, cols, lens, hole=None):
    """random columns, non-decreasing inside every row (repeats allowed); `hole`: a column no entry takes"""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    col = rng.integers(0, cols if hole is None else cols - 1, n)
    if hole is not None:
        col = col + (col >= hole)
    row = np.repeat(np.arange(rows, dtype=np.int64), lens)
    return csr(rows, cols, lens, col[np.lexsort((col, row))])


def structures(bands: int, seed: int = 0) -> dict:
    """name -> Csr (values unset): the shapes at which the plan's build, fold and band arithmetic can go wrong"""
    rng = np.random.default_rng(1000 + 17 * bands + seed)
    w = band_width(1000, bands)
    out = {}
    # several blocks of the fold, a row count that is no multiple of 4, a short last band whenever 1000 % bands != 0
    out["rows1027"] = sorted_rows(rng, 1027, 1000, rng.integers(0, 13, 1027), hole=333)
    out["cols5"] = sorted_rows(rng, 37, 5, rng.integers(0, 6, 37))                   # fewer columns than bands: band_width 1, empty trailing bands
    out["cols_eq_bands"] = sorted_rows(rng, 50, bands, rng.integers(0, 5, 50))
    out["cols1"] = sorted_rows(rng, 70, 1, rng.integers(0, 4, 70))
    edges = sorted({0, 999} | {c for k in range(1, bands) for c in (k * w - 1, k * w) if c < 1000})
    out["band_edges"] = csr(300, 1000, np.full(300, len(edges)), np.tile(edges, 300))  # both sides of every band edge, in every row
    base = sorted_rows(rng, 200, 1000, rng.integers(0, 5, 200), hole=777)
    rep = rng.integers(2, 4, base.nnz)                                                 # every column 2 or 3 times, side by side
    lens = np.zeros(200, np.int64); np.add.at(lens, base.row_of_entry(), rep)
    out["repeats"] = csr(200, 1000, lens, np.repeat(base.column_indices, rep))
    out["row5000"] = sorted_rows(rng, 41, 3000, np.where(np.arange(41) == 20, 5000, 0), hole=1500)   # longer than a 1024-chunk of the build
    for n in (1023, 1024, 1025):                                                       # around one chunk: in one row (and rows == 1) ...
        out[f"one_row_{n}"] = sorted_rows(rng, 1, 2000, [n], hole=5)
    out["rows341x3"] = sorted_rows(rng, 341, 1000, np.full(341, 3))                   # ... and as rows of 3: nnz 1023, 1024, 1025, 1026
    for last in (1, 2, 3):
        out[f"rows342_last{last}"] = sorted_rows(rng, 342, 1000, np.r_[np.full(341, 3), last])
    out["empty_ends"] = sorted_rows(rng, 500, 1000, np.where((np.arange(500) >= 100) & (np.arange(500) < 400), rng.integers(1, 7, 500), 0))
    out["rows1"] = sorted_rows(rng, 1, 40, [7])
    lo = (bands - 1) * w if (bands - 1) * w < 1000 else 999                            # entries in the last band that has columns only
    lb = sorted_rows(rng, 203, 1000 - lo, rng.integers(0, 6, 203))
    out["last_band"] = csr(203, 1000, np.diff(lb.row_offsets), lb.column_indices + lo)
    return out


def more_y_structures(seed: int = 0) -> dict:
    """the further shapes of the exact-y test: one row of 300 000 among 3000, one row in 97 of 40 000, and the row counts around a
    multiple of the fold's vector width over more than one of its blocks"""
    rng = np.random.default_rng(2000 + seed)
    out = {"giant_row": sorted_rows(rng, 3000, 100000, np.where(np.arange(3000) == 1500, 300000, rng.integers(0, 3, 3000)), hole=4242),
           "mostly_empty": sorted_rows(rng, 40000, 7000, np.where(np.arange(40000) % 97 == 0, 50, 0), hole=7)}
    for rows in (1026, 1027, 1028):
        out[f"rows{rows}"] = sorted_rows(rng, rows, 600, rng.integers(0, 9, rows), hole=300)
    return out
