"""An exact model of y = alpha*A*x + beta*y for tests/test_axpby_exact.py (numpy only, no GPU).

Inputs are small non-zero integers and alpha, beta multiples of a granule g = 2^-k <= 1, sized so that for every row
    (|alpha| * sum|v*x| + |beta*y0|) / g  <  2^24 (fp32)  |  2^53 (fp64).
Every product, every partial sum in any association, every carry, every alpha * carry and every old + alpha * carry -- fused or
not -- is then a multiple of g below 2^24 g (2^53 g) in magnitude and therefore exact: the kernel's result is DEFINED bit for bit,
whichever path computes it, and the model computes it in int64.  The bound is a condition on the inputs (model() asserts it),
not a tolerance.  Nothing drawn is zero, so no product is -0.0: a zero in y is an exact cancellation or the empty sum, +0.0
(include/mspmv.h at mspmv_csrmv_axpby_*).
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import numpy as np

# dyadic and integer, both signs, beta in {0, 1, other}, alpha == 0
PAIRS = [(1, 0), (2, 0), (-0.5, 3), (-1.5, 0.5), (1, 1), (2.5, -1), (0, -2), (3, -5)]

LIMIT = {np.dtype(np.float32): 1 << 24, np.dtype(np.float64): 1 << 53}


@dataclass
class Csr:
    """(the fields of oracle.Csr that the GPU tests use)"""
    rows: int
    cols: int
    row_offsets: np.ndarray
    column_indices: np.ndarray
    values: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.row_offsets[-1]) if self.row_offsets.size else 0


def _signed(rng, n, hi, dtype):
    """n draws from +-{1..hi}: never zero"""
    return (rng.integers(1, hi + 1, size=n) * (2 * rng.integers(0, 2, size=n) - 1)).astype(dtype)


def integer_problem(rng, rows, cols, lens, dtype, vmax=2, xmax=3, ymax=8):
    """CSR built like test_gpu_parity.random_csr (random columns, sorted within rows) with values from +-{1..vmax}, x from
    +-{1..xmax} and y0 from +-{1..ymax}.  Returns (csr, x, y0)."""
    lens = np.asarray(lens, np.int64)
    assert lens.size == rows
    off = np.zeros(rows + 1, dtype=np.int64); np.cumsum(lens, out=off[1:])
    nnz = int(off[-1])
    col = rng.integers(0, max(cols, 1), size=nnz).astype(np.int32)
    rowid = np.repeat(np.arange(rows), lens)
    col = col[np.lexsort((col, rowid))]
    csr = Csr(int(rows), int(cols), off.astype(np.int32), col, _signed(rng, nnz, vmax, dtype))
    return csr, _signed(rng, cols, xmax, dtype), _signed(rng, rows, ymax, dtype)


def granule(alpha, beta) -> Fraction:
    """the largest g = 2^-k <= 1 that alpha and beta are both multiples of"""
    a, b = Fraction(alpha), Fraction(beta)          # (exact for a float: every float is a dyadic rational)
    g = Fraction(1, max(a.denominator, b.denominator))
    assert g.denominator & (g.denominator - 1) == 0 and (a / g).denominator == 1 and (b / g).denominator == 1
    return g


def _exact_int(a, what):
    a = np.asarray(a)
    i = a.astype(np.int64)
    assert np.array_equal(i.astype(a.dtype), a), f"{what} must hold integers"
    return i


def row_sums(csr, x):
    """(sum v*x, sum |v*x|) per row in int64"""
    off = csr.row_offsets.astype(np.int64)
    prod = _exact_int(csr.values, "values") * _exact_int(x, "x")[csr.column_indices]
    cs = np.concatenate([[0], np.cumsum(prod)])
    ca = np.concatenate([[0], np.cumsum(np.abs(prod))])
    return cs[off[1:]] - cs[off[:-1]], ca[off[1:]] - ca[off[:-1]]


def quotient(csr, x, y0, alpha, beta) -> int:
    """max over rows of (|alpha| * sum|v*x| + |beta*y0|) / g: what must stay below 2^24 (2^53)"""
    g = granule(alpha, beta)
    A, B = abs(int(Fraction(alpha) / g)), abs(int(Fraction(beta) / g))
    _, sa = row_sums(csr, x)
    q = A * sa
    if B:
        q = q + B * np.abs(_exact_int(y0, "y0"))
    return int(q.max(initial=0))


def model(csr, x, y0, alpha, beta) -> np.ndarray:
    """alpha*A*x + beta*y0 in int64 units of the granule, scaled back into the compute dtype.  beta == 0: y0 is not used (it may
    hold anything).  Asserts the exactness bound for every row."""
    dtype = np.dtype(csr.values.dtype)
    g = granule(alpha, beta)
    A, B = int(Fraction(alpha) / g), int(Fraction(beta) / g)
    q = quotient(csr, x, y0, alpha, beta)
    assert q < LIMIT[dtype], f"not exact in {dtype}: a row reaches {q} granules of {g}, the limit is {LIMIT[dtype]}"
    s, _ = row_sums(csr, x)
    units = A * s
    if B:
        units = units + B * _exact_int(y0, "y0")
    # |units| < 2^53: the conversion is exact, and so is the scaling by a power of two; an int64 zero becomes +0.0
    return (units.astype(np.float64) * float(g)).astype(dtype)


def bits(a) -> np.ndarray:
    """the bit patterns: NaN-safe, and -0.0 is not +0.0"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)
