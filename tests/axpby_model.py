"""An exact model of y = alpha*A*x + beta*y for tests/test_axpby_exact.py (numpy only, no GPU).

Inputs are small integers and alpha, beta multiples of a granule g = 2^-k <= 1, sized so that for every row
    (|alpha| * sum|v*x| + |beta*y0|) / g  <  2^24 (fp32)  |  2^53 (fp64).
Every product, every partial sum in any association, every carry, every alpha * carry and every old + alpha * carry -- fused or
not -- is then a multiple of g below 2^24 g (2^53 g) in magnitude and therefore exact: the kernel's result is DEFINED bit for bit,
whichever path computes it, and the model computes it in int64.  The bound is a condition on the inputs (model() asserts it),
not a tolerance.

ZEROS.  integer_problem draws no zero; zero_problem draws stored zeros and zeros in x of both signs and plants rows whose products
are all zeros.  The sign of a zero result follows the definition of include/mspmv.h at mspmv_csrmv_axpby_*: every sum and every
carry starts from +0.0 and so is never -0.0, y[r] = alpha * s + t with t = (beta == 0 ? +0.0 : beta * y0[r]).  Hence a zero
result is +0.0 unless t is -0.0; where t is -0.0 and every product of the row is zero (or the row is empty) it is -0.0 for a
negative alpha and +0.0 otherwise; where t is -0.0 and non-zero products cancel, the sign depends on where tiles cut the row: that
corner is undefined, zero_problem never draws it and model() asserts that.  test_axpby_model.py shows by brute force that the
rule does not depend on cuts, association or the order of the carries.

WIDE.  integer_problem's numbers sit at the bottom of that budget: every product, sum, carry and result is an integer below about
2^21, so the low 32 bits of every fp64 number on the way are zero and alpha, beta are fp32 (and bf16) numbers -- half of a double, or
a scalar narrowed to float, could be lost without one bit of any result changing.  wide_problem draws the same structure with ODD
magnitudes that fill the budget (LIMIT // 2 // 8 per row: the 8 is the largest |alpha| / g + |beta| / g of PAIRS), so the lowest used
bit of every input is a one and sums, carries and results carry bits in both halves; low_half() / low_half_share() /
carry_low_half_shares() say how much of a problem's results and of a long row's running sums do.  WIDE_PAIRS are scalars that are
no fp32 (no bf16, no fp16) numbers; their granule is 2^-30 (2^-12), so they run on the narrow draw, where the bound allows them.

SCALES.  scaled() multiplies values and x by powers of two; the model's result is the exact ldexp of its int64 units.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

# dyadic and integer, both signs, beta in {0, 1, other}, alpha == 0
PAIRS = [(1, 0), (2, 0), (-0.5, 3), (-1.5, 0.5), (1, 1), (2.5, -1), (0, -2), (3, -5)]

LIMIT = {np.dtype(np.float32): 1 << 24, np.dtype(np.float64): 1 << 53}

# scalars that fill the significand: no number here is an fp32 number (fp64) / a bf16 or fp16 number (fp32)
WIDE_PAIRS = {np.dtype(np.float64): [(1 + 2.0 ** -30, 0), (-(1 + 2.0 ** -29), 1 + 2.0 ** -30)],
              np.dtype(np.float32): [(1 + 2.0 ** -12, 0), (-(1 + 2.0 ** -11), 1 + 2.0 ** -12)]}
WIDE_XMAX = {np.dtype(np.float32): 1 << 8, np.dtype(np.float64): 1 << 20}
LOW_BITS = {np.dtype(np.float32): 16, np.dtype(np.float64): 32}        # the "low half" of a number's bit pattern
CARRY_STRIDES = (256 * 7, 256 * 11)                                      # the two tile sizes: where a long row's running sum is cut


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


def _odd(rng, hi):
    """odd integers from +-[1, hi], hi an array (or a size-1 array broadcast by the caller): never zero, the lowest bit a one"""
    hi = np.asarray(hi, np.int64)
    assert (hi >= 1).all()
    return (2 * rng.integers(0, (hi + 1) // 2) + 1) * (2 * rng.integers(0, 2, size=hi.shape) - 1)


def wide_budget(dtype) -> int:
    """what sum |v*x| of a row and |y0| may reach: with |alpha| / g + |beta| / g <= 8 (PAIRS) the quotient stays below LIMIT / 2"""
    return LIMIT[np.dtype(dtype)] // 2 // 8


def wide_problem(rng, rows, cols, lens, dtype, vcap=None):
    """integer_problem's structure with magnitudes that FILL the exactness budget B = wide_budget(dtype):
      x       odd integers from +-[1, xmax], xmax = min(2^20 (fp64) | 2^8 (fp32), isqrt(B // longest row));
      values  of a row of n entries: odd integers of magnitude in [1, max(1, B // (n * xmax))] (vcap: a further cap on it), signed
              by the sign of their x so that THREE PRODUCTS IN FOUR ARE POSITIVE -- with even odds a long row's sums stay near
              sqrt(n) products, and in fp32 a row of thousands of entries would leave the low half empty;
      y0      odd integers from +-[1, B].
    Then sum |v*x| <= B for every row of at most B entries.  A longer row (fp32 only) has values and x of +-1, and whether the
    bound holds depends on the pair: model() asserts it.  Returns (csr, x, y0)."""
    dtype = np.dtype(dtype)
    lens = np.asarray(lens, np.int64)
    csr, _, _ = integer_problem(rng, rows, cols, lens, dtype.type, vmax=1)
    budget = wide_budget(dtype)
    longest = max(int(lens.max(initial=0)), 1)
    xmax = max(1, min(WIDE_XMAX[dtype], math.isqrt(budget // longest)))
    vhi = np.maximum(1, budget // (np.maximum(lens, 1) * xmax))
    if vcap is not None:                            # (values a narrower stored type holds: tests/test_mixed_precision.py)
        vhi = np.minimum(vhi, vcap)
    x = _odd(rng, np.full(cols, xmax))
    val = np.abs(_odd(rng, np.repeat(vhi, lens))) * np.sign(x)[csr.column_indices] * np.where(rng.random(csr.nnz) < 0.75, 1, -1)
    val, x = val.astype(dtype), x.astype(dtype)
    y0 = _odd(rng, np.full(rows, budget)).astype(dtype)
    return Csr(csr.rows, csr.cols, csr.row_offsets, csr.column_indices, val), x, y0


def low_half(a) -> np.ndarray:
    """the low 32 (fp64) / 16 (fp32) bits of each number's bit pattern"""
    a = np.ascontiguousarray(a)
    return bits(a) & ((1 << LOW_BITS[a.dtype]) - 1)


def low_half_share(csr, y) -> float:
    """the share of the rows with entries whose y has a non-zero low half (1.0 for a matrix without entries)"""
    has = np.diff(csr.row_offsets.astype(np.int64)) > 0
    return float((low_half(y)[has] != 0).mean()) if has.any() else 1.0


def carry_low_half_shares(csr, x, strides=CARRY_STRIDES):
    """for every row longer than min(strides): (row, the number of its running sums v*x taken after every stride-th entry, for each
    stride -- what carries, records and folded carries of the row are made of --, the share of them with a non-zero low half as
    numbers of the values' type)"""
    dtype = np.dtype(csr.values.dtype)
    off = csr.row_offsets.astype(np.int64)
    prod = _exact_int(csr.values, "values") * _exact_int(x, "x")[csr.column_indices]
    out = []
    for r in np.flatnonzero(np.diff(off) > min(strides)):
        n = int(off[r + 1] - off[r])
        at = np.concatenate([np.arange(s, n, s) for s in strides])
        sums = np.cumsum(prod[off[r]:off[r + 1]])[at - 1]      # (a running sum of THIS row: nothing of other rows to wrap round)
        assert (np.abs(sums) < LIMIT[dtype]).all()
        out.append((int(r), at.size, float((low_half(sums.astype(dtype)) != 0).mean())))
    return out


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


def segment_sums(a, off):
    """the sum of a[off[r] : off[r + 1]] for every r, each row summed ON ITS OWN (np.add.reduceat over the rows with entries).
    A running sum over the whole array would pass 2^63 -- the wide draw holds sum |v*x| of about 2^47 per row, so after some 10^5
    rows -- and give the right differences only through two's-complement wraparound."""
    off = np.asarray(off, np.int64)
    out = np.zeros(off.size - 1, a.dtype)
    has = off[1:] > off[:-1]
    if has.any():
        out[has] = np.add.reduceat(a, off[:-1][has])     # (rows with entries start where the last such row ended: rows without lie between)
    return out


def row_sums(csr, x):
    """(sum v*x, sum |v*x|) per row in int64; asserts that no row's own sum comes near the int64 range"""
    off = csr.row_offsets.astype(np.int64)
    prod = _exact_int(csr.values, "values") * _exact_int(x, "x")[csr.column_indices]
    mag = np.abs(prod)
    assert float(segment_sums(mag.astype(np.float64), off).max(initial=0)) < 2.0 ** 62, "a row's sum |v*x| does not fit int64"
    return segment_sums(prod, off), segment_sums(mag, off)


def quotient(csr, x, y0, alpha, beta) -> int:
    """max over rows of (|alpha| * sum|v*x| + |beta*y0|) / g: what must stay below 2^24 (2^53)"""
    g = granule(alpha, beta)
    A, B = abs(int(Fraction(alpha) / g)), abs(int(Fraction(beta) / g))
    _, sa = row_sums(csr, x)
    q = A * sa
    if B:
        q = q + B * np.abs(_exact_int(y0, "y0"))
    return int(q.max(initial=0))


def t_is_negative_zero(y0, beta):
    """rows where t = (beta == 0 ? +0.0 : beta * y0[r]) is -0.0"""
    y0 = np.asarray(y0)
    if beta == 0:
        return np.zeros(y0.shape, bool)
    return (y0 == 0) & (np.signbit(y0) != (beta < 0))


def model(csr, x, y0, alpha, beta, scale=0) -> np.ndarray:
    """alpha*A*x + beta*y0 in int64 units of the granule, scaled back into the compute dtype.  beta == 0: y0 is not used (it may
    hold anything).  Asserts the exactness bound for every row, and the domain of the zero-sign rule: where t is -0.0 and the result
    is zero, every product of the row is zero.  csr, x, y0 hold the UNSCALED integers; scale = e_values + e_x of scaled(): the result
    is that of the scaled arrays, an exact ldexp of the units."""
    dtype = np.dtype(csr.values.dtype)
    g = granule(alpha, beta)
    A, B = int(Fraction(alpha) / g), int(Fraction(beta) / g)
    q = quotient(csr, x, y0, alpha, beta)
    assert q < LIMIT[dtype], f"not exact in {dtype}: a row reaches {q} granules of {g}, the limit is {LIMIT[dtype]}"
    s, sa = row_sums(csr, x)
    units = A * s
    if B:
        units = units + B * _exact_int(y0, "y0")
    # |units| < 2^53: the conversion is exact, and so is the scaling by a power of two; an int64 zero becomes +0.0
    e = int(scale) - (g.denominator.bit_length() - 1)
    wide = np.ldexp(units.astype(np.float64), e)
    y = wide.astype(dtype)
    assert np.array_equal(np.ldexp(y.astype(np.float64), -e), units.astype(np.float64)), f"the scaled result is not representable in {dtype}"
    # the sign of a zero result: +0.0 unless t is -0.0; then every product must be zero, and alpha * (+0.0) + (-0.0) decides
    tneg = t_is_negative_zero(y0, beta) if B else np.zeros(csr.rows, bool)
    at = (units == 0) & tneg
    assert not (at & (sa != 0)).any(), "outside the definition: t is -0.0 on a row whose non-zero products cancel (or alpha == 0)"
    if alpha < 0:
        y[at] = -0.0
    return y


def scaled(problem, e_values, e_x):
    """(csr, x, y0) with values * 2^e_values, x * 2^e_x and y0 * 2^(e_values + e_x), built in float64 and cast; every scaled
    number must be representable (asserted).  model(..., scale=e_values + e_x) on the UNSCALED problem is its result."""
    csr, x, y0 = problem
    dtype = np.dtype(csr.values.dtype)

    def sc(a, e, dt):
        w = np.ldexp(np.asarray(a, np.float64), e)
        out = w.astype(dt)
        assert np.array_equal(out.astype(np.float64), w) and np.array_equal(np.signbit(out), np.signbit(np.asarray(a))), "a scaled input is not representable"
        return out
    c2 = Csr(csr.rows, csr.cols, csr.row_offsets, csr.column_indices, sc(csr.values, e_values, csr.values.dtype))
    return c2, sc(x, e_x, dtype), sc(y0, e_values + e_x, dtype)


# the two ends of the exponent range, from the type alone: the smallest subnormal and 2^(emax - mantissa bits)
BOTTOM = {np.dtype(np.float32): -149, np.dtype(np.float64): -1074}
TOP = {np.dtype(np.float32): 127 - 24, np.dtype(np.float64): 1023 - 53}
SCALE_PAIRS = [(1, 0), (-1.5, 0.5), (3, -5)]             # (granule 1/2: the product scale is one binade above the result's granule)


def scale_exponents(dtype, which, pairs=SCALE_PAIRS, e_values=None):
    """(e_values, e_x) that put the granule of the results of `pairs` at the smallest subnormal ("bottom": every product, sum, carry
    and result a subnormal or one of the smallest normals; "bottom_stored": the stored values themselves subnormal, x small integers)
    or at 2^(emax - mantissa) ("top": every intermediate in any association below the largest finite number)."""
    dtype = np.dtype(dtype)
    k = max(granule(a, b).denominator for a, b in pairs).bit_length() - 1
    total = (TOP if which == "top" else BOTTOM)[dtype] + k
    if e_values is None:
        e_values = total if which == "bottom_stored" else total // 2
    return e_values, total - e_values


# ---------------------------------------------------------------------------------------------------------------- zeros

KIND_I, KIND_II, KIND_III = 1, 2, 3      # (i) every value a zero, signs mixed; (ii) every product exactly -0.0; (iii) non-zero products cancel


def _with_zeros(rng, n, hi, dtype):
    """n draws from {-hi..-1, -0.0, +0.0, 1..hi}: about a quarter zeros, both signs"""
    a = _signed(rng, n, hi, dtype)
    z = rng.random(n) < 0.25
    a[z] = np.where(rng.integers(0, 2, int(z.sum())) == 1, -0.0, 0.0).astype(dtype)
    return a


def zero_problem(rng, rows, cols, lens, dtype, vmax=2, xmax=3, ymax=8, forced=None):
    """integer_problem with zeros: values from {-vmax.., -0.0, +0.0, ..vmax}, x from {-xmax.., -0.0, +0.0, ..xmax}, about a quarter
    zeros each.  Rows are planted of kind (i) every value a zero of mixed sign, (ii) every product exactly -0.0 (a negative value
    times +0.0, -0.0 times a positive x, ...: the one kind a sum started from its first product gets wrong) and (iii) non-zero
    products that cancel exactly (pairs v, -v on one column): the three longest rows are of kinds (ii), (iii), (i), `forced`
    ({row: kind}) says more, and of the other rows with entries about a quarter are planted.  y0 is from +-{1..ymax} with zeros: of
    both signs on rows whose products are all zero (or that are empty), -0.0 alone on rows with a non-zero sum (alpha == 0 with a
    negative beta would make +0.0 a t of -0.0 under a zero result there), none where non-zero products cancel.
    Returns (csr, x, y0)."""
    lens = np.asarray(lens, np.int64)
    csr, _, _ = integer_problem(rng, rows, cols, lens, dtype, vmax=vmax)
    off = csr.row_offsets.astype(np.int64)
    nnz = csr.nnz
    val = _with_zeros(rng, nnz, vmax, dtype)
    x = _with_zeros(rng, cols, xmax, dtype)
    if cols >= 4:                                    # both signs of zero and both signs of a number, whatever was drawn
        x[:4] = np.array([0.0, -0.0, 1, -1], dtype)[rng.permutation(4)]
    col = csr.column_indices.copy()
    kind = np.zeros(rows, np.int8)
    has = np.flatnonzero(lens > 0)
    pick = rng.random(has.size)
    kind[has[pick < 0.05]] = KIND_I
    kind[has[(pick >= 0.05) & (pick < 0.15)]] = KIND_II
    kind[has[(pick >= 0.15) & (pick < 0.25)]] = KIND_III
    longest = has[np.argsort(-lens[has], kind="stable")[:3]]
    for r, k in zip(longest, (KIND_II, KIND_III, KIND_I)):
        kind[r] = k
    for r, k in (forced or {}).items():
        assert lens[r] > 0
        kind[r] = k
    nonzero_cols = np.flatnonzero(x != 0)
    kind[(kind == KIND_III) & ((lens < 2) | (nonzero_cols.size == 0))] = 0
    rowid = np.repeat(np.arange(rows), lens)
    # (i): zeros, the signs alternating from a random start (both signs in every row of two entries and more)
    m = kind[rowid] == KIND_I
    pos = np.arange(nnz) - off[rowid]
    val[m] = np.where((pos[m] + rng.integers(0, 2, rows)[rowid[m]]) % 2 == 1, -0.0, 0.0).astype(dtype)
    # (ii): the value that makes the product with its x exactly -0.0
    m = kind[rowid] == KIND_II
    xs = x[col[m]]
    mag = rng.integers(1, vmax + 1, int(m.sum())).astype(dtype)
    val[m] = np.where(xs > 0, -0.0,                                                  # -0.0 * positive
             np.where(xs < 0, 0.0,                                                   # +0.0 * negative
             np.where(np.signbit(xs), mag, -mag))).astype(dtype)                     # positive * -0.0, negative * +0.0
    # (iii): pairs (v, -v) on one column with a non-zero x; an odd row's last value is a zero
    for r in np.flatnonzero(kind == KIND_III):
        a, n = int(off[r]), int(lens[r])
        c = np.sort(rng.choice(nonzero_cols, n // 2)).astype(np.int32)
        v = _signed(rng, n // 2, vmax, dtype)
        col[a:a + 2 * (n // 2)] = np.repeat(c, 2)
        val[a:a + 2 * (n // 2):2] = v
        val[a + 1:a + 2 * (n // 2):2] = -v
        if n % 2:
            col[a + n - 1] = max(int(col[a + n - 2]), int(col[a + n - 1]))
            val[a + n - 1] = dtype(-0.0) if r % 2 else dtype(0.0)
    out = Csr(int(rows), int(cols), csr.row_offsets, col, val)
    s, sa = row_sums(out, x)
    y0 = _signed(rng, rows, ymax, dtype)
    z = rng.random(rows) < 0.25
    zero = np.where(rng.integers(0, 2, rows) == 1, -0.0, 0.0).astype(dtype)
    y0 = np.where(z & (sa == 0), zero, np.where(z & (s != 0), dtype(-0.0), y0)).astype(dtype)
    return out, x, y0


def census(csr, x, y0, pairs, tiles):
    """what a zero-laden problem holds: rows of each kind, rows of kind (ii) that cross a tile boundary of each tile size (row r's
    nonzeros are the merge-path items r + row_offsets[r] .. r + row_offsets[r + 1] - 1), zero results under t = -0.0 over `pairs`,
    and the signs of zero among values, x and y0"""
    off = csr.row_offsets.astype(np.int64)
    lens = np.diff(off)
    rowid = np.repeat(np.arange(csr.rows), lens)
    prod = csr.values * np.asarray(x)[csr.column_indices]
    cnt = lambda m: np.bincount(rowid[m], minlength=csr.rows)
    s, sa = row_sums(csr, x)
    neg0 = (prod == 0) & np.signbit(prod)
    k1 = (lens > 0) & (cnt(csr.values == 0) == lens)
    k2 = (lens > 0) & (cnt(neg0) == lens)
    k3 = (sa != 0) & (s == 0)
    r = np.arange(csr.rows)
    out = {"kind_i": int(k1.sum()), "kind_ii": int(k2.sum()), "kind_iii": int(k3.sum()), "empty": int((lens == 0).sum()),
           "kind_i_mixed_signs": int((k1 & (cnt((csr.values == 0) & np.signbit(csr.values)) > 0) & (cnt((csr.values == 0) & ~np.signbit(csr.values)) > 0)).sum()),
           "longest": int(lens.max(initial=0)), "longest_kind_ii": int(lens[k2].max(initial=0))}
    for T in tiles:
        out[f"kind_ii_crosses:{T}"] = int((k2 & ((r + off[:-1]) // T != (r + off[1:] - 1) // T)).sum())
        out[f"kind_iii_crosses:{T}"] = int((k3 & ((r + off[:-1]) // T != (r + off[1:] - 1) // T)).sum())
    z = 0
    for alpha, beta in pairs:
        z += int((t_is_negative_zero(y0, beta) & (sa == 0)).sum())
    out["zero_results_under_negative_zero_t"] = z
    for name, a in (("values", csr.values), ("x", x), ("y0", y0)):
        a = np.asarray(a)
        out[f"{name}:+0"] = int(((a == 0) & ~np.signbit(a)).sum())
        out[f"{name}:-0"] = int(((a == 0) & np.signbit(a)).sum())
    return out


def bits(a) -> np.ndarray:
    """the bit patterns: NaN-safe, and -0.0 is not +0.0"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)
