"""Every kernel form of mspmv_csrmm_f32 / _f64 on the device, exact, with the form that ran pinned by the launch log.

For every row of spmm_forms.CASES: the `mspmv: <kernel><<<grid, block>>>` lines of a debug_synchronous call must equal the launches
the restated dispatch rule (tests/spmm_forms.py) expects -- the kernel name gives the form, grid and block the tile size -- and Y
must equal an int64 reference BIT FOR BIT (the bit patterns are compared: -0.0 is not +0.0): matrix values (nonzero integers in [-8, 8], +-1 on the giant row), X (+-1 .. 3),
Y0 (+-1 .. 8), alpha in {1, -2} and beta in {0, 3} are integers with |alpha| sum |a x| + |beta| |y0| <= 2^24 (fp32; 2^53 in fp64) on
every row and column, which the test asserts on the reference's own sums first: every partial sum in any association order is then
an integer the format holds, and a dropped, doubled or misplaced product changes Y.  No row or column is left out.  X and Y are
views inside wider buffers; the other columns of X hold NaN, those of Y a sentinel that must survive.  Y is NaN before a call with
beta = 0.  A second call gives the same bits.

ZEROS.  Y0 is never zero here, so t = beta * Y0 is never -0.0 and every zero of Y is defined as +0.0 (include/mspmv.h at
mspmv_csrmm_*: sums start from +0.0, Y = alpha * s + (beta == 0 ? +0.0 : beta * Y0)), which is what the int64 reference converts
to.  The cases with alpha < 0 and beta == 0 are asserted to hold rows without entries and zero sums of rows with entries.
spmm_forms.ZERO_CASES run the tiny, mid and big cases again on ZERO-LADEN data: a quarter of the matrix values and of X zeros of
both signs, and planted rows -- every value a zero of mixed sign; every product exactly -0.0 in every column of X (or in every
second one); pairs v, -v on one column that cancel wherever X is not zero there.  The huge cases run the same arithmetic with
non-temporal loads and keep their non-zero data.  spmm_forms.SCALED (one pack and one slot case per precision) run with the
integers scaled so that one unit of the reference is the smallest subnormal (values and X normal; the stored values subnormal)
and 2^(emax - mantissa bits); the scaled arrays are made on the host.  test_negative_zero_in_y0_on_rows_without_entries is the one
place where t is -0.0: on rows without entries, where the definition gives alpha * (+0.0) + (-0.0).

WIDE.  All of the above are integers of a few bits: the low 32 bits of every fp64 product, sum and carry are zero.
spmm_forms.WIDE_CASES run one case per form and precision -- the row-wise kernel, every pack width, the slot form of 16 and 8, two
groups of 16 in the slot form; all but the row-wise through the carries and the fix-up on the giant row -- on odd integers that fill
the exactness budget per row and per column of X (Call.plant_wide: the rule of tests/axpby_model.wide_problem, made on the device
from the same hashes); Call.assert_wide asserts on the reference that at least 95 % of the results of every column, and in fp64 at
least 90 % of the running sums of every row longer than a tile at every tile-th entry, have a non-zero low half.  The launch log is
pinned as for every other case.

The log names the kernel, grid.x and block of every launch: that pins the form and the tile size.  Which AXPBY / NT instantiation
ran, the width of a pack launch among those sharing a tile size, and the fix-up's grid.y (groups) are not printed; the coverage
table's axpby and nt columns are what the restated rule says of the call's alpha, beta and stream size, not an observation.  A wrong
width or group count does show in the exact comparison (columns left unwritten stay NaN or Y0).

The matrices (spmm_forms.structure) are built once each and freed before the next.

Measured on one MI355X: the 78 tests of this file take 11.6 s (the reference now adds its running sums in two halves that cannot wrap), the 70 of the
parent commit 8.8 s (the 30 before the zero-laden and
scaled cases: 5.3 s), beside some four minutes for the other GPU tests.  Sensitivity, each a one-line change of mspmv_spmm.hpp tried against this file, every failure the exact comparison:
the slot form's before() stopping one slot early fails the 10 big_slots / big_slot_groups / huge_slots_nt cases; its carries
indexed without g * num_tiles the 4 cases with two groups of 16 (big_slot_groups, huge_slots_nt_plain); the pack kernel without
its nz_tail store every case that runs a pack (24 tests: the last row, in the pack widths' columns); the fix-up without its
look-ahead sum all 26 tests off the row-wise kernel (the giant row).  Writing the pack kernel's select `in ? val * xv : 0` as a
product with 0 / 1 changes nothing in Y: the positions it zeroes lie outside the tile's own nonzeros in LDS, where no row sum,
carry or scan result that is used reads -- with X[0, :] = NaN those positions hold NaN and Y is still the clean run's, which is
what test_nan_and_inf_stay_where_they_are asserts.  The "+ 0" of the beta == 0 write taken out again (pack kernel's row phase and
the slot form's put, the state before the sign of a zero sum was pinned): 10 tests fail, all on the sign of a zero -- mid_wide_groups_* (alpha = -2, beta = 0) with
and without zeros, big_slots_negative_alpha_beta_0_*_zeros, and step 4 of test_nan_and_inf_stay_where_they_are on the pack and the
slot case of both precisions.  The slot form's fp64 carry stored through (float) (`cr->value.v[c + k] = (T) (float) s[k]`), tried
against the parent commit's version of this file and against this one: 3 / 5 tests fail -- both see it where the scaled case puts
one unit at the smallest subnormal (the cast flushes: test_both_ends_of_the_exponent_range[big_slots_axpby_f64-*]); at the plain
scale only big_slots_axpby_f64_wide and big_slot_groups_f64_wide do.  The other one-line changes tried against the wide data:
tests/test_axpby_exact.py.
"""
import re

import numpy as np
import pytest

import axpby_model as AM
import spmm_forms as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "f64": torch.float64}
EXACT = {"f32": 1 << 24, "f64": 1 << 53}
SENTINEL = 777.0
ROW_CHUNK = 1 << 21
MAT_ORDER = {"tiny": 0, "mid": 1, "big": 2, "huge": 3}
ORDERED = sorted(F.CASES + F.ZERO_CASES + F.WIDE_CASES, key=lambda c: MAT_ORDER[c.mat])
NPDT = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64)}
# the constants of the wide rule are axpby_model's; the draw itself is restated on the device (Call.plant_wide: hashes, not an rng)
WIDE_XMAX = {p: AM.WIDE_XMAX[d] for p, d in NPDT.items()}
LOW_BITS = {p: AM.LOW_BITS[d] for p, d in NPDT.items()}       # the "low half" of a bit pattern
assert all(AM.LIMIT[d] == EXACT[p] for p, d in NPDT.items())
BOTTOM, TOP = {"f32": -149, "f64": -1074}, {"f32": 127 - 24, "f64": 1023 - 53}        # the smallest subnormal; 2^(emax - mantissa bits)
KIND_I, KIND_II, KIND_III, KIND_II_EVEN = 3, 7, 11, 13      # row % 16 of the planted rows of the zero-laden data
ZERO_COL, POS_COL, NEG_ZERO_COL, NEG_COL, EVEN_COL = 1, 2, 3, 4, 5
LAUNCH = re.compile(r"^mspmv: (\w+)<<<(\d+), (\d+)>>>$", re.M)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _hash(seed, idx):
    from merge_spmv_amd.generators import splitmix64
    return splitmix64(seed, idx) & ((1 << 63) - 1)


def _odd(seed, idx, hi):
    """odd integers in [1, hi] (hi a number or a tensor, >= 1)"""
    return 2 * (_hash(seed, idx) % ((hi + 1) // 2)) + 1


def _sign(seed, idx, negative_in=2):
    """-1 for one index in `negative_in`, else 1"""
    return 1 - 2 * (_hash(seed, idx) % negative_in == 0).to(torch.int64)


def _low_half(t, prec):
    return _bits(t) & ((1 << LOW_BITS[prec]) - 1)


def _pm(seed, idx, m):
    """nonzero integers in [-m, m]"""
    t = _hash(seed, idx) % (2 * m)
    return t - m + (t >= m).to(torch.int64)


class Mat:
    """one structure on the device: int64 values, row offsets per trim, column indices per column count"""

    def __init__(self, name):
        self.name, self.s = name, F.structure(name)
        s = self.s
        self.rows, self.nnz_full = s.rows, s.nnz()
        k = torch.arange(self.nnz_full, dtype=torch.int64, device="cuda")
        self.vals64 = _pm(0x5F0001, k, 8)
        if s.giant:
            off = s.offsets()
            g = int(s.lens.argmax())
            self.giant_row, self.giant_lo, self.giant_hi = g, int(off[g]), int(off[g + 1])
            self.vals64[self.giant_lo:self.giant_hi] = torch.sign(self.vals64[self.giant_lo:self.giant_hi])     # the giant row: +-1
        self._off, self._cols, self._vals = {}, {}, {}

    def off(self, trim):
        if trim not in self._off:
            self._off[trim] = torch.from_numpy(self.s.offsets(trim)).cuda()
        return self._off[trim]

    def cols(self, n):
        """column indices in [1, n): column 0 is never referenced"""
        if n not in self._cols:
            k = torch.arange(self.nnz_full, dtype=torch.int64, device="cuda")
            c = 1 + _hash(0x5F0002 + n, k) % (n - 1)
            self._cols = {n: c}                        # (one at a time)
        return self._cols[n]

    def vals(self, prec):
        if prec not in self._vals:
            self._vals = {prec: self.vals64.to(TDT[prec])}
        return self._vals[prec]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    import merge_spmv_amd as M_
    M_.load_library()          # raises if the HIP extension is missing: no fallback
    return M_


@pytest.fixture(scope="module")
def mats():
    """the matrix of the current case; the tests come ordered by matrix, so each is built once"""
    held = {}

    def get(name):
        if name not in held:
            held.clear()
            torch.cuda.empty_cache()
            held[name] = Mat(name)
        return held[name]
    yield get
    held.clear()
    torch.cuda.empty_cache()


TARGET_MEMORY = 250 << 30               # an MI355X reports 288 GB: on such a card every case fits, and one that does not is a failure


def _room(need, what):
    """`need`: X's buffer, three int64 columns of X for the reference, the chunk temporaries of X's generator, Y's buffer three times,
    six int64 [rows, k] arrays (Y0, reference, sums, comparisons), eight int64 arrays of nnz entries, 2 GiB of slack.  Only a card
    smaller than the target may skip: a skipped case could be the only cover of a form."""
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert free >= need or total < TARGET_MEMORY, f"{what}: needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free of {total / 2**30:.1f}"
    if free < need:
        pytest.skip(f"{what}: needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free of {total / 2**30:.1f}")


class Call:
    """the device arrays of one case: the CSR views, X inside its NaN-filled buffer, Y0, the exact reference"""

    def __init__(self, mat, c):
        self.c, self.mat = c, mat
        dt, eb = TDT[c.prec], F.ELEM[c.prec]
        rows, cols, nnz = c.dims()
        self.rows, self.cols, self.nnz, self.dt = rows, cols, nnz, dt
        _room(cols * c.xw * eb + cols * 8 * 3 + ROW_CHUNK * c.k * 8 * 6 + rows * (c.yw * eb * 3 + c.k * 8 * 6) + nnz * 8 * 8 + (2 << 30), c.name)
        self.off64 = mat.off(c.trim)
        self.off = self.off64.to(torch.int32)
        self.cidx = mat.cols(cols)[:nnz].clone()
        self.cidx[-1] = cols - 1                   # the last nonzero sits in the last column (its neighbours keep theirs: the tail's
                                                   # products then differ from column to column of X)
        self.vals64 = mat.vals64[:nnz]
        v = mat.vals(c.prec)[:nnz]
        if c.zeros:
            v = self.plant_zeros()
        if c.wide:
            v = self.plant_wide()
        ci = self.cidx.to(torch.int32)
        if c.pad:
            vp = torch.empty(nnz + c.pad, dtype=dt, device="cuda")[c.pad:]; vp.copy_(v); v = vp
            cp = torch.empty(nnz + c.pad, dtype=torch.int32, device="cuda")[c.pad:]; cp.copy_(ci); ci = cp
            assert v.data_ptr() % 16 != 0 and ci.data_ptr() % 16 != 0
        else:
            assert v.data_ptr() % 16 == 0 and ci.data_ptr() % 16 == 0 and self.off.data_ptr() % 16 == 0
        self.vals, self.ci = v, ci
        # X: the view holds integers, every other column of the buffer NaN
        self.Xw = torch.full((cols, c.xw), float("nan"), dtype=dt, device="cuda")
        self.X = self.Xw[:, c.x_off:c.x_off + c.k]
        j = torch.arange(c.k, dtype=torch.int64, device="cuda")
        for lo in range(0, cols, ROW_CHUNK):
            hi = min(lo + ROW_CHUNK, cols)
            r = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
            self.X[lo:hi] = _pm(0x5F0003, r[:, None] * 64 + j[None, :], 3).to(dt)
            if c.wide:                                 # odd, up to xmax; one sign per row of X (plant_wide signs the values by it)
                self.X[lo:hi] = (_odd(0x5F0024, r[:, None] * 64 + j[None, :], self.xmax) * _sign(0x5F0023, r)[:, None]).to(dt)
            if c.zeros:                                # a quarter zeros, of both signs
                h = _hash(0x5F0013, r[:, None] * 64 + j[None, :]) % 8
                self.X[lo:hi] = torch.where(h == 0, 0.0, torch.where(h == 1, -0.0, self.X[lo:hi].to(torch.float64))).to(dt)
        if c.zeros:
            # the columns a planted row refers to: X all +0.0, all positive, all -0.0, all negative, +0.0 in every second column
            self.X[ZERO_COL], self.X[cols - 1] = 0.0, 0.0
            self.X[POS_COL], self.X[NEG_ZERO_COL], self.X[NEG_COL] = self.X[POS_COL].abs().clamp(min=1), -0.0, -self.X[NEG_COL].abs().clamp(min=1)
            self.X[EVEN_COL] = torch.where(j % 2 == 0, 0.0, 2.0).to(dt)
            xb = _bits(self.X)
            assert bool((xb == 0).any()) and bool((xb == _bits(torch.tensor([-0.0], dtype=dt, device="cuda"))).any())
        assert self.Xw.data_ptr() % 256 == 0
        r = torch.arange(rows, dtype=torch.int64, device="cuda")
        self.y0 = _pm(0x5F0004, r[:, None] * 64 + j[None, :], 8)
        if c.wide:
            self.y0 = _odd(0x5F0025, r[:, None] * 64 + j[None, :], self.budget) * _sign(0x5F0026, r[:, None] * 64 + j[None, :])
        self.y_ref, self.s = self.reference(self.vals64, self.X)

    def plant_zeros(self):
        """the zero-laden values (and column indices) of this case; returns the float values, leaves their integers in vals64"""
        c, nnz, dt = self.c, self.nnz, self.dt
        k = torch.arange(nnz, dtype=torch.int64, device="cuda")
        row = torch.searchsorted(self.off64, k, right=True) - 1
        pos, length = k - self.off64[row], (self.off64[1:] - self.off64[:-1])[row]
        kind = row % 16
        v = self.vals64.clone()
        h = _hash(0x5F0011, k) % 8
        v[h < 2] = 0
        negz = h == 1                                                       # the zeros that are -0.0
        if self.cols > EVEN_COL + 1:
            # (ii): every product exactly -0.0, whatever the column of X: negative * +0.0, -0.0 * positive, positive * -0.0, +0.0 * negative
            m = kind == KIND_II
            to = 1 + _hash(0x5F0012, k) % 4
            self.cidx = torch.where(m, to, self.cidx)
            mag = self.vals64.abs()
            v = torch.where(m & (to == ZERO_COL), -mag, torch.where(m & (to == NEG_ZERO_COL), mag, torch.where(m, 0, v)))
            negz = torch.where(m, to == POS_COL, negz)
            # (ii) in every second column of X, a negative sum in the others
            m = kind == KIND_II_EVEN
            self.cidx = torch.where(m, EVEN_COL, self.cidx)
            v = torch.where(m, -mag, v)
            # (iii): pairs v, -v on one column; the last value of a row of odd length is a zero
            m = kind == KIND_III
            head = m & (pos % 2 == 0)
            v = torch.where(head & (v == 0), 1, v)
            tail = (m & (pos % 2 == 1)).nonzero()[:, 0]
            v[tail] = -v[tail - 1]
            self.cidx[tail] = self.cidx[tail - 1]
            v = torch.where(head & (pos == length - 1), 0, v)
        # (i): every value a zero, the signs alternating
        m = kind == KIND_I
        v = torch.where(m, 0, v)
        negz = torch.where(m, (pos + row // 16) % 2 == 1, negz)
        # the last nonzero meets X[cols - 1, :] = +0.0 with a negative value
        self.cidx[-1] = self.cols - 1
        v[-1] = -1
        if nnz < 64:                                                        # (the tiny case: a stored -0.0 whatever the hash drew)
            v[0], negz[0] = 0, True
        self.vals64 = v
        f = v.to(torch.float64)
        f = torch.where((v == 0) & negz, -0.0, f).to(dt)
        fb = _bits(f)
        assert bool((fb == _bits(torch.tensor([-0.0], dtype=dt, device="cuda"))).any()) and (nnz < 64 or bool((fb == 0).any()))
        return f

    def plant_wide(self):
        """the wide values of this case, the rule of axpby_model.wide_problem per row and per column of X: with the budget
        B = 2^24 (2^53) // 16, X odd integers up to xmax = min(2^8 (2^20), isqrt(B // longest row)) and the values of a row of n
        entries odd integers up to max(1, B // (n * xmax)), signed so that three products in four are positive in every column
        of X (a row of X has one sign).  Returns the float values, leaves their integers in vals64."""
        import math
        c, nnz = self.c, self.nnz
        self.budget = AM.wide_budget(NPDT[c.prec])
        lens = self.off64[1:] - self.off64[:-1]
        self.xmax = max(1, min(WIDE_XMAX[c.prec], math.isqrt(self.budget // int(lens.max()))))
        k = torch.arange(nnz, dtype=torch.int64, device="cuda")
        row = torch.searchsorted(self.off64, k, right=True) - 1
        hi = (self.budget // (lens[row] * self.xmax)).clamp(min=1)
        self.vals64 = _odd(0x5F0021, k, hi) * _sign(0x5F0023, self.cidx) * _sign(0x5F0022, k, 4)
        return self.vals64.to(self.dt)

    def assert_wide(self):
        """conditions on the wide data, from the reference: in every column at least 95 % of the rows with entries have a Y with a
        non-zero low half (low 32 bits of an fp64 pattern, low 16 of an fp32 one); in fp64, of the running sums of every row longer
        than a tile of the case, taken at every tile-th entry (column 0 of X) -- what carries are made of --, at least 90 %"""
        c = self.c
        lens = self.off64[1:] - self.off64[:-1]
        low = _low_half(self.want().to(self.dt), c.prec)[lens > 0]
        share = (low != 0).to(torch.float64).mean(0)
        assert float(share.min()) >= 0.95, f"{c.name}: the share of results with a non-zero low half is {share.tolist()}"
        if c.prec != "f64" or c.launches()[0][0] == "spmm_rowwise_kernel":
            return
        p = self.vals64 * self.X[:, 0].to(torch.int64)[self.cidx]
        seen = 0
        for T in sorted({g.tile for g in c.groups()}):
            for r in torch.nonzero(lens > T)[:, 0].tolist():
                lo, hi = int(self.off64[r]), int(self.off64[r + 1])
                sums = torch.cumsum(p[lo:hi], 0)[torch.arange(T - 1, hi - lo - 1, T, device="cuda")]      # (this row's own running sum)
                wide = float((_low_half(sums.to(self.dt), c.prec) != 0).to(torch.float64).mean())
                assert wide >= 0.9, f"{c.name}: row {r}, tile {T}: {wide} of {sums.numel()} running sums have a non-zero low half"
                seen += 1
        assert seen >= 2                                        # (the giant row and the open last row at least)

    def reference(self, vals64, X):
        """int64 [rows, k]: the segmented sums of a * X[col] and of |a * X[col]|, from running sums that CANNOT WRAP: a product is
        split into p = hi * 2^24 + lo (0 <= lo < 2^24, hi the floor), and each half gets its own running sum over all nonzeros --
        both stay below 2^62, which is asserted.  (One running sum of p itself passes 2^63 on the wide data, where sum |a x| is
        about 2^47 per row, and would give the right differences only through two's-complement wraparound.  No atomics.)"""
        a, b = self.off64[:-1], self.off64[1:]

        def segment_sums(p):
            hi = p >> 24                                 # (arithmetic shift: the floor, also of a negative product)
            lo = p - (hi << 24)
            assert (int(hi.abs().max()) + 1) * p.numel() < 1 << 62 and p.numel() < 1 << 38
            ch = torch.nn.functional.pad(torch.cumsum(hi, 0), (1, 0))
            cl = torch.nn.functional.pad(torch.cumsum(lo, 0), (1, 0))
            return ((ch[b] - ch[a]) << 24) + (cl[b] - cl[a])
        y = torch.empty(self.rows, self.c.k, dtype=torch.int64, device="cuda")
        s = torch.empty_like(y)
        for jj in range(self.c.k):
            p = vals64 * X[:, jj].to(torch.int64)[self.cidx]
            y[:, jj] = segment_sums(p)
            s[:, jj] = segment_sums(p.abs())
        return y, s

    def want(self, alpha=None, beta=None):
        c = self.c
        alpha, beta = c.alpha if alpha is None else alpha, c.beta if beta is None else beta
        return alpha * self.y_ref + (beta * self.y0 if beta else 0)

    def fresh_y(self, beta=None, y0=None):
        """(buffer, view): the view holds Y0 -- NaN when beta == 0 --, the other columns the sentinel"""
        c = self.c
        beta = c.beta if beta is None else beta
        Yw = torch.full((self.rows, c.yw), SENTINEL, dtype=self.dt, device="cuda")
        Y = Yw[:, c.y_off:c.y_off + c.k]
        if beta == 0:
            Y.fill_(float("nan"))
        else:
            Y.copy_((self.y0 if y0 is None else y0).to(self.dt))
        assert Yw.data_ptr() % 256 == 0
        return Yw, Y

    def run(self, M, vals=None, alpha=None, beta=None, debug=False):
        c = self.c
        alpha, beta = c.alpha if alpha is None else alpha, c.beta if beta is None else beta
        Yw, Y = self.fresh_y(beta)
        M.csrmm(self.vals if vals is None else vals, self.off, self.ci, self.X, Y=Y, alpha=float(alpha), beta=float(beta),
                debug_synchronous=debug)
        torch.cuda.synchronize()
        c0, c1 = c.y_off, c.y_off + c.k
        assert bool((Yw[:, :c0] == SENTINEL).all()) and bool((Yw[:, c1:] == SENTINEL).all()), f"{c.name}: a column of the buffer outside Y was written"
        return Y


def _assert_exact(name, Y, want, off64, what=""):
    """the bit patterns: an int64 zero of the reference is +0.0, and a -0.0 in Y differs from it"""
    ref = want.to(Y.dtype) if want.dtype == torch.int64 else want
    assert bool((ref.to(torch.float64) == want.to(torch.float64)).all()), f"{name}: the reference is not representable"
    bad = _bits(Y) != _bits(ref)
    if not bool(bad.any()):
        return
    got, ref = Y.to(torch.float64), ref.to(torch.float64)
    at = torch.nonzero(bad)
    r, j = int(at[0, 0]), int(at[0, 1])
    pytest.fail(f"{name} {what}: {int(bad.sum())} of {bad.numel()} entries differ from the exact reference, in {int(bad.any(1).sum())} rows and "
                f"columns {sorted(set(at[:, 1].tolist()))[:48]}; first: row {r} (nonzeros {int(off64[r])}..{int(off64[r + 1])}) column {j}: "
                f"got {float(got[r, j])!r}, want {float(ref[r, j])!r}")


def _assert_zero_rows(call):
    """a case with alpha < 0 and beta == 0 is about the sign of a zero: it must hold rows without entries and zero sums of rows with
    entries (on the reference, before the call)"""
    lens = call.off64[1:] - call.off64[:-1]
    assert bool((lens == 0).any()), f"{call.c.name}: no row without entries"
    assert bool(((call.y_ref == 0) & (lens > 0)[:, None]).any()), f"{call.c.name}: no zero result on a row with entries"


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: c.name)
def test_form_runs_and_is_exact(M, mats, capfd, case):
    c = case
    call = Call(mats(c.mat), c)
    # the condition under which every association order is exact, on the reference's own sums
    worst = int((abs(c.alpha) * call.s + abs(c.beta) * call.y0.abs()).max())
    assert worst <= EXACT[c.prec], f"{c.name}: |alpha| sum |a x| + |beta| |y0| reaches {worst}"
    assert int(call.s.min()) >= 0 and int(call.cidx.min()) >= 1 and int(call.cidx.max()) == call.cols - 1
    if c.alpha < 0 and c.beta == 0:
        _assert_zero_rows(call)
    if c.wide:
        call.assert_wide()
    if c.zeros and c.mat != "tiny":
        # per column of X: zero sums of rows whose products are all zero, and of rows whose non-zero products cancel
        lens = (call.off64[1:] - call.off64[:-1])[:, None]
        assert bool(((call.s == 0) & (lens > 0)).any(0).all()) and bool(((call.s > 0) & (call.y_ref == 0)).any(0).all())
    capfd.readouterr()
    Y = call.run(M, debug=True)
    log = [(n, int(g), int(b)) for n, g, b in LAUNCH.findall(capfd.readouterr().out)]
    expect = c.launches()
    assert log == [e[:3] for e in expect], f"{c.name}: the call launched {log}, the dispatch rule says {expect}"
    _assert_exact(c.name, Y, call.want(), call.off64)
    Y2 = call.run(M)
    assert torch.equal(_bits(Y), _bits(Y2)), f"{c.name}: a second call gives other bits"


@pytest.mark.parametrize("case", sorted(F.CONTAINMENT, key=lambda c: MAT_ORDER[c.mat]), ids=lambda c: c.name)
def test_nan_and_inf_stay_where_they_are(M, mats, case):
    """NaN in X[0, :] (the row the masked dummy gathers read; no nonzero references column 0) reaches nothing; a NaN matrix value
    poisons all k columns of its row only -- on a short row, a row of exactly one tile and the giant row, whose sums travel through
    the carries and the fix-up --; an Inf in X[c, j] column j of the rows that reference c only; NaN in Y0 is never read with
    beta = 0.  Everything else is bit for bit the clean run."""
    c = case
    mat = mats(c.mat)
    call = Call(mat, c)
    clean = call.run(M)
    _assert_exact(c.name, clean, call.want(), call.off64, "clean run")
    k, rows = c.k, call.rows

    def compare(Y, mask, what):
        assert torch.equal(_bits(Y)[~mask], _bits(clean)[~mask]), f"{c.name}: {what}: entries outside the poisoned ones differ from the clean run"
        assert not bool(torch.isfinite(Y[mask]).any()), f"{c.name}: {what}: a poisoned entry is finite"

    none = torch.zeros(rows, k, dtype=torch.bool, device="cuda")
    # 1. NaN in row 0 of X (the whole buffer row)
    keep = call.Xw[0].clone()
    call.Xw[0] = float("nan")
    compare(call.run(M), none, "NaN in X[0, :]")
    call.Xw[0] = keep
    # 2. NaN matrix values
    lens = torch.from_numpy(mat.s.lens).cuda()
    T = c.groups()[0].tile
    picks = [int(torch.nonzero(lens == 5)[0]), int(torch.nonzero(lens == T - 1)[0]), mat.giant_row]
    vals = call.vals.clone()
    mask = none.clone()
    for r in picks:
        lo, hi = int(call.off64[r]), int(call.off64[r + 1])
        vals[(lo + hi) // 2] = float("nan")
        mask[r, :] = True
    compare(call.run(M, vals=vals), mask, f"NaN values in rows {picks}")
    del vals
    # 3. Inf in X[c1, 0] and X[c2, k - 1]
    mask = none.clone()
    q = int(call.off64[picks[0]])
    spots = [(int(call.cidx[q]), 0), (int(call.cidx[q + 1]) if int(call.cidx[q + 1]) != int(call.cidx[q]) else int(call.cidx[q + 2]), k - 1)]
    kept = []
    for col, j in spots:
        at = torch.nonzero(call.cidx == col)[:, 0]
        hit = torch.unique(torch.searchsorted(call.off64, at, right=True) - 1)
        assert hit.numel() >= 1
        mask[hit, j] = True
        kept.append(float(call.X[col, j]))
        call.X[col, j] = float("inf")
    compare(call.run(M), mask, f"Inf in X at {spots}")
    for (col, j), v in zip(spots, kept):
        call.X[col, j] = v
    # 4. beta = 0: Y0 = NaN is never read (alpha = -2), and a zero sum under a negative alpha is +0.0
    _assert_zero_rows(call)
    Y = call.run(M, alpha=c.alpha, beta=0)
    _assert_exact(c.name, Y, call.want(c.alpha, 0), call.off64, "beta = 0 over a NaN Y")


@pytest.mark.parametrize("which", ["bottom", "bottom_stored", "top"])
@pytest.mark.parametrize("case", sorted(F.SCALED, key=lambda c: MAT_ORDER[c.mat]), ids=lambda c: c.name)
def test_both_ends_of_the_exponent_range(M, mats, case, which):
    """The case's integers times powers of two: one unit of the reference is the smallest subnormal -- values and X both normal, only
    products and sums subnormal (bottom), or the stored values themselves subnormal and X small integers (bottom_stored) -- or
    2^(emax - mantissa bits) (top: at most 2^24 | 2^53 units in any association, so nothing may overflow).  Every intermediate
    stays an exact multiple of the unit; a flush to zero anywhere changes Y.  Scaled on the host: numpy's ldexp is exact."""
    c = case
    call = Call(mats(c.mat), c)
    assert int((abs(c.alpha) * call.s + abs(c.beta) * call.y0.abs()).max()) <= EXACT[c.prec]
    total = TOP[c.prec] if which == "top" else BOTTOM[c.prec]
    ev = total if which == "bottom_stored" else total // 2
    ex = total - ev
    ndt = np.float32 if c.prec == "f32" else np.float64

    def scaled(t, e):
        a = t.cpu().numpy().astype(np.float64)
        w = np.ldexp(a, e)
        out = w.astype(ndt)
        assert np.array_equal(out.astype(np.float64)[~np.isnan(a)], w[~np.isnan(a)]), "a scaled input is not representable"
        host[len(host):] = [out]
        return torch.from_numpy(out).cuda()
    host = []
    vals = scaled(call.vals64, ev)
    if c.pad:
        vp = torch.empty(call.nnz + c.pad, dtype=call.dt, device="cuda")[c.pad:]; vp.copy_(vals); vals = vp
    tiny = float(np.finfo(ndt).tiny)
    mag = np.abs(host[0])                                      # (the host copy: a device op that flushed would hide what it checks)
    if which == "bottom_stored":
        assert 0 < mag.min() and mag.max() < tiny
    keep = call.Xw.clone()
    try:
        call.Xw.copy_(scaled(call.Xw, ex))
        if which == "bottom":
            xh = np.abs(host[1][:, c.x_off:c.x_off + c.k])
            assert mag.min() >= tiny and xh.min() >= tiny
        want = scaled(call.want(), total)
        Yw, Y = call.fresh_y()
        Y.copy_(scaled(call.y0, total))
        M.csrmm(vals, call.off, call.ci, call.X, Y=Y, alpha=float(c.alpha), beta=float(c.beta))
        torch.cuda.synchronize()
        assert bool((Yw[:, :c.y_off] == SENTINEL).all()) and bool((Yw[:, c.y_off + c.k:] == SENTINEL).all())
        _assert_exact(c.name, Y, want, call.off64, which)
    finally:
        call.Xw.copy_(keep)


@pytest.mark.parametrize("alpha", [2, -2])
@pytest.mark.parametrize("case", sorted(F.CONTAINMENT, key=lambda c: MAT_ORDER[c.mat]), ids=lambda c: c.name)
def test_negative_zero_in_y0_on_rows_without_entries(M, mats, case, alpha):
    """t = beta * Y0 = -0.0 on every row without entries (beta = 3): such a row is alpha * (+0.0) + (-0.0) -- +0.0 for a positive
    alpha, -0.0 for a negative one -- in the pack kernel and in the slot form, whose rows without entries are written by a loop of
    their own (writing beta * Y alone there gives -0.0 for alpha = 2).  Rows with entries keep their non-zero Y0: a zero sum of
    non-zero products under t = -0.0 is the undefined corner."""
    c = case
    call = Call(mats(c.mat), c)
    empty = (call.off64[1:] == call.off64[:-1])
    assert int(empty.sum()) > F.TILE_SLOT
    Yw, Y = call.fresh_y(beta=3)
    Y[empty] = -0.0
    assert bool((_bits(Y[empty]) != 0).all())
    M.csrmm(call.vals, call.off, call.ci, call.X, Y=Y, alpha=float(alpha), beta=3.0)
    torch.cuda.synchronize()
    want = call.want(alpha, 3).to(call.dt)
    want[empty] = -0.0 if alpha < 0 else 0.0
    _assert_exact(c.name, Y, want, call.off64, f"alpha = {alpha}, Y0 = -0.0 on rows without entries")
