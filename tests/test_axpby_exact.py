"""y = alpha*A*x + beta*y on every CsrMV dispatch path, BIT FOR BIT against the int64 model of tests/axpby_model.py.

Every CsrMV kernel is compiled twice (AXPBY = false / true), the fix-up kernels take alpha, the column-band passes rewrite beta per
pass: a second copy of the hot path.  The inputs here are small integers and (alpha, beta) dyadic, sized so that every sum
in every association is exact (axpby_model.model asserts it per row): y is then defined on the bits, whichever kernels compute it,
and every comparison below is on the bit patterns -- no tolerance anywhere, no row left out, -0.0 is not +0.0.

Every problem comes in two draws: without a zero anywhere (a zero of y is then an exact cancellation or the empty sum, +0.0), and
ZERO-LADEN (axpby_model.zero_problem: stored zeros and zeros in x of both signs, zeros in y0, rows whose products are all -0.0, all
zeros, or cancel), where the sign of every zero result is what include/mspmv.h defines at mspmv_csrmv_axpby_*: sums and carries
start from +0.0.  The zero-laden draw also runs SCALED to the two ends of the exponent range (axpby_model.scale_exponents): the
granule at the smallest subnormal -- once with normal values and x, once with the stored values themselves subnormal -- and at
2^(emax - mantissa bits); the scaled arrays are built on the host.  A flush to zero or a sum started from its first product in any
one instantiation fails here.

Sensitivity of the zero-laden tests, each a one-line change of csrc/mspmv_kernels.hpp tried against this file on one MI355X
(counted over this file, test_mixed_precision.py and test_plan_exact.py; the unchanged library passes all of them):
  * consume_tile_flags' `s[k] += lead ? carry_in : (V) 0` made conditional (`if (lead) s[k] += carry_in`): 362 of the zero-laden tests
    of this file and of test_mixed_precision.py fail (every path test of the flags reduction, 68 tile shapes, the planted rows on all
    6 paths that run it, band passes, clocked bands, prepared calls, the deep fix-ups, tiny x, the three other calls), and 2 of
    test_plan_exact.py now that it masks no sign;
  * the `+ 0` dropped from the beta == 0 write of consume_tile_rows (`beta == 0 ? alpha * acc : alpha * acc + beta * y`): 185
    zero-laden tests fail -- and 176 of the draws without zeros, which reach it through their rows without entries;
  * a lean row sum started from its first product (consume_tile_rows' `acc` entered as -0.0 where the row has entries, which is the
    same arithmetic): 198 zero-laden tests fail (the compact front end and the general kernel on 64 of 68 shapes, 69 path tests,
    32 tile shapes, the planted rows, prepared calls, tiny x, the deep fix-ups, the mixed calls) and 2 of test_plan_exact.py.

WIDE.  The draws above hold integers below about 2^21: the low 32 bits of every fp64 product, sum, carry and result are zero, and
every alpha and beta is an fp32 (and a bf16) number.  So every test that runs a dispatch path runs a third data kind as well,
axpby_model.wide_problem -- odd integers that fill the exactness budget, (1, 0), (-1.5, 0.5) and (-0.5, 0), the plain call included
--, and the path table and the prepared calls run alpha, beta = 1 + 2^-30, -(1 + 2^-29) (fp32: 1 + 2^-12, -(1 + 2^-11)) on the narrow
draw wherever the model's bound admits them (Problem.wide_scalars: computed, not listed; the plain mspmv_csrmv_* entry point takes
no alpha or beta, so it has no scalars to widen and runs the wide DATA instead).  WUSED lists the wide problems;
tests/test_axpby_model.py asserts on the CPU that at least 95 % of their results, and in fp64 at least 90 % of the running sums of
every row longer than a tile taken at every 1792nd and 2816th entry, have a non-zero low half.

Sensitivity of the wide data, each a one-line change of the fp64 instantiations built once and run once on one MI355X against the
parent commit's test_axpby_exact.py, test_spmm_forms.py, test_forward_progress.py, test_plan_exact.py and test_mixed_precision.py
and against this commit's (failing tests: parent's files / these files; the unchanged library passes all):
  * lb_publish handing rec_store p0 = 0: 147 / 161.  p0 is the HIGH word of the double: the sum is gone, and the parent sees it.
  * the same with p1 = 0, the LOW word: 48 / 116 (this file 10 / 64, test_plan_exact.py 0 / 7).  What the parent sees it with: the
    draws scaled to the smallest subnormal, whose integers then sit in the low word -- they run on the path table and the deep
    fix-ups only -- and the tolerance tests on real data (2^-21 of a carry is far outside the strict bound).
  * the carries read by fixup_kernel and fixup_onepass_kernel passed through (float): 125 / 253 (this file 35 / 160); the parent
    again by the flush of the subnormal draws and on real data.
  * alpha passed through (float) in csrmv_call<double>: 0 / 1.  Only the plans call it, and with more than one band alpha is applied
    by the fold: test_plan_exact.py::test_plans_are_exact_with_scalars_that_fill_the_significand[f64-1] fails.  The same cast where
    the entry points fill Params (csrmv_call_mv): 0 / 200 -- 187 path tests and 12 prepared ones of this file, 1 of test_plan_exact.py.
  * the column-band passes' `c.value += carry_out->value` with the low 8 bits of the double cleared: 0 / 6
    (test_forced_band_passes_equal_the_model, fp64, the shapes whose rows cross tiles).
  (the slot form's carry: tests/test_spmm_forms.py.)

Measured on one MI355X: the 1444 tests of this file take 20.1 s, 15.5 s at the parent commit (the same tests without the wide data).

Forms are forced with the development setters (include/mspmv_dev.h) the way tests/test_gpu_parity.py, test_band_passes.py and
test_tdm.py force them, and every form a test claims is asserted to have run (launch_info, band_passes, clocked_bands, the launch
log).  PROBLEMS / USED list every (matrix, pair) of this file: tests/test_axpby_model.py checks the exactness bound on each of them
on the CPU, so an edited shape cannot silently turn an exact test into a rounding-dependent one; ZUSED lists the zero-laden ones, for
which it also checks the census of planted rows and the domain of the sign rule.
"""
import functools

import numpy as np
import pytest

import axpby_model as A
from axpby_model import PAIRS

torch = pytest.importorskip("torch")
import test_gpu_parity as T          # noqa: E402 - PATHS, SHAPES, COMPACT_SHAPES, the M fixture
import test_tdm as TDM               # noqa: E402 - its SHAPES, _clocked, _reset
from test_gpu_parity import M        # noqa: E402,F401 - (fixture)
from test_mixed_precision import off_by_one   # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"f32": (np.float32, 4), "f64": (np.float64, 8)}
PRECS = ["f32", "f64"]
# beta == 0 with alpha < 0: alpha * (+0) is -0.0, which the "+ 0" of the definition turns into +0.0 on a row without entries (no
# pair of PAIRS has alpha < 0 with beta == 0, and with beta != 0 the non-zero beta * y0 hides the sign of alpha * 0)
NEG_ALPHA_ZERO_BETA = (-0.5, 0)
ALL_PAIRS = PAIRS + [NEG_ALPHA_ZERO_BETA]
NO_FUSED, TWO_LAUNCH = 16, 0x40000000


# ---------------------------------------------------------------------------------------------------------------- the problems

def _tile_grid(ipt):
    def make(rng):                                  # the matrix of test_gpu_parity.test_every_compiled_tile_shape
        lens = np.minimum((rng.pareto(1.1, 20000) * 2).astype(np.int64), 50000)
        lens[7777] = 90000
        return 20000, 20000, lens
    return make, 256 * 100 + ipt


# fix-up depth (item d): rows + nnz just above FIX_CHUNK (512) tiles of the large-problem shape -- 256 x 11 items in fp32, 256 x 7
# in fp64 at this size -- so that the multi-level fix-up needs a second level (asserted from launch_info where it is used)
DEEP_NNZ = {"f32": 1_445_000, "f64": 920_000}


def _deep_one_row(nnz):
    def make(rng):                                  # one row holds nearly everything: every tile carries into the same key
        lens = np.zeros(4001, np.int64); lens[::100] = 1; lens[2000] = nnz
        return 4001, 5000, lens
    return make


def _deep_long_rows(nnz):
    def make(rng):                                  # rows of 3000-6000: a few carries on each row
        lens = rng.integers(3000, 6001, nnz // 4500)
        return lens.size, 5000, lens
    return make


def _planted(tile_items):
    """item f: short rows, a stretch of empty rows wider than a tile, a giant row between two short ones -- and one row made to END
    exactly on the tile boundary at merge-path diagonal 2 * tile_items (row r ends at diagonal (r + 1) + row_offsets[r + 1])"""
    def make(rng):
        rows, g = 12000, 6000
        lens = rng.integers(0, 7, rows).astype(np.int64)
        lens[2000:5800] = 0                          # (more than a tile of row ends)
        lens[g - 1], lens[g], lens[g + 1] = 2, 40000, 3
        lens[0], lens[rows - 1] = 4, 5
        ends = np.arange(1, rows + 1) + np.cumsum(lens)
        d = 2 * tile_items
        r = int(np.searchsorted(ends, d, side="right")) - 1
        assert 0 < r < 2000
        lens[r] += d - ends[r]
        return rows, 3000, lens
    return make


def kind_ii_lengths(tile_items):
    """the lengths of the kind-(ii) rows planted for a tile of 256 x IPT items (NPT = the products a thread stages): inside one
    thread, across two threads of a wave, across waves, across tiles"""
    npt = (tile_items // 256 // 4 + 1) * 4
    return [1, 2, npt - 1, 2 * npt + 1, 64 * npt + 3, tile_items + 5]


PLANTED_ZERO_ROWS = [6100 + 37 * j for j in range(18)]      # (behind the giant row: the row made to end on a tile boundary stays)


def _planted_zero(tile_items):
    """_planted with rows whose products are all -0.0 (kind (ii)) of every length of kind_ii_lengths, three of each"""
    base = _planted(tile_items)

    def make(rng):
        rows, cols, lens = base(rng)
        want = kind_ii_lengths(tile_items)
        for j, r in enumerate(PLANTED_ZERO_ROWS):
            lens[r] = want[j % len(want)]
        return rows, cols, lens, {r: A.KIND_II for r in PLANTED_ZERO_ROWS}
    return make


def planted_rows(csr, tile_items):
    """label -> row of the rows item f plants a non-finite y0 at"""
    off = csr.row_offsets.astype(np.int64)
    ends = np.arange(1, csr.rows + 1) + off[1:]
    on_boundary = np.flatnonzero(ends == 2 * tile_items)
    assert on_boundary.size == 1 and off[on_boundary[0] + 1] > off[on_boundary[0]]
    rows = {"first": 0, "last": csr.rows - 1, "empty": 4000, "before_giant": 5999, "giant": 6000, "after_giant": 6001,
            "ends_on_tile_boundary": int(on_boundary[0])}
    assert off[4001] == off[4000] and off[6001] - off[6000] == 40000
    return rows


def _tiny_x(cols, rows, hi):
    return lambda rng: (rows, cols, rng.integers(0, hi, rows))


TINY_COLS = [1, 512, 513, 1024, 1025]               # the LDS copy of x and its edges (test_tiny_x_is_gathered_from_lds)
TINY_ROWS = [(3001, 9), (50003, 40)]
PLANTED_TILES = [256 * 7, 256 * 11]                 # the tile sizes the paths of item f run

# label -> (lambda rng: (rows, cols, lens), seed, vmax, xmax)
PROBLEMS = {}
for _n, _f in T.COMPACT_SHAPES.items():
    PROBLEMS["parity:" + _n] = (_f, sum(map(ord, _n)), 2, 3)
for _ipt in (7, 11):
    PROBLEMS[f"tile_grid:{_ipt}"] = _tile_grid(_ipt) + (2, 3)
for _p, _nnz in DEEP_NNZ.items():
    PROBLEMS[f"deep_one_row:{_p}"] = (_deep_one_row(_nnz), 41, 1, 1)          # (rows longer than 200 000: values and x of +-1)
    PROBLEMS[f"deep_long_rows:{_p}"] = (_deep_long_rows(_nnz), 42, 1, 1)
for _n in ("giant_row", "mostly_empty", "ragged_tail"):
    PROBLEMS["tdm:" + _n] = (TDM.SHAPES[_n], len(_n) * 7, 2, 3)
for _t in PLANTED_TILES:
    PROBLEMS[f"planted:{_t}"] = (_planted(_t), 43, 2, 3)
    PROBLEMS[f"planted_zero:{_t}"] = (_planted_zero(_t), 44, 2, 3)
for _c in TINY_COLS:
    for _r, _h in TINY_ROWS:
        PROBLEMS[f"tiny_x:{_c}:{_r}"] = (_tiny_x(_c, _r, _h), _c, 2, 3)

# label -> the pairs some test below runs on it, per precision it runs in (filled in next to each test)
USED = {}


def uses(labels, pairs, precs=PRECS):
    for label in labels:
        assert label in PROBLEMS, label
        for prec in precs:
            USED.setdefault((label, prec), set()).update(pairs)


# the zero-laden draw and its scalings (axpby_model.scale_exponents)
ZEROS, SCALED = "zeros", ["zeros@bottom", "zeros@bottom_stored", "zeros@top"]
# label, precision, data -> the pairs the zero-laden tests run (tests/test_axpby_model.py: census, domain, bound)
ZUSED = {}
# what the census of a problem must count besides what every shape must hold (label prefix -> keys; {tile}: the label's tile size)
CENSUS_MUST = {"planted_zero:": ["kind_ii_crosses:{tile}"], "deep_long_rows:": ["kind_iii_crosses:1792", "kind_iii_crosses:2816"],
               "deep_one_row:": ["kind_ii_crosses:1792", "kind_ii_crosses:2816"]}


# the wide draw (axpby_model.wide_problem): odd magnitudes that fill the exactness budget, so that both halves of every fp64 number
# on the way -- products, sums, carries, records, results -- hold bits; the pairs it runs with on every dispatch path
WIDE = "wide"
WIDE_RUN = [(1, 0), (-1.5, 0.5), NEG_ALPHA_ZERO_BETA]
# label, precision -> the pairs the wide draw runs (tests/test_axpby_model.py: the bound, the share of results and of running sums
# of long rows with a non-zero low half)
WUSED = {}


def wuses(labels, pairs=WIDE_RUN, precs=PRECS):
    for label in labels:
        assert label in PROBLEMS, label
        for prec in precs:
            WUSED.setdefault((label, prec), set()).update(pairs)


def uses_wide_scalars(labels, precs=PRECS):
    """axpby_model.WIDE_PAIRS (alpha, beta no fp32 / no bf16 numbers) on the NARROW draw: their granule is 2^-30 (2^-12), so a row
    may hold sum |v*x| < 2^22 (< 4095).  Whether a problem qualifies is Problem.fits(), the model's own bound, computed -- not a
    list kept by hand; tests/test_axpby_model.py checks it and that every group of tests keeps problems that qualify."""
    for prec in precs:
        uses(labels, A.WIDE_PAIRS[np.dtype(DT[prec][0])], [prec])


def zuses(labels, pairs, precs=PRECS, data=(ZEROS,)):
    for label in labels:
        assert label in PROBLEMS, label
        for prec in precs:
            for d in data:
                ZUSED.setdefault((label, prec, d), set()).update(pairs)


class Problem:
    def __init__(self, label, prec, data="nonzero"):
        make, seed, vmax, xmax = PROBLEMS[label]
        rng = np.random.default_rng(seed)
        shape = make(rng)
        rows, cols, lens = shape[:3]
        self.label, self.prec, self.data = label, prec, data
        self.dtype, self.vb = DT[prec]
        self.scale = 0
        if data == "nonzero":
            self.base = A.integer_problem(rng, rows, cols, np.asarray(lens, np.int64), self.dtype, vmax=vmax, xmax=xmax)
            self.csr, self.x, self.y0 = self.base
        elif data == WIDE:
            self.base = A.wide_problem(rng, rows, cols, np.asarray(lens, np.int64), self.dtype)
            self.csr, self.x, self.y0 = self.base
        else:
            # base: the unscaled integers and zeros the model computes on; csr, x, y0: what the device gets
            self.base = A.zero_problem(rng, rows, cols, np.asarray(lens, np.int64), self.dtype, vmax=vmax, xmax=xmax,
                                       forced=shape[3] if len(shape) > 3 else None)
            zeros, _, which = data.partition("@")
            assert zeros == ZEROS
            ev, ex = A.scale_exponents(self.dtype, which) if which else (0, 0)
            self.csr, self.x, self.y0 = A.scaled(self.base, ev, ex)
            self.scale = ev + ex
        self._want = {}

    def want(self, alpha, beta):
        """the model's y: computed once per pair, shared by every test on this problem, never written to"""
        if (alpha, beta) not in self._want:
            w = A.model(*self.base, alpha, beta, scale=self.scale)
            w.setflags(write=False)
            self._want[(alpha, beta)] = w
        return self._want[(alpha, beta)]

    def fits(self, alpha, beta):
        """the model's bound for this pair: every row's quotient below 2^24 (2^53) granules"""
        return A.quotient(*self.base, alpha, beta) < A.LIMIT[np.dtype(self.dtype)]

    def wide_scalars(self):
        """the pairs of axpby_model.WIDE_PAIRS this problem is exact with (fp32: none where a row's sum |v*x| reaches 4095)"""
        return [p for p in A.WIDE_PAIRS[np.dtype(self.dtype)] if self.fits(*p)]


@functools.lru_cache(maxsize=None)
def problem(label, prec, data="nonzero"):
    return Problem(label, prec, data)


# ------------------------------------------------------------------------------------------------------------------ on the GPU

class OnDevice:
    """a problem's arrays on the device (optionally all one element off a 16-byte boundary) and the calls on them"""

    def __init__(self, Mod, P, shift=False):
        self.M, self.P = Mod, P
        self.place = off_by_one if shift else (lambda t: t)
        self.tdt = torch.float32 if P.vb == 4 else torch.float64
        c = P.csr
        self.val, self.off, self.col, self.x = (self.place(torch.from_numpy(np.ascontiguousarray(a)).cuda())
                                                for a in (c.values, c.row_offsets, c.column_indices, P.x))

    def workspace(self, prepare=False, garbage=False):
        ws = self.M.CsrMVWorkspace(self.P.csr.rows, self.P.csr.nnz, self.tdt)
        if garbage:
            ws.buffer.random_(0, 255)               # (the hints of the one-launch kernel: every byte pattern, as in test_gpu_parity)
        return ws.prepare(self.off) if prepare else ws

    def axpby(self, ws, alpha, beta, y0=None, **kw):
        """mspmv_csrmv_axpby_* (on a prepared workspace: mspmv_csrmv_prepared_*) on a copy of y0"""
        c = self.P.csr
        y = self.place(torch.from_numpy(np.array(self.P.y0 if y0 is None else y0, copy=True)).cuda())
        self.M.csrmv(self.val, self.off, self.col, self.x, y=y, num_cols=c.cols, workspace=ws, alpha=float(alpha), beta=float(beta), **kw)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    def plain(self, ws):
        """mspmv_csrmv_* into a y filled with NaN"""
        c = self.P.csr
        y = self.place(torch.full((c.rows,), float("nan"), dtype=self.tdt, device="cuda"))
        self.M.csrmv(self.val, self.off, self.col, self.x, y=y, num_cols=c.cols, workspace=ws)
        torch.cuda.synchronize()
        return y.cpu().numpy()


def same(got, want, *where):
    gb, wb = A.bits(got), A.bits(want)
    if not np.array_equal(gb, wb):
        bad = np.flatnonzero(gb != wb)
        raise AssertionError(f"{where}: {bad.size} of {gb.size} rows differ on the bits; first rows {bad[:5].tolist()}: "
                             f"got {np.asarray(got)[bad[:5]].tolist()}, model {np.asarray(want)[bad[:5]].tolist()}")


def both_calls(D, pairs, *where, garbage=False):
    """every pair: the call on a fresh workspace (no hints: every tile searches) and again on it (hints now right) equal the model"""
    ws = None
    for alpha, beta in pairs:
        ws = D.workspace(garbage=garbage)
        for call in ("first", "second"):
            same(D.axpby(ws, alpha, beta), D.P.want(alpha, beta), *where, (alpha, beta), call + " call")
    return ws


def zero_calls(D, pairs, *where, garbage=False):
    """both_calls, and the plain entry point (the AXPBY = false instantiations) on a fresh workspace and on the hints"""
    P = D.P
    ws = both_calls(D, pairs, *where, P.data, garbage=garbage)
    same(D.plain(D.workspace(garbage=garbage)), P.want(1, 0), *where, P.data, "plain call, fresh workspace")
    same(D.plain(ws), P.want(1, 0), *where, P.data, "plain call on hints")
    return ws


# ------------------------------------------------------------------------------------------------- a. every path, every shape

uses(["parity:" + n for n in T.SHAPES], ALL_PAIRS)
uses_wide_scalars(["parity:" + n for n in T.SHAPES])
wuses(["parity:" + n for n in T.SHAPES])


@pytest.mark.parametrize("shape", sorted(T.SHAPES))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(T.PATHS))
def test_every_path_equals_the_model(M, shape, prec, path):
    """All 17 dispatch paths of test_gpu_parity.PATHS: the alpha/beta call equals the model for every pair, first call and call on
    hints; (1, 0) through the AXPBY kernels has the bits of the plain call (the two template halves agree).  Exact data make the
    atomic fix-up order-independent, so it is held to the bits as well.  Then alpha and beta that fill the significand
    (axpby_model.WIDE_PAIRS, where the rows are short enough for them) and the wide draw, plain call included."""
    P = problem("parity:" + shape, prec)
    try:
        M.set_tuning(P.vb, 0, 0, T.PATHS[path])
        assert M.launch_info(P.csr.rows, P.csr.nnz, P.vb)["flags"] == T.PATHS[path]
        D = OnDevice(M, P)
        ws = both_calls(D, ALL_PAIRS, shape, prec, path)
        same(D.plain(D.workspace()), P.want(1, 0), shape, prec, path, "plain call, fresh workspace")
        plain = D.plain(ws)
        same(plain, P.want(1, 0), shape, prec, path, "plain call on hints")
        same(D.axpby(ws, 1, 0), plain, shape, prec, path, "(1, 0) through the AXPBY kernels against the plain call")
        both_calls(D, P.wide_scalars(), shape, prec, path, "wide scalars")
        zero_calls(OnDevice(M, problem("parity:" + shape, prec, WIDE)), WIDE_RUN, shape, prec, path)
    finally:
        M.set_tuning(P.vb)


uses(["parity:" + n for n in T.COMPACT_SHAPES], ALL_PAIRS)
wuses(["parity:" + n for n in T.COMPACT_SHAPES])


@pytest.mark.parametrize("shape", sorted(T.COMPACT_SHAPES))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("compact", [0, -1], ids=["compact_front_end", "general_kernel"])
def test_compact_front_end_and_general_kernel_equal_the_model(M, shape, prec, compact):
    """The default path of a small problem: behind the compact front end the first call (garbage hints) runs the general body and
    the second the fast lane -- both under AXPBY --, with set_compact_tiles(-1) the general kernel alone."""
    P = problem("parity:" + shape, prec)
    try:
        M.set_compact_tiles(compact)
        D = OnDevice(M, P)
        ws = both_calls(D, ALL_PAIRS, shape, prec, compact, garbage=True)
        same(D.plain(ws), P.want(1, 0), shape, prec, compact, "plain call on hints")
        zero_calls(OnDevice(M, problem("parity:" + shape, prec, WIDE)), WIDE_RUN, shape, prec, compact, garbage=True)
    finally:
        M.set_compact_tiles(0)


# --------------------------------------------------------------------------------------------------------- b. prepared calls

PREPARED_SHAPES = ["power_law", "giant_plus_sprinkle", "leading_trailing_empty"]
PREPARED_FLAGS = {"one_launch_small_shape": 0, "one_launch_large_shape": 16, "classic_small_shape": TWO_LAUNCH, "classic_three_launch": TWO_LAUNCH | 16}
uses(["parity:" + n for n in PREPARED_SHAPES], ALL_PAIRS)
uses_wide_scalars(["parity:" + n for n in PREPARED_SHAPES])
wuses(["parity:" + n for n in PREPARED_SHAPES])


@pytest.mark.parametrize("shape", PREPARED_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(PREPARED_FLAGS))
def test_prepared_calls_equal_the_model(M, shape, prec, path):
    """CsrMVWorkspace.prepare + mspmv_csrmv_prepared_*: (1, 0) takes the plain kernels, every other pair the AXPBY set; the narrow
    draw with every pair and the wide scalars it is exact with, the wide draw with WIDE_RUN and the plain prepared call"""
    vb = DT[prec][1]
    try:
        M.set_tuning(vb, 0, 0, PREPARED_FLAGS[path])
        for P in (problem("parity:" + shape, prec), problem("parity:" + shape, prec, WIDE)):
            D = OnDevice(M, P)
            ws = D.workspace(prepare=True)
            assert ws.is_prepared_for(D.off, P.csr.rows, P.csr.nnz, D.tdt)          # (csrmv then calls the prepared entry point)
            for alpha, beta in (WIDE_RUN if P.data == WIDE else ALL_PAIRS + P.wide_scalars()):
                for call in ("first", "second"):
                    same(D.axpby(ws, alpha, beta), P.want(alpha, beta), shape, prec, path, P.data, (alpha, beta), call + " prepared call")
            if P.data == WIDE:
                same(D.plain(ws), P.want(1, 0), shape, prec, path, P.data, "plain prepared call")
    finally:
        M.set_tuning(vb)


# -------------------------------------------------------------------------------------------- c. tile shapes and alignment

TILE_PAIRS = [(-1.5, 0.5), (2, 0)]
TILE_FLAGS = [0, 2, 4, 16, 18, 20, 24, 48, 80, 128, 144, 0xF000010, 0x3000010, 0x20000010, 0x10000010, 0x40000000, 0x40000010, 0x4F000010, 0x60000010]
uses(["tile_grid:7", "tile_grid:11"], TILE_PAIRS)
wuses(["tile_grid:7", "tile_grid:11"])


@pytest.mark.parametrize("vb,block,ipt", [(4, 256, 7), (4, 256, 11), (8, 256, 7), (8, 256, 11)])
@pytest.mark.parametrize("flags", TILE_FLAGS)
def test_every_compiled_tile_shape_equals_the_model(M, vb, block, ipt, flags):
    """the (value bytes, block, items per thread) x flags grid of test_gpu_parity.test_every_compiled_tile_shape"""
    P = problem(f"tile_grid:{ipt}", "f32" if vb == 4 else "f64")
    try:
        M.set_tuning(vb, block, ipt, flags)
        info = M.launch_info(P.csr.rows, P.csr.nnz, vb)
        assert (info["block_threads"], info["items_per_thread"], info["flags"]) == (block, ipt, flags)
        both_calls(OnDevice(M, P), TILE_PAIRS, vb, block, ipt, hex(flags))
        zero_calls(OnDevice(M, problem(f"tile_grid:{ipt}", P.prec, WIDE)), WIDE_RUN, vb, block, ipt, hex(flags))
    finally:
        M.set_tuning(vb)


UNALIGNED_PAIRS = [(-1.5, 0.5), (2, 0), (0, -2)]
uses(["parity:power_law", "parity:one_giant_row"], UNALIGNED_PAIRS)
wuses(["parity:power_law", "parity:one_giant_row"])


@pytest.mark.parametrize("shape", ["power_law", "one_giant_row"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("flags", [0, 16, TWO_LAUNCH | 16])
def test_unaligned_arrays_equal_the_model(M, shape, prec, flags, capfd):
    """every array one element off a 16-byte boundary: the dword-per-lane tile_kernel is reached by alignment, not by a flag"""
    P = problem("parity:" + shape, prec)
    try:
        M.set_tuning(P.vb, 0, 0, flags)
        D = OnDevice(M, P, shift=True)
        assert all(t.data_ptr() % 16 for t in (D.val, D.off, D.col, D.x))
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, flags, "logged call")
        log = capfd.readouterr().out
        assert "tile_kernel<<<" in log and "tile_kernel_vec" not in log and "tile_kernel_snap" not in log, log
        both_calls(D, UNALIGNED_PAIRS, shape, prec, flags, "unaligned")
        W = OnDevice(M, problem("parity:" + shape, prec, WIDE), shift=True)
        assert all(t.data_ptr() % 16 for t in (W.val, W.off, W.col, W.x))
        zero_calls(W, WIDE_RUN, shape, prec, flags, "unaligned")
    finally:
        M.set_tuning(P.vb)


# ------------------------------------------------------- d. fix-up of more than one level, many carries into one row

DEEP_PAIRS = [(-1.5, 0.5), (2, 0), (0, -2)]
DEEP_PATHS = {"multilevel_fix": 0x90, "classic_multilevel_fix": TWO_LAUNCH | 0x90, "onepass_fix": TWO_LAUNCH | 16, "atomic_fix": 0x12,
              "one_launch_records_taken": 16, "one_launch_records_recomputed": 16}
for _p in PRECS:
    uses([f"deep_one_row:{_p}", f"deep_long_rows:{_p}"], DEEP_PAIRS, [_p])
    wuses([f"deep_one_row:{_p}", f"deep_long_rows:{_p}"], WIDE_RUN, [_p])


@pytest.mark.parametrize("matrix", ["deep_one_row", "deep_long_rows"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(DEEP_PATHS))
def test_deep_fixup_and_many_carries_per_row_equal_the_model(M, matrix, prec, path):
    """More than FIX_CHUNK = 512 tiles, so the multi-level fix-up runs a second level (alpha must be applied once, not per level) and
    the one-pass fix-up's blocks look back across chunks; every tile carries into one key, or a few tiles into each.  The
    one-launch kernel adds the carries itself: taken from the published records, or (set_record_polls(-1)) recomputed."""
    P = problem(f"{matrix}:{prec}", prec)
    try:
        M.set_tuning(P.vb, 0, 0, DEEP_PATHS[path])
        if path == "one_launch_records_recomputed":
            M.set_record_polls(-1)
        info = M.launch_info(P.csr.rows, P.csr.nnz, P.vb)
        assert info["num_tiles"] > info["fixup_chunk"]
        if "multilevel" in path:
            assert info["fixup_levels"] >= 2, info
            # the smallest such size: one chunk of tiles fewer needs a single level
            assert M.launch_info(P.csr.rows, P.csr.nnz - info["tile_items"] * 8, P.vb)["fixup_levels"] == 1
        elif path.startswith("one_launch"):
            assert info["fixup_levels"] == 0 and info["snap_head_max"] > 0
        else:
            assert info["fixup_levels"] == 1
        D = OnDevice(M, P)
        both_calls(D, DEEP_PAIRS, matrix, prec, path)
        if path == "one_launch_records_recomputed":
            # the episode counter of the workspace (launch_info: diag_offset) moves when a tile computed a sum itself instead of taking
            # the record, and only then: tests/test_forward_progress.py
            ws = D.workspace(); ws.buffer.zero_()
            episodes = lambda: int(ws.buffer[info["diag_offset"] + 4: info["diag_offset"] + 8].view(torch.int32).item())
            before = episodes()
            for alpha, beta in DEEP_PAIRS:
                same(D.axpby(ws, alpha, beta), P.want(alpha, beta), matrix, prec, path, (alpha, beta), "counted call")
            assert episodes() != before, "no tile recomputed a partial sum: the form this case is about did not run"
        # the wide draw on the same shape, forced form and poll budget: every carry, record and group record of the giant row (of
        # the long rows) now holds bits in both halves of the double
        W = OnDevice(M, problem(f"{matrix}:{prec}", prec, WIDE))
        zero_calls(W, WIDE_RUN, matrix, prec, path)
        if path == "one_launch_records_recomputed":      # ... and the wide sums too were recomputed, not taken: the counter again
            ws = W.workspace(); ws.buffer.zero_()
            before = episodes()
            for alpha, beta in WIDE_RUN:
                same(W.axpby(ws, alpha, beta), W.P.want(alpha, beta), matrix, prec, path, WIDE, (alpha, beta), "counted call")
            assert episodes() != before, "no tile recomputed a partial sum of the wide draw"
    finally:
        M.set_tuning(P.vb); M.set_record_polls(0)


# ---------------------------------------------------------------- e. column-band passes and the clocked form

BAND_SHAPES = ["giant_row", "mostly_empty", "ragged_tail"]
uses(["tdm:" + n for n in BAND_SHAPES], ALL_PAIRS)
wuses(["tdm:" + n for n in BAND_SHAPES])


def _only_tile_kernel_vec(log):
    names = [line.split("<<<")[0].replace("mspmv: ", "") for line in log.splitlines() if line.startswith("mspmv: ")]
    return "tile_kernel_vec" in names and "tile_kernel_snap" not in names and "tile_kernel" not in names


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("passes", [2, 3, 8])
def test_forced_band_passes_equal_the_model(M, shape, prec, passes, capfd):
    """run_band_passes: pass 0 applies the caller's beta, every later pass adds with beta = 1 (p.beta = b == 0 ? s_beta0 : 1)"""
    P = problem("tdm:" + shape, prec)
    c = P.csr
    try:
        M.set_tuning(P.vb, 256, 11, NO_FUSED); M.set_tdm(P.vb, -1); M.set_band_passes(P.vb, passes)       # test_band_passes.forced_shape
        assert M.band_passes(c.rows, c.cols, c.nnz, P.vb) == passes and M.clocked_bands(c.rows, c.cols, c.nnz, P.vb) == (0, 0)
        D = OnDevice(M, P)
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, passes, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        both_calls(D, ALL_PAIRS, shape, prec, passes, "band passes")
        W = OnDevice(M, problem("tdm:" + shape, prec, WIDE))
        capfd.readouterr()
        same(W.axpby(W.workspace(), -1.5, 0.5, debug_synchronous=True), W.P.want(-1.5, 0.5), shape, prec, passes, WIDE, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        zero_calls(W, WIDE_RUN, shape, prec, passes, "band passes")
    finally:
        TDM._reset()


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("clock", [(0, 0, 0), (1, 1, 13)], ids=["default_clock", "fast_clock_narrow_bands"])
def test_clocked_bands_equal_the_model(M, shape, prec, clock, capfd):
    """the clock-scheduled form (csrc/mspmv_tdm.hpp) with alpha and beta, against an oracle"""
    P = problem("tdm:" + shape, prec)
    c = P.csr
    try:
        TDM._clocked(P.vb, 11, *clock)
        assert M.band_passes(c.rows, c.cols, c.nnz, P.vb) == 3
        bands, band_cols = M.clocked_bands(c.rows, c.cols, c.nnz, P.vb)
        assert bands >= 1 and band_cols >= 1, "not a candidate for the clocked form: nothing here would test it"
        if clock[2]:
            assert band_cols == 1 << clock[2]
        D = OnDevice(M, P)
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, clock, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        both_calls(D, ALL_PAIRS, shape, prec, clock, "clocked bands")
        W = OnDevice(M, problem("tdm:" + shape, prec, WIDE))
        capfd.readouterr()
        same(W.axpby(W.workspace(), -1.5, 0.5, debug_synchronous=True), W.P.want(-1.5, 0.5), shape, prec, clock, WIDE, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        zero_calls(W, WIDE_RUN, shape, prec, clock, "clocked bands")
    finally:
        TDM._reset()


# -------------------------------------------------------------------------- f. what y may and may not be read for

def _forced_passes_3(Mod, vb):
    Mod.set_tuning(vb, 256, 11, NO_FUSED); Mod.set_tdm(vb, -1); Mod.set_band_passes(vb, 3)


Y_PATHS = {name: (lambda Mod, vb, f=T.PATHS[name]: Mod.set_tuning(vb, 0, 0, f))
           for name in ("one_launch_small_shape", "one_launch_large_shape", "classic_three_launch", "classic_atomic_fix", "classic_multilevel_fix", "reference_walk")}
Y_PATHS["forced_passes_3"] = _forced_passes_3

BETA0_PAIRS = [(1, 0), (2, 0), NEG_ALPHA_ZERO_BETA]
# rows without entries in every position: inside tiles of short rows, as whole tile ranges, around a giant row, and nnz == 0
BETA0_SHAPES = ["power_law", "all_empty", "leading_trailing_empty", "giant_row_between_empties", "giant_plus_sprinkle"]
uses(["parity:" + n for n in BETA0_SHAPES], BETA0_PAIRS)


def poisoned(n, dtype):
    """NaN, +Inf, -Inf, -0.0, 1e38, repeating: whatever reads it shows in the result"""
    return np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 1e38], dtype), n)


@pytest.mark.parametrize("shape", BETA0_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(Y_PATHS))
def test_beta_zero_never_reads_y(M, shape, prec, path):
    """beta == 0: y is written, not read -- rows without entries, a matrix without nonzeros and the carries' rows included -- and a
    row without entries is +0.0 whatever the sign of alpha"""
    P = problem("parity:" + shape, prec)
    try:
        Y_PATHS[path](M, P.vb)
        D = OnDevice(M, P)
        for alpha, beta in BETA0_PAIRS:
            ws = D.workspace()
            for call in ("first", "second"):
                same(D.axpby(ws, alpha, beta, y0=poisoned(P.csr.rows, P.dtype)), P.want(alpha, beta), shape, prec, path, (alpha, beta), call + " call")
    finally:
        TDM._reset()


PLANTED_PAIRS = [p for p in PAIRS if p[1] != 0]
uses([f"planted:{t}" for t in PLANTED_TILES], PLANTED_PAIRS)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(Y_PATHS))
def test_beta_nonzero_reads_exactly_its_own_row_of_y(M, prec, path):
    """beta != 0: NaN / +Inf / -Inf planted in y0 at an empty row, the rows around a giant row and the giant row, the first and last
    row and a row that ends exactly on a tile boundary come out non-finite at exactly those rows -- NaN as NaN, an infinity as
    beta * itself --; every other row equals the model on the bits"""
    vb = DT[prec][1]
    try:
        Y_PATHS[path](M, vb)
        tile_items = M.launch_info(12000, 70000, vb)["tile_items"]
        assert tile_items in PLANTED_TILES, tile_items
        P = problem(f"planted:{tile_items}", prec)
        assert M.launch_info(P.csr.rows, P.csr.nnz, vb)["tile_items"] == tile_items
        rows = planted_rows(P.csr, tile_items)
        y0 = P.y0.copy()
        for k, r in enumerate(sorted(rows.values())):
            y0[r] = (np.nan, np.inf, -np.inf)[k % 3]
        at = np.zeros(P.csr.rows, bool); at[list(rows.values())] = True
        D = OnDevice(M, P)
        for alpha, beta in PLANTED_PAIRS:
            ws = D.workspace()
            for call in ("first", "second"):
                y = D.axpby(ws, alpha, beta, y0=y0)
                assert np.array_equal(~np.isfinite(y), at), (prec, path, (alpha, beta), call, np.flatnonzero(~np.isfinite(y) != at)[:8].tolist(), rows)
                assert np.array_equal(np.isnan(y), np.isnan(y0))
                inf = np.isinf(y0)
                same(y[inf], (P.dtype(beta) * y0[inf]).astype(P.dtype), prec, path, (alpha, beta), call, "planted infinities")
                same(y[~at], P.want(alpha, beta)[~at], prec, path, (alpha, beta), call + " call, rows nothing was planted at")
    finally:
        TDM._reset()


# ------------------------------------------------------------------------------------------------------------- g. tiny x

TINY_PAIRS = [(-1.5, 0.5), (2, 0)]
uses([f"tiny_x:{c}:{r}" for c in TINY_COLS for r, _ in TINY_ROWS], TINY_PAIRS)
wuses([f"tiny_x:{c}:{r}" for c in TINY_COLS for r, _ in TINY_ROWS])


@pytest.mark.parametrize("cols", TINY_COLS)
@pytest.mark.parametrize("prec", PRECS)
def test_tiny_x_equals_the_model(M, cols, prec):
    """x of at most 4 KB is gathered from an LDS copy (and from memory with MSPMV_TUNE_NO_XLDS = 0x80000, or behind the compact front
    end): cols at the copy's edges, small- and large-problem kernel, as in test_gpu_parity.test_tiny_x_is_gathered_from_lds"""
    vb = DT[prec][1]
    for rows, _ in TINY_ROWS:
        P = problem(f"tiny_x:{cols}:{rows}", prec)
        D, W = OnDevice(M, P), OnDevice(M, problem(f"tiny_x:{cols}:{rows}", prec, WIDE))
        for flags in ("compact", 0, 0x80000, 16, 16 | 0x80000):
            try:
                M.set_compact_tiles(0 if flags == "compact" else -1)
                M.set_tuning(vb, 0, 0, 0 if flags == "compact" else flags)
                both_calls(D, TINY_PAIRS, cols, rows, prec, flags)
                zero_calls(W, WIDE_RUN, cols, rows, prec, flags)
            finally:
                M.set_tuning(vb); M.set_compact_tiles(0)


# ------------------------------------------------------------------------------------------------- z. the zero-laden draws
# The tests above again on axpby_model.zero_problem's data (same shapes, same forced forms, the same assertions that the form
# ran), plain and alpha / beta entry points, and -- every path, the deep fix-ups -- at both ends of the exponent range.

zuses(["parity:" + n for n in T.SHAPES], ALL_PAIRS)
zuses(["parity:" + n for n in T.SHAPES], A.SCALE_PAIRS, data=SCALED)


@pytest.mark.parametrize("shape", sorted(T.SHAPES))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(T.PATHS))
def test_every_path_equals_the_model_on_zeros_and_at_both_ends_of_the_range(M, shape, prec, path):
    """all 17 dispatch paths x shapes: the zero-laden draw with every pair, then scaled to subnormal products and sums (values and x
    normal), to subnormal stored values, and to the top of the range, with the pairs (1, 0), (-1.5, 0.5), (3, -5)"""
    try:
        vb = DT[prec][1]
        M.set_tuning(vb, 0, 0, T.PATHS[path])
        for data in [ZEROS] + SCALED:
            P = problem("parity:" + shape, prec, data)
            assert M.launch_info(P.csr.rows, P.csr.nnz, P.vb)["flags"] == T.PATHS[path]
            zero_calls(OnDevice(M, P), ALL_PAIRS if data == ZEROS else A.SCALE_PAIRS, shape, prec, path)
    finally:
        M.set_tuning(vb)


zuses(["parity:" + n for n in T.COMPACT_SHAPES], ALL_PAIRS)


@pytest.mark.parametrize("shape", sorted(T.COMPACT_SHAPES))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("compact", [0, -1], ids=["compact_front_end", "general_kernel"])
def test_compact_front_end_and_general_kernel_equal_the_model_on_zeros(M, shape, prec, compact):
    P = problem("parity:" + shape, prec, ZEROS)
    try:
        M.set_compact_tiles(compact)
        zero_calls(OnDevice(M, P), ALL_PAIRS, shape, prec, compact, garbage=True)
    finally:
        M.set_compact_tiles(0)


zuses(["parity:" + n for n in PREPARED_SHAPES], ALL_PAIRS)


@pytest.mark.parametrize("shape", PREPARED_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(PREPARED_FLAGS))
def test_prepared_calls_equal_the_model_on_zeros(M, shape, prec, path):
    P = problem("parity:" + shape, prec, ZEROS)
    try:
        M.set_tuning(P.vb, 0, 0, PREPARED_FLAGS[path])
        D = OnDevice(M, P)
        ws = D.workspace(prepare=True)
        assert ws.is_prepared_for(D.off, P.csr.rows, P.csr.nnz, D.tdt)
        for alpha, beta in ALL_PAIRS:
            for call in ("first", "second"):
                same(D.axpby(ws, alpha, beta), P.want(alpha, beta), shape, prec, path, (alpha, beta), call + " prepared call")
        same(D.plain(ws), P.want(1, 0), shape, prec, path, "plain prepared call")
    finally:
        M.set_tuning(P.vb)


TILE_ZERO_PAIRS = TILE_PAIRS + [NEG_ALPHA_ZERO_BETA]
zuses(["tile_grid:7", "tile_grid:11"], TILE_ZERO_PAIRS + [(1, 0)])


@pytest.mark.parametrize("vb,block,ipt", [(4, 256, 7), (4, 256, 11), (8, 256, 7), (8, 256, 11)])
@pytest.mark.parametrize("flags", TILE_FLAGS)
def test_every_compiled_tile_shape_equals_the_model_on_zeros(M, vb, block, ipt, flags):
    P = problem(f"tile_grid:{ipt}", "f32" if vb == 4 else "f64", ZEROS)
    try:
        M.set_tuning(vb, block, ipt, flags)
        info = M.launch_info(P.csr.rows, P.csr.nnz, vb)
        assert (info["block_threads"], info["items_per_thread"], info["flags"]) == (block, ipt, flags)
        zero_calls(OnDevice(M, P), TILE_ZERO_PAIRS, vb, block, ipt, hex(flags))
    finally:
        M.set_tuning(vb)


UNALIGNED_ZERO_PAIRS = UNALIGNED_PAIRS + [NEG_ALPHA_ZERO_BETA]
zuses(["parity:power_law", "parity:one_giant_row"], UNALIGNED_ZERO_PAIRS + [(1, 0)])


@pytest.mark.parametrize("shape", ["power_law", "one_giant_row"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("flags", [0, 16, TWO_LAUNCH | 16])
def test_unaligned_arrays_equal_the_model_on_zeros(M, shape, prec, flags, capfd):
    P = problem("parity:" + shape, prec, ZEROS)
    try:
        M.set_tuning(P.vb, 0, 0, flags)
        D = OnDevice(M, P, shift=True)
        assert all(t.data_ptr() % 16 for t in (D.val, D.off, D.col, D.x))
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, flags, "logged call")
        log = capfd.readouterr().out
        assert "tile_kernel<<<" in log and "tile_kernel_vec" not in log and "tile_kernel_snap" not in log, log
        zero_calls(D, UNALIGNED_ZERO_PAIRS, shape, prec, flags, "unaligned")
    finally:
        M.set_tuning(P.vb)


# deep_one_row: the giant row is the longest row, which zero_problem makes of kind (ii) -- every carry, record and group record of
# it is a zero; deep_long_rows: about a tenth of its rows are of kind (iii), cut by tiles (CENSUS_MUST)
DEEP_ZERO_PAIRS = DEEP_PAIRS + [NEG_ALPHA_ZERO_BETA]
DEEP_ZERO_PATHS = dict(DEEP_PATHS, one_launch_records_one_look=16)
for _p in PRECS:
    zuses([f"deep_one_row:{_p}", f"deep_long_rows:{_p}"], DEEP_ZERO_PAIRS + [(1, 0)], [_p])
    zuses([f"deep_one_row:{_p}", f"deep_long_rows:{_p}"], A.SCALE_PAIRS, [_p], data=SCALED)


@pytest.mark.parametrize("matrix", ["deep_one_row", "deep_long_rows"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(DEEP_ZERO_PATHS))
def test_deep_fixup_and_many_carries_per_row_equal_the_model_on_zeros_and_at_both_ends_of_the_range(M, matrix, prec, path):
    """the fix-up of more than one level, the one-pass and the atomic fix-up, the one-launch kernel's records taken, looked for once
    (set_record_polls(1)) and recomputed (-1: recompute_row_head): zero carries of a kind-(ii) giant row, kind-(iii) rows cut by
    tiles, subnormal carries and carries at the top of the range"""
    try:
        vb = DT[prec][1]
        M.set_tuning(vb, 0, 0, DEEP_ZERO_PATHS[path])
        M.set_record_polls({"one_launch_records_recomputed": -1, "one_launch_records_one_look": 1}.get(path, 0))
        for data in [ZEROS] + SCALED:
            P = problem(f"{matrix}:{prec}", prec, data)
            info = M.launch_info(P.csr.rows, P.csr.nnz, P.vb)
            assert info["num_tiles"] > info["fixup_chunk"]
            if "multilevel" in path:
                assert info["fixup_levels"] >= 2, info
            elif path.startswith("one_launch"):
                assert info["fixup_levels"] == 0 and info["snap_head_max"] > 0
            else:
                assert info["fixup_levels"] == 1
            zero_calls(OnDevice(M, P), DEEP_ZERO_PAIRS if data == ZEROS else A.SCALE_PAIRS, matrix, prec, path)
    finally:
        M.set_tuning(vb); M.set_record_polls(0)


zuses(["tdm:" + n for n in BAND_SHAPES], ALL_PAIRS)


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("passes", [2, 3, 8])
def test_forced_band_passes_equal_the_model_on_zeros(M, shape, prec, passes, capfd):
    """a band without a non-zero product of a row adds +0.0 with beta = 1: nothing a later pass adds may turn the sign round"""
    P = problem("tdm:" + shape, prec, ZEROS)
    c = P.csr
    try:
        M.set_tuning(P.vb, 256, 11, NO_FUSED); M.set_tdm(P.vb, -1); M.set_band_passes(P.vb, passes)
        assert M.band_passes(c.rows, c.cols, c.nnz, P.vb) == passes and M.clocked_bands(c.rows, c.cols, c.nnz, P.vb) == (0, 0)
        D = OnDevice(M, P)
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, passes, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        zero_calls(D, ALL_PAIRS, shape, prec, passes, "band passes")
    finally:
        TDM._reset()


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("clock", [(0, 0, 0), (1, 1, 13)], ids=["default_clock", "fast_clock_narrow_bands"])
def test_clocked_bands_equal_the_model_on_zeros(M, shape, prec, clock, capfd):
    P = problem("tdm:" + shape, prec, ZEROS)
    c = P.csr
    try:
        TDM._clocked(P.vb, 11, *clock)
        assert M.band_passes(c.rows, c.cols, c.nnz, P.vb) == 3
        bands, band_cols = M.clocked_bands(c.rows, c.cols, c.nnz, P.vb)
        assert bands >= 1 and band_cols >= 1, "not a candidate for the clocked form: nothing here would test it"
        D = OnDevice(M, P)
        capfd.readouterr()
        same(D.axpby(D.workspace(), -1.5, 0.5, debug_synchronous=True), P.want(-1.5, 0.5), shape, prec, clock, "logged call")
        assert _only_tile_kernel_vec(capfd.readouterr().out)
        zero_calls(D, ALL_PAIRS, shape, prec, clock, "clocked bands")
    finally:
        TDM._reset()


zuses([f"planted_zero:{t}" for t in PLANTED_TILES], ALL_PAIRS)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", sorted(Y_PATHS))
def test_planted_rows_of_negative_zero_products_equal_the_model(M, prec, path):
    """rows whose products are all -0.0, of 1, 2, NPT - 1, 2 NPT + 1, 64 NPT + 3 and tile + 5 products: inside one thread, across two
    threads of a wave, across waves, across tiles -- +0.0 (-0.0 only under t = -0.0 and a negative alpha), on every path"""
    vb = DT[prec][1]
    try:
        Y_PATHS[path](M, vb)
        for t in PLANTED_TILES:
            P = problem(f"planted_zero:{t}", prec, ZEROS)
            if M.launch_info(P.csr.rows, P.csr.nnz, vb)["tile_items"] == t:
                break
        else:
            pytest.fail(f"{path}: runs neither tile size of {PLANTED_TILES}")
        lens = np.diff(P.csr.row_offsets)[PLANTED_ZERO_ROWS]
        assert sorted(set(lens.tolist())) == sorted(kind_ii_lengths(t))
        zero_calls(OnDevice(M, P), ALL_PAIRS, prec, path, t)
    finally:
        TDM._reset()


zuses([f"tiny_x:{c}:{r}" for c in TINY_COLS for r, _ in TINY_ROWS], TINY_PAIRS + [NEG_ALPHA_ZERO_BETA, (1, 0)])


@pytest.mark.parametrize("cols", TINY_COLS)
@pytest.mark.parametrize("prec", PRECS)
def test_tiny_x_equals_the_model_on_zeros(M, cols, prec):
    vb = DT[prec][1]
    for rows, _ in TINY_ROWS:
        P = problem(f"tiny_x:{cols}:{rows}", prec, ZEROS)
        D = OnDevice(M, P)
        for flags in ("compact", 0, 0x80000, 16, 16 | 0x80000):
            try:
                M.set_compact_tiles(0 if flags == "compact" else -1)
                M.set_tuning(vb, 0, 0, 0 if flags == "compact" else flags)
                zero_calls(D, TINY_PAIRS + [NEG_ALPHA_ZERO_BETA], cols, rows, prec, flags)
            finally:
                M.set_tuning(vb); M.set_compact_tiles(0)


# ------------------------------------------------------------------------- the calls that are tested against the stateless call
# The hot-column plan, the transposed call and coomv are compared with mspmv_csrmv_* elsewhere: an error they share with it passes
# there.  One zero-laden problem each against the model.

OTHER_CALLS = ["hot_column_plan", "transposed", "coomv"]
zuses(["parity:power_law"], ALL_PAIRS)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("call", OTHER_CALLS)
def test_hot_column_plan_transposed_call_and_coomv_equal_the_model_on_zeros(M, prec, call):
    P = problem("parity:power_law", prec, ZEROS)
    c = P.csr
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd = d(P.x)
    if call == "hot_column_plan":
        plan = M.CsrMVHotColumns(d(c.values), d(c.row_offsets), d(c.column_indices), c.cols)
        run = lambda y, alpha, beta: plan(xd, y, alpha=float(alpha), beta=float(beta))
    elif call == "transposed":
        # A = B^T for the problem's matrix B (stable by row: A's rows hold their columns in ascending order), so that A^T x = B x
        rowid = np.repeat(np.arange(c.rows, dtype=np.int32), np.diff(c.row_offsets))
        order = np.argsort(c.column_indices, kind="stable")
        off = np.zeros(c.cols + 1, np.int32); np.cumsum(np.bincount(c.column_indices, minlength=c.cols), out=off[1:])
        av, ao, ac = d(c.values[order]), d(off), d(rowid[order])
        run = lambda y, alpha, beta: M.csrmv(av, ao, ac, xd, y=y, num_cols=c.rows, alpha=float(alpha), beta=float(beta), transpose=True)
    else:
        rowid = np.repeat(np.arange(c.rows, dtype=np.int32), np.diff(c.row_offsets))
        order = np.random.default_rng(7).permutation(c.nnz)          # unsorted triples (repeated columns of a row: duplicates, which add)
        cv, cr, cc = d(c.values[order]), d(rowid[order]), d(c.column_indices[order])
        run = lambda y, alpha, beta: M.coomv(cv, cr, cc, xd, y=y, num_rows=c.rows, num_cols=c.cols, alpha=float(alpha), beta=float(beta))
    for alpha, beta in ALL_PAIRS:
        y = run(d(P.y0.copy()), alpha, beta)
        torch.cuda.synchronize()
        same(y.cpu().numpy(), P.want(alpha, beta), call, prec, (alpha, beta))
