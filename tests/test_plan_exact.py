"""The band-major plan (mspmv_csrmv_plan_*, CsrMVPlan) pinned exactly: the stacked matrix the build leaves in the storage against
tests/plan_model.py's stable sort, the `unsorted` flag at the places where it can be missed, y bit for bit on integer-valued cases
(every association of the sums gives the same number), the kernels an apply and a build launch, what a real-valued y equals, a
side stream, graph capture and the degenerate sizes.  tests/test_prepared_plan.py keeps the tolerance checks on real data.

The integer cases hold numbers of a few bits and alpha, beta that are fp32 numbers; plan_model.wide_case (odd integers that fill the
exactness budget) runs the band-major plan's fold and the hot-column plan, x_is_permuted included, with bits in the low half of
every partial sum, and plan_model.WIDE_SCALARS run alpha, beta that are no fp32 (no bf16) numbers through both plans.  Measured on
one MI355X: the 136 tests of this file take 4.7 s, the 110 before the wide cases 3.8 s."""
import ctypes
import re

import numpy as np
import pytest

import merge_spmv_amd as M
from oracle import oracle as O
import plan_model as PM

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

PREC = {"f32": (np.float32, np.uint32, 4), "f64": (np.float64, np.uint64, 8)}
BANDS = PM.BANDS
SENTINEL = 12345.0
PAD = 4                                   # entries in front of and behind the views of x and y (16 / 32 bytes: the view stays aligned)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tdt(prec):
    return torch.float32 if prec == "f32" else torch.float64


def plan_bytes(rows, cols, nnz, vb, bands):
    size = ctypes.c_size_t(0)
    assert M.load_library().mspmv_csrmv_plan_size(rows, cols, nnz, vb, bands, ctypes.byref(size), None) == 0
    return int(size.value)


def build(a, prec, bands, fill=None, **kw):
    """the plan of PM.Csr `a` (values cast to the precision); fill: the byte the storage holds before the build"""
    npdt, _, vb = PREC[prec]
    storage = None if fill is None else torch.full((max(plan_bytes(a.rows, a.cols, a.nnz, vb, bands), 1),), fill, dtype=torch.uint8, device="cuda")
    arrays = [dev(a.values.astype(npdt)), dev(a.row_offsets.astype(np.int32)), dev(a.column_indices.astype(np.int32))]
    plan = M.CsrMVPlan(*arrays, a.cols, bands=bands, storage=storage, **kw)
    assert plan.bands == bands
    return plan, arrays


def inversions(a):
    """positions j whose column is below its predecessor's inside one row"""
    row = a.row_of_entry()
    return np.flatnonzero((np.diff(a.column_indices) < 0) & (row[1:] == row[:-1])) + 1


def stacked_arrays(plan, prec):
    off, col, val = (t.cpu().numpy() for t in plan.stacked())
    return off.astype(np.int64), col.astype(np.int64), val.view(PREC[prec][1])


def describe_difference(model, off, col, valbits, rows, want_col, want_bits):
    """the first group in which the device and the model differ: its band, its row and both versions of it"""
    if not np.array_equal(off, model.row_offsets):
        g = int(np.flatnonzero(off != model.row_offsets)[0]) - 1
    else:
        p = int(np.flatnonzero((col != want_col) | (valbits != want_bits))[0])
        g = int(np.searchsorted(model.row_offsets, p, side="right")) - 1
    g = max(g, 0)
    lo, hi = int(model.row_offsets[g]), int(model.row_offsets[g + 1])
    return (f"first differing group {g} = band {g // max(rows, 1)}, row {g % max(rows, 1)}: offsets device {off[g:g + 2].tolist()} model {[lo, hi]}; "
            f"columns device {col[lo:hi].tolist()} model {want_col[lo:hi].tolist()}; value bits device {valbits[lo:hi].tolist()} model {want_bits[lo:hi].tolist()}")


def assert_stacked(plan, a, prec, bands, label):
    """sorted rows: the three arrays are the model's; rows in another order: the offsets are, and every group holds the model's
    multiset of (column, value bits)"""
    npdt, udt, _ = PREC[prec]
    model = PM.stack(PM.Csr(a.rows, a.cols, a.row_offsets, a.column_indices, a.values.astype(npdt)), bands)
    off, col, valbits = stacked_arrays(plan, prec)
    want_col, want_bits = model.column_indices, model.values.view(udt)
    assert off.size == bands * a.rows + 1 and col.size == a.nnz and valbits.size == a.nnz, label
    if inversions(a).size:
        assert np.array_equal(off, model.row_offsets), (label, describe_difference(model, off, col, valbits, a.rows, want_col, want_bits))
        group = np.repeat(np.arange(model.rows), np.diff(model.row_offsets))
        o_dev, o_model = np.lexsort((valbits, col, group)), np.lexsort((want_bits, want_col, group))
        col, valbits, want_col, want_bits = col[o_dev], valbits[o_dev], want_col[o_model], want_bits[o_model]
    ok = np.array_equal(off, model.row_offsets) and np.array_equal(col, want_col) and np.array_equal(valbits, want_bits)
    assert ok, (label, describe_difference(model, off, col, valbits, a.rows, want_col, want_bits))
    return off, col, valbits


def real_values(rng, st):
    return PM.Csr(st.rows, st.cols, st.row_offsets, st.column_indices, rng.standard_normal(st.nnz))


def shuffled_rows(rng, a):
    """the same matrix with the entries of every row in a random order"""
    o = np.lexsort((rng.random(a.nnz), a.row_of_entry()))
    return PM.Csr(a.rows, a.cols, a.row_offsets, a.column_indices[o], a.values[o])


def test_stacked_accessors_point_into_the_storage_or_return_null():
    """no GPU: the accessors launch nothing and read nothing -- offsets of the layout from a made-up base address, NULL for no
    plan and for sizes mspmv_csrmv_plan_size refuses"""
    lib = M.load_library()
    fns = (lib.mspmv_csrmv_plan_row_offsets, lib.mspmv_csrmv_plan_columns, lib.mspmv_csrmv_plan_values)
    base = 1 << 20
    for vb in (4, 8):
        for rows, cols, nnz, bands in ((1000, 1000, 5000, 8), (1000, 1000, 5000, 0), (0, 0, 0, 3), (7, 5, 0, 64)):
            off, col, val = (fn(ctypes.c_void_p(base), rows, cols, nnz, vb, bands) for fn in fns)
            used = ctypes.c_int32(0); size = ctypes.c_size_t(0)
            assert lib.mspmv_csrmv_plan_size(rows, cols, nnz, vb, bands, ctypes.byref(size), ctypes.byref(used)) == 0
            assert base < off and off % 256 == 0 and col % 256 == 0 and val % 256 == 0
            assert col - off >= 4 * (used.value * rows + 1) and val - col >= 4 * nnz and base + size.value - val >= vb * nnz
    for fn in fns:
        assert fn(None, 1000, 1000, 5000, 4, 8) is None                                   # no plan
        assert fn(ctypes.c_void_p(base), 1000, 1000, 5000, 2, 8) is None                  # value_bytes
        assert fn(ctypes.c_void_p(base), 1000, 1000, 5000, 4, 65) is None                 # bands
        assert fn(ctypes.c_void_p(base), 1000, 1000, 5000, 4, -1) is None
        assert fn(ctypes.c_void_p(base), -1, 1000, 5000, 4, 8) is None
        assert fn(ctypes.c_void_p(base), 60_000_000, 60_000_000, 100_000_000, 8, 64) is None      # bands * rows + nnz beyond the int32 range


# ---- C1 -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_stacked_matrix_of_sorted_rows_is_the_model(prec, bands):
    """row offsets, column indices and value bits of plan.stacked() equal the stable sort by (band, row), whatever the storage
    held before the build"""
    rng = np.random.default_rng(11)
    for name, st in PM.structures(bands).items():
        a = real_values(rng, st)
        assert inversions(a).size == 0
        first = None
        for fill in (0x00, 0xFF):
            plan, _ = build(a, prec, bands, fill=fill)
            got = assert_stacked(plan, a, prec, bands, (name, prec, bands, fill))
            if first is not None:
                assert all(np.array_equal(p, q) for p, q in zip(first, got)), (name, "two builds differ")
            first = got


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_stacked_matrix_of_unsorted_rows_holds_the_models_groups(prec, bands):
    rng = np.random.default_rng(12)
    shuffled = 0
    for name, st in PM.structures(bands).items():
        a = shuffled_rows(rng, real_values(rng, st))
        shuffled += inversions(a).size > 0               # (a shape whose rows hold one column stays sorted: compared exactly)
        plan, _ = build(a, prec, bands, fill=0xFF)
        assert_stacked(plan, a, prec, bands, (name, prec, bands))
    assert shuffled >= 10


# ---- C3: exact y ------------------------------------------------------------------------------------------------------------------
def framed(values, prec, offset=0, fill=SENTINEL):
    """a view [PAD + offset, PAD + offset + len) of a longer buffer that holds `fill` everywhere else"""
    buf = torch.full((values.size + 2 * PAD + 1,), fill, dtype=tdt(prec), device="cuda")
    view = buf[PAD + offset: PAD + offset + values.size]
    view.copy_(dev(values.astype(PREC[prec][0])))
    return buf, view


def device_x(case, prec, x=None):
    """x as a view of a buffer that is NaN outside [0, cols); every column the matrix does not reference is NaN too"""
    x = (case.x if x is None else x).astype(np.float64)
    unreferenced = np.setdiff1d(np.arange(case.a.cols), case.a.column_indices)
    x[unreferenced] = np.nan
    return framed(x, prec, fill=float("nan"))[1], unreferenced.size


def assert_exact_y(plan, case, prec, alpha, beta, offset, xd, label, want=None, skip_rows=None):
    """y = alpha A x + beta y0 on the bits, y a view of a buffer of sentinels at an aligned (offset 0) or misaligned (offset 1)
    address; beta == 0: y starts as NaN.  x holds zeros (+0.0), so products are +-0.0 and whole rows sum zeros: the sign of every
    zero result is DEFINED (include/mspmv.h at mspmv_csrmv_axpby_*: every sum, every band's partial sum and every carry starts from
    +0.0; beta is never negative here and y0 holds no -0.0, so t = beta * y0 is never -0.0) -- it is +0.0, for every band count, and
    no row is masked."""
    npdt, udt, _ = PREC[prec]
    rows = case.a.rows
    y0 = case.y0.astype(np.float64) if beta != 0.0 else np.full(rows, np.nan)
    buf, y = framed(y0, prec, offset)
    assert (y.data_ptr() % 16 == 0) == (offset == 0)
    plan(xd, y, alpha=alpha, beta=beta)
    got = buf.cpu().numpy()
    front, body, back = got[:PAD + offset], got[PAD + offset: PAD + offset + rows].copy(), got[PAD + offset + rows:]
    sentinel = np.full(1, SENTINEL, npdt).view(udt)[0]
    assert np.all(front.view(udt) == sentinel) and np.all(back.view(udt) == sentinel), (label, "y written outside its rows", front, back)
    want = (case.want(alpha, beta) if want is None else want).astype(npdt)
    if skip_rows is not None:
        body[skip_rows], want = 0.0, np.where(skip_rows, 0.0, want).astype(npdt)
    bad = np.flatnonzero(body.view(udt) != want.view(udt))
    assert np.array_equal(body.view(udt), want.view(udt)), (label, alpha, beta, offset, "first wrong rows", bad[:5].tolist(), body[bad[:5]].tolist(), want[bad[:5]].tolist())
    return got[PAD + offset: PAD + offset + rows]


def exact_y_suite(st, prec, bands, label, cap=4, seed=3):
    """everything C3 asks of one sparsity structure"""
    case = PM.exact_case(np.random.default_rng(seed), st, cap=cap)                  # (asserts the exactness bound on the CPU)
    plan, originals = build(case.a, prec, bands, fill=0xFF)
    xd, holes = device_x(case, prec)
    for alpha, beta in PM.ALPHA_BETA:
        for offset in (0, 1):
            assert_exact_y(plan, case, prec, alpha, beta, offset, xd, label)
    if case.a.nnz:
        # an Inf in x reaches exactly the rows that reference its column
        c = int(case.a.column_indices[case.a.nnz // 2])
        x_inf = case.x.astype(np.float64); x_inf[c] = np.inf
        hit = np.zeros(case.a.rows, bool); hit[case.a.row_of_entry()[case.a.column_indices == c]] = True
        y = assert_exact_y(plan, case, prec, 1.0, 0.0, 0, device_x(case, prec, x_inf)[0], (label, "inf"), skip_rows=hit)
        assert not np.any(np.isfinite(y[hit])) and np.all(np.isfinite(y[~hit])), (label, "inf")
    # the plan does not need the original arrays after the build
    originals[0].fill_(float("nan")); originals[1].zero_(); originals[2].zero_()
    del originals
    assert_exact_y(plan, case, prec, -0.5, 3.0, 1, xd, (label, "originals gone"))
    assert_exact_y(plan, case, prec, 1.0, 0.0, 0, xd, (label, "originals gone"))
    return holes


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_y_is_exact_on_integer_cases(prec, bands):
    holes = 0
    for name, st in PM.structures(bands).items():
        holes += exact_y_suite(st, prec, bands, (name, prec, bands)) > 0
    assert holes >= 6                                    # (shapes that leave a column out on purpose: NaN there never reaches y)


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_y_is_exact_on_long_rows_and_both_fold_forms(prec, bands):
    """one row of 300 000 (values +-1: under the bound), one row in 97, and rows = 1026 / 1027 / 1028: the scalar and the vector
    form of the fold over more than one block (rows % 4, and y at a misaligned address with rows % 4 == 0)"""
    for name, st in PM.more_y_structures().items():
        exact_y_suite(st, prec, bands, (name, prec, bands), cap=1 if name == "giant_row" else 4)


# ---- C3w: exact y on numbers that fill the significand -----------------------------------------------------------------------------
WIDE_SHAPES = ("rows1027", "band_edges", "repeats", "row5000", "rows342_last2", "last_band")


def assert_wide(case, prec, bands, label):
    """conditions on the wide data: at least 95 % of the rows with entries have a result with a non-zero low half for every pair, and
    so have at least 90 % of the non-empty (band, row) groups' sums -- what the fold adds"""
    has = np.diff(case.a.row_offsets) > 0
    for alpha, beta in PM.ALPHA_BETA:
        units = (2 * case.want(alpha, beta)).astype(np.int64)                               # (halves: alpha = -0.5)
        assert PM.low_half_share(units, prec, has) >= 0.95, (label, alpha, beta)
    model = PM.stack(case.a, bands)
    parts = PM.product_int(model, case.x)
    assert np.array_equal(PM.fold(parts, case.a.rows, bands), case.ax)
    if prec == "f64":
        assert PM.low_half_share(parts, prec, np.diff(model.row_offsets) > 0) >= 0.90, label


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_fold_is_exact_on_numbers_that_fill_the_significand(prec, bands, capfd):
    """plan_model.wide_case: odd integers that fill the exactness budget, so the stacked matrix's partial sums y' -- written by the
    CsrMV kernels with their carries and records, read again and added by the fold -- hold bits in both halves of a double (in the
    low 16 bits of a float).  y on the bits for every pair at an aligned and a misaligned y; the fold is asserted to have run."""
    sts = {n: st for n, st in PM.structures(bands).items() if n in WIDE_SHAPES}
    sts.update({n: st for n, st in PM.more_y_structures().items() if n in ("giant_row", "rows1027")})
    assert len(sts) == len(WIDE_SHAPES) + 1                                              # (rows1027 of both: the later one, 600 columns)
    for name, st in sts.items():
        case = PM.wide_case(np.random.default_rng(8), st, prec)
        assert_wide(case, prec, bands, (name, prec, bands))
        plan, _ = build(case.a, prec, bands, fill=0xFF)
        xd, _ = device_x(case, prec)
        capfd.readouterr()
        plan(xd, debug_synchronous=True)
        names = launch_names(capfd.readouterr().out)
        assert ("plan_combine_kernel" in names) == (bands > 1), (name, names)
        for alpha, beta in PM.ALPHA_BETA:
            for offset in (0, 1):
                assert_exact_y(plan, case, prec, alpha, beta, offset, xd, (name, prec, bands, "wide"))


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plans_are_exact_with_scalars_that_fill_the_significand(prec, bands):
    """alpha and beta that are no fp32 (no bf16, no fp16) numbers -- plan_model.WIDE_SCALARS -- on the small integers of exact_case,
    where their granule of 2^-30 (2^-12) leaves room: the band-major plan (the scalars travel through the plan's inner call into
    the kernels and, with more than one band, into the fold) and, once, the hot-column plan."""
    fitted = 0
    for name in ("rows1027", "band_edges", "repeats", "empty_ends", "row5000"):
        st = PM.structures(bands)[name]
        case = PM.exact_case(np.random.default_rng(13), st, cap=1 if name == "row5000" else 4)
        if not PM.fits_wide_scalars(case, prec):
            continue
        fitted += 1
        plan, _ = build(case.a, prec, bands, fill=0xFF)
        xd, _ = device_x(case, prec)
        for alpha, beta in PM.WIDE_SCALARS[prec]:
            for offset in (0, 1):
                assert_exact_y(plan, case, prec, alpha, beta, offset, xd, (name, prec, bands, "wide scalars"))
        if bands == BANDS[0]:
            npdt, udt, _ = PREC[prec]
            hot = M.CsrMVHotColumns(dev(case.a.values.astype(npdt)), dev(case.a.row_offsets.astype(np.int32)), dev(case.a.column_indices.astype(np.int32)), case.a.cols)
            for alpha, beta in PM.WIDE_SCALARS[prec]:
                y = hot(dev(case.x.astype(npdt)), dev(case.y0.astype(npdt)), alpha=alpha, beta=beta).cpu().numpy()
                want = case.want(alpha, beta).astype(npdt)
                assert np.array_equal(y.view(udt), want.view(udt)), (name, prec, alpha, beta, "hot-column plan")
    assert fitted >= 4


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_hot_column_plan_is_exact_on_numbers_that_fill_the_significand(prec):
    """the hot-column plan (renumbered columns, x gathered through the plan's order or permuted once by the caller) on
    plan_model.wide_case: y on the bits against the int64 model, with x as it is and with x_is_permuted"""
    npdt, udt, _ = PREC[prec]
    sts = {"rows1027": PM.structures(3)["rows1027"], "repeats": PM.structures(3)["repeats"], "giant_row": PM.more_y_structures()["giant_row"]}
    for name, st in sts.items():
        case = PM.wide_case(np.random.default_rng(9), st, prec)
        assert_wide(case, prec, 1, (name, prec))
        val, off, col = dev(case.a.values.astype(npdt)), dev(case.a.row_offsets.astype(np.int32)), dev(case.a.column_indices.astype(np.int32))
        plan = M.CsrMVHotColumns(val, off, col, case.a.cols)
        order = plan.order().cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(case.a.cols)) and not np.array_equal(order, np.arange(case.a.cols)), name
        x = dev(case.x.astype(npdt))
        xp = plan.permute(x)
        assert np.array_equal(xp.cpu().numpy(), case.x.astype(npdt)[order])
        for alpha, beta in PM.ALPHA_BETA:
            want = case.want(alpha, beta).astype(npdt)
            for permuted in (False, True):
                y = dev(case.y0.astype(npdt)) if beta != 0.0 else torch.full((case.a.rows,), float("nan"), dtype=tdt(prec), device="cuda")
                plan(xp if permuted else x, y, alpha=alpha, beta=beta, x_is_permuted=permuted)
                got = y.cpu().numpy()
                bad = np.flatnonzero(got.view(udt) != want.view(udt))
                assert bad.size == 0, (name, prec, alpha, beta, permuted, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


# ---- C2: the unsorted flag ---------------------------------------------------------------------------------------------------------
def flag_matrix(bands):
    """Sorted rows of distinct columns in which every row's last column is above the next row's first; row 2 has 3000 entries at
    positions 10 .. 3009 of the nonzero stream, across the chunk boundaries at 1024 and 2048.  The entries at positions 0 / 1,
    1023 / 1024 and nnz - 2 / nnz - 1 are the two columns k * w - 1, k * w on either side of a band edge (any two neighbours with
    one band): swapped, they are an inversion that crosses bands -- the only kind the sorted path of the scatter cannot take,
    its position `j - lo` then counts one entry that belongs to another group."""
    rng = np.random.default_rng(21)
    rows, cols = 40, 4000
    w = PM.band_width(cols, bands)
    first, last = (w, (bands - 1) * w) if bands > 1 else (1500, 1500)
    mid = -(-1014 // w) * w if bands > 1 else 1500                # an edge with >= 1013 columns below and >= 1985 above it
    assert 1014 <= mid <= 2014 and 1 <= first and last < cols - 1

    def row(n, below=None, edge=None, above=None, end=cols - 1):
        """`below` columns under edge - 1, then edge - 1, edge, then `above` columns over it, then `end`"""
        if edge is None:
            return np.r_[np.sort(rng.choice(cols - 1, n - 1, replace=False)), end]
        lo = np.sort(rng.choice(edge - 1, below, replace=False))
        hi = np.sort(rng.choice(np.arange(edge + 1, cols - 1), above, replace=False))
        return np.r_[lo, edge - 1, edge, hi, [] if end is None else end].astype(np.int64)

    lens = np.r_[5, 5, 3000, rng.integers(2, 10, rows - 4), 6]
    parts = [row(5, 0, first, 2), row(5), row(3000, 1013, mid, 3000 - 1016)] + [row(n) for n in lens[3:-1]] + [row(6, 4, last, 0, end=None)]
    return PM.csr(rows, cols, lens, np.concatenate(parts))


def swapped(st, p):
    col = st.column_indices.copy()
    col[[p, p + 1]] = col[[p + 1, p]]
    return PM.Csr(st.rows, st.cols, st.row_offsets, col, st.values)


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_inversion_anywhere_takes_the_cursor_path_and_row_boundaries_do_not_count(prec, bands):
    """(a) the only inversion sits across the 1024-nonzero chunk boundary of the build's blocks, (b) between the last two entries
    of the last row, (c) between the first two entries of the matrix: the groups must still hold the model's entries (every
    swapped pair lies on the two sides of a band edge: the sorted path would count the entry of the lower band into the upper
    one's run, write it one slot past its group and leave a slot of the storage's 0xFF fill behind) and y stays exact.  (d) no inversion inside a row, but every row's last column
    above the next row's first: the sorted path, byte for byte the model."""
    base = flag_matrix(bands)
    row = base.row_of_entry()
    w = PM.band_width(base.cols, bands)
    for p in (0, 1023, base.nnz - 2):                    # each swap crosses a band edge (and stays inside one row)
        lo, hi = base.column_indices[p], base.column_indices[p + 1]
        assert row[p] == row[p + 1] and hi == lo + 1 and (bands == 1 or hi // w == lo // w + 1), (p, lo, hi)
    assert inversions(base).size == 0 and np.all(base.column_indices[base.row_offsets[1:-1] - 1] > base.column_indices[base.row_offsets[1:-1]])
    assert row[1023] == row[1024] == 2 and row[2047] == row[2048] == 2
    rng = np.random.default_rng(22)
    variants = {"a": swapped(base, 1023), "b": swapped(base, base.nnz - 2), "c": swapped(base, 0), "d": base}
    for name, st in variants.items():
        want = {"a": [1024], "b": [base.nnz - 1], "c": [1], "d": []}[name]
        assert inversions(st).tolist() == want
        a = real_values(rng, st)
        plan, _ = build(a, prec, bands, fill=0xFF)
        assert_stacked(plan, a, prec, bands, ("flag", name, prec, bands))
        exact_y_suite(st, prec, bands, ("flag", name, prec, bands))


# ---- C4: which kernels run ---------------------------------------------------------------------------------------------------------
def launch_names(text):
    return re.findall(r"^mspmv: (.*?)<<<", text, flags=re.M)


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_launch_log_of_build_and_apply(prec, bands, capfd):
    """Build: the count pass, the three scan kernels, the scatter pass and ONE coordinate kernel.  Apply: one band writes y by the
    one-launch kernel alone (this size: behind its compact front end) -- no fold, no coordinate kernel; more bands run, on the
    contiguous tile map, the one-launch kernel in fp64 and the classic tile kernel + fix-up in fp32, then the fold."""
    st = PM.structures(bands)["rows1027"]
    case = PM.exact_case(np.random.default_rng(4), st)
    capfd.readouterr()
    plan, _ = build(case.a, prec, bands, debug_synchronous=True)
    assert launch_names(capfd.readouterr().out) == ["plan_count_kernel", "scan_reduce_kernel", "scan_blocksums_kernel", "scan_apply_kernel",
                                                    "plan_scatter_kernel", "coords_scatter_kernel"]
    xd, _ = device_x(case, prec)
    y = plan(xd, debug_synchronous=True)
    names = launch_names(capfd.readouterr().out)
    if bands == 1:
        assert names == ["tile_kernel_snap (compact front end)"], names
    elif prec == "f64":
        assert names == ["tile_kernel_snap", "plan_combine_kernel"], names
    else:
        assert names == ["tile_kernel_vec", "fixup_onepass_kernel", "plan_combine_kernel"], names
    assert np.array_equal(y.cpu().numpy(), case.want(1.0, 0.0).astype(PREC[prec][0]))


# ---- C5: what a real-valued y equals ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("rows,cols,top", [(1027, 1000, 13), (20000, 50000, 12)])
def test_one_band_is_bit_for_bit_the_stateless_call(prec, rows, cols, top):
    npdt, udt, vb = PREC[prec]
    rng = np.random.default_rng(31)
    st = PM.sorted_rows(rng, rows, cols, rng.integers(0, top, rows))
    a = PM.Csr(st.rows, st.cols, st.row_offsets, st.column_indices, rng.uniform(-1, 1, st.nnz))
    assert M.band_passes(rows, cols, a.nnz, vb) <= 1
    plan, (val, off, col) = build(a, prec, 1)
    x = dev(rng.uniform(-1, 1, cols).astype(npdt)); y0 = dev(rng.uniform(-1, 1, rows).astype(npdt))
    for alpha, beta in ((1.0, 0.0), (-0.5, 3.0)):
        want = M.csrmv(val, off, col, x, y=y0.clone(), alpha=alpha, beta=beta, num_cols=cols)
        got = plan(x, y0.clone(), alpha=alpha, beta=beta)
        assert np.array_equal(got.cpu().numpy().view(udt), want.cpu().numpy().view(udt)), (prec, alpha, beta)


@gpu
@pytest.mark.parametrize("bands", [b for b in BANDS if b > 1])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_several_bands_on_short_groups(prec, bands):
    """Every (band, row) group has at most 8 entries, so every tile of the stacked matrix is a closed tile of short rows.
    fp64 (the one-launch kernel): such tiles sum every row left to right from +0.0, so y' is the sequential sum of the stacked
    model (O.spmv_gold) and y its fold in band order, bit for bit (alpha = 1 and -2, beta = 0: exact scalings -- with beta != 0
    the fold's multiply-add may be contracted, which the strict bound of tests/test_prepared_plan.py covers).
    fp32 (the classic launches): tile_kernel_vec sums the products of a tile in runs of eight consecutive STREAM positions per
    thread and joins the runs by a segmented scan, tiles by the fix-up: the order in which a row's products are added depends
    on where the row falls in its tile's runs -- on all the rows before it, not on the row -- so no per-row order is defined to
    pin; y is held to the strict bound of the oracle and must repeat bit for bit."""
    npdt, udt, vb = PREC[prec]
    rng = np.random.default_rng(32)
    st = PM.sorted_rows(rng, 1027, 1000, rng.integers(0, 9, 1027))
    a = PM.Csr(st.rows, st.cols, st.row_offsets, st.column_indices, rng.uniform(-1, 1, st.nnz).astype(npdt))
    x = rng.uniform(-1, 1, st.cols).astype(npdt)
    model = PM.stack(a, bands)
    assert np.diff(model.row_offsets).max() <= 8
    plan, _ = build(a, prec, bands)
    y = plan(dev(x)).cpu().numpy()
    assert np.array_equal(plan(dev(x)).cpu().numpy().view(udt), y.view(udt))
    if prec == "f64":
        stacked = O.Csr(model.rows, model.cols, model.row_offsets.astype(np.int32), model.column_indices.astype(np.int32), model.values)
        folded = PM.fold(O.spmv_gold(stacked, x), a.rows, bands)
        assert folded.dtype == npdt
        for alpha in (1.0, -2.0):
            got = plan(dev(x), alpha=alpha).cpu().numpy()
            want = (npdt(alpha) * folded + npdt(0)).astype(npdt)
            assert np.array_equal(got.view(udt), want.view(udt)), (bands, alpha, np.flatnonzero(got != want)[:5])
    else:
        csr = O.Csr(a.rows, a.cols, a.row_offsets.astype(np.int32), a.column_indices.astype(np.int32), a.values)
        g, s = O.spmv_gold_acc64(csr, x)
        ok, worst = O.strict_check(csr, y, g, s, items_per_thread=M.serial_sum_depth(a.rows * bands, a.cols, a.nnz, vb, extra=bands))
        assert ok, (bands, worst)


# ---- C6: streams and graphs -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_side_stream_and_graph_replay_are_exact(prec, bands):
    npdt, udt, _ = PREC[prec]
    case = PM.exact_case(np.random.default_rng(6), PM.structures(bands)["rows1027"])
    plan, _ = build(case.a, prec, bands)
    xd, _ = device_x(case, prec)
    want = case.want(-2.0, 0.0).astype(npdt)
    y = torch.full((case.a.rows,), float("nan"), dtype=tdt(prec), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan(xd, y, alpha=-2.0, stream=side)
    side.synchronize()
    assert np.array_equal((y.cpu().numpy() + npdt(0)).view(udt), want.view(udt))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan(xd, y, alpha=-2.0)
    for sign in (1.0, -1.0):                             # x changed in place between the replays: -x keeps the bound
        y.fill_(float("nan"))
        g.replay(); torch.cuda.synchronize()
        assert np.array_equal((y.cpu().numpy() + npdt(0)).view(udt), (sign * want + npdt(0)).view(udt)), sign
        xd.neg_()


# ---- C7: degenerate sizes ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_no_rows_and_no_nonzeros(prec, bands):
    npdt, udt, _ = PREC[prec]
    # rows == 0: build and apply succeed and touch nothing
    empty = PM.csr(0, 0, [], [])
    plan, _ = build(empty, prec, bands, fill=0xFF)
    assert plan.rows == 0 and plan.nnz == 0
    y = torch.full((8,), SENTINEL, dtype=tdt(prec), device="cuda")
    plan(torch.empty(0, dtype=tdt(prec), device="cuda"), y, alpha=-2.0, beta=3.0)
    torch.cuda.synchronize()
    assert np.all(y.cpu().numpy().view(udt) == np.full(1, SENTINEL, npdt).view(udt)[0])
    # nnz == 0 with rows: y = beta * y0 exactly, +0.0 with beta == 0 (sign bit included), nothing outside the rows
    for rows in (1027, 1028):
        st = PM.csr(rows, 50, np.zeros(rows, np.int64), [])
        case = PM.exact_case(np.random.default_rng(7), st)
        plan, _ = build(case.a, prec, bands, fill=0xFF)
        off = stacked_arrays(plan, prec)[0]
        assert off.size == bands * rows + 1 and not off.any()
        xd, _ = device_x(case, prec)                     # all NaN: no column is referenced
        for alpha, beta in PM.ALPHA_BETA:
            for offset in (0, 1):
                assert_exact_y(plan, case, prec, alpha, beta, offset, xd, ("no nonzeros", rows, prec, bands))
