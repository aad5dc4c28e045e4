"""The models of tests/plan_model.py checked on their own (no GPU): the stacked matrix on an example typed out by hand, stack +
fold against the plain integer product for every band count and shape the GPU tests use, the exactness bound of the generated
cases, and the skew probe's model on a band matrix and on uniform columns."""
import numpy as np
import pytest

import plan_model as PM


def test_stack_on_a_hand_written_example():
    #        col: 0  1  2  3  4
    # row 0:      1  .  .  2  3
    # row 1:      .  .  .  .  .
    # row 2:      .  4 5,6 .  7        (column 2 twice)
    a = PM.csr(3, 5, [3, 0, 4], [0, 3, 4, 1, 2, 2, 4], np.array([1., 2., 3., 4., 5., 6., 7.]))
    s = PM.stack(a, 2)                   # band_width 3: columns 0-2 | 3-4
    assert s.rows == 6 and PM.band_width(5, 2) == 3
    assert s.row_offsets.tolist() == [0, 1, 1, 4, 6, 6, 7]
    assert s.column_indices.tolist() == [0, 1, 2, 2, 3, 4, 4]
    assert s.values.tolist() == [1., 4., 5., 6., 2., 3., 7.]
    assert s.order.tolist() == [0, 3, 4, 5, 1, 2, 6]
    s = PM.stack(a, 3)                   # band_width 2: columns 0-1 | 2-3 | 4
    assert s.row_offsets.tolist() == [0, 1, 1, 2, 3, 3, 5, 6, 6, 7]
    assert s.column_indices.tolist() == [0, 1, 3, 2, 2, 4, 4]
    assert s.values.tolist() == [1., 4., 2., 5., 6., 3., 7.]
    s = PM.stack(a, 1)
    assert s.row_offsets.tolist() == a.row_offsets.tolist() and s.column_indices.tolist() == a.column_indices.tolist()
    s = PM.stack(a, 8)                   # more bands than columns: band_width 1, bands 5 .. 7 empty
    assert PM.band_width(5, 8) == 1 and s.rows == 24 and s.row_offsets[15] == 7
    assert s.column_indices.tolist() == [0, 1, 2, 2, 3, 4, 4] and s.values.tolist() == [1., 4., 5., 6., 2., 3., 7.]
    # a row in another order: the entries of a group keep the order they have in A (stable)
    u = PM.csr(3, 5, [3, 0, 4], [0, 3, 4, 2, 1, 4, 2], np.array([1., 2., 3., 5., 4., 7., 6.]))
    s = PM.stack(u, 2)
    assert s.row_offsets.tolist() == [0, 1, 1, 4, 6, 6, 7]
    assert s.column_indices.tolist() == [0, 2, 1, 2, 3, 4, 4] and s.values.tolist() == [1., 5., 4., 6., 2., 3., 7.]


@pytest.mark.parametrize("bands", PM.BANDS)
def test_stack_then_fold_is_the_plain_product(bands):
    shapes = dict(PM.structures(bands))
    if bands == PM.BANDS[0]:
        shapes.update(PM.more_y_structures())
    for name, st in shapes.items():
        case = PM.exact_case(np.random.default_rng(5), st, cap=1 if name == "giant_row" else 4)      # (asserts the exactness bound)
        s = PM.stack(case.a, bands)
        assert s.nnz == st.nnz and np.array_equal(np.sort(s.order), np.arange(st.nnz)), name
        w = PM.band_width(st.cols, bands)
        group = np.repeat(np.arange(s.rows), np.diff(s.row_offsets))
        assert np.array_equal(s.column_indices // w, group // st.rows), name                       # every entry in its band's block of rows
        assert np.array_equal(PM.fold(PM.product_int(s, case.x), st.rows, bands), case.ax), name
        assert np.array_equal(case.want(1.0, 0.0), case.ax.astype(np.float64)), name
        # sorted rows: the groups are sorted too, and a group's entries are a contiguous piece of their row
        assert np.all((np.diff(s.column_indices) >= 0) | (np.diff(group) > 0)), name
        assert np.all((np.diff(s.order) == 1) | (np.diff(group) > 0)), name


def test_exact_case_refuses_a_row_beyond_the_bound():
    st = PM.csr(1, 10, [300000], np.sort(np.random.default_rng(0).integers(0, 10, 300000)))
    with pytest.raises(AssertionError):
        PM.exact_case(np.random.default_rng(1), st, cap=4)          # 300 000 x 4 x ~4.2 x 2 > 2^22
    PM.exact_case(np.random.default_rng(1), st, cap=1)


@pytest.mark.parametrize("vb", [4, 8])
def test_skew_model_on_a_band_and_on_uniform_columns(vb):
    # a band of half-width 50, three entries per row, 12 M nonzeros: a window of 2048 nonzeros spans 683 rows + 100 columns, i.e. at
    # most 783 / 16 + 2 = 51 lines; 512 of them at most 26 112 of the >= 125 000 lines of x: below 150 permille, and no window is wide
    rows = 4_000_000
    col = np.clip(np.repeat(np.arange(rows, dtype=np.int32), 3) + np.tile(np.array([-50, 0, 50], np.int32), rows), 0, rows - 1)
    distinct, wide, samples, permille, _ = PM.skew(col, rows, vb)
    assert samples == 512 * 2048 and wide == 0 and 0 < distinct <= 512 * 51 and 1 <= permille < 150
    rng = np.random.default_rng(7)
    distinct, wide, samples, permille, _ = PM.skew(rng.integers(0, 200_000, 1_200_000).astype(np.int32), 200_000, vb)
    assert wide == 512 and 950 <= permille <= 1050
    assert distinct <= ((200_000 - 1) >> (5 if vb == 4 else 4)) + 1


def test_skew_model_window_starts_and_small_sizes():
    # one distinct window start at nnz == 2048; two at 2049 (windows 0 .. 510 start at 0, the last at 1); nothing to say below
    lone = np.full(2049, 5, np.int64); lone[2048] = 4000
    assert PM.skew(lone[:2048], 4096, 4)[:2] == (1, 0)
    assert PM.skew(lone, 4096, 4)[:2] == (2, 1)
    assert PM.skew(lone[:2047], 4096, 4)[3] == -1 and PM.skew(lone, 0, 8)[3] == -1
    # two lines, the second holding one column: columns 0 .. 32 of 4-byte values, 0 .. 16 of 8-byte values
    assert PM.skew(np.arange(4096) % 33, 33, 4)[0] == 2 and PM.skew(np.arange(4096) % 32, 33, 4)[0] == 1
    assert PM.skew(np.arange(4096) % 17, 17, 8)[0] == 2 and PM.skew(np.arange(4096) % 16, 17, 8)[0] == 1


def test_wide_case_fills_the_budget_and_wide_scalars_are_no_narrower_numbers():
    """the wide magnitude rule: odd numbers (a one in the lowest used bit), the budget of the precision filled and kept for every
    pair of ALPHA_BETA (wide_case asserts the bound), results and the bands' partial sums with bits in the low half; the wide
    scalars are what they say and fit the small integers of exact_case"""
    for prec, limit in (("f32", 1 << 24), ("f64", 1 << 53)):
        for bands in (1, 3, 64):
            st = PM.structures(bands)["rows1027"]
            case = PM.wide_case(np.random.default_rng(8), st, prec)
            v = case.a.values.astype(np.int64)
            assert (v % 2 == 1).all() and (case.x % 2 == 1).all() and (case.y0 % 2 == 1).all()
            s_abs = np.zeros(case.a.rows, np.int64)
            np.add.at(s_abs, case.a.row_of_entry(), np.abs(v * case.x[case.a.column_indices]))
            assert limit // 128 < s_abs.max() <= limit // 16 and limit // 32 < np.abs(case.y0).max() <= limit // 16
            has = np.diff(case.a.row_offsets) > 0
            assert PM.low_half_share(case.ax, prec, has) >= 0.95
            narrow = PM.exact_case(np.random.default_rng(8), st)
            assert PM.low_half_share(narrow.ax, prec, has) == 0.0            # what the small integers leave empty
            assert PM.fits_wide_scalars(narrow, prec) and not PM.fits_wide_scalars(case, prec)
    for alpha, beta in PM.WIDE_SCALARS["f64"]:
        assert all(v == 0 or float(np.float32(v)) != v for v in (alpha, beta))
    for alpha, beta in PM.WIDE_SCALARS["f32"]:
        assert all(float(np.float32(v)) == v and (v == 0 or float(np.float16(v)) != v) for v in (alpha, beta))
        assert all(v == 0 or (np.float32(v).view(np.uint32) & 0xFFFF) != 0 for v in (alpha, beta))           # not a bf16
    assert PM.low_half_share(np.array([1, 257, 1 << 20]), "f32") == 1 / 3 and PM.low_half_share(np.array([1, (1 << 21) + 1]), "f64") == 0.5
