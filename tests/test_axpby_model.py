"""tests/axpby_model.py checked on the CPU: the int64 model of y = alpha*A*x + beta*y against answers typed in by hand, its
exactness assertion, and that assertion over every (matrix, pair) tests/test_axpby_exact.py runs on the GPU -- so a later edit of
a shape there cannot silently turn an exact test into a rounding-dependent one."""
import numpy as np
import pytest

import axpby_model as A


def hand_case(dtype):
    # row 0: 2*3 - 1*2 = 4;  row 1: no entries;  row 2: 1*3 + 1*(-3) cancels;  row 3: -2*(-3) = 6
    off = np.array([0, 2, 2, 4, 5], np.int32)
    col = np.array([0, 1, 0, 2, 2], np.int32)
    val = np.array([2, -1, 1, 1, -2], dtype)
    x = np.array([3, 2, -3], dtype)
    y0 = np.array([1, -2, 4, -8], dtype)
    return A.Csr(4, 3, off, col, val), x, y0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_against_hand_written_answers(dtype):
    csr, x, y0 = hand_case(dtype)
    expect = {(1, 0): [4, 0, 0, 6],
              (2, 0): [8, 0, 0, 12],
              (-0.5, 3): [1, -6, 12, -27],
              (-1.5, 0.5): [-5.5, -1, 2, -13],
              (1, 1): [5, -2, 4, -2],
              (2.5, -1): [9, 2, -4, 23],
              (0, -2): [-2, 4, -8, 16],                         # alpha == 0: beta * y0 alone
              (3, -5): [7, 10, -20, 58]}
    assert sorted(expect) == sorted(A.PAIRS)
    for (alpha, beta), want in expect.items():
        y = A.model(csr, x, y0, alpha, beta)
        assert y.dtype == dtype
        assert np.array_equal(A.bits(y), A.bits(np.array(want, dtype))), (alpha, beta, y)
    # an empty row and a cancelling row are +0.0, whatever the sign of alpha
    for alpha in (1, -0.5, -3):
        y = A.model(csr, x, y0, alpha, 0)
        assert not np.signbit(y[1]) and not np.signbit(y[2]) and y[1] == 0 and y[2] == 0
    # a cancellation between alpha * s and beta * y0 as well: 2 * 4 + (-8) * 1
    assert A.bits(A.model(csr, x, y0, 2, -8))[0] == 0
    # beta == 0: y0 is not used -- NaN, infinities and -0.0 there change nothing
    poison = np.array([np.nan, np.inf, -np.inf, -0.0], dtype)
    for alpha in (1, 2, -0.5):
        assert np.array_equal(A.bits(A.model(csr, x, poison, alpha, 0)), A.bits(A.model(csr, x, y0, alpha, 0)))
    # alpha == 0 and beta == 0: all +0.0
    assert not A.bits(A.model(csr, x, poison, 0, 0)).any()
    # beta != 0 needs an integer y0
    with pytest.raises((AssertionError, ValueError, FloatingPointError)):
        with np.errstate(invalid="raise"):
            A.model(csr, x, poison, 1, 1)


def test_granule():
    assert [A.granule(a, b) for a, b in A.PAIRS] == [1, 1, 0.5, 0.5, 1, 0.5, 1, 1]
    assert A.granule(0.375, 2) == 0.125 and A.granule(0, 0) == 1
    assert A.granule(1 / 3, 0) == 2.0 ** -54                    # (0.333... is dyadic as a float: a granule far below anything exact here)
    with pytest.raises(AssertionError, match="not exact"):
        A.model(*hand_case(np.float64), 1 / 3, 0)


@pytest.mark.parametrize("dtype,limit", [(np.float32, 1 << 24), (np.float64, 1 << 53)])
def test_the_bound_fires(dtype, limit):
    """one row of n entries, all +-1: the quotient is |alpha| / g * n + |beta * y0| / g"""
    n = 1 << 22
    csr = A.Csr(2, 1, np.array([0, n, n], np.int32), np.zeros(n, np.int32), np.ones(n, dtype))
    x, y0 = np.ones(1, dtype), np.array([4, 4], dtype)
    assert A.quotient(csr, x, y0, 3, -5) == 3 * n + 20
    A.model(csr, x, y0, 3, -5)                                   # 3 * 2^22 + 20 < 2^24
    assert A.quotient(csr, x, y0, 2.5, -1) == 5 * n + 8          # granule 1/2: 5 * 2^22 + 8 halves >= 2^24
    if dtype == np.float32:
        with pytest.raises(AssertionError, match="not exact"):
            A.model(csr, x, y0, 2.5, -1)
        with pytest.raises(AssertionError, match="not exact"):
            A.model(csr, x, np.array([4, 4], dtype), 4, 1)       # exactly 2^24 + 4
        # y0 alone can break it: |beta * y0| / g
        big = np.array([1 << 23, 1], dtype)
        with pytest.raises(AssertionError, match="not exact"):
            A.model(csr, x, big, 1, 2)
        A.model(csr, x, big, 1, 0)                               # beta == 0: y0 does not count
    else:
        A.model(csr, x, y0, 2.5, -1)
        with pytest.raises(AssertionError, match="not exact"):
            A.model(csr, x, np.array([2.0 ** 52, 1]), 1, -2)


def test_generator_draws_no_zero_and_sorts_columns():
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 9, 500)
    csr, x, y0 = A.integer_problem(rng, 500, 40, lens, np.float32)
    assert np.array_equal(np.diff(csr.row_offsets), lens) and csr.nnz == lens.sum()
    assert set(np.unique(np.abs(csr.values))) == {1, 2} and set(np.unique(np.abs(x))) == {1, 2, 3} and set(np.unique(np.abs(y0))) == set(range(1, 9))
    assert (csr.values < 0).any() and (x < 0).any() and (y0 < 0).any()
    for r in range(500):
        c = csr.column_indices[csr.row_offsets[r]:csr.row_offsets[r + 1]]
        assert np.all(np.diff(c) >= 0) and np.all((c >= 0) & (c < 40))
    csr1, x1, _ = A.integer_problem(rng, 3, 1, [5, 0, 2], np.float64, vmax=1, xmax=1)
    assert set(np.abs(csr1.values)) == {1} and abs(x1[0]) == 1 and not csr1.column_indices.any()


def _gpu_file():
    pytest.importorskip("torch")
    import test_axpby_exact as E
    return E


def test_every_gpu_problem_and_pair_is_within_the_bound():
    E = _gpu_file()
    assert set(label for label, _ in E.USED) == set(E.PROBLEMS), "a problem no test uses, or a test on an unlisted problem"
    for (label, prec), pairs in sorted(E.USED.items()):
        P = E.problem(label, prec)
        limit = A.LIMIT[np.dtype(P.dtype)]
        assert not (P.csr.values == 0).any() and not (P.x == 0).any() and not (P.y0 == 0).any()
        for alpha, beta in sorted(pairs):
            assert A.quotient(P.csr, P.x, P.y0, alpha, beta) < limit, (label, prec, alpha, beta)
            P.want(alpha, beta)                                  # (the model's own assertion)
    # the longest row of the shapes of test_gpu_parity run with the default value ranges: 200 000 entries, 6 per product, 5 granules
    # per unit of alpha, 64 for y0 -- the arithmetic of the bound
    assert 5 * 6 * 200_000 + 64 < 1 << 24


def test_the_planted_problem_has_the_rows_the_gpu_test_plants_at():
    E = _gpu_file()
    for tile_items in E.PLANTED_TILES:
        P = E.problem(f"planted:{tile_items}", "f32")
        rows = E.planted_rows(P.csr, tile_items)
        off = P.csr.row_offsets.astype(np.int64)
        r = rows["ends_on_tile_boundary"]
        assert (r + 1 + off[r + 1]) % tile_items == 0 and off[r + 1] > off[r]
        assert len(set(rows.values())) == len(rows)
        assert not np.diff(off)[2000:5800].any() and 5800 - 2000 > tile_items
