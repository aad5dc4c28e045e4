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
    zero_only = {label for label in E.PROBLEMS if label.startswith("planted_zero:")}           # (shapes made for the zero-laden tests alone)
    assert set(label for label, _ in E.USED) == set(E.PROBLEMS) - zero_only, "a problem no test uses, or a test on an unlisted problem"
    assert zero_only <= set(label for label, _, _ in E.ZUSED) <= set(E.PROBLEMS)
    qualifies = {}
    for (label, prec), pairs in sorted(E.USED.items()):
        P = E.problem(label, prec)
        limit = A.LIMIT[np.dtype(P.dtype)]
        # (the draws without a zero; the zero-laden ones: test_every_zero_laden_gpu_problem_has_its_rows_and_is_in_the_domain)
        assert not (P.csr.values == 0).any() and not (P.x == 0).any() and not (P.y0 == 0).any()
        wide = A.WIDE_PAIRS[np.dtype(P.dtype)]
        assert not pairs & {p for dt, ps in A.WIDE_PAIRS.items() if dt != np.dtype(P.dtype) for p in ps}, "wide scalars of the other type"
        for alpha, beta in sorted(pairs):
            if (alpha, beta) in wide and not P.fits(alpha, beta):
                continue                                         # (the GPU tests ask Problem.wide_scalars(), the same computation)
            assert A.quotient(P.csr, P.x, P.y0, alpha, beta) < limit, (label, prec, alpha, beta)
            P.want(alpha, beta)                                  # (the model's own assertion)
        if pairs & set(wide):
            assert set(P.wide_scalars()) <= set(wide) and (set(wide) <= pairs)
            qualifies.setdefault(prec, set()).update([label] if len(P.wide_scalars()) == len(wide) else [])
            # the arithmetic of the bound: both pairs fit exactly where sum |v*x| + |y0| stays below 2^23 (below 4095 and a bit)
            _, sa = A.row_sums(P.csr, P.x)
            g = 1 << (30 if prec == "f64" else 12)
            fit = bool(((g + 2) * sa + (g + 1) * np.abs(P.y0.astype(np.int64)) < limit).all())
            assert fit == (len(P.wide_scalars()) == len(wide)), (label, prec)
    # which problems the wide scalars run on: in fp64 every one (the longest row, 1 445 000 entries of +-1, is below 2^22); in fp32
    # those whose rows hold sum |v*x| < 4095 -- some of the path table and one of the prepared shapes
    assert qualifies["f64"] == {label for (label, prec), pairs in E.USED.items() if prec == "f64" and pairs & set(A.WIDE_PAIRS[np.dtype(np.float64)])}
    assert len(qualifies["f32"] & {"parity:" + n for n in E.T.SHAPES}) >= 6, qualifies["f32"]
    assert qualifies["f32"] & {"parity:" + n for n in E.PREPARED_SHAPES}, qualifies["f32"]
    # the longest row of the shapes of test_gpu_parity run with the default value ranges: 200 000 entries, 6 per product, 5 granules
    # per unit of alpha, 64 for y0 -- the arithmetic of the bound
    assert 5 * 6 * 200_000 + 64 < 1 << 24


def test_wide_scalars_are_what_they_say():
    """no number of WIDE_PAIRS survives the narrower format, and granule() takes them"""
    import torch
    for alpha, beta in A.WIDE_PAIRS[np.dtype(np.float64)]:
        for v in (alpha, beta):
            assert v == 0 or float(np.float32(v)) != v
        assert A.granule(alpha, beta) == 2.0 ** -30
    for alpha, beta in A.WIDE_PAIRS[np.dtype(np.float32)]:
        for v in (alpha, beta):
            assert float(np.float32(v)) == v
            assert v == 0 or (float(np.float16(v)) != v and float(torch.tensor(v, dtype=torch.float32).bfloat16().float()) != v)
        assert A.granule(alpha, beta) == 2.0 ** -12
    for pairs in A.WIDE_PAIRS.values():
        assert [b == 0 for _, b in pairs] == [True, False] and pairs[1][0] < 0


def test_wide_problem_draws_what_it_says():
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 9, 600); lens[5] = 3000; lens[6] = 1
    for dtype, xcap in ((np.float32, 1 << 8), (np.float64, 1 << 20)):
        budget = A.wide_budget(dtype)
        assert budget == A.LIMIT[np.dtype(dtype)] // 16
        csr, x, y0 = A.wide_problem(rng, 600, 40, lens, dtype)
        assert csr.values.dtype == dtype and x.dtype == dtype and y0.dtype == dtype
        assert np.array_equal(np.diff(csr.row_offsets), lens)
        v, xi, yi = (a.astype(np.int64) for a in (csr.values, x, y0))
        assert (v % 2 == 1).all() and (xi % 2 == 1).all() and (yi % 2 == 1).all()            # odd: never zero, the lowest bit a one
        assert (v < 0).any() and (v > 0).any() and (xi < 0).any() and (yi < 0).any()
        import math
        xmax = min(xcap, math.isqrt(budget // 3000))
        assert np.abs(xi).max() <= xmax and np.abs(xi).max() > xmax // 2
        assert np.abs(yi).max() <= budget and np.abs(yi).max() > budget // 2
        off = csr.row_offsets
        for r in range(600):
            n = int(lens[r])
            if n:
                hi = max(1, budget // (n * xmax))
                assert np.abs(v[off[r]:off[r + 1]]).max() <= hi
            c = csr.column_indices[off[r]:off[r + 1]]
            assert np.all(np.diff(c) >= 0) and np.all((c >= 0) & (c < 40))
        assert np.abs(v[off[6]:off[7]]).max() > 1 << 8                                        # (a one-entry row: up to budget // xmax)
        _, sa = A.row_sums(csr, x)
        assert sa.max() <= budget and sa.max() > budget // 8                                  # the budget is filled, not only respected
        for alpha, beta in A.PAIRS + [(-0.5, 0)]:
            y = A.model(csr, x, y0, alpha, beta)
            assert A.quotient(csr, x, y0, alpha, beta) <= A.LIMIT[np.dtype(dtype)] // 2
            assert A.low_half_share(csr, y) >= 0.95
        # the narrow draw is what the wide one is not
        n = A.integer_problem(rng, 600, 40, lens, dtype)
        assert A.low_half_share(n[0], A.model(*n, 1, 0)) == 0
        assert all(share == 0 for _, _, share in A.carry_low_half_shares(n[0], n[1]))
        shares = A.carry_low_half_shares(csr, x)
        assert [(r, k) for r, k, _ in shares] == [(5, 2)]                                      # 3000 entries: one cut at 1792, one at 2816
    assert A.low_half(np.array([1.0, 1 + 2.0 ** -30, 3 * 2.0 ** 40])).tolist() == [0, 1 << 22, 0]
    assert A.low_half(np.array([1, 1 + 2.0 ** -12, 257], np.float32)).tolist() == [0, 1 << 11, 1 << 15]


def test_row_sums_do_not_lean_on_wraparound():
    """400 000 rows of the wide fp64 draw hold sum |v*x| of 2^47 and more each: a running sum over the whole matrix passes 2^63 (the
    total is shown to, in exact Python integers).  row_sums adds every row on its own: its sums equal exact per-row sums, the
    absolute sums are positive and within the budget, and rows without entries are zero."""
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 9, 400_000)
    csr, x, y0 = A.wide_problem(rng, lens.size, 1000, lens, np.float64)
    s, sa = A.row_sums(csr, x)
    assert sum(int(v) for v in sa) > 1 << 63                     # the whole-matrix running sum would have wrapped
    assert s.dtype == np.int64 and (sa[lens > 0] > 0).all() and not sa[lens == 0].any() and not s[lens == 0].any()
    assert sa.max() <= A.wide_budget(np.float64) and (np.abs(s) <= sa).all()
    off = csr.row_offsets.astype(np.int64)
    prod = csr.values.astype(np.int64) * x.astype(np.int64)[csr.column_indices]
    for r in list(range(50)) + list(range(lens.size - 50, lens.size)) + rng.integers(0, lens.size, 300).tolist():
        pr = [int(v) for v in prod[off[r]:off[r + 1]]]
        assert int(s[r]) == sum(pr) and int(sa[r]) == sum(abs(v) for v in pr), r
    assert A.segment_sums(np.array([5, 7, 11], np.int64), [0, 0, 2, 2, 3, 3]).tolist() == [0, 12, 0, 11, 0]
    assert A.segment_sums(np.zeros(0, np.int64), [0, 0, 0]).tolist() == [0, 0]
    with pytest.raises(AssertionError, match="does not fit int64"):
        big = A.Csr(1, 1, np.array([0, 4], np.int32), np.zeros(4, np.int32), np.full(4, 2.0 ** 52))
        A.row_sums(big, np.array([2.0 ** 9]))


def test_every_wide_gpu_problem_fills_both_halves():
    """every (matrix, precision, pair) the wide draw runs on the GPU: the bound (model() asserts it), at least 95 % of the rows with
    entries have a y with a non-zero low half (low 32 bits of an fp64 pattern, low 16 of an fp32 one), and in fp64 at least 90 % of
    the running sums of every row longer than a tile, taken after every 1792nd and every 2816th entry -- what carries and records are
    made of --, have non-zero low 32 bits.  Conditions on the data: a shape that cannot meet one needs another shape or draw."""
    E = _gpu_file()
    assert E.WUSED, "no wide problem is registered"
    # (the planted shapes are about which rows of y are read, not about a dispatch path's sums)
    assert set(label for label, _ in E.WUSED) == set(label for label, _ in E.USED if not label.startswith("planted:")), \
        "a problem the narrow draw runs and the wide one does not"
    long_rows = 0
    for (label, prec), pairs in sorted(E.WUSED.items()):
        P = E.problem(label, prec, E.WIDE)
        assert {(1, 0), E.NEG_ALPHA_ZERO_BETA} <= pairs and any(b != 0 for _, b in pairs)
        for alpha, beta in sorted(pairs):
            share = A.low_half_share(P.csr, P.want(alpha, beta))
            assert share >= 0.95, (label, prec, alpha, beta, share)
        if prec == "f64":
            for row, count, share in A.carry_low_half_shares(P.csr, P.x):
                long_rows += 1
                assert count >= 1 and share >= 0.90, (label, row, count, share)
    assert long_rows > 200


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


# ------------------------------------------------------------------------------------------------ zeros and their signs

def test_the_zero_sign_rule_by_hand():
    # x = [+0, -0, 1, -1];  row 0: kind (ii) -2 * +0, -0 * 1;  row 1: kind (i);  row 2: 1 - 1 cancels;  row 3: empty;  row 4: 2 * 1
    off = np.array([0, 2, 4, 6, 6, 7], np.int32)
    col = np.array([0, 2, 2, 3, 2, 2, 2], np.int32)
    for dtype in (np.float32, np.float64):
        val = np.array([-2, -0.0, 0.0, -0.0, 1, -1, 2], dtype)
        x = np.array([0.0, -0.0, 1, -1], dtype)
        csr = A.Csr(5, 4, off, col, val)
        c = A.census(csr, x, np.zeros(5, dtype), [(1, 1)], [4])
        assert (c["kind_i"], c["kind_ii"], c["kind_iii"], c["empty"]) == (1, 1, 1, 1) and c["kind_i_mixed_signs"] == 1
        y0 = np.array([-0.0, 0.0, 5, -0.0, -0.0], dtype)
        neg, pos = A.bits(np.array([-0.0], dtype))[0], 0
        two = A.bits(np.array([2], dtype))[0]
        # beta == 0: every zero is +0.0, whatever the sign of alpha
        for alpha in (1, -0.5, 2):
            assert A.bits(A.model(csr, x, y0, alpha, 0)).tolist()[:4] == [pos] * 4
        # t = 1 * -0.0 on rows 0 and 3: alpha * (+0.0) + (-0.0) is -0.0 for a negative alpha only; row 1: t = +0.0
        assert A.bits(A.model(csr, x, y0, 1, 1)).tolist() == [pos, pos, A.bits(np.array([5], dtype))[0], pos, two]
        assert A.bits(A.model(csr, x, y0, -0.5, 3)).tolist()[:2] == [neg, pos] and A.bits(A.model(csr, x, y0, -0.5, 3))[3] == neg
        # a negative beta turns the signs round: now row 1 (y0 = +0.0) has t = -0.0
        assert A.bits(A.model(csr, x, y0, -1.5, -1)).tolist()[:2] == [pos, neg]
        assert A.bits(A.model(csr, x, y0, 0, -2)).tolist()[:2] == [pos, pos]           # alpha == 0: 0 * (+0.0) is +0.0
        # the undefined corner is refused: t = -0.0 on the row whose non-zero products cancel
        bad = y0.copy(); bad[2] = -0.0
        with pytest.raises(AssertionError, match="outside the definition"):
            A.model(csr, x, bad, 1, 1)
        A.model(csr, x, bad, 1, -1)                                                     # (t = +0.0 there: defined, +0.0)
        bad = y0.copy(); bad[4] = 0.0                                                   # alpha == 0 leaves a zero result under t = -0.0
        with pytest.raises(AssertionError, match="outside the definition"):
            A.model(csr, x, bad, 0, -2)


def test_zero_problem_draws_what_it_says():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 9, 800); lens[11] = 5000; lens[12] = 301; lens[13] = 300
    for dtype in (np.float32, np.float64):
        csr, x, y0 = A.zero_problem(rng, 800, 50, lens, dtype, forced={20: A.KIND_II, 21: A.KIND_III})
        assert np.array_equal(np.diff(csr.row_offsets), lens)
        assert set(np.unique(np.abs(csr.values))) == {0, 1, 2} and set(np.unique(np.abs(x))) == {0, 1, 2, 3}
        c = A.census(csr, x, y0, A.PAIRS, [256 * 7, 256 * 11])
        for key in ("kind_i", "kind_ii", "kind_iii", "kind_i_mixed_signs", "kind_ii_crosses:1792", "kind_ii_crosses:2816", "zero_results_under_negative_zero_t",
                    "values:+0", "values:-0", "x:+0", "x:-0", "y0:+0", "y0:-0"):
            assert c[key] > 0, (key, c)
        assert c["longest_kind_ii"] == 5000
        off = csr.row_offsets
        for r in range(800):
            cc = csr.column_indices[off[r]:off[r + 1]]
            assert np.all(np.diff(cc) >= 0) and np.all((cc >= 0) & (cc < 50))
        prod = csr.values * x[csr.column_indices]
        for r in (11, 20):                                       # kind (ii): every product -0.0
            pr = prod[off[r]:off[r + 1]]
            assert pr.size and np.all(pr == 0) and np.all(np.signbit(pr))
        for r in (12, 21):                                       # kind (iii): non-zero products that cancel
            pr = prod[off[r]:off[r + 1]]
            assert pr.any() and pr.sum() == 0
        assert not csr.values[off[13]:off[14]].any()             # kind (i)
        for alpha, beta in A.PAIRS + [(-0.5, 0)]:
            A.model(csr, x, y0, alpha, beta)                     # (the domain: no zero result under t = -0.0 with non-zero products)


def _fma(a, b, c, dtype):
    """a * b + c rounded once: exact in long double for the numbers of this model (alpha has a few bits, s at most 53)"""
    L = np.longdouble
    return dtype(L(a) * L(b) + L(c))


def _piece_sum(rng, prods, dtype, first_product_start=False):
    """one tile's share of a row in a random association: cut into runs, each summed left to right FROM +0.0 (a thread's running
    sum, a lane's partial), the runs folded in a random order of adjacent pairs (the scans, the group folds)"""
    n = len(prods)
    cuts = sorted(set(rng.integers(1, n, rng.integers(0, 3)).tolist())) if n > 1 else []
    runs = []
    for a, b in zip([0] + cuts, cuts + [n]):
        if first_product_start:
            acc = prods[a]
            for p in prods[a + 1:b]:
                acc = dtype(acc + p)
        else:
            acc = dtype(0.0)
            for p in prods[a:b]:
                acc = dtype(acc + p)
        runs.append(acc)
    while len(runs) > 1:
        i = int(rng.integers(0, len(runs) - 1))
        runs[i:i + 2] = [dtype(runs[i] + runs[i + 1])]
    return runs[0]


def _any_path(rng, prods, y0, alpha, beta, dtype, first_product_start=False):
    """y of one row as some path may compute it: tile cuts anywhere, the last piece's sum enters alpha * s + t (fused or not), every
    other piece is a carry that is added into s first or arrives as y + alpha * c (fused or not), in a random order"""
    alpha, beta = dtype(alpha), dtype(beta)
    n = len(prods)
    cuts = sorted(set(rng.integers(0, n + 1, rng.integers(0, 4)).tolist())) if n else []    # (a cut at 0 or n: an empty piece, as a
    bounds = [0] + cuts + [n]                                                                #  tile that begins at the row's end)
    pieces = [_piece_sum(rng, prods[a:b], dtype, first_product_start) if b > a else dtype(0.0) for a, b in zip(bounds[:-1], bounds[1:])]
    s, carries = pieces[-1], pieces[:-1]
    later = []
    for k in rng.permutation(len(carries)):
        if rng.integers(0, 2):
            s = dtype(s + carries[k])
        else:
            later.append(carries[k])
    t = dtype(0.0) if beta == 0 else dtype(beta * y0)
    y = _fma(alpha, s, t, dtype) if rng.integers(0, 2) else dtype(dtype(alpha * s) + t)
    for c in later:
        y = _fma(alpha, c, y, dtype) if rng.integers(0, 2) else dtype(y + dtype(alpha * c))
    return y


@pytest.mark.parametrize("which", ["plain", "bottom", "bottom_stored", "top"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_definition_is_association_free(dtype, which):
    """Rows of up to 6 products from {+-2, +-1, +-0} x {+-3 .. +-0}, planted kinds included, computed in the compute type with numpy
    scalars under random tile cuts, random association inside each piece, carries folded into s or into y in random order, fused and
    unfused: with every piece started from +0.0 the bits are model()'s on every row -- no mask is needed --, at the plain scale and
    with the granule at the smallest subnormal and at 2^(emax - mantissa bits) (so numpy's own arithmetic is shown exact there).
    Started from the first product instead, rows differ: the test can tell the two behaviours apart."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(77)
    rows = 1500
    lens = rng.integers(0, 7, rows)
    pairs = A.PAIRS + [(-0.5, 0)] if which == "plain" else A.SCALE_PAIRS
    base = A.zero_problem(rng, rows, 12, lens, dtype)
    ev, ex = (0, 0) if which == "plain" else A.scale_exponents(dtype, which, pairs)
    csr, x, y0 = A.scaled(base, ev, ex)
    off = csr.row_offsets
    tiny = np.finfo(dtype).tiny
    wrong_from_first = 0
    with np.errstate(under="ignore"):
        prod = [dtype(v * x[c]) for v, c in zip(csr.values, csr.column_indices)]
        if which.startswith("bottom"):
            assert all(abs(p) < 64 * tiny for p in prod) and any(0 < abs(p) < tiny for p in prod)
        for alpha, beta in pairs:
            want = A.model(*base, alpha, beta, scale=ev + ex)
            if which == "top":
                assert np.isfinite(want).all() and np.abs(want).max() >= 2.0 ** A.TOP[np.dtype(dtype)]
            wb = A.bits(want)
            for r in range(rows):
                pr = prod[off[r]:off[r + 1]]
                for _ in range(3):
                    got = _any_path(rng, pr, y0[r], alpha, beta, dtype)
                    assert A.bits(np.array([got], dtype))[0] == wb[r], (r, alpha, beta, got, want[r], pr, y0[r])
                wrong_from_first += A.bits(np.array([_any_path(rng, pr, y0[r], alpha, beta, dtype, True)], dtype))[0] != wb[r]
    assert wrong_from_first > 0


def test_every_zero_laden_gpu_problem_has_its_rows_and_is_in_the_domain():
    """every (matrix, data variant, pair) of the zero-laden GPU tests: the bound, the domain of the sign rule (model() asserts both), that
    the scaled arrays are representable, and the census -- each kind of row present wherever the shape can hold it, a kind-(ii) row
    across a tile boundary of every tile size wherever a row is longer than a tile, zero results under t = -0.0"""
    E = _gpu_file()
    assert E.ZUSED, "no zero-laden problem is registered"
    seen = set()
    for (label, prec, data), pairs in sorted(E.ZUSED.items()):
        P = E.problem(label, prec, data)
        for alpha, beta in sorted(pairs):
            P.want(alpha, beta)
        if (label, prec) in seen:
            continue
        seen.add((label, prec))
        csr, x, y0 = P.base
        c = A.census(csr, x, y0, sorted(pairs), E.PLANTED_TILES)
        lens = np.diff(csr.row_offsets.astype(np.int64))
        with_entries = int((lens > 0).sum())
        if with_entries >= 1:
            assert c["kind_ii"] > 0 and c["longest_kind_ii"] == c["longest"], (label, prec, c)
        if with_entries >= 3:
            assert c["kind_i"] > 0, (label, prec, c)
        if int((lens >= 2).sum()) >= 2 and (x != 0).any():
            assert c["kind_iii"] > 0, (label, prec, c)
        for T in E.PLANTED_TILES:
            if c["longest"] > T:
                assert c[f"kind_ii_crosses:{T}"] > 0, (label, prec, T, c)
        if csr.rows >= 1000 and any(b != 0 for _, b in pairs):
            assert c["zero_results_under_negative_zero_t"] > 0, (label, prec, c)
        if csr.nnz >= 1000:
            assert c["values:+0"] > 0 and c["values:-0"] > 0, (label, prec, c)
        if csr.cols >= 4:
            assert c["x:+0"] > 0 and c["x:-0"] > 0, (label, prec, c)
        for want_label, keys in E.CENSUS_MUST.items():
            if label.startswith(want_label):
                for key in keys:
                    assert c[key.format(tile=label.split(":")[-1])] > 0, (label, prec, key, c)
