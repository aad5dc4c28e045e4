"""CPU guards of tests/mg_model.py, the model that tests/test_mg_exact.py holds the partitioned CsrMV to: the model's partition and
local CSR against the library's host entry points (up to 64 parts and with more parts than merge items), the model's carry routing
against the int64 model of the whole matrix, the condition under which the integer problems are exact, and a census that keeps the
problems on the edges they were chosen for."""
import numpy as np
import pytest

import axpby_model as AM
import mg_model as MM
from merge_spmv_amd import multi_gpu as MG

NAMES = sorted(MM.PROBLEMS)
DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("parts", MM.PARTS)
def test_partition_and_local_offsets_equal_the_librarys(name, parts):
    off = MM.offsets(name)
    rows, nnz = off.size - 1, int(off[-1])
    row_split, nz_split = MM.partition(off, parts)
    lib_rows, lib_nz = MG.partition(off, parts)
    assert np.array_equal(row_split, lib_rows) and np.array_equal(nz_split, lib_nz)
    assert (row_split[0], nz_split[0]) == (0, 0) and (row_split[-1], nz_split[-1]) == (rows, nnz)
    per = -(-(rows + nnz) // parts)
    assert np.all(np.diff(row_split) >= 0) and np.all(np.diff(nz_split) >= 0)
    assert np.all(np.diff(row_split) + np.diff(nz_split) <= per)
    csr, _ = MM.integer_problem(name, np.float32)
    assert np.array_equal(csr.row_offsets.astype(np.int64), off)
    for g in range(parts):
        local = MM.local_csr(csr, row_split, nz_split, g)
        lo = MG.local_offsets(off, row_split[g], row_split[g + 1], nz_split[g], nz_split[g + 1])
        assert local.row_offsets.dtype == np.int32 and np.array_equal(local.row_offsets, lo)
        assert lo[0] == 0 and lo[-1] == local.nnz == local.values.size == nz_split[g + 1] - nz_split[g] and np.all(np.diff(lo) >= 0)
        assert local.rows == row_split[g + 1] - row_split[g] + 1


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_problems_are_exact_in_both_precisions(name, dtype):
    """the condition, not a tolerance: an edited shape must not turn the exact tests into rounding-dependent ones"""
    csr, x = MM.integer_problem(name, dtype)
    assert np.all(csr.values != 0) and np.all(x != 0)
    q = AM.quotient(csr, x, None, 1, 0)
    assert q < AM.LIMIT[np.dtype(dtype)], (name, q)
    assert q <= 6 * 200_000 < 1 << 24                   # values +-{1,2}, x +-{1..3}, the longest row of any problem


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("parts", MM.PARTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_models_routing_reproduces_the_whole_matrix(name, parts, dtype):
    """exact int64 row sums of every part's local CSR, pushed through fold(), are the int64 model of the whole matrix bit for bit"""
    csr, x = MM.integer_problem(name, dtype)
    row_split, nz_split = MM.partition(csr.row_offsets.astype(np.int64), parts)
    y_locals = []
    for g in range(parts):
        s, _ = AM.row_sums(MM.local_csr(csr, row_split, nz_split, g), x)
        y_locals.append(s.astype(dtype))
    y, opens = MM.fold(y_locals, row_split, dtype)
    want = AM.model(csr, x, None, 1, 0)
    assert y.dtype == want.dtype == np.dtype(dtype)
    assert np.array_equal(AM.bits(y), AM.bits(want))
    assert opens.size == parts and all(AM.bits(opens[g:g + 1])[0] == AM.bits(y_locals[g][-1:])[0] for g in range(parts))
    # every carry is taken exactly once or belongs to nobody (it is the empty sum beyond the last row)
    src = MM.sources(row_split)
    taken = [s for lst in src for s in lst]
    assert len(taken) == len(set(taken))
    for g in range(parts):
        if g not in taken:
            assert opens[g] == 0 and not np.signbit(opens[g])
        assert all(s < g for s in src[g]) and src[g] == sorted(src[g])


@pytest.mark.parametrize("name", MM.WIDE_NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_problems_are_exact_and_fill_both_halves(name, dtype):
    """the wide draw of tests/test_mg_exact.py: the bound (model() asserts it), at least 95 % of the rows with entries have a y with
    a non-zero low half, in fp64 at least 90 % of the running sums of every row longer than a tile and of the non-zero open-row
    entries at every part count have one -- and the shared boundary rows do hand on such entries"""
    csr, x = MM.wide_problem(name, dtype)
    assert np.all(csr.values.astype(np.int64) % 2 == 1) and np.all(x.astype(np.int64) % 2 == 1)
    want = AM.model(csr, x, None, 1, 0)
    assert AM.low_half_share(csr, want) >= 0.95, name
    taken = 0
    for parts in MM.WIDE_PARTS:
        count, share = MM.wide_open_row_share(csr, x, parts)
        taken += count
        if dtype == np.float64:
            assert share >= 0.90, (name, parts, count, share)
        # the routing of the model on this draw as well
        row_split, nz_split = MM.partition(csr.row_offsets.astype(np.int64), parts)
        y_locals = [AM.row_sums(MM.local_csr(csr, row_split, nz_split, g), x)[0].astype(dtype) for g in range(parts)]
        assert np.array_equal(AM.bits(MM.fold(y_locals, row_split, dtype)[0]), AM.bits(want))
    if dtype == np.float64:
        assert all(share >= 0.90 for _, _, share in AM.carry_low_half_shares(csr, x)), name
    if name != "cuts_on_row_ends":
        assert taken >= (40 if name.startswith(("giant", "single")) else 2), (name, taken)


@pytest.mark.parametrize("dtype,worlds", [(np.float64, (2, 4)), (np.float32, (2,))])
def test_the_ipc_workers_wide_problem_hands_on_carries_with_a_low_word(dtype, worlds):
    """kind `wide` of tests/mg_ipc_worker.py at the process counts tests/test_mg_plan.py runs it with: the bound (model() asserts
    it), the giant row spans every rank (4 ranks: the middle ones own nothing), every rank but the last hands on a non-zero
    open-row entry -- the carry the hipIpc backend ships as two tagged 32-bit halves -- and in fp64 every one of them has non-zero
    low 32 bits, as have at least 95 % of the results"""
    lens, csr, x = MM.ipc_wide_problem(dtype)
    assert lens.size == MM.IPC_ROWS and lens.max() == MM.IPC_GIANT and np.array_equal(np.diff(csr.row_offsets), lens)
    want = AM.model(csr, x, None, 1, 0)
    assert AM.low_half_share(csr, want) >= 0.95
    for world in worlds:
        row_split, _ = MM.partition(csr.row_offsets.astype(np.int64), world)
        owned = np.diff(row_split)
        assert owned[0] > 0 and owned[-1] > 0 and (world < 4 or (owned[1:-1] == 0).all())
        count, share = MM.wide_open_row_share(csr, x, world)
        assert count == world - 1, (world, count)
        if dtype == np.float64:
            assert share == 1.0, (world, share)


def test_a_dropped_or_misrouted_carry_changes_the_models_result():
    """the fold is not vacuous on these problems: without the sources, or with one fewer, y differs from the whole-matrix model"""
    csr, x = MM.integer_problem("giant_middle", np.float64)
    row_split, nz_split = MM.partition(csr.row_offsets.astype(np.int64), 8)
    y_locals = [AM.row_sums(MM.local_csr(csr, row_split, nz_split, g), x)[0].astype(np.float64) for g in range(8)]
    want = AM.model(csr, x, None, 1, 0)
    plain = np.concatenate([yl[:-1] for yl in y_locals])
    assert not np.array_equal(plain, want)
    assert np.array_equal(MM.fold(y_locals, row_split, np.float64)[0], want)


def test_census_the_problems_keep_hitting_the_edges():
    c = MM.census("giant_middle", 64)
    assert c["zero_owned"] >= 50 and c["max_sources"] >= 50
    for parts in MM.PARTS:
        assert MM.census("single_row", parts)["max_sources"] == parts - 1
    assert MM.census("giant_then_empty_rows", 64)["zero_owned"] >= 50
    assert MM.census("fewer_items_than_parts", 64)["empty_parts"] >= 50
    for parts in (2, 8, 64):
        c = MM.census("cuts_on_row_ends", parts)
        assert c["taken"] == c["taken_empty"] == parts - 1          # every cut on a row end: every taken carry is the empty sum
    assert MM.census("empty_runs", 64)["takers"] >= 50
    for name in ("giant_first", "giant_last", "giant_middle", "single_row"):
        for parts in (3, 8, 64):
            assert MM.census(name, parts)["max_sources"] >= 2, (name, parts)      # where the ORDER of the fold shows
    for name in ("short", "power_law"):
        assert MM.census(name, 64)["takers"] >= 32
    c = MM.census("all_empty", 64)                                  # one row per part: every part takes its neighbour's empty carry
    assert c["zero_owned"] == 0 and c["taken"] == c["taken_empty"] == 63
