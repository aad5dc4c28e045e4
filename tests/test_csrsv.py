"""The level-scheduled sparse triangular solve (include/mspmv.h: mspmv_csrsv_*; merge_spmv_amd.CsrSv / csrsv): op(A) x = alpha * b.
CPU: exports, argument conventions (nothing launched, no device), wrapper refusals, and the numpy model (tests/csrsv_model.py) pinned
to exact rational arithmetic rounded per operation and to a hand-written example of levels.  GPU: the plan's levels, order, level
offsets and launches against the model, and x by torch.equal on the BIT PATTERNS against the model; the guard words around x stay
untouched, the matrix arrays and b stay unchanged.  Expected values never come from the library."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import csrsv_model as model

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csrsv_plan_create", "mspmv_csrsv_plan_info", "mspmv_csrsv_plan_order", "mspmv_csrsv_plan_level_offsets",
       "mspmv_csrsv_solve_f32", "mspmv_csrsv_solve_f64", "mspmv_csrsv_plan_destroy"]
MAX_ITEMS = 2 ** 31 - 1 - 65536
NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csrsv_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" T {name}\n" in out + "\n", (kind, name)
        assert sorted(re.findall(r" T (mspmv_csrsv_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("MSPMV_CSRSV_LOWER 0", "MSPMV_CSRSV_UPPER 1", "MSPMV_CSRSV_NON_UNIT 0", "MSPMV_CSRSV_UNIT 1"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name
    assert "CsrSv" in M.__all__ and "csrsv" in M.__all__ and callable(M.csrsv)
    assert lib.mspmv_version() == 102


def _create(rows, nnz, uplo=0, diag=0, off=ctypes.c_void_p(4096), col=ctypes.c_void_p(4096), plan=True):
    lib = M.load_library()
    handle = ctypes.c_void_p(0)
    status = lib.mspmv_csrsv_plan_create(ctypes.byref(handle) if plan else None, off, col, rows, nnz, uplo, diag, None, 0)
    return status, handle


def test_csrsv_argument_conventions():
    """every refusal comes before anything is launched or allocated: this runs without a device"""
    lib = M.load_library()
    assert _create(-1, 0)[0] == 1 and _create(5, -1)[0] == 1
    assert _create(MAX_ITEMS + 1, 0)[0] == 1 and _create(1000, MAX_ITEMS - 1000 + 1)[0] == 1 and _create(2 ** 31 - 1, 2 ** 31 - 1)[0] == 1
    for bad in (-1, 2, 7):
        assert _create(5, 7, uplo=bad)[0] == 1 and _create(5, 7, diag=bad)[0] == 1
        assert _create(0, 0, uplo=bad)[0] == 1 and _create(0, 0, diag=bad)[0] == 1
    assert _create(5, 7, off=None)[0] == 1 and _create(5, 7, col=None)[0] == 1
    assert _create(0, 7)[0] == 1                                  # entries without rows
    assert _create(0, 0, plan=False)[0] == 1                      # nowhere to put the plan
    # a NULL plan
    info = M._CsrSvInfo()
    f = ctypes.c_void_p(4096)
    assert lib.mspmv_csrsv_plan_info(None, ctypes.byref(info)) == 1 and lib.mspmv_csrsv_plan_destroy(None) == 1
    assert lib.mspmv_csrsv_plan_order(None) is None and lib.mspmv_csrsv_plan_level_offsets(None) is None
    assert lib.mspmv_csrsv_solve_f32(None, f, f, f, 1.0, f, f, None, 0) == 1 and lib.mspmv_csrsv_solve_f64(None, f, f, f, 1.0, f, f, None, 0) == 1
    # rows == 0: a valid plan with 0 levels and 0 launches, for every triangle and diagonal; a solve on it launches nothing
    for uplo in (0, 1):
        for diag in (0, 1):
            status, handle = _create(0, 0, uplo, diag, off=None, col=None)
            assert status == 0 and handle.value
            assert lib.mspmv_csrsv_plan_info(handle, None) == 1
            assert lib.mspmv_csrsv_plan_info(handle, ctypes.byref(info)) == 0
            assert (info.rows, info.nnz, info.uplo, info.diag, info.levels, info.launches, info.max_level_rows) == (0, 0, uplo, diag, 0, 0, 0)
            assert info.bad_diagonal_row == -1 and info.used_entries == 0 and info.device_bytes == 0 and info.narrow_rows >= 1
            assert lib.mspmv_csrsv_solve_f32(handle, None, None, None, 1.0, None, None, None, 0) == 0
            assert lib.mspmv_csrsv_solve_f64(handle, None, None, None, 1.0, None, None, None, 0) == 0
            assert lib.mspmv_csrsv_plan_destroy(handle) == 0


def test_csrsv_wrapper_rejects_bad_tensors_without_a_device():
    off, col = torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(M.MspmvError):
        M.CsrSv(off, col)                                         # not on the device
    with pytest.raises(M.MspmvError):
        M.CsrSv(None, col)
    with pytest.raises(M.MspmvError):
        M.csrsv(torch.zeros(0), off, col, torch.zeros(3))
    with pytest.raises(M.MspmvError):
        M.csrsv(torch.zeros(0), off, col, torch.zeros(3), lower=False, unit_diagonal=True)


# ---- exact rational arithmetic, rounded per operation to the nearest, ties to even (subnormals included)
def _round(fr, dtype):
    p, emin = (24, -126) if dtype == np.float32 else (53, -1022)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    n = round(a / quantum)                                       # (Fraction.__round__: ties to even)
    v = float(n * quantum)                                       # (exact: at most 53 bits)
    return dtype(-v if fr < 0 else v)


def _mul(a, b, dtype):
    fr = Fraction(float(a)) * Fraction(float(b))
    if fr == 0:
        return dtype(-0.0) if bool(np.signbit(a)) != bool(np.signbit(b)) else dtype(0.0)
    return _round(fr, dtype)


def _add(a, b, dtype):
    fr = Fraction(float(a)) + Fraction(float(b))
    if fr == 0:
        return dtype(-0.0) if (np.signbit(a) and np.signbit(b)) else dtype(0.0)
    return _round(fr, dtype)


def _sub(a, b, dtype):
    return _add(a, -b, dtype)


def _div(a, b, dtype):
    fr = Fraction(float(a)) / Fraction(float(b))
    if fr == 0:
        return dtype(-0.0) if bool(np.signbit(a)) != bool(np.signbit(b)) else dtype(0.0)
    return _round(fr, dtype)


def _exact(off, col, val, b, alpha, lower, unit, dtype):
    rows = len(off) - 1
    x = np.zeros(rows, dtype)
    for r in (range(rows) if lower else range(rows - 1, -1, -1)):
        s, d = dtype(0.0), None
        for e in range(off[r], off[r + 1]):
            c = int(col[e])
            if model.in_triangle(r, c, lower):
                s = _add(s, _mul(val[e], x[c], dtype), dtype)
            elif c == r:
                d = val[e]
        v = _sub(_mul(dtype(alpha), b[r], dtype), s, dtype)
        x[r] = v if unit else _div(v, d, dtype)
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _csr(rowlists):
    off = np.zeros(len(rowlists) + 1, np.int32)
    np.cumsum([len(r) for r in rowlists], out=off[1:])
    return off, np.asarray([c for r in rowlists for c in r], np.int32)


def _values(off, col, rng, dtype):
    """diagonal in [1, 2], everything else in [-1, 1] divided by the row length; general mantissas"""
    val = np.empty(len(col), dtype)
    for r in range(len(off) - 1):
        n = int(off[r + 1] - off[r])
        for e in range(off[r], off[r + 1]):
            val[e] = rng.uniform(1, 2) if col[e] == r else rng.uniform(-1, 1) / n
    return val


def _flip(rowlists):
    """the mirror image: (r, c) -> (n-1-r, n-1-c); a lower pattern becomes an upper one with the same levels"""
    n = len(rowlists)
    return [[n - 1 - c for c in row] for row in reversed(rowlists)]


SIX = [[0], [1], [0, 2, 1], [3, 1], [4, 2, 5], [3, 4, 5, 0]]     # unsorted rows; (4, 5) lies in the upper triangle


def test_the_model_levels_on_a_hand_written_example():
    off, col = _csr(SIX)
    assert model.levels(off, col, True).tolist() == [0, 0, 1, 1, 2, 3]
    order, lo = model.schedule(model.levels(off, col, True))
    assert order.tolist() == [0, 1, 2, 3, 4, 5] and lo.tolist() == [0, 2, 4, 5, 6]
    # the upper triangle of the same matrix holds (4, 5) alone: row 4 waits for row 5
    assert model.levels(off, col, False).tolist() == [0, 0, 0, 0, 1, 0]
    order, lo = model.schedule(model.levels(off, col, False))
    assert order.tolist() == [0, 1, 2, 3, 5, 4] and lo.tolist() == [0, 5, 6]
    assert model.used_entries(off, col, True) == 7 and model.used_entries(off, col, False) == 1
    assert model.bad_diagonal_row(off, col) == -1
    off2, col2 = _csr([[0], [1, 1], [0], [3]])
    assert model.bad_diagonal_row(off2, col2) == 1 and model.bad_diagonal_row(off2, col2, unit=True) == -1
    off3, col3 = _csr([[0], [1], [0], [3, 3]])
    assert model.bad_diagonal_row(off3, col3) == 2
    # segments: runs of narrow levels fuse, a wide level stands alone
    assert model.segments([0, 2, 4, 5, 6], 2) == [(0, 4, True)]
    assert model.segments([0, 2, 4, 5, 6], 1) == [(0, 1, False), (1, 2, False), (2, 4, True)]
    assert model.segments([0, 3, 4, 9, 10, 11, 20], 4) == [(0, 2, True), (2, 3, False), (3, 5, True), (5, 6, False)]
    assert model.segments([0], 4) == []
    info, _, _ = model.plan_info(off, col, True, False, 2)
    assert (info["levels"], info["launches"], info["max_level_rows"], info["used_entries"]) == (4, 1, 2, 7)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_hand_written_cases(dtype):
    """the model's arithmetic is the definition's: exact rationals rounded per operation, on tiny cases of every kind"""
    rng = np.random.default_rng(5)
    cases = [SIX, _flip(SIX), [[0]], [[], [0], [1, 0, 0]], [[1, 0], [1], [2, 0, 1, 1]], [[0, 2], [1, 2, 0], [2]]]
    for rowlists in cases:
        off, col = _csr(rowlists)
        for lower in (True, False):
            for unit in (False, True):
                if not unit and model.bad_diagonal_row(off, col) >= 0:
                    continue
                for alpha in (1.0, -0.5, 0.0, 1 / 3):
                    val = _values(off, col, rng, dtype)
                    b = rng.uniform(-1, 1, len(rowlists)).astype(dtype)
                    want = _exact(off, col, val, b, alpha, lower, unit, dtype)
                    got = model.solve(off, col, val, b, alpha, lower, unit)
                    assert got.dtype == dtype and np.array_equal(_bits(got), _bits(want)), (rowlists, lower, unit, alpha)
    # a sum that rounds differently when fused or reordered: s = 1 * (1 + 2^-p) ... checked through the exact path on fixed values
    off, col = _csr([[0], [1], [0, 1, 2]])
    eps = np.finfo(dtype).eps
    val = np.array([1, 1, 1 + eps, -(1 + eps), 1], dtype)
    b = np.array([1 + eps, 1 - eps / 2, eps], dtype)
    want = _exact(off, col, val, b, 1.0, True, False, dtype)
    assert np.array_equal(_bits(model.solve(off, col, val, b)), _bits(want))


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 8
SENTINEL = 12345.0


def _raw(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _shifted(a, shift_bytes, tdt=None):
    """a host array as a device tensor whose first element sits shift_bytes behind a 16-byte boundary (whole elements)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    k = shift_bytes // t.element_size()
    buf = torch.zeros(k + t.numel(), dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[k:]
    view.copy_(t)
    return buf, view


def _guarded(rows, tdt, fill=None):
    buf = torch.full((GUARD + rows + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    x = buf[GUARD: GUARD + rows]
    if fill is not None:
        x.copy_(torch.from_numpy(fill))
    return buf, x


def _guards_intact(buf, rows):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + rows:] == SENTINEL).all())


def _check_plan(plan, off, col, lower, unit):
    """levels, launches, figures, order and level offsets against the model, W read from the plan"""
    W = plan.info["narrow_rows"]
    assert W >= 1
    want, order, lo = model.plan_info(off, col, lower, unit, W)
    got = {k: plan.info[k] for k in want}
    assert got == want
    assert plan.info["device_bytes"] >= 4 * (len(order) + len(lo)) if len(order) else plan.info["device_bytes"] == 0
    assert torch.equal(plan.order.cpu(), torch.from_numpy(order)), "order"
    assert torch.equal(plan.level_offsets.cpu(), torch.from_numpy(lo)), "level_offsets"
    return want


def run(prec, rowlists, lower=True, unit=False, alpha=1.0, seed=0, shift=0, in_place=False, poison=False, val=None):
    """One plan and one solve on guarded, possibly misaligned arrays: the plan against the model, x bit for bit against the model,
    the inputs unchanged.  poison: every entry the solve must ignore holds NaN.  Returns (plan, info, arrays) for further solves."""
    dtype, tdt = NP[prec], TORCH[prec]
    rng = np.random.default_rng(seed)
    off, col = _csr(rowlists)
    rows = len(rowlists)
    if val is None:
        val = _values(off, col, rng, dtype)
    if poison:
        r_of = np.repeat(np.arange(rows), np.diff(off))
        ignored = ~(model.in_triangle(r_of, col, lower) | ((col == r_of) & (not unit)))
        val = val.copy(); val[ignored] = np.nan
    b = rng.uniform(-1, 1, rows).astype(dtype)
    want = model.solve(off, col, val, b, alpha, lower, unit)
    assert np.isfinite(want).all()
    obuf, d_off = _shifted(off, shift)
    cbuf, d_col = _shifted(col, shift)
    vbuf, d_val = _shifted(val, shift if shift % val.itemsize == 0 else val.itemsize)   # (whole elements: fp64 moves by 8 bytes)
    if shift:
        assert d_off.data_ptr() % 16 == shift and (col.size == 0 or d_col.data_ptr() % 16 == shift) and (val.size == 0 or d_val.data_ptr() % 16 in (shift, 8))
    d_b = torch.from_numpy(b).cuda()
    xbuf, d_x = _guarded(rows, tdt, fill=b if in_place else None)
    plan = M.CsrSv(d_off, d_col, lower=lower, unit_diagonal=unit)
    info = _check_plan(plan, off, col, lower, unit)
    keep = [_raw(t).clone() for t in (obuf, cbuf, vbuf, d_b)]
    got = plan.solve(d_val, d_x if in_place else d_b, x=d_x, alpha=alpha)
    torch.cuda.synchronize()
    assert got is d_x
    assert torch.equal(_raw(d_x).cpu(), torch.from_numpy(_bits(want))), (prec, lower, unit, alpha)
    assert _guards_intact(xbuf, rows), "guard words written"
    for t, was in zip((obuf, cbuf, vbuf, d_b), keep):
        assert torch.equal(_raw(t), was), "an input was modified"
    return plan, info, dict(off=off, col=col, val=val, b=b, d_off=d_off, d_col=d_col, d_val=d_val, d_b=d_b, d_x=d_x, xbuf=xbuf, want=want,
                            keep=(obuf, cbuf, vbuf))


def _W():
    status, handle = _create(0, 0, off=None, col=None)
    info = M._CsrSvInfo()
    lib = M.load_library()
    assert status == 0 and lib.mspmv_csrsv_plan_info(handle, ctypes.byref(info)) == 0 and lib.mspmv_csrsv_plan_destroy(handle) == 0
    return int(info.narrow_rows)


def _orient(rowlists, lower):
    return rowlists if lower else _flip(rowlists)


def _chain(n):
    return [[0]] + [[r - 1, r] for r in range(1, n)]


def _grid(n):
    return [[c for c in ((i - 1) * n + j if i else -1, i * n + j - 1 if j else -1, i * n + j) if c >= 0] for i in range(n) for j in range(n)]


def _layered(sizes, rng, extra=0, fan=3):
    """levels of the given sizes, numbered level by level: a row names one row of the level below and up to fan - 1 rows anywhere
    before its level, then its diagonal; `extra` rows with a diagonal alone come last (they belong to level 0, so order != identity)"""
    rowlists, start = [], 0
    for k, n in enumerate(sizes):
        for _ in range(n):
            if k == 0:
                rowlists.append([len(rowlists)])
            else:
                prev0 = start - sizes[k - 1]
                deps = [int(rng.integers(prev0, start))] + [int(c) for c in rng.integers(0, start, int(rng.integers(0, fan)))]
                rowlists.append(deps + [len(rowlists)])
        start += n
    return rowlists + [[len(rowlists) + i] for i in range(extra)]


def _messy(n, rng, unit):
    """a FULL matrix: entries on both sides of the diagonal in random stored order, repeated columns inside both strict triangles,
    the diagonal somewhere in the middle of its row; unit: some rows empty, some diagonals missing, some stored twice"""
    rowlists = []
    for r in range(n):
        k = int(rng.integers(0, 9))
        cs = [int(c) for c in rng.integers(0, n, k) if c != r]
        cs += cs[:2]                                                 # repeated columns
        d = [r]
        if unit:
            d = [[], [r], [r, r]][int(rng.integers(0, 3))]
            if rng.integers(0, 5) == 0:
                cs = []
                d = []                                               # an empty row
        cs = cs + d
        rng.shuffle(cs)
        rowlists.append(cs)
    return rowlists


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_degenerate_sizes(prec):
    for lower in (True, False):
        for unit in (False, True):
            plan, info, _ = run(prec, [], lower, unit)
            assert (info["levels"], info["launches"]) == (0, 0)
            plan, info, _ = run(prec, [[0]], lower, unit, alpha=-0.5)
            assert (info["levels"], info["launches"]) == (1, 1)
            plan, info, _ = run(prec, [[r] for r in range(300)], lower, unit, seed=1)     # a diagonal matrix
            assert (info["levels"], info["launches"], info["max_level_rows"], info["used_entries"]) == (1, 1, 300, 0)
        plan, info, a = run(prec, [[] for _ in range(37)], lower, True, alpha=-0.5, seed=2)   # nnz == 0 with UNIT: x = alpha * b
        assert (info["levels"], info["launches"]) == (1, 1)
        assert torch.equal(_raw(a["d_x"]).cpu(), torch.from_numpy(_bits((NP[prec](-0.5) * a["b"]).astype(NP[prec]))))


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bidiagonal_chain(prec, lower):
    plan, info, _ = run(prec, _orient(_chain(4096), lower), lower, seed=3)
    assert (info["levels"], info["launches"], info["max_level_rows"]) == (4096, 1, 1)


@gpu
@pytest.mark.parametrize("unit", [False, True], ids=["non_unit", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_five_point_grid(prec, lower, unit):
    plan, info, _ = run(prec, _orient(_grid(64), lower), lower, unit, seed=4)
    assert info["levels"] == 127 and info["max_level_rows"] == 64


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_two_levels_the_second_wide(prec, lower):
    """100 independent rows, then 2W + 37 rows that depend only on those: several workgroups, the last one ending inside a wave"""
    W = _W()
    rng = np.random.default_rng(6)
    rowlists = _layered([100, 2 * W + 37], rng)
    plan, info, _ = run(prec, _orient(rowlists, lower), lower, seed=6)
    assert info["levels"] == 2 and info["max_level_rows"] == 2 * W + 37
    assert info["launches"] == (2 if W >= 100 else len(model.segments([0, 100, 2 * W + 137], W)))


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_narrow_wide_transitions(prec, lower):
    """levels of exactly W - 1, W, W + 1 rows: narrow, narrow | wide | narrow | wide | narrow, narrow"""
    W = _W()
    rng = np.random.default_rng(7)
    sizes = [W - 1, W, W + 1, W - 1, W + 1, W, 3]
    rowlists = _layered(sizes, rng, extra=0)
    plan, info, _ = run(prec, _orient(rowlists, lower), lower, seed=7)
    assert info["levels"] == len(sizes) and info["launches"] == 5
    # the same with rows of level 0 at the far end: the first level grows past W, and order is no longer the identity
    rowlists = _layered(sizes, rng, extra=5)
    plan, info, _ = run(prec, _orient(rowlists, lower), lower, seed=8)
    assert info["levels"] == len(sizes) and info["launches"] == 6
    assert not torch.equal(plan.order.cpu(), torch.arange(len(rowlists), dtype=torch.int32))


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_long_row_among_short_ones(prec, lower):
    rng = np.random.default_rng(9)
    rowlists = _layered([40, 60, 5000, 30], rng)
    n = len(rowlists)
    long_row = [int(c) for c in rng.permutation(n)[:5000]] + [n]
    rowlists.append(long_row)                                      # 5000 strict entries in stored (random) order
    rowlists += [[n, n + 1], [n + 2, 3, n], [n + 3]]               # rows that wait for it
    plan, info, _ = run(prec, _orient(rowlists, lower), lower, seed=9)
    assert info["used_entries"] >= 5000


@gpu
@pytest.mark.parametrize("unit", [False, True], ids=["non_unit", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_full_unsorted_matrix_with_repeated_columns(prec, lower, unit):
    """unsorted rows, repeated strict columns, the other triangle present (a Gauss-Seidel sweep on A itself), stored diagonals under
    UNIT, empty rows: every entry the solve must ignore holds NaN"""
    rowlists = _messy(700, np.random.default_rng(10), unit)
    run(prec, rowlists, lower, unit, seed=10, poison=True)


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_arrays_off_16_byte_alignment(prec, lower):
    """row offsets, columns and values 4 bytes behind a 16-byte boundary (fp64 values: 8 bytes, the nearest a double can be)"""
    run(prec, _messy(300, np.random.default_rng(11), False), lower, seed=11, shift=4)
    run(prec, _orient(_chain(70), lower), lower, seed=11, shift=4)


@gpu
@pytest.mark.parametrize("alpha", [1.0, -0.5, 0.0])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_alpha(prec, alpha):
    for lower in (True, False):
        for unit in (False, True):
            run(prec, _messy(200, np.random.default_rng(12), unit), lower, unit, alpha=alpha, seed=12)


@gpu
def test_bad_diagonal_row():
    """a missing diagonal and a doubled one: the smallest row wins, the solve is refused, x is untouched"""
    base = _chain(50)
    for rowlists, bad in ((base[:7] + [[6]] + base[8:], 7), (base[:3] + [[2, 3, 3]] + base[4:7] + [[6]] + base[8:], 3),
                          (base[:20] + [[19, 20, 20]] + base[21:], 20)):
        off, col = _csr(rowlists)
        assert model.bad_diagonal_row(off, col) == bad
        for lower in (True, False):
            d_off, d_col = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda()
            plan = M.CsrSv(d_off, d_col, lower=lower)
            assert plan.info["bad_diagonal_row"] == bad
            for tdt, fn, ct in ((torch.float32, "mspmv_csrsv_solve_f32", ctypes.c_float), (torch.float64, "mspmv_csrsv_solve_f64", ctypes.c_double)):
                val = torch.ones(col.size, dtype=tdt, device="cuda")
                b = torch.ones(len(rowlists), dtype=tdt, device="cuda")
                xbuf, x = _guarded(len(rowlists), tdt)
                with pytest.raises(M.MspmvError):
                    plan.solve(val, b, x=x)
                status = getattr(M.load_library(), fn)(plan._handle, M._ptr(val), M._ptr(d_off), M._ptr(d_col), ct(1.0), M._ptr(b), M._ptr(x),
                                                       M._stream_handle(None), 0)
                torch.cuda.synchronize()
                assert status == 1
                assert bool((xbuf == SENTINEL).all())
            # the same pattern with a unit diagonal has no bad row and solves
            assert M.CsrSv(d_off, d_col, lower=lower, unit_diagonal=True).info["bad_diagonal_row"] == -1
    run("f64", base[:7] + [[6]] + base[8:], True, True, seed=13)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_reuse_in_place_and_repeatability(prec):
    dtype = NP[prec]
    rng = np.random.default_rng(14)
    rowlists = _layered([30, 50, 20, 70, 10], rng, extra=4)
    plan, info, a = run(prec, rowlists, True, seed=14)
    first = _raw(a["d_x"]).clone()
    # two consecutive solves are bit-equal
    plan.solve(a["d_val"], a["d_b"], x=a["d_x"])
    torch.cuda.synchronize()
    assert torch.equal(_raw(a["d_x"]), first)
    # new values on the same plan (a refactorisation), another alpha
    val2 = _values(a["off"], a["col"], rng, dtype)
    a["d_val"].copy_(torch.from_numpy(val2))
    plan.solve(a["d_val"], a["d_b"], x=a["d_x"], alpha=-0.5)
    torch.cuda.synchronize()
    want = model.solve(a["off"], a["col"], val2, a["b"], -0.5)
    assert torch.equal(_raw(a["d_x"]).cpu(), torch.from_numpy(_bits(want))) and _guards_intact(a["xbuf"], len(rowlists))
    # in place: x is b
    a["d_x"].copy_(a["d_b"])
    got = plan.solve(a["d_val"], a["d_x"], x=a["d_x"], alpha=-0.5)
    torch.cuda.synchronize()
    assert got is a["d_x"] and torch.equal(_raw(a["d_x"]).cpu(), torch.from_numpy(_bits(want))) and _guards_intact(a["xbuf"], len(rowlists))
    for lower in (True, False):
        run(prec, _orient(_grid(20), lower), lower, seed=15, in_place=True)
    # the one-shot call
    x = M.csrsv(a["d_val"], a["d_off"], a["d_col"], a["d_b"], alpha=-0.5)
    assert torch.equal(_raw(x).cpu(), torch.from_numpy(_bits(want)))
    plan.close()
    plan.close()
    with pytest.raises(M.MspmvError):
        plan.solve(a["d_val"], a["d_b"])


@gpu
def test_graph_capture_and_replay():
    """one solve of several launches (narrow, wide, narrow) captured, replayed twice with changed b"""
    W = _W()
    rng = np.random.default_rng(16)
    rowlists = _layered([20, W + 1, 30, 10], rng)
    plan, info, a = run("f32", rowlists, True, seed=16)
    assert info["launches"] == 3
    a["d_x"].fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.solve(a["d_val"], a["d_b"], x=a["d_x"], alpha=2.0)
    for seed in (17, 18):
        b = np.random.default_rng(seed).uniform(-1, 1, len(rowlists)).astype(np.float32)
        a["d_b"].copy_(torch.from_numpy(b))
        graph.replay()
        torch.cuda.synchronize()
        want = model.solve(a["off"], a["col"], a["val"], b, 2.0)
        assert torch.equal(_raw(a["d_x"]).cpu(), torch.from_numpy(_bits(want)))
        assert _guards_intact(a["xbuf"], len(rowlists))


@gpu
def test_launch_lines_number_the_launches(capfd):
    W = _W()
    rng = np.random.default_rng(19)
    for sizes in ([5], [20, W + 1, 30, W + 2, W + 3, 10], [W + 1]):
        rowlists = _layered(sizes, rng)
        plan, info, a = run("f64", rowlists, True, seed=19)
        capfd.readouterr()
        plan.solve(a["d_val"], a["d_b"], x=a["d_x"], debug_synchronous=True)
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
        assert len(lines) == info["launches"] == len(model.segments(model.schedule(model.levels(a["off"], a["col"]))[1], W)), lines
        narrow = [l.startswith("mspmv: sv_narrow_kernel<<<1,") for l in lines]
        assert narrow == [s[2] for s in model.segments(model.schedule(model.levels(a["off"], a["col"]))[1], W)]
        assert torch.equal(_raw(a["d_x"]).cpu(), torch.from_numpy(_bits(a["want"])))


@gpu
@pytest.mark.parametrize("unit", [False, True], ids=["non_unit", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_round_trip_residual(lower, unit):
    """meaning, not only bits: in fp64, |T x - alpha b| <= len * eps * (|T||x| + |b|) elementwise, T the extracted triangle multiplied
    through M.csrmv and len the entries of T's row: substitution (gamma_len |T||x|, Higham, Accuracy and Stability, 8.1) plus the
    rounding of the product that checks it (another gamma_len |T||x|), 2 len u = len eps"""
    alpha = -0.5
    rowlists = _messy(600, np.random.default_rng(20), unit)
    plan, info, a = run("f64", rowlists, lower, unit, alpha=alpha, seed=20)
    off, col, val, n = a["off"], a["col"], a["val"], len(rowlists)
    t_rows = []
    for r in range(n):
        ent = [(int(col[e]), float(val[e])) for e in range(off[r], off[r + 1]) if model.in_triangle(r, int(col[e]), lower)]
        ent.append((r, 1.0 if unit else next(float(val[e]) for e in range(off[r], off[r + 1]) if col[e] == r)))
        t_rows.append(ent)
    t_off, t_col = _csr([[c for c, _ in ent] for ent in t_rows])
    t_val = np.asarray([v for ent in t_rows for _, v in ent], np.float64)
    x = a["d_x"].clone()
    y = M.csrmv(torch.from_numpy(t_val).cuda(), torch.from_numpy(t_off).cuda(), torch.from_numpy(t_col).cuda(), x, num_cols=n)
    torch.cuda.synchronize()
    y, xh = y.cpu().numpy().astype(np.longdouble), x.cpu().numpy()
    lens = np.diff(t_off).astype(np.longdouble)
    mag = np.asarray([sum(abs(v) * abs(xh[c]) for c, v in ent) for ent in t_rows], np.longdouble)
    resid = np.abs(y - np.longdouble(alpha) * a["b"].astype(np.longdouble))
    bound = lens * np.longdouble(np.finfo(np.float64).eps) * (mag + np.abs(a["b"]).astype(np.longdouble))
    print("worst residual / bound:", float((resid / bound).max()))
    assert (resid <= bound).all()
