"""ILU(0) on the device (include/mspmv.h: mspmv_csrilu0_*; merge_spmv_amd.csrilu0 / Ilu0): A ~ L U on A's own pattern, along the levels
of a LOWER CsrSv plan.  CPU: exports, argument conventions (nothing launched, no device), wrapper refusals, and the numpy model
(tests/csrilu0_model.py) pinned to exact rational arithmetic rounded per operation, to a hand-written example, to the defining
property (L U = A on the pattern, in exact arithmetic) and to an integer tridiagonal L U that must come back exactly.  GPU: the factor
by torch.equal on the BIT PATTERNS against the model, the pivot against the model's, guard words around the factor intact, the
pattern arrays and (out of place) the values unchanged.  Expected values never come from the library."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import csrilu0_model as model
import csrsv_model as sv_model
import test_csrsv as SV            # noqa: E402 - _round/_mul/_sub/_div, _csr, _bits, _raw, _shifted, _layered, _grid, _create, _W

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csrilu0_group", "mspmv_csrilu0_f32", "mspmv_csrilu0_f64"]
NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}
PRECS = ["f32", "f64"]


# ---------------------------------------------------------------------------------------------------------------- patterns
def _sym(rowlists):
    """the pattern of L + L^T + I, rows sorted, no column twice"""
    n = len(rowlists)
    rows = [set([r]) for r in range(n)]
    for r, row in enumerate(rowlists):
        for c in row:
            rows[r].add(int(c)); rows[int(c)].add(r)
    return [sorted(s) for s in rows]


def _tridiag(n):
    return [[c for c in (r - 1, r, r + 1) if 0 <= c < n] for r in range(n)]


def _grid5(n):
    return _sym(SV._grid(n))


def _layered_sym(W, seed=7):
    return _sym(SV._layered([1, W + 1, 3, 2 * W + 5, W, 1], np.random.default_rng(seed), extra=5))


def _dense(n):
    return [list(range(n)) for _ in range(n)]


def _long_row(n=600):
    return _tridiag(n + 1)[:n] + [list(range(n + 1))]


def _cases(W):
    """name -> rowlists of every pattern the GPU tests factorise (test_the_groups_the_cases_take reads their sizes)"""
    return {"none": [], "one": [[0]], "diagonal": [[r] for r in range(300)], "empty": [[] for _ in range(37)], "chain": _tridiag(3000),
            "grid": _grid5(40), "layered": _layered_sym(W), "dense": _dense(70), "long_row": _long_row(), "shifted": _grid5(13),
            "capture": _sym(SV._layered([20, W + 1, 30, 10], np.random.default_rng(16)))}


def _values(off, col, rng, dtype):
    """off-diagonals uniform in (-1, 1), diagonals in [4, 5]: finite factors (the issue's recipe)"""
    r_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    val = rng.uniform(-1, 1, len(col))
    d = col == r_of
    val[d] = rng.uniform(4, 5, int(d.sum()))
    return val.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csrilu0_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r" T (mspmv_csrilu0_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert "csrilu0" in M.__all__ and "Ilu0" in M.__all__ and callable(M.csrilu0) and callable(M.Ilu0)
    assert lib.mspmv_version() == 102


def _call(lib, fn, handle, temp, size, arrays=(None, None, None, None), pivot=None):
    return getattr(lib, fn)(handle, temp, ctypes.byref(size) if size is not None else None, *arrays, pivot, None, 0)


def test_csrilu0_argument_conventions():
    """every refusal comes before anything is launched: this runs without a device"""
    lib = M.load_library()
    for fn in ("mspmv_csrilu0_f32", "mspmv_csrilu0_f64"):
        size = ctypes.c_size_t(12345)
        assert _call(lib, fn, None, None, size) == 1                                  # a NULL plan
        for diag in (0, 1):
            status, upper = SV._create(0, 0, 1, diag, off=None, col=None)
            assert status == 0 and _call(lib, fn, upper, None, size) == 1             # an UPPER plan
            assert _call(lib, fn, upper, ctypes.c_void_p(4096), size) == 1
            assert lib.mspmv_csrsv_plan_destroy(upper) == 0
            status, lower = SV._create(0, 0, 0, diag, off=None, col=None)
            assert status == 0
            assert _call(lib, fn, lower, None, None) == 1                             # nowhere to put the size
            size = ctypes.c_size_t(12345)
            assert _call(lib, fn, lower, None, size) == 0 and 0 <= size.value <= 64   # the size query: every pointer NULL
            need = size.value
            assert need % 16 == 0
            temp = ctypes.c_void_p(4096)
            assert _call(lib, fn, lower, temp, ctypes.c_size_t(need)) == 0            # rows == 0: succeeds, launches nothing
            if need > 0:
                assert _call(lib, fn, lower, temp, ctypes.c_size_t(need - 1)) == 1    # one byte too small
            for bad in (4097, 4100, 4104):
                assert _call(lib, fn, lower, ctypes.c_void_p(bad), ctypes.c_size_t(need + 64)) == 1   # misaligned
            assert lib.mspmv_csrsv_plan_destroy(lower) == 0
    g = ctypes.c_int32(0)
    assert lib.mspmv_csrilu0_group(-1, 0, ctypes.byref(g)) == 1 and lib.mspmv_csrilu0_group(5, -1, ctypes.byref(g)) == 1
    assert lib.mspmv_csrilu0_group(5, 5, None) == 1
    for rows, nnz in ((0, 0), (1, 0), (1, 1), (7, 7), (1000, 2998), (1600, 7840), (10, 330), (70, 4900), (3, 2 ** 31 - 70000), (2 ** 31 - 70000, 3)):
        assert lib.mspmv_csrilu0_group(rows, nnz, ctypes.byref(g)) == 0
        assert 1 <= g.value <= 64 and g.value & (g.value - 1) == 0 and g.value == model.group(rows, nnz), (rows, nnz, g.value)


def test_the_groups_the_cases_take():
    """across the GPU cases mspmv_csrilu0_group takes at least three values, its smallest and 64 among them"""
    got = {M.csrilu0_group(len(rows), sum(len(r) for r in rows)) for rows in _cases(SV._W()).values()}
    assert len(got) >= 3 and 1 in got and 64 in got, got


def test_csrilu0_wrapper_rejects_bad_tensors_without_a_device():
    off, col, val = torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    with pytest.raises(M.MspmvError):
        M.csrilu0(val, off, col)                                   # not on the device
    with pytest.raises(M.MspmvError):
        M.csrilu0(None, off, col)
    with pytest.raises(M.MspmvError):
        M.csrilu0(val, off, [0, 1])
    with pytest.raises(M.MspmvError):
        M.Ilu0(off, col)
    with pytest.raises(M.MspmvError):
        M.Ilu0(off, None)


def _eliminate(off, col, a, div, mul, sub, zero):
    """the definition of include/mspmv.h with the arithmetic handed in"""
    rows = len(off) - 1
    diag = {int(col[e]): e for r in range(rows) for e in range(off[r], off[r + 1]) if int(col[e]) == r}
    for i in range(rows):
        for e in range(off[i], off[i + 1]):
            k = int(col[e])
            if k >= i:
                continue
            a[e] = div(a[e], a[diag[k]] if k in diag else zero)
            for f in range(off[k], off[k + 1]):
                j = int(col[f])
                for g in range(off[i], off[i + 1]):
                    if j > k and int(col[g]) == j:
                        a[g] = sub(a[g], mul(a[e], a[f]))
    return a


def _rounded(off, col, val, dtype):
    a = _eliminate(off, col, list(val), lambda x, y: SV._div(x, y, dtype), lambda x, y: SV._mul(x, y, dtype), lambda x, y: SV._sub(x, y, dtype),
                   dtype(0.0))
    return np.asarray(a, dtype)


FOUR = [[0, 1, 3], [0, 1, 2], [1, 2, 3], [0, 2, 3]]
FOUR_A = [4, 1, 1, 2, 4.5, 1, 2, 4.5, 1, 1, 2, 4.75]
FOUR_LU = [4, 1, 1, 0.5, 4, 1, 0.5, 4, 1, 0.25, 0.5, 4]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_a_hand_written_example(dtype):
    """    A = [4 1   .   1   ]   row 1: l10 = 2/4 = .5; u11 = 4.5 - .5*1 = 4; (0,3) meets no entry of row 1: dropped
        [2 4.5 1   .   ]   row 2: l21 = 2/4 = .5; u22 = 4.5 - .5*1 = 4
        [. 2   4.5 1   ]   row 3: l30 = 1/4 = .25; (0,1) dropped; u33 = 4.75 - .25*1 = 4.5; l32 = 2/4 = .5; u33 = 4.5 - .5*1 = 4
        [1 .   2   4.75]   so LU = [4 1 . 1 | .5 4 1 . | . .5 4 1 | .25 . .5 4], every step exact
    then general mantissas against exact rationals rounded per operation"""
    off, col = SV._csr(FOUR)
    lu, pivot = model.ilu0(off, col, np.asarray(FOUR_A, dtype))
    assert lu.dtype == dtype and pivot == -1 and lu.tolist() == FOUR_LU
    rng = np.random.default_rng(1)
    for _ in range(5):
        val = _values(off, col, rng, dtype)
        lu, pivot = model.ilu0(off, col, val)
        assert pivot == -1 and np.array_equal(SV._bits(lu), SV._bits(_rounded(off, col, val, dtype)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_a_small_grid(dtype):
    off, col = SV._csr(_grid5(6))
    val = _values(off, col, np.random.default_rng(2), dtype)
    lu, pivot = model.ilu0(off, col, val)
    assert pivot == -1 and np.isfinite(lu).all()
    assert np.array_equal(SV._bits(lu), SV._bits(_rounded(off, col, val, dtype)))


def test_exact_ilu0_reproduces_a_on_the_pattern():
    """the defining property: in exact arithmetic (L U)ij = aij for every (i, j) of the pattern"""
    rowlists = _grid5(6)
    off, col = SV._csr(rowlists)
    val = _values(off, col, np.random.default_rng(3), np.float64)
    A = [Fraction(float(v)) for v in val]
    a = _eliminate(off, col, list(A), lambda x, y: x / y, lambda x, y: x * y, lambda x, y: x - y, Fraction(0))
    n = len(rowlists)
    entry = [{int(col[e]): a[e] for e in range(off[r], off[r + 1])} for r in range(n)]
    for i in range(n):
        for e in range(off[i], off[i + 1]):
            j = int(col[e])
            s = sum((1 if k == i else entry[i].get(k, 0)) * entry[k].get(j, 0) for k in range(min(i, j) + 1) if k == i or k in entry[i])
            assert s == A[e], (i, j)


def _integer_lu(n, rng, dtype):
    """tridiagonal A = L U from a unit lower bidiagonal L and an upper bidiagonal U of small integers, U's diagonal powers of two:
    (values of A, the expected factor in A's layout), all exact in fp32"""
    l = rng.integers(-3, 4, n); d = 2.0 ** rng.integers(0, 3, n); u = rng.integers(-3, 4, n)
    l[l == 0] = 1
    A, LU = [], []
    for r in range(n):
        if r:
            A.append(l[r] * d[r - 1]); LU.append(l[r])
        A.append(d[r] + (l[r] * u[r - 1] if r else 0)); LU.append(d[r])
        if r + 1 < n:
            A.append(u[r]); LU.append(u[r])
    return np.asarray(A, dtype), np.asarray(LU, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_integer_tridiagonal_lu_comes_back_exactly(dtype):
    n = 200
    off, col = SV._csr(_tridiag(n))
    A, LU = _integer_lu(n, np.random.default_rng(4), dtype)
    lu, pivot = model.ilu0(off, col, A)
    assert np.array_equal(SV._bits(lu), SV._bits(LU)) and pivot == -1


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 8
SENTINEL = 12345.0
_MODEL = {}                     # (name, prec, seed) -> (off, col, val, want, pivot): computed once, shared, never changed


def _reference(name, rowlists, prec, seed, val=None):
    key = (name, prec, seed)
    if key not in _MODEL:
        off, col = SV._csr(rowlists)
        if val is None:
            val = _values(off, col, np.random.default_rng(seed), NP[prec])
        want, pivot = model.ilu0(off, col, val)
        _MODEL[key] = (off, col, val, want, pivot)
    return _MODEL[key]


def _guarded(n, tdt, shift_elems=0):
    buf = torch.full((GUARD + shift_elems + n + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    return buf, buf[GUARD + shift_elems: GUARD + shift_elems + n]


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


def run(name, rowlists, prec, seed=0, val=None, shift=0, in_place=False, unit=True, finite=True):
    """One LOWER plan and one factorisation through M.csrilu0 on guarded, possibly misaligned arrays: the factor bit for bit against
    the model, the pivot against the model's, the inputs unchanged.  Returns a dict for further calls."""
    dtype, tdt = NP[prec], TORCH[prec]
    off, col, val, want, want_pivot = _reference(name, rowlists, prec, seed, val)
    if finite:
        assert np.isfinite(want).all() and want_pivot == -1
    assert not np.isnan(want).any()
    nnz = len(col)
    obuf, d_off = SV._shifted(off, shift)
    cbuf, d_col = SV._shifted(col, shift)
    vshift = (shift // val.itemsize or 1) if shift else 0                            # (whole elements: fp64 moves by 8 bytes)
    vbuf, d_val = _guarded(nnz, tdt, vshift)
    d_val.copy_(torch.from_numpy(val))
    lbuf, d_lu = (vbuf, d_val) if in_place else _guarded(nnz, tdt, vshift)
    if shift:
        assert d_off.data_ptr() % 16 == shift and d_col.data_ptr() % 16 == shift and d_val.data_ptr() % 16 != 0 and d_lu.data_ptr() % 16 != 0
    plan = M.CsrSv(d_off, d_col, lower=True, unit_diagonal=unit)
    keep = [SV._raw(t).clone() for t in (obuf, cbuf, vbuf)]
    lu, pivot = M.csrilu0(d_val, d_off, d_col, plan=plan, out=d_lu)
    torch.cuda.synchronize()
    assert lu is d_lu and pivot.dtype == torch.int32 and pivot.is_cuda and pivot.numel() == 1
    assert torch.equal(SV._raw(d_lu).cpu(), torch.from_numpy(SV._bits(want))), (name, prec)
    assert int(pivot.item()) == want_pivot
    assert _guards_intact(lbuf, d_lu), "guard words written"
    for t, was in zip((obuf, cbuf) if in_place else (obuf, cbuf, vbuf), keep):
        assert torch.equal(SV._raw(t), was), "an input was modified"
    return dict(plan=plan, off=off, col=col, val=val, want=want, pivot=want_pivot, d_off=d_off, d_col=d_col, d_val=d_val, d_lu=d_lu, lbuf=lbuf,
                keep=(obuf, cbuf, vbuf), G=M.csrilu0_group(len(rowlists), nnz))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_sizes(prec):
    dtype = NP[prec]
    cases = _cases(1)
    a = run("none", cases["none"], prec)
    assert a["plan"].info["launches"] == 0
    a = run("one", cases["one"], prec)
    assert a["G"] == 1
    # a diagonal matrix with a -0.0 and a negative entry: the values come back bit for bit, the pivot is the row of the -0.0
    val = np.random.default_rng(5).uniform(4, 5, 300).astype(dtype)
    val[17] = -3.5; val[201] = -0.0; val[250] = 0.0
    a = run("diagonal", cases["diagonal"], prec, val=val, finite=False)
    assert a["pivot"] == 201 and a["G"] == 1 and torch.equal(SV._raw(a["d_lu"]).cpu(), torch.from_numpy(SV._bits(val)))
    # no entries at all: row 0 already lacks its diagonal
    a = run("empty", cases["empty"], prec, finite=False)
    assert a["pivot"] == 0


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_tridiagonal_chain(prec):
    """one narrow launch of more levels than one LDS chunk of level offsets holds"""
    a = run("chain", _tridiag(3000), prec, seed=6)
    assert (a["plan"].info["levels"], a["plan"].info["launches"]) == (3000, 1)


@gpu
@pytest.mark.parametrize("unit", [True, False], ids=["unit_plan", "non_unit_plan"])
@pytest.mark.parametrize("prec", PRECS)
def test_five_point_grid_in_and_out_of_place(prec, unit):
    rowlists = _grid5(40)
    a = run("grid", rowlists, prec, seed=7, unit=unit)
    b = run("grid", rowlists, prec, seed=7, unit=unit, in_place=True)
    assert torch.equal(SV._raw(a["d_lu"]), SV._raw(b["d_lu"])) and a["G"] == 8


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_narrow_wide_transitions(prec):
    """L + L^T + I of a layered L: narrow -> wide -> narrow, a level one row past W, order[] != identity"""
    W = SV._W()
    rowlists = _layered_sym(W)
    a = run("layered", rowlists, prec, seed=8)
    plan = a["plan"]
    sizes = np.diff(plan.level_offsets.cpu().numpy()).tolist()
    assert sizes == [6, W + 1, 3, 2 * W + 5, W, 1] and plan.info["launches"] == 5
    assert not torch.equal(plan.order.cpu(), torch.arange(len(rowlists), dtype=torch.int32))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_dense_block(prec):
    """every update hits, rows longer than a wave, G = 64"""
    a = run("dense", _dense(70), prec, seed=9)
    assert a["G"] == 64


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_one_long_row_among_short_ones(prec):
    a = run("long_row", _long_row(), prec, seed=10)
    assert a["G"] < 64


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_arrays_off_16_byte_alignment(prec):
    run("shifted", _grid5(13), prec, seed=11, shift=4)
    run("shifted", _grid5(13), prec, seed=11, shift=4, in_place=True)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_unsorted_input_stays_inside_the_arrays(prec):
    """rows in random order with repeated columns: the values are unspecified, but the call ends, the guard words around the factor
    are intact and the pattern and the values passed in are unchanged"""
    rng = np.random.default_rng(19)
    n = 400
    rowlists = [[int(c) for c in rng.integers(0, n, int(rng.integers(0, 12)))] for _ in range(n)]
    off, col = SV._csr(rowlists)
    val = _values(off, col, rng, NP[prec])
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off, col, val))
    lbuf, d_lu = _guarded(len(col), TORCH[prec])
    plan = M.CsrSv(d_off, d_col, lower=True, unit_diagonal=True)
    lu, pivot = M.csrilu0(d_val, d_off, d_col, plan=plan, out=d_lu)
    torch.cuda.synchronize()
    assert _guards_intact(lbuf, d_lu) and -1 <= int(pivot.item()) < n
    assert torch.equal(d_off.cpu(), torch.from_numpy(off)) and torch.equal(d_col.cpu(), torch.from_numpy(col))
    assert torch.equal(SV._raw(d_val).cpu(), torch.from_numpy(SV._bits(val)))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_pivots(prec):
    dtype = NP[prec]
    a = run("p1", [[0, 1], [0, 1]], prec, val=np.ones(4, dtype), finite=False)
    assert a["pivot"] == 1
    # a missing diagonal in row 3 and a numeric zero in row 5 (rows 4, 5 are [[1, 1], [1, 1]]); nothing depends on either
    rowlists = [[0], [0, 1], [1, 2], [2], [4, 5], [4, 5], [6], [6, 7]]
    val = np.asarray([4, 1, 4, 1, 4, 1, 1, 1, 1, 1, 4, 1, 4], dtype)
    a = run("p2", rowlists, prec, val=val, finite=False)
    assert a["pivot"] == 3 and a["want"][9] == 0
    # a division by a zero pivot whose row has no upper entries: the quotient alone is affected, +-inf on the model's bits
    for name, zero, sign in (("p3", 0.0, -1), ("p3n", -0.0, 1)):
        a = run(name, [[0], [0, 1]], prec, val=np.asarray([zero, -2, 3], dtype), finite=False)
        assert a["pivot"] == 0 and np.isinf(a["want"][1]) and np.sign(a["want"][1]) == sign and a["want"][2] == 3
    # d_pivot == NULL is accepted
    a = run("shifted", _grid5(13), prec, seed=11)
    temp = torch.empty(M._ilu0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    a["d_lu"].fill_(SENTINEL)
    M._ilu0_call(a["plan"], temp, a["d_val"], a["d_lu"], a["d_off"], a["d_col"], None, None, False)
    torch.cuda.synchronize()
    assert torch.equal(SV._raw(a["d_lu"]).cpu(), torch.from_numpy(SV._bits(a["want"]))) and _guards_intact(a["lbuf"], a["d_lu"])


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_refactorisation_and_repeatability(prec):
    """new values on the same plan and temp storage; two runs give identical bits"""
    a = run("grid", _grid5(40), prec, seed=7)
    temp = torch.empty(M._ilu0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    pivot = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    first = SV._raw(a["d_lu"]).clone()
    for _ in range(2):
        a["d_lu"].fill_(SENTINEL)
        M._ilu0_call(a["plan"], temp, a["d_val"], a["d_lu"], a["d_off"], a["d_col"], pivot, None, False)
        torch.cuda.synchronize()
        assert torch.equal(SV._raw(a["d_lu"]), first) and int(pivot.item()) == -1
    off, col, val2, want2, piv2 = _reference("grid", _grid5(40), prec, 12, val=_values(a["off"], a["col"], np.random.default_rng(12), NP[prec]))
    a["d_val"].copy_(torch.from_numpy(val2))
    M._ilu0_call(a["plan"], temp, a["d_val"], a["d_lu"], a["d_off"], a["d_col"], pivot, None, False)
    torch.cuda.synchronize()
    assert torch.equal(SV._raw(a["d_lu"]).cpu(), torch.from_numpy(SV._bits(want2))) and int(pivot.item()) == piv2 == -1
    assert _guards_intact(a["lbuf"], a["d_lu"])


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ilu0_object_factors_twice_and_solves_exactly(prec):
    """Ilu0.factor on two sets of values; then, no model: an integer tridiagonal L U and an integer x, Ilu0.solve(A x) == x exactly"""
    dtype = NP[prec]
    rowlists = _grid5(13)
    off, col, val, want, _ = _reference("shifted", rowlists, prec, 11)
    d_off, d_col = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda()
    ilu = M.Ilu0(d_off, d_col)
    for seed in (11, 13):
        off, col, val, want, piv = _reference("shifted", rowlists, prec, seed)
        pivot = ilu.factor(torch.from_numpy(val).cuda())
        torch.cuda.synchronize()
        assert pivot is ilu.pivot and int(pivot.item()) == piv == -1
        assert torch.equal(SV._raw(ilu.lu_values).cpu(), torch.from_numpy(SV._bits(want)))
    # U^-1 (L^-1 r) against the model of the solve on the model's factor
    r = np.random.default_rng(14).uniform(-1, 1, len(rowlists)).astype(dtype)
    y = sv_model.solve(off, col, want, r, 1.0, True, True)
    x = sv_model.solve(off, col, want, y, 1.0, False, False)
    got = ilu.solve(torch.from_numpy(r).cuda())
    torch.cuda.synchronize()
    assert torch.equal(SV._raw(got).cpu(), torch.from_numpy(SV._bits(x)))
    ilu.close(); ilu.close()
    with pytest.raises(M.MspmvError):
        ilu.factor(torch.from_numpy(val).cuda())
    n = 500
    off, col = SV._csr(_tridiag(n))
    rng = np.random.default_rng(15)
    A, LU = _integer_lu(n, rng, dtype)
    x = rng.integers(-4, 5, n).astype(dtype)
    b = np.zeros(n, dtype)
    for i in range(n):
        for e in range(off[i], off[i + 1]):
            b[i] += A[e] * x[col[e]]                                # (small integers: exact)
    ilu = M.Ilu0(torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda())
    pivot = ilu.factor(torch.from_numpy(A).cuda())
    out = torch.empty(n, dtype=TORCH[prec], device="cuda")
    got = ilu.solve(torch.from_numpy(b).cuda(), out=out)
    torch.cuda.synchronize()
    assert got is out and int(pivot.item()) == -1
    assert torch.equal(SV._raw(ilu.lu_values).cpu(), torch.from_numpy(SV._bits(LU)))
    assert torch.equal(SV._raw(out).cpu(), torch.from_numpy(SV._bits(x)))
    ilu.close()


@gpu
def test_graph_capture_and_replay():
    """one factorisation of several launches (narrow, wide, narrow) captured, replayed on new values"""
    W = SV._W()
    rowlists = _cases(W)["capture"]
    a = run("capture", rowlists, "f32", seed=16)
    assert a["plan"].info["launches"] == 3
    temp = torch.empty(M._ilu0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    pivot = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    a["d_lu"].fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M._ilu0_call(a["plan"], temp, a["d_val"], a["d_lu"], a["d_off"], a["d_col"], pivot, None, False)
    for seed in (17, 18):
        off, col, val, want, piv = _reference("capture", rowlists, "f32", seed)
        a["d_val"].copy_(torch.from_numpy(val))
        pivot.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(SV._raw(a["d_lu"]).cpu(), torch.from_numpy(SV._bits(want))) and int(pivot.item()) == piv == -1
        assert _guards_intact(a["lbuf"], a["d_lu"])


@gpu
def test_launch_lines_number_the_launches(capfd):
    W = SV._W()
    a = run("layered", _layered_sym(W), "f64", seed=8)
    plan = a["plan"]
    capfd.readouterr()
    lu, pivot = M.csrilu0(a["d_val"], a["d_off"], a["d_col"], plan=plan, out=a["d_lu"], debug_synchronous=True)
    lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
    segments = sv_model.segments(plan.level_offsets.cpu().numpy(), W)
    assert len(lines) == 1 + plan.info["launches"] == 1 + len(segments), lines
    assert lines[0].startswith("mspmv: ilu0_prologue_kernel<<<")
    assert [l.startswith("mspmv: ilu0_narrow_kernel<<<1,") for l in lines[1:]] == [s[2] for s in segments]
    assert all(l.startswith("mspmv: ilu0_narrow_kernel<<<") or l.startswith("mspmv: ilu0_level_kernel<<<") for l in lines[1:])
    assert all(l.endswith(f" {a['G']} lanes per row") for l in lines)
    assert torch.equal(SV._raw(lu).cpu(), torch.from_numpy(SV._bits(a["want"])))
