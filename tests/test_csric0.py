"""IC(0) on the device (include/mspmv.h: mspmv_csric0_*; merge_spmv_amd.csric0 / Ic0): A ~ L L^T on the pattern of A's lower triangle,
along the levels of a LOWER CsrSv plan, with the mirror epilogue that writes L^T into the upper triangle.  CPU: exports, argument
conventions (nothing launched, no device), wrapper refusals, and the numpy model (tests/csric0_model.py) pinned to exact rational
arithmetic rounded per operation, to a hand-written example, to an integer Cholesky factor that must come back exactly, and to the
pivot rule.  GPU: the factor on the BIT PATTERNS against the model (a NaN of the model is a NaN of the device at the same place,
payload and sign not compared), the pivot against the model's, guard words around the factor intact, the pattern arrays and (out of
place) the values unchanged; the roots against numpy's correctly rounded sqrt; a preconditioned conjugate gradient end to end.
Expected values never come from the library."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import csric0_model as model
import csrsv_model as sv_model
import test_csrsv as SV            # noqa: E402 - _mul/_sub/_div, _csr, _bits, _raw, _shifted, _layered, _grid, _create, _W

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csric0_group", "mspmv_csric0_f32", "mspmv_csric0_f64"]
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


def _band(n, half):
    return [[c for c in range(r - half, r + half + 1) if 0 <= c < n] for r in range(n)]


def _grid5(n):
    return _sym(SV._grid(n))


def _layered_sym(W, seed=7):
    """level widths [20 (+ 5 rows that come last), W + 1, 30, 10]: narrow -> wide -> narrow"""
    return _sym(SV._layered([20, W + 1, 30, 10], np.random.default_rng(seed), extra=5))


def _dense(n):
    return [list(range(n)) for _ in range(n)]


def _arrow(n=600):
    """the last row and column full over a tridiagonal"""
    return _sym(_tridiag(n)[: n - 1] + [list(range(n))])


def _cases(W):
    """name -> rowlists of every pattern the GPU tests factorise (the CPU test of the group rule reads their sizes)"""
    return {"none": [], "one": [[0]], "norow": [[]], "empty": [[] for _ in range(37)], "diagonal": _band(300, 0), "probe": _band(4096, 0),
            "chain": _tridiag(3000), "grid": _grid5(40), "layered": _layered_sym(W), "band7": _band(200, 7), "band15": _band(200, 15),
            "band31": _band(200, 31), "dense": _dense(70), "arrow": _arrow(), "shifted": _grid5(13), "tri50": _tridiag(50),
            "tri500": _tridiag(500), "pcg": _grid5(24)}


GROUPS = {"diagonal": 1, "chain": 2, "grid": 4, "band7": 8, "band15": 16, "band31": 32, "dense": 64}      # the rule, case by case


def _values(off, col, rng, dtype):
    """the issue's recipe: the lower triangle holds the matrix (off-diagonals uniform in [-1, 1], the diagonal 1 + the sum of the
    absolute off-diagonals of the row of the SYMMETRIC matrix: dominant, so no breakdown); the upper triangle holds other numbers
    (7 + uniform), so that "untouched" and "mirrored" both show"""
    rows = len(off) - 1
    r_of = np.repeat(np.arange(rows), np.diff(off))
    val = rng.uniform(-1, 1, len(col))
    low = col < r_of
    s = np.zeros(rows)
    np.add.at(s, r_of[low], np.abs(val[low]))
    np.add.at(s, col[low], np.abs(val[low]))
    val[col == r_of] = 1 + s[r_of[col == r_of]]
    val[col > r_of] = 7 + rng.uniform(0, 1, int((col > r_of).sum()))
    return val.astype(dtype)


def _same(got, want):
    """bit for bit, but a NaN for a NaN whatever its payload and sign"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(SV._bits(got)[~nan], SV._bits(want)[~nan])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csric0_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r" T (mspmv_csric0_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert "csric0" in M.__all__ and "Ic0" in M.__all__ and callable(M.csric0) and callable(M.Ic0) and callable(M.csric0_group)


def _call(lib, fn, handle, temp, size, mirror=0, arrays=(None, None, None, None), pivot=None):
    return getattr(lib, fn)(handle, temp, ctypes.byref(size) if size is not None else None, *arrays, mirror, pivot, None, 0)


def test_csric0_argument_conventions():
    """every refusal comes before anything is launched: this runs without a device"""
    lib = M.load_library()
    for fn in ("mspmv_csric0_f32", "mspmv_csric0_f64"):
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
            for mirror in (0, 1):
                size = ctypes.c_size_t(12345)
                assert _call(lib, fn, lower, None, size, mirror) == 0 and size.value == 16      # the size query: every pointer NULL
            need = size.value
            temp = ctypes.c_void_p(4096)
            for mirror in (0, 1):
                assert _call(lib, fn, lower, temp, ctypes.c_size_t(need), mirror) == 0          # rows == 0: succeeds, launches nothing
            for mirror in (2, -1, 7):
                assert _call(lib, fn, lower, None, ctypes.c_size_t(0), mirror) == 1             # mirror not in {0, 1}
                assert _call(lib, fn, lower, temp, ctypes.c_size_t(need), mirror) == 1
            assert _call(lib, fn, lower, temp, ctypes.c_size_t(need - 1)) == 1        # one byte too small
            for bad in (4097, 4100, 4104):
                assert _call(lib, fn, lower, ctypes.c_void_p(bad), ctypes.c_size_t(need + 64)) == 1   # misaligned
            assert lib.mspmv_csrsv_plan_destroy(lower) == 0
    g = ctypes.c_int32(0)
    assert lib.mspmv_csric0_group(-1, 0, ctypes.byref(g)) == 1 and lib.mspmv_csric0_group(5, -1, ctypes.byref(g)) == 1
    assert lib.mspmv_csric0_group(5, 5, None) == 1
    for rows, nnz in ((0, 0), (1, 0), (1, 1), (7, 7), (1000, 2998), (1600, 7840), (10, 330), (70, 4900), (3, 2 ** 31 - 70000), (2 ** 31 - 70000, 3)):
        assert lib.mspmv_csric0_group(rows, nnz, ctypes.byref(g)) == 0
        assert 1 <= g.value <= 64 and g.value & (g.value - 1) == 0 and g.value == model.group(rows, nnz), (rows, nnz, g.value)


def test_the_group_of_every_gpu_case():
    """csric0_group is the model's rule on every pattern the GPU tests factorise, and takes each of 1, 2, 4, ..., 64 among them"""
    cases = _cases(SV._W())
    got = {}
    for name, rows in cases.items():
        got[name] = M.csric0_group(len(rows), sum(len(r) for r in rows))
        assert got[name] == model.group(len(rows), sum(len(r) for r in rows)), name
    assert {name: got[name] for name in GROUPS} == GROUPS
    assert got["arrow"] < 64


def test_csric0_wrapper_rejects_bad_tensors_without_a_device():
    off, col, val = torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    with pytest.raises(M.MspmvError):
        M.csric0(val, off, col)                                    # not on the device
    with pytest.raises(M.MspmvError):
        M.csric0(val, off, col, mirror=True)
    with pytest.raises(M.MspmvError):
        M.csric0(None, off, col)
    with pytest.raises(M.MspmvError):
        M.csric0(val, off, [0, 1])
    with pytest.raises(M.MspmvError):
        M.Ic0(off, col)
    with pytest.raises(M.MspmvError):
        M.Ic0(off, None)


def _rounded(off, col, val, dtype, mirror):
    """the definition of include/mspmv.h once more, every divide, multiply and subtract computed exactly in rationals and rounded once
    to the type; the root as math.sqrt of the value as a double, then rounded to the type (fp32: 53 >= 2 * 24 + 2, so the double
    rounding is harmless)"""
    rows = len(off) - 1
    a = list(val)
    where = [{int(col[e]): e for e in range(off[r], off[r + 1])} for r in range(rows)]
    for i in range(rows):
        for e in range(off[i], off[i + 1]):
            j = int(col[e])
            if j >= i:
                continue
            a[e] = SV._div(a[e], a[where[j][j]] if j in where[j] else dtype(0.0), dtype)
            for g in range(e + 1, off[i + 1]):
                k = int(col[g])
                if k == i:
                    a[g] = SV._sub(a[g], SV._mul(a[e], a[e], dtype), dtype)
                elif k < i and j in where[k]:
                    a[g] = SV._sub(a[g], SV._mul(a[e], a[where[k][j]], dtype), dtype)
        if i in where[i]:
            a[where[i][i]] = dtype(math.sqrt(float(a[where[i][i]])))
    if mirror:
        for i in range(rows):
            for g in range(off[i], off[i + 1]):
                j = int(col[g])
                if j > i:
                    a[g] = a[where[j][i]] if i in where[j] else dtype(0.0)
    return np.asarray(a, dtype)


FOUR = [[0, 1, 2, 3], [0, 1, 2], [0, 1, 2, 3], [0, 2, 3]]
FOUR_A = [4, 70, 71, 72, 2, 5, 73, 4, 4, 9, 74, 2, 6, 14]
FOUR_L = [2, 70, 71, 72, 1, 2, 73, 2, 1, 2, 74, 1, 2, 3]
FOUR_LLT = [2, 1, 2, 1, 1, 2, 1, 2, 1, 2, 2, 1, 2, 3]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_a_hand_written_example(dtype):
    """    A = [4  .  .  . ]   row 0: l00 = sqrt 4 = 2
        [2  5  .    ]   row 1: l10 = 2/2 = 1; 5 - 1*1 = 4, l11 = 2
        [4  4  9  . ]   row 2: l20 = 4/2 = 2; (2,1): 4 - l20*l10 = 2; 9 - 2*2 = 5; l21 = 2/2 = 1; 5 - 1*1 = 4, l22 = 2
        [2     6  14]   row 3: l30 = 2/2 = 1; (3,2): 6 - l30*l20 = 4; 14 - 1*1 = 13; l32 = 4/2 = 2; 13 - 2*2 = 9, l33 = 3
    ((3,1) is not stored: l30*l10 is dropped; the upper triangle holds 70..74), every step exact; then general mantissas against
    exact rationals rounded per operation"""
    off, col = SV._csr(FOUR)
    for mirror, want in ((False, FOUR_L), (True, FOUR_LLT)):
        l, pivot = model.ic0(off, col, np.asarray(FOUR_A, dtype), mirror)
        assert l.dtype == dtype and pivot == -1 and l.tolist() == want
    rng = np.random.default_rng(1)
    for _ in range(5):
        val = _values(off, col, rng, dtype)
        for mirror in (False, True):
            l, pivot = model.ic0(off, col, val, mirror)
            assert pivot == -1 and np.isfinite(l).all() and np.array_equal(SV._bits(l), SV._bits(_rounded(off, col, val, dtype, mirror)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_a_small_grid(dtype):
    off, col = SV._csr(_grid5(6))
    val = _values(off, col, np.random.default_rng(2), dtype)
    for mirror in (False, True):
        l, pivot = model.ic0(off, col, val, mirror)
        assert pivot == -1 and np.isfinite(l).all()
        assert np.array_equal(SV._bits(l), SV._bits(_rounded(off, col, val, dtype, mirror)))
    r_of = np.repeat(np.arange(36), np.diff(off))
    assert np.array_equal(l[col <= r_of], model.ic0(off, col, val, False)[0][col <= r_of])
    assert np.array_equal(model.ic0(off, col, val, False)[0][col > r_of], val[col > r_of])       # unchanged without the mirror


def _integer_cholesky(n, rng, dtype, dense=True, pow2=False):
    """(rowlists, values of A = L L^T in the full symmetric layout with the upper triangle replaced by 99, L in that layout, L\\L^T in
    that layout) for an integer lower triangular L (dense or bidiagonal) with a positive integer diagonal: every operation is exact"""
    L = np.zeros((n, n))
    for i in range(n):
        for j in (range(i) if dense else range(max(i - 1, 0), i)):
            L[i, j] = rng.integers(-3, 4) or 1
        L[i, i] = 2.0 ** rng.integers(0, 3) if pow2 else rng.integers(1, 5)
    A = L @ L.T
    rowlists = _dense(n) if dense else _tridiag(n)
    a, l, llt = [], [], []
    for i, row in enumerate(rowlists):
        for j in row:
            a.append(A[i, j] if j <= i else 99.0)
            l.append(L[i, j] if j <= i else 99.0)
            llt.append(L[i, j] if j <= i else L[j, i])
    return rowlists, np.asarray(a, dtype), np.asarray(l, dtype), np.asarray(llt, dtype), A, L


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_integer_factor_comes_back_exactly(dtype):
    """no fill in a dense triangle: IC(0) is Cholesky, and on integers every operation is exact"""
    rowlists, a, l, llt, _, _ = _integer_cholesky(8, np.random.default_rng(4), dtype)
    off, col = SV._csr(rowlists)
    for mirror, want in ((False, l), (True, llt)):
        got, pivot = model.ic0(off, col, a, mirror)
        assert pivot == -1 and np.array_equal(SV._bits(got), SV._bits(want))


def _bad_tridiagonal(dtype, n=50, missing=(), negative=()):
    """(rowlists, values): a dominant tridiagonal of n rows without the diagonals of `missing`, the diagonals of `negative` set to -1"""
    rowlists = [[c for c in row if not (c == r and r in missing)] for r, row in enumerate(_tridiag(n))]
    off, col = SV._csr(rowlists)
    val = _values(off, col, np.random.default_rng(20), dtype)
    for r in negative:
        val[off[r] + rowlists[r].index(r)] = -1.0
    return rowlists, val


PIVOT_CASES = {"first_missing": (dict(missing=(0,)), 0), "last_missing": (dict(missing=(49,)), 49), "negative": (dict(negative=(10,)), 10),
               "negative_then_missing": (dict(negative=(10,), missing=(30,)), 10), "missing_then_negative": (dict(missing=(5,), negative=(10,)), 5)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_names_the_pivot(dtype):
    for name, (kw, row) in PIVOT_CASES.items():
        rowlists, val = _bad_tridiagonal(dtype, **kw)
        off, col = SV._csr(rowlists)
        l, pivot = model.ic0(off, col, val)
        assert pivot == row, name
        if name in ("negative", "negative_then_missing"):
            d = off[10] + rowlists[10].index(10)
            assert np.isnan(l[d]) and np.isnan(l[off[11]]) and np.isfinite(l[:d]).all(), name     # NaN from row 10 on
    off, col = SV._csr([[0], [1], [2]])
    for v, want, piv in (([4, -0.0, 9], [2, -0.0, 3], 1), ([4, 0.0, -0.0], [2, 0.0, -0.0], 1), ([1, 4, 9], [1, 2, 3], -1)):
        l, pivot = model.ic0(off, col, np.asarray(v, dtype))
        assert pivot == piv and np.array_equal(SV._bits(l), SV._bits(np.asarray(want, dtype)))
    l, pivot = model.ic0(*SV._csr([[0], [1]]), np.asarray([float("nan"), 4], dtype))
    assert pivot == -1 and np.isnan(l[0]) and l[1] == 2                               # a NaN is not <= 0


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 8
SENTINEL = 12345.0
_MODEL = {}                     # (name, prec, seed) -> (off, col, val, mirrored factor, pivot): computed once, shared, never changed


def _reference(name, rowlists, prec, seed, val=None):
    key = (name, prec, seed)
    if key not in _MODEL:
        off, col = SV._csr(rowlists)
        if val is None:
            val = _values(off, col, np.random.default_rng(seed), NP[prec])
        want, pivot = model.ic0(off, col, val, True)
        _MODEL[key] = (off, col, val, want, pivot)
    return _MODEL[key]


def _unmirrored(off, col, val, mirrored):
    """the factor without the mirror, from the one with it: the entries behind the diagonal are A's (the model's own statement, which
    test_the_model_on_a_small_grid checks)"""
    r_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return np.where(col > r_of, val, mirrored)


def _guarded(n, tdt, shift_elems=0):
    buf = torch.full((GUARD + shift_elems + n + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    return buf, buf[GUARD + shift_elems: GUARD + shift_elems + n]


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


def run(name, rowlists, prec, seed=0, val=None, shift=0, in_place=False, unit=False, mirror=False, finite=True):
    """One LOWER plan and one factorisation through M.csric0 on guarded, possibly misaligned arrays: the factor bit for bit against
    the model, the pivot against the model's, the inputs unchanged.  Returns a dict for further calls."""
    tdt = TORCH[prec]
    off, col, val, mirrored, want_pivot = _reference(name, rowlists, prec, seed, val)
    want = mirrored if mirror else _unmirrored(off, col, val, mirrored)
    if finite:
        assert np.isfinite(mirrored).all() and want_pivot == -1
    nnz = len(col)
    obuf, d_off = SV._shifted(off, shift)
    cbuf, d_col = SV._shifted(col, shift)
    vshift = (shift // val.itemsize or 1) if shift else 0                            # (whole elements: fp64 moves by 8 bytes)
    vbuf, d_val = _guarded(nnz, tdt, vshift)
    d_val.copy_(torch.from_numpy(val))
    lbuf, d_l = (vbuf, d_val) if in_place else _guarded(nnz, tdt, vshift)
    if shift:
        assert d_off.data_ptr() % 16 == shift and d_col.data_ptr() % 16 == shift and d_val.data_ptr() % 16 != 0 and d_l.data_ptr() % 16 != 0
    plan = M.CsrSv(d_off, d_col, lower=True, unit_diagonal=unit)
    keep = [SV._raw(t).clone() for t in (obuf, cbuf, vbuf)]
    l, pivot = M.csric0(d_val, d_off, d_col, plan=plan, out=d_l, mirror=mirror)
    torch.cuda.synchronize()
    assert l is d_l and pivot.dtype == torch.int32 and pivot.is_cuda and pivot.numel() == 1
    assert _same(d_l.cpu().numpy(), want), (name, prec, mirror)
    assert int(pivot.item()) == want_pivot
    assert _guards_intact(lbuf, d_l), "guard words written"
    for t, was in zip((obuf, cbuf) if in_place else (obuf, cbuf, vbuf), keep):
        assert torch.equal(SV._raw(t), was), "an input was modified"
    return dict(plan=plan, off=off, col=col, val=val, want=want, mirrored=mirrored, pivot=want_pivot, d_off=d_off, d_col=d_col, d_val=d_val,
                d_l=d_l, lbuf=lbuf, keep=(obuf, cbuf, vbuf), G=M.csric0_group(len(rowlists), nnz))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_sizes(prec):
    dtype = NP[prec]
    cases = _cases(1)
    for mirror in (False, True):
        a = run("none", cases["none"], prec, mirror=mirror)
        assert a["plan"].info["launches"] == 0
        a = run("norow", cases["norow"], prec, mirror=mirror, finite=False)          # one row, no entry
        assert a["pivot"] == 0
        a = run("four", cases["one"], prec, val=np.asarray([4], dtype), mirror=mirror)
        assert a["G"] == 1 and a["want"].tolist() == [2]
        a = run("minus", cases["one"], prec, val=np.asarray([-1], dtype), mirror=mirror, finite=False)
        assert a["pivot"] == 0 and np.isnan(a["want"][0])
        a = run("empty", cases["empty"], prec, mirror=mirror, finite=False)
        assert a["pivot"] == 0
        a = run("diagonal", cases["diagonal"], prec, seed=5, mirror=mirror)
        assert a["G"] == 1


def _probe_values(dtype):
    """positive numbers of every kind, in chunks of 4096 rows: the first chunk begins with -0.0, +0.0 and a negative number, the second
    with +0.0, so that each kind of zero is once the smallest row that is reported"""
    f32 = dtype == np.float32
    bits, frac, top = (np.uint32, 23, 0x7F800000) if f32 else (np.uint64, 52, 0x7FF0000000000000)
    rng = np.random.default_rng(21)
    one = np.asarray([1 << frac], bits)[0]
    powers = (np.arange(1, 255 if f32 else 2047, dtype=bits) * one)                  # every normal power of two
    squares = (rng.integers(1, 4000, 300).astype(np.float64) ** 2).astype(dtype).view(bits)
    parts = [np.asarray([-0.0, 0.0, -2.5], dtype).view(bits),
             np.asarray([top - 1, 1, 2, 3, one - 1, one, one + 1], bits),                # the largest finite value, the edges of the subnormals
             powers, powers - bits(1), powers + bits(1), squares, squares - bits(1), squares + bits(1),
             rng.integers(1, int(one), 300).astype(bits)]                               # subnormals
    have = sum(len(p) for p in parts) + 1
    parts.append(rng.integers(1, top, -have % 4096 + 4096).astype(bits))                # bit patterns over the whole positive range
    v = np.insert(np.concatenate(parts), 4096, bits(0)).view(dtype)
    assert len(v) % 4096 == 0 and not np.isnan(v).any() and np.isfinite(v).all()
    return v.reshape(-1, 4096)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_root_probe(prec):
    """a diagonal matrix is a[d] = sqrt(a[d]) and nothing else: the device's roots against numpy's (the host's correctly rounded
    instruction), subnormals, the neighbours of every power of two and of perfect squares included"""
    rowlists = _cases(1)["probe"]
    for chunk, val in enumerate(_probe_values(NP[prec])):
        with np.errstate(invalid="ignore"):
            want = np.sqrt(val)
        off, col, _, mirrored, pivot = _reference(f"probe{chunk}", rowlists, prec, 0, val=val.copy())
        assert _same(mirrored, want) and pivot == (0 if chunk < 2 else -1)              # the model's roots are numpy's
        if chunk == 0:
            assert np.isnan(want[2]) and SV._bits(want[:2]).tolist() == SV._bits(val[:2]).tolist() and np.signbit(val[0])
        if chunk == 1:
            assert SV._bits(val[:1]).tolist() == [0] and (val[1:] > 0).all()
        a = run(f"probe{chunk}", rowlists, prec, finite=False)
        got = a["d_l"].cpu().numpy()
        bad = np.flatnonzero(~(np.isnan(want) | (SV._bits(got) == SV._bits(want))))
        assert bad.size == 0, [(float(val[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_tridiagonal_chain(prec):
    """one narrow launch of more levels than one LDS chunk of level offsets holds"""
    a = run("chain", _tridiag(3000), prec, seed=6, mirror=True)
    assert (a["plan"].info["levels"], a["plan"].info["launches"]) == (3000, 1) and a["G"] == 2


@gpu
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit_plan", "non_unit_plan"])
@pytest.mark.parametrize("prec", PRECS)
def test_five_point_grid_in_and_out_of_place(prec, unit, mirror):
    rowlists = _grid5(40)
    a = run("grid", rowlists, prec, seed=7, unit=unit, mirror=mirror)
    b = run("grid", rowlists, prec, seed=7, unit=unit, mirror=mirror, in_place=True)
    assert torch.equal(SV._raw(a["d_l"]), SV._raw(b["d_l"])) and a["G"] == 4


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_narrow_wide_transitions(prec):
    """L + L^T + I of a layered L: narrow -> wide -> narrow, a level one row past W, order[] != identity"""
    W = SV._W()
    rowlists = _layered_sym(W)
    a = run("layered", rowlists, prec, seed=8, mirror=True)
    plan = a["plan"]
    sizes = np.diff(plan.level_offsets.cpu().numpy()).tolist()
    assert sizes == [25, W + 1, 30, 10] and plan.info["launches"] == 3
    assert not torch.equal(plan.order.cpu(), torch.arange(len(rowlists), dtype=torch.int32))


@gpu
@pytest.mark.parametrize("name", ["band7", "band15", "band31", "dense"])
@pytest.mark.parametrize("prec", PRECS)
def test_every_wider_group(prec, name):
    """G = 8, 16, 32 and 64 (1, 2 and 4: the diagonal, the chain and the grid above); the dense block: rows longer than a wave, every
    update hits"""
    a = run(name, _cases(1)[name], prec, seed=9, mirror=True)
    assert a["G"] == GROUPS[name]


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_one_long_row_among_short_ones(prec):
    """the arrow's last row: 600 / G entries per lane, 599 updates of the diagonal"""
    a = run("arrow", _arrow(), prec, seed=10, mirror=True)
    assert a["G"] < 64


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_arrays_off_16_byte_alignment(prec):
    for mirror in (False, True):
        run("shifted", _grid5(13), prec, seed=11, shift=4, mirror=mirror)
        run("shifted", _grid5(13), prec, seed=11, shift=4, mirror=mirror, in_place=True)


@gpu
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("prec", PRECS)
def test_unsorted_input_stays_inside_the_arrays(prec, mirror):
    """rows in random order with repeated columns: the values are unspecified, but the call ends, the guard words around the factor
    are intact and the pattern and the values passed in are unchanged"""
    rng = np.random.default_rng(19)
    n = 400
    rowlists = [[int(c) for c in rng.integers(0, n, int(rng.integers(0, 12)))] for _ in range(n)]
    off, col = SV._csr(rowlists)
    val = rng.uniform(1, 2, len(col)).astype(NP[prec])
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off, col, val))
    lbuf, d_l = _guarded(len(col), TORCH[prec])
    plan = M.CsrSv(d_off, d_col, lower=True, unit_diagonal=True)
    l, pivot = M.csric0(d_val, d_off, d_col, plan=plan, out=d_l, mirror=mirror)
    torch.cuda.synchronize()
    assert _guards_intact(lbuf, d_l) and -1 <= int(pivot.item()) < n
    assert torch.equal(d_off.cpu(), torch.from_numpy(off)) and torch.equal(d_col.cpu(), torch.from_numpy(col))
    assert torch.equal(SV._raw(d_val).cpu(), torch.from_numpy(SV._bits(val)))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_pivots(prec):
    dtype = NP[prec]
    for name, (kw, row) in PIVOT_CASES.items():
        rowlists, val = _bad_tridiagonal(dtype, **kw)
        a = run(name, rowlists, prec, val=val, mirror=name == "negative", finite=False)
        assert a["pivot"] == row, name
    assert np.isnan(_MODEL[("negative", prec, 0)][3]).sum() > 80                      # NaN from row 10 on, compared place by place
    # d_pivot == NULL is accepted
    a = run("shifted", _grid5(13), prec, seed=11, mirror=True)
    temp = torch.empty(M._ic0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    a["d_l"].fill_(SENTINEL)
    M._ic0_call(a["plan"], temp, a["d_val"], a["d_l"], a["d_off"], a["d_col"], True, None, None, False)
    torch.cuda.synchronize()
    assert _same(a["d_l"].cpu().numpy(), a["want"]) and _guards_intact(a["lbuf"], a["d_l"])


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_refactorisation_and_repeatability(prec):
    """three sets of values on one plan and one temp storage; the same call twice gives identical bits"""
    rowlists = _grid5(40)
    a = run("grid", rowlists, prec, seed=7, mirror=True)
    temp = torch.empty(M._ic0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    pivot = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    first = SV._raw(a["d_l"]).clone()
    for _ in range(2):
        a["d_l"].fill_(SENTINEL)
        M._ic0_call(a["plan"], temp, a["d_val"], a["d_l"], a["d_off"], a["d_col"], True, pivot, None, False)
        torch.cuda.synchronize()
        assert torch.equal(SV._raw(a["d_l"]), first) and int(pivot.item()) == -1
    for seed in (12, 13):
        off, col, val2, want2, piv2 = _reference("grid", rowlists, prec, seed)
        a["d_val"].copy_(torch.from_numpy(val2))
        pivot.fill_(77)
        M._ic0_call(a["plan"], temp, a["d_val"], a["d_l"], a["d_off"], a["d_col"], True, pivot, None, False)
        torch.cuda.synchronize()
        assert _same(a["d_l"].cpu().numpy(), want2) and int(pivot.item()) == piv2 == -1
    assert _guards_intact(a["lbuf"], a["d_l"])


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ic0_object_factors_twice_and_solves_exactly(prec):
    """Ic0.factor on two sets of values; solve against the model of the two sweeps on the model's mirrored factor; then, no model: an
    integer bidiagonal L with powers of two on its diagonal and an integer x, Ic0.solve(A x) == x exactly"""
    dtype = NP[prec]
    rowlists = _grid5(13)
    off, col = SV._csr(rowlists)
    d_off, d_col = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda()
    ic = M.Ic0(d_off, d_col)
    for seed in (11, 14):
        off, col, val, want, piv = _reference("shifted", rowlists, prec, seed)
        pivot = ic.factor(torch.from_numpy(val).cuda())
        torch.cuda.synchronize()
        assert pivot is ic.pivot and int(pivot.item()) == piv == -1
        assert _same(ic.l_values.cpu().numpy(), want)
    # L^-T (L^-1 r) against the model of the solve on the model's factor
    r = np.random.default_rng(15).uniform(-1, 1, len(rowlists)).astype(dtype)
    y = sv_model.solve(off, col, want, r, 1.0, True, False)
    x = sv_model.solve(off, col, want, y, 1.0, False, False)
    got = ic.solve(torch.from_numpy(r).cuda())
    torch.cuda.synchronize()
    assert torch.equal(SV._raw(got).cpu(), torch.from_numpy(SV._bits(x)))
    ic.close(); ic.close()
    with pytest.raises(M.MspmvError):
        ic.factor(torch.from_numpy(val).cuda())
    n = 500
    rng = np.random.default_rng(16)
    rowlists, a, l, llt, A, L = _integer_cholesky(n, rng, dtype, dense=False, pow2=True)
    off, col = SV._csr(rowlists)
    x = rng.integers(-4, 5, n).astype(np.float64)
    b = (A @ x).astype(dtype)                                       # (small integers: exact)
    ic = M.Ic0(torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda())
    pivot = ic.factor(torch.from_numpy(a).cuda())
    out = torch.empty(n, dtype=TORCH[prec], device="cuda")
    got = ic.solve(torch.from_numpy(b).cuda(), out=out)
    torch.cuda.synchronize()
    assert got is out and int(pivot.item()) == -1
    assert torch.equal(SV._raw(ic.l_values).cpu(), torch.from_numpy(SV._bits(llt)))
    assert torch.equal(SV._raw(out).cpu(), torch.from_numpy(SV._bits(x.astype(dtype))))
    ic.close()
    # a pattern without a diagonal: factor reports the row, the NON_UNIT plan's refusal of the solve comes through as it is
    rowlists, val = _bad_tridiagonal(dtype, missing=(5,))
    off, col = SV._csr(rowlists)
    ic = M.Ic0(torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda())
    assert int(ic.factor(torch.from_numpy(val).cuda()).item()) == 5
    with pytest.raises(M.MspmvError, match="CsrSv.solve: row 5 "):
        ic.solve(torch.zeros(50, dtype=TORCH[prec], device="cuda"))
    ic.close()


@gpu
def test_graph_capture_and_replay():
    """one mirrored factorisation of several launches (narrow, wide, narrow, the mirror) captured, replayed on new values"""
    W = SV._W()
    rowlists = _layered_sym(W)
    a = run("layered", rowlists, "f32", seed=8, mirror=True)
    assert a["plan"].info["launches"] == 3
    temp = torch.empty(M._ic0_temp_bytes(a["plan"]), dtype=torch.uint8, device="cuda")
    pivot = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    a["d_l"].fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M._ic0_call(a["plan"], temp, a["d_val"], a["d_l"], a["d_off"], a["d_col"], True, pivot, None, False)
    for seed in (17, 18):
        off, col, val, want, piv = _reference("layered", rowlists, "f32", seed)
        a["d_val"].copy_(torch.from_numpy(val))
        pivot.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a["d_l"].cpu().numpy(), want) and int(pivot.item()) == piv == -1
        assert _guards_intact(a["lbuf"], a["d_l"])


@gpu
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
def test_launch_lines_number_the_launches(capfd, mirror):
    W = SV._W()
    a = run("layered", _layered_sym(W), "f64", seed=8, mirror=mirror)
    plan = a["plan"]
    capfd.readouterr()
    l, pivot = M.csric0(a["d_val"], a["d_off"], a["d_col"], plan=plan, out=a["d_l"], mirror=mirror, debug_synchronous=True)
    lines = [s for s in capfd.readouterr().out.splitlines() if s.startswith("mspmv: ")]
    segments = sv_model.segments(plan.level_offsets.cpu().numpy(), W)
    assert len(lines) == 1 + plan.info["launches"] + mirror == 1 + len(segments) + mirror, lines
    assert lines[0].startswith("mspmv: ic0_prologue_kernel<<<")
    body = lines[1: 1 + len(segments)]
    assert [s.startswith("mspmv: ic0_narrow_kernel<<<1,") for s in body] == [s[2] for s in segments]
    assert all(s.startswith("mspmv: ic0_narrow_kernel<<<") or s.startswith("mspmv: ic0_level_kernel<<<") for s in body)
    assert [s.startswith("mspmv: ic0_mirror_kernel<<<") for s in lines[1 + len(segments):]] == [True] * mirror
    assert all(s.endswith(f" {a['G']} lanes per row") for s in lines)
    assert _same(l.cpu().numpy(), a["want"])


def _pcg(d_val, d_off, d_col, b, precondition, limit=400):
    """conjugate gradients on the device: A p by csrmv, dots and updates in torch; stops when the recurrence residual reaches
    1e-10 |b|.  (x, iterations)"""
    n = b.numel()
    x = torch.zeros_like(b)
    r = b.clone()
    z = precondition(r).clone()
    p = z.clone()
    rz = torch.dot(r, z)
    stop = 1e-10 * float(torch.linalg.norm(b))
    for it in range(1, limit + 1):
        q = M.csrmv(d_val, d_off, d_col, p, num_cols=n)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            return x, it
        z = precondition(r)
        rz_new = torch.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, limit + 1


@gpu
def test_preconditioned_conjugate_gradients_end_to_end():
    """the 5-point Laplacian of a 24 x 24 grid (condition number about 250), fp64: both runs converge, the true residual recomputed on
    the host is <= 1e-8 |b| (100 times the stopping bound: the drift between the recurrence and the true residual is of order 1e-13
    here), and Ic0.solve as the preconditioner takes at most half the plain run's iterations (the numpy model of this loop: 31
    against 87, a property of the matrix)"""
    rowlists = _grid5(24)
    off, col = SV._csr(rowlists)
    n = len(rowlists)
    r_of = np.repeat(np.arange(n), np.diff(off))
    val = np.where(col == r_of, 4.0, -1.0)
    b = np.random.default_rng(22).uniform(-1, 1, n)
    d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
    ic = M.Ic0(d_off, d_col)
    assert int(ic.factor(d_val).item()) == -1
    x_ic, it_ic = _pcg(d_val, d_off, d_col, d_b, ic.solve)
    x_cg, it_cg = _pcg(d_val, d_off, d_col, d_b, lambda r: r)
    torch.cuda.synchronize()
    ic.close()
    print(f"pcg: {it_ic} iterations with IC(0), {it_cg} without")
    assert it_ic <= 400 and it_cg <= 400
    for x in (x_ic, x_cg):
        ax = np.zeros(n)
        np.add.at(ax, r_of, val * x.cpu().numpy()[col])
        res = float(np.linalg.norm(b - ax))
        print(f"pcg: true residual {res:.3e}, |b| {np.linalg.norm(b):.3e}")
        assert res <= 1e-8 * float(np.linalg.norm(b))
    assert 2 * it_ic <= it_cg, (it_ic, it_cg)
