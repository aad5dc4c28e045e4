"""The level-scheduled sparse triangular solve for k right-hand sides (include/mspmv.h: mspmv_csrsm_*; merge_spmv_amd.CsrSv.solve_many /
many_info / csrsm; Ilu0.solve_many, Ic0.solve_many): op(A) X = alpha * B, B and X rows x k row-major.
CPU: exports, argument conventions (nothing launched, no device), mspmv_csrsm_info on a plan of no rows, wrapper refusals, and the
model's segments at the budget boundary.  GPU: X by torch.equal on the BIT PATTERNS against the numpy model (tests/csrsm_model.py:
tests/csrsv_model.py column by column); the guard words around X and the sentinel in X's padding columns stay untouched, the inputs
stay unchanged, and many_info(k)["launches"] equals the model's count.  Expected values never come from the library.
Measured on MI355X: the 145 GPU tests of this file take 5 s."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import csrsv_model as sv_model
import csrsm_model as model

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csrsm_info", "mspmv_csrsm_solve_f32", "mspmv_csrsm_solve_f64"]
NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}
SOLVE = {"f32": ("mspmv_csrsm_solve_f32", ctypes.c_float), "f64": ("mspmv_csrsm_solve_f64", ctypes.c_double)}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csrsm_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r" T (mspmv_csrsm_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert re.search(r"\}\s*mspmv_csrsm_info_t\s*;", text)
    assert "csrsm" in M.__all__ and callable(M.csrsm)
    for cls in (M.CsrSv, M.Ilu0, M.Ic0):
        assert callable(cls.solve_many)
    assert callable(M.CsrSv.many_info)
    assert lib.mspmv_version() == 102


def _empty_plan(uplo=0, diag=0):
    handle = ctypes.c_void_p(0)
    assert M.load_library().mspmv_csrsv_plan_create(ctypes.byref(handle), None, None, 0, 0, uplo, diag, None, 0) == 0 and handle.value
    return handle


def test_csrsm_argument_conventions():
    """every refusal comes before anything is launched: this runs on a plan of no rows and fake pointers, without a device"""
    lib = M.load_library()
    f = ctypes.c_void_p(4096)
    info = M._CsrSmInfo()
    assert lib.mspmv_csrsm_info(None, 1, ctypes.byref(info)) == 1
    for prec, (name, ct) in SOLVE.items():
        fn = getattr(lib, name)
        assert fn(None, f, f, f, ct(1.0), f, 4, f, 4, 4, None, 0) == 1                    # a NULL plan
        for uplo in (0, 1):
            for diag in (0, 1):
                plan = _empty_plan(uplo, diag)
                assert lib.mspmv_csrsm_info(plan, 0, ctypes.byref(info)) == 1 and lib.mspmv_csrsm_info(plan, -3, ctypes.byref(info)) == 1
                assert lib.mspmv_csrsm_info(plan, 4, None) == 1
                for k in (0, -1):
                    assert fn(plan, f, f, f, ct(1.0), f, 4, f, 4, k, None, 0) == 1        # k < 1
                assert fn(plan, f, f, f, ct(1.0), f, 3, f, 4, 4, None, 0) == 1            # ldb < k
                assert fn(plan, f, f, f, ct(1.0), f, 4, f, 3, 4, None, 0) == 1            # ldx < k
                assert fn(plan, f, f, f, ct(1.0), f, 0, f, 0, 1, None, 0) == 1
                # rows == 0 succeeds and touches nothing: fake pointers and NULL ones alike
                assert fn(plan, f, f, f, ct(1.0), f, 4, f, 4, 4, None, 0) == 0
                assert fn(plan, None, None, None, ct(1.0), None, 7, None, 5, 3, None, 0) == 0
                assert fn(plan, None, None, None, ct(1.0), None, 130, None, 130, 130, None, 1) == 0
                assert lib.mspmv_csrsv_plan_destroy(plan) == 0


def test_csrsm_info_on_a_plan_of_no_rows():
    lib = M.load_library()
    plan = _empty_plan()
    info = M._CsrSmInfo()
    for k, P, passes in ((1, 1, 1), (2, 2, 1), (3, 4, 1), (64, 64, 1), (65, 64, 2), (130, 64, 3)):
        assert lib.mspmv_csrsm_info(plan, k, ctypes.byref(info)) == 0
        assert (info.k, info.lanes_per_row, info.passes, info.launches) == (k, P, passes, 0)
        assert info.narrow_lanes == 256
        assert (model.lanes_per_row(k), model.passes(k)) == (P, passes)
    for k in range(1, 200):
        assert lib.mspmv_csrsm_info(plan, k, ctypes.byref(info)) == 0
        assert (info.lanes_per_row, info.passes) == (model.lanes_per_row(k), model.passes(k))
    assert lib.mspmv_csrsv_plan_destroy(plan) == 0


def test_csrsm_wrapper_rejects_bad_tensors_without_a_device():
    off, col, val = torch.zeros(5, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    with pytest.raises(M.MspmvError, match="2-D"):
        M.csrsm(val, off, col, torch.zeros(4))                                            # 1-D B
    with pytest.raises(M.MspmvError, match="2-D"):
        M.csrsm(val, off, col, torch.zeros(4, 0))                                         # no right-hand side
    with pytest.raises(M.MspmvError, match="unit stride"):
        M.csrsm(val, off, col, torch.zeros(3, 4).t())                                     # column-major
    with pytest.raises(M.MspmvError, match="unit stride"):
        M.csrsm(val, off, col, torch.zeros(4, 6)[:, ::2])
    with pytest.raises(M.MspmvError, match="leading dimension"):
        M.csrsm(val, off, col, torch.as_strided(torch.zeros(20), (4, 3), (2, 1)))          # stride(0) < k: overlapping rows
    with pytest.raises(M.MspmvError, match="leading dimension"):
        M.csrsm(val, off, col, torch.zeros(1, 3).expand(4, 3))
    with pytest.raises(TypeError):
        M.csrsm(val, off, col, torch.zeros(4, 3, dtype=torch.float64))                    # values fp32, B fp64
    with pytest.raises(TypeError):
        M.csrsm(val.to(torch.float16), off, col, torch.zeros(4, 3, dtype=torch.float16))
    with pytest.raises(M.MspmvError, match="tensor"):
        M.csrsm(val, off, col, None)
    with pytest.raises(M.MspmvError, match="CUDA"):
        M.csrsm(val, off, col, torch.zeros(4, 3))                                         # a good layout, not on the device
    with pytest.raises(M.MspmvError, match="2-D"):
        M._many_layout("x", val, torch.zeros(4, 3), torch.zeros(12))                      # X is held to the same layout
    with pytest.raises(TypeError):
        M._many_layout("x", val, torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64))
    assert M._many_layout("x", val, torch.zeros(4, 6)[:, :3], torch.zeros(4, 3)) == 3


def test_the_model_segments_at_the_budget_boundary():
    """n * P == budget is narrow, n * P == budget + P is wide; with P = 1 and the budget W the segments are csrsv's"""
    lo = np.concatenate([[0], np.cumsum([15, 16, 17, 16, 5, 64, 65, 1])])
    assert model.segments(lo, 256, 16) == [(0, 2, True), (2, 3, False), (3, 5, True), (5, 6, False), (6, 7, False), (7, 8, True)]
    assert model.segments(lo, 256, 4) == [(0, 6, True), (6, 7, False), (7, 8, True)]
    assert model.segments(lo, 256, 64) == [(l, l + 1, False) for l in range(7)] + [(7, 8, True)]                       # 5 * 64 > 256
    assert model.segments(lo, 255, 16)[:2] == [(0, 1, True), (1, 2, False)]
    assert model.segments([0, 4], 256, 64) == [(0, 1, True)] and model.segments([0, 5], 256, 64) == [(0, 1, False)]
    assert model.segments([0], 256, 16) == []
    rng = np.random.default_rng(1)
    for W in (1, 3, 256):
        lo = np.concatenate([[0], np.cumsum(rng.integers(1, 2 * W + 2, 50))])
        assert model.segments(lo, W, 1) == sv_model.segments(lo, W)
        assert model.launches(lo, W, 1) == len(sv_model.segments(lo, W))
    assert model.launches([0, 16, 33, 49], 256, 16) == 3 and model.launches([0, 16, 33, 49], 256, 9) == 3
    assert model.launches([0, 16, 33, 49], 256, 8) == 1 and model.launches([0, 16, 33, 49], 256, 130) == 3


def test_the_model_solves_column_by_column():
    rng = np.random.default_rng(2)
    off, col = _csr([[0], [1, 0], [0, 2, 1], [3, 1]])
    val = rng.uniform(1, 2, len(col))
    B = rng.uniform(-1, 1, (4, 3))
    X = model.solve(off, col, val, B, -0.5, True, False)
    assert X.shape == B.shape and X.dtype == B.dtype
    for j in range(3):
        assert np.array_equal(_bits(X[:, j]), _bits(sv_model.solve(off, col, val, B[:, j].copy(), -0.5, True, False)))


# ---------------------------------------------------------------------------------------------------------------- helpers
GUARD = 8
SENTINEL = 12345.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _raw(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _csr(rowlists):
    off = np.zeros(len(rowlists) + 1, np.int32)
    np.cumsum([len(r) for r in rowlists], out=off[1:])
    return off, np.asarray([c for r in rowlists for c in r], np.int32)


def _values(off, col, rng, dtype):
    """a dominant diagonal in [1, 2], everything else in [-1, 1] divided by the row length; general mantissas"""
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


def _orient(rowlists, lower):
    return rowlists if lower else _flip(rowlists)


def _chain(n):
    return [[0]] + [[r - 1, r] for r in range(1, n)]


def _grid(n):
    return [[c for c in ((i - 1) * n + j if i else -1, i * n + j - 1 if j else -1, i * n + j) if c >= 0] for i in range(n) for j in range(n)]


def _layered(sizes, rng, fan=3):
    """levels of exactly the given sizes, numbered level by level: a row names one row of the level below and up to fan - 1 rows
    anywhere before its level, then its diagonal"""
    rowlists, start = [], 0
    for lvl, n in enumerate(sizes):
        for _ in range(n):
            if lvl == 0:
                rowlists.append([len(rowlists)])
            else:
                deps = [int(rng.integers(start - sizes[lvl - 1], start))] + [int(c) for c in rng.integers(0, start, int(rng.integers(0, fan)))]
                rowlists.append(deps + [len(rowlists)])
        start += n
    return rowlists


def _messy(n, rng, unit):
    """a FULL matrix: entries on both sides of the diagonal in random stored order, repeated columns inside both strict triangles,
    the diagonal somewhere in the middle of its row; unit: some rows empty, some diagonals missing, some stored twice"""
    rowlists = []
    for r in range(n):
        cs = [int(c) for c in rng.integers(0, n, int(rng.integers(0, 9))) if c != r]
        cs += cs[:2]                                                 # repeated columns
        d = [r]
        if unit:
            d = [[], [r], [r, r]][int(rng.integers(0, 3))]
            if rng.integers(0, 5) == 0:
                cs, d = [], []                                       # an empty row
        cs = cs + d
        rng.shuffle(cs)
        rowlists.append(cs)
    return rowlists


def _shifted(a, shift_bytes):
    """a host array as a device tensor whose first element sits shift_bytes behind a 16-byte boundary (whole elements)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    n = shift_bytes // t.element_size()
    buf = torch.zeros(n + t.numel(), dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[n:]
    view.copy_(t)
    return buf, view


def _block(rows, k, ld, tdt, pad, guard=0.0):
    """(buffer, [rows, k] view of leading dimension ld): GUARD guard words before and after, `pad` in the padding columns"""
    buf = torch.full((GUARD + rows * ld + GUARD,), pad, dtype=tdt, device="cuda")
    if guard:
        buf[:GUARD] = guard
        buf[GUARD + rows * ld:] = guard
    return buf, torch.as_strided(buf, (rows, k), (ld, 1), GUARD)


def _untouched_outside(xbuf, X):
    """the guard words and the padding columns of X's buffer still hold the sentinel"""
    probe = xbuf.clone()
    torch.as_strided(probe, tuple(X.shape), tuple(X.stride()), GUARD).fill_(SENTINEL)
    return bool((probe == SENTINEL).all())


def _check_info(plan, k, lo=None):
    got = plan.many_info(k)
    lo = plan.level_offsets.cpu().numpy() if lo is None else lo
    assert got["k"] == k and got["lanes_per_row"] == model.lanes_per_row(k) and got["passes"] == model.passes(k)
    assert got["narrow_lanes"] >= 1
    assert got["launches"] == model.launches(lo, got["narrow_lanes"], k), (k, got)
    return got


class Case:
    """one matrix on the device (possibly misaligned), its plan checked against the csrsv model, and solves on it"""

    def __init__(self, prec, rowlists, lower=True, unit=False, seed=0, shift=0, poison=False):
        self.prec, self.dtype, self.tdt = prec, NP[prec], TORCH[prec]
        self.lower, self.unit, self.rows = lower, unit, len(rowlists)
        self.rng = np.random.default_rng(seed)
        self.off, self.col = _csr(rowlists)
        val = _values(self.off, self.col, self.rng, self.dtype)
        if poison:                                                   # every entry the solve must ignore holds NaN
            r_of = np.repeat(np.arange(self.rows), np.diff(self.off))
            val[~(sv_model.in_triangle(r_of, self.col, lower) | ((self.col == r_of) & (not unit)))] = np.nan
        self.val = val
        self.obuf, self.d_off = _shifted(self.off, shift)
        self.cbuf, self.d_col = _shifted(self.col, shift)
        self.vbuf, self.d_val = _shifted(val, shift if shift % val.itemsize == 0 else val.itemsize)
        if shift:
            assert self.d_off.data_ptr() % 16 == shift and self.d_col.data_ptr() % 16 == shift and self.d_val.data_ptr() % 16 in (shift, 8)
        self.plan = M.CsrSv(self.d_off, self.d_col, lower=lower, unit_diagonal=unit)
        want, order, lo = sv_model.plan_info(self.off, self.col, lower, unit, self.plan.info["narrow_rows"])
        assert {n: self.plan.info[n] for n in want} == want
        assert torch.equal(self.plan.level_offsets.cpu(), torch.from_numpy(lo))
        self.lo = lo

    def rhs(self, k):
        return self.rng.uniform(-1, 1, (self.rows, k)).astype(self.dtype)

    def solve(self, k, alpha=1.0, ldb=None, ldx=None, in_place=False, B=None, want=None, debug=False):
        """one solve_many on guarded buffers: X bit for bit against the model, guards, padding and inputs intact, launches as modelled"""
        ldx = ldx or k
        ldb = ldx if in_place else (ldb or k)
        B = self.rhs(k) if B is None else B
        if want is None:
            want = model.solve(self.off, self.col, self.val, B, alpha, self.lower, self.unit)
        assert want.shape == (self.rows, k) and np.isfinite(want).all()
        info = _check_info(self.plan, k, self.lo)
        xbuf, d_X = _block(self.rows, k, ldx, self.tdt, SENTINEL)
        if in_place:
            bbuf, d_B = xbuf, d_X
        else:
            bbuf, d_B = _block(self.rows, k, ldb, self.tdt, float("nan"), guard=SENTINEL)   # B's padding holds NaN
        d_B.copy_(torch.from_numpy(B))
        inputs = (self.obuf, self.cbuf, self.vbuf) + (() if in_place else (bbuf,))
        keep = [_raw(t).clone() for t in inputs]
        got = self.plan.solve_many(self.d_val, d_B, X=d_X, alpha=alpha, debug_synchronous=debug)
        torch.cuda.synchronize()
        assert got is d_X
        assert torch.equal(_raw(d_X).cpu(), torch.from_numpy(_bits(want))), (self.prec, self.lower, self.unit, k, alpha, ldb, ldx)
        assert _untouched_outside(xbuf, d_X), "guard words or padding columns of X written"
        for t, was in zip(inputs, keep):
            assert torch.equal(_raw(t), was), "an input was modified"
        return info, d_X, want


def _narrow_lanes():
    plan = _empty_plan()
    info = M._CsrSmInfo()
    lib = M.load_library()
    assert lib.mspmv_csrsm_info(plan, 1, ctypes.byref(info)) == 0 and lib.mspmv_csrsv_plan_destroy(plan) == 0
    return int(info.narrow_lanes)


# ---------------------------------------------------------------------------------------------------------------- GPU
KS = [1, 2, 3, 4, 7, 8, 16, 17, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def _sweep_case(prec, lower, unit):
    """the messy matrix of the k sweep, one right-hand side block of 130 columns and its expected X, computed once: column j of the
    solution depends on column j of B alone, so the first k columns serve every k"""
    case = Case(prec, _messy(300, np.random.default_rng(30), unit), lower, unit, seed=30, poison=True)
    B = case.rhs(max(KS))
    return case, B, model.solve(case.off, case.col, case.val, B, 1.0, lower, unit)


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("unit", [False, True], ids=["non_unit", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_k_sweep_on_a_full_unsorted_matrix(prec, lower, unit, k):
    """idle lanes when k is no power of two, the 64-lane cap, two and three passes; NaN in every entry the solve must ignore"""
    case, B, want = _sweep_case(prec, lower, unit)
    case.solve(k, B=np.ascontiguousarray(B[:, :k]), want=np.ascontiguousarray(want[:, :k]), ldx=k + (k % 3))


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_right_hand_side_is_csrsv(prec, lower):
    """k = 1: the bits of CsrSv.solve on the same plan; with ld = 1 the launches of the plan while the two budgets agree; a strided vector"""
    rng = np.random.default_rng(31)
    nl = _narrow_lanes()
    for rowlists in (_messy(300, rng, False), _layered([20, nl + 1, 30, nl, nl + 2, 10], rng), _orient(_grid(20), True)):
        case = Case(prec, _orient(rowlists, lower), lower, seed=31)
        B = case.rhs(1)
        x = case.plan.solve(case.d_val, torch.from_numpy(B[:, 0].copy()).cuda())
        torch.cuda.synchronize()
        info, X, want = case.solve(1, B=B)
        assert torch.equal(_raw(X[:, 0]), _raw(x))
        if info["narrow_lanes"] == case.plan.info["narrow_rows"]:
            assert info["launches"] == case.plan.info["launches"]
            assert model.segments(case.lo, info["narrow_lanes"], 1) == sv_model.segments(case.lo, case.plan.info["narrow_rows"])
        _, X, _ = case.solve(1, B=B, want=want, ldb=3, ldx=2, alpha=1.0)
        assert torch.equal(_raw(X[:, 0]), _raw(x))


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_leading_dimensions_and_alignment(prec, lower):
    """ldb != ldx, both > k, both odd: the rows of B and X start at every 4-byte (fp64: 8-byte) phase of a 16-byte line; B's padding
    holds NaN; the matrix arrays 4 and 8 bytes off a 16-byte boundary"""
    rowlists = _messy(200, np.random.default_rng(32), False)
    for shift in (0, 4, 8):
        case = Case(prec, rowlists, lower, seed=32, shift=shift)
        B = case.rhs(3)
        _, _, want = case.solve(3, B=B, ldb=5, ldx=7)
        case.solve(3, B=B, want=want, ldb=7, ldx=5)
    case = Case(prec, _orient(_chain(70), lower), lower, seed=32, shift=4)
    case.solve(3, ldb=5, ldx=7)


@gpu
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bidiagonal_chain(prec, lower, k):
    """1100 levels of one row: one narrow launch that crosses the 1024-level LDS staging chunk"""
    case = Case(prec, _orient(_chain(1100), lower), lower, seed=33)
    info, _, _ = case.solve(k, ldx=k + 1)
    assert case.plan.info["levels"] == 1100 and info["launches"] == 1


@gpu
@pytest.mark.parametrize("k", [2, 16])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_five_point_grid(prec, lower, k):
    """40 x 40: at k = 2 every level is narrow; at k = 16 the levels above 16 rows are wide (the starting budget of 256 lanes)"""
    case = Case(prec, _orient(_grid(40), lower), lower, seed=34)
    info, _, _ = case.solve(k)
    assert case.plan.info["levels"] == 79 and case.plan.info["max_level_rows"] == 40
    segs = model.segments(case.lo, info["narrow_lanes"], info["lanes_per_row"])
    assert info["launches"] == len(segs)
    if info["narrow_lanes"] == 256:
        assert info["launches"] == (1 if k == 2 else 49)              # 1..16 | 17, ..., 40, ..., 17 each alone | 16..1
        if k == 16:
            assert segs[0] == (0, 16, True) and segs[-1] == (63, 79, True) and not any(s[2] for s in segs[1:-1])


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_budget_boundary(prec, lower):
    nl = _narrow_lanes()
    rng = np.random.default_rng(35)
    # P = 16: levels of exactly narrow_lanes / P rows and one more; narrow -> wide -> narrow -> wide -> narrow; a level of 5 rows (80
    # lanes: its last wave is partial) inside a run of narrow levels and as a launch of its own between two wide ones
    n = nl // 16
    assert n > 5
    sizes = [n - 1, n, n + 1, n, 5, n + 1, 5, n + 2, 3]
    case = Case(prec, _orient(_layered(sizes, rng), lower), lower, seed=35)
    info, _, _ = case.solve(16, ldb=17, ldx=19)
    assert model.segments(case.lo, nl, 16) == [(0, 2, True), (2, 3, False), (3, 5, True), (5, 6, False), (6, 7, True), (7, 8, False), (8, 9, True)]
    assert info["lanes_per_row"] == 16 and info["launches"] == 7
    # the same plan at k = 9 (P = 16 with seven idle lanes) and at k = 8 (P = 8: every level narrow)
    assert case.solve(9)[0]["launches"] == 7
    assert case.solve(8)[0]["launches"] == 1
    # P = 4: a wide level of 300 rows, 1200 lanes: its last workgroup is partial (4 workgroups and 176 lanes)
    assert 300 * 4 > nl
    case = Case(prec, _orient(_layered([10, 300, 7], rng), lower), lower, seed=36)
    info, _, _ = case.solve(4, ldx=6)
    assert info["launches"] == 3


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_long_row_among_short_ones(prec, lower):
    rng = np.random.default_rng(37)
    rowlists = _layered([40, 60, 300, 30], rng)
    n = len(rowlists)
    rowlists.append([int(c) for c in rng.permutation(n)[:300]] + [n])   # 300 strict entries in stored (random) order
    rowlists += [[n, n + 1], [n + 2, 3, n], [n + 3]]                    # rows that wait for it
    case = Case(prec, _orient(rowlists, lower), lower, seed=37)
    assert case.plan.info["used_entries"] >= 300
    case.solve(8, ldx=9)


@gpu
@pytest.mark.parametrize("alpha", [1.0, -0.5, 0.0])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_alpha(prec, alpha):
    for lower in (True, False):
        for unit in (False, True):
            Case(prec, _messy(120, np.random.default_rng(38), unit), lower, unit, seed=38).solve(5, alpha=alpha, ldb=6, ldx=8)


@gpu
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_in_place(prec, lower):
    """X is B, ldx == ldb: a lane reads B[r, j] before it writes X[r, j], and nothing else reads that word"""
    case = Case(prec, _messy(200, np.random.default_rng(39), False), lower, seed=39)
    for k, ld in ((3, 3), (3, 5), (16, 17), (70, 70)):
        case.solve(k, ldx=ld, in_place=True, alpha=-0.5)
    Case(prec, _orient(_grid(20), lower), lower, seed=39).solve(16, ldx=16, in_place=True)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_degenerate_sizes(prec):
    for lower in (True, False):
        for unit in (False, True):
            case = Case(prec, [[0]], lower, unit, seed=40)                                  # rows = 1
            for k in (1, 5, 65):
                assert case.solve(k, alpha=-0.5)[0]["launches"] == 1
            # an empty row in the middle (UNIT), a row with its diagonal alone (NON_UNIT)
            rowlists = _orient([[0], [0, 1], [] if unit else [2], [1, 3], [2, 4, 3]], lower)
            Case(prec, rowlists, lower, unit, seed=41).solve(3, ldx=4)
        case = Case(prec, [[] for _ in range(37)], lower, True, seed=42)                    # nnz == 0 with UNIT: X = alpha * B
        B = case.rhs(6)
        info, X, _ = case.solve(6, alpha=-0.5, B=B, ldb=7, ldx=9)
        assert info["launches"] == 1
        assert torch.equal(_raw(X).cpu(), torch.from_numpy(_bits((NP[prec](-0.5) * B).astype(NP[prec]))))


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_reuse(prec):
    """one plan serves solve, solve_many at k = 3, at k = 16, and solve again; a second solve_many gives identical bits"""
    rng = np.random.default_rng(43)
    case = Case(prec, _layered([30, 50, 20, 70, 10], rng), True, seed=43)
    b = case.rhs(1)[:, 0].copy()
    want = sv_model.solve(case.off, case.col, case.val, b)
    d_b = torch.from_numpy(b).cuda()
    x1 = case.plan.solve(case.d_val, d_b)
    torch.cuda.synchronize()
    assert torch.equal(_raw(x1).cpu(), torch.from_numpy(_bits(want)))
    case.solve(3, ldx=4)
    B = case.rhs(16)
    _, X, want16 = case.solve(16, B=B)
    first = _raw(X).clone()
    _, X, _ = case.solve(16, B=B, want=want16)
    assert torch.equal(_raw(X), first)
    x2 = case.plan.solve(case.d_val, d_b)
    torch.cuda.synchronize()
    assert torch.equal(_raw(x2), _raw(x1))
    # the one-shot call, on a view of a wider block
    wide = torch.full((case.rows, 20), float("nan"), dtype=case.tdt, device="cuda")
    wide[:, :16].copy_(torch.from_numpy(B))
    Xo = M.csrsm(case.d_val, case.d_off, case.d_col, wide[:, :16])
    assert Xo.shape == (case.rows, 16) and torch.equal(_raw(Xo).cpu(), torch.from_numpy(_bits(want16)))
    case.plan.close()
    with pytest.raises(M.MspmvError):
        case.plan.solve_many(case.d_val, wide[:, :16])
    with pytest.raises(M.MspmvError):
        case.plan.many_info(4)


@gpu
def test_refusals_launch_nothing():
    """a plan with a bad diagonal row, NULL B or X with rows > 0, NULL matrix arrays with nnz > 0, k < 1, ld < k: refused, X untouched"""
    lib = M.load_library()
    base = _chain(50)
    off, col = _csr(base[:7] + [[6]] + base[8:])
    assert sv_model.bad_diagonal_row(off, col) == 7
    d_off, d_col = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda()
    goff, gcol = _csr(base)
    d_goff, d_gcol = torch.from_numpy(goff).cuda(), torch.from_numpy(gcol).cuda()
    for lower in (True, False):
        bad = M.CsrSv(d_off, d_col, lower=lower)
        good = M.CsrSv(d_goff, d_gcol, lower=lower)
        assert bad.info["bad_diagonal_row"] == 7 and good.info["bad_diagonal_row"] == -1
        assert bad.many_info(4)["launches"] >= 1                                            # (the figures exist; the solve is refused)
        for prec, (name, ct) in SOLVE.items():
            fn = getattr(lib, name)
            val = torch.ones(col.size, dtype=TORCH[prec], device="cuda")
            gval = torch.ones(gcol.size, dtype=TORCH[prec], device="cuda")
            B = torch.ones(50, 4, dtype=TORCH[prec], device="cuda")
            xbuf, X = _block(50, 4, 5, TORCH[prec], SENTINEL)
            with pytest.raises(M.MspmvError):
                bad.solve_many(val, B, X=X)
            s = M._stream_handle(None)
            p = M._ptr
            assert fn(bad._handle, p(val), p(d_off), p(d_col), ct(1.0), p(B), 4, p(X), 5, 4, s, 0) == 1
            g = (good._handle, p(gval), p(d_goff), p(d_gcol), ct(1.0))
            assert fn(*g, None, 4, p(X), 5, 4, s, 0) == 1 and fn(*g, p(B), 4, None, 5, 4, s, 0) == 1
            assert fn(good._handle, None, p(d_goff), p(d_gcol), ct(1.0), p(B), 4, p(X), 5, 4, s, 0) == 1
            assert fn(good._handle, p(gval), None, p(d_gcol), ct(1.0), p(B), 4, p(X), 5, 4, s, 0) == 1
            assert fn(good._handle, p(gval), p(d_goff), None, ct(1.0), p(B), 4, p(X), 5, 4, s, 0) == 1
            assert fn(*g, p(B), 4, p(X), 5, 0, s, 0) == 1 and fn(*g, p(B), 3, p(X), 5, 4, s, 0) == 1 and fn(*g, p(B), 4, p(X), 3, 4, s, 0) == 1
            torch.cuda.synchronize()
            assert bool((xbuf == SENTINEL).all())
            # wrong shapes and devices are the wrapper's to refuse
            with pytest.raises(M.MspmvError):
                good.solve_many(gval, torch.ones(49, 4, dtype=TORCH[prec], device="cuda"))
            with pytest.raises(M.MspmvError):
                good.solve_many(gval, B, X=torch.ones(50, 3, dtype=TORCH[prec], device="cuda"))
            with pytest.raises(M.MspmvError):
                good.solve_many(gval[:-1], B)
            assert fn(*g, p(B), 4, p(X), 5, 4, s, 0) == 0                                   # and the good call goes through
            torch.cuda.synchronize()
            assert not bool((X == SENTINEL).any()) and _untouched_outside(xbuf, X)


@gpu
def test_graph_capture_and_replay():
    """one solve_many on the grid captured (k = 4: one launch; k = 16: 49 launches in a chain), replayed twice on new B"""
    case = Case("f32", _grid(40), True, seed=44)
    for k in (4, 16):
        info = _check_info(case.plan, k, case.lo)
        d_B = torch.zeros(case.rows, k, dtype=torch.float32, device="cuda")
        xbuf, d_X = _block(case.rows, k, k + 1, torch.float32, SENTINEL)
        case.plan.solve_many(case.d_val, d_B, X=d_X, alpha=2.0)                             # (warm-up outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            case.plan.solve_many(case.d_val, d_B, X=d_X, alpha=2.0)
        for seed in (45, 46):
            B = np.random.default_rng(seed).uniform(-1, 1, (case.rows, k)).astype(np.float32)
            want = model.solve(case.off, case.col, case.val, B, 2.0)
            assert np.isfinite(want).all()
            d_B.copy_(torch.from_numpy(B))
            d_X.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(_raw(d_X).cpu(), torch.from_numpy(_bits(want)))
            assert _untouched_outside(xbuf, d_X)
        assert info["launches"] == (1 if k == 4 else 49) or info["narrow_lanes"] != 256


@gpu
def test_launch_lines_number_the_launches(capfd):
    nl = _narrow_lanes()
    rng = np.random.default_rng(47)
    n = nl // 16
    for sizes, k in (([5], 16), ([3, n + 1, n, n + 2, n + 3, 2], 16), ([n + 1], 16), ([3, n + 1, n, n + 2, n + 3, 2], 3), ([nl + 1, 4], 1)):
        case = Case("f64", _layered(sizes, rng), True, seed=47)
        capfd.readouterr()
        info, _, _ = case.solve(k, debug=True)
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
        segs = model.segments(case.lo, nl, model.lanes_per_row(k))
        assert len(lines) == info["launches"] == len(segs), lines
        assert all(l.startswith("mspmv: sm_") for l in lines)
        for line, (l0, l1, narrow) in zip(lines, segs):
            if narrow:
                assert line == "mspmv: sm_narrow_kernel<<<1, 1024>>>", line
            else:
                lanes = int(case.lo[l1] - case.lo[l0]) * model.lanes_per_row(k)
                assert line == f"mspmv: sm_level_kernel<<<{-(-lanes // 256)}, 256>>>", line


def _grid_full(n, rng, dtype):
    """the symmetric 5-point matrix of an n x n grid, rows sorted: a dominant diagonal, -1 beside it (exactly symmetric)"""
    rowlists, vals = [], []
    for i in range(n):
        for j in range(n):
            r = i * n + j
            cs = sorted(c for c in ((i - 1) * n + j if i else -1, r - 1 if j else -1, r, r + 1 if j < n - 1 else -1, (i + 1) * n + j if i < n - 1 else -1) if c >= 0)
            rowlists.append(cs)
            vals += [rng.uniform(4, 5) if c == r else -1.0 for c in cs]
    off, col = _csr(rowlists)
    return off, col, np.asarray(vals, dtype)


@gpu
@pytest.mark.parametrize("which", ["Ilu0", "Ic0"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_preconditioners_solve_many(prec, which):
    """k = 5 on a 12 x 12 grid: column by column and on the bits, solve on each column; the kept block follows k"""
    rng = np.random.default_rng(48)
    off, col, val = _grid_full(12, rng, NP[prec])
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off, col, val))
    pre = getattr(M, which)(d_off, d_col)
    with pytest.raises(M.MspmvError):
        pre.solve_many(torch.zeros(144, 5, dtype=TORCH[prec], device="cuda"))               # nothing factorised yet
    pre.factor(d_val)
    for k, ld in ((5, 8), (2, 2), (5, 5)):
        R = rng.uniform(-1, 1, (144, k)).astype(NP[prec])
        rbuf, d_R = _block(144, k, ld, TORCH[prec], float("nan"))
        d_R.copy_(torch.from_numpy(R))
        Z = pre.solve_many(d_R)
        torch.cuda.synchronize()
        assert Z.shape == (144, k) and pre._mid_many.shape == (144, k) and bool(torch.isfinite(Z).all())
        for j in range(k):
            z = pre.solve(torch.from_numpy(R[:, j].copy()).cuda())
            torch.cuda.synchronize()
            assert torch.equal(_raw(Z[:, j]), _raw(z)), (which, k, j)
        obuf, out = _block(144, k, k + 2, TORCH[prec], SENTINEL)
        assert pre.solve_many(d_R, out=out) is out
        torch.cuda.synchronize()
        assert torch.equal(_raw(out), _raw(Z)) and _untouched_outside(obuf, out)
    pre.close()
    with pytest.raises(M.MspmvError):
        pre.solve_many(d_R)


@gpu
@pytest.mark.parametrize("unit", [False, True], ids=["non_unit", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_round_trip_through_csrmm(lower, unit):
    """meaning, not only bits: in fp64, |T X - alpha B| <= (len + 1) * eps * (|T||X| + |alpha B|) elementwise, T the triangle extracted
    on the host (with its diagonal; 1 for UNIT) and multiplied through M.csrmm, len the entries of T's row: substitution (gamma_len
    |T||X|, Higham, Accuracy and Stability, 8.1) plus the rounding of the product that checks it (another gamma_len |T||X|)"""
    alpha, k = -0.5, 6
    case = Case("f64", _messy(300, np.random.default_rng(49), unit), lower, unit, seed=49)
    B = case.rhs(k)
    _, d_X, _ = case.solve(k, alpha=alpha, B=B, ldx=k + 1)
    off, col, val, n = case.off, case.col, case.val, case.rows
    t_rows = []
    for r in range(n):
        ent = [(int(col[e]), float(val[e])) for e in range(off[r], off[r + 1]) if sv_model.in_triangle(r, int(col[e]), lower)]
        ent.append((r, 1.0 if unit else next(float(val[e]) for e in range(off[r], off[r + 1]) if col[e] == r)))
        t_rows.append(ent)
    t_off, t_col = _csr([[c for c, _ in ent] for ent in t_rows])
    t_val = np.asarray([v for ent in t_rows for _, v in ent], np.float64)
    Y = M.csrmm(torch.from_numpy(t_val).cuda(), torch.from_numpy(t_off).cuda(), torch.from_numpy(t_col).cuda(), d_X)   # X's own layout, no copy
    torch.cuda.synchronize()
    Y, Xh = Y.cpu().numpy().astype(np.longdouble), d_X.cpu().numpy().astype(np.longdouble)
    lens = np.diff(t_off).astype(np.longdouble)[:, None]
    mag = np.stack([sum(abs(np.longdouble(v)) * np.abs(Xh[c]) for c, v in ent) for ent in t_rows])
    aB = np.longdouble(alpha) * B.astype(np.longdouble)
    bound = (lens + 1) * np.longdouble(np.finfo(np.float64).eps) * (mag + np.abs(aB))
    resid = np.abs(Y - aB)
    print("worst residual / bound:", float((resid / bound).max()))
    assert (resid <= bound).all()
