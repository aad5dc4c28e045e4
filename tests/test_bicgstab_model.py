"""The CPU side of BiCGStab (mspmv_bicgstab_* of include/mspmv_krylov.h): tests/bicgstab_model.py, the numpy restatement of the
arithmetic, converges on the matrices the device tests use and takes every exit of the table; the header is plain C99, the new
library exports what it declares and nothing else, the ctypes prototypes match it, and the refusals come before any device is
touched.  Every precondition of a device test's reference is asserted here with a product on the host."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import bicgstab_common as C
import bicgstab_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, _bits, _host_product, _true_residual
from test_abi_prototypes import declared, mismatches, prototyped
from test_pcg_shapes import _host_ilu0

B = importlib.import_module("merge_spmv_amd.bicgstab")        # (the package attribute of this name is the one-shot function)
NEW = ["mspmv_bicgstab_create", "mspmv_bicgstab_destroy", "mspmv_bicgstab_set_factor", "mspmv_bicgstab_solve_f32", "mspmv_bicgstab_solve_f64",
       "mspmv_bicgstab_state"]
ALL = ["DeviceSpmv", "csrmv", "csrmv_mixed", "csrmm", "CsrMVWorkspace", "CsrMVPlan", "csr_transpose", "CsrTranspose", "coo_to_csr", "CooToCsr",
       "csr_sum_duplicates", "coomv", "csr_add", "CsrAdd", "csr_symmetrize", "csr_gemm", "CsrGemm", "csr_gemm_products", "sddmm", "CsrSv", "csrsv",
       "csrsm", "csrilu0", "Ilu0", "csric0", "Ic0", "CsrColoring", "csr_color", "csr_permute", "multicolor_reorder", "vec_dot", "Pcg", "pcg",
       "plan_bench_record", "library_path", "load_library", "launch_info", "set_tuning", "set_tdm", "clocked_bands", "debug_read_tiles",
       "profile_begin", "profile_end", "MspmvError", "TUNE_ATOMIC_FIX", "TUNE_NO_VEC"]
NONE, JACOBI, FACTOR = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------ the model
def _host_preconds(off, col, val):
    d = C.diagonal_of(off, col, val)
    return {"none": lambda r: r, "jacobi": lambda r: r / d}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("grid", C.GRIDS, ids=["24x24", "40x25"])
def test_the_model_converges_on_the_grids(grid, prec):
    """no shift of the diagonal was needed: 4 + (i + 1) / (2 n + 1) converges within the limits as it is"""
    off, col, val = C.convection_diffusion(grid[0], grid[1], NP[prec])
    n = len(off) - 1
    d = C.diagonal_of(off, col, val)
    assert n == grid[0] * grid[1] and np.unique(d).size == n and (np.frexp(d)[0] != 0.5).all()         # all differ, no power of two
    dense = np.zeros((n, n))
    dense[C.rows_of(off), col] = val
    assert not np.array_equal(dense, dense.T)                                                          # nonsymmetric
    b = C.rhs(n, NP[prec])
    runs = {}
    for name, apply_m in _host_preconds(off, col, val).items():
        x, status, iterations, history, left = model.bicgstab(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, LIMIT)
        assert status == model.CONVERGED and left in ("half", "rr") and 7 < iterations <= LIMIT and history.size == iterations + 1
        assert x.dtype == NP[prec] and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
        runs[name] = x
        # from a guess
        x, status, iterations, _, _ = model.bicgstab(_host_product(off, col, val), apply_m, b, C.guess(n, NP[prec]), RTOL[prec], 0.0, LIMIT)
        assert status == model.CONVERGED and 7 < iterations <= LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
    assert not np.array_equal(_bits(runs["none"]), _bits(runs["jacobi"]))                               # Jacobi differs from none


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_converges_with_ilu0_on_the_host(prec):
    """ILU(0) in fp64 on the host (the device's is in the value type): convergence, more than 5 iterations on the 24 x 24 grid (the
    launch lines are counted over 5), and on the 40 x 25 grid in fp64 at most a third of the iterations of no preconditioner (the device test asserts half)"""
    counts = {}
    for grid in C.GRIDS:
        off, col, val = C.convection_diffusion(grid[0], grid[1], NP[prec])
        b = C.rhs(len(off) - 1, NP[prec])
        for name, apply_m in (("none", lambda r: r), ("ilu0", _host_ilu0(off, col, val))):
            x, status, iterations, _, _ = model.bicgstab(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, LIMIT)
            assert status == model.CONVERGED and 5 < iterations <= LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
            counts[grid, name] = iterations
    assert prec == "f32" or 3 * counts[(40, 25), "ilu0"] <= counts[(40, 25), "none"]
    off, col, val = C.banded(4160, NP[prec])
    b = C.rhs(4160, NP[prec])
    x, status, iterations, _, _ = model.bicgstab(_host_product(off, col, val), _host_ilu0(off, col, val), b, None, RTOL[prec], 0.0, LIMIT)
    assert status == model.CONVERGED and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", C.SIZES)
def test_the_model_converges_on_the_band(n, prec):
    off, col, val = C.banded(n, NP[prec])
    assert len(off) - 1 == n
    d = C.diagonal_of(off, col, val)
    assert (np.frexp(d)[0] != 0.5).all() and (n < 2 or np.unique(d).size > 1)
    b = C.rhs(n, NP[prec])
    for apply_m in _host_preconds(off, col, val).values():
        x, status, iterations, _, _ = model.bicgstab(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, LIMIT)
        assert status == model.CONVERGED and 0 < iterations <= LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_is_running_after_three_iterations_of_the_long_matrix(prec):
    off, col, val = C.bidiagonal(C.FOLD_N, NP[prec])
    assert -(-C.FOLD_N // 1024) == 1026 and C.FOLD_N % 4 == 1
    for apply_m in _host_preconds(off, col, val).values():
        info = {}
        _, status, iterations, history, left = model.bicgstab(_host_product(off, col, val), apply_m, C.rhs(C.FOLD_N, NP[prec]), None, RTOL[prec],
                                                              0.0, C.FOLD_ITERATIONS, info)
        assert (status, iterations, left) == (model.RUNNING, C.FOLD_ITERATIONS, None)
        assert np.isfinite(history).all() and (history > info["stop2"]).all()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(C.EXIT_CASES))
def test_every_exit_is_taken_on_the_host(name, prec):
    a, b, max_iterations, status, iterations, left = C.EXIT_CASES[name]
    a, b = np.asarray(a, NP[prec]), np.asarray(b, NP[prec])
    info = {}
    got = model.bicgstab(lambda p: a @ p, lambda r: r, b, None, RTOL[prec], 0.0, max_iterations, info)
    assert got[1:3] == (status, iterations) and got[4] == left == info["exit"] and got[3].size == iterations + 1
    # ... and the sparse product of the device tests' pattern (every entry stored) is the dense one on these exact systems
    off, col, val = C.dense_csr(a, NP[prec])
    again = model.bicgstab(_host_product(off, col, val), lambda r: r, b, None, RTOL[prec], 0.0, max_iterations)
    assert again[1:3] == got[1:3] and again[4] == left and np.array_equal(_bits(again[0]), _bits(got[0]))
    if name == "rv":
        assert not _bits(got[0]).any()                              # nothing of the iteration is written
    if name == "tt":
        assert got[0].any() and got[3][1] == info["rr"]              # x keeps the half step, rr is ss
    if name in ("half", "rr"):
        assert _true_residual(off, col, val, got[0], b) <= RESIDUAL[prec]


def test_special_values_in_b_on_the_host():
    """the preconditions of the device test: what Inf, NaN and -0.0 in b do to the model"""
    off, col, val = C.banded(1025, np.float64)
    for bad, want in ((np.inf, (model.BREAKDOWN, 0, "rv")), (np.nan, (model.BREAKDOWN, 0, "rv"))):
        b = C.rhs(1025, np.float64)
        b[1000] = bad
        x, status, iterations, history, left = model.bicgstab(_host_product(off, col, val), lambda r: r, b, None, 1e-10, 0.0, 10)
        assert (status, iterations, left) == want and not _bits(x).any() and not np.isfinite(history[0])
    b = C.rhs(1025, np.float64)
    b[::3] = -0.0
    x, status, iterations, _, _ = model.bicgstab(_host_product(off, col, val), lambda r: r, b, None, 1e-10, 0.0, LIMIT)
    assert status == model.CONVERGED and _true_residual(off, col, val, x, b) <= RESIDUAL["f64"]


# ------------------------------------------------------------------------------------------------------------ the boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T mspmv_" in l)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "include/mspmv_krylov.h"\n'
                   "int use(void) { mspmv_bicgstab_t *s = 0; mspmv_bicgstab_state_t st;\n"
                   "  int e = mspmv_bicgstab_create(&s, 0, 0, 0, 0, 8, MSPMV_BICGSTAB_NONE, 0, 0);\n"
                   "  e |= mspmv_bicgstab_solve_f64(s, 0, 0, 0, 0, 0, 0, 1e-8, 0.0, 10, 0, 0, 0, 0); e |= mspmv_bicgstab_state(s, &st, 0);\n"
                   "  return e | mspmv_bicgstab_destroy(s) | (st.exit_test == MSPMV_BICGSTAB_EXIT_START) | MSPMV_PCG_CONVERGED; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "hdr.o"), "-I", ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_what_the_header_declares_and_nothing_else():
    functions = declared("mspmv_krylov.h")
    assert sorted(functions) == NEW
    krylov = os.path.join(os.path.dirname(M.library_path("product")), "libmspmv_krylov.so")
    assert _exported(krylov) == NEW
    assert not set(_exported(M.library_path("product"))) & set(NEW)            # the product library exports none of them
    assert not set(declared("mspmv.h")) & set(NEW)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", krylov], capture_output=True, text=True, check=True).stdout
    needs = sorted(l.split()[-1] for l in undefined.splitlines() if " mspmv_" in l)
    assert needs and set(needs) <= set(declared("mspmv.h"))                     # it calls only what mspmv.h declares


def test_the_prototypes_match_the_header():
    lib = B.load_krylov_library()
    functions = declared("mspmv_krylov.h")
    assert mismatches(lib, functions) == []
    assert sorted(prototyped(lib)) == sorted(functions)
    assert functions["mspmv_bicgstab_solve_f32"][1][7:9] == ["double", "double"] and len(functions["mspmv_bicgstab_solve_f64"][1]) == 14
    # the table went on the new CDLL, never on the product's
    prev = M.active_library()
    try:
        M.use_library("product")
        product = M.load_library()
    finally:
        M.use_library(prev)
    assert lib is not product and not [n for n in prototyped(product) if "bicgstab" in n]
    # the state block as ctypes lays it out is the header's: six int32, six doubles, one uint64
    assert ctypes.sizeof(B._BicgstabState) == 6 * 4 + 6 * 8 + 8 and B._BicgstabState.rr.offset == 24


def test_one_product_library_is_mapped_and_the_surface_is_unchanged():
    B.load_krylov_library()
    with open("/proc/self/maps") as f:
        files = {line.split()[-1] for line in f if line.rstrip().endswith("/libmspmv.so")}
    assert len(files) == 1 and os.path.samefile(files.pop(), M.library_path("product"))
    assert M.__all__ == ALL
    assert M.Bicgstab is B.Bicgstab and M.bicgstab is B.bicgstab and M.BICGSTAB_EXIT is B.BICGSTAB_EXIT
    assert M.BICGSTAB_EXIT == model.EXITS and len(M.BICGSTAB_EXIT) == 9
    assert M.load_library().mspmv_version() == 102


# ------------------------------------------------------------------------------------------------------------ refusals
def _create(rows, nnz, vb=8, kind=NONE, off=4096, col=4096, out=True):
    """mspmv_bicgstab_create on fake device pointers (refusals come before anything is touched; rows == 0 touches nothing at all)"""
    lib = B.load_krylov_library()
    handle = ctypes.c_void_p(0)
    st = lib.mspmv_bicgstab_create(ctypes.byref(handle) if out else None, ctypes.c_void_p(off) if off else None, ctypes.c_void_p(col) if col else None,
                                   rows, nnz, vb, kind, None, 0)
    return st, handle


def test_create_refuses_before_any_launch():
    assert _create(-1, 0)[0] == 1 and _create(5, -1)[0] == 1
    assert _create(2 ** 30, 2 ** 30)[0] == 1                                      # rows + nnz beyond the library's limit
    assert _create(2 ** 30 + 1, 0)[0] == 1                                        # rows beyond the reduction's
    assert _create(0, 5)[0] == 1
    assert _create(5, 5, vb=2)[0] == 1 and _create(5, 5, kind=3)[0] == 1 and _create(5, 5, kind=-1)[0] == 1
    assert _create(5, 5, off=0)[0] == 1 and _create(5, 5, col=0)[0] == 1          # NULL arrays
    assert _create(0, 0, out=False)[0] == 1
    lib = B.load_krylov_library()
    assert lib.mspmv_bicgstab_destroy(None) == 1 and lib.mspmv_bicgstab_state(None, None, None) == 1


def _solve(lib, handle, vb=8, rtol=1e-8, atol=0.0, max_iterations=10, check_every=0):
    fn = lib.mspmv_bicgstab_solve_f32 if vb == 4 else lib.mspmv_bicgstab_solve_f64
    return fn(handle, None, None, None, None, None, 0, rtol, atol, max_iterations, check_every, None, None, 0)


@pytest.mark.parametrize("kind", [NONE, JACOBI, FACTOR])
def test_no_rows_touch_no_device_and_solve_refusals(kind):
    lib, product = B.load_krylov_library(), M.load_library()
    st, handle = _create(0, 0, vb=8, kind=kind, off=0, col=0)
    assert st == 0 and handle.value
    state = B._BicgstabState()
    assert lib.mspmv_bicgstab_state(handle, ctypes.byref(state), None) == 0
    assert (state.launches_per_iteration, state.precond_kind, state.bad_diagonal_row, state.exit_test) == (9, kind, -1, 0)
    if kind == FACTOR:
        assert _solve(lib, handle) == 1                                           # FACTOR without set_factor
        assert lib.mspmv_bicgstab_set_factor(handle, None, None, None, None, None) == 1
        plans = []
        for uplo in (0, 1):
            plan = ctypes.c_void_p(0)
            assert product.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, uplo, 0, None, 0) == 0
            plans.append(plan)
        assert lib.mspmv_bicgstab_set_factor(handle, plans[0], None, None, None, None) == 1
        assert lib.mspmv_bicgstab_set_factor(handle, plans[0], plans[1], None, None, None) == 0
    else:
        plan = ctypes.c_void_p(0)
        assert product.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, 0, 0, None, 0) == 0
        assert lib.mspmv_bicgstab_set_factor(handle, plan, plan, None, None, None) == 1      # a handle of another kind
        plans = [plan]
    for bad in (dict(rtol=-1e-8), dict(rtol=float("nan")), dict(atol=-1.0), dict(atol=float("nan")), dict(max_iterations=-1),
                dict(check_every=-1), dict(vb=4)):
        assert _solve(lib, handle, **bad) == 1, bad
    assert lib.mspmv_bicgstab_solve_f64(None, None, None, None, None, None, 0, 1e-8, 0.0, 10, 0, None, None, 0) == 1
    for check_every in (0, 3):
        assert _solve(lib, handle, atol=0.5, check_every=check_every) == 0
        assert lib.mspmv_bicgstab_state(handle, ctypes.byref(state), None) == 0
        assert (state.status, state.iterations, state.exit_test, state.rr, state.bb, state.stop2) == (1, 0, 1, 0.0, 0.0, 0.25)     # CONVERGED (start)
    assert lib.mspmv_bicgstab_destroy(handle) == 0
    for plan in plans:
        assert product.mspmv_csrsv_plan_destroy(plan) == 0
