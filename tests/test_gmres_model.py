"""The CPU side of GMRES(m) (mspmv_gmres_* of include/mspmv_gmres.h): tests/gmres_model.py, the numpy restatement of the arithmetic,
converges on the matrices the device tests use, at every restart length they use, and takes every exit of the table; the header is
plain C99, the new library exports what it declares and nothing else, the ctypes prototypes match it, and the refusals come before
any device is touched.  Every precondition of a device test's reference is asserted here with a product on the host."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import bicgstab_common as C
import gmres_common as G
import gmres_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, _bits, _host_product, _true_residual
from test_abi_prototypes import declared, mismatches, prototyped
from test_pcg_shapes import _host_ilu0

GM = importlib.import_module("merge_spmv_amd.gmres")          # (the package attribute of this name is the one-shot function)
NEW = ["mspmv_gmres_create", "mspmv_gmres_destroy", "mspmv_gmres_set_factor", "mspmv_gmres_solve_f32", "mspmv_gmres_solve_f64", "mspmv_gmres_state"]
KRYLOV = ["mspmv_bicgstab_create", "mspmv_bicgstab_destroy", "mspmv_bicgstab_set_factor", "mspmv_bicgstab_solve_f32", "mspmv_bicgstab_solve_f64",
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
def test_the_model_converges_on_the_grids_at_every_restart(grid, prec):
    off, col, val = C.convection_diffusion(grid[0], grid[1], NP[prec])
    n = len(off) - 1
    b = C.rhs(n, NP[prec])
    for name, apply_m in _host_preconds(off, col, val).items():
        for restart in G.RESTARTS:
            info = {}
            x, status, iterations, history, left = model.gmres(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, restart, LIMIT, info)
            assert (status, left) == (model.CONVERGED, "rr") and 7 < iterations <= info["slots"] <= LIMIT, (name, restart, iterations, info)
            assert history.size == iterations + 1 and history[-1] == info["rr"] <= info["stop2"]
            assert info["cycles"] >= -(-iterations // restart) and x.dtype == NP[prec]
            assert _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
            if restart == 30:
                assert info["cycles"] >= 2                           # the device tests at restart = 30 run through a restart
        # from a guess
        x, status, iterations, _, _ = model.gmres(_host_product(off, col, val), apply_m, b, C.guess(n, NP[prec]), RTOL[prec], 0.0, 30, LIMIT)
        assert status == model.CONVERGED and 7 < iterations <= LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_converges_with_ilu0_on_the_host(prec):
    """ILU(0) in fp64 on the host (the device's is in the value type): convergence on both grids and the long band at restart = 30,
    and, in fp64 on the 24 x 24 grid, GMRES(3) still RUNNING after 8 slots (the launch lines are counted over 2, 5 and 8)"""
    for off, col, val in [C.convection_diffusion(g[0], g[1], NP[prec]) for g in C.GRIDS] + [C.banded(4160, NP[prec])]:
        b = C.rhs(len(off) - 1, NP[prec])
        x, status, iterations, _, _ = model.gmres(_host_product(off, col, val), _host_ilu0(off, col, val), b, None, RTOL[prec], 0.0, 30, LIMIT)
        assert status == model.CONVERGED and 3 < iterations <= LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
    if prec == "f64":
        off, col, val = C.convection_diffusion(24, 24, NP[prec])
        b = C.rhs(576, NP[prec])
        for apply_m in (lambda r: r, _host_ilu0(off, col, val)):
            info = {}
            got = model.gmres(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, 3, 8, info)
            assert (got[1], got[2], info["slots"], info["cycles"]) == (model.RUNNING, 8, 8, 3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", C.SIZES)
def test_the_model_converges_on_the_band(n, prec):
    off, col, val = C.banded(n, NP[prec])
    b = C.rhs(n, NP[prec])
    for apply_m in _host_preconds(off, col, val).values():
        for restart in G.BAND_RESTARTS:
            info = {}
            x, status, iterations, _, left = model.gmres(_host_product(off, col, val), apply_m, b, None, RTOL[prec], 0.0, restart, LIMIT, info)
            assert (status, left) == (model.CONVERGED, "rr") and 0 < iterations <= LIMIT, (restart, iterations, info)
            assert _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
            if restart > n:
                assert iterations <= n + 1 and iterations < info["slots"]        # fewer columns than slots: closed by hn or the estimate


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_is_running_after_three_iterations_of_the_long_matrix(prec):
    off, col, val = C.bidiagonal(C.FOLD_N, NP[prec])
    assert -(-C.FOLD_N // 1024) == 1026 and C.FOLD_N % 4 == 1
    for apply_m in _host_preconds(off, col, val).values():
        info = {}
        _, status, iterations, history, left = model.gmres(_host_product(off, col, val), apply_m, C.rhs(C.FOLD_N, NP[prec]), None, RTOL[prec], 0.0,
                                                           3, C.FOLD_ITERATIONS, info)
        assert (status, iterations, left, info["slots"], info["cycles"]) == (model.RUNNING, C.FOLD_ITERATIONS, None, 3, 1)
        assert np.isfinite(history).all() and (history > info["stop2"]).all()


def test_the_estimate_closes_a_cycle_whose_true_residual_misses():
    """fp32 at rtol = 3e-7: the rotations' estimate passes stop2, the true residual does not, and the next cycle runs"""
    prec = G.MISS["prec"]
    off, col, val = C.convection_diffusion(*G.MISS["grid"], NP[prec])
    b = C.rhs(len(off) - 1, NP[prec])
    info = {}
    x, status, iterations, history, left = model.gmres(_host_product(off, col, val), lambda r: r, b, None, G.MISS["rtol"], 0.0, G.MISS["restart"],
                                                       LIMIT, info)
    print(f"gmres model, early close: {iterations} iterations, {info['cycles']} cycles, {info['slots']} slots, {info['missed']} missed, {status}")
    assert info["missed"] >= 1 and iterations < info["slots"] <= LIMIT and info["cycles"] >= 2


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(G.EXIT_CASES))
def test_every_exit_is_taken_on_the_host(name, prec):
    a, b, restart, max_iterations, status, iterations, left = G.EXIT_CASES[name]
    a, b = np.asarray(a, NP[prec]), np.asarray(b, NP[prec])
    off, col, val = C.dense_csr(a, NP[prec])
    info = {}
    got = model.gmres(_host_product(off, col, val), lambda r: r, b, None, RTOL[prec], 0.0, restart, max_iterations, info)
    assert got[1:3] == (status, iterations) and got[4] == left == info["exit"] and got[3].size == iterations + 1, (got[1:], info)
    assert got[3][-1] == info["rr"] or np.isnan(info["rr"])
    if name.startswith("beta"):
        assert not _bits(got[0]).any() and not np.isfinite(got[3][0]) and not np.isfinite(info["beta"])
    if name == "d-first":
        assert not _bits(got[0]).any() and info["rr"] == 2 and (info["slots"], info["cycles"]) == (10, 1)      # x, r and rr stay
    if name == "d-second":
        assert info["rr"] == 1 and got[3][1] == 1
    if name == "none":
        assert (info["slots"], info["cycles"]) == (1, 1)                                                       # width 1 < restart
    if name == "stagnation":
        assert not _bits(got[0]).any() and (got[3] == 1).all() and (info["slots"], info["cycles"]) == (6, 6)
    if name in ("lucky", "stagnation-2"):
        assert _true_residual(off, col, val, got[0], b) <= RESIDUAL[prec]


def test_special_values_in_b_on_the_host():
    off, col, val = C.banded(1025, np.float64)
    for bad in (np.inf, -np.inf, np.nan):
        b = C.rhs(1025, np.float64)
        b[1000] = bad
        x, status, iterations, history, left = model.gmres(_host_product(off, col, val), lambda r: r, b, None, 1e-10, 0.0, 30, 10)
        assert (status, iterations, left) == (model.BREAKDOWN, 0, "beta") and not _bits(x).any() and not np.isfinite(history[0])
    b = C.rhs(1025, np.float64)
    b[::3] = -0.0
    x, status, iterations, _, _ = model.gmres(_host_product(off, col, val), lambda r: r, b, None, 1e-10, 0.0, 30, LIMIT)
    assert status == model.CONVERGED and _true_residual(off, col, val, x, b) <= RESIDUAL["f64"]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("restart,max_iterations", [(3, 12), (30, 12), (2, 5)])
def test_the_slow_loops_agree_with_the_vectorised_model(restart, max_iterations, prec):
    """the model's own check: plain loops over scalars, the reduction as pcg_model.reduce_loop"""
    off, col, val = C.banded(7, NP[prec])
    a = np.zeros((7, 7), NP[prec])
    a[C.rows_of(off), col] = val
    b = C.rhs(7, NP[prec])
    info = {}
    want = model.gmres(_host_product(*C.dense_csr(a, NP[prec])), lambda r: r, b, None, RTOL[prec], 0.0, restart, max_iterations, info)
    got = model.gmres_loop(a, b, RTOL[prec], 0.0, restart, max_iterations)
    assert got[1:3] == want[1:3] and got[4] == want[4] and got[5:] == (info["slots"], info["cycles"]) and want[2] > 2
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[3]), _bits(want[3]))


# ------------------------------------------------------------------------------------------------------------ the boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T mspmv_" in l)


def _next_to_the_product(name):
    return os.path.join(os.path.dirname(M.library_path("product")), name)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "include/mspmv_gmres.h"\n'
                   "int use(void) { mspmv_gmres_t *s = 0; mspmv_gmres_state_t st;\n"
                   "  int e = mspmv_gmres_create(&s, 0, 0, 0, 0, 8, MSPMV_GMRES_NONE, MSPMV_GMRES_MAX_RESTART, 0, 0);\n"
                   "  e |= mspmv_gmres_solve_f64(s, 0, 0, 0, 0, 0, 0, 1e-8, 0.0, 10, 0, 0, 0, 0); e |= mspmv_gmres_state(s, &st, 0);\n"
                   "  return e | mspmv_gmres_destroy(s) | (st.exit_test == MSPMV_GMRES_EXIT_D) | (st.slots + st.cycles) | MSPMV_PCG_CONVERGED; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "hdr.o"), "-I", ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_what_the_header_declares_and_nothing_else():
    functions = declared("mspmv_gmres.h")
    assert sorted(functions) == NEW
    gmres = _next_to_the_product("libmspmv_gmres.so")
    assert _exported(gmres) == NEW
    assert not set(_exported(M.library_path("product"))) & set(NEW)            # the product library exports none of them
    assert not set(declared("mspmv.h")) & set(NEW)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", gmres], capture_output=True, text=True, check=True).stdout
    needs = sorted(l.split()[-1] for l in undefined.splitlines() if " mspmv_" in l)
    assert needs and set(needs) <= set(declared("mspmv.h"))                     # it calls only what mspmv.h declares
    assert set(needs) <= {"mspmv_csrmv_prepare", "mspmv_csrmv_prepared_f32", "mspmv_csrmv_prepared_f64", "mspmv_csrsv_solve_f32",
                          "mspmv_csrsv_solve_f64", "mspmv_csrsv_plan_info"}
    # the other layer and its header are what they were
    assert sorted(declared("mspmv_krylov.h")) == KRYLOV and _exported(_next_to_the_product("libmspmv_krylov.so")) == KRYLOV


def test_the_prototypes_match_the_header():
    lib = GM.load_gmres_library()
    functions = declared("mspmv_gmres.h")
    assert mismatches(lib, functions) == []
    assert sorted(prototyped(lib)) == sorted(functions)
    assert functions["mspmv_gmres_solve_f32"][1][7:9] == ["double", "double"] and len(functions["mspmv_gmres_solve_f64"][1]) == 14
    assert functions["mspmv_gmres_create"][1] == ["pointer"] * 3 + ["i32"] * 5 + ["pointer", "i32"]
    # the table went on the new CDLL, never on the product's
    prev = M.active_library()
    try:
        M.use_library("product")
        product = M.load_library()
    finally:
        M.use_library(prev)
    assert lib is not product and not [n for n in prototyped(product) if "gmres" in n]
    # the state block as ctypes lays it out is the header's: ten int32, four doubles, one uint64
    assert ctypes.sizeof(GM._GmresState) == 10 * 4 + 4 * 8 + 8 and GM._GmresState.rr.offset == 40 and GM._GmresState.exit_test.offset == 36
    header = open(os.path.join(ROOT, "include", "mspmv_gmres.h")).read()
    body = header[header.index("typedef struct mspmv_gmres_state {"):header.index("} mspmv_gmres_state_t;")]
    import re
    fields = [name for line in body.splitlines()[1:] for name in re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", line))]
    assert fields == [name for name, _ in GM._GmresState._fields_]


def test_one_product_library_is_mapped_and_the_surface_is_unchanged():
    GM.load_gmres_library()
    with open("/proc/self/maps") as f:
        files = {line.split()[-1] for line in f if line.rstrip().endswith("/libmspmv.so")}
    assert len(files) == 1 and os.path.samefile(files.pop(), M.library_path("product"))
    assert M.__all__ == ALL
    assert M.Gmres is GM.Gmres and M.gmres is GM.gmres and M.GMRES_EXIT is GM.GMRES_EXIT
    assert M.GMRES_EXIT == model.EXITS and len(M.GMRES_EXIT) == 5
    assert M.load_library().mspmv_version() == 102


# ------------------------------------------------------------------------------------------------------------ refusals
def _create(rows, nnz, vb=8, kind=NONE, restart=30, off=4096, col=4096, out=True):
    """mspmv_gmres_create on fake device pointers (refusals come before anything is touched; rows == 0 touches nothing at all)"""
    lib = GM.load_gmres_library()
    handle = ctypes.c_void_p(0)
    st = lib.mspmv_gmres_create(ctypes.byref(handle) if out else None, ctypes.c_void_p(off) if off else None, ctypes.c_void_p(col) if col else None,
                                rows, nnz, vb, kind, restart, None, 0)
    return st, handle


def test_create_refuses_before_any_launch():
    assert _create(-1, 0)[0] == 1 and _create(5, -1)[0] == 1
    assert _create(2 ** 30, 2 ** 30)[0] == 1                                      # rows + nnz beyond the library's limit
    assert _create(2 ** 30 + 1, 0)[0] == 1                                        # rows beyond the reduction's
    assert _create(0, 5)[0] == 1
    assert _create(5, 5, vb=2)[0] == 1 and _create(5, 5, kind=3)[0] == 1 and _create(5, 5, kind=-1)[0] == 1
    assert _create(5, 5, restart=0)[0] == 1 and _create(5, 5, restart=-3)[0] == 1 and _create(5, 5, restart=129)[0] == 1
    assert _create(0, 0, restart=129, off=0, col=0)[0] == 1
    assert _create(5, 5, off=0)[0] == 1 and _create(5, 5, col=0)[0] == 1          # NULL arrays
    assert _create(0, 0, out=False)[0] == 1
    lib = GM.load_gmres_library()
    assert lib.mspmv_gmres_destroy(None) == 1 and lib.mspmv_gmres_state(None, None, None) == 1


def _solve(lib, handle, vb=8, rtol=1e-8, atol=0.0, max_iterations=10, check_every=0):
    fn = lib.mspmv_gmres_solve_f32 if vb == 4 else lib.mspmv_gmres_solve_f64
    return fn(handle, None, None, None, None, None, 0, rtol, atol, max_iterations, check_every, None, None, 0)


@pytest.mark.parametrize("kind", [NONE, JACOBI, FACTOR])
def test_no_rows_touch_no_device_and_solve_refusals(kind):
    lib, product = GM.load_gmres_library(), M.load_library()
    st, handle = _create(0, 0, vb=8, kind=kind, restart=128, off=0, col=0)
    assert st == 0 and handle.value
    state = GM._GmresState()
    assert lib.mspmv_gmres_state(handle, ctypes.byref(state), None) == 0
    assert (state.launches_per_iteration, state.launches_per_cycle, state.restart) == (7, 6 if kind == FACTOR else 5, 128)
    assert (state.precond_kind, state.bad_diagonal_row, state.exit_test, state.device_bytes) == (kind, -1, 0, 0)
    if kind == FACTOR:
        assert _solve(lib, handle) == 1                                           # FACTOR without set_factor
        assert lib.mspmv_gmres_set_factor(handle, None, None, None, None, None) == 1
        plans = []
        for uplo in (0, 1):
            plan = ctypes.c_void_p(0)
            assert product.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, uplo, 0, None, 0) == 0
            plans.append(plan)
        assert lib.mspmv_gmres_set_factor(handle, plans[0], None, None, None, None) == 1
        assert lib.mspmv_gmres_set_factor(handle, plans[0], plans[1], None, None, None) == 0
    else:
        plan = ctypes.c_void_p(0)
        assert product.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, 0, 0, None, 0) == 0
        assert lib.mspmv_gmres_set_factor(handle, plan, plan, None, None, None) == 1         # a handle of another kind
        plans = [plan]
    for bad in (dict(rtol=-1e-8), dict(rtol=float("nan")), dict(atol=-1.0), dict(atol=float("nan")), dict(max_iterations=-1),
                dict(check_every=-1), dict(vb=4)):
        assert _solve(lib, handle, **bad) == 1, bad
    assert lib.mspmv_gmres_solve_f64(None, None, None, None, None, None, 0, 1e-8, 0.0, 10, 0, None, None, 0) == 1
    for check_every in (0, 3):
        assert _solve(lib, handle, atol=0.5, check_every=check_every) == 0
        assert lib.mspmv_gmres_state(handle, ctypes.byref(state), None) == 0
        assert (state.status, state.iterations, state.slots, state.cycles, state.exit_test) == (1, 0, 0, 0, 1)     # CONVERGED (start)
        assert (state.rr, state.bb, state.stop2, state.beta) == (0.0, 0.0, 0.25, 0.0)
    assert lib.mspmv_gmres_destroy(handle) == 0
    for plan in plans:
        assert product.mspmv_csrsv_plan_destroy(plan) == 0
