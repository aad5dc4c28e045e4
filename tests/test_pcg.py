"""mspmv_pcg_* (merge_spmv_amd.Pcg / pcg): conjugate gradients on the device, compared ON THE BITS -- x, the iteration count, the status
and the whole history of rr -- with tests/pcg_model.py, the numpy restatement of the arithmetic that include/mspmv.h states.  The model's
operators are the library's own, which have exact tests of theirs: A p is M.csrmv on the device, M^-1 r is the identity, the model's
division by the diagonal, or Ic0.solve.  Everything else in the model is numpy."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import pcg_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, TORCH, _bits, _host_product, _true_residual

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_pcg_create", "mspmv_pcg_set_factor", "mspmv_pcg_solve_f32", "mspmv_pcg_solve_f64", "mspmv_pcg_state", "mspmv_pcg_destroy"]
GRIDS = [(24, 24), (40, 25)]
PRECONDS = ["none", "jacobi", "ic0", "ic0-multicolour"]
NONE, JACOBI, FACTOR = 0, 1, 2


def _laplacian(w, h, dtype, diagonal=True):
    """the 5-point Laplacian of a w x h grid: rows sorted, 4 on the diagonal, -1 beside it"""
    rows = []
    for i in range(h):
        for j in range(w):
            me = i * w + j
            rows.append([c for c, ok in ((me - w, i > 0), (me - 1, j > 0), (me, diagonal), (me + 1, j < w - 1), (me + w, i < h - 1)) if ok])
    off = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=off[1:])
    col = np.asarray([c for r in rows for c in r], np.int32)
    r_of = np.repeat(np.arange(len(rows)), np.diff(off))
    return off, col, np.where(col == r_of, 4.0, -1.0).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_pcg_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\b%s\s*\(" % name, text) and f" T {name}\n" in out, (kind, name)


def _create(rows, nnz, vb=8, kind=NONE, off=4096, col=4096, out=True):
    """mspmv_pcg_create on fake device pointers (refusals come before anything is touched; rows == 0 touches nothing at all)"""
    lib = M.load_library()
    handle = ctypes.c_void_p(0)
    st = lib.mspmv_pcg_create(ctypes.byref(handle) if out else None, ctypes.c_void_p(off) if off else None, ctypes.c_void_p(col) if col else None,
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
    lib = M.load_library()
    assert lib.mspmv_pcg_destroy(None) == 1 and lib.mspmv_pcg_state(None, None, None) == 1


def _solve(lib, handle, vb=8, rtol=1e-8, atol=0.0, max_iterations=10, check_every=0):
    fn = lib.mspmv_pcg_solve_f32 if vb == 4 else lib.mspmv_pcg_solve_f64
    return fn(handle, None, None, None, None, None, 0, rtol, atol, max_iterations, check_every, None, None, 0)


@pytest.mark.parametrize("kind", [NONE, JACOBI, FACTOR])
def test_no_rows_touch_no_device_and_solve_refusals(kind):
    lib = M.load_library()
    st, handle = _create(0, 0, vb=8, kind=kind, off=0, col=0)
    assert st == 0 and handle.value
    state = M._PcgState()
    assert lib.mspmv_pcg_state(handle, ctypes.byref(state), None) == 0
    assert state.launches_per_iteration == (7 if kind == FACTOR else 5) and state.precond_kind == kind and state.bad_diagonal_row == -1
    if kind == FACTOR:
        assert _solve(lib, handle) == 1                                           # FACTOR without set_factor
        assert lib.mspmv_pcg_set_factor(handle, None, None, None, None, None) == 1
        plans = []
        for uplo in (0, 1):
            plan = ctypes.c_void_p(0)
            assert lib.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, uplo, 0, None, 0) == 0
            plans.append(plan)
        assert lib.mspmv_pcg_set_factor(handle, plans[0], None, None, None, None) == 1
        assert lib.mspmv_pcg_set_factor(handle, plans[0], plans[1], None, None, None) == 0
    else:
        plan = ctypes.c_void_p(0)
        assert lib.mspmv_csrsv_plan_create(ctypes.byref(plan), None, None, 0, 0, 0, 0, None, 0) == 0
        assert lib.mspmv_pcg_set_factor(handle, plan, plan, None, None, None) == 1          # a handle of another kind
        plans = [plan]
    for bad in (dict(rtol=-1e-8), dict(rtol=float("nan")), dict(atol=-1.0), dict(atol=float("nan")), dict(max_iterations=-1),
                dict(check_every=-1), dict(vb=4)):
        assert _solve(lib, handle, **bad) == 1, bad
    assert lib.mspmv_pcg_solve_f64(None, None, None, None, None, None, 0, 1e-8, 0.0, 10, 0, None, None, 0) == 1
    for check_every in (0, 3):
        assert _solve(lib, handle, atol=0.5, check_every=check_every) == 0
        assert lib.mspmv_pcg_state(handle, ctypes.byref(state), None) == 0
        assert (state.status, state.iterations, state.rr, state.bb, state.stop2) == (1, 0, 0.0, 0.0, 0.25)       # CONVERGED at 0
    assert lib.mspmv_pcg_destroy(handle) == 0
    for plan in plans:
        assert lib.mspmv_csrsv_plan_destroy(plan) == 0


def _dense(off, col, val):
    n = len(off) - 1
    a = np.zeros((n, n), val.dtype)
    a[np.repeat(np.arange(n), np.diff(off)), col] = val
    return a


def test_the_model_solves_a_small_grid():
    off, col, val = _laplacian(6, 6, np.float64)
    a = _dense(off, col, val)
    b = np.random.default_rng(3).uniform(-1, 1, 36)
    want = np.linalg.solve(a, b)
    for apply_m in (lambda r: r, lambda r: r / 4.0, lambda r: np.linalg.solve(np.tril(a) @ np.diag(1 / np.diag(a)) @ np.triu(a), r)):
        x, status, its, history = model.pcg(_host_product(off, col, val), apply_m, b, None, 1e-13, 0.0, 100)
        assert status == model.CONVERGED and 0 < its and history.size == its + 1
        assert np.linalg.norm(x - want) <= 1e-11 * np.linalg.norm(want)
        assert history[-1] <= (np.float64(1e-13) * np.float64(1e-13)) * model.dot(b, b) < history[-2]
    # a guess, a cut-off, a breakdown, a zero right-hand side
    x, status, its, _ = model.pcg(_host_product(off, col, val), lambda r: r, b, want + 1e-3, 1e-13, 0.0, 100)
    assert status == model.CONVERGED and np.linalg.norm(x - want) <= 1e-11 * np.linalg.norm(want)
    assert model.pcg(_host_product(off, col, val), lambda r: r, b, None, 1e-13, 0.0, 5)[1:3] == (model.RUNNING, 5)
    x, status, its, history = model.pcg(_host_product(off, col, -val), lambda r: r, b, None, 1e-13, 0.0, 100)
    assert (status, its, history.size) == (model.BREAKDOWN, 0, 1) and not x.any()
    x, status, its, _ = model.pcg(_host_product(off, col, val), lambda r: r, np.zeros(36), None, 1e-13, 0.0, 100)
    assert (status, its) == (model.CONVERGED, 0) and not np.signbit(x).any()


def test_the_model_keeps_the_fp32_bound_on_the_24_x_24_grid():
    """rtol 1e-5 by the recurrence leaves the true residual inside 1e-4 |b| in fp32 (the bound the GPU test asserts)"""
    off, col, val = _laplacian(24, 24, np.float32)
    b = np.random.default_rng(22).uniform(-1, 1, 576).astype(np.float32)
    for apply_m in (lambda r: r, lambda r: r / np.float32(4)):
        x, status, its, _ = model.pcg(_host_product(off, col, val), apply_m, b, None, RTOL["f32"], 0.0, LIMIT)
        assert status == model.CONVERGED and x.dtype == np.float32
        assert _true_residual(off, col, val, x, b) <= RESIDUAL["f32"]


# ---------------------------------------------------------------------------------------------------------------- GPU
class _System:
    """one matrix, one right-hand side, one preconditioner: the device arrays, the model's operators, the Pcg"""

    def __init__(self, grid, prec, precond, negate=False, diagonal=True):
        dt = NP[prec]
        off, col, val = _laplacian(grid[0], grid[1], dt, diagonal)
        if negate:
            val = -val
        n = self.n = len(off) - 1
        b = np.random.default_rng(22).uniform(-1, 1, n).astype(dt)
        d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
        self.coloring = None
        if precond == "ic0-multicolour":
            self.coloring, p = M.multicolor_reorder(d_val, d_off, d_col)
            d_off, d_col, d_val = p.row_offsets, p.column_indices, p.values
            d_b = self.coloring.permute_vector(d_b)
            off, col, val, b = (t.cpu().numpy() for t in (d_off, d_col, d_val, d_b))
        self.off, self.col, self.val, self.b = off, col, val, b
        self.d_off, self.d_col, self.d_val, self.d_b = d_off, d_col, d_val, d_b
        self.apply_A = lambda p: M.csrmv(d_val, d_off, d_col, torch.from_numpy(p).cuda(), num_cols=n).cpu().numpy()
        self.ic = None
        if precond == "none":
            self.apply_M, m = (lambda r: r), None
        elif precond == "jacobi":
            r_of = np.repeat(np.arange(n), np.diff(off))
            d = np.ones(n, dt)
            d[r_of[col == r_of]] = val[col == r_of]
            self.apply_M, m = (lambda r: r / d), "jacobi"
        else:
            self.ic = M.Ic0(d_off, d_col)
            assert int(self.ic.factor(d_val).item()) == -1
            self.apply_M, m = (lambda r: self.ic.solve(torch.from_numpy(r).cuda()).cpu().numpy()), self.ic
        self.pcg = M.Pcg(d_off, d_col, TORCH[prec], preconditioner=m)
        self.prec = prec

    def model(self, x0=None, rtol=None, max_iterations=LIMIT):
        return model.pcg(self.apply_A, self.apply_M, self.b, x0, RTOL[self.prec] if rtol is None else rtol, 0.0, max_iterations)

    def solve(self, x0=None, rtol=None, max_iterations=LIMIT, check_every=8, b=None, **kw):
        """(x, status, iterations, history[0 .. iterations]) of the device"""
        x = None if x0 is None else torch.from_numpy(x0).cuda()
        x = self.pcg.solve(self.d_val, self.d_b if b is None else b, x=x, rtol=RTOL[self.prec] if rtol is None else rtol, max_iterations=max_iterations,
                           check_every=check_every, history=True, **kw)
        state = self.pcg.state
        return x.cpu().numpy(), state["status"], state["iterations"], self.pcg.history.cpu().numpy()[:state["iterations"] + 1]


@functools.lru_cache(maxsize=None)
def _system(grid, prec, precond):
    return _System(grid, prec, precond)


@functools.lru_cache(maxsize=None)
def _reference(grid, prec, precond):
    """the model's run to convergence, computed once and shared"""
    return _system(grid, prec, precond).model()


def _equal(got, want):
    (x, status, its, history), (mx, mstatus, mits, mhistory) = got, want
    assert (status, its) == (mstatus, mits)
    assert history.dtype == mhistory.dtype and np.array_equal(_bits(history), _bits(mhistory))
    assert x.dtype == mx.dtype and np.array_equal(_bits(x), _bits(mx))


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("grid", GRIDS, ids=["24x24", "40x25"])
def test_on_the_bits_and_the_true_residual(grid, prec, precond):
    s, want = _system(grid, prec, precond), _reference(grid, prec, precond)
    got = s.solve()
    print(f"pcg {grid} {prec} {precond}: {got[2]} iterations, status {got[1]}, true residual {_true_residual(s.off, s.col, s.val, got[0], s.b):.3e}")
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    _equal(got, want)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]
    state = s.pcg.state
    assert state["launches_per_iteration"] == s.pcg.launches_per_iteration == (7 if precond.startswith("ic0") else 5)
    assert state["rr"] == float(want[3][-1]) and state["rr"] <= state["stop2"] and state["bb"] == float(model.dot(s.b, s.b))


@gpu
def test_ic0_halves_the_iterations_on_the_24_x_24_grid():
    plain, ic = _reference((24, 24), "f64", "none")[2], _reference((24, 24), "f64", "ic0")[2]
    print(f"pcg: {ic} iterations with IC(0), {plain} without")
    assert 2 * ic <= plain, (ic, plain)


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
def test_a_guess_and_a_cut_off(prec, precond):
    s = _system((40, 25), prec, precond)
    x0 = np.random.default_rng(5).uniform(-1, 1, s.n).astype(NP[prec])
    want = s.model(x0=x0)
    assert want[1] == model.CONVERGED
    _equal(s.solve(x0=x0), want)
    cut = s.solve(max_iterations=5)
    assert cut[1:3] == ("RUNNING", 5)
    _equal(cut, s.model(max_iterations=5))
    assert np.array_equal(_bits(cut[3]), _bits(_reference((40, 25), prec, precond)[3][:6]))


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ic0"])
@pytest.mark.parametrize("prec", PRECS)
def test_check_every_and_the_freeze(prec, precond):
    """the same x, iterations and history however often the host looks; iterations enqueued past the end change nothing"""
    s, want = _system((24, 24), prec, precond), _reference((24, 24), prec, precond)
    limit = 3 * want[2]
    for check_every in (0, 1, 7, limit):
        got = s.solve(max_iterations=limit, check_every=check_every)
        _equal(got, want)
        tail = s.pcg.history.cpu().numpy()[want[2] + 1:]
        assert tail.size == limit - want[2] and not tail.any()                  # history beyond `iterations` is never written


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_unaligned_right_hand_side_and_solution(prec):
    s, want = _system((40, 25), prec, "jacobi"), _reference((40, 25), prec, "jacobi")
    bb, xb = torch.zeros(s.n + 1, dtype=TORCH[prec], device="cuda"), torch.full((s.n + 2,), 9.0, dtype=TORCH[prec], device="cuda")
    bb[1:].copy_(s.d_b)
    x = s.pcg.solve(s.d_val, bb[1:], x=None, rtol=RTOL[prec], max_iterations=LIMIT, history=True)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[0]))
    # a guess (here zeros) in an unaligned x with guard words on both sides
    xb[1:-1] = 0
    assert xb[1:-1].data_ptr() % 16 == xb.element_size()
    s.pcg.solve(s.d_val, bb[1:], x=xb[1:-1], rtol=RTOL[prec], max_iterations=LIMIT)
    h = xb.cpu().numpy()
    assert h[0] == 9.0 and h[-1] == 9.0 and s.pcg.state["iterations"] == want[2]
    assert np.array_equal(_bits(h[1:-1]), _bits(want[0]))                       # (x = +0 and r = b - A 0 = b: the same bits)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_breakdown_and_edge_inputs(prec):
    # -A is negative definite: p.q < 0 in the first iteration -> BREAKDOWN, nothing of it written
    s = _System((24, 24), prec, "none", negate=True)
    x, status, its, history = s.solve()
    assert (status, its, history.size) == ("BREAKDOWN", 0, 1) and not _bits(x).any()
    _equal((x, status, its, history), s.model())
    x0 = np.random.default_rng(6).uniform(-1, 1, s.n).astype(NP[prec])
    x, status, its, _ = s.solve(x0=x0, check_every=0, max_iterations=9)
    assert (status, its) == ("BREAKDOWN", 0) and np.array_equal(_bits(x), _bits(x0)) and np.isfinite(x).all()
    # b = 0: CONVERGED before the first iteration, x = +0
    for precond in ("none", "jacobi", "ic0"):
        s = _system((24, 24), prec, precond)
        x, status, its, history = s.solve(b=torch.zeros_like(s.d_b))
        assert (status, its) == ("CONVERGED", 0) and not _bits(x).any() and not _bits(history).any()
    # Jacobi on a pattern that lacks a diagonal entry: the state names the row, the solve is refused
    off, col, val = _laplacian(24, 24, NP[prec])
    keep = np.ones(col.size, bool)
    keep[off[5] + list(col[off[5]:off[6]]).index(5)] = False
    off2 = off.copy(); off2[6:] -= 1
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off2, col[keep], val[keep]))
    solver = M.Pcg(d_off, d_col, TORCH[prec], preconditioner="jacobi")
    assert solver.state["bad_diagonal_row"] == 5
    with pytest.raises(M.MspmvError, match="mspmv_pcg_solve"):
        solver.solve(d_val, s.d_b)
    solver.close()
    assert M.Pcg(d_off, d_col, TORCH[prec]).state["bad_diagonal_row"] == -1


@gpu
def test_plans_of_other_rows_are_refused():
    s = _system((24, 24), "f64", "ic0")
    other = _system((40, 25), "f64", "ic0")
    lib = M.load_library()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mspmv_pcg_set_factor(s.pcg._handle, other.ic.lower._handle, other.ic.upper._handle, ptr(other.ic.l_values), ptr(other.d_off),
                                    ptr(other.d_col)) == 1
    assert lib.mspmv_pcg_set_factor(s.pcg._handle, s.ic.lower._handle, other.ic.upper._handle, ptr(s.ic.l_values), ptr(s.d_off), ptr(s.d_col)) == 1
    with pytest.raises(M.MspmvError, match="do not fit"):
        M.Pcg(s.d_off, s.d_col, torch.float64, preconditioner=(other.ic.lower, other.ic.upper, other.ic.l_values, other.d_off, other.d_col))
    with pytest.raises(M.MspmvError, match="nothing is factorised"):
        M.Pcg(s.d_off, s.d_col, torch.float64, preconditioner=M.Ic0(s.d_off, s.d_col))
    # the sweeps given one by one: symmetric Gauss-Seidel on A itself, M = (D + L) D^-1 (D + U), is not what two plain sweeps give, but
    # the tuple form with the Ic0's own plans and factor is the Ic0 form
    want = _reference((24, 24), "f64", "ic0")
    solver = M.Pcg(s.d_off, s.d_col, torch.float64, preconditioner=(s.ic.lower, s.ic.upper, s.ic.l_values))
    x = solver.solve(s.d_val, s.d_b, rtol=RTOL["f64"], max_iterations=LIMIT)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[0])) and solver.state["iterations"] == want[2]
    solver.close()


@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi", "ic0"])
def test_launch_lines_number_the_launches(capfd, precond):
    """debug_synchronous prints one line per launch: the solver's own are those of pcg_*_kernel, launches_per_iteration per iteration"""
    s = _system((24, 24), "f64", precond)
    counts = {}
    for its in (2, 5):
        capfd.readouterr()
        s.solve(max_iterations=its, check_every=0, debug_synchronous=True)
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
        counts[its] = (sum(l.startswith("mspmv: pcg_") for l in lines), len(lines))
        assert s.pcg.state["iterations"] == its
    per = s.pcg.state["launches_per_iteration"]
    assert counts[5][0] - counts[2][0] == 3 * per, counts
    start = {"none": 3, "jacobi": 3, "ic0": 5}[precond]                         # init, the starting step, (r.z and its step,) p = z
    assert counts[2][0] == start + 2 * per, counts
    others = 1 + (s.ic.lower.info["launches"] + s.ic.upper.info["launches"] if precond == "ic0" else 0)       # the product, the sweeps
    assert counts[5][1] - counts[2][1] >= 3 * (per + others), counts


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ic0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_graph_capture_and_replay(prec, precond):
    """a solve that reads nothing back, captured and replayed twice onto a zeroed x: the eager solve's bits both times"""
    s, want = _system((40, 25), prec, precond), _reference((40, 25), prec, precond)
    limit = want[2] + 6
    x = torch.zeros(s.n, dtype=TORCH[prec], device="cuda")
    history = torch.zeros(limit + 1, dtype=TORCH[prec], device="cuda")
    s.pcg.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)       # (warm-up, eager)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[0]))
    graph = torch.cuda.CUDAGraph()
    x.zero_()
    with torch.cuda.graph(graph):
        s.pcg.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)
    for _ in range(2):
        x.zero_(); history.fill_(3)
        graph.replay()
        state = s.pcg.state
        assert (state["status"], state["iterations"]) == (want[1], want[2])
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[0]))
        assert np.array_equal(_bits(history.cpu().numpy()[:want[2] + 1]), _bits(want[3])) and (history.cpu().numpy()[want[2] + 1:] == 3).all()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_the_one_shot_call_answers_in_the_callers_numbering(prec):
    off, col, val = _laplacian(40, 25, NP[prec])
    b = np.random.default_rng(22).uniform(-1, 1, 1000).astype(NP[prec])
    d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
    seen = {}
    for kw in (dict(preconditioner="ic0", reorder=True), dict(preconditioner="ic0", reorder=False), dict(preconditioner="jacobi"),
               dict(preconditioner=None)):
        x, state = M.pcg(d_val, d_off, d_col, d_b, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True, **kw)
        assert state["status"] == "CONVERGED", kw
        assert _true_residual(off, col, val, x.cpu().numpy(), b) <= RESIDUAL[prec], kw
        seen[(kw["preconditioner"], kw.get("reorder", True))] = (state["iterations"], x)
    # the permuted solve is the solve of the permuted system: the iteration count of the multicolour case of this file
    assert seen[("ic0", True)][0] == _reference((40, 25), prec, "ic0-multicolour")[2]
    assert seen[("ic0", False)][0] == _reference((40, 25), prec, "ic0")[2]
    # a guess in the caller's numbering: starting from the answer ends at once
    x, state = M.pcg(d_val, d_off, d_col, d_b, x=seen[("ic0", True)][1].clone(), rtol=2 * RESIDUAL[prec], max_iterations=LIMIT, return_state=True)
    assert (state["status"], state["iterations"]) == ("CONVERGED", 0)
