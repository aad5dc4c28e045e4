"""mspmv_bicgstab_* (merge_spmv_amd.Bicgstab / bicgstab): BiCGStab on the device, compared ON THE BITS -- x, the iteration count, the
status, the exit, the whole history of rr and the scalars of the state block -- with tests/bicgstab_model.py, the numpy restatement of
the arithmetic that include/mspmv_krylov.h states.  The model's operators are the library's own, which have exact tests of theirs:
A p is M.csrmv on the device, M^-1 p is the identity, the model's division by the diagonal, or Ilu0.solve.  Everything else in the
model is numpy.  tests/test_bicgstab_model.py asserts the preconditions of the references on the CPU.  A NaN equals any NaN."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import merge_spmv_amd as M
import bicgstab_common as C
import bicgstab_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, TORCH, _bits, _true_residual

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

PRECONDS = ["none", "jacobi", "ilu0", "ilu0-multicolour"]
SCALARS = ("rr", "bb", "stop2", "rho", "alpha", "omega")
_grid_id = lambda g: "%dx%d" % g


def _same(got, want):
    """equal bits; a NaN equals any NaN (its sign and payload are not defined)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


@functools.lru_cache(maxsize=None)
def _matrix(key, prec):
    if key[0] == "grid":
        return C.convection_diffusion(key[1], key[2], NP[prec])
    if key[0] == "band":
        return C.banded(key[1], NP[prec])
    if key[0] == "exit":
        return C.dense_csr(C.EXIT_CASES[key[1]][0], NP[prec])
    assert key == ("fold",)
    return C.bidiagonal(C.FOLD_N, NP[prec])


class _System:
    """one matrix, one right-hand side, one preconditioner: the device arrays, the model's operators, the Bicgstab"""

    def __init__(self, matrix, prec, precond, b=None):
        dt = NP[prec]
        off, col, val = matrix
        n = self.n = len(off) - 1
        b = C.rhs(n, dt) if b is None else np.asarray(b, dt)
        d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
        self.coloring = self.ilu = None
        if precond == "ilu0-multicolour":
            self.coloring, p = M.multicolor_reorder(d_val, d_off, d_col)
            d_off, d_col, d_val = p.row_offsets, p.column_indices, p.values
            d_b = self.coloring.permute_vector(d_b)
            off, col, val, b = (t.cpu().numpy() for t in (d_off, d_col, d_val, d_b))
        self.off, self.col, self.val, self.b = off, col, val, b
        self.d_off, self.d_col, self.d_val, self.d_b = d_off, d_col, d_val, d_b
        self.prec, self.precond = prec, precond
        if precond == "none":
            m = None
        elif precond == "jacobi":
            m = "jacobi"
        else:
            self.ilu = M.Ilu0(d_off, d_col)
            assert int(self.ilu.factor(d_val).item()) == -1
            m = self.ilu
        self.solver = M.Bicgstab(d_off, d_col, TORCH[prec], preconditioner=m)

    def close(self):
        self.solver.close()
        for held in (self.ilu, self.coloring):
            if held is not None:
                held.close()

    def operators(self, d_val):
        apply_A = lambda p: M.csrmv(d_val, self.d_off, self.d_col, torch.from_numpy(p).cuda(), num_cols=self.n).cpu().numpy()
        if self.precond == "none":
            return apply_A, lambda r: r
        if self.precond == "jacobi":
            d = C.diagonal_of(self.off, self.col, d_val.cpu().numpy())
            return apply_A, lambda r: r / d
        return apply_A, lambda r: self.ilu.solve(torch.from_numpy(r).cuda()).cpu().numpy()

    def model(self, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, b=None, values=None):
        """((x, status, iterations, history, exit), info) of the model on the library's operators"""
        apply_A, apply_M = self.operators(self.d_val if values is None else values)
        info = {}
        b = self.b if b is None else np.asarray(b, NP[self.prec])
        return model.bicgstab(apply_A, apply_M, b, x0, RTOL[self.prec] if rtol is None else rtol, atol, max_iterations, info), info

    def solve(self, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, check_every=8, b=None, values=None, history=True, **kw):
        """((x, status, iterations, history[0 .. iterations] or None, exit), state) of the device"""
        x = None if x0 is None else torch.from_numpy(x0).cuda()
        x = self.solver.solve(self.d_val if values is None else values, self.d_b if b is None else torch.from_numpy(np.asarray(b, NP[self.prec])).cuda(),
                              x=x, rtol=RTOL[self.prec] if rtol is None else rtol, atol=atol, max_iterations=max_iterations,
                              check_every=check_every, history=history, **kw)
        state = self.solver.state                                      # (synchronises the device)
        kept = None if self.solver.history is None else self.solver.history.cpu().numpy()[:state["iterations"] + 1]
        return (x.cpu().numpy(), state["status"], state["iterations"], kept, state["exit"]), state


def _equal(got, want, state=None, info=None):
    (x, status, its, history, left), (mx, mstatus, mits, mhistory, mleft) = got, want
    assert (status, its, left) == (mstatus, mits, mleft)
    assert history is None or _same(history, mhistory)
    assert _same(x, mx)
    if state is not None:
        t = mx.dtype.type
        for name in SCALARS:
            assert _same(t(state[name]), info[name]), (name, state[name], info[name])
        assert state["launches_per_iteration"] == 9


@functools.lru_cache(maxsize=None)
def _system(key, prec, precond):
    return _System(_matrix(key, prec), prec, precond)


@functools.lru_cache(maxsize=None)
def _reference(key, prec, precond, guess=False, max_iterations=LIMIT):
    """the model's run, computed once and shared"""
    s = _system(key, prec, precond)
    return s.model(x0=C.guess(s.n, NP[prec]) if guess else None, max_iterations=max_iterations)


# ---------------------------------------------------------------------------------------------------------------- the grids
@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("grid", C.GRIDS, ids=_grid_id)
def test_on_the_bits_and_the_true_residual(grid, prec, precond):
    key = ("grid",) + grid
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    got, state = s.solve()
    print(f"bicgstab {grid} {prec} {precond}: {got[2]} iterations, {got[1]} ({got[4]}), true residual {_true_residual(s.off, s.col, s.val, got[0], s.b):.3e}")
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    _equal(got, want, state, info)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]
    assert state["rr"] <= state["stop2"] and state["bb"] == float(model.dot(s.b, s.b)) and state["precond_kind"] == min(PRECONDS.index(precond), 2)
    assert s.solver.launches_per_iteration == 9


@gpu
def test_ilu0_halves_the_iterations_on_the_40_x_25_grid():
    plain, ilu = _reference(("grid", 40, 25), "f64", "none")[0][2], _reference(("grid", 40, 25), "f64", "ilu0")[0][2]
    print(f"bicgstab: {ilu} iterations with ILU(0), {plain} without")
    assert 2 * ilu <= plain, (ilu, plain)


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
def test_a_guess_and_the_cut_offs(prec, precond):
    key = ("grid", 40, 25)
    s = _system(key, prec, precond)
    want, info = _reference(key, prec, precond, guess=True)
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    got, state = s.solve(x0=C.guess(s.n, NP[prec]))
    _equal(got, want, state, info)
    whole = _reference(key, prec, precond)[0]
    assert whole[2] > 7 or precond.startswith("ilu0")
    for cut in (0, 1, 7):
        want, info = _reference(key, prec, precond, max_iterations=cut)
        if whole[2] > cut:                                             # (ILU(0) in fp32 may be done by then: the cut-off then changes nothing)
            assert want[1:3] == (model.RUNNING, cut) and want[4] is None
        got, state = s.solve(max_iterations=cut)
        _equal(got, want, state, info)
        assert _same(got[3], whole[3][:cut + 1])


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0"])
@pytest.mark.parametrize("prec", PRECS)
def test_check_every_and_the_freeze(prec, precond):
    """the same bits however often the host looks; iterations enqueued well past the end change neither x nor the history beyond"""
    key = ("grid", 24, 24)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    limit = want[2] + 12
    for check_every in (0, 1, 3, 8):
        history = torch.full((limit + 1,), 7.0, dtype=TORCH[prec], device="cuda")
        got, state = s.solve(max_iterations=limit, check_every=check_every, history=history)
        _equal(got, want, state, info)
        tail = history.cpu().numpy()[want[2] + 1:]
        assert tail.size == 12 and (tail == 7.0).all()                # history beyond `iterations` is never written


# ---------------------------------------------------------------------------------------------------------------- every exit
@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(C.EXIT_CASES))
def test_every_exit_on_the_bits(name, prec):
    _, b, max_iterations, status, iterations, left = C.EXIT_CASES[name]
    s = _System(_matrix(("exit", name), prec), prec, "none", b=b)
    try:
        want, info = s.model(max_iterations=max_iterations)
        assert (want[1], want[2], want[4]) == (status, iterations, left), (want[1:3], info)
        for check_every in (8, 0):
            got, state = s.solve(max_iterations=max_iterations, check_every=check_every)
            _equal(got, want, state, info)
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_a_handle_solves_again_after_a_breakdown(prec):
    """one handle on the dense 2 x 2 pattern: the rv system breaks down; then the rr system gives the model's bits (a stale status,
    stale partials and a stale state block); then the rv system again"""
    s = _System(_matrix(("exit", "rv"), prec), prec, "none", b=C.EXIT_CASES["rv"][1])
    try:
        for name in ("rv", "rr", "tt", "rv"):
            values = torch.from_numpy(_matrix(("exit", name), prec)[2]).cuda()
            b = C.EXIT_CASES[name][1]
            want, info = s.model(values=values, b=b)
            assert (want[1], want[2], want[4]) == C.EXIT_CASES[name][3:]
            got, state = s.solve(values=values, b=b)
            _equal(got, want, state, info)
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("prec", PRECS)
def test_special_values_in_b(prec, precond):
    s = _system(("band", 1025), prec, precond)
    for bad in (np.inf, -np.inf, np.nan):
        b = s.b.copy()
        b[1000] = bad
        want, info = s.model(b=b, max_iterations=10)
        assert want[1] == model.BREAKDOWN, (bad, want[1:3], info)
        for check_every in (8, 0):
            got, state = s.solve(b=b, max_iterations=10, check_every=check_every)
            _equal(got, want, state, info)                             # (x by value, NaNs equal)
    b = s.b.copy()
    b[::3] = -0.0
    want, info = s.model(b=b)
    assert want[1] == model.CONVERGED
    got, state = s.solve(b=b)
    _equal(got, want, state, info)


# ---------------------------------------------------------------------------------------------------------------- index arithmetic
@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi", "ilu0"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", C.SIZES)
def test_every_size_on_the_bits(n, prec, precond):
    key = ("band", n)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    got, state = s.solve()
    _equal(got, want, state, info)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]


@gpu
@pytest.mark.parametrize("precond,guess", [("none", False), ("jacobi", False), ("jacobi", True)], ids=["none", "jacobi", "jacobi-guess"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_two_level_fold(prec, precond, guess):
    """n = 2^20 + 1029: the step kernel folds 1026 partials in two levels"""
    s = _system(("fold",), prec, precond)
    want, info = _reference(("fold",), prec, precond, guess=guess, max_iterations=C.FOLD_ITERATIONS)
    assert -(-s.n // 1024) == 1026 and s.n % 4 == 1
    assert want[1:3] == (model.RUNNING, C.FOLD_ITERATIONS) and want[3].size == C.FOLD_ITERATIONS + 1 and np.isfinite(want[3]).all()
    got, state = s.solve(x0=C.guess(s.n, NP[prec]) if guess else None, max_iterations=C.FOLD_ITERATIONS)
    _equal(got, want, state, info)


@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi", "ilu0"])
@pytest.mark.parametrize("prec", PRECS)
def test_b_and_x_one_element_behind_a_16_byte_boundary(prec, precond):
    """unaligned b and x take the element path; guard words around x and around the history"""
    key = ("band", 4160)
    s = _system(key, prec, precond)
    want, _ = _reference(key, prec, precond, guess=True)
    b = torch.full((s.n + 2,), 7.0, dtype=TORCH[prec], device="cuda")
    x = torch.full((s.n + 2,), 9.0, dtype=TORCH[prec], device="cuda")
    history = torch.full((LIMIT + 3,), 5.0, dtype=TORCH[prec], device="cuda")
    b[1:-1].copy_(s.d_b)
    x[1:-1].copy_(torch.from_numpy(C.guess(s.n, NP[prec])))
    assert b[1:-1].data_ptr() % 16 == b.element_size() and x[1:-1].data_ptr() % 16 == x.element_size()
    s.solver.solve(s.d_val, b[1:-1], x=x[1:-1], rtol=RTOL[prec], max_iterations=LIMIT, history=history[1:-1])
    state = s.solver.state
    assert (state["status"], state["iterations"], state["exit"]) == (want[1], want[2], want[4])
    hb, hx, hh = b.cpu().numpy(), x.cpu().numpy(), history.cpu().numpy()
    assert hb[0] == 7.0 and hb[-1] == 7.0 and hx[0] == 9.0 and hx[-1] == 9.0 and np.array_equal(_bits(hb[1:-1]), _bits(s.b))
    assert _same(hx[1:-1], want[0]) and _same(hh[1:want[2] + 2], want[3])
    assert hh[0] == 5.0 and (hh[want[2] + 2:] == 5.0).all()


# ---------------------------------------------------------------------------------------------------------------- plumbing
@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi", "ilu0"])
def test_launch_lines_number_the_launches(capfd, precond):
    """debug_synchronous prints one line per launch: the solver's own are those of bicgstab_*_kernel, 9 per iteration for every kind"""
    s = _system(("grid", 24, 24), "f64", precond)
    counts = {}
    for its in (2, 5):
        capfd.readouterr()
        s.solve(max_iterations=its, check_every=0, debug_synchronous=True)
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
        counts[its] = (sum(l.startswith("mspmv: bicgstab_") for l in lines), len(lines))
        assert s.solver.state["iterations"] == its
    per = s.solver.state["launches_per_iteration"]
    assert per == 9 and counts[5][0] - counts[2][0] == 3 * per, counts
    assert counts[2][0] == 2 + 2 * per, counts                          # init and the starting step
    others = 2 + (2 * (s.ilu.lower.info["launches"] + s.ilu.upper.info["launches"]) if precond == "ilu0" else 0)     # two products, four sweeps
    assert counts[5][1] - counts[2][1] >= 3 * (per + others), counts


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_solve_on_a_side_stream(prec, precond):
    key = ("grid", 40, 25)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for check_every, history in ((0, True), (3, True), (3, None)):
        got, state = s.solve(max_iterations=want[2] + 2, check_every=check_every, history=history, stream=side)
        assert (got[3] is None) == (history is None)
        _equal(got, want, state, info)


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_graph_capture_and_replay(prec, precond):
    """a solve that reads nothing back, captured and replayed twice onto a zeroed x: the eager solve's bits both times"""
    key = ("grid", 40, 25)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    limit = want[2] + 6
    x = torch.zeros(s.n, dtype=TORCH[prec], device="cuda")
    history = torch.zeros(limit + 1, dtype=TORCH[prec], device="cuda")
    s.solver.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)       # (warm-up, eager)
    torch.cuda.synchronize()
    assert _same(x.cpu().numpy(), want[0])
    graph = torch.cuda.CUDAGraph()
    x.zero_()
    with torch.cuda.graph(graph):
        s.solver.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)
    for _ in range(2):
        x.zero_(); history.fill_(3)
        graph.replay()
        state = s.solver.state
        assert (state["status"], state["iterations"], state["exit"]) == (want[1], want[2], want[4])
        assert _same(x.cpu().numpy(), want[0])
        assert _same(history.cpu().numpy()[:want[2] + 1], want[3]) and (history.cpu().numpy()[want[2] + 1:] == 3).all()


@gpu
def test_plans_of_other_rows_are_refused_and_the_tuple_form():
    s, other = _system(("grid", 24, 24), "f64", "ilu0"), _system(("grid", 40, 25), "f64", "ilu0")
    with pytest.raises(M.MspmvError, match="do not fit"):
        M.Bicgstab(s.d_off, s.d_col, torch.float64, preconditioner=(other.ilu.lower, other.ilu.upper, other.ilu.lu_values, other.d_off, other.d_col))
    lib = importlib.import_module("merge_spmv_amd.bicgstab").load_krylov_library()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mspmv_bicgstab_set_factor(s.solver._handle, other.ilu.lower._handle, other.ilu.upper._handle, ptr(other.ilu.lu_values),
                                         ptr(other.d_off), ptr(other.d_col)) == 1
    assert lib.mspmv_bicgstab_set_factor(s.solver._handle, s.ilu.lower._handle, other.ilu.upper._handle, ptr(s.ilu.lu_values), ptr(s.d_off),
                                         ptr(s.d_col)) == 1
    with pytest.raises(M.MspmvError, match="nothing is factorised"):
        M.Bicgstab(s.d_off, s.d_col, torch.float64, preconditioner=M.Ilu0(s.d_off, s.d_col))
    want, _ = _reference(("grid", 24, 24), "f64", "ilu0")
    solver = M.Bicgstab(s.d_off, s.d_col, torch.float64, preconditioner=(s.ilu.lower, s.ilu.upper, s.ilu.lu_values))
    x = solver.solve(s.d_val, s.d_b, rtol=RTOL["f64"], max_iterations=LIMIT)
    assert _same(x.cpu().numpy(), want[0]) and solver.state["iterations"] == want[2]
    solver.close()
    # Jacobi on a pattern that lacks a diagonal entry: the state names the row, the solve is refused
    off, col, val = _matrix(("band", 5), "f64")
    keep = np.ones(col.size, bool)
    keep[off[2] + list(col[off[2]:off[3]]).index(2)] = False
    off2 = off.copy(); off2[3:] -= 1
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off2, col[keep], val[keep]))
    solver = M.Bicgstab(d_off, d_col, torch.float64, preconditioner="jacobi")
    assert solver.state["bad_diagonal_row"] == 2
    with pytest.raises(M.MspmvError, match="mspmv_bicgstab_solve"):
        solver.solve(d_val, torch.ones(5, dtype=torch.float64, device="cuda"))
    solver.close()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_the_one_shot_call_answers_in_the_callers_numbering(prec):
    off, col, val = _matrix(("grid", 40, 25), prec)
    b = C.rhs(1000, NP[prec])
    d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
    seen = {}
    for kw in (dict(preconditioner="ilu0", reorder=True), dict(preconditioner="ilu0", reorder=False), dict(preconditioner="jacobi"),
               dict(preconditioner=None)):
        x, state = M.bicgstab(d_val, d_off, d_col, d_b, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True, **kw)
        assert state["status"] == "CONVERGED" and state["exit"] in ("half", "rr"), kw
        assert _true_residual(off, col, val, x.cpu().numpy(), b) <= RESIDUAL[prec], kw
        seen[(kw["preconditioner"], kw.get("reorder", True))] = (state["iterations"], x)
    # the permuted solve is the solve of the permuted system, mapped back: the bits of the multicolour case of this file
    s = _system(("grid", 40, 25), prec, "ilu0-multicolour")
    want = _reference(("grid", 40, 25), prec, "ilu0-multicolour")[0]
    assert seen[("ilu0", True)][0] == want[2]
    assert _same(seen[("ilu0", True)][1].cpu().numpy(), s.coloring.permute_vector(torch.from_numpy(want[0]).cuda(), back=True).cpu().numpy())
    natural = _reference(("grid", 40, 25), prec, "ilu0")[0]
    assert seen[("ilu0", False)][0] == natural[2] and _same(seen[("ilu0", False)][1].cpu().numpy(), natural[0])
    # a guess in the caller's numbering, the answer in the caller's tensor: starting from the answer ends at once
    x = seen[("ilu0", True)][1].clone()
    out, state = M.bicgstab(d_val, d_off, d_col, d_b, x=x, rtol=2 * RESIDUAL[prec], max_iterations=LIMIT, return_state=True)
    assert out is x and (state["status"], state["iterations"], state["exit"]) == ("CONVERGED", 0, "start")
