"""mspmv_gmres_* (merge_spmv_amd.Gmres / gmres): restarted GMRES(m) on the device, compared ON THE BITS -- x, the iteration count, the
slots, the cycles, the status, the exit, the whole history and the scalars of the state block -- with tests/gmres_model.py, the numpy
restatement of the arithmetic that include/mspmv_gmres.h states.  The model's operators are the library's own, which have exact tests
of theirs: A p is M.csrmv on the device, M^-1 p is the identity, the model's division by the diagonal, or Ilu0.solve.  Everything else
in the model is numpy.  tests/test_gmres_model.py asserts the preconditions of the references on the CPU.  A NaN equals any NaN."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import merge_spmv_amd as M
import bicgstab_common as C
import gmres_common as G
import gmres_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, TORCH, _bits, _true_residual

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

PRECONDS = ["none", "jacobi", "ilu0", "ilu0-multicolour"]
SCALARS = ("rr", "bb", "stop2", "beta")
COUNTS = ("slots", "cycles")
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
        return C.dense_csr(G.EXIT_CASES[key[1]][0], NP[prec])
    assert key == ("fold",)
    return C.bidiagonal(C.FOLD_N, NP[prec])


class _System:
    """one matrix, one right-hand side, one preconditioner: the device arrays, the model's operators, a Gmres per restart length"""

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
            self.m = None
        elif precond == "jacobi":
            self.m = "jacobi"
        else:
            self.ilu = M.Ilu0(d_off, d_col)
            assert int(self.ilu.factor(d_val).item()) == -1
            self.m = self.ilu
        self.solvers = {}

    def solver(self, restart=30):
        if restart not in self.solvers:
            self.solvers[restart] = M.Gmres(self.d_off, self.d_col, TORCH[self.prec], preconditioner=self.m, restart=restart)
        return self.solvers[restart]

    def close(self):
        for held in list(self.solvers.values()) + [self.ilu, self.coloring]:
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

    def model(self, restart=30, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, b=None, values=None):
        """((x, status, iterations, history, exit), info) of the model on the library's operators"""
        apply_A, apply_M = self.operators(self.d_val if values is None else values)
        info = {}
        b = self.b if b is None else np.asarray(b, NP[self.prec])
        return model.gmres(apply_A, apply_M, b, x0, RTOL[self.prec] if rtol is None else rtol, atol, restart, max_iterations, info), info

    def solve(self, restart=30, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, check_every=8, b=None, values=None, history=True, **kw):
        """((x, status, iterations, history[0 .. iterations] or None, exit), state) of the device"""
        solver = self.solver(restart)
        x = None if x0 is None else torch.from_numpy(x0).cuda()
        x = solver.solve(self.d_val if values is None else values, self.d_b if b is None else torch.from_numpy(np.asarray(b, NP[self.prec])).cuda(),
                         x=x, rtol=RTOL[self.prec] if rtol is None else rtol, atol=atol, max_iterations=max_iterations,
                         check_every=check_every, history=history, **kw)
        state = solver.state                                           # (synchronises the device)
        kept = None if solver.history is None else solver.history.cpu().numpy()[:state["iterations"] + 1]
        return (x.cpu().numpy(), state["status"], state["iterations"], kept, state["exit"]), state


def _equal(got, want, state=None, info=None):
    (x, status, its, history, left), (mx, mstatus, mits, mhistory, mleft) = got, want
    assert (status, its, left) == (mstatus, mits, mleft), (got[1:3], got[4], want[1:3], want[4], info)
    assert history is None or _same(history, mhistory)
    assert _same(x, mx)
    if state is not None:
        t = mx.dtype.type
        for name in COUNTS:
            assert state[name] == info[name], (name, state[name], info[name])
        for name in SCALARS:
            assert _same(t(state[name]), info[name]), (name, state[name], info[name])
        assert state["launches_per_iteration"] == 7 and state["iterations"] <= state["slots"]
        assert history is None or _same(t(state["rr"]), history[-1])    # history[iterations] is state.rr


@functools.lru_cache(maxsize=None)
def _system(key, prec, precond):
    return _System(_matrix(key, prec), prec, precond)


@functools.lru_cache(maxsize=None)
def _reference(key, prec, precond, restart=30, guess=False, max_iterations=LIMIT, rtol=None, atol=0.0):
    """the model's run, computed once and shared"""
    s = _system(key, prec, precond)
    return s.model(restart=restart, x0=C.guess(s.n, NP[prec]) if guess else None, max_iterations=max_iterations, rtol=rtol, atol=atol)


# ---------------------------------------------------------------------------------------------------------------- the grids
@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("grid", C.GRIDS, ids=_grid_id)
def test_on_the_bits_and_the_true_residual(grid, prec, precond):
    key = ("grid",) + grid
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    got, state = s.solve()
    print(f"gmres(30) {grid} {prec} {precond}: {got[2]} iterations in {state['cycles']} cycles and {state['slots']} slots, {got[1]} ({got[4]}), "
          f"true residual {_true_residual(s.off, s.col, s.val, got[0], s.b):.3e}")
    assert want[1] == model.CONVERGED and want[4] == "rr" and 0 < want[2] < LIMIT
    _equal(got, want, state, info)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]
    assert state["rr"] <= state["stop2"] and state["bb"] == float(model.dot(s.b, s.b)) and state["precond_kind"] == min(PRECONDS.index(precond), 2)
    assert state["restart"] == 30 and state["launches_per_cycle"] == (6 if precond.startswith("ilu0") else 5)
    assert s.solver().launches_per_iteration == 7 and state["device_bytes"] > 31 * s.n * got[0].itemsize


@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("restart", [1, 2, 5, 64, 128])
def test_every_restart_length(restart, prec, precond):
    """one column per cycle, the rotation chain, a cycle longer than the solve, the cap"""
    key = ("grid", 24, 24)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond, restart=restart)
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT, (want[1:3], info)
    assert restart < 64 or info["cycles"] <= 2
    got, state = s.solve(restart=restart)
    _equal(got, want, state, info)
    assert state["restart"] == restart and _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]


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
    for cut in (0, 1, 7, 37):                                          # 37: the second cycle is 7 slots wide
        want, info = _reference(key, prec, precond, max_iterations=cut)
        if whole[2] > cut:
            assert want[1] == model.RUNNING and want[4] is None and info["slots"] == cut and info["cycles"] == -(-cut // 30)
        got, state = s.solve(max_iterations=cut)
        _equal(got, want, state, info)
    want, info = _reference(key, prec, precond, max_iterations=0)
    assert (want[2], info["slots"], info["cycles"]) == (0, 0, 0) and not _bits(want[0]).any()


@gpu
@pytest.mark.parametrize("precond", ["none", "ilu0"])
@pytest.mark.parametrize("prec", PRECS)
def test_atol(prec, precond):
    """atol decides where rtol = 0: stop2 = atol^2"""
    key = ("grid", 24, 24)
    s = _system(key, prec, precond)
    atol = {"f32": 1e-3, "f64": 1e-7}[prec]
    want, info = _reference(key, prec, precond, rtol=0.0, atol=atol)
    t = NP[prec]
    assert want[1] == model.CONVERGED and _same(info["stop2"], t(atol) * t(atol)) and info["rr"] <= info["stop2"]
    got, state = s.solve(rtol=0.0, atol=atol)
    _equal(got, want, state, info)


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("restart", [5, 30])
def test_check_every_and_the_freeze(restart, prec, precond):
    """the same bits however often the host looks; slots enqueued well past the end change neither x, nor the words around it, nor
    the history beyond `iterations`"""
    key = ("grid", 24, 24)
    s = _system(key, prec, precond)
    limit = _reference(key, prec, precond, restart=restart)[1]["slots"] + 2 * restart + 3
    want, info = _reference(key, prec, precond, restart=restart, max_iterations=limit)
    assert want[1] == model.CONVERGED and info["slots"] + 2 * restart < limit
    for check_every in (0, 1, 7, restart):
        history = torch.full((limit + 1,), 7.0, dtype=TORCH[prec], device="cuda")
        x = torch.full((s.n + 8,), 9.0, dtype=TORCH[prec], device="cuda")
        s.solver(restart).solve(s.d_val, s.d_b, x=None, rtol=RTOL[prec], max_iterations=limit, check_every=check_every, history=history)
        first = s.solver(restart).state
        x[4:-4].zero_()
        s.solver(restart).solve(s.d_val, s.d_b, x=x[4:-4], rtol=RTOL[prec], max_iterations=limit, check_every=check_every, history=history)
        state = s.solver(restart).state
        hx, hh = x.cpu().numpy(), history.cpu().numpy()
        _equal((hx[4:-4], state["status"], state["iterations"], hh[:want[2] + 1], state["exit"]), want, state, info)
        assert first["iterations"] == want[2] and (hx[:4] == 9.0).all() and (hx[-4:] == 9.0).all()
        tail = hh[want[2] + 1:]
        assert tail.size == limit - want[2] and (tail == 7.0).all()   # history beyond `iterations` is never written


@gpu
def test_the_estimate_closes_a_cycle_whose_true_residual_misses():
    """fp32 at rtol = 3e-7: the estimate passes stop2, the true residual does not; the slots the cycle forfeits are counted, the next
    cycle runs, and the solve ends on a true residual"""
    key, prec = ("grid",) + G.MISS["grid"], G.MISS["prec"]
    s = _system(key, prec, "none")
    want, info = _reference(key, prec, "none", restart=G.MISS["restart"], rtol=G.MISS["rtol"])
    print(f"gmres, early close: {want[2]} iterations, {info['cycles']} cycles, {info['slots']} slots, {info['missed']} missed, {want[1]}")
    assert info["missed"] >= 1 and want[2] < info["slots"] and info["cycles"] >= 2
    for check_every in (0, 1, 30):
        got, state = s.solve(restart=G.MISS["restart"], rtol=G.MISS["rtol"], check_every=check_every)
        _equal(got, want, state, info)


# ---------------------------------------------------------------------------------------------------------------- every exit
@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(G.EXIT_CASES))
def test_every_exit_on_the_bits(name, prec):
    _, b, restart, max_iterations, status, iterations, left = G.EXIT_CASES[name]
    s = _System(_matrix(("exit", name), prec), prec, "none", b=b)
    try:
        want, info = s.model(restart=restart, max_iterations=max_iterations)
        assert (want[1], want[2], want[4]) == (status, iterations, left), (want[1:3], info)
        for check_every in (8, 1, 0):
            got, state = s.solve(restart=restart, max_iterations=max_iterations, check_every=check_every)
            _equal(got, want, state, info)
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_a_handle_solves_again_after_a_breakdown(prec):
    """one handle on the dense 2 x 2 pattern: a (d) breakdown with a column pending; then a solve that converges gives the model's bits (a
    stale status, stale flags, stale partials and rotations); then the breakdowns again"""
    s = _System(_matrix(("exit", "d-second"), prec), prec, "none", b=G.EXIT_CASES["d-second"][1])
    try:
        for name in ("d-second", "lucky", "d-first", "stagnation-2", "beta-nan", "lucky", "d-second"):
            values = torch.from_numpy(_matrix(("exit", name), prec)[2]).cuda()
            b = G.EXIT_CASES[name][1]
            want, info = s.model(values=values, b=b, max_iterations=10)
            if name != "stagnation-2":
                assert (want[1], want[2], want[4]) == G.EXIT_CASES[name][4:]
            got, state = s.solve(values=values, b=b, max_iterations=10)
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
        assert (want[1], want[2], want[4]) == (model.BREAKDOWN, 0, "beta"), (bad, want[1:3], info)
        for check_every in (8, 0):
            got, state = s.solve(b=b, max_iterations=10, check_every=check_every)
            _equal(got, want, state, info)
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
    """one lane, a lane across n, several workgroups, a partly empty last chunk; restart = 30 > n at the small sizes"""
    key = ("band", n)
    s = _system(key, prec, precond)
    for restart in G.BAND_RESTARTS:
        want, info = _reference(key, prec, precond, restart=restart)
        assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
        got, state = s.solve(restart=restart)
        _equal(got, want, state, info)
        assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]


@gpu
@pytest.mark.parametrize("precond,guess", [("none", False), ("jacobi", False), ("jacobi", True)], ids=["none", "jacobi", "jacobi-guess"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_two_level_fold(prec, precond, guess):
    """n = 2^20 + 1029: every fold of the step kernel takes 1026 partials in two levels"""
    s = _system(("fold",), prec, precond)
    want, info = _reference(("fold",), prec, precond, restart=3, guess=guess, max_iterations=C.FOLD_ITERATIONS)
    assert -(-s.n // 1024) == 1026 and s.n % 4 == 1
    assert want[1:3] == (model.RUNNING, C.FOLD_ITERATIONS) and want[3].size == C.FOLD_ITERATIONS + 1 and np.isfinite(want[3]).all()
    got, state = s.solve(restart=3, x0=C.guess(s.n, NP[prec]) if guess else None, max_iterations=C.FOLD_ITERATIONS)
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
    s.solver().solve(s.d_val, b[1:-1], x=x[1:-1], rtol=RTOL[prec], max_iterations=LIMIT, history=history[1:-1])
    state = s.solver().state
    assert (state["status"], state["iterations"], state["exit"]) == (want[1], want[2], want[4])
    hb, hx, hh = b.cpu().numpy(), x.cpu().numpy(), history.cpu().numpy()
    assert hb[0] == 7.0 and hb[-1] == 7.0 and hx[0] == 9.0 and hx[-1] == 9.0 and np.array_equal(_bits(hb[1:-1]), _bits(s.b))
    assert _same(hx[1:-1], want[0]) and _same(hh[1:want[2] + 2], want[3])
    assert hh[0] == 5.0 and (hh[want[2] + 2:] == 5.0).all()


# ---------------------------------------------------------------------------------------------------------------- plumbing
@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi", "ilu0"])
def test_launch_lines_number_the_launches(capfd, precond):
    """debug_synchronous prints one line per launch: the solver's own are those of gmres_*_kernel -- two at the start,
    launches_per_iteration for every slot and launches_per_cycle for every cycle of ceil(max_iterations / restart), for every kind"""
    s = _system(("grid", 24, 24), "f64", precond)
    counts = {}
    for its in (2, 5, 8):                                              # restart = 3: one, two and three cycles
        capfd.readouterr()
        s.solve(restart=3, max_iterations=its, check_every=0, debug_synchronous=True)
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
        counts[its] = (sum(l.startswith("mspmv: gmres_") for l in lines), len(lines))
        state = s.solver(3).state
        assert (state["iterations"], state["slots"], state["cycles"], state["status"]) == (its, its, -(-its // 3), "RUNNING")
    per, cycle = state["launches_per_iteration"], state["launches_per_cycle"]
    assert per == 7 and cycle == (6 if precond == "ilu0" else 5)
    assert [counts[its][0] for its in (2, 5, 8)] == [2 + cycles * cycle + its * per for its, cycles in ((2, 1), (5, 2), (8, 3))], counts
    sweeps = s.ilu.lower.info["launches"] + s.ilu.upper.info["launches"] if precond == "ilu0" else 0
    assert counts[5][1] - counts[2][1] >= 3 * (per + 1 + sweeps), counts               # a product and the sweeps per slot


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_solve_on_a_side_stream(prec, precond):
    key = ("grid", 40, 25)
    s, (want, info) = _system(key, prec, precond), _reference(key, prec, precond)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for check_every, history in ((0, True), (3, True), (3, None)):
        got, state = s.solve(check_every=check_every, history=history, stream=side)
        assert (got[3] is None) == (history is None)
        _equal(got, want, state, info)


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ilu0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_graph_capture_and_replay(prec, precond):
    """a solve that reads nothing back, captured (one stream) and replayed twice onto a zeroed x: the eager solve's bits both times"""
    key = ("grid", 40, 25)
    s = _system(key, prec, precond)
    limit = _reference(key, prec, precond)[1]["slots"] + 33
    want, info = _reference(key, prec, precond, max_iterations=limit)
    assert want[1] == model.CONVERGED
    solver = s.solver()
    x = torch.zeros(s.n, dtype=TORCH[prec], device="cuda")
    history = torch.zeros(limit + 1, dtype=TORCH[prec], device="cuda")
    solver.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)       # (warm-up, eager)
    torch.cuda.synchronize()
    assert _same(x.cpu().numpy(), want[0])
    graph = torch.cuda.CUDAGraph()
    x.zero_()
    with torch.cuda.graph(graph):
        solver.solve(s.d_val, s.d_b, x=x, rtol=RTOL[prec], max_iterations=limit, check_every=0, history=history)
    for _ in range(2):
        x.zero_(); history.fill_(3)
        graph.replay()
        state = solver.state
        assert (state["status"], state["iterations"], state["slots"], state["cycles"], state["exit"]) == (want[1], want[2], info["slots"],
                                                                                                         info["cycles"], want[4])
        assert _same(x.cpu().numpy(), want[0])
        assert _same(history.cpu().numpy()[:want[2] + 1], want[3]) and (history.cpu().numpy()[want[2] + 1:] == 3).all()


@gpu
def test_plans_of_other_rows_are_refused_and_the_tuple_form():
    s, other = _system(("grid", 24, 24), "f64", "ilu0"), _system(("grid", 40, 25), "f64", "ilu0")
    with pytest.raises(M.MspmvError, match="do not fit"):
        M.Gmres(s.d_off, s.d_col, torch.float64, preconditioner=(other.ilu.lower, other.ilu.upper, other.ilu.lu_values, other.d_off, other.d_col))
    for restart in (0, 129, 2.5):
        with pytest.raises(M.MspmvError, match="restart"):
            M.Gmres(s.d_off, s.d_col, torch.float64, restart=restart)
    lib = importlib.import_module("merge_spmv_amd.gmres").load_gmres_library()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    handle = s.solver()._handle
    assert lib.mspmv_gmres_set_factor(handle, other.ilu.lower._handle, other.ilu.upper._handle, ptr(other.ilu.lu_values), ptr(other.d_off),
                                      ptr(other.d_col)) == 1
    assert lib.mspmv_gmres_set_factor(handle, s.ilu.lower._handle, other.ilu.upper._handle, ptr(s.ilu.lu_values), ptr(s.d_off), ptr(s.d_col)) == 1
    with pytest.raises(M.MspmvError, match="nothing is factorised"):
        M.Gmres(s.d_off, s.d_col, torch.float64, preconditioner=M.Ilu0(s.d_off, s.d_col))
    want, info = _reference(("grid", 24, 24), "f64", "ilu0")
    solver = M.Gmres(s.d_off, s.d_col, torch.float64, preconditioner=(s.ilu.lower, s.ilu.upper, s.ilu.lu_values))
    x = solver.solve(s.d_val, s.d_b, rtol=RTOL["f64"], max_iterations=LIMIT)
    assert _same(x.cpu().numpy(), want[0]) and solver.state["iterations"] == want[2] and solver.state["cycles"] == info["cycles"]
    solver.close()
    # Jacobi on a pattern that lacks a diagonal entry: the state names the row, the solve is refused
    off, col, val = _matrix(("band", 5), "f64")
    keep = np.ones(col.size, bool)
    keep[off[2] + list(col[off[2]:off[3]]).index(2)] = False
    off2 = off.copy(); off2[3:] -= 1
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off2, col[keep], val[keep]))
    solver = M.Gmres(d_off, d_col, torch.float64, preconditioner="jacobi")
    assert solver.state["bad_diagonal_row"] == 2
    with pytest.raises(M.MspmvError, match="mspmv_gmres_solve"):
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
               dict(preconditioner=None), dict(preconditioner="jacobi", restart=5)):
        x, state = M.gmres(d_val, d_off, d_col, d_b, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True, **kw)
        assert state["status"] == "CONVERGED" and state["exit"] == "rr" and state["restart"] == kw.get("restart", 30), kw
        assert _true_residual(off, col, val, x.cpu().numpy(), b) <= RESIDUAL[prec], kw
        seen[(kw["preconditioner"], kw.get("reorder", True), kw.get("restart", 30))] = (state["iterations"], x)
    # the permuted solve is the solve of the permuted system, mapped back: the bits of the multicolour case of this file
    s = _system(("grid", 40, 25), prec, "ilu0-multicolour")
    want = _reference(("grid", 40, 25), prec, "ilu0-multicolour")[0]
    assert seen[("ilu0", True, 30)][0] == want[2]
    assert _same(seen[("ilu0", True, 30)][1].cpu().numpy(), s.coloring.permute_vector(torch.from_numpy(want[0]).cuda(), back=True).cpu().numpy())
    natural = _reference(("grid", 40, 25), prec, "ilu0")[0]
    assert seen[("ilu0", False, 30)][0] == natural[2] and _same(seen[("ilu0", False, 30)][1].cpu().numpy(), natural[0])
    # a guess in the caller's numbering, the answer in the caller's tensor: starting from the answer ends at once
    x = seen[("ilu0", True, 30)][1].clone()
    out, state = M.gmres(d_val, d_off, d_col, d_b, x=x, rtol=2 * RESIDUAL[prec], max_iterations=LIMIT, return_state=True)
    assert out is x and (state["status"], state["iterations"], state["exit"]) == ("CONVERGED", 0, "start")
    # ... and a guess that is not the answer: the solve of the permuted system from the permuted guess
    guess = torch.from_numpy(C.guess(1000, NP[prec])).cuda()
    out, state = M.gmres(d_val, d_off, d_col, d_b, x=guess, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True)
    assert out is guess and state["status"] == "CONVERGED" and _true_residual(off, col, val, out.cpu().numpy(), b) <= RESIDUAL[prec]
    want = s.model(x0=s.coloring.permute_vector(torch.from_numpy(C.guess(1000, NP[prec])).cuda()).cpu().numpy())[0]
    assert state["iterations"] == want[2]
    assert _same(out.cpu().numpy(), s.coloring.permute_vector(torch.from_numpy(want[0]).cuda(), back=True).cpu().numpy())
