"""mspmv_pcg_* past one workgroup, at every exit and with a diagonal that tells the rows apart.  tests/test_pcg.py compares the solver ON
THE BITS with tests/pcg_model.py, but on systems below one chunk of 1024 rows and with the constant 4 on the diagonal.  Here the same
comparison runs where the kernels' index arithmetic differs: several workgroups, a partly empty last chunk, a lane that straddles n
behind full chunks, the two-level fold (more than 1024 partials), and matrices whose diagonals are all different and no power of two.
The model's operators are the library's own calls (M.csrmv, Ic0.solve, Ilu0.solve, CsrSv.solve), which have exact tests of theirs.
Every precondition of a reference -- the exit it takes, convergence below LIMIT, the true residual -- is asserted on the CPU from the
model with a product on the host, so that no device test can hide that its input took another path.  A NaN equals any NaN."""
import functools

import numpy as np
import pytest

import color_model
import merge_spmv_amd as M
import pcg_model as model
from pcg_common import LIMIT, NP, PRECS, RESIDUAL, RTOL, TORCH, _bits, _host_product, _true_residual

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

SEED = 3
SHAPES = [(1, 1), (3, 1), (5, 1), (32, 32), (41, 25), (37, 29), (64, 65)]          # n = 1, 3, 5, 1024, 1025, 1073, 4160
LARGE = [(37, 29), (64, 65)]                    # n % 4 == 1 behind one full chunk; five workgroups, the last one partial
PRECONDS = ["none", "jacobi", "ic0", "ic0-multicolour"]
CHAIN_N = 2 ** 20 + 1029                        # 1026 partials: two chunks of them, the second holding two; n % 4 == 1
CHAIN_ITERATIONS = 3
ROW = 1050                                      # a row of the second chunk of the 37 x 29 grid
_id = lambda shape: "%dx%d" % shape


def _same(got, want):
    """equal bits; a NaN equals any NaN (its sign and payload are not defined)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


# ------------------------------------------------------------------------------------------------------------ matrices
def _assemble(n, u, v, weights, shift, dtype):
    """CSR with sorted rows: weights[e] (rounded to dtype) at (u[e], v[e]) and at (v[e], u[e]); on the diagonal the sum of the row's
    |off-diagonal| values in fp64 plus shift[i], rounded to dtype"""
    weights = weights.astype(dtype)
    mag = np.abs(weights.astype(np.float64))
    diag = (np.bincount(u, weights=mag, minlength=n) + np.bincount(v, weights=mag, minlength=n) + shift).astype(dtype)
    here = np.arange(n)
    r, c, a = np.concatenate([u, v, here]), np.concatenate([v, u, here]), np.concatenate([weights, weights, diag])
    order = np.lexsort((c, r))
    off = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=off[1:])
    return off, c[order].astype(np.int32), a[order]


def varied_grid(w, h, dtype, seed):
    """the 5-point pattern of a w x h grid, rows sorted: one draw from (-2, -1) per undirected edge, stored at both mirror entries; the
    diagonal is the row's sum of |off-diagonal| plus a draw from (0.5, 1.5): strictly diagonally dominant, hence SPD"""
    rng = np.random.default_rng(seed)
    idx = np.arange(w * h).reshape(h, w)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return _assemble(w * h, u, v, rng.uniform(-2, -1, u.size), rng.uniform(0.5, 1.5, w * h), dtype)


def varied_chain(n, dtype, seed):
    """the same for the tridiagonal pattern of a chain of n rows"""
    rng = np.random.default_rng(seed)
    u = np.arange(n - 1)
    return _assemble(n, u, u + 1, rng.uniform(-2, -1, n - 1), rng.uniform(0.5, 1.5, n), dtype)


def _rows_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _diagonal_positions(off, col):
    at = np.flatnonzero(col == _rows_of(off))
    assert at.size == len(off) - 1
    return at


def _rhs(n, dtype, seed=22):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)


def _guess(n, dtype, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)


@functools.lru_cache(maxsize=None)
def _matrix(shape, prec):
    return varied_grid(shape[0], shape[1], NP[prec], SEED)


@functools.lru_cache(maxsize=None)
def _chain(prec):
    return varied_chain(CHAIN_N, NP[prec], SEED)


def _signs(n):
    """mixed signs: every third row negative.  (With a positive majority alpha is about 1 and the first update all but cancels r on the positive rows
    and doubles it on the negative ones, so r.z turns negative at once.)"""
    return np.where(np.arange(n) % 3 == 0, -1.0, 1.0)


def _diagonal_factor(precond, d):
    """(factor values, is the second sweep UNIT?) of a factor on the pattern of a diagonal matrix.  Both sweeps read the ONE value array
    that mspmv_pcg_set_factor takes, so two NON_UNIT sweeps on s give M = s^2 > 0 whatever the signs of s; an indefinite M is a
    NON_UNIT sweep on the signed values and a UNIT sweep (the identity) behind it."""
    if precond == "diagonal":
        return np.sqrt(d.astype(np.float64)).astype(d.dtype), False
    if precond == "diagonal-negative":
        return -d, True
    assert precond == "diagonal-mixed"
    return (d * _signs(d.size)).astype(d.dtype), True


def _host_ilu0(off, col, val):
    """U^-1 (L^-1 r) with ILU(0) of the matrix, in fp64 on the host, as plain loops over the rows.  For a symmetric matrix L U is
    L D L^T, the M of IC(0) in exact arithmetic, so this one restatement serves the CPU checks of both factors."""
    n = len(off) - 1
    rows = [dict(zip(col[off[i]:off[i + 1]].tolist(), val[off[i]:off[i + 1]].astype(np.float64).tolist())) for i in range(n)]
    for i, row in enumerate(rows):
        for k in sorted(c for c in row if c < i):
            row[k] /= rows[k][k]
            for j, u in rows[k].items():
                if j > k and j in row:
                    row[j] -= row[k] * u
    lower = [[(c, v) for c, v in row.items() if c < i] for i, row in enumerate(rows)]
    upper = [[(c, v) for c, v in row.items() if c > i] for i, row in enumerate(rows)]

    def apply(r):
        y = r.astype(np.float64).tolist()
        for i in range(n):
            y[i] -= sum(v * y[c] for c, v in lower[i])
        for i in reversed(range(n)):
            y[i] = (y[i] - sum(v * y[c] for c, v in upper[i])) / rows[i][i]
        return np.asarray(y, r.dtype)
    return apply


def _host_multicolour(off, col, val, b):
    """P A P^T and P b in the multicolour numbering, from the numpy model of the ordering (tests/color_model.py)"""
    c = color_model.coloring(off, col)
    off_b, col_b, val_b, _ = color_model.permute(off, col, val, len(off) - 1, row_perm=c["order"], col_map=c["inverse"])
    return off_b, col_b, val_b, b[c["order"]]


def _chain_colours(n):
    """the colours color_model.colors gives a chain of n rows (greedy in descending key order), vectorised: a row takes the smallest
    colour that no neighbour of larger key holds, as soon as those neighbours have theirs"""
    key = color_model.keys(n)
    wait_left, wait_right = np.zeros(n, bool), np.zeros(n, bool)
    wait_left[1:], wait_right[:-1] = key[:-1] > key[1:], key[1:] > key[:-1]
    colour = np.full(n, -1, np.int32)
    while (colour < 0).any():
        left, right = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        left[1:], right[:-1] = colour[:-1], colour[1:]
        ready = (colour < 0) & (~wait_left | (left >= 0)) & (~wait_right | (right >= 0))
        left, right = np.where(wait_left, left, -1), np.where(wait_right, right, -1)
        c = np.zeros(n, np.int32)
        for _ in range(2):
            c = np.where((left == c) | (right == c), c + 1, c)
        colour[ready] = c[ready]
    return colour


def _host_chain_ic0(off, col, val, colour):
    """L^-T (L^-1 r) with IC(0) of P A P^T for a tridiagonal A and P the stable sort of the rows by `colour`, in fp64 on the host and in
    A's own numbering.  Neighbours never share a colour and the two neighbours of a row are not neighbours of each other, so no
    entry of L meets another: L[i][j] = A[i][j] / L[j][j] for a neighbour j of smaller colour, L[i][i]^2 = A[i][i] - the sum of their
    squares, and a colour's rows are worked at once."""
    at = _diagonal_positions(off, col)
    n = at.size
    d = val[at].astype(np.float64)
    beside = np.concatenate([[0.0], val[at[:-1] + 1].astype(np.float64), [0.0]])       # beside[i] = A[i][i-1], beside[i + 1] = A[i][i+1]
    rows_of = [np.flatnonzero(colour == c) for c in range(int(colour.max()) + 1)]
    root = np.ones(n)

    def sides(rows, lower):
        """(rows, their neighbour, the entry between them) for the left and the right neighbours that come before (lower) or after them"""
        out = []
        for step in (-1, 1):
            i = rows[(rows + step >= 0) & (rows + step < n)]
            before = colour[i + step] < colour[i]
            i = i[before == lower]
            out.append((i, i + step, beside[i + (step + 1) // 2]))
        return out

    for rows in rows_of:
        s = d.copy()
        for i, j, a in sides(rows, True):
            s[i] -= (a / root[j]) ** 2
        root[rows] = np.sqrt(s[rows])

    def apply(r):
        y = r.astype(np.float64)
        for rows in rows_of:
            for i, j, a in sides(rows, True):
                y[i] -= a / root[j] * y[j]
            y[rows] /= root[rows]
        for rows in reversed(rows_of):
            for i, j, a in sides(rows, False):
                y[i] -= a / root[i] * y[j]
            y[rows] /= root[rows]
        return y.astype(r.dtype)
    return apply


def _host_precond(precond, off, col, val):
    """M^-1 r on the host, for the CPU checks of the references' preconditions"""
    if precond == "none":
        return lambda r: r
    if precond in ("ic0", "ic0-multicolour", "ilu0"):
        return _host_ilu0(off, col, val)
    d = val[_diagonal_positions(off, col)]
    if precond == "jacobi":
        return lambda r: r / d
    s, unit = _diagonal_factor(precond, d)
    return (lambda r: r / s) if unit else (lambda r: (r / s) / s)


# ------------------------------------------------------------------------------------------------------------ the exits
EXITS = ["negative-M", "mixed-M", "inf-on-the-diagonal", "nan-in-b", "inf-in-b", "inf-in-b-zero-tolerances", "inf-in-b-by-rr", "inf-in-b-1x1",
         "no-iterations", "no-iterations-with-a-guess", "atol", "zero-A", "alpha-overflows"]


def _exit_case(name, prec):
    """the input of one row of the table of exits (on varied_grid 37 x 29, no preconditioner unless the row names one) and what it must
    leave: (status, iterations or None for "some", the test that ended the solve)"""
    dt = NP[prec]
    off, col, val = _matrix((37, 29), prec)
    n = len(off) - 1
    case = dict(off=off, col=col, val=val, b=_rhs(n, dt), precond="none", x0=None, rtol=RTOL[prec], atol=0.0, max_iterations=LIMIT)
    if name == "negative-M":
        case.update(precond="diagonal-negative", want=(model.BREAKDOWN, 1, "rz"))
    elif name == "mixed-M":
        case.update(precond="diagonal-mixed", want=(model.BREAKDOWN, 1, "rz"))
    elif name == "inf-on-the-diagonal":
        val = val.copy()
        val[_diagonal_positions(off, col)[ROW]] = np.inf
        case.update(val=val, want=(model.BREAKDOWN, 1, "rr-nan"))
    elif name in ("nan-in-b", "inf-in-b", "inf-in-b-zero-tolerances"):
        case["b"][ROW] = np.nan if name == "nan-in-b" else np.inf
        case.update(want=(model.BREAKDOWN, 0, "pq"))
        if name == "inf-in-b-zero-tolerances":
            case.update(rtol=0.0)
    elif name == "inf-in-b-by-rr":
        # An Inf in b leaves by pq only if some p[i] q[i] is -Inf.  q[ROW] is +Inf and q of a neighbour j is -Inf (the entry beside the
        # diagonal is negative), so with b[j] < 0 at every neighbour all infinite products are +Inf: pq = +Inf > 0, alpha = Inf / Inf
        # is a NaN, and the first update writes it into every x[i] and r[i].
        rows = _rows_of(off)
        neighbours = col[(rows == ROW) & (col != ROW)]
        assert neighbours.size == 3                                    # (ROW lies in the last row of the grid)
        case["b"][ROW] = np.inf
        case["b"][neighbours] = -np.abs(case["b"][neighbours])
        case.update(want=(model.BREAKDOWN, 1, "rr-nan"))
    elif name == "inf-in-b-1x1":
        off, col, val = _matrix((1, 1), prec)                          # the same path with no neighbour at all: A = [d], b = [Inf]
        case.update(off=off, col=col, val=val, b=np.array([np.inf], dt), want=(model.BREAKDOWN, 1, "rr-nan"))
    elif name == "no-iterations":
        case.update(max_iterations=0, want=(model.RUNNING, 0, None))
    elif name == "no-iterations-with-a-guess":
        case.update(max_iterations=0, x0=_guess(n, dt), want=(model.RUNNING, 0, None))
    elif name == "atol":
        case.update(atol=3.0, want=(model.CONVERGED, None, "rr"))
    elif name == "zero-A":
        case.update(val=np.zeros_like(val), want=(model.BREAKDOWN, 0, "pq"))
    else:
        # A scaled into the subnormals (nothing is flushed to zero): rz / pq overflows, alpha = +Inf, every r[i] is an infinity and rr =
        # +Inf -- not a NaN, and not converged.  beta = +Inf then makes p hold Inf - Inf, and the next pq is a NaN.
        assert name == "alpha-overflows"
        case.update(val=(val * dt(2.0) ** (-136 if prec == "f32" else -1034)).astype(dt), want=(model.BREAKDOWN, 1, "pq"))
    return case


def _check_exit(name, case, result, info):
    """what the row leaves behind, asserted of the model's result on the CPU and of the device's on the GPU.  info: bb, stop2, rr, rz
    as numbers of the value type, and on the CPU the last pq (the device's state block does not show it)"""
    x, status, iterations, history = result
    t = x.dtype.type
    want_status, want_iterations, _ = case["want"]
    assert status == want_status and history.size == iterations + 1
    assert iterations == want_iterations if want_iterations is not None else 0 < iterations < LIMIT
    start = np.zeros_like(x) if case["x0"] is None else case["x0"]
    if name in ("negative-M", "mixed-M"):
        assert np.isfinite(history).all() and np.isfinite(x).all() and x.any()          # x is updated once
    elif name == "inf-on-the-diagonal":
        assert np.isnan(history[1]) and np.isfinite(history[0]) and not _bits(x).any()   # alpha = +0: x keeps the start's bits
    elif name == "nan-in-b":
        assert np.isnan(history[0]) and not _bits(x).any() and np.isnan(info.get("pq", np.nan))
    elif name in ("inf-in-b", "inf-in-b-zero-tolerances"):
        assert history[0] == np.inf and not _bits(x).any() and np.isnan(info.get("pq", np.nan))
        assert np.isinf(info["bb"]) and (info["stop2"] == np.inf if case["rtol"] > 0 else info["stop2"] == 0)      # (a NaN s: stop2 is a2)
    elif name in ("inf-in-b-by-rr", "inf-in-b-1x1"):
        assert history[0] == np.inf and np.isnan(history[1]) and np.isnan(x).all() and info.get("pq", np.inf) == np.inf
        assert info["bb"] == np.inf and info["stop2"] == np.inf
    elif name.startswith("no-iterations"):
        assert _same(history, np.array([info["rr"]], x.dtype)) and np.array_equal(_bits(x), _bits(start)) and history[0] > info["stop2"]
    elif name == "atol":
        a2 = t(case["atol"]) * t(case["atol"])
        rt = t(case["rtol"])
        assert float(info["stop2"]) == float(a2) and a2 > t(rt * rt) * info["bb"]
        assert history[-1] <= a2 < history[-2]
    elif name == "zero-A":
        assert not _bits(x).any() and history[0] == info["bb"] > 0 and info.get("pq", 0) == 0
    else:
        assert history[1] == np.inf and np.isinf(x).all()


# ------------------------------------------------------------------------------------------------------------------ CPU
def _assert_varied(off, col, val, distinct):
    n = len(off) - 1
    r_of = _rows_of(off)
    assert (np.diff(off) > 0).all() and (col[1:] > col[:-1])[r_of[1:] == r_of[:-1]].all()          # rows sorted, no column twice
    mirror = np.lexsort((r_of, col))                                   # the entries in the order of the transpose
    assert np.array_equal(col[mirror], r_of) and np.array_equal(r_of[mirror], col) and np.array_equal(_bits(val[mirror]), _bits(val))
    at = _diagonal_positions(off, col)
    d = val[at].astype(np.float64)
    rest = np.abs(val.astype(np.float64))
    rest[at] = 0
    assert (d > np.bincount(r_of, weights=rest, minlength=n)).all()    # strictly dominant after the rounding
    assert (np.frexp(d)[0] != 0.5).all()                               # no power of two: a division by d is not exact
    if distinct:
        assert np.unique(d).size == n
    return d


@pytest.mark.parametrize("prec", PRECS)
def test_the_varied_matrices_are_symmetric_dominant_and_tell_the_rows_apart(prec):
    for shape in SHAPES:
        off, col, val = _matrix(shape, prec)
        assert len(off) - 1 == shape[0] * shape[1] and val.dtype == NP[prec]
        _assert_varied(off, col, val, distinct=True)
    _assert_varied(*varied_chain(1029, NP[prec], SEED), distinct=True)
    # 2^20 diagonals cannot all differ among the 2^23 numbers of an fp32 binade: there, neighbours differ (a row's own four lanes too)
    d = _assert_varied(*_chain(prec), distinct=prec == "f64")
    for step in (1, 2, 3, 4):
        assert (d[step:] != d[:-step]).all()


def _converges_on_the_host(shape, prec, precond, guess=False):
    """the preconditions of the device tests' references: CONVERGED below LIMIT, the true residual inside RESIDUAL"""
    off, col, val = _matrix(shape, prec)
    b = _rhs(len(off) - 1, NP[prec])
    if precond == "ic0-multicolour":
        off, col, val, b = _host_multicolour(off, col, val, b)
    x0 = _guess(len(off) - 1, NP[prec]) if guess else None
    x, status, iterations, _ = model.pcg(_host_product(off, col, val), _host_precond(precond, off, col, val), b, x0, RTOL[prec], 0.0, LIMIT)
    assert status == model.CONVERGED and 0 < iterations < LIMIT, (status, iterations)
    assert _true_residual(off, col, val, x, b) <= RESIDUAL[prec]
    return iterations


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_model_converges_on_the_host(shape, prec, precond):
    iterations = _converges_on_the_host(shape, prec, precond)
    assert shape not in LARGE or iterations > 5                        # the cut-off at 5 iterations is RUNNING


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LARGE, ids=_id)
def test_the_model_converges_on_the_host_from_the_guess(shape, prec, precond):
    _converges_on_the_host(shape, prec, precond, guess=True)


@pytest.mark.parametrize("precond", ["ilu0", "diagonal"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_model_converges_on_the_host_with_ilu0_and_the_diagonal_factor(prec, precond):
    _converges_on_the_host((37, 29), prec, precond)


@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_model_is_running_after_three_iterations_of_the_chain(prec, precond):
    off, col, val = _chain(prec)
    for x0 in (None, _guess(CHAIN_N, NP[prec])):
        info = {}
        _, status, iterations, history = model.pcg(_host_product(off, col, val), _host_precond(precond, off, col, val), _rhs(CHAIN_N, NP[prec]), x0,
                                                   RTOL[prec], 0.0, CHAIN_ITERATIONS, info)
        assert (status, iterations, info["exit"]) == (model.RUNNING, CHAIN_ITERATIONS, None)
        assert np.isfinite(history).all() and (history > info["stop2"]).all()


def test_the_chain_colours_and_its_host_ic0_are_the_general_ones():
    """on a chain short enough for the loops: the vectorised colours are color_model's, the vectorised IC(0) is the host ILU(0) of the
    permuted matrix"""
    off, col, val = varied_chain(1029, np.float64, SEED)
    colour = _chain_colours(1029)
    assert np.array_equal(colour, color_model.colors(off, col)) and 2 <= colour.max() + 1 <= 3
    r = _rhs(1029, np.float64)
    off_b, col_b, val_b, r_b = _host_multicolour(off, col, val, r)
    order = color_model.schedule(colour)[0]
    assert np.allclose(_host_chain_ic0(off, col, val, colour)(r)[order], _host_ilu0(off_b, col_b, val_b)(r_b), rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_is_running_after_three_iterations_of_the_chain_with_ic0(prec):
    """IC(0) of a chain in natural order is exact (one iteration); in the multicolour order it is not.  The solve of P A P^T x' = P b
    is the solve of A x = b with M = P^T L L^T P, which is what runs here, in A's numbering."""
    off, col, val = _chain(prec)
    info = {}
    apply_m = _host_chain_ic0(off, col, val, _chain_colours(CHAIN_N))
    _, status, iterations, history = model.pcg(_host_product(off, col, val), apply_m, _rhs(CHAIN_N, NP[prec]), None, RTOL[prec], 0.0,
                                               CHAIN_ITERATIONS, info)
    assert (status, iterations, info["exit"]) == (model.RUNNING, CHAIN_ITERATIONS, None)
    assert np.isfinite(history).all() and (history > info["stop2"]).all()


@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_solves_of_a_reused_handle_on_the_host(prec, precond):
    """the preconditions of test_solving_again_after_a_breakdown: -A leaves by pq before the first iteration; another b with a guess
    converges"""
    off, col, val = _matrix((64, 65), prec)
    n = len(off) - 1
    info = {}
    x, status, iterations, _ = model.pcg(_host_product(off, col, -val), _host_precond(precond, off, col, -val), _rhs(n, NP[prec]), None,
                                         RTOL[prec], 0.0, LIMIT, info)
    assert (status, iterations, info["exit"]) == (model.BREAKDOWN, 0, "pq") and info["pq"] < 0 and not _bits(x).any()
    b, x0 = _rhs(n, NP[prec], seed=23), _guess(n, NP[prec], seed=24)
    x, status, iterations, _ = model.pcg(_host_product(off, col, val), _host_precond(precond, off, col, val), b, x0, RTOL[prec], 0.0, LIMIT, info)
    assert status == model.CONVERGED and 0 < iterations < LIMIT and _true_residual(off, col, val, x, b) <= RESIDUAL[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", EXITS)
def test_every_exit_is_taken_on_the_host(name, prec):
    case = _exit_case(name, prec)
    off, col, val = case["off"], case["col"], case["val"]
    info = {}
    result = model.pcg(_host_product(off, col, val), _host_precond(case["precond"], off, col, _matrix((37, 29), prec)[2]), case["b"], case["x0"],
                       case["rtol"], case["atol"], case["max_iterations"], info)
    assert info["exit"] == case["want"][2], info
    _check_exit(name, case, result, info)


def test_an_infinite_residual_never_converges():
    """the rule of include/mspmv.h, in the model: rr <= stop2 AND rr < +Inf.  With an Inf in b and rtol > 0, bb = stop2 = rr = +Inf: the
    start stays RUNNING and the solve breaks down -- here by a NaN pq (a -Inf among the products); the exits "inf-in-b-by-rr" and
    "inf-in-b-1x1" take the other way out."""
    off, col, val = _matrix((5, 1), "f64")
    b = np.array([1.0, np.inf, 1.0, -2.0, 0.5])
    info = {}
    x, status, iterations, history = model.pcg(_host_product(off, col, val), lambda r: r, b, None, 1e-8, 0.0, 10, info)
    assert (status, iterations, info["exit"]) == (model.BREAKDOWN, 0, "pq") and info["stop2"] == np.inf and history[0] == np.inf and not _bits(x).any()
    # finite inputs: rr <= stop2 is finite, nothing changes
    x, status, iterations, _ = model.pcg(_host_product(off, col, val), lambda r: r, np.zeros(5), None, 1e-8, 0.0, 10, info)
    assert (status, iterations, info["exit"]) == (model.CONVERGED, 0, "start")


# ------------------------------------------------------------------------------------------------------------------ GPU
class _System:
    """one matrix, one right-hand side, one preconditioner: the device arrays, the model's operators, the Pcg"""

    def __init__(self, matrix, prec, precond, b=None):
        dt = NP[prec]
        off, col, val = matrix
        n = self.n = len(off) - 1
        b = _rhs(n, dt) if b is None else b
        d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, b))
        self.coloring = None
        if precond == "ic0-multicolour":
            self.coloring, p = M.multicolor_reorder(d_val, d_off, d_col)
            d_off, d_col, d_val = p.row_offsets, p.column_indices, p.values
            d_b = self.coloring.permute_vector(d_b)
            off, col, val, b = (t.cpu().numpy() for t in (d_off, d_col, d_val, d_b))
        self.off, self.col, self.val, self.b = off, col, val, b
        self.d_off, self.d_col, self.d_val, self.d_b = d_off, d_col, d_val, d_b
        self.prec, self.precond = prec, precond
        self.factor = self.plans = None
        through = lambda solve: (lambda r: solve(torch.from_numpy(r).cuda()).cpu().numpy())
        if precond == "none":
            self.apply_M, m = (lambda r: r), None
        elif precond == "jacobi":
            self.apply_M, m = None, "jacobi"                           # (the diagonal of the values of the solve: operators())
        elif precond in ("ic0", "ic0-multicolour", "ilu0"):
            self.factor = (M.Ilu0 if precond == "ilu0" else M.Ic0)(d_off, d_col)
            assert int(self.factor.factor(d_val).item()) == -1
            self.apply_M, m = through(self.factor.solve), self.factor
        else:
            # a factor with pattern arrays of its own: a diagonal matrix
            values, unit = _diagonal_factor(precond, val[_diagonal_positions(off, col)])
            f_off, f_col, f_val = (torch.from_numpy(a).cuda() for a in (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), values))
            first = M.CsrSv(f_off, f_col, lower=True, unit_diagonal=False)
            second = M.CsrSv(f_off, f_col, lower=False, unit_diagonal=unit)
            self.plans = (first, second)
            self.apply_M, m = through(lambda r: second.solve(f_val, first.solve(f_val, r))), (first, second, f_val, f_off, f_col)
        self.pcg = M.Pcg(d_off, d_col, TORCH[prec], preconditioner=m)

    def close(self):
        self.pcg.close()
        for held in (self.factor, self.coloring) + (self.plans or ()):
            if held is not None:
                held.close()

    def operators(self, d_val):
        apply_A = lambda p: M.csrmv(d_val, self.d_off, self.d_col, torch.from_numpy(p).cuda(), num_cols=self.n).cpu().numpy()
        if self.precond != "jacobi":
            return apply_A, self.apply_M
        d = d_val.cpu().numpy()[_diagonal_positions(self.off, self.col)]
        return apply_A, lambda r: r / d

    def model(self, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, b=None, values=None):
        """((x, status, iterations, history), info) of the model on the library's operators"""
        apply_A, apply_M = self.operators(self.d_val if values is None else values)
        info = {}
        return model.pcg(apply_A, apply_M, self.b if b is None else b, x0, RTOL[self.prec] if rtol is None else rtol, atol, max_iterations, info), info

    def solve(self, x0=None, rtol=None, atol=0.0, max_iterations=LIMIT, check_every=8, b=None, values=None, history=True, stream=None):
        """((x, status, iterations, history[0 .. iterations] or None), state) of the device"""
        x = None if x0 is None else torch.from_numpy(x0).cuda()
        x = self.pcg.solve(self.d_val if values is None else values, self.d_b if b is None else torch.from_numpy(b).cuda(), x=x,
                           rtol=RTOL[self.prec] if rtol is None else rtol, atol=atol, max_iterations=max_iterations, check_every=check_every,
                           history=history, stream=stream)
        state = self.pcg.state                                         # (synchronises the device)
        kept = None if self.pcg.history is None else self.pcg.history.cpu().numpy()[:state["iterations"] + 1]
        return (x.cpu().numpy(), state["status"], state["iterations"], kept), state


def _equal(got, want, state=None, info=None):
    (x, status, its, history), (mx, mstatus, mits, mhistory) = got, want
    assert (status, its) == (mstatus, mits)
    assert history is None or _same(history, mhistory)
    assert _same(x, mx)
    if state is not None:
        t = mx.dtype.type
        for name in ("rr", "bb", "stop2"):
            assert _same(t(state[name]), info[name]), (name, state[name], info[name])
        assert info["rz"] is None or _same(t(state["rz"]), info["rz"]), (state["rz"], info["rz"])


@functools.lru_cache(maxsize=None)
def _system(shape, prec, precond):
    return _System(_matrix(shape, prec), prec, precond)


@functools.lru_cache(maxsize=None)
def _reference(shape, prec, precond, guess=False, max_iterations=LIMIT):
    """the model's run, computed once and shared"""
    s = _system(shape, prec, precond)
    return s.model(x0=_guess(s.n, NP[prec]) if guess else None, max_iterations=max_iterations)


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_shape_on_the_bits_and_the_true_residual(shape, prec, precond):
    s, (want, info) = _system(shape, prec, precond), _reference(shape, prec, precond)
    got, state = s.solve()
    print(f"pcg {_id(shape)} {prec} {precond}: {got[2]} iterations, status {got[1]}, true residual {_true_residual(s.off, s.col, s.val, got[0], s.b):.3e}")
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    assert _true_residual(s.off, s.col, s.val, want[0], s.b) <= RESIDUAL[prec]
    _equal(got, want, state, info)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]
    assert state["launches_per_iteration"] == (7 if precond.startswith("ic0") else 5)
    assert state["rr"] <= state["stop2"] and state["bb"] == float(model.dot(s.b, s.b))


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LARGE, ids=_id)
def test_a_random_guess_and_a_cut_off(shape, prec, precond):
    s = _system(shape, prec, precond)
    want, info = _reference(shape, prec, precond, guess=True)
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    got, state = s.solve(x0=_guess(s.n, NP[prec]))
    _equal(got, want, state, info)
    want, info = _reference(shape, prec, precond, max_iterations=5)
    assert want[1:3] == (model.RUNNING, 5)
    got, state = s.solve(max_iterations=5)
    _equal(got, want, state, info)
    assert _same(got[3], _reference(shape, prec, precond)[0][3][:6])


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LARGE, ids=_id)
def test_check_every_and_six_surplus_iterations(shape, prec, precond):
    """the same x, iterations and history however often the host looks; iterations enqueued past the end change nothing"""
    s, (want, info) = _system(shape, prec, precond), _reference(shape, prec, precond)
    limit = want[2] + 6
    for check_every in (0, 1, 7):
        got, state = s.solve(max_iterations=limit, check_every=check_every)
        _equal(got, want, state, info)
        tail = s.pcg.history.cpu().numpy()[want[2] + 1:]
        assert tail.size == 6 and not _bits(tail).any()               # history beyond `iterations` is never written


@gpu
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LARGE, ids=_id)
def test_b_and_x_one_element_behind_a_16_byte_boundary(shape, prec, precond):
    s = _system(shape, prec, precond)
    want, _ = _reference(shape, prec, precond, guess=True)
    b = torch.full((s.n + 2,), 7.0, dtype=TORCH[prec], device="cuda")
    x = torch.full((s.n + 2,), 9.0, dtype=TORCH[prec], device="cuda")
    b[1:-1].copy_(s.d_b)
    x[1:-1].copy_(torch.from_numpy(_guess(s.n, NP[prec])))
    assert b[1:-1].data_ptr() % 16 == b.element_size() and x[1:-1].data_ptr() % 16 == x.element_size()
    s.pcg.solve(s.d_val, b[1:-1], x=x[1:-1], rtol=RTOL[prec], max_iterations=LIMIT, history=True)
    state = s.pcg.state
    assert (state["status"], state["iterations"]) == want[1:3]
    hb, hx = b.cpu().numpy(), x.cpu().numpy()
    assert hb[0] == 7.0 and hb[-1] == 7.0 and hx[0] == 9.0 and hx[-1] == 9.0 and np.array_equal(_bits(hb[1:-1]), _bits(s.b))
    assert _same(hx[1:-1], want[0]) and _same(s.pcg.history.cpu().numpy()[:want[2] + 1], want[3])


# ---- the two-level fold: more than 1024 partials
@functools.lru_cache(maxsize=None)
def _chain_system(prec, precond):
    return _System(_chain(prec), prec, precond)


@functools.lru_cache(maxsize=None)
def _chain_reference(prec, precond, guess):
    s = _chain_system(prec, precond)
    return s.model(x0=_guess(s.n, NP[prec]) if guess else None, max_iterations=CHAIN_ITERATIONS)


@gpu
@pytest.mark.parametrize("precond,guess", [("none", False), ("jacobi", False), ("ic0-multicolour", False), ("jacobi", True)],
                         ids=["none", "jacobi", "ic0-multicolour", "jacobi-guess"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_two_level_fold(prec, precond, guess):
    """n = 2^20 + 1029: the step kernel folds 1026 partials in two levels.  IC(0) is made of the multicolour order (a chain in natural
    order has n levels)."""
    s, (want, info) = _chain_system(prec, precond), _chain_reference(prec, precond, guess)
    assert -(-s.n // 1024) == 1026 and s.n % 4 == 1
    if s.factor is not None:
        print(f"pcg chain {prec}: {s.factor.lower.info['levels']} levels in the lower sweep")
    assert want[1:3] == (model.RUNNING, CHAIN_ITERATIONS) and want[3].size == CHAIN_ITERATIONS + 1 and np.isfinite(want[3]).all()
    got, state = s.solve(x0=_guess(s.n, NP[prec]) if guess else None, max_iterations=CHAIN_ITERATIONS)
    _equal(got, want, state, info)


# ---- preconditioner forms
@gpu
@pytest.mark.parametrize("precond", ["ilu0", "diagonal"])
@pytest.mark.parametrize("prec", PRECS)
def test_ilu0_and_a_factor_with_pattern_arrays_of_its_own(prec, precond):
    s, (want, info) = _system((37, 29), prec, precond), _reference((37, 29), prec, precond)
    got, state = s.solve()
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    _equal(got, want, state, info)
    assert _true_residual(s.off, s.col, s.val, got[0], s.b) <= RESIDUAL[prec]
    assert state["launches_per_iteration"] == s.pcg.launches_per_iteration == 7 and state["precond_kind"] == 2
    if precond == "diagonal":
        assert s.plans[0].nnz == s.n != s.pcg.nnz                      # the factor's pattern is not the matrix's


# ---- every exit
@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", EXITS)
def test_every_exit_on_the_bits(name, prec):
    case = _exit_case(name, prec)
    shared = case["val"] is _matrix((37, 29), prec)[2] and _same(case["b"], _rhs(len(case["off"]) - 1, NP[prec]))
    if shared:
        s = _system((37, 29), prec, case["precond"])
    else:
        # the factor of a diagonal preconditioner is made of the unchanged matrix; here only "none" meets changed values
        assert case["precond"] == "none"
        s = _System((case["off"], case["col"], case["val"]), prec, "none", b=case["b"])
    try:
        args = dict(x0=case["x0"], rtol=case["rtol"], atol=case["atol"], max_iterations=case["max_iterations"])
        want, info = s.model(**args)
        assert (want[1], info["exit"]) == (case["want"][0], case["want"][2]), (want[1:3], info)
        for check_every in (8, 0):
            got, state = s.solve(check_every=check_every, **args)
            _equal(got, want, state, info)
            t = NP[prec]
            _check_exit(name, case, got, {k: t(state[k]) for k in ("rr", "bb", "stop2", "rz")})      # (the state block does not show pq)
    finally:
        if not shared:
            s.close()


# ---- reuse and plumbing
@gpu
@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("prec", PRECS)
def test_solving_again_after_a_breakdown(prec, precond):
    """one handle: -A breaks down; then A gives the reference's bits (stale partials of five chunks, a stale status; Jacobi takes the
    new diagonal); then another b with a guess gives the model's"""
    shape = (64, 65)
    s = _System(_matrix(shape, prec), prec, precond)
    negated = -s.d_val
    want, info = s.model(values=negated)
    assert (want[1], want[2], info["exit"]) == (model.BREAKDOWN, 0, "pq")
    got, state = s.solve(values=negated)
    _equal(got, want, state, info)
    want, info = _reference(shape, prec, precond)
    got, state = s.solve()
    _equal(got, want, state, info)
    b, x0 = _rhs(s.n, NP[prec], seed=23), _guess(s.n, NP[prec], seed=24)
    want, info = s.model(x0=x0, b=b)
    assert want[1] == model.CONVERGED and 0 < want[2] < LIMIT
    got, state = s.solve(x0=x0, b=b)
    _equal(got, want, state, info)
    s.close()


@gpu
@pytest.mark.parametrize("precond", ["jacobi", "ic0-multicolour"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_solve_on_a_side_stream(prec, precond):
    s, (want, info) = _system((64, 65), prec, precond), _reference((64, 65), prec, precond)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for check_every, history in ((0, True), (3, True), (3, None)):
        got, state = s.solve(max_iterations=want[2] + 2, check_every=check_every, history=history, stream=side)
        assert (got[3] is None) == (history is None)
        _equal(got, want, state, info)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_the_one_shot_call_with_a_random_guess(prec):
    """reorder=True with IC(0): the guess and the answer are in the caller's numbering, the answer in the caller's tensor; the bits are
    those of a Pcg on the permuted system with the permuted guess, permuted back"""
    s = _system((37, 29), prec, "ic0-multicolour")
    off, col, val = _matrix((37, 29), prec)
    d_off, d_col, d_val, d_b = (torch.from_numpy(a).cuda() for a in (off, col, val, _rhs(s.n, NP[prec])))
    guess = torch.from_numpy(_guess(s.n, NP[prec])).cuda()
    x = guess.clone()
    out, state = M.pcg(d_val, d_off, d_col, d_b, preconditioner="ic0", reorder=True, x=x, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True)
    assert out is x and state["status"] == "CONVERGED"
    x0 = s.coloring.permute_vector(guess).cpu().numpy()
    want, _ = s.model(x0=x0)
    got, mine = s.solve(x0=x0)
    _equal(got, want)
    assert (state["status"], state["iterations"], state["rr"]) == (mine["status"], mine["iterations"], mine["rr"])
    back = s.coloring.permute_vector(torch.from_numpy(got[0]).cuda(), back=True).cpu().numpy()
    assert _same(out.cpu().numpy(), back)
    assert _true_residual(off, col, val, back, _rhs(s.n, NP[prec])) <= RESIDUAL[prec]
