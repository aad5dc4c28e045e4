"""What the BiCGStab tests share (tests/test_bicgstab_model.py, tests/test_bicgstab.py): the matrices, the right-hand sides and the
table of exits.  Nothing here calls the library."""
import numpy as np

GRIDS = [(24, 24), (40, 25)]
SIZES = [1, 3, 5, 1024, 1025, 4160]             # the banded matrix: one lane .. five workgroups, the last one partial; a lane across n
FOLD_N = 2 ** 20 + 1029                         # 1026 partials: the fold takes two levels; n % 4 == 1
FOLD_ITERATIONS = 3


def _csr(n, r, c, a, dtype):
    order = np.lexsort((c, r))
    off = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=off[1:])
    return off, c[order].astype(np.int32), a[order].astype(dtype)


def convection_diffusion(w, h, dtype):
    """The 5-point upwind-free convection-diffusion stencil of a w x h grid, rows sorted: -1.3 to the west, -0.7 to the east, -1.2 to
    the south, -0.8 to the north (nonsymmetric), and on the diagonal 4 + (i + 1) / (2 n + 1): every row's differs and none is a power
    of two, so a division by it is not exact and Jacobi is not a scaling."""
    n = w * h
    idx = np.arange(n).reshape(h, w)
    r = [idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel(), idx.ravel()]
    c = [idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel(), idx.ravel()]
    a = [np.full(r[0].size, -1.3), np.full(r[1].size, -0.7), np.full(r[2].size, -1.2), np.full(r[3].size, -0.8),
         4.0 + (np.arange(n) + 1.0) / (2 * n + 1)]
    return _csr(n, np.concatenate(r), np.concatenate(c), np.concatenate(a), dtype)


def banded(n, dtype, seed=3):
    """A nonsymmetric band: entries from (-1, -0.25) at the columns i - 3, i - 1, i + 1, i + 3 that exist, each drawn on its own; the
    diagonal is the row's sum of |off-diagonal| plus a draw from (0.5, 1.5) (strictly dominant: every solver here converges)"""
    rng = np.random.default_rng(seed)
    r, c = [], []
    for step in (-3, -1, 1, 3):
        i = np.arange(max(0, -step), min(n, n - step))
        r.append(i); c.append(i + step)
    r, c = np.concatenate(r).astype(np.int64), np.concatenate(c).astype(np.int64)
    a = rng.uniform(-1, -0.25, r.size).astype(dtype)
    diag = (np.bincount(r, weights=np.abs(a.astype(np.float64)), minlength=n) + rng.uniform(0.5, 1.5, n)).astype(dtype)
    here = np.arange(n)
    return _csr(n, np.concatenate([r, here]), np.concatenate([c, here]), np.concatenate([a, diag]), dtype)


def bidiagonal(n, dtype, seed=3):
    """the diagonal, drawn from (2, 3), and the one entry right of it, drawn from (-2, -1): barely dominant, so a few iterations do not
    converge"""
    rng = np.random.default_rng(seed)
    here = np.arange(n)
    d, u = rng.uniform(2, 3, n), rng.uniform(-2, -1, n - 1)
    return _csr(n, np.concatenate([here, here[:-1]]), np.concatenate([here, here[1:]]), np.concatenate([d, u]), dtype)


def dense_csr(a, dtype):
    """every entry of the dense matrix a stored, zeros too (so that every row has its diagonal entry)"""
    a = np.asarray(a, dtype)
    n = a.shape[0]
    return np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n), a.ravel().copy()


def rows_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def diagonal_of(off, col, val):
    at = np.flatnonzero(col == rows_of(off))
    assert at.size == len(off) - 1
    return val[at]


def rhs(n, dtype, seed=22):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)


def guess(n, dtype, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)


# name -> (A, b, max_iterations, status, iterations, exit): small systems whose every intermediate is exactly representable, so the
# exit is taken in exact arithmetic (fp32 and fp64 alike, with no preconditioner)
EXIT_CASES = {
    "rv": ([[0, 1], [2, -2]], [2, 0], 10, "BREAKDOWN", 0, "rv"),
    "tt": ([[0, 0], [1, -1]], [1, -1], 10, "BREAKDOWN", 1, "tt"),
    "omega": ([[2, -1], [-2, 0]], [-1, 0], 10, "BREAKDOWN", 1, "omega"),
    "rho": ([[0, 2, 1], [1, -1, 1], [-2, 0, 0]], [2, -2, 2], 10, "BREAKDOWN", 1, "rho"),
    "half": ([[3, 0], [0, 3]], [1, -2], 10, "CONVERGED", 1, "half"),
    "rr": ([[1, 0], [-1, -1]], [1, 0], 10, "CONVERGED", 1, "rr"),
    "start": ([[1, 2], [3, 4]], [0, 0], 10, "CONVERGED", 0, "start"),
    "none": ([[4, -1, 0], [-2, 4, -1], [0, -2, 4]], [1, 2, 3], 1, "RUNNING", 1, None),
}
