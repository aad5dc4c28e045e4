"""Right-preconditioned BiCGStab on the device (mspmv_bicgstab_* of include/mspmv_krylov.h), for nonsymmetric systems with ILU(0).

The solver is libmspmv_krylov.so, a layer on top of the C ABI: it has its own small table of prototypes here, on a CDLL of its own
(_solver._load_layer).  It ALWAYS runs on the product libmspmv.so next to it (its products and sweeps are that library's exports),
never on the development library, whatever use_library() has made active for the rest of the package."""
from __future__ import annotations

import ctypes

from ._lib import _F
from .solve import Ilu0, Iluk
from ._solver import _KrylovSolver, _load_layer, _one_shot


class _BicgstabState(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("launches_per_iteration", ctypes.c_int32),
                ("precond_kind", ctypes.c_int32), ("bad_diagonal_row", ctypes.c_int32), ("exit_test", ctypes.c_int32),
                ("rr", ctypes.c_double), ("bb", ctypes.c_double), ("stop2", ctypes.c_double), ("rho", ctypes.c_double),
                ("alpha", ctypes.c_double), ("omega", ctypes.c_double), ("device_bytes", ctypes.c_uint64)]


# every function of include/mspmv_krylov.h, in the letters of _lib._TOKENS (the state block goes as "p": ctypes.byref(_BicgstabState()))
_PROTOTYPES = (
    ("bicgstab_create", (), "H pp iiii pn"),
    ("bicgstab_set_factor", (), "p pp ppp"),
    ("bicgstab_solve", _F, "p ppp pp i dd ii p pn"),
    ("bicgstab_state", (), "p p p"),
    ("bicgstab_destroy", (), "p"),
)

BICGSTAB_EXIT = (None, "start", "half", "rr", "rv", "tt", "rr-nan", "omega", "rho")


def load_krylov_library() -> ctypes.CDLL:
    """libmspmv_krylov.so, loaded once after the product library; fails loudly when absent"""
    return _load_layer("libmspmv_krylov.so", _PROTOTYPES)


class Bicgstab(_KrylovSolver):
    """Right-preconditioned BiCGStab on the device (mspmv_bicgstab_*; include/mspmv_krylov.h states the arithmetic bit for bit) for one
    square CSR pattern and value type.  preconditioner: None, "jacobi", an Ilu0 or Ic0 that holds a factor (its two CsrSv plans and its
    factor are used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor
    column_indices]): M^-1 p = second^-1 (first^-1 p) (the pattern arrays default to the matrix's).  The constructor allocates and is
    synchronous.  `solve` returns x; `.state` then reads the state block back (synchronises): status ("RUNNING" | "CONVERGED" |
    "BREAKDOWN"), exit (one of BICGSTAB_EXIT: the test that ended the solve; None at max_iterations), iterations, rr, bb, stop2, rho,
    alpha, omega, launches_per_iteration, ...; `.history` (after solve(history=True)): the tensor of rr, entries 0 .. iterations."""

    _prefix, _State, _hidden, _exits = "mspmv_bicgstab_", _BicgstabState, "exit_test", BICGSTAB_EXIT
    _library = staticmethod(load_krylov_library)
    launches_per_iteration = 9


def bicgstab(values, row_offsets, column_indices, b, preconditioner="ilu0", reorder: bool = True, x=None, rtol: float = 1e-8,
             atol: float = 0.0, max_iterations: int = 1000, check_every: int = 8, stream=None, return_state: bool = False,
             fill_level: int = 0):
    """One-shot A x = b for a square CSR matrix (sorted rows, no duplicates; "ilu0" and "jacobi" need every diagonal entry stored).
    preconditioner: "ilu0" | "jacobi" | None.  With reorder (and "ilu0") the matrix is permuted to multicolour order
    (multicolor_reorder), ILU(0) is made of P A P^T, the system is solved in that numbering and x is mapped back
    (CsrColoring.permute_vector(back=True)): b, x, and a guess given as x, are in the caller's numbering.  fill_level > 0 (with
    "ilu0" only): ILU(fill_level) instead, an Iluk on the filled pattern of the matrix that is factorised (P A P^T with reorder).
    Returns x, or (x, state) with return_state.  A loop over right-hand sides or values keeps a Bicgstab (and the Ilu0 and
    CsrColoring) instead."""
    return _one_shot("bicgstab", Bicgstab, Ilu0, Iluk, "ilu0", values, row_offsets, column_indices, b, preconditioner, reorder, x, rtol, atol,
                     max_iterations, check_every, stream, return_state, fill_level)
