"""Right-preconditioned restarted GMRES(m) on the device (mspmv_gmres_* of include/mspmv_gmres.h), for nonsymmetric systems with ILU(0).

The solver is libmspmv_gmres.so, a layer on top of the C ABI: it has its own small table of prototypes here, on a CDLL of its own
(_solver._load_layer).  It ALWAYS runs on the product libmspmv.so next to it (its products and sweeps are that library's exports),
never on the development library, whatever use_library() has made active for the rest of the package."""
from __future__ import annotations

import ctypes

from ._lib import _F, MspmvError
from .solve import Ilu0, Iluk
from ._solver import _KrylovSolver, _load_layer, _one_shot


class _GmresState(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("slots", ctypes.c_int32), ("cycles", ctypes.c_int32),
                ("restart", ctypes.c_int32), ("launches_per_iteration", ctypes.c_int32), ("launches_per_cycle", ctypes.c_int32),
                ("precond_kind", ctypes.c_int32), ("bad_diagonal_row", ctypes.c_int32), ("exit_test", ctypes.c_int32),
                ("rr", ctypes.c_double), ("bb", ctypes.c_double), ("stop2", ctypes.c_double), ("beta", ctypes.c_double),
                ("device_bytes", ctypes.c_uint64)]


# every function of include/mspmv_gmres.h, in the letters of _lib._TOKENS (the state block goes as "p": ctypes.byref(_GmresState()))
_PROTOTYPES = (
    ("gmres_create", (), "H pp iiiii pn"),
    ("gmres_set_factor", (), "p pp ppp"),
    ("gmres_solve", _F, "p ppp pp i dd ii p pn"),
    ("gmres_state", (), "p p p"),
    ("gmres_destroy", (), "p"),
)

GMRES_EXIT = (None, "start", "rr", "beta", "d")
MAX_RESTART = 128


def load_gmres_library() -> ctypes.CDLL:
    """libmspmv_gmres.so, loaded once after the product library; fails loudly when absent"""
    return _load_layer("libmspmv_gmres.so", _PROTOTYPES)


class Gmres(_KrylovSolver):
    """Right-preconditioned restarted GMRES(restart) on the device (mspmv_gmres_*; include/mspmv_gmres.h states the arithmetic bit for bit:
    classical Gram-Schmidt applied twice, Givens rotations, convergence declared on true residuals only) for one square CSR pattern and
    value type; 1 <= restart <= 128.  preconditioner: None, "jacobi", an Ilu0 or Ic0 that holds a factor (its two CsrSv plans and its
    factor are used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor
    column_indices]): M^-1 p = second^-1 (first^-1 p) (the pattern arrays default to the matrix's).  The constructor allocates and is
    synchronous.  `solve` returns x: rr is a true residual, max_iterations counts iteration slots (a cycle that closes early forfeits
    the rest of its slots), and check_every = c reads the state back once c inner slots were enqueued since the last look.  `.state`
    then reads the state block back (synchronises): status ("RUNNING" | "CONVERGED" | "BREAKDOWN"), exit (one of GMRES_EXIT: the test
    that ended the solve; None when the slots of max_iterations are used up), iterations, slots, cycles, restart, rr, bb, stop2, beta,
    launches_per_iteration, launches_per_cycle, ...; `.history` (after solve(history=True)): entries 0 .. iterations -- true residuals
    rr where a cycle closed (the last entry always), the rotations' estimates between."""

    _prefix, _State, _hidden, _exits = "mspmv_gmres_", _GmresState, "exit_test", GMRES_EXIT
    _library = staticmethod(load_gmres_library)
    launches_per_iteration = 7

    def __init__(self, row_offsets, column_indices, dtype, preconditioner=None, restart: int = 30, stream=None,
                 debug_synchronous: bool = False):
        if int(restart) != restart or not 1 <= restart <= MAX_RESTART:
            raise MspmvError(f"Gmres: restart must be an integer in 1 .. {MAX_RESTART}, got {restart!r}")
        self.restart = int(restart)
        super().__init__(row_offsets, column_indices, dtype, preconditioner, stream, debug_synchronous)

    def _create_extra(self):
        return (self.restart,)


def gmres(values, row_offsets, column_indices, b, preconditioner="ilu0", reorder: bool = True, restart: int = 30, x=None,
          rtol: float = 1e-8, atol: float = 0.0, max_iterations: int = 1000, check_every: int = 8, stream=None, return_state: bool = False,
          fill_level: int = 0):
    """One-shot A x = b for a square CSR matrix (sorted rows, no duplicates; "ilu0" and "jacobi" need every diagonal entry stored).
    preconditioner: "ilu0" | "jacobi" | None.  With reorder (and "ilu0") the matrix is permuted to multicolour order
    (multicolor_reorder), ILU(0) is made of P A P^T, the system is solved in that numbering and x is mapped back
    (CsrColoring.permute_vector(back=True)): b, x, and a guess given as x, are in the caller's numbering.  fill_level > 0 (with
    "ilu0" only): ILU(fill_level) instead, an Iluk on the filled pattern of the matrix that is factorised (P A P^T with reorder).
    Returns x, or (x, state) with return_state.  A loop over right-hand sides or values keeps a Gmres (and the Ilu0 and CsrColoring)
    instead."""
    return _one_shot("gmres", Gmres, Ilu0, Iluk, "ilu0", values, row_offsets, column_indices, b, preconditioner, reorder, x, rtol, atol,
                     max_iterations, check_every, stream, return_state, fill_level, restart=restart)
