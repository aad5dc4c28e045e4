"""Right-preconditioned restarted GMRES(m) on the device (mspmv_gmres_* of include/mspmv_gmres.h), for nonsymmetric systems with ILU(0).

The solver is libmspmv_gmres.so, a layer on top of the C ABI: it has its own loader and its own small table of prototypes here, on
a CDLL of its own.  It ALWAYS runs on the product libmspmv.so next to it (its products and sweeps are that library's exports), never
on the development library, whatever use_library() has made active for the rest of the package."""
from __future__ import annotations

import ctypes
import os

from ._lib import _F, _HERE, MspmvError, _check, _prototype, load_library, use_library
from ._args import _Handle, _index_check, _pattern_check, _ptr, _stream_handle, _typed
from .solve import CsrSv, Ilu0, Iluk, _Factor0
from .reorder import multicolor_reorder
from .krylov import PCG_STATUS

_GMRES_NAME = "libmspmv_gmres.so"
_gmres = None


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

_KINDS = {"none": 0, "jacobi": 1, "factor": 2}
GMRES_EXIT = (None, "start", "rr", "beta", "d")
MAX_RESTART = 128


def _product_library() -> ctypes.CDLL:
    """the product libmspmv.so, whatever library is active"""
    prev = use_library("product")
    try:
        return load_library()
    finally:
        use_library(prev)


def load_gmres_library() -> ctypes.CDLL:
    """dlopen libmspmv_gmres.so (built in-tree by `make -C merge_spmv_amd`).  The product library is loaded first, so that torch's HIP
    runtime and libmspmv.so are bound before the layer that needs both; fails loudly when absent."""
    global _gmres
    if _gmres is not None:
        return _gmres
    path = os.path.join(_HERE, _GMRES_NAME)
    if not os.path.exists(path):
        raise MspmvError(f"{path} not found: build the HIP extension first "
                         f"(python -c 'import __graft_entry__ as g; g.build()' or make -C merge_spmv_amd)")
    _product_library()
    lib = ctypes.CDLL(path)
    _prototype(lib, _PROTOTYPES)
    _gmres = lib
    return lib


class Gmres(_Handle):
    """Right-preconditioned restarted GMRES(restart) on the device (mspmv_gmres_*; include/mspmv_gmres.h states the arithmetic bit for bit:
    classical Gram-Schmidt applied twice, Givens rotations, convergence declared on true residuals only) for one square CSR pattern and
    value type; 1 <= restart <= 128.  preconditioner: None, "jacobi", an Ilu0 or Ic0 that holds a factor (its two CsrSv plans and its
    factor are used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor
    column_indices]): M^-1 p = second^-1 (first^-1 p) (the pattern arrays default to the matrix's).  The constructor allocates and is
    synchronous.  `solve` returns x; `.state` then reads the state block back (synchronises): status ("RUNNING" | "CONVERGED" |
    "BREAKDOWN"), exit (one of GMRES_EXIT: the test that ended the solve; None when the slots of max_iterations are used up), iterations,
    slots, cycles, restart, rr, bb, stop2, beta, launches_per_iteration, launches_per_cycle, ...; `.history` (after
    solve(history=True)): entries 0 .. iterations -- true residuals rr where a cycle closed (the last entry always), the rotations'
    estimates between."""

    _destroy = "mspmv_gmres_destroy"

    def __init__(self, row_offsets, column_indices, dtype, preconditioner=None, restart: int = 30, stream=None,
                 debug_synchronous: bool = False):
        import torch
        self.device, self.rows, self.nnz = _pattern_check("Gmres", row_offsets, column_indices)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"Gmres is instantiated for float32 and float64, got {dtype}")
        if int(restart) != restart or not 1 <= restart <= MAX_RESTART:
            raise MspmvError(f"Gmres: restart must be an integer in 1 .. {MAX_RESTART}, got {restart!r}")
        self.dtype, self.restart = dtype, int(restart)
        self.row_offsets, self.column_indices = row_offsets, column_indices
        self.history = None
        factor = None
        if preconditioner is None:
            kind = "none"
        elif isinstance(preconditioner, str):
            if preconditioner != "jacobi":
                raise MspmvError(f"Gmres: unknown preconditioner {preconditioner!r}")
            kind = "jacobi"
        elif isinstance(preconditioner, _Factor0):
            preconditioner._ready("solve")
            kind, factor = "factor", (preconditioner.lower, preconditioner.upper, preconditioner._factor, preconditioner.row_offsets,
                                      preconditioner.column_indices)
        elif isinstance(preconditioner, (tuple, list)) and len(preconditioner) in (3, 5):
            kind, factor = "factor", tuple(preconditioner) + ((row_offsets, column_indices) if len(preconditioner) == 3 else ())
        else:
            raise MspmvError("Gmres: preconditioner must be None, 'jacobi', an Ilu0 / Ic0 or (first CsrSv, second CsrSv, factor values)")
        self.kind = kind
        self._lib = load_gmres_library()
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(self._lib.mspmv_gmres_create(ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz,
                                                4 if dtype == torch.float32 else 8, _KINDS[kind], self.restart, _stream_handle(stream),
                                                int(bool(debug_synchronous))), "mspmv_gmres_create")
        self._handle = handle
        self._kept = (preconditioner, factor)                          # (the handle holds pointers into these)
        if factor is not None:
            first, second, fvalues, foff, fcols = factor
            if not isinstance(first, CsrSv) or not isinstance(second, CsrSv) or first._handle is None or second._handle is None:
                raise MspmvError("Gmres: the factor's sweeps must be two open CsrSv plans")
            if first._lib is not _product_library() or second._lib is not _product_library():
                raise MspmvError("Gmres: the factor's plans must be made by the product library (use_library('product'))")
            if not isinstance(fvalues, torch.Tensor) or fvalues.dtype != dtype or fvalues.device != self.device or fvalues.dim() != 1 \
                    or not fvalues.is_contiguous() or fvalues.numel() != first.nnz or second.nnz != first.nnz:
                raise MspmvError(f"Gmres: the factor values must be a contiguous 1-D {dtype} tensor of the plans' {first.nnz} entries on {self.device}")
            _pattern_check("Gmres (factor)", foff, fcols)
            if foff.numel() != self.rows + 1 or fcols.numel() != first.nnz:
                raise MspmvError("Gmres: the factor's pattern arrays do not fit its plans")
            _check(self._lib.mspmv_gmres_set_factor(self._handle, first._handle, second._handle, _ptr(fvalues), _ptr(foff), _ptr(fcols)),
                   "mspmv_gmres_set_factor")

    def _state(self, stream=None):
        raw = _GmresState()
        _check(self._lib.mspmv_gmres_state(self._live(), ctypes.byref(raw), _stream_handle(stream) if self.rows > 0 else None),
               "mspmv_gmres_state")
        state = {name: getattr(raw, name) for name, _ in _GmresState._fields_ if name != "exit_test"}
        state["status"] = PCG_STATUS[state["status"]]
        state["exit"] = GMRES_EXIT[raw.exit_test]
        return state

    @property
    def state(self):
        import torch
        if self.rows > 0:
            torch.cuda.synchronize(self.device)                        # (a replayed graph may have run on any stream)
        return self._state()

    @property
    def launches_per_iteration(self) -> int:
        return 7

    def solve(self, values, b, x=None, rtol: float = 1e-8, atol: float = 0.0, max_iterations: int = 1000, check_every: int = 8,
              history=False, stream=None, debug_synchronous: bool = False):
        """Solves A x = b to a true residual rr <= max(rtol^2 bb, atol^2) or until the iteration slots of max_iterations are used up (a
        cycle that closes early forfeits the rest of its slots); an infinite rr never counts as converged.  x: None (a new tensor, the
        start is +0) or a tensor that holds the guess and receives the solution.  check_every = c: the state is read back once c inner
        slots were enqueued since the last look; 0: nothing is read back and the call is asynchronous (and capturable).  history: False, True (a new tensor of max_iterations + 1 entries, kept as
        .history) or such a tensor."""
        import torch
        handle = self._live()
        guess = x is not None
        if x is None:
            x = torch.empty(self.rows, dtype=self.dtype, device=self.device)
        for t, name, need in ((values, "values", self.nnz), (b, "b", self.rows), (x, "x", self.rows)):
            _index_check("Gmres.solve", t, name, need, self.device, (self.dtype,))
        if x.data_ptr() == b.data_ptr() and self.rows > 0:
            raise MspmvError("Gmres.solve: x must not be b")
        if history is True:
            history = torch.zeros(int(max_iterations) + 1, dtype=self.dtype, device=self.device)
        elif history is False or history is None:
            history = None
        elif not isinstance(history, torch.Tensor) or history.dtype != self.dtype or history.device != self.device or history.dim() != 1 \
                or not history.is_contiguous() or history.numel() < int(max_iterations) + 1:
            raise MspmvError(f"Gmres.solve: history must be a contiguous 1-D {self.dtype} tensor of at least max_iterations + 1 entries")
        self.history = history
        fn, _ = _typed(self._lib, "mspmv_gmres_solve", self.dtype)
        with torch.cuda.device(self.device):
            _check(fn(handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), _ptr(b), _ptr(x), int(guess), float(rtol),
                      float(atol), int(max_iterations), int(check_every), _ptr(history), _stream_handle(stream), int(bool(debug_synchronous))),
                   "mspmv_gmres_solve")
        return x

    def close(self):
        super().close()
        self._kept = None                                              # (the preconditioner lived as long as the handle pointed into it)


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
    if preconditioner not in ("ilu0", "jacobi", None):
        raise MspmvError(f"gmres: unknown preconditioner {preconditioner!r}")
    if int(fill_level) < 0:
        raise MspmvError(f"gmres: fill_level must not be negative, got {fill_level}")
    coloring = ilu = None
    val, off, col, rhs, x0 = values, row_offsets, column_indices, b, x
    try:
        if reorder and preconditioner == "ilu0":
            coloring, p = multicolor_reorder(values, row_offsets, column_indices, stream=stream)
            val, off, col = p.values, p.row_offsets, p.column_indices
            rhs = coloring.permute_vector(b, stream=stream)
            x0 = None if x is None else coloring.permute_vector(x, stream=stream)
        m = None
        if preconditioner == "ilu0":
            ilu = Iluk(off, col, int(fill_level), stream=stream) if int(fill_level) > 0 else Ilu0(off, col, stream=stream)
            ilu.factor(val, stream=stream)
            m = ilu
        solver = Gmres(off, col, b.dtype, preconditioner="jacobi" if preconditioner == "jacobi" else m, restart=restart, stream=stream)
        try:
            out = solver.solve(val, rhs, x=x0, rtol=rtol, atol=atol, max_iterations=max_iterations, check_every=check_every, stream=stream)
            if coloring is not None:
                out = coloring.permute_vector(out, back=True, out=x, stream=stream)
            elif x is not None:
                out = x
            state = solver._state(stream) if return_state else None
        finally:
            solver.close()
    finally:
        for h in (ilu, coloring):
            if h is not None:
                h.close()
    return (out, state) if return_state else out
