"""What Pcg, Bicgstab and Gmres share on the Python side: the loader of a layer library built on the C ABI, the solver base class (the
preconditioner's forms and checks, the state read-back, solve, close) and the one body of the one-shot functions pcg, bicgstab, gmres."""
from __future__ import annotations

import ctypes
import os

from ._lib import _HERE, MspmvError, _check, _prototype, load_library, use_library
from ._args import _Handle, _index_check, _pattern_check, _ptr, _stream_handle, _typed
from .solve import CsrSv, _Factor0
from .reorder import multicolor_reorder

_KINDS = {"none": 0, "jacobi": 1, "factor": 2}
PCG_STATUS = ("RUNNING", "CONVERGED", "BREAKDOWN")
_layers = {}               # file name -> ctypes.CDLL


def _product_library() -> ctypes.CDLL:
    """the product libmspmv.so, whatever library is active"""
    prev = use_library("product")
    try:
        return load_library()
    finally:
        use_library(prev)


def _load_layer(file_name: str, prototypes) -> ctypes.CDLL:
    """dlopen a layer library (built in-tree by `make -C merge_spmv_amd`), once.  The product library is loaded first, so that torch's
    HIP runtime and libmspmv.so are bound before the layer that needs both; fails loudly when absent."""
    if file_name not in _layers:
        path = os.path.join(_HERE, file_name)
        if not os.path.exists(path):
            raise MspmvError(f"{path} not found: build the HIP extension first "
                             f"(python -c 'import __graft_entry__ as g; g.build()' or make -C merge_spmv_amd)")
        _product_library()
        lib = ctypes.CDLL(path)
        _prototype(lib, prototypes)
        _layers[file_name] = lib
    return _layers[file_name]


class _KrylovSolver(_Handle):
    """A solver handle of one CSR pattern and value type.  A subclass states `_prefix` ("mspmv_<name>_"), `_State` (the ctypes state
    block), `_hidden` (the state field that is not shown), `_exits` (the names of exit_test, or None), `_product_plans` (whether a
    factor's plans must come from the product library), `_library()`, `launches_per_iteration` and, for more *_create arguments,
    `_create_extra()`."""

    _exits = None
    _product_plans = True

    def _create_extra(self):
        return ()

    def __init__(self, row_offsets, column_indices, dtype, preconditioner=None, stream=None, debug_synchronous: bool = False):
        import torch
        name = type(self).__name__
        self.device, self.rows, self.nnz = _pattern_check(name, row_offsets, column_indices)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name} is instantiated for float32 and float64, got {dtype}")
        self.dtype = dtype
        self.row_offsets, self.column_indices = row_offsets, column_indices
        self.history = None
        factor = None
        if preconditioner is None:
            kind = "none"
        elif isinstance(preconditioner, str):
            if preconditioner != "jacobi":
                raise MspmvError(f"{name}: unknown preconditioner {preconditioner!r}")
            kind = "jacobi"
        elif isinstance(preconditioner, _Factor0):
            preconditioner._ready("solve")
            kind, factor = "factor", (preconditioner.lower, preconditioner.upper, preconditioner._factor, preconditioner.row_offsets,
                                      preconditioner.column_indices)
        elif isinstance(preconditioner, (tuple, list)) and len(preconditioner) in (3, 5):
            kind, factor = "factor", tuple(preconditioner) + ((row_offsets, column_indices) if len(preconditioner) == 3 else ())
        else:
            raise MspmvError(f"{name}: preconditioner must be None, 'jacobi', an Ilu0 / Ic0 or (first CsrSv, second CsrSv, factor values)")
        self.kind = kind
        self._lib = self._library()
        self._destroy = self._prefix + "destroy"
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(getattr(self._lib, self._prefix + "create")(
                ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz, 4 if dtype == torch.float32 else 8,
                _KINDS[kind], *self._create_extra(), _stream_handle(stream), int(bool(debug_synchronous))), self._prefix + "create")
        self._handle = handle
        self._kept = (preconditioner, factor)                          # (the handle holds pointers into these)
        if factor is not None:
            first, second, fvalues, foff, fcols = factor
            if not isinstance(first, CsrSv) or not isinstance(second, CsrSv) or first._handle is None or second._handle is None:
                raise MspmvError(f"{name}: the factor's sweeps must be two open CsrSv plans")
            if self._product_plans and (first._lib is not _product_library() or second._lib is not _product_library()):
                raise MspmvError(f"{name}: the factor's plans must be made by the product library (use_library('product'))")
            if not isinstance(fvalues, torch.Tensor) or fvalues.dtype != dtype or fvalues.device != self.device or fvalues.dim() != 1 \
                    or not fvalues.is_contiguous() or fvalues.numel() != first.nnz or second.nnz != first.nnz:
                raise MspmvError(f"{name}: the factor values must be a contiguous 1-D {dtype} tensor of the plans' {first.nnz} entries on {self.device}")
            _pattern_check(f"{name} (factor)", foff, fcols)
            if foff.numel() != self.rows + 1 or fcols.numel() != first.nnz:
                raise MspmvError(f"{name}: the factor's pattern arrays do not fit its plans")
            _check(getattr(self._lib, self._prefix + "set_factor")(self._handle, first._handle, second._handle, _ptr(fvalues), _ptr(foff),
                                                                   _ptr(fcols)), self._prefix + "set_factor")

    def _state(self, stream=None):
        raw = self._State()
        _check(getattr(self._lib, self._prefix + "state")(self._live(), ctypes.byref(raw), _stream_handle(stream) if self.rows > 0 else None),
               self._prefix + "state")
        state = {name: getattr(raw, name) for name, _ in self._State._fields_ if name != self._hidden}
        state["status"] = PCG_STATUS[state["status"]]
        if self._exits is not None:
            state["exit"] = self._exits[raw.exit_test]
        return state

    @property
    def state(self):
        import torch
        if self.rows > 0:
            torch.cuda.synchronize(self.device)                        # (a replayed graph may have run on any stream)
        return self._state()

    def solve(self, values, b, x=None, rtol: float = 1e-8, atol: float = 0.0, max_iterations: int = 1000, check_every: int = 8,
              history=False, stream=None, debug_synchronous: bool = False):
        """Solves A x = b to rr <= max(rtol^2 bb, atol^2) or max_iterations; an infinite rr never counts as converged.  x: None (a new
        tensor, the start is +0) or a tensor that holds the guess and receives the solution.  check_every = 0: nothing is read back and
        the call is asynchronous (and capturable).  history: False, True (a new tensor of max_iterations + 1 entries, kept as
        .history) or such a tensor."""
        import torch
        what = type(self).__name__ + ".solve"
        handle = self._live()
        guess = x is not None
        if x is None:
            x = torch.empty(self.rows, dtype=self.dtype, device=self.device)
        for t, name, need in ((values, "values", self.nnz), (b, "b", self.rows), (x, "x", self.rows)):
            _index_check(what, t, name, need, self.device, (self.dtype,))
        if x.data_ptr() == b.data_ptr() and self.rows > 0:
            raise MspmvError(f"{what}: x must not be b")
        if history is True:
            history = torch.zeros(int(max_iterations) + 1, dtype=self.dtype, device=self.device)
        elif history is False or history is None:
            history = None
        elif not isinstance(history, torch.Tensor) or history.dtype != self.dtype or history.device != self.device or history.dim() != 1 \
                or not history.is_contiguous() or history.numel() < int(max_iterations) + 1:
            raise MspmvError(f"{what}: history must be a contiguous 1-D {self.dtype} tensor of at least max_iterations + 1 entries")
        self.history = history
        fn, _ = _typed(self._lib, self._prefix + "solve", self.dtype)
        with torch.cuda.device(self.device):
            _check(fn(handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), _ptr(b), _ptr(x), int(guess), float(rtol),
                      float(atol), int(max_iterations), int(check_every), _ptr(history), _stream_handle(stream), int(bool(debug_synchronous))),
                   self._prefix + "solve")
        return x

    def close(self):
        super().close()
        self._kept = None                                              # (the preconditioner lived as long as the handle pointed into it)


def _one_shot(what, solver_class, factor0, factork, factored, values, row_offsets, column_indices, b, preconditioner, reorder, x, rtol, atol,
              max_iterations, check_every, stream, return_state, fill_level, **solver_kw):
    """The body of pcg, bicgstab and gmres.  `factored`: the preconditioner's name that asks for a factorisation ("ic0" | "ilu0");
    factor0 / factork: its classes at fill level 0 and above."""
    if preconditioner not in (factored, "jacobi", None):
        raise MspmvError(f"{what}: unknown preconditioner {preconditioner!r}")
    if int(fill_level) < 0:
        raise MspmvError(f"{what}: fill_level must not be negative, got {fill_level}")
    coloring = m = None
    val, off, col, rhs, x0 = values, row_offsets, column_indices, b, x
    try:
        if reorder and preconditioner == factored:
            coloring, p = multicolor_reorder(values, row_offsets, column_indices, stream=stream)
            val, off, col = p.values, p.row_offsets, p.column_indices
            rhs = coloring.permute_vector(b, stream=stream)
            x0 = None if x is None else coloring.permute_vector(x, stream=stream)
        if preconditioner == factored:
            m = factork(off, col, int(fill_level), stream=stream) if int(fill_level) > 0 else factor0(off, col, stream=stream)
            m.factor(val, stream=stream)
        solver = solver_class(off, col, b.dtype, preconditioner="jacobi" if preconditioner == "jacobi" else m, stream=stream, **solver_kw)
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
        for h in (m, coloring):
            if h is not None:
                h.close()
    return (out, state) if return_state else out
