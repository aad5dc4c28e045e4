"""The deterministic dot product and preconditioned conjugate gradients on the device."""
from __future__ import annotations

import ctypes

from ._lib import MspmvError, _PcgState, _check, load_library
from ._args import _Handle, _index_check, _pattern_check, _ptr, _stream_handle, _two_phase, _typed
from .solve import CsrSv, Ic0, Ick, _Factor0
from .reorder import multicolor_reorder


def vec_dot(a, b, out=None, stream=None, temp=None):
    """The deterministic dot product (mspmv_vec_dot_*): a one-element tensor ON THE DEVICE holding R(a o b), the fixed tree that
    include/mspmv.h states; a is b gives the squared norm.  Nothing is read back; asynchronous on `stream`.  `temp`: a kept uint8
    tensor of at least the queried size (a captured call passes one, so that nothing is allocated)."""
    import torch
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float64) or t.dim() != 1 \
                or not t.is_contiguous():
            raise MspmvError(f"vec_dot: {name} must be a contiguous 1-D float32 / float64 CUDA tensor")
    if a.dtype != b.dtype or a.device != b.device or a.numel() != b.numel():
        raise MspmvError("vec_dot: a and b must agree in dtype, device and length")
    if out is None:
        out = torch.empty(1, dtype=a.dtype, device=a.device)
    if not isinstance(out, torch.Tensor) or out.dtype != a.dtype or out.device != a.device or out.numel() != 1:
        raise MspmvError("vec_dot: out must be a one-element tensor of a's dtype on a's device")
    fn, _ = _typed(load_library(), "mspmv_vec_dot", a.dtype)
    with torch.cuda.device(a.device):
        _two_phase(fn, "mspmv_vec_dot", a.device, stream, (_ptr(a), _ptr(b), a.numel(), ctypes.c_void_p(out.data_ptr())), temp=temp)
    return out


_PCG_KINDS = {"none": 0, "jacobi": 1, "factor": 2}
PCG_STATUS = ("RUNNING", "CONVERGED", "BREAKDOWN")


class Pcg(_Handle):
    """Preconditioned conjugate gradients on the device (mspmv_pcg_*; include/mspmv.h states the arithmetic bit for bit) for one CSR
    pattern and value type.  preconditioner: None, "jacobi", an Ic0 or Ilu0 that holds a factor (its two CsrSv plans and its factor are
    used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor column_indices]):
    z = second^-1 (first^-1 r) (the pattern arrays default to the matrix's).  The constructor allocates and is synchronous.
    `solve` returns x; `.state` then reads the state block back (synchronises): status ("RUNNING" | "CONVERGED" | "BREAKDOWN"),
    iterations, rr, bb, stop2, rz, launches_per_iteration, ...; `.history` (after solve(history=True)): the tensor of rr, entries
    0 .. iterations."""

    _destroy = "mspmv_pcg_destroy"

    def __init__(self, row_offsets, column_indices, dtype, preconditioner=None, stream=None, debug_synchronous: bool = False):
        import torch
        self.device, self.rows, self.nnz = _pattern_check("Pcg", row_offsets, column_indices)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"Pcg is instantiated for float32 and float64, got {dtype}")
        self.dtype = dtype
        self.row_offsets, self.column_indices = row_offsets, column_indices
        self.history = None
        factor = None
        if preconditioner is None:
            kind = "none"
        elif isinstance(preconditioner, str):
            if preconditioner != "jacobi":
                raise MspmvError(f"Pcg: unknown preconditioner {preconditioner!r}")
            kind = "jacobi"
        elif isinstance(preconditioner, _Factor0):
            preconditioner._ready("solve")
            kind, factor = "factor", (preconditioner.lower, preconditioner.upper, preconditioner._factor, preconditioner.row_offsets,
                                      preconditioner.column_indices)
        elif isinstance(preconditioner, (tuple, list)) and len(preconditioner) in (3, 5):
            kind, factor = "factor", tuple(preconditioner) + ((row_offsets, column_indices) if len(preconditioner) == 3 else ())
        else:
            raise MspmvError("Pcg: preconditioner must be None, 'jacobi', an Ic0 / Ilu0 or (first CsrSv, second CsrSv, factor values)")
        self.kind = kind
        self._lib = load_library()
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(self._lib.mspmv_pcg_create(ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz,
                                              4 if dtype == torch.float32 else 8, _PCG_KINDS[kind], _stream_handle(stream),
                                              int(bool(debug_synchronous))), "mspmv_pcg_create")
        self._handle = handle
        self._kept = (preconditioner, factor)                          # (the handle holds pointers into these)
        if factor is not None:
            first, second, fvalues, foff, fcols = factor
            if not isinstance(first, CsrSv) or not isinstance(second, CsrSv) or first._handle is None or second._handle is None:
                raise MspmvError("Pcg: the factor's sweeps must be two open CsrSv plans")
            if not isinstance(fvalues, torch.Tensor) or fvalues.dtype != dtype or fvalues.device != self.device or fvalues.dim() != 1 \
                    or not fvalues.is_contiguous() or fvalues.numel() != first.nnz or second.nnz != first.nnz:
                raise MspmvError(f"Pcg: the factor values must be a contiguous 1-D {dtype} tensor of the plans' {first.nnz} entries on {self.device}")
            _pattern_check("Pcg (factor)", foff, fcols)
            if foff.numel() != self.rows + 1 or fcols.numel() != first.nnz:
                raise MspmvError("Pcg: the factor's pattern arrays do not fit its plans")
            _check(self._lib.mspmv_pcg_set_factor(self._handle, first._handle, second._handle, _ptr(fvalues), _ptr(foff), _ptr(fcols)),
                   "mspmv_pcg_set_factor")

    def _state(self, stream=None):
        raw = _PcgState()
        _check(self._lib.mspmv_pcg_state(self._live(), ctypes.byref(raw), _stream_handle(stream) if self.rows > 0 else None), "mspmv_pcg_state")
        state = {name: getattr(raw, name) for name, _ in _PcgState._fields_ if name != "reserved"}
        state["status"] = PCG_STATUS[state["status"]]
        return state

    @property
    def state(self):
        import torch
        if self.rows > 0:
            torch.cuda.synchronize(self.device)                        # (a replayed graph may have run on any stream)
        return self._state()

    @property
    def launches_per_iteration(self) -> int:
        return 7 if self.kind == "factor" else 5

    def solve(self, values, b, x=None, rtol: float = 1e-8, atol: float = 0.0, max_iterations: int = 1000, check_every: int = 8,
              history=False, stream=None, debug_synchronous: bool = False):
        """Solves A x = b to rr <= max(rtol^2 bb, atol^2) or max_iterations; an infinite rr never counts as converged (an Inf in b ends
        BREAKDOWN: at 0 iterations, or at 1 with x all NaN).  x: None (a new tensor, the start is +0) or a tensor that holds the guess and receives the solution.
        check_every = 0: nothing is read back and the call is asynchronous (and capturable).  history: False, True (a new tensor of
        max_iterations + 1 entries, kept as .history) or such a tensor."""
        import torch
        handle = self._live()
        guess = x is not None
        if x is None:
            x = torch.empty(self.rows, dtype=self.dtype, device=self.device)
        for t, name, need in ((values, "values", self.nnz), (b, "b", self.rows), (x, "x", self.rows)):
            _index_check("Pcg.solve", t, name, need, self.device, (self.dtype,))
        if x.data_ptr() == b.data_ptr() and self.rows > 0:
            raise MspmvError("Pcg.solve: x must not be b")
        if history is True:
            history = torch.zeros(int(max_iterations) + 1, dtype=self.dtype, device=self.device)
        elif history is False or history is None:
            history = None
        elif not isinstance(history, torch.Tensor) or history.dtype != self.dtype or history.device != self.device or history.dim() != 1 \
                or not history.is_contiguous() or history.numel() < int(max_iterations) + 1:
            raise MspmvError(f"Pcg.solve: history must be a contiguous 1-D {self.dtype} tensor of at least max_iterations + 1 entries")
        self.history = history
        fn, _ = _typed(self._lib, "mspmv_pcg_solve", self.dtype)
        with torch.cuda.device(self.device):
            _check(fn(handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), _ptr(b), _ptr(x), int(guess), float(rtol),
                      float(atol), int(max_iterations), int(check_every), _ptr(history), _stream_handle(stream), int(bool(debug_synchronous))),
                   "mspmv_pcg_solve")
        return x

    def close(self):
        super().close()
        self._kept = None                                              # (the preconditioner lived as long as the handle pointed into it)


def pcg(values, row_offsets, column_indices, b, preconditioner="ic0", reorder: bool = True, x=None, rtol: float = 1e-8, atol: float = 0.0,
        max_iterations: int = 1000, check_every: int = 8, stream=None, return_state: bool = False, fill_level: int = 0):
    """One-shot A x = b for a symmetric positive definite CSR matrix (sorted rows, no duplicates, structurally symmetric for "ic0").
    preconditioner: "ic0" | "jacobi" | None.  With reorder (and "ic0") the matrix is permuted to multicolour order
    (multicolor_reorder), IC(0) is made of P A P^T, the system is solved in that numbering and x is mapped back
    (CsrColoring.permute_vector(back=True)): x, and a guess given as x, are in the caller's numbering.  fill_level > 0 (with "ic0"
    only): IC(fill_level) instead, an Ick on the filled pattern of the matrix that is factorised (P A P^T with reorder).  Returns x,
    or (x, state) with return_state.  A loop over right-hand sides or values keeps a Pcg (and the Ic0 and CsrColoring) instead."""
    if preconditioner not in ("ic0", "jacobi", None):
        raise MspmvError(f"pcg: unknown preconditioner {preconditioner!r}")
    if int(fill_level) < 0:
        raise MspmvError(f"pcg: fill_level must not be negative, got {fill_level}")
    coloring = ic = None
    val, off, col, rhs, x0 = values, row_offsets, column_indices, b, x
    try:
        if reorder and preconditioner == "ic0":
            coloring, p = multicolor_reorder(values, row_offsets, column_indices, stream=stream)
            val, off, col = p.values, p.row_offsets, p.column_indices
            rhs = coloring.permute_vector(b, stream=stream)
            x0 = None if x is None else coloring.permute_vector(x, stream=stream)
        m = None
        if preconditioner == "ic0":
            ic = Ick(off, col, int(fill_level), stream=stream) if int(fill_level) > 0 else Ic0(off, col, stream=stream)
            ic.factor(val, stream=stream)
            m = ic
        solver = Pcg(off, col, b.dtype, preconditioner="jacobi" if preconditioner == "jacobi" else m, stream=stream)
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
        for h in (ic, coloring):
            if h is not None:
                h.close()
    return (out, state) if return_state else out
