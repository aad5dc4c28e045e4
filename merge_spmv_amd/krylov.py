"""The deterministic dot product and preconditioned conjugate gradients on the device."""
from __future__ import annotations

import ctypes

from ._lib import MspmvError, _PcgState, load_library
from ._args import _ptr, _two_phase, _typed
from .solve import Ic0, Ick
from ._solver import PCG_STATUS, _KrylovSolver, _one_shot


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


class Pcg(_KrylovSolver):
    """Preconditioned conjugate gradients on the device (mspmv_pcg_*; include/mspmv.h states the arithmetic bit for bit) for one CSR
    pattern and value type.  preconditioner: None, "jacobi", an Ic0 or Ilu0 that holds a factor (its two CsrSv plans and its factor are
    used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor column_indices]):
    z = second^-1 (first^-1 r) (the pattern arrays default to the matrix's).  The constructor allocates and is synchronous.
    `solve` returns x (an Inf in b ends BREAKDOWN: at 0 iterations, or at 1 with x all NaN); `.state` then reads the state block back
    (synchronises): status ("RUNNING" | "CONVERGED" | "BREAKDOWN"), iterations, rr, bb, stop2, rz, launches_per_iteration, ...;
    `.history` (after solve(history=True)): the tensor of rr, entries 0 .. iterations."""

    _prefix, _State, _hidden = "mspmv_pcg_", _PcgState, "reserved"
    _product_plans = False                                             # (it is part of the library that is active)
    _library = staticmethod(load_library)

    @property
    def launches_per_iteration(self) -> int:
        return 7 if self.kind == "factor" else 5


def pcg(values, row_offsets, column_indices, b, preconditioner="ic0", reorder: bool = True, x=None, rtol: float = 1e-8, atol: float = 0.0,
        max_iterations: int = 1000, check_every: int = 8, stream=None, return_state: bool = False, fill_level: int = 0):
    """One-shot A x = b for a symmetric positive definite CSR matrix (sorted rows, no duplicates, structurally symmetric for "ic0").
    preconditioner: "ic0" | "jacobi" | None.  With reorder (and "ic0") the matrix is permuted to multicolour order
    (multicolor_reorder), IC(0) is made of P A P^T, the system is solved in that numbering and x is mapped back
    (CsrColoring.permute_vector(back=True)): x, and a guess given as x, are in the caller's numbering.  fill_level > 0 (with "ic0"
    only): IC(fill_level) instead, an Ick on the filled pattern of the matrix that is factorised (P A P^T with reorder).  Returns x,
    or (x, state) with return_state.  A loop over right-hand sides or values keeps a Pcg (and the Ic0 and CsrColoring) instead."""
    return _one_shot("pcg", Pcg, Ic0, Ick, "ic0", values, row_offsets, column_indices, b, preconditioner, reorder, x, rtol, atol,
                     max_iterations, check_every, stream, return_state, fill_level)
