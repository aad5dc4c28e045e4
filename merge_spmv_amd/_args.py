"""What the wrappers share on the way to the C ABI: raw pointers and streams, the checks the ABI cannot make (it sees raw pointers),
the two-phase temp-storage call, the f32 / f64 selection and the life of a library-owned handle."""
from __future__ import annotations

import ctypes
from typing import Optional

from ._lib import MspmvError, _check


def _value_bytes(t) -> int:
    import torch
    if t.dtype == torch.float32:
        return 4
    if t.dtype == torch.float64:
        return 8
    raise TypeError(f"CsrMV is instantiated for float32 and float64 only (gpu_spmv.cu:730,734), got {t.dtype}")


def _typed(lib, stem: str, dtype):
    """(lib.<stem>_f32, c_float) or (lib.<stem>_f64, c_double) for a torch dtype: the function and the C type of its scalars"""
    import torch
    if dtype == torch.float32:
        return getattr(lib, stem + "_f32"), ctypes.c_float
    if dtype == torch.float64:
        return getattr(lib, stem + "_f64"), ctypes.c_double
    raise TypeError(f"CsrMV is instantiated for float32 and float64 only (gpu_spmv.cu:730,734), got {dtype}")


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _stream_handle(stream) -> ctypes.c_void_p:
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


def _validate(values, row_offsets, column_indices, x, y, rows: int, cols: int, nnz: int, what: str,
              x_rows: Optional[int] = None, y_rows: Optional[int] = None, values_dtype=None) -> None:
    """The checks the C ABI cannot make (it sees raw pointers): every csrmv / csrmm / DeviceSpmv.CsrMV
    call goes through here, so a wrong dtype, device, stride or length is an MspmvError instead of
    a reinterpretation of memory.  x / y may be 1-D (CsrMV) or 2-D row-major (SpMM)."""
    import torch
    dev = y.device if y is not None else values.device
    if dev.type != "cuda":
        raise MspmvError(f"{what} needs CUDA (HIP) tensors: the merge-path kernels only run on the GPU")
    if y is None or y.dtype not in (torch.float32, torch.float64):
        raise MspmvError(f"{what}: y must be a float32 or float64 tensor (gpu_spmv.cu:730,734)")
    if rows < 0 or cols < 0 or nnz < 0:
        raise MspmvError(f"{what}: negative size")
    for t, name, need in ((row_offsets, "row_offsets", rows + 1), (column_indices, "column_indices", nnz)):
        if need == 0 and (t is None or t.numel() == 0):
            continue
        if t is None or t.dtype != torch.int32:
            raise MspmvError(f"{what}: {name} must be int32 (OffsetT=int, gpu_spmv.cu:730,734), got {None if t is None else t.dtype}")
        if t.device != dev or not t.is_contiguous() or t.numel() < need:
            raise MspmvError(f"{what}: {name} must be a contiguous tensor on {dev} with at least {need} entries")
    if nnz > 0:
        vdt = y.dtype if values_dtype is None else values_dtype       # (csrmv_mixed: the matrix is stored narrower than y)
        if values is None or values.dtype != vdt or values.device != dev or not values.is_contiguous() or values.numel() < nnz:
            raise MspmvError(f"{what}: values must be a contiguous {vdt} tensor on {dev} with at least {nnz} entries")
    for t, name, need in ((x, "x", cols if x_rows is None else x_rows), (y, "y", rows if y_rows is None else y_rows)):
        if t is None:
            if need == 0 or (name == "x" and nnz == 0):
                continue
            raise MspmvError(f"{what}: {name} is missing")
        if t.dtype != y.dtype or t.device != dev:
            raise MspmvError(f"{what}: {name} must be {y.dtype} on {dev}, got {t.dtype} on {t.device}")
        if t.dim() == 1:
            if t.numel() > 1 and t.stride(0) != 1:
                raise MspmvError(f"{what}: {name} must have unit stride")
            if t.numel() < need and not (name == "x" and nnz == 0):
                raise MspmvError(f"{what}: {name} has {t.numel()} entries, needs {need}")
        elif t.dim() == 2:
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise MspmvError(f"{what}: {name} must be row-major (unit stride along the right-hand-side index)")
            if t.shape[0] < need and not (name == "x" and nnz == 0):
                raise MspmvError(f"{what}: {name} has {t.shape[0]} rows, needs {need}")
        else:
            raise MspmvError(f"{what}: {name} must be 1-D or 2-D")


def _pattern_check(what, row_offsets, column_indices, int32_error=MspmvError):
    """the checks the C ABI cannot make for a CSR pattern; returns (device, rows, nnz).  int32_error: what another index type raises
    (the solves and factorisations raise TypeError there)"""
    import torch
    for t, name in ((row_offsets, "row_offsets"), (column_indices, "column_indices")):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"{what}: {name} must be a tensor")
    if not (row_offsets.is_cuda and column_indices.is_cuda):
        raise MspmvError(f"{what} needs CUDA (HIP) tensors: the kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise int32_error(f"{what}: row_offsets / column_indices must be int32")
    if row_offsets.dim() != 1 or row_offsets.numel() < 1 or not row_offsets.is_contiguous() or column_indices.dim() != 1 \
            or not column_indices.is_contiguous() or column_indices.device != row_offsets.device:
        raise MspmvError(f"{what}: row_offsets (rows + 1 entries) and column_indices must be contiguous 1-D tensors on one device")
    return row_offsets.device, row_offsets.numel() - 1, column_indices.numel()


def _index_check(what, t, name, need, dev, dtypes=None):
    """one 1-D array of exactly `need` entries on `dev`: int32 unless `dtypes` names others"""
    import torch
    dtypes = dtypes or (torch.int32,)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or t.device != dev or t.dim() != 1 \
            or not t.is_contiguous() or t.numel() != need:
        raise MspmvError(f"{what}: {name} must be a contiguous 1-D {' / '.join(str(d) for d in dtypes)} tensor of {need} entries on {dev}")


def _coo_check(values, row_indices, column_indices, what: str):
    """the checks the C ABI cannot make for COO input; returns (device, value dtype, nnz)"""
    import torch
    for t, name in ((row_indices, "row_indices"), (column_indices, "column_indices")):
        if t is None or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1:
            raise MspmvError(f"{what}: {name} must be a contiguous 1-D int32 CUDA tensor")
    dev, nnz = row_indices.device, row_indices.numel()
    if column_indices.device != dev or column_indices.numel() != nnz:
        raise MspmvError(f"{what}: column_indices must have row_indices' {nnz} entries on {dev}")
    if values is not None:
        if values.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{what} is instantiated for float32 and float64 only, got {values.dtype}")
        if values.device != dev or not values.is_contiguous() or values.dim() != 1 or values.numel() != nnz:
            raise MspmvError(f"{what}: values must be a contiguous 1-D tensor of {nnz} entries on {dev}")
    return dev, (torch.float32 if values is None else values.dtype), nnz


def _many_layout(what, values, B, X) -> int:
    """the refusals of solve_many / csrsm that need neither a plan nor a device: B (and X) 2-D, row-major, of one value type; returns k"""
    import torch
    for t, name in ((values, "values"), (B, "B")) + (((X, "X"),) if X is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"{what}: {name} must be a tensor")
    for t, name in ((B, "B"),) + (((X, "X"),) if X is not None else ()):
        if t.dim() != 2 or t.shape[1] < 1:
            raise MspmvError(f"{what}: {name} must be 2-D, [rows, k] with k >= 1")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise MspmvError(f"{what}: {name} must have unit stride along the right-hand-side index (row-major)")
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise MspmvError(f"{what}: the leading dimension of {name} (stride(0)) must be at least k (no overlapping / broadcast rows)")
    if B.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} is instantiated for float32 and float64, got {B.dtype}")
    if values.dtype != B.dtype:
        raise TypeError(f"{what}: values hold {values.dtype}, B {B.dtype}")
    if X is not None and X.dtype != B.dtype:
        raise TypeError(f"{what}: X must be a {B.dtype} tensor")
    return int(B.shape[1])


def _two_phase(fn, what, dev, stream, args, temp=None, debug_synchronous: bool = False):
    """The temp-storage convention of the C ABI in one place: size query, temp allocation (or the caller's `temp` when it is large
    enough), the call on `stream`; returns the temp tensor.  A temp allocated HERE for a torch side stream is record_stream'd (the
    allocator must not hand it out again before the work on `stream` has run); a caller's `temp` never is."""
    import torch
    size = ctypes.c_size_t(0)
    _check(fn(ctypes.c_void_p(0), ctypes.byref(size), *args, ctypes.c_void_p(0), 0), what + " (size query)")
    fresh = temp is None or temp.numel() < size.value
    if fresh:
        temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=dev)
    size = ctypes.c_size_t(temp.numel())
    _check(fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), *args, _stream_handle(stream), int(bool(debug_synchronous))), what)
    if fresh and stream is not None and hasattr(stream, "cuda_stream"):
        temp.record_stream(stream)
    return temp


class _PlanArray:
    """library-owned device memory seen by torch (torch.as_tensor reads __cuda_array_interface__: no copy)"""

    def __init__(self, ptr: int, count: int, typestr: str = "<i4"):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


class _Handle:
    """The life of one library-owned handle (a plan, a colouring, a solver).  A subclass names its C destructor in `_destroy`, sets
    `_lib` (the library that made the handle: the one that must destroy it, whatever is active by then) and, once its *_create has
    succeeded, `_handle`.  close() destroys once; __del__ never raises and finds nothing to do when the constructor raised before
    the handle existed."""

    _destroy = None         # "mspmv_..._destroy"
    _lib = None
    _handle = None

    def _live(self):
        """the handle, or MspmvError once it is closed"""
        if self._handle is None:
            raise MspmvError(f"{type(self).__name__}: closed")
        return self._handle

    def _int32_copy(self, getter: str, count: int):
        """a copy of `count` int32 entries the handle owns on self.device, read through the C accessor `getter`; zeros where it holds none"""
        import torch
        ptr = getattr(self._lib, getter)(self._live())
        if not ptr or count == 0:
            return torch.zeros(count, dtype=torch.int32, device=self.device)
        return torch.as_tensor(_PlanArray(ptr, count), device=self.device).clone()

    def close(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            getattr(self._lib, self._destroy)(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
