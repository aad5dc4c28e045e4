"""The drop-in call and its kin: DeviceSpmv.CsrMV (the mirror of cub::DeviceSpmv::CsrMV), the csrmv / csrmv_mixed / csrmm wrappers,
the caller-owned workspace and the stateless transposed product."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

from ._lib import MspmvError, _check, load_library
from ._args import _ptr, _stream_handle, _two_phase, _typed, _validate, _value_bytes
from .introspect import launch_info


class DeviceSpmv:
    """Mirror of ``cub::DeviceSpmv`` (reference cub/device/device_spmv.cuh:70-170)."""

    @staticmethod
    def CsrMV(d_temp_storage, temp_storage_bytes: int, d_values, d_row_offsets, d_column_indices,
              d_vector_x, d_vector_y, num_rows: int, num_cols: int, num_nonzeros: int,
              stream=None, debug_synchronous: bool = False, alpha: Optional[float] = None,
              beta: Optional[float] = None, _checked: bool = False) -> Tuple[int, int]:
        """y = A*x.  Returns ``(status, temp_storage_bytes)``.

        ``d_temp_storage is None`` -> size query only (no work), exactly like the
        reference (dispatch_spmv_orig.cuh:651-655); otherwise a uint8 CUDA tensor of
        at least the queried size.  All d_* arguments are CUDA tensors (int32
        offsets/indices, float32|float64 values/x/y).  ``alpha``/``beta`` select the
        y = alpha*A*x + beta*y extension (mspmv_csrmv_axpby_*); leave None for the
        reference semantics.  Wrong dtypes / devices / strides / lengths raise MspmvError
        before anything reaches the library.
        """
        lib = load_library()
        vb = _value_bytes(d_vector_y)             # (the hot path: the selection below stays inline, _typed would add a call's worth of work)
        size = ctypes.c_size_t(int(temp_storage_bytes))
        if d_temp_storage is None:
            temp_ptr = ctypes.c_void_p(0)
        else:
            if not _checked:
                _validate(d_values, d_row_offsets, d_column_indices, d_vector_x, d_vector_y, int(num_rows), int(num_cols),
                          int(num_nonzeros), "DeviceSpmv.CsrMV")
            if not d_temp_storage.is_cuda or not d_temp_storage.is_contiguous():
                raise MspmvError("DeviceSpmv.CsrMV: d_temp_storage must be a contiguous CUDA tensor")
            size = ctypes.c_size_t(min(int(temp_storage_bytes), d_temp_storage.numel() * d_temp_storage.element_size()))
            temp_ptr = ctypes.c_void_p(d_temp_storage.data_ptr())
        args = [temp_ptr, ctypes.byref(size), _ptr(d_values), _ptr(d_row_offsets), _ptr(d_column_indices),
                _ptr(d_vector_x), _ptr(d_vector_y), int(num_rows), int(num_cols), int(num_nonzeros)]
        if alpha is None and beta is None:
            fn = lib.mspmv_csrmv_f32 if vb == 4 else lib.mspmv_csrmv_f64
        else:
            fn = lib.mspmv_csrmv_axpby_f32 if vb == 4 else lib.mspmv_csrmv_axpby_f64
            ct = ctypes.c_float if vb == 4 else ctypes.c_double
            args += [ct(1.0 if alpha is None else alpha), ct(0.0 if beta is None else beta)]
        args += [_stream_handle(stream) if d_temp_storage is not None else ctypes.c_void_p(0),
                 int(bool(debug_synchronous))]
        status = fn(*args)
        return int(status), int(size.value)


class CsrMVWorkspace:
    """Caller-owned temp storage for repeated CsrMV calls on one matrix shape
    (what TestGpuMergeCsrmv does by hand, gpu_spmv.cu:385-398)."""

    def __init__(self, num_rows: int, num_nonzeros: int, dtype, device="cuda"):
        import torch
        self.rows, self.nnz, self.dtype = int(num_rows), int(num_nonzeros), dtype
        probe = torch.empty(0, dtype=dtype)
        self.value_bytes = _value_bytes(probe)
        info = launch_info(self.rows, self.nnz, self.value_bytes)
        self.bytes = int(info["temp_bytes"])
        self.buffer = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self._checked = None            # the tensors of the last validated csrmv call through this workspace
        self.prepared_for = None        # the row_offsets TENSOR the coordinates in `buffer` belong to
        self.prepared_info = None       # launch_info at prepare time (tile shape / flags / tile count)

    def prepare(self, row_offsets, stream=None):
        """Run the tile-coordinate pass once for this matrix (mspmv_csrmv_prepare); later
        ``csrmv(..., workspace=ws)`` calls with the SAME row_offsets tensor (identity, not address)
        and unchanged tuning skip it."""
        import torch
        if row_offsets.dtype != torch.int32 or not row_offsets.is_cuda or not row_offsets.is_contiguous() or \
                row_offsets.numel() < self.rows + 1:
            raise MspmvError("prepare: row_offsets must be a contiguous int32 CUDA tensor with rows + 1 entries")
        size = ctypes.c_size_t(self.bytes)
        _check(load_library().mspmv_csrmv_prepare(ctypes.c_void_p(self.buffer.data_ptr()), ctypes.byref(size), _ptr(row_offsets),
                                                  self.rows, self.nnz, self.value_bytes,
                                                  _stream_handle(stream), 0), "mspmv_csrmv_prepare")
        self.prepared_for = row_offsets           # keeps the tensor alive: its address cannot be recycled
        self.prepared_info = launch_info(self.rows, self.nnz, self.value_bytes)
        return self

    def is_prepared_for(self, row_offsets, rows: int, nnz: int, dtype) -> bool:
        return (self.prepared_for is row_offsets and rows == self.rows and nnz == self.nnz and dtype == self.dtype and
                self.prepared_info == launch_info(rows, nnz, self.value_bytes))


def csrmv(values, row_offsets, column_indices, x, y=None, num_cols: Optional[int] = None,
          workspace: Optional[CsrMVWorkspace] = None, stream=None, alpha=None, beta=None,
          debug_synchronous: bool = False, transpose: bool = False):
    """Convenience wrapper: size query + temp allocation + CsrMV.  Tensors must
    be contiguous CUDA tensors.  Returns y.  transpose=True: y = alpha*A^T*x + beta*y through the stateless
    mspmv_csrmv_transpose_* (x has rows entries, y cols; `workspace` is not used) -- a caller that multiplies by
    A^T more than once builds it once with CsrTranspose instead."""
    import torch
    if transpose:
        return _csrmv_transpose(values, row_offsets, column_indices, x, y, num_cols, stream, alpha, beta, debug_synchronous)
    if not values.is_cuda or not row_offsets.is_cuda or not x.is_cuda:
        raise MspmvError("csrmv needs CUDA (HIP) tensors: the merge-path kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise TypeError("row_offsets/column_indices must be int32 (OffsetT=int, gpu_spmv.cu:730,734)")
    rows = row_offsets.numel() - 1
    nnz = values.numel()
    cols = int(num_cols) if num_cols is not None else x.numel()
    if y is None:
        y = torch.empty(rows, dtype=values.dtype, device=values.device)
    if workspace is None:
        _validate(values, row_offsets, column_indices, x, y, rows, cols, nnz, "csrmv")
        workspace = CsrMVWorkspace(rows, nnz, values.dtype, device=values.device)
    else:
        if workspace.rows != rows or workspace.nnz != nnz or workspace.dtype != values.dtype:
            raise MspmvError("csrmv: the workspace was sized for another matrix shape or precision")
        # repeated calls with the very same tensor objects (a solver loop, a timing loop) are checked once: the
        # workspace keeps the checked tensors alive, so their identities cannot be recycled
        checked = workspace._checked
        if not (checked is not None and checked[0] is values and checked[1] is row_offsets and checked[2] is column_indices
                and checked[3] is x and checked[4] is y and checked[5] == cols):
            _validate(values, row_offsets, column_indices, x, y, rows, cols, nnz, "csrmv")
            workspace._checked = (values, row_offsets, column_indices, x, y, cols)
    if workspace.is_prepared_for(row_offsets, rows, nnz, values.dtype):
        # coordinates already in the workspace (CsrMVWorkspace.prepare): mspmv_csrmv_prepared_*
        vb = _value_bytes(values)                 # (the hot path again: inline, as in DeviceSpmv.CsrMV)
        fn = load_library().mspmv_csrmv_prepared_f32 if vb == 4 else load_library().mspmv_csrmv_prepared_f64
        ct = ctypes.c_float if vb == 4 else ctypes.c_double
        size = ctypes.c_size_t(workspace.bytes)
        status = fn(ctypes.c_void_p(workspace.buffer.data_ptr()), ctypes.byref(size), _ptr(values), _ptr(row_offsets),
                    _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz, ct(1.0 if alpha is None else alpha),
                    ct(0.0 if beta is None else beta), _stream_handle(stream), int(bool(debug_synchronous)))
        _check(int(status), "mspmv_csrmv_prepared")
        return y
    status, _ = DeviceSpmv.CsrMV(workspace.buffer, workspace.bytes, values, row_offsets, column_indices, x, y,
                                 rows, cols, nnz, stream=stream, debug_synchronous=debug_synchronous,
                                 alpha=alpha, beta=beta, _checked=True)
    _check(status, "mspmv_csrmv")
    return y


def _mixed_pair(values_dtype, x_dtype) -> str:
    """suffix of the mspmv_csrmv_mixed_* entry points for (stored dtype of the matrix values, compute dtype of x and y)"""
    import torch
    if (values_dtype, x_dtype) == (torch.float32, torch.float64):
        return "f32_f64"
    if (values_dtype, x_dtype) == (torch.bfloat16, torch.float32):
        return "bf16_f32"
    raise MspmvError(f"csrmv_mixed: values / x must be (float32, float64) or (bfloat16, float32), got ({values_dtype}, {x_dtype}); "
                     "equal dtypes go through csrmv")


def csrmv_mixed(values, row_offsets, column_indices, x, y=None, num_cols: Optional[int] = None,
                workspace: Optional[CsrMVWorkspace] = None, stream=None, alpha=None, beta=None,
                debug_synchronous: bool = False):
    """Mixed-precision CsrMV (mspmv_csrmv_mixed_*): y = alpha*A*x + beta*y with the matrix values STORED narrow -- float32
    values with float64 x / y, or bfloat16 values with float32 x / y -- and widened in registers; x, y, alpha, beta and
    every sum are in x's dtype.  Bit for bit what csrmv returns for values.to(x.dtype) (mspmv.h says when), on a third
    less of a stream.  `workspace`: a CsrMVWorkspace of the COMPUTE dtype (x.dtype); a prepared one routes to
    mspmv_csrmv_mixed_prepared_*.  Returns y."""
    import torch
    for t, name in ((values, "values"), (row_offsets, "row_offsets"), (column_indices, "column_indices"), (x, "x")):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"csrmv_mixed: {name} must be a tensor")
    pair = _mixed_pair(values.dtype, x.dtype)
    if not values.is_cuda or not row_offsets.is_cuda or not column_indices.is_cuda or not x.is_cuda:
        raise MspmvError("csrmv_mixed needs CUDA (HIP) tensors: the merge-path kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise MspmvError("csrmv_mixed: row_offsets / column_indices must be int32")
    if row_offsets.numel() < 1:
        raise MspmvError("csrmv_mixed: row_offsets needs rows + 1 entries")
    rows = row_offsets.numel() - 1
    nnz = values.numel()
    cols = int(num_cols) if num_cols is not None else x.numel()
    if y is None:
        y = torch.empty(rows, dtype=x.dtype, device=x.device)
    if workspace is None:
        _validate(values, row_offsets, column_indices, x, y, rows, cols, nnz, "csrmv_mixed", values_dtype=values.dtype)
        workspace = CsrMVWorkspace(rows, nnz, x.dtype, device=x.device)
    else:
        if workspace.rows != rows or workspace.nnz != nnz or workspace.dtype != x.dtype:
            raise MspmvError("csrmv_mixed: the workspace was sized for another matrix shape or compute precision")
        if workspace.buffer.device != x.device:
            raise MspmvError("csrmv_mixed: the workspace lives on another device")
        checked = workspace._checked
        if not (checked is not None and checked[0] is values and checked[1] is row_offsets and checked[2] is column_indices
                and checked[3] is x and checked[4] is y and checked[5] == cols):
            _validate(values, row_offsets, column_indices, x, y, rows, cols, nnz, "csrmv_mixed", values_dtype=values.dtype)
            workspace._checked = (values, row_offsets, column_indices, x, y, cols)
    prepared = workspace.is_prepared_for(row_offsets, rows, nnz, x.dtype)
    lib = load_library()
    fn = getattr(lib, ("mspmv_csrmv_mixed_prepared_" if prepared else "mspmv_csrmv_mixed_") + pair)
    ct = ctypes.c_double if x.dtype == torch.float64 else ctypes.c_float
    size = ctypes.c_size_t(workspace.bytes)
    status = fn(ctypes.c_void_p(workspace.buffer.data_ptr()), ctypes.byref(size), _ptr(values), _ptr(row_offsets),
                _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz, ct(1.0 if alpha is None else alpha),
                ct(0.0 if beta is None else beta), _stream_handle(stream), int(bool(debug_synchronous)))
    _check(int(status), fn.__name__)
    return y


def csrmm(values, row_offsets, column_indices, X, Y=None, alpha: float = 1.0, beta: float = 0.0, temp=None, stream=None,
          debug_synchronous: bool = False):
    """Y = alpha*A*X + beta*Y (mspmv_csrmm_*).  X: [cols, k] CUDA tensor, row-major (stride (ldx, 1));
    Y likewise [rows, k].  Returns Y."""
    import torch
    if not values.is_cuda or not X.is_cuda:
        raise MspmvError("csrmm needs CUDA (HIP) tensors: the merge-path kernels only run on the GPU")
    if X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1):
        raise MspmvError("X must be 2-D with unit stride along the right-hand-side index (row-major)")
    rows, nnz, k = row_offsets.numel() - 1, values.numel(), X.shape[1]
    if Y is None:
        Y = torch.empty(rows, k, dtype=values.dtype, device=values.device)
    if Y.dim() != 2 or (k > 1 and Y.stride(1) != 1) or Y.shape != (rows, k):
        raise MspmvError("Y must be a row-major [rows, k] tensor")
    _validate(values, row_offsets, column_indices, X, Y, rows, X.shape[0], nnz, "csrmm")
    fn, ct = _typed(load_library(), "mspmv_csrmm", values.dtype)
    ldx = X.stride(0) if X.shape[0] > 1 else max(k, 1)
    ldy = Y.stride(0) if Y.shape[0] > 1 else max(k, 1)
    if ldx < k or ldy < k:
        raise MspmvError("csrmm: leading dimensions must be at least k (no overlapping / broadcast rows)")
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), _ptr(X), int(ldx), _ptr(Y), int(ldy), rows, X.shape[0], nnz, k,
            ct(alpha), ct(beta))
    _two_phase(fn, "mspmv_csrmm", values.device, stream, args, temp=temp, debug_synchronous=debug_synchronous)
    return Y


def _csrmv_transpose(values, row_offsets, column_indices, x, y, num_cols, stream, alpha, beta, debug_synchronous):
    import torch
    if not values.is_cuda or not row_offsets.is_cuda or not x.is_cuda:
        raise MspmvError("csrmv needs CUDA (HIP) tensors: the merge-path kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise TypeError("row_offsets/column_indices must be int32 (OffsetT=int, gpu_spmv.cu:730,734)")
    if num_cols is None:
        raise MspmvError("csrmv(transpose=True) needs num_cols: y has one entry per column of A")
    rows, cols, nnz = row_offsets.numel() - 1, int(num_cols), values.numel()
    if y is None:
        y = torch.empty(cols, dtype=values.dtype, device=values.device)
    # the checks of the forward call with the roles of rows and cols swapped for the vectors: x has `rows` entries, y has `cols`
    _validate(values, row_offsets, column_indices, x, y, rows, cols, nnz, "csrmv(transpose=True)", x_rows=rows, y_rows=cols)
    fn, ct = _typed(load_library(), "mspmv_csrmv_transpose", values.dtype)
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz,
            ct(1.0 if alpha is None else alpha), ct(0.0 if beta is None else beta))
    _two_phase(fn, "mspmv_csrmv_transpose", values.device, stream, args, debug_synchronous=debug_synchronous)
    return y
