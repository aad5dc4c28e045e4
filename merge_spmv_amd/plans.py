"""The opt-in prepared plans of CsrMV -- the band-major copy (CsrMVPlan) and the hot-column renumbering (CsrMVHotColumns) -- and the
sub-records bench.py makes of them."""
from __future__ import annotations

import ctypes

from ._lib import MspmvError, _check, active_library, load_library, use_library
from ._args import _ptr, _stream_handle, _typed, _validate, _value_bytes
from .csrmv import csrmv
from .introspect import profile_begin, profile_end, set_band_passes


class CsrMVPlan:
    """The opt-in prepared plan (mspmv_csrmv_plan_*): a band-major copy of the matrix made once, so that every
    XCD gathers from an L2-sized slice of x.  For a matrix that is multiplied many times and whose x does not
    fit an XCD's 4 MiB L2; the stateless `csrmv` never uses it.  `plan(x, y)` computes y = alpha*A*x + beta*y.
    `storage`: a caller-provided uint8 tensor on the matrix's device of at least `bytes` bytes (mspmv_csrmv_plan_size) that the
    plan is built into, whatever it held before; by default the plan allocates its own.  `debug_synchronous`: the build prints
    its launch lines and synchronises after each, as the same argument of `plan(x, y)` does for an apply."""

    def __init__(self, values, row_offsets, column_indices, num_cols: int, bands: int = 0, stream=None, storage=None, debug_synchronous: bool = False):
        import torch
        self.rows, self.cols, self.nnz = row_offsets.numel() - 1, int(num_cols), values.numel()
        y_probe = torch.empty(0, dtype=values.dtype, device=values.device)
        _validate(values, row_offsets, column_indices, None, torch.empty(self.rows, dtype=values.dtype, device=values.device)
                  if self.rows == 0 else y_probe.new_empty(self.rows), self.rows, 0, self.nnz, "CsrMVPlan")
        self.dtype = values.dtype
        self.vb = _value_bytes(values)
        size = ctypes.c_size_t(0); used = ctypes.c_int32(0)
        _check(load_library().mspmv_csrmv_plan_size(self.rows, self.cols, self.nnz, self.vb, int(bands), ctypes.byref(size),
                                                    ctypes.byref(used)), "mspmv_csrmv_plan_size")
        self.bytes, self.bands = int(size.value), int(used.value)
        if storage is None:
            storage = torch.empty(max(self.bytes, 1), dtype=torch.uint8, device=values.device)
        elif storage.dtype != torch.uint8 or storage.device != values.device or storage.dim() != 1 or not storage.is_contiguous() \
                or storage.numel() < self.bytes or storage.data_ptr() % 16:
            raise MspmvError(f"CsrMVPlan: storage must be a contiguous 16-byte aligned uint8 tensor on {values.device} of at least {self.bytes} bytes")
        self.storage = storage
        fn, _ = _typed(load_library(), "mspmv_csrmv_plan_build", self.dtype)
        _check(fn(ctypes.c_void_p(self.storage.data_ptr()), self.bytes, _ptr(values), _ptr(row_offsets), _ptr(column_indices),
                  self.rows, self.cols, self.nnz, self.bands, _stream_handle(stream), int(bool(debug_synchronous))), "mspmv_csrmv_plan_build")

    def _view(self, fn, count, dtype):
        import torch
        ptr = fn(ctypes.c_void_p(self.storage.data_ptr()), self.rows, self.cols, self.nnz, self.vb, self.bands)
        if not ptr or count == 0:
            return torch.empty(0, dtype=dtype, device=self.storage.device)
        off = int(ptr) - self.storage.data_ptr()
        return self.storage[off: off + count * torch.empty(0, dtype=dtype).element_size()].view(dtype)

    def stacked(self):
        """(row_offsets, column_indices, values) of the stacked matrix A' = [A_0; ...; A_{bands-1}] (mspmv_csrmv_plan_row_offsets /
        _columns / _values): views of the plan's storage -- bands * rows + 1 offsets, nnz absolute column indices, nnz values"""
        import torch
        lib = load_library()
        return (self._view(lib.mspmv_csrmv_plan_row_offsets, self.bands * self.rows + 1, torch.int32),
                self._view(lib.mspmv_csrmv_plan_columns, self.nnz, torch.int32),
                self._view(lib.mspmv_csrmv_plan_values, self.nnz, self.dtype))

    def __call__(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, stream=None, debug_synchronous: bool = False):
        import torch
        if y is None:
            y = torch.empty(self.rows, dtype=self.dtype, device=self.storage.device)
        if x.dtype != self.dtype or y.dtype != self.dtype or x.device != self.storage.device or y.device != self.storage.device \
                or not x.is_contiguous() or not y.is_contiguous() or x.dim() != 1 or y.dim() != 1 \
                or x.numel() < self.cols or y.numel() < self.rows:
            raise MspmvError("CsrMVPlan: x / y must be contiguous 1-D tensors of the plan's dtype on its device, with at least cols / rows entries")
        fn, _ = _typed(load_library(), "mspmv_csrmv_plan_apply", self.dtype)
        _check(fn(ctypes.c_void_p(self.storage.data_ptr()), self.bytes, _ptr(x), _ptr(y), self.rows, self.cols, self.nnz, self.bands,
                  float(alpha), float(beta), _stream_handle(stream), int(bool(debug_synchronous))), "mspmv_csrmv_plan_apply")
        return y


class CsrMVHotColumns:
    """The opt-in hot-column plan (mspmv_csrmv_hotcols_*): the columns renumbered once by how often the matrix references
    them, so that the hot part of a huge x is contiguous and stays in the caches (scale-free graphs; BASELINE config 5).
    Values and row offsets are used from the caller's tensors (kept alive here); y is bit for bit the stateless result."""

    def __init__(self, values, row_offsets, column_indices, num_cols: int, stream=None):
        import torch
        self.rows, self.cols, self.nnz = row_offsets.numel() - 1, int(num_cols), values.numel()
        _validate(values, row_offsets, column_indices, None, torch.empty(self.rows, dtype=values.dtype, device=values.device),
                  self.rows, 0, self.nnz, "CsrMVHotColumns")
        self.dtype, self.vb = values.dtype, _value_bytes(values)
        self.values, self.row_offsets = values, row_offsets
        size = ctypes.c_size_t(0)
        _check(load_library().mspmv_csrmv_hotcols_size(self.rows, self.cols, self.nnz, self.vb, ctypes.byref(size)), "mspmv_csrmv_hotcols_size")
        self.bytes = int(size.value)
        self.storage = torch.empty(max(self.bytes, 1), dtype=torch.uint8, device=values.device)
        _check(load_library().mspmv_csrmv_hotcols_build(ctypes.c_void_p(self.storage.data_ptr()), self.bytes, _ptr(row_offsets), _ptr(column_indices),
                                                        self.rows, self.cols, self.nnz, self.vb, _stream_handle(stream), 0), "mspmv_csrmv_hotcols_build")

    def _view(self, fn, count):
        import torch
        ptr = fn(ctypes.c_void_p(self.storage.data_ptr()), self.rows, self.cols, self.nnz, self.vb)
        if not ptr or count == 0:
            return torch.empty(0, dtype=torch.int32, device=self.storage.device)
        off = int(ptr) - self.storage.data_ptr()
        return self.storage[off: off + 4 * count].view(torch.int32)

    def order(self):
        """order[k] = the original column that became column k"""
        return self._view(load_library().mspmv_csrmv_hotcols_order, self.cols)

    def columns(self):
        """the renumbered column indices"""
        return self._view(load_library().mspmv_csrmv_hotcols_columns, self.nnz)

    def permute(self, x, out=None, stream=None):
        """x in the plan's numbering (mspmv_csrmv_hotcols_permute_*): out[k] = x[order[k]]; pass the result to __call__(..., x_is_permuted=True)"""
        import torch
        if out is None:
            out = torch.empty(max(self.cols, 1), dtype=self.dtype, device=self.storage.device)[:self.cols]
        if x.dtype != self.dtype or out.dtype != self.dtype or not x.is_contiguous() or not out.is_contiguous() or x.numel() < self.cols or out.numel() < self.cols \
                or x.data_ptr() == out.data_ptr():
            raise MspmvError("CsrMVHotColumns.permute: x / out must be distinct contiguous tensors of the plan's dtype with at least cols entries")
        fn, _ = _typed(load_library(), "mspmv_csrmv_hotcols_permute", self.dtype)
        _check(fn(ctypes.c_void_p(self.storage.data_ptr()), self.bytes, _ptr(x), _ptr(out), self.rows, self.cols, self.nnz, _stream_handle(stream), 0),
               "mspmv_csrmv_hotcols_permute")
        return out

    def __call__(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, stream=None, debug_synchronous: bool = False, x_is_permuted: bool = False):
        import torch
        if y is None:
            y = torch.empty(self.rows, dtype=self.dtype, device=self.storage.device)
        if x.dtype != self.dtype or y.dtype != self.dtype or x.device != self.storage.device or y.device != self.storage.device \
                or not x.is_contiguous() or not y.is_contiguous() or x.dim() != 1 or y.dim() != 1 \
                or x.numel() < self.cols or y.numel() < self.rows:
            raise MspmvError("CsrMVHotColumns: x / y must be contiguous 1-D tensors of the plan's dtype on its device, with at least cols / rows entries")
        fn, _ = _typed(load_library(), "mspmv_csrmv_hotcols_apply_permuted" if x_is_permuted else "mspmv_csrmv_hotcols_apply", self.dtype)
        _check(fn(ctypes.c_void_p(self.storage.data_ptr()), self.bytes, _ptr(self.values), _ptr(self.row_offsets), _ptr(x), _ptr(y), self.rows, self.cols,
                  self.nnz, float(alpha), float(beta), _stream_handle(stream), int(bool(debug_synchronous))), "mspmv_csrmv_hotcols_apply")
        return y


def hotcols_bench_record(A, x, y_stateless, steps: int = 5, warmup: int = 2, peak_gbs: float = 8000.0) -> dict:
    """bench.py's `hot_column_plan` sub-record: set-up time, SpMV time (x permutation included), agreement with the stateless y."""
    import time
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    plan = CsrMVHotColumns(A.values, A.row_offsets, A.column_indices, A.cols)
    torch.cuda.synchronize(); setup_ms = (time.perf_counter() - t0) * 1e3
    y = torch.empty_like(y_stateless)
    for _ in range(max(warmup, 1)):
        plan(x, y)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        plan(x, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    vb = A.values.element_size()
    b_alg = A.nnz * (vb + 4) + (A.rows + 1) * 4 + A.rows * vb + A.cols * vb
    xp = plan.permute(x)
    yp = torch.empty_like(y_stateless)
    for _ in range(max(warmup, 1)):
        plan(xp, yp, x_is_permuted=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        plan(xp, yp, x_is_permuted=True)
    torch.cuda.synchronize()
    ms_p = (time.perf_counter() - t0) * 1e3 / steps
    permuted = {"api": "mspmv_csrmv_hotcols_permute_* once, mspmv_csrmv_hotcols_apply_permuted_* per SpMV (the caller keeps x in the plan's numbering)",
                "ms_per_step": round(ms_p, 5), "value": round(2.0 * A.nnz / (ms_p * 1e-3) / 1e9, 3), "frac": round(b_alg / (ms_p * 1e-3) / 1e9 / peak_gbs, 4),
                "bitwise_equal_to_apply": bool(torch.equal(yp, y))}
    return {"api": "mspmv_csrmv_hotcols_build once, then mspmv_csrmv_hotcols_apply_* per SpMV (opt-in; not the drop-in call)", "x_kept_permuted": permuted,
            "what": "columns renumbered by reference count (hot columns contiguous); x permuted once per SpMV, inside the timed call",
            "setup_ms": round(setup_ms, 3), "storage_bytes": plan.bytes, "ms_per_step": round(ms, 5),
            "value": round(2.0 * A.nnz / (ms * 1e-3) / 1e9, 3), "unit": "GFLOP/s",
            "roofline": {"bound": "hbm", "achieved": round(b_alg / (ms * 1e-3) / 1e9, 2), "peak": peak_gbs, "unit": "GB/s",
                         "frac": round(b_alg / (ms * 1e-3) / 1e9 / peak_gbs, 4),
                         "note": "algorithmic bytes of the ORIGINAL matrix / whole plan SpMV (x permutation + tile kernel)"},
            "bitwise_equal_to_stateless": bool(torch.equal(y, y_stateless)),
            "bitwise_equal_to_stateless_one_launch": _equal_to_one_launch(A, x, y),
            "bitwise_note": "the plan's y is bit for bit the stateless call's in its one-launch form; a stateless call that is a CANDIDATE for the "
                            "column-band passes (mspmv_get_band_passes > 1) runs the classic three launches, another association: compared "
                            "with mspmv_set_band_passes(vb, -1) in `bitwise_equal_to_stateless_one_launch`"}


def _equal_to_one_launch(A, x, y_plan) -> bool:
    """y_plan == the stateless call's y with the column-band candidacy switched off (mspmv_set_band_passes(vb, -1))"""
    import torch
    vb = A.values.element_size()
    prev = active_library()
    try:
        set_band_passes(vb, -1)               # (development library: the same kernels + the override)
        y = csrmv(A.values, A.row_offsets, A.column_indices, x, num_cols=A.cols)
        torch.cuda.synchronize()
    finally:
        set_band_passes(vb, 0)
        use_library(prev)
    return bool(torch.equal(y, y_plan))


def plan_bench_record(A, x, y_stateless, steps: int = 50, warmup: int = 5, peak_gbs: float = 8000.0) -> dict:
    """bench.py's `prepared_plan` sub-record: set-up time of the plan, its SpMV time on the same matrix,
    agreement with the stateless call's y."""
    import time
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    plan = CsrMVPlan(A.values, A.row_offsets, A.column_indices, A.cols)
    torch.cuda.synchronize(); setup_ms = (time.perf_counter() - t0) * 1e3
    y = torch.empty_like(y_stateless)
    for _ in range(max(warmup, 1)):
        plan(x, y)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        plan(x, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    profile_begin(steps)
    for _ in range(steps):
        plan(x, y)
    torch.cuda.synchronize()
    prof = profile_end()
    vb = A.values.element_size()
    b_alg = A.nnz * (vb + 4) + (A.rows + 1) * 4 + A.rows * vb + A.cols * vb
    diff = float((y.double() - y_stateless.double()).abs().max())
    scale = float(y_stateless.double().abs().max())
    return {"api": "mspmv_csrmv_plan_build_* once, then mspmv_csrmv_plan_apply_* per SpMV (opt-in; not the drop-in call)",
            "bands": plan.bands, "setup_ms": round(setup_ms, 3), "storage_bytes": plan.bytes,
            "ms_per_step": round(ms, 5), "value": round(2.0 * A.nnz / (ms * 1e-3) / 1e9, 3), "unit": "GFLOP/s",
            "tile_kernel_ms": round(prof["tile_ms"], 5),
            "roofline": {"bound": "hbm", "achieved": round(b_alg / (ms * 1e-3) / 1e9, 2), "peak": peak_gbs, "unit": "GB/s",
                         "frac": round(b_alg / (ms * 1e-3) / 1e9 / peak_gbs, 4),
                         "note": "algorithmic bytes of the ORIGINAL matrix / whole plan SpMV (tile kernel + fix-up + band fold)"},
            "max_abs_diff_vs_stateless": diff, "max_abs_y": scale}
