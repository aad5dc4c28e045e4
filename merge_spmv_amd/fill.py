"""Level-of-fill patterns on the device (mspmv_csr_fill_* of include/mspmv_fill.h): the symbolic phase of ILU(p) / IC(p).

The pass is libmspmv_fill.so, a library of its own beside libmspmv.so: it has its own loader and its own small table of prototypes
here, on a CDLL of its own, as bicgstab.py and gmres.py have."""
from __future__ import annotations

import ctypes
import os

from ._lib import _F, _HERE, MspmvError, _check, _prototype, load_library
from ._args import _Handle, _index_check, _pattern_check, _ptr, _stream_handle, _typed

_FILL_NAME = "libmspmv_fill.so"
_fill = None

FILL_MAX_LEVEL = 32


class _CsrFillInfo(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("nnz", ctypes.c_int32), ("level", ctypes.c_int32), ("nnz_filled", ctypes.c_int32),
                ("max_level", ctypes.c_int32), ("reserved", ctypes.c_int32), ("device_bytes", ctypes.c_uint64)]


# every function of include/mspmv_fill.h, in the letters of _lib._TOKENS (the info block goes as "p": ctypes.byref(_CsrFillInfo()))
_PROTOTYPES = (
    ("csr_fill_create", (), "H pp iii pn"),
    ("csr_fill_info", (), "p p"),
    ("csr_fill_row_offsets csr_fill_column_indices csr_fill_levels csr_fill_source", (), "p", "p"),
    ("csr_fill_values", _F, "p pp pn"),
    ("csr_fill_destroy", (), "p"),
)


def fill_library_path() -> str:
    return os.path.join(_HERE, _FILL_NAME)


def load_fill_library() -> ctypes.CDLL:
    """dlopen libmspmv_fill.so (built in-tree by `make -C merge_spmv_amd`).  The package's library is loaded first, so that torch's HIP
    runtime is bound before the library that needs it; fails loudly when absent."""
    global _fill
    if _fill is not None:
        return _fill
    path = fill_library_path()
    if not os.path.exists(path):
        raise MspmvError(f"{path} not found: build the HIP extension first "
                         f"(python -c 'import __graft_entry__ as g; g.build()' or make -C merge_spmv_amd)")
    load_library()
    lib = ctypes.CDLL(path)
    _prototype(lib, _PROTOTYPES)
    _fill = lib
    return lib


class CsrFill(_Handle):
    """The level-of-fill pattern F_p of a square CSR pattern (sorted rows, no column twice; include/mspmv_fill.h states the
    definition): every position whose level is at most `level`, 0 <= level <= 32.  The constructor analyses the PATTERN (synchronous;
    the handle owns what it allocates).
    .row_offsets, .column_indices, .levels, .source (the entry's index in the given arrays, -1 for a fill entry): int32 tensors on the
    pattern's device -- COPIES of the handle's arrays, made once when first asked for and kept after close(); .nnz_filled; .info: the
    handle's figures (rows, nnz, level, nnz_filled, max_level, device_bytes).
    `values(values)` scatters the values of the given pattern into the filled one (+0.0 at fill entries): one launch, nothing
    allocated but a missing `out`, nothing read back."""

    _destroy = "mspmv_csr_fill_destroy"

    def __init__(self, row_offsets, column_indices, level: int, stream=None, debug_synchronous: bool = False):
        import torch
        self.device, self.rows, self.nnz = _pattern_check("CsrFill", row_offsets, column_indices)
        self.level = int(level)
        if not 0 <= self.level <= FILL_MAX_LEVEL:
            raise MspmvError(f"CsrFill: level must be in [0, {FILL_MAX_LEVEL}], got {level}")
        self._lib = load_fill_library()
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(self._lib.mspmv_csr_fill_create(ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz,
                                                   self.level, _stream_handle(stream), int(bool(debug_synchronous))),
                   "mspmv_csr_fill_create")
        self._handle = handle
        raw = _CsrFillInfo()
        _check(self._lib.mspmv_csr_fill_info(self._handle, ctypes.byref(raw)), "mspmv_csr_fill_info")
        self.info = {name: int(getattr(raw, name)) for name, _ in _CsrFillInfo._fields_ if name != "reserved"}
        self.nnz_filled = self.info["nnz_filled"]
        self._kept = {}

    def _array(self, name, count):
        if name not in self._kept:                                 # (copied once: a closed handle still shows what it was asked for before)
            self._kept[name] = self._int32_copy("mspmv_csr_fill_" + name, count)
        return self._kept[name]

    row_offsets = property(lambda self: self._array("row_offsets", self.rows + 1))
    column_indices = property(lambda self: self._array("column_indices", self.nnz_filled))
    levels = property(lambda self: self._array("levels", self.nnz_filled))
    source = property(lambda self: self._array("source", self.nnz_filled))

    def values(self, values, out=None, stream=None, debug_synchronous: bool = False):
        """out[e] = values[source[e]], +0.0 where source[e] is -1 (mspmv_csr_fill_values_*): values moved, never recomputed.  `out`:
        nnz_filled entries of values' dtype, any alignment of that type, not overlapping `values`.  Asynchronous on `stream`."""
        import torch
        handle = self._live()
        _index_check("CsrFill.values", values, "values", self.nnz, self.device, (torch.float32, torch.float64))
        if out is None:
            out = torch.empty(self.nnz_filled, dtype=values.dtype, device=self.device)
        _index_check("CsrFill.values", out, "out", self.nnz_filled, self.device, (values.dtype,))
        size = values.element_size()
        if self.nnz > 0 and self.nnz_filled > 0 and out.data_ptr() < values.data_ptr() + self.nnz * size \
                and values.data_ptr() < out.data_ptr() + self.nnz_filled * size:
            raise MspmvError("CsrFill.values: out must not overlap values")
        fn, _ = _typed(self._lib, "mspmv_csr_fill_values", values.dtype)
        with torch.cuda.device(self.device):
            _check(fn(handle, _ptr(values), _ptr(out), _stream_handle(stream), int(bool(debug_synchronous))), "mspmv_csr_fill_values")
        return out


def csr_fill(values, row_offsets, column_indices, level: int, stream=None):
    """One-shot fill: the generators.DeviceCsr of F_level with the given values scattered into it (+0.0 at fill entries; values None:
    structure only) and, as .levels, the level of every entry."""
    import torch
    from .generators import DeviceCsr
    fill = CsrFill(row_offsets, column_indices, level, stream=stream)
    try:
        filled = None if values is None else fill.values(values, stream=stream)
        csr = DeviceCsr(fill.rows, fill.rows, fill.row_offsets, fill.column_indices, filled)
        csr.levels = fill.levels
        return csr
    finally:
        (stream if stream is not None else torch.cuda.current_stream(fill.device)).synchronize()
        fill.close()
