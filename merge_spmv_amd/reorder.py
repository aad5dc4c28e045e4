"""Multicolour reordering: the deterministic colouring of a pattern (CsrColoring) and P A P^T through csr_permute."""
from __future__ import annotations

import ctypes

from ._lib import MspmvError, _CsrColorInfo, _check, load_library
from ._args import _Handle, _index_check, _pattern_check, _ptr, _stream_handle, _typed
from .convert import csr_permute


class CsrColoring(_Handle):
    """The deterministic multicolouring of a square CSR pattern (mspmv_csr_color_*; include/mspmv.h states the definition): u and v are
    neighbours when A[u,v] or A[v,u] is stored, and color[v] is the smallest colour that no neighbour of larger key holds, key(v) =
    priorities[v] << 32 | v (priorities: rows entries, int32 or uint32, their 32 bits read as unsigned; None: a hash of the index).  The
    constructor analyses the PATTERN (synchronous; the handle owns what it allocates).
    .colors, .order (the vertices sorted stably by colour), .inverse (inverse[order[i]] = i), .offsets (num_colors + 1 entries): int32
    tensors on the pattern's device (copies); .num_colors; .info: the handle's figures (colors, max_color_rows, rounds, edges, ...).
    `permute_vector(v)` is v[order], `permute_vector(v, back=True)` v[inverse]; csr_permute(..., row_perm=.order, col_map=.inverse) is
    P A P^T, whose LOWER CsrSv plan has at most num_colors levels."""

    _destroy = "mspmv_csr_color_destroy"

    def __init__(self, row_offsets, column_indices, priorities=None, stream=None, debug_synchronous: bool = False):
        import torch
        self.device, self.rows, self.nnz = _pattern_check("CsrColoring", row_offsets, column_indices)
        if priorities is not None:
            _index_check("CsrColoring", priorities, "priorities", self.rows, self.device,
                         (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()))
        self._lib = load_library()
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(self._lib.mspmv_csr_color_create(ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz,
                                                    _ptr(priorities), _stream_handle(stream), int(bool(debug_synchronous))),
                   "mspmv_csr_color_create")
        self._handle = handle
        raw = _CsrColorInfo()
        _check(self._lib.mspmv_csr_color_info(self._handle, ctypes.byref(raw)), "mspmv_csr_color_info")
        self.info = {name: int(getattr(raw, name)) for name, _ in _CsrColorInfo._fields_}
        self.num_colors = self.info["colors"]
        self._kept = {}

    def _array(self, name, count):
        if name not in self._kept:                                 # (copied once: a closed handle still shows what it was asked for before)
            self._kept[name] = self._int32_copy("mspmv_csr_color_" + name, count)
        return self._kept[name]

    colors = property(lambda self: self._array("colors", self.rows))
    order = property(lambda self: self._array("order", self.rows))
    inverse = property(lambda self: self._array("inverse", self.rows))
    offsets = property(lambda self: self._array("offsets", self.num_colors + 1))

    def permute_vector(self, v, back: bool = False, out=None, stream=None):
        """v[order] (the vector in the multicolour numbering), or with back=True v[inverse] (back in the original numbering), through
        mspmv_coo_to_csr_values_*.  Asynchronous on `stream`."""
        import torch
        _index_check("CsrColoring.permute_vector", v, "v", self.rows, self.device, (torch.float32, torch.float64))
        if out is None:
            out = torch.empty_like(v)
        if not isinstance(out, torch.Tensor) or out.dtype != v.dtype or out.device != v.device or out.dim() != 1 or not out.is_contiguous() \
                or out.numel() != self.rows or out.data_ptr() == v.data_ptr() and self.rows > 0:
            raise MspmvError("CsrColoring.permute_vector: out must be another contiguous tensor of v's dtype, length and device")
        index = self.inverse if back else self.order
        fn, _ = _typed(self._lib, "mspmv_coo_to_csr_values", v.dtype)
        _check(fn(_ptr(v), _ptr(index), _ptr(out), self.rows, _stream_handle(stream), 0), "mspmv_coo_to_csr_values")
        return out


def csr_color(row_offsets, column_indices, priorities=None):
    """One-shot colouring: (colors, num_colors) of the pattern (CsrColoring keeps the order, its inverse and the offsets too)."""
    coloring = CsrColoring(row_offsets, column_indices, priorities)
    try:
        return coloring.colors, coloring.num_colors
    finally:
        coloring.close()


def multicolor_reorder(values, row_offsets, column_indices, priorities=None, stream=None):
    """(coloring, csr): the CsrColoring of a square pattern and P A P^T = csr_permute(values, ..., row_perm=coloring.order,
    col_map=coloring.inverse).  Solve P A P^T x' = coloring.permute_vector(b); x = coloring.permute_vector(x', back=True)."""
    coloring = CsrColoring(row_offsets, column_indices, priorities, stream=stream)
    return coloring, csr_permute(values, row_offsets, column_indices, coloring.rows, row_perm=coloring.order, col_map=coloring.inverse,
                                 stream=stream)
