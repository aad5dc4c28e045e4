"""The passes that build one CSR matrix from another representation or from other matrices: transpose, COO -> CSR, duplicate
summing, coomv, addition, product, permutation -- and SDDMM, which fills the values of a given pattern."""
from __future__ import annotations

import ctypes
from typing import Optional

from ._lib import MspmvError, _check, load_library
from ._args import _coo_check, _index_check, _pattern_check, _ptr, _stream_handle, _two_phase, _typed, _validate
from .csrmv import CsrMVWorkspace, csrmm, csrmv


def csr_transpose(values, row_offsets, column_indices, num_cols: int, stream=None):
    """A^T as CSR on the device (mspmv_csr_transpose_*): returns (values_t, row_offsets_t, column_indices_t, permutation) with
    values_t[j] = values[permutation[j]]; the entries of each row of A^T in their order in A (stable), so the result is canonical.
    values=None: the structure only (values_t is None).  Asynchronous on `stream`."""
    import torch
    dev, rows, nnz = _pattern_check("csr_transpose", row_offsets, column_indices)
    cols = int(num_cols)
    dtype = torch.float32 if values is None else values.dtype
    probe = torch.empty(0, dtype=dtype, device=dev)
    if values is None:              # structure only: the pattern is checked, cols is left
        _validate(None, row_offsets, None, None, probe, rows, cols, 0, "csr_transpose", x_rows=0, y_rows=0)
    else:
        nnz = values.numel()
        _validate(values, row_offsets, column_indices, None, probe, rows, cols, nnz, "csr_transpose", x_rows=0, y_rows=0)
    fn, _ = _typed(load_library(), "mspmv_csr_transpose", dtype)
    values_t = None if values is None else torch.empty(nnz, dtype=dtype, device=dev)
    row_offsets_t = torch.empty(cols + 1, dtype=torch.int32, device=dev)
    column_indices_t = torch.empty(nnz, dtype=torch.int32, device=dev)
    permutation = torch.empty(nnz, dtype=torch.int32, device=dev)
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), rows, cols, nnz, _ptr(values_t), ctypes.c_void_p(row_offsets_t.data_ptr()),
            _ptr(column_indices_t), _ptr(permutation))
    _two_phase(fn, "mspmv_csr_transpose", dev, stream, args)
    return values_t, row_offsets_t, column_indices_t, permutation


class CsrTranspose:
    """A^T built once on the device (csr_transpose) for a caller that multiplies by it many times: holds A^T's tensors, the
    permutation and a CsrMVWorkspace prepared for A^T.  `t(x, y)` computes y = alpha*A^T*x + beta*y with the ordinary forward call on
    A^T (x has A's rows entries, y A's cols); `t.matmul(X, Y)` is csrmm on A^T; `t.refresh_values(values)` takes new values on the
    same pattern."""

    def __init__(self, values, row_offsets, column_indices, num_cols: int, stream=None):
        self.rows, self.cols, self.nnz = row_offsets.numel() - 1, int(num_cols), values.numel()
        self.dtype = values.dtype
        self.values_t, self.row_offsets_t, self.column_indices_t, self.permutation = \
            csr_transpose(values, row_offsets, column_indices, num_cols, stream=stream)
        self.workspace = CsrMVWorkspace(self.cols, self.nnz, self.dtype, device=values.device).prepare(self.row_offsets_t, stream=stream)

    def refresh_values(self, values, stream=None):
        """values_t[j] = values[permutation[j]] (mspmv_csr_transpose_values_*) for new values on A's pattern."""
        if values.dtype != self.dtype or values.device != self.values_t.device or not values.is_contiguous() or values.numel() != self.nnz:
            raise MspmvError(f"CsrTranspose.refresh_values: values must be a contiguous {self.dtype} tensor of {self.nnz} entries on "
                             f"{self.values_t.device}")
        fn, _ = _typed(load_library(), "mspmv_csr_transpose_values", values.dtype)
        _check(fn(_ptr(values), _ptr(self.permutation), _ptr(self.values_t), self.nnz, _stream_handle(stream), 0),
               "mspmv_csr_transpose_values")
        return self

    def __call__(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, stream=None):
        return csrmv(self.values_t, self.row_offsets_t, self.column_indices_t, x, y, num_cols=self.rows, workspace=self.workspace,
                     stream=stream, alpha=alpha, beta=beta)

    def matmul(self, X, Y=None, alpha: float = 1.0, beta: float = 0.0, stream=None):
        return csrmm(self.values_t, self.row_offsets_t, self.column_indices_t, X, Y, alpha=alpha, beta=beta, stream=stream)


def csr_sum_duplicates(values, row_offsets, column_indices, num_cols: int, stream=None):
    """Merges the duplicate entries of a CSR whose rows are sorted by column (mspmv_csr_sum_duplicates_*): each run of equal (row,
    column) becomes one entry, its values added left to right in the value type.  Returns (values_out, row_offsets_out,
    column_indices_out, count): the arrays keep nnz entries, of which the first `count` (a one-element int32 CUDA tensor) are
    written.  values=None: structure only.  Asynchronous on `stream`; nothing is read back."""
    import torch
    dev, rows, nnz = _pattern_check("csr_sum_duplicates", row_offsets, column_indices)
    cols = int(num_cols)
    if values is not None:
        _index_check("csr_sum_duplicates", values, "values", nnz, dev, (torch.float32, torch.float64))
    dtype = torch.float32 if values is None else values.dtype
    fn, _ = _typed(load_library(), "mspmv_csr_sum_duplicates", dtype)
    values_out = None if values is None else torch.empty(nnz, dtype=dtype, device=dev)
    row_offsets_out = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    column_indices_out = torch.empty(nnz, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    args = (_ptr(values), ctypes.c_void_p(row_offsets.data_ptr()), _ptr(column_indices), rows, cols, nnz, _ptr(values_out),
            ctypes.c_void_p(row_offsets_out.data_ptr()), _ptr(column_indices_out), ctypes.c_void_p(count.data_ptr()))
    _two_phase(fn, "mspmv_csr_sum_duplicates", dev, stream, args)
    return values_out, row_offsets_out, column_indices_out, count


def coo_to_csr(values, row_indices, column_indices, num_rows: int, num_cols: int, stream=None, sum_duplicates: bool = False,
               return_permutation: bool = False, _temp=None):
    """CSR from unsorted COO triples on the device (mspmv_coo_to_csr_*): the entries sorted stably by (row, column), duplicates kept
    next to each other in input order -- a generators.DeviceCsr (values=None: structure only, .values is None).  With
    return_permutation=True returns (csr, permutation): csr entry j is input entry permutation[j].  Asynchronous on `stream`.
    sum_duplicates=True also merges equal (row, column) entries, adding left to right (mspmv_csr_sum_duplicates_*), reads the new
    count back -- the ONLY synchronising step -- and narrows the arrays to it; the permutation still describes the build before merging."""
    import torch
    from .generators import DeviceCsr
    dev, dtype, nnz = _coo_check(values, row_indices, column_indices, "coo_to_csr")
    rows, cols = int(num_rows), int(num_cols)
    fn, _ = _typed(load_library(), "mspmv_coo_to_csr", dtype)
    row_offsets = torch.empty(max(rows, 0) + 1, dtype=torch.int32, device=dev)
    cols_csr = torch.empty(nnz, dtype=torch.int32, device=dev)
    values_csr = None if values is None else torch.empty(nnz, dtype=dtype, device=dev)
    permutation = torch.empty(nnz, dtype=torch.int32, device=dev) if return_permutation else None
    args = (_ptr(values), _ptr(row_indices), _ptr(column_indices), rows, cols, nnz, ctypes.c_void_p(row_offsets.data_ptr()), _ptr(cols_csr),
            _ptr(values_csr), _ptr(permutation))
    _two_phase(fn, "mspmv_coo_to_csr", dev, stream, args, temp=_temp)
    if sum_duplicates:
        v, o, c, count = csr_sum_duplicates(values_csr, row_offsets, cols_csr, cols, stream=stream)
        if stream is not None and hasattr(stream, "synchronize"):
            stream.synchronize()
        n = int(count.item())
        values_csr, row_offsets, cols_csr = (None if v is None else v[:n]), o, c[:n]
    csr = DeviceCsr(rows, cols, row_offsets, cols_csr, values_csr)
    return (csr, permutation) if return_permutation else csr


class CooToCsr:
    """A CSR built once from COO triples (coo_to_csr) for a caller whose values change on a fixed pattern: holds the CSR's tensors,
    the permutation and the build's temp storage.  `b.refresh_values(values)` takes new values in the triples' order
    (mspmv_coo_to_csr_values_*); `b.rebuild(values, row_indices, column_indices)` runs the build again for new triples of the same
    count into the same tensors; `b(x, y)` computes y = alpha*A*x + beta*y with the forward call."""

    def __init__(self, values, row_indices, column_indices, num_rows: int, num_cols: int, stream=None):
        import torch
        dev, self.dtype, self.nnz = _coo_check(values, row_indices, column_indices, "CooToCsr")
        if values is None:
            raise MspmvError("CooToCsr needs values (coo_to_csr builds the structure alone)")
        self.rows, self.cols = int(num_rows), int(num_cols)
        self._fn, _ = _typed(load_library(), "mspmv_coo_to_csr", self.dtype)
        self.row_offsets = torch.empty(self.rows + 1, dtype=torch.int32, device=dev)
        self.column_indices = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.values = torch.empty(self.nnz, dtype=self.dtype, device=dev)
        self.permutation = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.temp = None
        self.rebuild(values, row_indices, column_indices, stream=stream)

    def rebuild(self, values, row_indices, column_indices, stream=None):
        dev, dtype, nnz = _coo_check(values, row_indices, column_indices, "CooToCsr.rebuild")
        if values is None or dtype != self.dtype or nnz != self.nnz or dev != self.values.device:
            raise MspmvError(f"CooToCsr.rebuild: needs {self.nnz} triples with {self.dtype} values on {self.values.device}")
        args = (_ptr(values), _ptr(row_indices), _ptr(column_indices), self.rows, self.cols, self.nnz,
                ctypes.c_void_p(self.row_offsets.data_ptr()), _ptr(self.column_indices), _ptr(self.values), _ptr(self.permutation))
        self.temp = _two_phase(self._fn, "mspmv_coo_to_csr", dev, stream, args, temp=self.temp)
        return self

    def refresh_values(self, values, stream=None):
        """values_csr[j] = values[permutation[j]] (mspmv_coo_to_csr_values_*) for new values on the same triples."""
        if values.dtype != self.dtype or values.device != self.values.device or not values.is_contiguous() or values.numel() != self.nnz:
            raise MspmvError(f"CooToCsr.refresh_values: values must be a contiguous {self.dtype} tensor of {self.nnz} entries on "
                             f"{self.values.device}")
        fn, _ = _typed(load_library(), "mspmv_coo_to_csr_values", values.dtype)
        _check(fn(_ptr(values), _ptr(self.permutation), _ptr(self.values), self.nnz, _stream_handle(stream), 0), "mspmv_coo_to_csr_values")
        return self

    def __call__(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, stream=None):
        return csrmv(self.values, self.row_offsets, self.column_indices, x, y, num_cols=self.cols, stream=stream, alpha=alpha, beta=beta)


def coomv(values, row_indices, column_indices, x, y=None, num_rows: Optional[int] = None, num_cols: Optional[int] = None, stream=None,
          alpha=None, beta=None, debug_synchronous: bool = False):
    """y = alpha*A*x + beta*y from unsorted COO triples through the stateless mspmv_coomv_* (duplicates add): the CSR is built inside
    every call -- a caller that multiplies more than once builds it once (coo_to_csr / CooToCsr).  num_rows defaults to y's length,
    num_cols to x's.  Returns y."""
    import torch
    dev, dtype, nnz = _coo_check(values, row_indices, column_indices, "coomv")
    if values is None:
        raise MspmvError("coomv needs values")
    if num_rows is None and y is None:
        raise MspmvError("coomv needs num_rows or y")
    rows = int(num_rows) if num_rows is not None else y.numel()
    cols = int(num_cols) if num_cols is not None else x.numel()
    if y is None:
        y = torch.empty(rows, dtype=dtype, device=dev)
    for t, name, need in ((x, "x", cols), (y, "y", rows)):
        if t is None or t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != 1 or t.numel() < need:
            raise MspmvError(f"coomv: {name} must be a contiguous 1-D {dtype} tensor of at least {need} entries on {dev}")
    fn, ct = _typed(load_library(), "mspmv_coomv", dtype)
    args = (_ptr(values), _ptr(row_indices), _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz, ct(1.0 if alpha is None else alpha),
            ct(0.0 if beta is None else beta))
    _two_phase(fn, "mspmv_coomv", dev, stream, args, debug_synchronous=debug_synchronous)
    return y


def _add_check(m, name: str, what: str):
    """the checks the C ABI cannot make for one addend (a generators.DeviceCsr or anything with its five fields); returns nnz"""
    import torch
    off, col, val = m.row_offsets, m.column_indices, m.values
    if off is None or not off.is_cuda or off.dtype != torch.int32 or not off.is_contiguous() or off.dim() != 1 or off.numel() != int(m.rows) + 1:
        raise MspmvError(f"{what}: {name}.row_offsets must be a contiguous 1-D int32 CUDA tensor of rows + 1 entries")
    if col is None or col.dtype != torch.int32 or col.device != off.device or not col.is_contiguous() or col.dim() != 1:
        raise MspmvError(f"{what}: {name}.column_indices must be a contiguous 1-D int32 tensor on {off.device}")
    if val is not None:
        if val.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{what} is instantiated for float32 and float64 only, got {val.dtype}")
        if val.device != off.device or not val.is_contiguous() or val.dim() != 1 or val.numel() != col.numel():
            raise MspmvError(f"{what}: {name}.values must be a contiguous 1-D tensor of {col.numel()} entries on {off.device}")
    return col.numel()


class CsrAdd:
    """C = alpha*A + beta*B on the device (mspmv_csr_add_*) with the outputs and the temp storage allocated ONCE, so that `add()` can
    be captured in a graph and replayed after the addends' tensors were overwritten in place (new values, or a new pattern of the same
    counts).  a, b: generators.DeviceCsr of the same shape, rows sorted by column without repeated columns; values for both or for
    neither (structure only).  Holds row_offsets (rows + 1), column_indices and values (nnz_a + nnz_b entries, of which the first
    `count` -- a one-element int32 CUDA tensor -- are written) and reads nothing back; `trimmed()` waits for the stream the last
    `add()` ran on, reads the count and returns the DeviceCsr narrowed to it."""

    def __init__(self, a, b, alpha: float = 1.0, beta: float = 1.0, stream=None):
        import torch
        self.nnz_a, self.nnz_b = _add_check(a, "a", "csr_add"), _add_check(b, "b", "csr_add")
        if (int(a.rows), int(a.cols)) != (int(b.rows), int(b.cols)):
            raise MspmvError(f"csr_add: a is {a.rows} x {a.cols}, b is {b.rows} x {b.cols}")
        if (a.values is None) != (b.values is None):
            raise MspmvError("csr_add: values for both matrices or for neither (structure only)")
        dev = a.row_offsets.device
        if b.row_offsets.device != dev:
            raise MspmvError(f"csr_add: b must be on {dev}")
        if a.values is not None and a.values.dtype != b.values.dtype:
            raise MspmvError(f"csr_add: a holds {a.values.dtype}, b {b.values.dtype}")
        self.a, self.b, self.rows, self.cols = a, b, int(a.rows), int(a.cols)
        self.alpha, self.beta = float(alpha), float(beta)
        self.dtype = torch.float32 if a.values is None else a.values.dtype
        self._fn, self._ct = _typed(load_library(), "mspmv_csr_add", self.dtype)
        n = self.nnz_a + self.nnz_b
        self.row_offsets = torch.empty(self.rows + 1, dtype=torch.int32, device=dev)
        self.column_indices = torch.empty(n, dtype=torch.int32, device=dev)
        self.values = None if a.values is None else torch.empty(n, dtype=self.dtype, device=dev)
        self.count = torch.empty(1, dtype=torch.int32, device=dev)
        self.temp = None
        self._stream = None
        self.add(stream=stream)

    def add(self, stream=None, alpha=None, beta=None):
        """runs the addition on the addends' tensors as they are now, into the same outputs; asynchronous on `stream`"""
        a, b = self.a, self.b
        if _add_check(a, "a", "CsrAdd.add") != self.nnz_a or _add_check(b, "b", "CsrAdd.add") != self.nnz_b:
            raise MspmvError(f"CsrAdd.add: the addends must keep their {self.nnz_a} and {self.nnz_b} entries")
        ct = self._ct
        args = (self.rows, self.cols, ct(self.alpha if alpha is None else alpha), _ptr(a.values), _ptr(a.row_offsets), _ptr(a.column_indices),
                self.nnz_a, ct(self.beta if beta is None else beta), _ptr(b.values), _ptr(b.row_offsets), _ptr(b.column_indices), self.nnz_b,
                _ptr(self.values), ctypes.c_void_p(self.row_offsets.data_ptr()), _ptr(self.column_indices),
                ctypes.c_void_p(self.count.data_ptr()))
        self.temp = _two_phase(self._fn, "mspmv_csr_add", self.row_offsets.device, stream, args, temp=self.temp)
        self._stream = stream
        return self

    def trimmed(self):
        from .generators import DeviceCsr
        if self._stream is not None and hasattr(self._stream, "synchronize"):
            self._stream.synchronize()                           # (the count is read on the current stream: wait for add()'s first)
        n = int(self.count.item())
        return DeviceCsr(self.rows, self.cols, self.row_offsets, self.column_indices[:n], None if self.values is None else self.values[:n])


def csr_add(a, b, alpha: float = 1.0, beta: float = 1.0, stream=None, trim: bool = False):
    """C = alpha*A + beta*B for two generators.DeviceCsr of the same shape whose rows are sorted by column without repeated columns
    (mspmv_csr_add_*): C's pattern is the union of the two patterns whatever the values, its values alpha*a, beta*b or
    (alpha*a) + (beta*b), each operation rounded on its own.  values None in both: structure only.  Returns (c, count): c a
    DeviceCsr whose column_indices / values keep nnz_a + nnz_b entries, of which the first `count` (a one-element int32 CUDA tensor)
    are written.  Asynchronous on `stream`; nothing is read back -- unless trim=True, which reads the count (the ONLY synchronising
    step) and narrows the arrays to it."""
    from .generators import DeviceCsr
    op = CsrAdd(a, b, alpha=alpha, beta=beta, stream=stream)
    if trim:
        return op.trimmed(), op.count
    return DeviceCsr(op.rows, op.cols, op.row_offsets, op.column_indices, op.values), op.count


def csr_symmetrize(a, stream=None):
    """A + A^T of a square DeviceCsr (the undirected graph of an edge list): csr_add(a, csr_transpose(a)), trimmed to its count."""
    from .generators import DeviceCsr
    if int(a.rows) != int(a.cols):
        raise MspmvError(f"csr_symmetrize: the matrix must be square, got {a.rows} x {a.cols}")
    vt, ot, ct, _ = csr_transpose(a.values, a.row_offsets, a.column_indices, a.cols, stream=stream)
    return csr_add(a, DeviceCsr(a.cols, a.rows, ot, ct, vt), stream=stream, trim=True)[0]


_MAX_ITEMS = 2 ** 31 - 1 - 65536


def _gemm_check(a, b, what: str):
    """the checks the C ABI cannot make for the two factors of a product; returns (nnz_a, nnz_b, device)"""
    nnz_a, nnz_b = _add_check(a, "a", what), _add_check(b, "b", what)
    if int(a.cols) != int(b.rows):
        raise MspmvError(f"{what}: a is {a.rows} x {a.cols}, b is {b.rows} x {b.cols}")
    dev = a.row_offsets.device
    if b.row_offsets.device != dev:
        raise MspmvError(f"{what}: b must be on {dev}")
    if (a.values is None) != (b.values is None):
        raise MspmvError(f"{what}: values for both matrices or for neither (structure only)")
    if a.values is not None and a.values.dtype != b.values.dtype:
        raise MspmvError(f"{what}: a holds {a.values.dtype}, b {b.values.dtype}")
    return nnz_a, nnz_b, dev


def csr_gemm_products(a, b, stream=None) -> int:
    """The number of scalar products a_ik * b_kj of A * B (mspmv_csr_gemm_products): the sum over A's entries of the length of the
    row of B they point at, exact in 64 bits.  Reads the count back: it SYNCHRONISES with `stream`."""
    import torch
    nnz_a, nnz_b, dev = _gemm_check(a, b, "csr_gemm_products")
    out = torch.empty(1, dtype=torch.int64, device=dev)
    args = (_ptr(a.row_offsets), _ptr(a.column_indices), int(a.rows), int(a.cols), nnz_a, _ptr(b.row_offsets), nnz_b,
            ctypes.c_void_p(out.data_ptr()))
    _two_phase(load_library().mspmv_csr_gemm_products, "mspmv_csr_gemm_products", dev, stream, args)
    if stream is not None and hasattr(stream, "synchronize"):
        stream.synchronize()
    return int(out.item())


class CsrGemm:
    """C = A * B on the device (mspmv_csr_gemm_*) with the outputs and the temp storage allocated ONCE, so that calling the object
    again can be captured in a graph and replayed after the factors' tensors were overwritten in place (new values, or new patterns
    of the same sizes and the same number of products).  a: generators.DeviceCsr of rows x inner, b: of inner x cols, any valid CSR
    (rows need not be sorted, columns may repeat); values for both or for neither (structure only).  products: the count of
    csr_gemm_products(a, b), which is called (and synchronises) when it is None.  capacity: the entries column_indices / values
    hold, `products` by default (always enough); 0 is the symbolic phase.  Holds row_offsets (rows + 1), column_indices, values and
    `count` (a one-element int32 CUDA tensor: C's entries, -1 when `products` is not the factors' count; above `capacity`, nothing
    but row_offsets and count was written) and reads nothing back; `trimmed()` waits for the stream of the last call, reads the
    count and returns the DeviceCsr narrowed to it."""

    def __init__(self, a, b, products: Optional[int] = None, capacity: Optional[int] = None, stream=None):
        import torch
        self.nnz_a, self.nnz_b, dev = _gemm_check(a, b, "csr_gemm")
        self.a, self.b = a, b
        self.rows, self.inner, self.cols = int(a.rows), int(a.cols), int(b.cols)
        self.products = csr_gemm_products(a, b, stream=stream) if products is None else int(products)
        if self.products < 0 or self.rows + self.products > _MAX_ITEMS:
            raise MspmvError(f"csr_gemm: rows + products = {self.rows} + {self.products} must lie in [0, 2^31 - 65537]")
        self.capacity = self.products if capacity is None else int(capacity)
        if self.capacity < 0 or self.capacity > _MAX_ITEMS:
            raise MspmvError(f"csr_gemm: capacity {self.capacity} must lie in [0, 2^31 - 65537]")
        self.dtype = torch.float32 if a.values is None else a.values.dtype
        self._fn, _ = _typed(load_library(), "mspmv_csr_gemm", self.dtype)
        self.row_offsets = torch.empty(self.rows + 1, dtype=torch.int32, device=dev)
        self.column_indices = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.values = None if a.values is None else torch.empty(self.capacity, dtype=self.dtype, device=dev)
        self.count = torch.empty(1, dtype=torch.int32, device=dev)
        self.temp = None
        self._stream = None
        self(stream=stream)

    def __call__(self, stream=None):
        """runs the product on the factors' tensors as they are now, into the same outputs; asynchronous on `stream`"""
        a, b = self.a, self.b
        if _gemm_check(a, b, "CsrGemm")[:2] != (self.nnz_a, self.nnz_b) or (a.values is None) != (self.values is None):
            raise MspmvError(f"CsrGemm: the factors must keep their {self.nnz_a} and {self.nnz_b} entries")
        args = (self.rows, self.inner, self.cols, _ptr(a.values), _ptr(a.row_offsets), _ptr(a.column_indices), self.nnz_a,
                _ptr(b.values), _ptr(b.row_offsets), _ptr(b.column_indices), self.nnz_b, self.products, self.capacity,
                _ptr(self.values), ctypes.c_void_p(self.row_offsets.data_ptr()), _ptr(self.column_indices),
                ctypes.c_void_p(self.count.data_ptr()))
        self.temp = _two_phase(self._fn, "mspmv_csr_gemm", self.row_offsets.device, stream, args, temp=self.temp)
        self._stream = stream
        return self

    def trimmed(self):
        from .generators import DeviceCsr
        if self._stream is not None and hasattr(self._stream, "synchronize"):
            self._stream.synchronize()                           # (the count is read on the current stream: wait for the call's first)
        n = int(self.count.item())
        if n < 0:
            raise MspmvError(f"csr_gemm: the factors do not have the {self.products} products stated")
        if n > self.capacity:
            raise MspmvError(f"csr_gemm: C has {n} entries, the outputs hold {self.capacity}")
        return DeviceCsr(self.rows, self.cols, self.row_offsets, self.column_indices[:n], None if self.values is None else self.values[:n])


def csr_gemm(a, b, stream=None, trim: bool = True):
    """C = A * B for two generators.DeviceCsr, a of rows x inner and b of inner x cols, any valid CSR (mspmv_csr_gemm_*): C in
    canonical form (rows sorted by column, no column twice), its pattern the structural product, every value the products a * b of
    its entry, each rounded on its own, added left to right in the order of A's row and, under one entry of A, of B's row.  values
    None in both: structure only.  Reads the number of products back first (csr_gemm_products: it synchronises).  Returns a DeviceCsr:
    with trim=True (which reads C's count back too) narrowed to C's entries; with trim=False column_indices / values keep
    `products` entries, of which the first row_offsets[-1] are written."""
    from .generators import DeviceCsr
    op = CsrGemm(a, b, stream=stream)
    if trim:
        return op.trimmed()
    return DeviceCsr(op.rows, op.cols, op.row_offsets, op.column_indices, op.values)


def csr_permute(values, row_offsets, column_indices, num_cols: int, row_perm=None, col_map=None, return_permutation: bool = False,
                stream=None):
    """B = A[row_perm, :] with every column c renamed col_map[c] and every row sorted stably by its new column (mspmv_csr_permute_*): a
    generators.DeviceCsr (values=None: structure only, .values is None).  row_perm: a permutation of the rows, col_map: num_cols entries
    into [0, num_cols) (None: the identity; neither is checked).  With return_permutation=True returns (csr, permutation): B entry j is
    A entry permutation[j].  With a CsrColoring's (order, inverse) this is P A P^T.  Asynchronous on `stream`; nothing is read back."""
    import torch
    from .generators import DeviceCsr
    dev, rows, nnz = _pattern_check("csr_permute", row_offsets, column_indices)
    cols = int(num_cols)
    if cols < 0:
        raise MspmvError("csr_permute: negative num_cols")
    if values is not None:
        _index_check("csr_permute", values, "values", nnz, dev, (torch.float32, torch.float64))
    if row_perm is not None:
        _index_check("csr_permute", row_perm, "row_perm", rows, dev)
    if col_map is not None:
        _index_check("csr_permute", col_map, "col_map", cols, dev)
    dtype = torch.float32 if values is None else values.dtype
    fn, _ = _typed(load_library(), "mspmv_csr_permute", dtype)
    row_offsets_b = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    cols_b = torch.empty(nnz, dtype=torch.int32, device=dev)
    values_b = None if values is None else torch.empty(nnz, dtype=dtype, device=dev)
    permutation = torch.empty(nnz, dtype=torch.int32, device=dev) if return_permutation else None
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), rows, cols, nnz, _ptr(row_perm), _ptr(col_map), _ptr(values_b),
            ctypes.c_void_p(row_offsets_b.data_ptr()), _ptr(cols_b), _ptr(permutation))
    with torch.cuda.device(dev):
        _two_phase(fn, "mspmv_csr_permute", dev, stream, args)
    csr = DeviceCsr(rows, cols, row_offsets_b, cols_b, values_b)
    return (csr, permutation) if return_permutation else csr


def sddmm(row_offsets, column_indices, U, V, out=None, alpha: float = 1.0, beta: float = 0.0, stream=None,
          debug_synchronous: bool = False):
    """The sampled dense-dense product (mspmv_sddmm_*): for every stored entry e of the CSR pattern, in row r and column c,
    out[e] = alpha * (U[r, :] . V[c, :]) + beta * out[e], the dot product added left to right, every operation rounded on its own
    (include/mspmv.h states the bits).  U: [rows, k], V: [cols, k] CUDA tensors with unit stride along k (leading dimensions from
    stride(0)), both float32, both float64, or both bfloat16 with a float32 `out`.  `out`: the nnz values, required when
    beta != 0; with beta == 0 it is never read.  U = dY, V = X gives the gradient of csrmm with respect to the matrix values.
    Asynchronous on `stream`; one launch, no temp storage.  Returns out."""
    import torch
    for t, name in ((row_offsets, "row_offsets"), (column_indices, "column_indices"), (U, "U"), (V, "V")):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"sddmm: {name} must be a tensor")
    if not (row_offsets.is_cuda and column_indices.is_cuda and U.is_cuda and V.is_cuda):
        raise MspmvError("sddmm needs CUDA (HIP) tensors: the kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise TypeError("sddmm: row_offsets / column_indices must be int32")
    dev = U.device
    if U.dtype != V.dtype:
        raise TypeError(f"sddmm: U holds {U.dtype}, V {V.dtype}")
    if U.dtype not in (torch.float32, torch.float64, torch.bfloat16):
        raise TypeError(f"sddmm is instantiated for float32, float64 and bfloat16 (with float32 out), got {U.dtype}")
    out_dtype = torch.float32 if U.dtype == torch.bfloat16 else U.dtype
    for t, name in ((U, "U"), (V, "V")):
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise MspmvError(f"sddmm: {name} must be 2-D with unit stride along k (row-major)")
    if row_offsets.dim() != 1 or row_offsets.numel() < 1 or not row_offsets.is_contiguous() or column_indices.dim() != 1 \
            or not column_indices.is_contiguous():
        raise MspmvError("sddmm: row_offsets (rows + 1 entries) and column_indices must be contiguous 1-D tensors")
    rows, cols, nnz, k = row_offsets.numel() - 1, V.shape[0], column_indices.numel(), U.shape[1]
    if U.shape[0] != rows or V.shape[1] != k:
        raise MspmvError(f"sddmm: U must be [{rows}, k] and V [cols, k] with the same k, got {tuple(U.shape)} and {tuple(V.shape)}")
    ldu = U.stride(0) if rows > 1 else max(k, 1)
    ldv = V.stride(0) if cols > 1 else max(k, 1)
    if ldu < k or ldv < k:
        raise MspmvError("sddmm: leading dimensions must be at least k (no overlapping / broadcast rows)")
    if out is None:
        if beta != 0:
            raise MspmvError("sddmm: beta != 0 needs `out`, the values it scales")
        out = torch.empty(nnz, dtype=out_dtype, device=dev)
    if not isinstance(out, torch.Tensor) or out.dtype != out_dtype:
        raise TypeError(f"sddmm: out must be a {out_dtype} tensor for {U.dtype} U and V")
    if out.dim() != 1 or out.numel() != nnz or not out.is_contiguous():
        raise MspmvError(f"sddmm: out must be a contiguous 1-D tensor of {nnz} entries")
    for t, name in ((row_offsets, "row_offsets"), (column_indices, "column_indices"), (V, "V"), (out, "out")):
        if t.device != dev:
            raise MspmvError(f"sddmm: {name} must be on {dev}")
    lib = load_library()
    fn, ct = {torch.float32: (lib.mspmv_sddmm_f32, ctypes.c_float), torch.float64: (lib.mspmv_sddmm_f64, ctypes.c_double),
              torch.bfloat16: (lib.mspmv_sddmm_bf16_f32, ctypes.c_float)}[U.dtype]
    _check(int(fn(_ptr(row_offsets), _ptr(column_indices), _ptr(U), int(ldu), _ptr(V), int(ldv), _ptr(out), rows, cols, nnz, k,
                  ct(alpha), ct(beta), _stream_handle(stream), int(bool(debug_synchronous)))), "mspmv_sddmm")
    return out
