"""The level-scheduled triangular solves (CsrSv: csrsv for one right-hand side, csrsm for k) and the two factorisations that run along
the same levels, ILU(0) and IC(0), and ILU(k) / IC(k): the same two on a level-of-fill pattern (fill.py)."""
from __future__ import annotations

import ctypes

from ._lib import MspmvError, _CsrSmInfo, _CsrSvInfo, _check, load_library
from ._args import _Handle, _many_layout, _pattern_check, _ptr, _stream_handle, _typed
from .fill import CsrFill


class CsrSv(_Handle):
    """The level-scheduled sparse triangular solve (mspmv_csrsv_*): op(A) x = alpha * b for one right-hand side.  The constructor
    analyses the PATTERN (synchronous; the plan owns what it allocates); `solve` runs on any values with that pattern.  `lower`
    chooses the triangle, `unit_diagonal` the diagonal; entries of the other triangle (and, with a unit diagonal, stored diagonals) are
    ignored, so a full matrix may be swept with both of its parts.  include/mspmv.h states the bits of x.
    .info: the plan's figures (levels, launches, narrow_rows, bad_diagonal_row, ...); .order: the rows sorted stably by level;
    .level_offsets: levels + 1 entries (both int32 tensors on the matrix's device, copies)."""

    _destroy = "mspmv_csrsv_plan_destroy"

    def __init__(self, row_offsets, column_indices, lower: bool = True, unit_diagonal: bool = False, stream=None,
                 debug_synchronous: bool = False):
        import torch
        self.device, self.rows, self.nnz = _pattern_check("CsrSv", row_offsets, column_indices, int32_error=TypeError)
        self.row_offsets, self.column_indices = row_offsets, column_indices
        self._lib = load_library()
        handle = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _check(self._lib.mspmv_csrsv_plan_create(ctypes.byref(handle), _ptr(row_offsets), _ptr(column_indices), self.rows, self.nnz,
                                                     0 if lower else 1, 1 if unit_diagonal else 0, _stream_handle(stream),
                                                     int(bool(debug_synchronous))), "mspmv_csrsv_plan_create")
        self._handle = handle
        raw = _CsrSvInfo()
        _check(self._lib.mspmv_csrsv_plan_info(self._handle, ctypes.byref(raw)), "mspmv_csrsv_plan_info")
        self.info = {name: int(getattr(raw, name)) for name, _ in _CsrSvInfo._fields_}

    @property
    def order(self):
        return self._int32_copy("mspmv_csrsv_plan_order", self.rows)

    @property
    def level_offsets(self):
        if self.rows == 0:                                         # (a plan of no rows holds nothing on the device)
            import torch
            return torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._int32_copy("mspmv_csrsv_plan_level_offsets", self.info["levels"] + 1)

    def solve(self, values, b, x=None, alpha: float = 1.0, stream=None, debug_synchronous: bool = False):
        """x = the solution of op(A) x = alpha * b on `values` (the plan's pattern); x may be b (in place).  Asynchronous on `stream`;
        info["launches"] launches, nothing allocated but a missing x, nothing read back."""
        import torch
        handle = self._live()
        for t, name in ((values, "values"), (b, "b")):
            if not isinstance(t, torch.Tensor):
                raise MspmvError(f"CsrSv.solve: {name} must be a tensor")
        if not (values.is_cuda and b.is_cuda):
            raise MspmvError("CsrSv.solve needs CUDA (HIP) tensors: the kernels only run on the GPU")
        if b.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"CsrSv.solve is instantiated for float32 and float64, got {b.dtype}")
        if values.dtype != b.dtype:
            raise TypeError(f"CsrSv.solve: values hold {values.dtype}, b {b.dtype}")
        if x is None:
            x = torch.empty(self.rows, dtype=b.dtype, device=self.device)
        if not isinstance(x, torch.Tensor) or x.dtype != b.dtype:
            raise TypeError(f"CsrSv.solve: x must be a {b.dtype} tensor")
        for t, name, need in ((values, "values", self.nnz), (b, "b", self.rows), (x, "x", self.rows)):
            if t.device != self.device or t.dim() != 1 or not t.is_contiguous() or t.numel() != need:
                raise MspmvError(f"CsrSv.solve: {name} must be a contiguous 1-D tensor of {need} entries on {self.device}")
        if self.info["bad_diagonal_row"] >= 0:
            raise MspmvError(f"CsrSv.solve: row {self.info['bad_diagonal_row']} has no or more than one stored diagonal entry")
        fn, ct = _typed(self._lib, "mspmv_csrsv_solve", b.dtype)
        _check(int(fn(handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), ct(alpha), _ptr(b), _ptr(x),
                      _stream_handle(stream), int(bool(debug_synchronous)))), "mspmv_csrsv_solve")
        return x

    def many_info(self, k: int) -> dict:
        """The figures of mspmv_csrsm_info for k right-hand sides on this plan: k, lanes_per_row (P), passes, narrow_lanes, launches."""
        raw = _CsrSmInfo()
        _check(self._lib.mspmv_csrsm_info(self._live(), int(k), ctypes.byref(raw)), "mspmv_csrsm_info")
        return {name: int(getattr(raw, name)) for name, _ in _CsrSmInfo._fields_}

    def solve_many(self, values, B, X=None, alpha: float = 1.0, stream=None, debug_synchronous: bool = False):
        """X = the solution of op(A) X = alpha * B for the k columns of B (mspmv_csrsm_solve_*), column j bit for bit what `solve` gives
        for column j.  B and X: [rows, k], row-major (stride(1) == 1, stride(0) >= k: the leading dimension is the stride, as in csrmm);
        X may be B (in place).  Asynchronous on `stream`; many_info(k)["launches"] launches, nothing allocated but a missing X."""
        import torch
        handle = self._live()
        k = _many_layout("CsrSv.solve_many", values, B, X)
        if not (values.is_cuda and B.is_cuda):
            raise MspmvError("CsrSv.solve_many needs CUDA (HIP) tensors: the kernels only run on the GPU")
        if X is None:
            X = torch.empty(self.rows, k, dtype=B.dtype, device=self.device)
        if values.device != self.device or values.dim() != 1 or not values.is_contiguous() or values.numel() != self.nnz:
            raise MspmvError(f"CsrSv.solve_many: values must be a contiguous 1-D tensor of {self.nnz} entries on {self.device}")
        for t, name in ((B, "B"), (X, "X")):
            if t.device != self.device or t.shape != (self.rows, k):
                raise MspmvError(f"CsrSv.solve_many: {name} must be a [{self.rows}, {k}] tensor on {self.device}")
        if self.info["bad_diagonal_row"] >= 0:
            raise MspmvError(f"CsrSv.solve_many: row {self.info['bad_diagonal_row']} has no or more than one stored diagonal entry")
        ldb = B.stride(0) if self.rows > 1 else k
        ldx = X.stride(0) if self.rows > 1 else k
        fn, ct = _typed(self._lib, "mspmv_csrsm_solve", B.dtype)
        _check(int(fn(handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), ct(alpha), _ptr(B), int(ldb), _ptr(X),
                      int(ldx), k, _stream_handle(stream), int(bool(debug_synchronous)))), "mspmv_csrsm_solve")
        return X


def csrsv(values, row_offsets, column_indices, b, lower: bool = True, unit_diagonal: bool = False, alpha: float = 1.0):
    """One-shot triangular solve: analyse the pattern, solve op(A) x = alpha * b, drop the plan.  A loop keeps a CsrSv."""
    plan = CsrSv(row_offsets, column_indices, lower=lower, unit_diagonal=unit_diagonal)
    try:
        return plan.solve(values, b, alpha=alpha)
    finally:
        import torch
        torch.cuda.current_stream(plan.device).synchronize()
        plan.close()


def csrsm(values, row_offsets, column_indices, B, lower: bool = True, unit_diagonal: bool = False, alpha: float = 1.0):
    """One-shot triangular solve for the k columns of B ([rows, k], row-major): analyse the pattern, solve op(A) X = alpha * B, drop
    the plan.  A loop keeps a CsrSv and calls solve_many."""
    _many_layout("csrsm", values, B, None)
    plan = CsrSv(row_offsets, column_indices, lower=lower, unit_diagonal=unit_diagonal)
    try:
        return plan.solve_many(values, B, alpha=alpha)
    finally:
        import torch
        torch.cuda.current_stream(plan.device).synchronize()
        plan.close()


def _mid_block(kept, what, factor, R):
    """the rows x k block between the two sweeps of a preconditioner: the kept one, or a new one when k or the dtype changed"""
    import torch
    k = _many_layout(what, factor, R, None)
    if kept is None or kept.dtype != R.dtype or kept.shape != (R.shape[0], k):
        kept = torch.empty(R.shape[0], k, dtype=R.dtype, device=R.device)
    return kept


def csrilu0_group(rows: int, nnz: int) -> int:
    """G, the lanes of one wave that work one row of mspmv_csrilu0_*: a function of rows and nnz alone (host only)."""
    g = ctypes.c_int32(0)
    _check(load_library().mspmv_csrilu0_group(int(rows), int(nnz), ctypes.byref(g)), "mspmv_csrilu0_group")
    return int(g.value)


def _ilu0_check(what, values, row_offsets, column_indices, plan=None, out=None):
    """the refusals of csrilu0 / Ilu0.factor, raised before any device call"""
    import torch
    if not isinstance(values, torch.Tensor):
        raise MspmvError(f"{what}: values must be a tensor")
    if not values.is_cuda:
        raise MspmvError(f"{what} needs CUDA (HIP) tensors: the kernels only run on the GPU")
    if values.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} is instantiated for float32 and float64, got {values.dtype}")
    _, rows, nnz = _pattern_check(what, row_offsets, column_indices, int32_error=TypeError)
    if values.device != row_offsets.device or values.dim() != 1 or not values.is_contiguous() or values.numel() != nnz:
        raise MspmvError(f"{what}: values must be a contiguous 1-D tensor of {nnz} entries on {row_offsets.device}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != values.dtype:
            raise TypeError(f"{what}: out must be a {values.dtype} tensor")
        if out.device != values.device or out.dim() != 1 or not out.is_contiguous() or out.numel() != nnz:
            raise MspmvError(f"{what}: out must be a contiguous 1-D tensor of {nnz} entries on {values.device}")
    if plan is not None:
        if not isinstance(plan, CsrSv):
            raise MspmvError(f"{what}: plan must be a CsrSv")
        if plan._handle is None:
            raise MspmvError(f"{what}: the plan is closed")
        if plan.info["uplo"] != 0:
            raise MspmvError(f"{what}: the plan must be a LOWER one (the factorisation runs along the levels of L x = b)")
        if plan.rows != rows or plan.nnz != nnz or plan.device != row_offsets.device:
            raise MspmvError(f"{what}: the plan was made for {plan.rows} rows and {plan.nnz} entries on {plan.device}")
    return rows, nnz


def _factor_temp_bytes(plan, family, extra) -> int:
    """the size query of mspmv_csrilu0_* / mspmv_csric0_* (`extra`: the arguments between column_indices and d_pivot)"""
    size = ctypes.c_size_t(0)
    fn = getattr(plan._lib, f"mspmv_{family}_f32")
    _check(fn(plan._handle, None, ctypes.byref(size), None, None, None, None, *extra, None, None, 0), f"mspmv_{family} (size query)")
    return int(size.value)


def _factor_call(plan, family, extra, temp, values, out, row_offsets, column_indices, pivot, stream, debug_synchronous):
    import torch
    fn, _ = _typed(plan._lib, f"mspmv_{family}", values.dtype)
    size = ctypes.c_size_t(temp.numel())
    with torch.cuda.device(plan.device):
        _check(int(fn(plan._handle, ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), _ptr(values), _ptr(out), _ptr(row_offsets),
                      _ptr(column_indices), *extra, _ptr(pivot), _stream_handle(stream), int(bool(debug_synchronous)))), f"mspmv_{family}")


def _ilu0_temp_bytes(plan) -> int:
    return _factor_temp_bytes(plan, "csrilu0", ())


def _ilu0_call(plan, temp, values, lu, row_offsets, column_indices, pivot, stream, debug_synchronous):
    _factor_call(plan, "csrilu0", (), temp, values, lu, row_offsets, column_indices, pivot, stream, debug_synchronous)


def _ic0_temp_bytes(plan) -> int:
    return _factor_temp_bytes(plan, "csric0", (0,))


def _ic0_call(plan, temp, values, l, row_offsets, column_indices, mirror, pivot, stream, debug_synchronous):
    _factor_call(plan, "csric0", (int(bool(mirror)),), temp, values, l, row_offsets, column_indices, pivot, stream, debug_synchronous)


def _factor_once(what, unit_diagonal, temp_bytes, call, values, row_offsets, column_indices, plan, out, stream):
    """csrilu0 / csric0: the plan given or one of its own, out / pivot / temp allocated, `call(plan, temp, out, pivot)`; a plan of its
    own is dropped after the stream has finished"""
    import torch
    rows, nnz = _ilu0_check(what, values, row_offsets, column_indices, plan, out)
    own = plan is None
    if own:
        plan = CsrSv(row_offsets, column_indices, lower=True, unit_diagonal=unit_diagonal, stream=stream)
    try:
        factor = out if out is not None else torch.empty(nnz, dtype=values.dtype, device=values.device)
        pivot = torch.empty(1, dtype=torch.int32, device=values.device)
        temp = torch.empty(temp_bytes(plan), dtype=torch.uint8, device=values.device)
        call(plan, temp, factor, pivot)
        return factor, pivot
    finally:
        if own:
            (stream if stream is not None else torch.cuda.current_stream(plan.device)).synchronize()
            plan.close()


def csrilu0(values, row_offsets, column_indices, plan=None, out=None, stream=None, debug_synchronous: bool = False):
    """ILU(0) of the CSR matrix (sorted rows, no column twice) on its own pattern (mspmv_csrilu0_*): returns (lu_values, pivot).
    lu_values: L in the strict lower part (unit diagonal implied), U on and above the diagonal -- what CsrSv sweeps with lower=True,
    unit_diagonal=True and lower=False.  pivot: a 1-element int32 DEVICE tensor (the smallest row with a missing or zero diagonal, -1
    if none), so nothing waits for the device.  `plan`: a LOWER CsrSv of this pattern (one is made and dropped if not given; a loop
    keeps an Ilu0).  `out`: where the factor goes; may be `values` (in place)."""
    def call(plan, temp, lu, pivot):
        _ilu0_call(plan, temp, values, lu, row_offsets, column_indices, pivot, stream, debug_synchronous)
    return _factor_once("csrilu0", True, _ilu0_temp_bytes, call, values, row_offsets, column_indices, plan, out, stream)


def csric0(values, row_offsets, column_indices, plan=None, out=None, mirror: bool = False, stream=None, debug_synchronous: bool = False):
    """IC(0) of the CSR matrix (sorted rows, no column twice) on the pattern of its lower triangle (mspmv_csric0_*): returns
    (l_values, pivot).  Only the lower triangle and the diagonal are read as numbers.  l_values: L in the lower part and on the diagonal
    of A's layout; the upper part is A's, unchanged, or with `mirror` L^T (entry (i, j) = the final entry (j, i), +0.0 where row j does
    not store column i) -- what CsrSv then sweeps with lower=True and lower=False, both with unit_diagonal=False.  pivot: a 1-element
    int32 DEVICE tensor (the smallest row whose diagonal is missing or whose value under the root is <= 0, -1 if none), so nothing
    waits for the device.  `plan`: a LOWER CsrSv of this pattern (one is made and dropped if not given; a loop keeps an Ic0).  `out`:
    where the factor goes; may be `values` (in place)."""
    def call(plan, temp, l, pivot):
        _ic0_call(plan, temp, values, l, row_offsets, column_indices, mirror, pivot, stream, debug_synchronous)
    return _factor_once("csric0", False, _ic0_temp_bytes, call, values, row_offsets, column_indices, plan, out, stream)


class _Factor0(_Handle):
    """What Ilu0 and Ic0 share: the LOWER and UPPER plans of one pattern, the temp storage, the pivot, the factor of the last `factor`
    and the kept vector and block between the two sweeps.  A subclass states _unit_lower (its lower plan's unit_diagonal), _temp_bytes
    and _call (its factorisation), and shows the factor under its public name.  Of _Handle it has the life (close() closes the two plans,
    which make the refusals of a pattern; __del__ never raises); it has no handle of its own."""

    lower = upper = None

    def __init__(self, row_offsets, column_indices, stream=None):
        import torch
        self.lower = CsrSv(row_offsets, column_indices, lower=True, unit_diagonal=self._unit_lower, stream=stream)
        self.upper = CsrSv(row_offsets, column_indices, lower=False, unit_diagonal=False, stream=stream)
        self.device, self.rows, self.nnz = self.lower.device, self.lower.rows, self.lower.nnz
        self.row_offsets, self.column_indices = row_offsets, column_indices
        self._temp = torch.empty(self._temp_bytes(self.lower), dtype=torch.uint8, device=self.device)
        self.pivot = torch.empty(1, dtype=torch.int32, device=self.device)
        self._factor = None
        self._mid = None
        self._mid_many = None

    def _ready(self, what=None):
        name = type(self).__name__
        if self.lower is None:
            raise MspmvError(f"{name}: closed")
        if what is not None and self._factor is None:
            raise MspmvError(f"{name}.{what}: nothing is factorised yet (call factor(values) first)")
        return name

    def factor(self, values, stream=None, debug_synchronous: bool = False):
        import torch
        name = self._ready()
        _ilu0_check(f"{name}.factor", values, self.row_offsets, self.column_indices, self.lower)
        if self._factor is None or self._factor.dtype != values.dtype:
            self._factor = torch.empty(self.nnz, dtype=values.dtype, device=self.device)
            self._mid = torch.empty(self.rows, dtype=values.dtype, device=self.device)
        self._call(self.lower, self._temp, values, self._factor, self.row_offsets, self.column_indices, self.pivot, stream, debug_synchronous)
        return self.pivot

    def solve(self, r, out=None, stream=None):
        self._ready("solve")
        self.lower.solve(self._factor, r, x=self._mid, stream=stream)
        return self.upper.solve(self._factor, self._mid, x=out, stream=stream)

    def solve_many(self, R, out=None, stream=None):
        """The two sweeps of `solve` for the k columns of R ([rows, k], row-major): two solve_many sweeps through one kept rows x k
        block (allocated when k or the dtype changes); column j is bit for bit solve(R[:, j])."""
        name = self._ready("solve_many")
        self._mid_many = _mid_block(self._mid_many, f"{name}.solve_many", self._factor, R)
        self.lower.solve_many(self._factor, R, X=self._mid_many, stream=stream)
        return self.upper.solve_many(self._factor, self._mid_many, X=out, stream=stream)

    def close(self):
        for plan in (self.lower, self.upper):
            if plan is not None:
                plan.close()
        self.lower = self.upper = None
        self._temp = self._factor = self._mid = self._mid_many = None


class Ilu0(_Factor0):
    """The ILU(0) preconditioner of one pattern: the LOWER + UNIT and UPPER + NON_UNIT plans of CsrSv and the temp storage of
    mspmv_csrilu0_*, made once (the constructor analyses the pattern twice; synchronous).  `factor(values)` factorises -- again and
    again, on new values of the same pattern -- and returns the pivot tensor (1 int32 on the device: -1, or the smallest row with a
    missing or zero diagonal); `solve(r)` is U^-1 (L^-1 r), two triangular solves through one kept vector; `solve_many(R)` is the
    same for the k columns of R; `close()` releases the plans and the storage.  .lu_values: the factor of the last `factor`."""

    _unit_lower = True
    _temp_bytes = staticmethod(_ilu0_temp_bytes)
    _call = staticmethod(_ilu0_call)
    lu_values = property(lambda self: self._factor)


def csric0_group(rows: int, nnz: int) -> int:
    """G, the lanes of one wave that work one row of mspmv_csric0_*: a function of rows and nnz alone (host only)."""
    g = ctypes.c_int32(0)
    _check(load_library().mspmv_csric0_group(int(rows), int(nnz), ctypes.byref(g)), "mspmv_csric0_group")
    return int(g.value)


class Ic0(_Factor0):
    """The IC(0) preconditioner of one (structurally symmetric) pattern: the LOWER + NON_UNIT and UPPER + NON_UNIT plans of CsrSv and
    the temp storage of mspmv_csric0_*, made once (the constructor analyses the pattern twice; synchronous).  `factor(values)`
    factorises with the mirror -- again and again, on new values of the same pattern -- and returns the pivot tensor (1 int32 on the
    device: -1, or the smallest row whose diagonal is missing or whose value under the root is <= 0); `solve(r)` is
    L^-T (L^-1 r), two triangular solves through one kept vector (a pattern that lacks a diagonal is refused there by the NON_UNIT
    plan, as it is); `solve_many(R)` is the same for the k columns of R; `close()` releases the plans and the storage.  .l_values: the
    factor of the last `factor`: L below and on the diagonal, L^T above it, in A's layout."""

    _unit_lower = False
    _temp_bytes = staticmethod(_ic0_temp_bytes)
    l_values = property(lambda self: self._factor)

    @staticmethod
    def _call(plan, temp, values, l, row_offsets, column_indices, pivot, stream, debug_synchronous):
        _ic0_call(plan, temp, values, l, row_offsets, column_indices, True, pivot, stream, debug_synchronous)


class _FactorK:
    """What Iluk and Ick add to Ilu0 / Ic0: the CsrFill of the given pattern, on whose filled pattern the plans are made, and the kept
    filled values that `factor` scatters A's values into before it factorises them."""

    fill = None

    def __init__(self, row_offsets, column_indices, level: int, stream=None):
        self.fill = CsrFill(row_offsets, column_indices, level, stream=stream)
        self.level, self.source_nnz = self.fill.level, self.fill.nnz
        self._filled = None
        try:
            super().__init__(self.fill.row_offsets, self.fill.column_indices, stream=stream)
        except Exception:
            self.close()
            raise

    def factor(self, values, stream=None, debug_synchronous: bool = False):
        """Factorises A's `values` (the entries of the pattern GIVEN to the constructor) on the filled pattern: they are scattered into a
        kept filled array (+0.0 at fill entries, one launch), which is then factorised as Ilu0 / Ic0 factorise theirs."""
        self._ready()
        if self._filled is not None and getattr(values, "dtype", None) != self._filled.dtype:
            self._filled = None
        self._filled = self.fill.values(values, out=self._filled, stream=stream)
        return super().factor(self._filled, stream=stream, debug_synchronous=debug_synchronous)

    def close(self):
        super().close()
        if self.fill is not None:
            self.fill.close()
        self._filled = None


class Iluk(_FactorK, Ilu0):
    """The ILU(k) preconditioner of one pattern: an Ilu0 made on the level-`level` filled pattern (CsrFill; synchronous).
    `factor(values)` takes the values of the pattern given here; .row_offsets / .column_indices are the FILLED pattern's, .lu_values the
    factor on it, .fill the CsrFill (levels, source).  solve, solve_many, .lower, .upper and the use as a preconditioner of Pcg,
    Bicgstab and Gmres are Ilu0's.  level = 0 is Ilu0 bit for bit."""


class Ick(_FactorK, Ic0):
    """The IC(k) preconditioner of one structurally symmetric pattern: an Ic0 made on the level-`level` filled pattern (CsrFill, which
    is symmetric when the pattern is; synchronous).  `factor(values)` takes the values of the pattern given here; .row_offsets /
    .column_indices are the FILLED pattern's, .l_values the factor on it, .fill the CsrFill.  Everything else is Ic0's.  level = 0 is
    Ic0 bit for bit."""
