"""merge_spmv_amd -- MI355X-native merge-based CsrMV.

Python face of the C ABI in include/mspmv.h (libmspmv.so: hand-written HIP
kernels for gfx950).  It mirrors the reference's device API
``cub::DeviceSpmv::CsrMV`` (reference cub/device/device_spmv.cuh:129-164) --
same argument order, same two-phase temp-storage convention -- so parity
tests read like the reference's own call sites (gpu_spmv.cu:390-409).

PyTorch is used only as plumbing: device memory (tensors), streams and, for
the multi-GPU path, torch.distributed.  There is NO CPU or eager fallback: if
libmspmv.so is missing or fails to load, importing the compute entry points
raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

__all__ = ["DeviceSpmv", "csrmv", "csrmv_mixed", "csrmm", "CsrMVWorkspace", "CsrMVPlan", "csr_transpose", "CsrTranspose", "coo_to_csr", "CooToCsr", "csr_sum_duplicates", "coomv",
           "csr_add", "CsrAdd", "csr_symmetrize", "csr_gemm", "CsrGemm", "csr_gemm_products", "sddmm", "CsrSv", "csrsv", "csrsm", "csrilu0", "Ilu0", "csric0", "Ic0",
           "CsrColoring", "csr_color", "csr_permute", "multicolor_reorder", "vec_dot", "Pcg", "pcg",
           "plan_bench_record", "library_path", "load_library", "launch_info",
           "set_tuning", "set_tdm", "clocked_bands", "debug_read_tiles", "profile_begin", "profile_end", "MspmvError",
           "TUNE_ATOMIC_FIX", "TUNE_NO_VEC"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAMES = {"product": "libmspmv.so", "dev": "libmspmv_dev.so"}
_libs = {}                 # kind -> ctypes.CDLL
_active = "product"

TUNE_ATOMIC_FIX = 2
TUNE_NO_VEC = 4


class MspmvError(RuntimeError):
    pass


def library_path(kind: Optional[str] = None) -> str:
    """The active library's file: libmspmv.so (the product: no setters, nothing read from the environment) or libmspmv_dev.so (the same
    sources built with -DMSPMV_TUNING: include/mspmv_dev.h) next to this file.  MSPMV_LIB=<path> replaces the PRODUCT library by another
    build of the same ABI (A/B tools)."""
    kind = kind or _active
    if kind == "product" and os.environ.get("MSPMV_LIB"):
        return os.environ["MSPMV_LIB"]
    return os.path.join(_HERE, _LIB_NAMES[kind])


def use_library(kind: str = "product") -> str:
    """Make `kind` ("product" | "dev") the library every wrapper of this module calls from now on; returns the previous kind.  The
    setters (set_tuning, set_band_passes, set_record_polls, set_compact_tiles) exist in the development library only and switch to
    it themselves when asked for a non-default value -- tests/conftest.py switches back to the product after every test."""
    global _active
    if kind not in _LIB_NAMES:
        raise ValueError(f"use_library: {kind!r} is not one of {sorted(_LIB_NAMES)}")
    prev, _active = _active, kind
    return prev


def active_library() -> str:
    return _active


class _CsrSvInfo(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("nnz", ctypes.c_int32), ("uplo", ctypes.c_int32), ("diag", ctypes.c_int32),
                ("levels", ctypes.c_int32), ("launches", ctypes.c_int32), ("narrow_rows", ctypes.c_int32),
                ("max_level_rows", ctypes.c_int32), ("bad_diagonal_row", ctypes.c_int32), ("used_entries", ctypes.c_int64),
                ("device_bytes", ctypes.c_uint64)]


class _CsrColorInfo(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("nnz", ctypes.c_int32), ("colors", ctypes.c_int32), ("max_color_rows", ctypes.c_int32),
                ("rounds", ctypes.c_int32), ("edges", ctypes.c_int64), ("device_bytes", ctypes.c_uint64)]


class _PcgState(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("launches_per_iteration", ctypes.c_int32),
                ("precond_kind", ctypes.c_int32), ("bad_diagonal_row", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rr", ctypes.c_double), ("bb", ctypes.c_double), ("stop2", ctypes.c_double), ("rz", ctypes.c_double),
                ("device_bytes", ctypes.c_uint64)]


class _CsrSmInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("lanes_per_row", ctypes.c_int32), ("passes", ctypes.c_int32), ("narrow_lanes", ctypes.c_int32),
                ("launches", ctypes.c_int32)]


class _LaunchInfo(ctypes.Structure):
    _fields_ = [("block_threads", ctypes.c_int32), ("items_per_thread", ctypes.c_int32),
                ("tile_items", ctypes.c_int32), ("num_tiles", ctypes.c_int32),
                ("fixup_chunk", ctypes.c_int32), ("fixup_levels", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("snap_head_max", ctypes.c_int32),
                ("temp_bytes", ctypes.c_uint64), ("coords_offset", ctypes.c_uint64),
                ("carries_offset", ctypes.c_uint64), ("diag_offset", ctypes.c_uint64), ("records_offset", ctypes.c_uint64)]


def load_library() -> ctypes.CDLL:
    """dlopen libmspmv.so (built in-tree by `make -C merge_spmv_amd` or
    __graft_entry__.build()).  Fails loudly when absent."""
    if _active in _libs:
        return _libs[_active]
    path = library_path()
    if not os.path.exists(path):
        raise MspmvError(f"{path} not found: build the HIP extension first "
                         f"(python -c 'import __graft_entry__ as g; g.build()' or make -C merge_spmv_amd)")
    # torch bundles its own libamdhip64.so.7; importing it first makes the
    # dynamic linker bind libmspmv.so to that same HIP runtime (same SONAME),
    # so tensors' device pointers and streams are valid inside the library.
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    vp, i32, sz_p = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)
    for name in ("mspmv_csrmv_f32", "mspmv_csrmv_f64"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, vp, ctypes.c_int]
    lib.mspmv_csrmv_axpby_f32.restype = ctypes.c_int
    lib.mspmv_csrmv_axpby_f32.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.c_float,
                                          ctypes.c_float, vp, ctypes.c_int]
    lib.mspmv_csrmv_axpby_f64.restype = ctypes.c_int
    lib.mspmv_csrmv_axpby_f64.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.c_double,
                                          ctypes.c_double, vp, ctypes.c_int]
    lib.mspmv_csrmv_prepare.restype = ctypes.c_int
    lib.mspmv_csrmv_prepare.argtypes = [vp, sz_p, vp, i32, i32, i32, vp, ctypes.c_int]
    lib.mspmv_csrmv_prepared_f32.restype = ctypes.c_int
    lib.mspmv_csrmv_prepared_f32.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.c_float,
                                             ctypes.c_float, vp, ctypes.c_int]
    lib.mspmv_csrmv_prepared_f64.restype = ctypes.c_int
    lib.mspmv_csrmv_prepared_f64.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.c_double,
                                             ctypes.c_double, vp, ctypes.c_int]
    for pair, ct in (("f32_f64", ctypes.c_double), ("bf16_f32", ctypes.c_float)):
        for name in ("mspmv_csrmv_mixed_" + pair, "mspmv_csrmv_mixed_prepared_" + pair):
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ct, ct, vp, ctypes.c_int]
    lib.mspmv_csrmm_f32.restype = ctypes.c_int
    lib.mspmv_csrmm_f32.argtypes = [vp, sz_p, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, ctypes.c_float, ctypes.c_float,
                                    vp, ctypes.c_int]
    lib.mspmv_csrmm_f64.restype = ctypes.c_int
    lib.mspmv_csrmm_f64.argtypes = [vp, sz_p, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, ctypes.c_double, ctypes.c_double,
                                    vp, ctypes.c_int]
    lib.mspmv_error_string.restype = ctypes.c_char_p
    lib.mspmv_error_string.argtypes = [ctypes.c_int]
    lib.mspmv_version.restype = ctypes.c_int
    lib.mspmv_get_launch_info.restype = ctypes.c_int
    lib.mspmv_get_launch_info.argtypes = [i32, i32, i32, ctypes.POINTER(_LaunchInfo)]
    lib.mspmv_get_launch_info_cols.restype = ctypes.c_int
    lib.mspmv_get_launch_info_cols.argtypes = [i32, i32, i32, i32, ctypes.POINTER(_LaunchInfo)]
    lib.mspmv_debug_read_tiles.restype = ctypes.c_int
    lib.mspmv_debug_read_tiles.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    lib.mspmv_profile_begin.restype = ctypes.c_int
    lib.mspmv_profile_begin.argtypes = [i32]
    lib.mspmv_profile_end.restype = ctypes.c_int
    lib.mspmv_profile_end.argtypes = [ctypes.POINTER(ctypes.c_int32)] + [ctypes.POINTER(ctypes.c_float)] * 3
    if hasattr(lib, "mspmv_set_tuning"):          # (the development library, or an MSPMV_LIB build that has the setters)
        lib.mspmv_set_tuning.restype = ctypes.c_int
        lib.mspmv_set_tuning.argtypes = [i32, i32, i32, i32]
        lib.mspmv_set_band_passes.restype = ctypes.c_int
        lib.mspmv_set_band_passes.argtypes = [ctypes.c_int32, ctypes.c_int32]
        lib.mspmv_set_record_polls.restype = ctypes.c_int
        lib.mspmv_set_record_polls.argtypes = [ctypes.c_int32]
        lib.mspmv_set_compact_tiles.restype = ctypes.c_int
        lib.mspmv_set_compact_tiles.argtypes = [ctypes.c_int32]
        lib.mspmv_set_tdm.restype = ctypes.c_int
        lib.mspmv_set_tdm.argtypes = [i32, i32, i32, i32, i32]
    lib.mspmv_get_band_passes.restype = ctypes.c_int
    lib.mspmv_get_band_passes.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    lib.mspmv_debug_band_windows.restype = ctypes.c_int
    lib.mspmv_debug_band_windows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.mspmv_mg_partition.restype = ctypes.c_int
    lib.mspmv_mg_partition.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, i32, vp, vp]
    lib.mspmv_mg_local_offsets.restype = ctypes.c_int
    lib.mspmv_mg_local_offsets.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int64, vp]
    lib.mspmv_mg_apply_carries.restype = ctypes.c_int
    lib.mspmv_mg_apply_carries.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    i64, u64 = ctypes.c_int64, ctypes.c_uint64
    lib.mspmv_csrmv_plan_size.restype = ctypes.c_int
    lib.mspmv_csrmv_plan_size.argtypes = [i32, i32, i32, i32, i32, sz_p, ctypes.POINTER(i32)]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        fn = getattr(lib, "mspmv_csrmv_plan_build_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_size_t, vp, vp, vp, i32, i32, i32, i32, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csrmv_plan_apply_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_size_t, vp, vp, i32, i32, i32, i32, ct, ct, vp, ctypes.c_int]
    for name in ("mspmv_csrmv_plan_row_offsets", "mspmv_csrmv_plan_columns", "mspmv_csrmv_plan_values"):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = [vp, i32, i32, i32, i32, i32]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        fn = getattr(lib, "mspmv_csr_transpose_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csr_transpose_values_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, i32, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csrmv_transpose_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ct, ct, vp, ctypes.c_int]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        fn = getattr(lib, "mspmv_coo_to_csr_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_coo_to_csr_values_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, i32, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csr_sum_duplicates_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_coomv_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, vp, vp, vp, vp, vp, i32, i32, i32, ct, ct, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csr_add_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, i32, i32, ct, vp, vp, vp, i32, ct, vp, vp, vp, i32, vp, vp, vp, vp, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csr_gemm_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, sz_p, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double), ("bf16_f32", ctypes.c_float)):
        fn = getattr(lib, "mspmv_sddmm_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, ct, ct, vp, ctypes.c_int]
    lib.mspmv_csrsv_plan_create.restype = ctypes.c_int
    lib.mspmv_csrsv_plan_create.argtypes = [ctypes.POINTER(vp), vp, vp, i32, i32, i32, i32, vp, ctypes.c_int]
    lib.mspmv_csrsv_plan_info.restype = ctypes.c_int
    lib.mspmv_csrsv_plan_info.argtypes = [vp, ctypes.POINTER(_CsrSvInfo)]
    for name in ("mspmv_csrsv_plan_order", "mspmv_csrsv_plan_level_offsets"):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = [vp]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        fn = getattr(lib, "mspmv_csrsv_solve_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, ct, vp, vp, vp, ctypes.c_int]
    lib.mspmv_csrsv_plan_destroy.restype = ctypes.c_int
    lib.mspmv_csrsv_plan_destroy.argtypes = [vp]
    lib.mspmv_csrsm_info.restype = ctypes.c_int
    lib.mspmv_csrsm_info.argtypes = [vp, i32, ctypes.POINTER(_CsrSmInfo)]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        fn = getattr(lib, "mspmv_csrsm_solve_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, vp, ct, vp, i32, vp, i32, i32, vp, ctypes.c_int]
    lib.mspmv_csrilu0_group.restype = ctypes.c_int
    lib.mspmv_csrilu0_group.argtypes = [i32, i32, ctypes.POINTER(i32)]
    for name in ("mspmv_csrilu0_f32", "mspmv_csrilu0_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, vp, sz_p, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.mspmv_csric0_group.restype = ctypes.c_int
    lib.mspmv_csric0_group.argtypes = [i32, i32, ctypes.POINTER(i32)]
    for name in ("mspmv_csric0_f32", "mspmv_csric0_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, vp, sz_p, vp, vp, vp, vp, i32, vp, vp, ctypes.c_int]
    lib.mspmv_csr_color_create.restype = ctypes.c_int
    lib.mspmv_csr_color_create.argtypes = [ctypes.POINTER(vp), vp, vp, i32, i32, vp, vp, ctypes.c_int]
    lib.mspmv_csr_color_info.restype = ctypes.c_int
    lib.mspmv_csr_color_info.argtypes = [vp, ctypes.POINTER(_CsrColorInfo)]
    for name in ("mspmv_csr_color_colors", "mspmv_csr_color_order", "mspmv_csr_color_inverse", "mspmv_csr_color_offsets"):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = [vp]
    lib.mspmv_csr_color_destroy.restype = ctypes.c_int
    lib.mspmv_csr_color_destroy.argtypes = [vp]
    for name in ("mspmv_csr_permute_f32", "mspmv_csr_permute_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, sz_p, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    for name in ("mspmv_vec_dot_f32", "mspmv_vec_dot_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, sz_p, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int]
    lib.mspmv_pcg_create.restype = ctypes.c_int
    lib.mspmv_pcg_create.argtypes = [ctypes.POINTER(vp), vp, vp, i32, i32, i32, i32, vp, ctypes.c_int]
    lib.mspmv_pcg_set_factor.restype = ctypes.c_int
    lib.mspmv_pcg_set_factor.argtypes = [vp, vp, vp, vp, vp, vp]
    for name in ("mspmv_pcg_solve_f32", "mspmv_pcg_solve_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, i32, ctypes.c_double, ctypes.c_double, i32, i32, vp, vp, ctypes.c_int]
    lib.mspmv_pcg_state.restype = ctypes.c_int
    lib.mspmv_pcg_state.argtypes = [vp, ctypes.POINTER(_PcgState), vp]
    lib.mspmv_pcg_destroy.restype = ctypes.c_int
    lib.mspmv_pcg_destroy.argtypes = [vp]
    lib.mspmv_csr_gemm_products.restype = ctypes.c_int
    lib.mspmv_csr_gemm_products.argtypes = [vp, sz_p, vp, vp, i32, i32, i32, vp, i32, vp, vp, ctypes.c_int]
    lib.mspmv_csrmv_hotcols_skew.restype = ctypes.c_int
    lib.mspmv_csrmv_hotcols_skew.argtypes = [vp, i32, i32, i32, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.mspmv_csrmv_hotcols_size.restype = ctypes.c_int
    lib.mspmv_csrmv_hotcols_size.argtypes = [i32, i32, i32, i32, sz_p]
    lib.mspmv_csrmv_hotcols_build.restype = ctypes.c_int
    lib.mspmv_csrmv_hotcols_build.argtypes = [vp, ctypes.c_size_t, vp, vp, i32, i32, i32, i32, vp, ctypes.c_int]
    for name, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        for stem in ("mspmv_csrmv_hotcols_apply_", "mspmv_csrmv_hotcols_apply_permuted_"):
            fn = getattr(lib, stem + name)
            fn.restype = ctypes.c_int
            fn.argtypes = [vp, ctypes.c_size_t, vp, vp, vp, vp, i32, i32, i32, ct, ct, vp, ctypes.c_int]
        fn = getattr(lib, "mspmv_csrmv_hotcols_permute_" + name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_size_t, vp, vp, i32, i32, i32, vp, ctypes.c_int]
    for name in ("mspmv_csrmv_hotcols_order", "mspmv_csrmv_hotcols_columns"):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = [vp, i32, i32, i32, i32]
    lib.mspmv_mg_unique_id.restype = ctypes.c_int
    lib.mspmv_mg_unique_id.argtypes = [vp]
    lib.mspmv_mg_plan_create.restype = ctypes.c_int
    lib.mspmv_mg_plan_create.argtypes = [ctypes.POINTER(vp), i32, i32, vp, vp, vp, vp, i64, i32, i32, vp]
    lib.mspmv_mg_plan_set_part.restype = ctypes.c_int
    lib.mspmv_mg_plan_set_part.argtypes = [vp, i32, vp, vp, vp]
    lib.mspmv_mg_plan_hot_columns.restype = ctypes.c_int
    lib.mspmv_mg_plan_hot_columns.argtypes = [vp, i32]
    lib.mspmv_mg_plan_ipc_export.restype = ctypes.c_int
    lib.mspmv_mg_plan_ipc_export.argtypes = [vp, vp, sz_p]
    lib.mspmv_mg_plan_ipc_import.restype = ctypes.c_int
    lib.mspmv_mg_plan_ipc_import.argtypes = [vp, vp, i32, ctypes.c_size_t]
    for name in ("mspmv_mg_plan_x", "mspmv_mg_plan_y", "mspmv_mg_plan_stream"):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = [vp, i32]
    lib.mspmv_mg_plan_info.restype = ctypes.c_int
    lib.mspmv_mg_plan_info.argtypes = [vp, vp]
    for name in ("mspmv_mg_csrmv", "mspmv_mg_allgather_rows", "mspmv_mg_synchronize", "mspmv_mg_plan_destroy"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp]
    _libs[_active] = lib
    return lib


def _setter(name: str, default: bool, *args) -> None:
    """The setters of include/mspmv_dev.h.  The product library has none: asking it for the defaults is a no-op; asking for anything else
    switches this module to the development library (use_library("dev")) -- the same kernels with the per-thread overrides compiled in."""
    lib = load_library()
    if not hasattr(lib, name):
        if default:
            if "dev" in _libs and _libs["dev"] is not lib:        # (a test may have left an override in the development library's thread state)
                _check(getattr(_libs["dev"], name)(*args), name)
            return
        use_library("dev")
        lib = load_library()
    _check(getattr(lib, name)(*args), name)


def _check(status: int, what: str) -> None:
    if status != 0:
        msg = load_library().mspmv_error_string(status)
        raise MspmvError(f"{what} failed: hipError {status} ({msg.decode() if msg else '?'})")


def _value_bytes(t) -> int:
    import torch
    if t.dtype == torch.float32:
        return 4
    if t.dtype == torch.float64:
        return 8
    raise TypeError(f"CsrMV is instantiated for float32 and float64 only (gpu_spmv.cu:730,734), got {t.dtype}")


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
        vb = _value_bytes(d_vector_y)
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
        vb = _value_bytes(values)
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
    vb = _value_bytes(values)
    fn = load_library().mspmv_csrmm_f32 if vb == 4 else load_library().mspmv_csrmm_f64
    ct = ctypes.c_float if vb == 4 else ctypes.c_double
    ldx = X.stride(0) if X.shape[0] > 1 else max(k, 1)
    ldy = Y.stride(0) if Y.shape[0] > 1 else max(k, 1)
    if ldx < k or ldy < k:
        raise MspmvError("csrmm: leading dimensions must be at least k (no overlapping / broadcast rows)")
    def call(tmp_ptr, size):
        return int(fn(tmp_ptr, ctypes.byref(size), _ptr(values), _ptr(row_offsets), _ptr(column_indices), _ptr(X), int(ldx),
                      _ptr(Y), int(ldy), rows, X.shape[0], nnz, k, ct(alpha), ct(beta), _stream_handle(stream),
                      int(bool(debug_synchronous))))
    size = ctypes.c_size_t(0)
    _check(call(ctypes.c_void_p(0), size), "mspmv_csrmm (size query)")
    if temp is None or temp.numel() < size.value:
        temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=values.device)
    size = ctypes.c_size_t(temp.numel())
    _check(call(ctypes.c_void_p(temp.data_ptr()), size), "mspmv_csrmm")
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
    vb = _value_bytes(values)
    lib = load_library()
    fn = lib.mspmv_csrmv_transpose_f32 if vb == 4 else lib.mspmv_csrmv_transpose_f64
    ct = ctypes.c_float if vb == 4 else ctypes.c_double
    a, b = ct(1.0 if alpha is None else alpha), ct(0.0 if beta is None else beta)
    size = ctypes.c_size_t(0)
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz, a, b)
    _check(fn(ctypes.c_void_p(0), ctypes.byref(size), *args, ctypes.c_void_p(0), 0), "mspmv_csrmv_transpose (size query)")
    temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=values.device)
    _check(fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), *args, _stream_handle(stream), int(bool(debug_synchronous))),
           "mspmv_csrmv_transpose")
    if stream is not None and hasattr(stream, "cuda_stream"):
        temp.record_stream(stream)
    return y


def csr_transpose(values, row_offsets, column_indices, num_cols: int, stream=None):
    """A^T as CSR on the device (mspmv_csr_transpose_*): returns (values_t, row_offsets_t, column_indices_t, permutation) with
    values_t[j] = values[permutation[j]]; the entries of each row of A^T in their order in A (stable), so the result is canonical.
    values=None: the structure only (values_t is None).  Asynchronous on `stream`."""
    import torch
    if row_offsets is None or not row_offsets.is_cuda or row_offsets.dtype != torch.int32 or not row_offsets.is_contiguous():
        raise MspmvError("csr_transpose: row_offsets must be a contiguous int32 CUDA tensor")
    rows, cols = row_offsets.numel() - 1, int(num_cols)
    nnz = column_indices.numel() if values is None else values.numel()
    if rows < 0:
        raise MspmvError("csr_transpose: row_offsets needs rows + 1 entries")
    dev = row_offsets.device
    dtype = torch.float32 if values is None else values.dtype
    probe = torch.empty(0, dtype=dtype, device=dev)
    if values is None:              # structure only
        _validate(None, row_offsets, None, None, probe, rows, cols, 0, "csr_transpose", x_rows=0, y_rows=0)
        if nnz > 0 and (column_indices.dtype != torch.int32 or column_indices.device != dev or not column_indices.is_contiguous()):
            raise MspmvError(f"csr_transpose: column_indices must be a contiguous int32 tensor on {dev}")
    else:
        _validate(values, row_offsets, column_indices, None, probe, rows, cols, nnz, "csr_transpose", x_rows=0, y_rows=0)
    vb = _value_bytes(probe)
    lib = load_library()
    fn = lib.mspmv_csr_transpose_f32 if vb == 4 else lib.mspmv_csr_transpose_f64
    values_t = None if values is None else torch.empty(nnz, dtype=dtype, device=dev)
    row_offsets_t = torch.empty(cols + 1, dtype=torch.int32, device=dev)
    column_indices_t = torch.empty(nnz, dtype=torch.int32, device=dev)
    permutation = torch.empty(nnz, dtype=torch.int32, device=dev)
    size = ctypes.c_size_t(0)
    args = (_ptr(values), _ptr(row_offsets), _ptr(column_indices), rows, cols, nnz, _ptr(values_t), ctypes.c_void_p(row_offsets_t.data_ptr()),
            _ptr(column_indices_t), _ptr(permutation))
    _check(fn(ctypes.c_void_p(0), ctypes.byref(size), *args, ctypes.c_void_p(0), 0), "mspmv_csr_transpose (size query)")
    temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=dev)
    _check(fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), *args, _stream_handle(stream), 0), "mspmv_csr_transpose")
    if stream is not None and hasattr(stream, "cuda_stream"):
        temp.record_stream(stream)        # (the allocator must not hand `temp` out again before the conversion on `stream` has run)
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
        vb = _value_bytes(values)
        fn = load_library().mspmv_csr_transpose_values_f32 if vb == 4 else load_library().mspmv_csr_transpose_values_f64
        _check(fn(_ptr(values), _ptr(self.permutation), _ptr(self.values_t), self.nnz, _stream_handle(stream), 0),
               "mspmv_csr_transpose_values")
        return self

    def __call__(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, stream=None):
        return csrmv(self.values_t, self.row_offsets_t, self.column_indices_t, x, y, num_cols=self.rows, workspace=self.workspace,
                     stream=stream, alpha=alpha, beta=beta)

    def matmul(self, X, Y=None, alpha: float = 1.0, beta: float = 0.0, stream=None):
        return csrmm(self.values_t, self.row_offsets_t, self.column_indices_t, X, Y, alpha=alpha, beta=beta, stream=stream)


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


def _two_phase(fn, what, dev, stream, args, temp=None):
    """size query, temp allocation (or `temp` when it is large enough), the call on `stream`; returns the temp tensor"""
    import torch
    size = ctypes.c_size_t(0)
    _check(fn(ctypes.c_void_p(0), ctypes.byref(size), *args, ctypes.c_void_p(0), 0), what + " (size query)")
    fresh = temp is None or temp.numel() < size.value
    if fresh:
        temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=dev)
    size = ctypes.c_size_t(temp.numel())
    _check(fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), *args, _stream_handle(stream), 0), what)
    if fresh and stream is not None and hasattr(stream, "cuda_stream"):
        temp.record_stream(stream)        # (the allocator must not hand `temp` out again before the work on `stream` has run)
    return temp


def csr_sum_duplicates(values, row_offsets, column_indices, num_cols: int, stream=None):
    """Merges the duplicate entries of a CSR whose rows are sorted by column (mspmv_csr_sum_duplicates_*): each run of equal (row,
    column) becomes one entry, its values added left to right in the value type.  Returns (values_out, row_offsets_out,
    column_indices_out, count): the arrays keep nnz entries, of which the first `count` (a one-element int32 CUDA tensor) are
    written.  values=None: structure only.  Asynchronous on `stream`; nothing is read back."""
    import torch
    if row_offsets is None or not row_offsets.is_cuda or row_offsets.dtype != torch.int32 or not row_offsets.is_contiguous():
        raise MspmvError("csr_sum_duplicates: row_offsets must be a contiguous int32 CUDA tensor")
    rows, cols, nnz = row_offsets.numel() - 1, int(num_cols), column_indices.numel()
    dev = row_offsets.device
    if rows < 0 or column_indices.dtype != torch.int32 or column_indices.device != dev or not column_indices.is_contiguous():
        raise MspmvError(f"csr_sum_duplicates: column_indices must be a contiguous int32 tensor on {dev}, row_offsets needs rows + 1 entries")
    if values is not None and (values.dtype not in (torch.float32, torch.float64) or values.device != dev or not values.is_contiguous()
                               or values.numel() != nnz):
        raise MspmvError(f"csr_sum_duplicates: values must be a contiguous float32 / float64 tensor of {nnz} entries on {dev}")
    dtype = torch.float32 if values is None else values.dtype
    lib = load_library()
    fn = lib.mspmv_csr_sum_duplicates_f32 if dtype == torch.float32 else lib.mspmv_csr_sum_duplicates_f64
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
    lib = load_library()
    fn = lib.mspmv_coo_to_csr_f32 if dtype == torch.float32 else lib.mspmv_coo_to_csr_f64
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
        lib = load_library()
        self._fn = lib.mspmv_coo_to_csr_f32 if self.dtype == torch.float32 else lib.mspmv_coo_to_csr_f64
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
        vb = _value_bytes(values)
        fn = load_library().mspmv_coo_to_csr_values_f32 if vb == 4 else load_library().mspmv_coo_to_csr_values_f64
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
    lib = load_library()
    fn = lib.mspmv_coomv_f32 if dtype == torch.float32 else lib.mspmv_coomv_f64
    ct = ctypes.c_float if dtype == torch.float32 else ctypes.c_double
    args = (_ptr(values), _ptr(row_indices), _ptr(column_indices), _ptr(x), _ptr(y), rows, cols, nnz, ct(1.0 if alpha is None else alpha),
            ct(0.0 if beta is None else beta))
    size = ctypes.c_size_t(0)
    _check(fn(ctypes.c_void_p(0), ctypes.byref(size), *args, ctypes.c_void_p(0), 0), "mspmv_coomv (size query)")
    temp = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=dev)
    _check(fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(size), *args, _stream_handle(stream), int(bool(debug_synchronous))), "mspmv_coomv")
    if stream is not None and hasattr(stream, "cuda_stream"):
        temp.record_stream(stream)
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
        lib = load_library()
        self._fn = lib.mspmv_csr_add_f32 if self.dtype == torch.float32 else lib.mspmv_csr_add_f64
        self._ct = ctypes.c_float if self.dtype == torch.float32 else ctypes.c_double
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
        lib = load_library()
        self._fn = lib.mspmv_csr_gemm_f32 if self.dtype == torch.float32 else lib.mspmv_csr_gemm_f64
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


class _PlanArray:
    """plan-owned device memory seen by torch (torch.as_tensor reads __cuda_array_interface__: no copy)"""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<i4", "data": (int(ptr), False), "version": 2, "strides": None}


class CsrSv:
    """The level-scheduled sparse triangular solve (mspmv_csrsv_*): op(A) x = alpha * b for one right-hand side.  The constructor
    analyses the PATTERN (synchronous; the plan owns what it allocates); `solve` runs on any values with that pattern.  `lower`
    chooses the triangle, `unit_diagonal` the diagonal; entries of the other triangle (and, with a unit diagonal, stored diagonals) are
    ignored, so a full matrix may be swept with both of its parts.  include/mspmv.h states the bits of x.
    .info: the plan's figures (levels, launches, narrow_rows, bad_diagonal_row, ...); .order: the rows sorted stably by level;
    .level_offsets: levels + 1 entries (both int32 tensors on the matrix's device, copies)."""

    def __init__(self, row_offsets, column_indices, lower: bool = True, unit_diagonal: bool = False, stream=None,
                 debug_synchronous: bool = False):
        import torch
        self._handle = None
        for t, name in ((row_offsets, "row_offsets"), (column_indices, "column_indices")):
            if not isinstance(t, torch.Tensor):
                raise MspmvError(f"CsrSv: {name} must be a tensor")
        if not (row_offsets.is_cuda and column_indices.is_cuda):
            raise MspmvError("CsrSv needs CUDA (HIP) tensors: the kernels only run on the GPU")
        if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
            raise TypeError("CsrSv: row_offsets / column_indices must be int32")
        if row_offsets.dim() != 1 or row_offsets.numel() < 1 or not row_offsets.is_contiguous() or column_indices.dim() != 1 \
                or not column_indices.is_contiguous() or column_indices.device != row_offsets.device:
            raise MspmvError("CsrSv: row_offsets (rows + 1 entries) and column_indices must be contiguous 1-D tensors on one device")
        self.device = row_offsets.device
        self.rows, self.nnz = row_offsets.numel() - 1, column_indices.numel()
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

    def _array(self, fn, count):
        import torch
        if self._handle is None:
            raise MspmvError("CsrSv: the plan is closed")
        ptr = fn(self._handle)
        if not ptr or count == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        return torch.as_tensor(_PlanArray(ptr, count), device=self.device).clone()

    @property
    def order(self):
        return self._array(self._lib.mspmv_csrsv_plan_order, self.rows)

    @property
    def level_offsets(self):
        import torch
        if self.rows == 0:                                         # (a plan of no rows holds nothing on the device)
            return torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._array(self._lib.mspmv_csrsv_plan_level_offsets, self.info["levels"] + 1)

    def solve(self, values, b, x=None, alpha: float = 1.0, stream=None, debug_synchronous: bool = False):
        """x = the solution of op(A) x = alpha * b on `values` (the plan's pattern); x may be b (in place).  Asynchronous on `stream`;
        info["launches"] launches, nothing allocated but a missing x, nothing read back."""
        import torch
        if self._handle is None:
            raise MspmvError("CsrSv: the plan is closed")
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
        fn, ct = (self._lib.mspmv_csrsv_solve_f32, ctypes.c_float) if b.dtype == torch.float32 else (self._lib.mspmv_csrsv_solve_f64, ctypes.c_double)
        _check(int(fn(self._handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), ct(alpha), _ptr(b), _ptr(x),
                      _stream_handle(stream), int(bool(debug_synchronous)))), "mspmv_csrsv_solve")
        return x

    def many_info(self, k: int) -> dict:
        """The figures of mspmv_csrsm_info for k right-hand sides on this plan: k, lanes_per_row (P), passes, narrow_lanes, launches."""
        if self._handle is None:
            raise MspmvError("CsrSv: the plan is closed")
        raw = _CsrSmInfo()
        _check(self._lib.mspmv_csrsm_info(self._handle, int(k), ctypes.byref(raw)), "mspmv_csrsm_info")
        return {name: int(getattr(raw, name)) for name, _ in _CsrSmInfo._fields_}

    def solve_many(self, values, B, X=None, alpha: float = 1.0, stream=None, debug_synchronous: bool = False):
        """X = the solution of op(A) X = alpha * B for the k columns of B (mspmv_csrsm_solve_*), column j bit for bit what `solve` gives
        for column j.  B and X: [rows, k], row-major (stride(1) == 1, stride(0) >= k: the leading dimension is the stride, as in csrmm);
        X may be B (in place).  Asynchronous on `stream`; many_info(k)["launches"] launches, nothing allocated but a missing X."""
        import torch
        if self._handle is None:
            raise MspmvError("CsrSv: the plan is closed")
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
        fn, ct = (self._lib.mspmv_csrsm_solve_f32, ctypes.c_float) if B.dtype == torch.float32 else (self._lib.mspmv_csrsm_solve_f64, ctypes.c_double)
        _check(int(fn(self._handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), ct(alpha), _ptr(B), int(ldb), _ptr(X),
                      int(ldx), k, _stream_handle(stream), int(bool(debug_synchronous)))), "mspmv_csrsm_solve")
        return X

    def close(self):
        if getattr(self, "_handle", None) is not None:
            handle, self._handle = self._handle, None
            self._lib.mspmv_csrsv_plan_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csrsv(values, row_offsets, column_indices, b, lower: bool = True, unit_diagonal: bool = False, alpha: float = 1.0):
    """One-shot triangular solve: analyse the pattern, solve op(A) x = alpha * b, drop the plan.  A loop keeps a CsrSv."""
    plan = CsrSv(row_offsets, column_indices, lower=lower, unit_diagonal=unit_diagonal)
    try:
        return plan.solve(values, b, alpha=alpha)
    finally:
        import torch
        torch.cuda.current_stream(plan.device).synchronize()
        plan.close()


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
    for t, name in ((values, "values"), (row_offsets, "row_offsets"), (column_indices, "column_indices")):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"{what}: {name} must be a tensor")
    if not (values.is_cuda and row_offsets.is_cuda and column_indices.is_cuda):
        raise MspmvError(f"{what} needs CUDA (HIP) tensors: the kernels only run on the GPU")
    if values.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} is instantiated for float32 and float64, got {values.dtype}")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise TypeError(f"{what}: row_offsets / column_indices must be int32")
    if row_offsets.dim() != 1 or row_offsets.numel() < 1 or not row_offsets.is_contiguous() or column_indices.dim() != 1 \
            or not column_indices.is_contiguous() or column_indices.device != row_offsets.device:
        raise MspmvError(f"{what}: row_offsets (rows + 1 entries) and column_indices must be contiguous 1-D tensors on one device")
    rows, nnz = row_offsets.numel() - 1, column_indices.numel()
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
    fn = getattr(plan._lib, f"mspmv_{family}_f32" if values.dtype == torch.float32 else f"mspmv_{family}_f64")
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


class _Factor0:
    """What Ilu0 and Ic0 share: the LOWER and UPPER plans of one pattern, the temp storage, the pivot, the factor of the last `factor`
    and the kept vector and block between the two sweeps.  A subclass states _unit_lower (its lower plan's unit_diagonal), _temp_bytes
    and _call (its factorisation), and shows the factor under its public name."""

    def __init__(self, row_offsets, column_indices, stream=None):
        import torch
        name = type(self).__name__
        self.lower = self.upper = None
        for t, tname in ((row_offsets, "row_offsets"), (column_indices, "column_indices")):
            if not isinstance(t, torch.Tensor):
                raise MspmvError(f"{name}: {tname} must be a tensor")
        if not (row_offsets.is_cuda and column_indices.is_cuda):
            raise MspmvError(f"{name} needs CUDA (HIP) tensors: the kernels only run on the GPU")
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
        for plan in (getattr(self, "lower", None), getattr(self, "upper", None)):
            if plan is not None:
                plan.close()
        self.lower = self.upper = None
        self._temp = self._factor = self._mid = self._mid_many = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


def _pattern_check(what, row_offsets, column_indices):
    """the checks the C ABI cannot make for a CSR pattern; returns (device, rows, nnz)"""
    import torch
    for t, name in ((row_offsets, "row_offsets"), (column_indices, "column_indices")):
        if not isinstance(t, torch.Tensor):
            raise MspmvError(f"{what}: {name} must be a tensor")
    if not (row_offsets.is_cuda and column_indices.is_cuda):
        raise MspmvError(f"{what} needs CUDA (HIP) tensors: the kernels only run on the GPU")
    if row_offsets.dtype != torch.int32 or column_indices.dtype != torch.int32:
        raise MspmvError(f"{what}: row_offsets / column_indices must be int32")
    if row_offsets.dim() != 1 or row_offsets.numel() < 1 or not row_offsets.is_contiguous() or column_indices.dim() != 1 \
            or not column_indices.is_contiguous() or column_indices.device != row_offsets.device:
        raise MspmvError(f"{what}: row_offsets (rows + 1 entries) and column_indices must be contiguous 1-D tensors on one device")
    return row_offsets.device, row_offsets.numel() - 1, column_indices.numel()


def _index_check(what, t, name, need, dev, dtypes=None):
    import torch
    dtypes = dtypes or (torch.int32,)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or t.device != dev or t.dim() != 1 \
            or not t.is_contiguous() or t.numel() != need:
        raise MspmvError(f"{what}: {name} must be a contiguous 1-D {' / '.join(str(d) for d in dtypes)} tensor of {need} entries on {dev}")


class CsrColoring:
    """The deterministic multicolouring of a square CSR pattern (mspmv_csr_color_*; include/mspmv.h states the definition): u and v are
    neighbours when A[u,v] or A[v,u] is stored, and color[v] is the smallest colour that no neighbour of larger key holds, key(v) =
    priorities[v] << 32 | v (priorities: rows entries, int32 or uint32, their 32 bits read as unsigned; None: a hash of the index).  The
    constructor analyses the PATTERN (synchronous; the handle owns what it allocates).
    .colors, .order (the vertices sorted stably by colour), .inverse (inverse[order[i]] = i), .offsets (num_colors + 1 entries): int32
    tensors on the pattern's device (copies); .num_colors; .info: the handle's figures (colors, max_color_rows, rounds, edges, ...).
    `permute_vector(v)` is v[order], `permute_vector(v, back=True)` v[inverse]; csr_permute(..., row_perm=.order, col_map=.inverse) is
    P A P^T, whose LOWER CsrSv plan has at most num_colors levels."""

    def __init__(self, row_offsets, column_indices, priorities=None, stream=None, debug_synchronous: bool = False):
        import torch
        self._handle = None
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
        import torch
        if name not in self._kept:
            if self._handle is None:
                raise MspmvError("CsrColoring: the handle is closed")
            ptr = getattr(self._lib, "mspmv_csr_color_" + name)(self._handle)
            if not ptr or count == 0:
                self._kept[name] = torch.zeros(count, dtype=torch.int32, device=self.device)
            else:
                self._kept[name] = torch.as_tensor(_PlanArray(ptr, count), device=self.device).clone()
        return self._kept[name]

    colors = property(lambda self: self._array("colors", self.rows))
    order = property(lambda self: self._array("order", self.rows))
    inverse = property(lambda self: self._array("inverse", self.rows))
    offsets = property(lambda self: self._array("offsets", self.num_colors + 1))

    def permute_vector(self, v, back: bool = False, out=None, stream=None):
        """v[order] (the vector in the multicolour numbering), or with back=True v[inverse] (back in the original numbering), through
        mspmv_coo_to_csr_values_*.  Asynchronous on `stream`."""
        import torch
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype not in (torch.float32, torch.float64) or v.device != self.device \
                or v.dim() != 1 or not v.is_contiguous() or v.numel() != self.rows:
            raise MspmvError(f"CsrColoring.permute_vector: v must be a contiguous 1-D float32 / float64 tensor of {self.rows} entries on {self.device}")
        if out is None:
            out = torch.empty_like(v)
        if not isinstance(out, torch.Tensor) or out.dtype != v.dtype or out.device != v.device or out.dim() != 1 or not out.is_contiguous() \
                or out.numel() != self.rows or out.data_ptr() == v.data_ptr() and self.rows > 0:
            raise MspmvError("CsrColoring.permute_vector: out must be another contiguous tensor of v's dtype, length and device")
        index = self.inverse if back else self.order
        fn = self._lib.mspmv_coo_to_csr_values_f32 if v.dtype == torch.float32 else self._lib.mspmv_coo_to_csr_values_f64
        _check(fn(_ptr(v), _ptr(index), _ptr(out), self.rows, _stream_handle(stream), 0), "mspmv_coo_to_csr_values")
        return out

    def close(self):
        if getattr(self, "_handle", None) is not None:
            handle, self._handle = self._handle, None
            self._lib.mspmv_csr_color_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_color(row_offsets, column_indices, priorities=None):
    """One-shot colouring: (colors, num_colors) of the pattern (CsrColoring keeps the order, its inverse and the offsets too)."""
    coloring = CsrColoring(row_offsets, column_indices, priorities)
    try:
        return coloring.colors, coloring.num_colors
    finally:
        coloring.close()


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
    if values is not None and (not isinstance(values, torch.Tensor) or values.dtype not in (torch.float32, torch.float64) or values.device != dev
                               or values.dim() != 1 or not values.is_contiguous() or values.numel() != nnz):
        raise MspmvError(f"csr_permute: values must be a contiguous 1-D float32 / float64 tensor of {nnz} entries on {dev}")
    if row_perm is not None:
        _index_check("csr_permute", row_perm, "row_perm", rows, dev)
    if col_map is not None:
        _index_check("csr_permute", col_map, "col_map", cols, dev)
    dtype = torch.float32 if values is None else values.dtype
    lib = load_library()
    fn = lib.mspmv_csr_permute_f32 if dtype == torch.float32 else lib.mspmv_csr_permute_f64
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


def multicolor_reorder(values, row_offsets, column_indices, priorities=None, stream=None):
    """(coloring, csr): the CsrColoring of a square pattern and P A P^T = csr_permute(values, ..., row_perm=coloring.order,
    col_map=coloring.inverse).  Solve P A P^T x' = coloring.permute_vector(b); x = coloring.permute_vector(x', back=True)."""
    coloring = CsrColoring(row_offsets, column_indices, priorities, stream=stream)
    return coloring, csr_permute(values, row_offsets, column_indices, coloring.rows, row_perm=coloring.order, col_map=coloring.inverse,
                                 stream=stream)


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
    lib = load_library()
    fn = lib.mspmv_vec_dot_f32 if a.dtype == torch.float32 else lib.mspmv_vec_dot_f64
    with torch.cuda.device(a.device):
        _two_phase(fn, "mspmv_vec_dot", a.device, stream, (_ptr(a), _ptr(b), a.numel(), ctypes.c_void_p(out.data_ptr())), temp=temp)
    return out


_PCG_KINDS = {"none": 0, "jacobi": 1, "factor": 2}
PCG_STATUS = ("RUNNING", "CONVERGED", "BREAKDOWN")


class Pcg:
    """Preconditioned conjugate gradients on the device (mspmv_pcg_*; include/mspmv.h states the arithmetic bit for bit) for one CSR
    pattern and value type.  preconditioner: None, "jacobi", an Ic0 or Ilu0 that holds a factor (its two CsrSv plans and its factor are
    used, and kept alive, as they are), or (first CsrSv, second CsrSv, factor values[, factor row_offsets, factor column_indices]):
    z = second^-1 (first^-1 r) (the pattern arrays default to the matrix's).  The constructor allocates and is synchronous.
    `solve` returns x; `.state` then reads the state block back (synchronises): status ("RUNNING" | "CONVERGED" | "BREAKDOWN"),
    iterations, rr, bb, stop2, rz, launches_per_iteration, ...; `.history` (after solve(history=True)): the tensor of rr, entries
    0 .. iterations."""

    def __init__(self, row_offsets, column_indices, dtype, preconditioner=None, stream=None, debug_synchronous: bool = False):
        import torch
        self._handle = None
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
        if self._handle is None:
            raise MspmvError("Pcg: closed")
        raw = _PcgState()
        _check(self._lib.mspmv_pcg_state(self._handle, ctypes.byref(raw), _stream_handle(stream) if self.rows > 0 else None), "mspmv_pcg_state")
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
        if self._handle is None:
            raise MspmvError("Pcg: closed")
        guess = x is not None
        if x is None:
            x = torch.empty(self.rows, dtype=self.dtype, device=self.device)
        for t, name, need in ((values, "values", self.nnz), (b, "b", self.rows), (x, "x", self.rows)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != self.dtype or t.device != self.device or t.dim() != 1 \
                    or not t.is_contiguous() or t.numel() != need:
                raise MspmvError(f"Pcg.solve: {name} must be a contiguous 1-D {self.dtype} tensor of {need} entries on {self.device}")
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
        fn = self._lib.mspmv_pcg_solve_f32 if self.dtype == torch.float32 else self._lib.mspmv_pcg_solve_f64
        with torch.cuda.device(self.device):
            _check(fn(self._handle, _ptr(values), _ptr(self.row_offsets), _ptr(self.column_indices), _ptr(b), _ptr(x), int(guess), float(rtol),
                      float(atol), int(max_iterations), int(check_every), _ptr(history), _stream_handle(stream), int(bool(debug_synchronous))),
                   "mspmv_pcg_solve")
        return x

    def close(self):
        if getattr(self, "_handle", None) is not None:
            handle, self._handle = self._handle, None
            self._lib.mspmv_pcg_destroy(handle)
        self._kept = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pcg(values, row_offsets, column_indices, b, preconditioner="ic0", reorder: bool = True, x=None, rtol: float = 1e-8, atol: float = 0.0,
        max_iterations: int = 1000, check_every: int = 8, stream=None, return_state: bool = False):
    """One-shot A x = b for a symmetric positive definite CSR matrix (sorted rows, no duplicates, structurally symmetric for "ic0").
    preconditioner: "ic0" | "jacobi" | None.  With reorder (and "ic0") the matrix is permuted to multicolour order
    (multicolor_reorder), IC(0) is made of P A P^T, the system is solved in that numbering and x is mapped back
    (CsrColoring.permute_vector(back=True)): x, and a guess given as x, are in the caller's numbering.  Returns x, or (x, state) with
    return_state.  A loop over right-hand sides or values keeps a Pcg (and the Ic0 and CsrColoring) instead."""
    if preconditioner not in ("ic0", "jacobi", None):
        raise MspmvError(f"pcg: unknown preconditioner {preconditioner!r}")
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
            ic = Ic0(off, col, stream=stream)
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
        fn = load_library().mspmv_csrmv_plan_build_f32 if self.vb == 4 else load_library().mspmv_csrmv_plan_build_f64
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
        fn = load_library().mspmv_csrmv_plan_apply_f32 if self.vb == 4 else load_library().mspmv_csrmv_plan_apply_f64
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
        lib = load_library()
        fn = lib.mspmv_csrmv_hotcols_permute_f32 if self.vb == 4 else lib.mspmv_csrmv_hotcols_permute_f64
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
        lib = load_library()
        if x_is_permuted:
            fn = lib.mspmv_csrmv_hotcols_apply_permuted_f32 if self.vb == 4 else lib.mspmv_csrmv_hotcols_apply_permuted_f64
        else:
            fn = lib.mspmv_csrmv_hotcols_apply_f32 if self.vb == 4 else lib.mspmv_csrmv_hotcols_apply_f64
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


def launch_info(num_rows: int, num_nonzeros: int, value_bytes: int, num_cols: Optional[int] = None) -> dict:
    """mspmv_get_launch_info; with `num_cols` mspmv_get_launch_info_cols: exactly the layout a stateless call of these sizes runs (one
    family of calls -- large fp64 matrices of short rows over a tiny x -- picks its tile shape by the column count too)."""
    info = _LaunchInfo()
    if num_cols is None:
        _check(load_library().mspmv_get_launch_info(int(num_rows), int(num_nonzeros), int(value_bytes),
                                                    ctypes.byref(info)), "mspmv_get_launch_info")
    else:
        _check(load_library().mspmv_get_launch_info_cols(int(num_rows), int(num_cols), int(num_nonzeros), int(value_bytes),
                                                         ctypes.byref(info)), "mspmv_get_launch_info_cols")
    return {name: getattr(info, name) for name, _ in _LaunchInfo._fields_}


def serial_sum_depth(num_rows: int, num_cols: int, num_nonzeros: int, value_bytes: int, extra: int = 0) -> int:
    """How many products one thread of the tile kernel adds up serially before the scan tree takes over, for a call of these
    sizes -- the compiled tile's items per thread rounded up to whole 4-element chunks -- plus one re-association per
    column-band pass the call may run, plus `extra` (parts of a multi-GPU split, bands of a prepared plan).  It is the
    `items_per_thread` term of the stated error bound |y - g| <= 2 (ceil(log2(len + 1)) + items_per_thread + 8) eps s
    (DESIGN.md 3): derived from the compiled shape, so the bound follows the library when a shape changes."""
    ipt = launch_info(num_rows, num_nonzeros, value_bytes)["items_per_thread"]
    return 4 * (ipt // 4 + 1) + max(band_passes(num_rows, num_cols, num_nonzeros, value_bytes), 0) + int(extra)


def set_tuning(value_bytes: int, block_threads: int = 0, items_per_thread: int = 0, flags: int = 0) -> None:
    """mspmv_set_tuning (development library: a non-default value switches to it, see _setter)."""
    _setter("mspmv_set_tuning", block_threads == 0 and items_per_thread == 0 and flags == 0,
            int(value_bytes), int(block_threads), int(items_per_thread), int(flags))


def profile_begin(max_calls: int) -> None:
    """Record hipEvents around the three kernels of the next `max_calls` CsrMV calls."""
    _check(load_library().mspmv_profile_begin(int(max_calls)), "mspmv_profile_begin")


def profile_end() -> dict:
    """Average per-call milliseconds of each pass since profile_begin()."""
    calls = ctypes.c_int32()
    ms = [ctypes.c_float() for _ in range(3)]
    _check(load_library().mspmv_profile_end(ctypes.byref(calls), *[ctypes.byref(m) for m in ms]), "mspmv_profile_end")
    return {"calls": calls.value, "search_ms": ms[0].value, "tile_ms": ms[1].value, "fixup_ms": ms[2].value}


def set_band_passes(value_bytes: int, passes: int = 0) -> None:
    """Column-band passes (mspmv_set_band_passes): 0 automatic, < 0 never, >= 2 always that many."""
    _setter("mspmv_set_band_passes", passes == 0, int(value_bytes), int(passes))


def set_tdm(value_bytes: int, policy: int = 0, slot_permille: int = 0, lookahead_plus_1: int = 0, band_shift: int = 0) -> None:
    """Clock-scheduled column bands (mspmv_set_tdm): policy 0 the library's rule, < 0 never (the passes), > 0 always where the passes are offered."""
    _setter("mspmv_set_tdm", policy == 0 and slot_permille == 0 and lookahead_plus_1 == 0 and band_shift == 0,
            int(value_bytes), int(policy), int(slot_permille), int(lookahead_plus_1), int(band_shift))


def device_caches() -> dict:
    """What the column-band policy is derived from (mspmv_get_device_caches): one XCD's L2 bytes, XCD count, CU count."""
    l2 = ctypes.c_int64(0); x = ctypes.c_int32(0); c = ctypes.c_int32(0)
    lib = load_library()
    lib.mspmv_get_device_caches.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.mspmv_get_device_caches(ctypes.byref(l2), ctypes.byref(x), ctypes.byref(c)), "mspmv_get_device_caches")
    return {"l2_bytes_per_xcd": l2.value, "xcds": x.value, "cus": c.value}


def set_record_polls(polls: int = 0) -> None:
    """Testing aid (mspmv_set_record_polls): 0 = library default, 1 = one look, -1 = never look: tiles in which a long row ends
    compute the pieces held by other workgroups themselves instead of taking the published records."""
    _setter("mspmv_set_record_polls", polls == 0, int(polls))


def cache_stream_rate(nbytes: int, reps: int = 20) -> float:
    """GB/s of a bare 16-byte-per-lane read stream (mspmv_probe_read_stream, ordinary loads) over a buffer of `nbytes` that has been
    read before -- for nbytes within the 256 MB Infinity Cache this is the rate out of that cache (and the L2s), the bound a
    cache-resident SpMV's algorithmic bytes are to be read against (bench.py)."""
    import time
    import torch
    lib = load_library()
    lib.mspmv_probe_read_stream.restype = ctypes.c_int
    lib.mspmv_probe_read_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_void_p]
    n = max(int(nbytes) // 16 * 16, 16)
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = _stream_handle(None)
    for _ in range(3):
        _check(lib.mspmv_probe_read_stream(ctypes.c_void_p(buf.data_ptr()), n, 0, st), "mspmv_probe_read_stream")
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        lib.mspmv_probe_read_stream(ctypes.c_void_p(buf.data_ptr()), n, 0, st)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    del buf
    return n / dt / 1e9


def set_compact_tiles(max_tiles: int = 0) -> None:
    """Testing / tuning aid (mspmv_set_compact_tiles): up to how many tiles a call of the small tile shape runs the one-launch kernel
    behind its compact front end (0 = library default, > 0 = that many, < 0 = never).  y is bit for bit the same either way."""
    _setter("mspmv_set_compact_tiles", max_tiles == 0, int(max_tiles))


def clocked_bands(rows: int, cols: int, nnz: int, value_bytes: int):
    """(bands, columns per band) of the clock-scheduled form for a call of these sizes (mspmv_get_clocked_bands); (0, 0): not a candidate."""
    b = ctypes.c_int32(0); c = ctypes.c_int32(0)
    lib = load_library()
    lib.mspmv_get_clocked_bands.restype = ctypes.c_int
    lib.mspmv_get_clocked_bands.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)] * 2
    _check(lib.mspmv_get_clocked_bands(int(rows), int(cols), int(nnz), int(value_bytes), ctypes.byref(b), ctypes.byref(c)), "mspmv_get_clocked_bands")
    return b.value, c.value


def band_passes(rows: int, cols: int, nnz: int, value_bytes: int) -> int:
    """Passes a call of these sizes is offered (0: none); automatic setting: subject to the device-side verdicts."""
    n = ctypes.c_int32(0)
    _check(load_library().mspmv_get_band_passes(int(rows), int(cols), int(nnz), int(value_bytes), ctypes.byref(n)), "mspmv_get_band_passes")
    return n.value


def debug_band_windows(workspace, rows: int, nnz: int, value_bytes: int):
    """The 64 window verdicts the last automatic large-problem call left in the workspace (numpy int32[64])."""
    import numpy as np
    out = np.zeros(64, np.int32)
    tmp = workspace.buffer if hasattr(workspace, "buffer") else workspace
    _check(load_library().mspmv_debug_band_windows(ctypes.c_void_p(tmp.data_ptr()), int(rows), int(nnz), int(value_bytes),
                                                   out.ctypes.data_as(ctypes.c_void_p), None), "mspmv_debug_band_windows")
    return out


def debug_read_tiles(workspace_buffer, num_rows: int, num_nonzeros: int, value_bytes: int, stream=None):
    """(coords[num_tiles+1, 2], carry_keys[num_tiles], carry_values[num_tiles])
    left in temp storage by the last CsrMV call, as numpy arrays."""
    import numpy as np
    info = launch_info(num_rows, num_nonzeros, value_bytes)
    nt = info["num_tiles"]
    coords = np.zeros((nt + 1, 2), dtype=np.int32)
    keys = np.zeros(max(nt, 1), dtype=np.int32)
    vals = np.zeros(max(nt, 1), dtype=np.float32 if value_bytes == 4 else np.float64)
    _check(load_library().mspmv_debug_read_tiles(
        ctypes.c_void_p(workspace_buffer.data_ptr()), int(num_rows), int(num_nonzeros), int(value_bytes),
        coords.ctypes.data_as(ctypes.c_void_p), keys.ctypes.data_as(ctypes.c_void_p),
        vals.ctypes.data_as(ctypes.c_void_p), _stream_handle(stream)), "mspmv_debug_read_tiles")
    return coords, keys[:nt], vals[:nt]


def sampled_check(A, x, y, samples: int = 1 << 16, seed: int = 0x5A3D, depth: Optional[int] = None) -> dict:
    """An untimed correctness witness for a benchmark record (NOT the parity tests: those are tests/ -m gpu against the oracle):
    `samples` seeded rows -- plus the first, the last and the longest row -- recomputed on the device in fp64 with torch gathers
    (val.double() * x.double()[col], rows up to 4096 nonzeros by index_add_, longer ones by torch.sum's tree) and compared with
    y under the stated bound of SURVEY 8d / DESIGN 3: |y - g| <= 2 (ceil(log2(len + 1)) + depth + 8) eps s, s = sum |val x|,
    eps = 2^-24 / 2^-53, empty rows exactly zero.  depth = serial_sum_depth of the call's shape unless given.
    Returns {"rows_checked", "worst_ratio" (max |y - g| / bound; < 1 passes), "violations", "longest_row"}."""
    import torch
    rows, nnz = int(A.rows), int(A.nnz)
    dev = A.values.device
    if rows == 0:
        return {"rows_checked": 0, "worst_ratio": 0.0, "violations": 0, "longest_row": 0}
    vb = A.values.element_size()
    if depth is None:
        depth = serial_sum_depth(rows, A.cols, nnz, vb)
    eps = 2.0 ** -24 if vb == 4 else 2.0 ** -53
    off = A.row_offsets.to(torch.int64)
    lens_all = off[1:] - off[:-1]
    g = torch.Generator(device="cpu"); g.manual_seed(int(seed))
    pick = torch.randint(0, rows, (min(int(samples), rows),), generator=g, dtype=torch.int64).to(dev)
    longest = int(torch.argmax(lens_all).item())
    pick = torch.unique(torch.cat([pick, torch.tensor([0, rows - 1, longest], dtype=torch.int64, device=dev)]))
    lens = lens_all[pick]
    start = off[pick]
    gold = torch.zeros(pick.numel(), dtype=torch.float64, device=dev)
    mag = torch.zeros_like(gold)
    xd = x.double()
    short = lens <= 4096
    if bool(short.any()):
        sl = lens[short]; st = start[short]
        total = int(sl.sum().item())
        if total > 0:
            seg = torch.repeat_interleave(torch.arange(sl.numel(), device=dev), sl)
            first = torch.cumsum(sl, 0) - sl
            j = st[seg] + (torch.arange(total, device=dev) - first[seg])
            p = A.values[j].double() * xd[A.column_indices[j].to(torch.int64)]
            gs = torch.zeros(sl.numel(), dtype=torch.float64, device=dev); ms = torch.zeros_like(gs)
            gs.index_add_(0, seg, p); ms.index_add_(0, seg, p.abs())
            gold[short] = gs; mag[short] = ms
    for k in torch.nonzero(~short).flatten().tolist():          # a handful of long rows: tree sums
        a, b = int(start[k].item()), int(start[k].item() + lens[k].item())
        gk, mk = 0.0, 0.0
        for c0 in range(a, b, 1 << 26):
            c1 = min(b, c0 + (1 << 26))
            p = A.values[c0:c1].double() * xd[A.column_indices[c0:c1].to(torch.int64)]
            gk += float(p.sum().item()); mk += float(p.abs().sum().item())
        gold[k] = gk; mag[k] = mk
    yy = y[pick].double()
    c = 2.0 * (torch.ceil(torch.log2(lens.double() + 1.0)) + float(depth) + 8.0)
    bound = c * eps * mag
    err = (yy - gold).abs()
    bad_empty = (lens == 0) & (y[pick] != 0)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isfinite(yy), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where(bad_empty, torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max().item())
    return {"rows_checked": int(pick.numel()), "worst_ratio": round(worst, 4) if worst != float("inf") else "inf",
            "violations": int((ratio > 1.0).sum().item()), "longest_row": int(lens_all[longest].item()), "depth_term": int(depth)}
