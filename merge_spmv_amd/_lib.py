"""The loader of libmspmv.so / libmspmv_dev.so and the ONE table of their C prototypes (include/mspmv.h, include/mspmv_dev.h).
Every other module of the package reaches the library through load_library(); tests/test_abi_prototypes.py holds what the table
sets against the headers."""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAMES = {"product": "libmspmv.so", "dev": "libmspmv_dev.so"}
_libs = {}                 # kind -> ctypes.CDLL (only ever mutated: merge_spmv_amd._libs is this dict)
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
    """Make `kind` ("product" | "dev") the library every wrapper of this package calls from now on; returns the previous kind.  The
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


class _MgInfo(ctypes.Structure):
    _fields_ = [("parts", ctypes.c_int32), ("local_parts", ctypes.c_int32), ("exchange", ctypes.c_int32),
                ("value_bytes", ctypes.c_int32), ("replicas", ctypes.c_int32), ("hot_parts", ctypes.c_int32),
                ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("carry_bytes_per_step", ctypes.c_uint64),
                ("allgather_bytes_per_step", ctypes.c_uint64), ("steps", ctypes.c_uint64)]


# One letter per argument (blanks only group them for the eye):
_TOKENS = {
    "p": ctypes.c_void_p,                       # any pointer that is passed through: device or host array, handle, stream
    "i": ctypes.c_int32, "l": ctypes.c_int64, "n": ctypes.c_int, "z": ctypes.c_size_t, "d": ctypes.c_double,
    "Z": ctypes.POINTER(ctypes.c_size_t), "I": ctypes.POINTER(ctypes.c_int32), "F": ctypes.POINTER(ctypes.c_float),
    "H": ctypes.POINTER(ctypes.c_void_p),       # where a *_create writes its handle
    "L": ctypes.POINTER(_LaunchInfo), "S": ctypes.POINTER(_CsrSvInfo), "M": ctypes.POINTER(_CsrSmInfo),
    "C": ctypes.POINTER(_CsrColorInfo), "G": ctypes.POINTER(_PcgState),
    # "v": the scalar type of the variant (alpha, beta): float for *_f32 and *_bf16_f32, double for *_f64 and *_f32_f64
}
_RETURNS = {"n": ctypes.c_int, "p": ctypes.c_void_p, "s": ctypes.c_char_p}
_F = ("_f32", "_f64")
_MIXED = ("_f32_f64", "_bf16_f32")
_CSRMV = "pZ ppppp iii vv pn"                   # temp, &bytes, values, offsets, columns, x, y, rows, cols, nnz, alpha, beta, stream, debug

# (names after "mspmv_", variants, arguments[, return]): every function of include/mspmv.h; _SETTERS: those of include/mspmv_dev.h
_PROTOTYPES = (
    ("version", (), ""),
    ("error_string", (), "n", "s"),
    ("csrmv", _F, "pZ ppppp iii pn"),
    ("csrmv_axpby csrmv_prepared csrmv_transpose coomv", _F, _CSRMV),
    ("csrmv_mixed csrmv_mixed_prepared", _MIXED, _CSRMV),
    ("csrmv_prepare", (), "pZ p iii pn"),
    ("csrmm", _F, "pZ ppp pi pi iiii vv pn"),
    ("get_launch_info", (), "iii L"),
    ("get_launch_info_cols", (), "iiii L"),
    ("get_band_passes", (), "iiii I"),
    ("get_clocked_bands", (), "iiii II"),
    ("get_device_caches", (), "ppp"),
    ("probe_read_stream", (), "p z i p"),
    ("debug_read_tiles", (), "p iii ppp p"),
    ("debug_band_windows", (), "p iii p p"),
    ("profile_begin", (), "i"),
    ("profile_end", (), "I FFF"),
    ("csrmv_plan_size", (), "iiiii Z I"),
    ("csrmv_plan_build", _F, "pz ppp iiii pn"),
    ("csrmv_plan_apply", _F, "pz pp iiii vv pn"),
    ("csrmv_plan_row_offsets csrmv_plan_columns csrmv_plan_values", (), "p iiiii", "p"),
    ("csrmv_hotcols_skew", (), "p iii p II"),
    ("csrmv_hotcols_size", (), "iiii Z"),
    ("csrmv_hotcols_build", (), "pz pp iiii pn"),
    ("csrmv_hotcols_apply csrmv_hotcols_apply_permuted", _F, "pz pppp iii vv pn"),
    ("csrmv_hotcols_permute", _F, "pz pp iii pn"),
    ("csrmv_hotcols_order csrmv_hotcols_columns", (), "p iiii", "p"),
    ("csr_transpose coo_to_csr csr_sum_duplicates", _F, "pZ ppp iii pppp pn"),
    ("csr_transpose_values coo_to_csr_values", _F, "ppp i pn"),
    ("csr_add", _F, "pZ ii v ppp i v ppp i pppp pn"),
    ("csr_gemm_products", (), "pZ pp iii p i p pn"),
    ("csr_gemm", _F, "pZ iii ppp i ppp i ii pppp pn"),
    ("csr_permute", _F, "pZ ppp iii pp pppp pn"),
    ("sddmm", _F + ("_bf16_f32",), "pp pi pi p iiii vv pn"),
    ("csrsv_plan_create", (), "H pp iiii pn"),
    ("csrsv_plan_info", (), "p S"),
    ("csrsv_plan_order csrsv_plan_level_offsets", (), "p", "p"),
    ("csrsv_solve", _F, "pppp v pp pn"),
    ("csrsm_info", (), "p i M"),
    ("csrsm_solve", _F, "pppp v pi pi i pn"),
    ("csrilu0_group csric0_group", (), "ii I"),
    ("csrilu0", _F, "p pZ pppp p pn"),
    ("csric0", _F, "p pZ pppp i p pn"),
    ("csr_color_create", (), "H pp ii p pn"),
    ("csr_color_info", (), "p C"),
    ("csr_color_colors csr_color_order csr_color_inverse csr_color_offsets", (), "p", "p"),
    ("vec_dot", _F, "pZ pp l p pn"),
    ("pcg_create", (), "H pp iiii pn"),
    ("pcg_set_factor", (), "p pp ppp"),
    ("pcg_solve", _F, "p ppp pp i dd ii p pn"),
    ("pcg_state", (), "p G p"),
    ("csrsv_plan_destroy csr_color_destroy pcg_destroy", (), "p"),
    ("mg_partition", (), "p ll i pp"),
    ("mg_local_offsets", (), "p lllll p"),
    ("mg_apply_carries", (), "ppp iii p"),
    ("mg_unique_id", (), "p"),
    ("mg_plan_create", (), "H ii pppp l ii p"),
    ("mg_plan_set_part", (), "p i ppp"),
    ("mg_plan_hot_columns", (), "p i"),
    ("mg_plan_ipc_export", (), "pp Z"),
    ("mg_plan_ipc_import", (), "pp i z"),
    ("mg_plan_x mg_plan_y mg_plan_stream", (), "p i", "p"),
    ("mg_plan_info", (), "pp"),
    ("mg_plan_exchange_ms", (), "p i p"),
    ("mg_csrmv mg_allgather_rows mg_synchronize mg_plan_destroy", (), "p"),
)
_SETTERS = (
    ("set_tuning", (), "iiii"),
    ("set_band_passes", (), "ii"),
    ("set_record_polls set_compact_tiles", (), "i"),
    ("set_tdm", (), "iiiii"),
)


def _prototype(lib, table) -> None:
    for names, variants, args, *ret in table:
        for variant in variants or ("",):
            scalar = ctypes.c_float if variant.endswith("_f32") else ctypes.c_double
            argtypes = [scalar if a == "v" else _TOKENS[a] for a in args.replace(" ", "")]
            for name in names.split():
                fn = getattr(lib, "mspmv_" + name + variant)
                fn.restype = _RETURNS[ret[0] if ret else "n"]
                fn.argtypes = argtypes


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
    _prototype(lib, _PROTOTYPES)
    if hasattr(lib, "mspmv_set_tuning"):          # (the development library, or an MSPMV_LIB build that has the setters)
        _prototype(lib, _SETTERS)
    _libs[_active] = lib
    return lib


def _setter(name: str, default: bool, *args) -> None:
    """The setters of include/mspmv_dev.h.  The product library has none: asking it for the defaults is a no-op; asking for anything else
    switches this package to the development library (use_library("dev")) -- the same kernels with the per-thread overrides compiled in."""
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
