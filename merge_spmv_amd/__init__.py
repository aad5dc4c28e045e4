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

This file only gathers the names; the code lives, one operation family per module, in
  _lib        the loader (library_path / use_library / load_library) and the one table of C prototypes
  _args       pointers, streams, argument checks, the two-phase temp call, the handle base class
  csrmv       DeviceSpmv, csrmv, csrmv_mixed, csrmm, CsrMVWorkspace
  convert     transpose, COO, duplicate summing, coomv, add, gemm, permute, sddmm
  fill        CsrFill, csr_fill: level-of-fill patterns, the symbolic phase of ILU(k) / IC(k) (include/mspmv_fill.h, libmspmv_fill.so, a
              library of its own); attributes of the package, not in __all__
  solve       CsrSv (csrsv, csrsm), ILU(0), IC(0); Iluk, Ick: the same on a filled pattern (attributes of the package, not in __all__)
  reorder     CsrColoring, csr_color, multicolor_reorder
  _solver     what Pcg, Bicgstab and Gmres share: the loader of a layer library, the solver base class, the one-shot body
  krylov      vec_dot, Pcg, pcg
  bicgstab    Bicgstab, bicgstab, BICGSTAB_EXIT: the Krylov layer on top of the C ABI (include/mspmv_krylov.h, libmspmv_krylov.so, which
              always runs on the product libmspmv.so next to it); attributes of the package, not in __all__
  gmres       Gmres, gmres, GMRES_EXIT: restarted GMRES(m), the same kind of layer (include/mspmv_gmres.h, libmspmv_gmres.so);
              attributes of the package, not in __all__
  plans       CsrMVPlan, CsrMVHotColumns and bench.py's records of them
  introspect  launch_info, the setters of the development library, profiling, debug readers, sampled_check
(multi_gpu and generators are imported by name, as before).  Imports run down this list only.
"""
from ._lib import (TUNE_ATOMIC_FIX, TUNE_NO_VEC, MspmvError, _CsrColorInfo, _CsrSmInfo, _CsrSvInfo, _LaunchInfo, _PcgState, _check,
                   _libs, _setter, active_library, library_path, load_library, use_library)
from ._args import (_coo_check, _index_check, _many_layout, _pattern_check, _PlanArray, _ptr, _stream_handle, _two_phase, _validate,
                    _value_bytes)
from .introspect import (band_passes, cache_stream_rate, clocked_bands, debug_band_windows, debug_read_tiles, device_caches, launch_info,
                         profile_begin, profile_end, sampled_check, serial_sum_depth, set_band_passes, set_compact_tiles,
                         set_record_polls, set_tdm, set_tuning)
from .csrmv import CsrMVWorkspace, DeviceSpmv, csrmm, csrmv, csrmv_mixed
from .convert import (CooToCsr, CsrAdd, CsrGemm, CsrTranspose, coo_to_csr, coomv, csr_add, csr_gemm, csr_gemm_products, csr_permute,
                      csr_sum_duplicates, csr_symmetrize, csr_transpose, sddmm)
from .fill import CsrFill, csr_fill
from .solve import (CsrSv, Ic0, Ick, Ilu0, Iluk, _ic0_call, _ic0_temp_bytes, _ilu0_call, _ilu0_temp_bytes, csric0, csric0_group, csrilu0,
                    csrilu0_group, csrsm, csrsv)
from .reorder import CsrColoring, csr_color, multicolor_reorder
from .krylov import PCG_STATUS, Pcg, pcg, vec_dot
from .bicgstab import BICGSTAB_EXIT, Bicgstab, bicgstab
from .gmres import GMRES_EXIT, Gmres, gmres
from .plans import CsrMVHotColumns, CsrMVPlan, hotcols_bench_record, plan_bench_record

__all__ = ["DeviceSpmv", "csrmv", "csrmv_mixed", "csrmm", "CsrMVWorkspace", "CsrMVPlan", "csr_transpose", "CsrTranspose", "coo_to_csr", "CooToCsr", "csr_sum_duplicates", "coomv",
           "csr_add", "CsrAdd", "csr_symmetrize", "csr_gemm", "CsrGemm", "csr_gemm_products", "sddmm", "CsrSv", "csrsv", "csrsm", "csrilu0", "Ilu0", "csric0", "Ic0",
           "CsrColoring", "csr_color", "csr_permute", "multicolor_reorder", "vec_dot", "Pcg", "pcg",
           "plan_bench_record", "library_path", "load_library", "launch_info",
           "set_tuning", "set_tdm", "clocked_bands", "debug_read_tiles", "profile_begin", "profile_end", "MspmvError",
           "TUNE_ATOMIC_FIX", "TUNE_NO_VEC"]
