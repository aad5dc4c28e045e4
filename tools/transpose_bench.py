"""tools/transpose_bench.py -- the device transpose against rocSPARSE (profiles/transpose_bench.txt).

Per matrix: the conversion (mspmv_csr_transpose_*, values and permutation) against rocsparse_?csr2csc (numeric), with the
conversion's bytes against 8 TB/s; A^T x through a built transpose (CsrTranspose: the forward call on A^T with prepared
coordinates), through the stateless mspmv_csrmv_transpose_*, and rocSPARSE's csrmv with the transpose operation; the forward A x
for scale.  Every time is the average of `--reps` calls between two hipEvents after warm-up.  Development / reporting aid.

    python tools/transpose_bench.py [--only c2_f32,grid2d] [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import merge_spmv_amd as M                                  # noqa: E402
from merge_spmv_amd import generators as G                  # noqa: E402
from tools import rocsparse_ref as R                        # noqa: E402

vp, i32 = ctypes.c_void_p, ctypes.c_int


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def conversion_bytes(rows, cols, nnz, vb):
    """(the least a conversion can move: read A, write A^T and the permutation; what this one moves: the first pass reads A,
    every pass reads its keys twice (histogram, scatter), every pass but the first reads and every pass writes (key, row, k, value),
    the last kernel reads the keys and writes the offsets)"""
    least = 4 * (rows + 1) + nnz * (4 + vb) + 4 * (cols + 1) + nnz * (4 + vb) + 4 * nnz
    bits = max(1, (cols - 1).bit_length()) if cols > 1 else 0
    passes = max(1, -(-bits // 8))
    item = 12 + vb
    moved = 4 * (rows + 1) + nnz * (4 + vb)                 # pass 0 reads A
    moved += passes * 4 * nnz                               # the histograms' key reads
    moved += (passes - 1) * item * nnz + passes * item * nnz
    moved += 4 * nnz + 4 * (cols + 1)
    return least, moved, passes


def rocsparse_csr2csc(A, reps):
    L = R.lib()
    handle = vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    f32 = A.values.dtype == torch.float32
    size = ctypes.c_size_t(0)
    assert L.rocsparse_csr2csc_buffer_size(handle, i32(A.rows), i32(A.cols), i32(A.nnz), vp(A.row_offsets.data_ptr()),
                                           vp(A.column_indices.data_ptr()), i32(1), ctypes.byref(size)) == 0
    buf = torch.empty(max(size.value, 1), dtype=torch.uint8, device="cuda")
    val_t = torch.empty_like(A.values)
    row_t = torch.empty(A.nnz, dtype=torch.int32, device="cuda")
    off_t = torch.empty(A.cols + 1, dtype=torch.int32, device="cuda")
    fn = L.rocsparse_scsr2csc if f32 else L.rocsparse_dcsr2csc

    def call():
        st = fn(handle, i32(A.rows), i32(A.cols), i32(A.nnz), vp(A.values.data_ptr()), vp(A.row_offsets.data_ptr()),
                vp(A.column_indices.data_ptr()), vp(val_t.data_ptr()), vp(row_t.data_ptr()), vp(off_t.data_ptr()), i32(1), i32(0),
                vp(buf.data_ptr()))
        assert st == 0, st
    ms = timed(call, reps)
    L.rocsparse_destroy_handle(handle)
    return ms, (val_t, off_t, row_t)


def rocsparse_csrmv_t(A, x, reps):
    """rocsparse_?csrmv with rocsparse_operation_transpose (y has cols entries); analysis when the library offers it for the
    transpose, else without info"""
    L = R.lib()
    handle, descr, info = vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    assert L.rocsparse_create_mat_info(ctypes.byref(info)) == 0
    f32 = A.values.dtype == torch.float32
    ct = ctypes.c_float if f32 else ctypes.c_double
    ana = L.rocsparse_scsrmv_analysis if f32 else L.rocsparse_dcsrmv_analysis
    mv = L.rocsparse_scsrmv if f32 else L.rocsparse_dcsrmv
    args = (i32(A.rows), i32(A.cols), i32(A.nnz))
    if ana(handle, i32(112), *args, descr, vp(A.values.data_ptr()), vp(A.row_offsets.data_ptr()), vp(A.column_indices.data_ptr()), info) != 0:
        info = vp()
    y = torch.empty(A.cols, dtype=A.values.dtype, device="cuda")
    alpha, beta = ct(1.0), ct(0.0)

    def call():
        st = mv(handle, i32(112), *args, ctypes.byref(alpha), descr, vp(A.values.data_ptr()), vp(A.row_offsets.data_ptr()),
                vp(A.column_indices.data_ptr()), info, vp(x.data_ptr()), ctypes.byref(beta), vp(y.data_ptr()))
        assert st == 0, st
    ms = timed(call, reps)
    if info.value:
        L.rocsparse_destroy_mat_info(info)
    L.rocsparse_destroy_mat_descr(descr); L.rocsparse_destroy_handle(handle)
    return ms, y


def run(label, A, reps):
    lib = M.load_library()
    vb = A.values.element_size()
    sfx = "f32" if vb == 4 else "f64"
    dev = A.values.device
    out = {"matrix": label, "rows": A.rows, "cols": A.cols, "nnz": A.nnz, "dtype": sfx}
    # the conversion, buffers allocated once
    conv = getattr(lib, "mspmv_csr_transpose_" + sfx)
    size = ctypes.c_size_t(0)
    val_t = torch.empty_like(A.values); off_t = torch.empty(A.cols + 1, dtype=torch.int32, device=dev)
    col_t = torch.empty(A.nnz, dtype=torch.int32, device=dev); perm = torch.empty(A.nnz, dtype=torch.int32, device=dev)
    args = (vp(A.values.data_ptr()), vp(A.row_offsets.data_ptr()), vp(A.column_indices.data_ptr()), A.rows, A.cols, A.nnz,
            vp(val_t.data_ptr()), vp(off_t.data_ptr()), vp(col_t.data_ptr()), vp(perm.data_ptr()))
    assert conv(None, ctypes.byref(size), *args, None, 0) == 0
    temp = torch.empty(size.value, dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    out["convert_ms"] = timed(lambda: conv(vp(temp.data_ptr()), ctypes.byref(size), *args, stream, 0), reps)
    out["convert_temp_bytes"] = int(size.value)
    least, moved, passes = conversion_bytes(A.rows, A.cols, A.nnz, vb)
    out.update(passes=passes, convert_bytes_least=least, convert_bytes_moved=moved,
               convert_ms_at_8tbs_least=least / 8e9, convert_ms_at_8tbs_moved=moved / 8e9)
    out["rocsparse_csr2csc_ms"], ref = rocsparse_csr2csc(A, reps)
    # rocSPARSE's stable csr2csc gives the same arrays (a cross-check of both)
    out["same_as_rocsparse_csr2csc"] = bool(torch.equal(ref[1], off_t) and torch.equal(ref[2], col_t) and torch.equal(ref[0], val_t))
    del ref
    # A^T x: built transpose (prepared), stateless, rocSPARSE; A x for scale
    x = G.uniform_pm1(12345, A.rows, A.values.dtype, "cuda")
    xf = G.uniform_pm1(12346, A.cols, A.values.dtype, "cuda")
    t = M.CsrTranspose(A.values, A.row_offsets, A.column_indices, A.cols)
    y_t = torch.empty(A.cols, dtype=A.values.dtype, device=dev)
    out["atx_built_ms"] = timed(lambda: t(x, y_t), reps)
    del temp
    st = getattr(lib, "mspmv_csrmv_transpose_" + sfx)
    ct = ctypes.c_float if vb == 4 else ctypes.c_double
    y_s = torch.empty(A.cols, dtype=A.values.dtype, device=dev)
    sargs = (vp(A.values.data_ptr()), vp(A.row_offsets.data_ptr()), vp(A.column_indices.data_ptr()), vp(x.data_ptr()), vp(y_s.data_ptr()),
             A.rows, A.cols, A.nnz, ct(1.0), ct(0.0))
    ssize = ctypes.c_size_t(0)
    assert st(None, ctypes.byref(ssize), *sargs, None, 0) == 0
    stemp = torch.empty(ssize.value, dtype=torch.uint8, device=dev)
    out["atx_stateless_ms"] = timed(lambda: st(vp(stemp.data_ptr()), ctypes.byref(ssize), *sargs, stream, 0), reps)
    del stemp
    out["atx_stateless_equals_built"] = bool(torch.equal(y_s, t(x)))
    out["rocsparse_csrmv_transpose_ms"], y_r = rocsparse_csrmv_t(A, x, reps)
    d = (y_r.double() - y_s.double()).abs().max().item() if A.cols else 0.0
    out["rocsparse_transpose_max_abs_diff"] = d
    ws = M.CsrMVWorkspace(A.rows, A.nnz, A.values.dtype).prepare(A.row_offsets)
    y_f = torch.empty(A.rows, dtype=A.values.dtype, device=dev)
    out["ax_forward_ms"] = timed(lambda: M.csrmv(A.values, A.row_offsets, A.column_indices, xf, y_f, num_cols=A.cols, workspace=ws), reps)
    return out


MATRICES = {
    "c2_f32": lambda: ("C2 uniform 3125000^2, 32/row, fp32", G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float32)),
    "c2_f64": lambda: ("C2 uniform 3125000^2, 32/row, fp64", G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float64)),
    "c3": lambda: ("C3 stand-in: R-MAT scale 20, 3105536 edges, fp64", G.rmat_csr(20, 3_105_536, dtype=torch.float64, seed=G.SEED_C3)),
    "c4": lambda: ("C4 degenerate_csr (2^24 rows, a 2^26-entry row), fp32", G.degenerate_csr(dtype=torch.float32)),
    "grid2d": lambda: ("grid2d 2000 (4 M rows, 5-point), fp64", G.grid2d_csr(2000, dtype=torch.float64)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(MATRICES))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for key in a.only.split(","):
        label, A = MATRICES[key]()
        rec = run(label, A, a.reps)
        print(json.dumps(rec), flush=True)
        del A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
