"""Times SDDMM on the device (mspmv_sddmm_*) against rocSPARSE's rocsparse_sddmm on the same arrays:
python tools/sddmm_bench.py [--reps 10] > profiles/sddmm_bench.txt

Cases: BASELINE config 2's pattern (3.1 M x 3.1 M, 100 M uniformly random entries); a 5-point grid of 2000 x 2000 points; an R-MAT
graph of scale 22; and 2^24 entries in ONE row (the balance case); fp32, fp64 and bf16 (fp32 C), k = 16, 64, 128; alpha = 1 and
beta = 0 unless --beta says otherwise.  U and V are dense row-major with ld = k, values uniform in [-1, 1).  Per case: the median of
--reps calls, each between its own events after a warm-up, the spread (max - min) / median, and GB/s of ALGORITHMIC bytes, counted as
    nnz x (4 + sizeof C x (1, or 2 when beta != 0)) + (rows + cols) x k x sizeof element
-- every column index and every C once, every row of U and V once; the gathers that re-read rows of V are not counted, so the figure
says how close a case comes to streaming its operands once.  The result of every case is checked before it is timed, over ALL
entries in chunks, against the dot products in fp64 by torch: within (k + 2) roundings of |alpha| sum|u v| + |beta c|.  rocSPARSE
(through ctypes, the library of tools/rocsparse_ref.py) runs rocsparse_sddmm with its default algorithm, A = U (row-major), op(B) =
the transpose of V (row-major); rocsparse_sddmm_buffer_size and rocsparse_sddmm_preprocess run once, outside the timing; its result
is checked against OURS within the same bound before it is timed."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R

DTYPES = {"f32": (torch.float32, torch.float32, 151), "f64": (torch.float64, torch.float64, 152), "bf16": (torch.bfloat16, torch.float32, 168)}
CHUNK = 1 << 21                                                  # entries per step of the check


def dense(n, k, dtype, seed):
    return G.uniform_pm1(seed, n * k, torch.float32 if dtype == torch.bfloat16 else dtype, "cuda").to(dtype).view(n, k)


def case_c2():
    a = G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float32)
    return "config 2: 3.1 M x 3.1 M, 32 per row, uniform", a.rows, a.cols, a.row_offsets, a.column_indices


def case_grid():
    k = 2000
    idx = torch.arange(k * k, device="cuda", dtype=torch.int64).view(k, k)
    pairs = [(idx, idx), (idx[1:], idx[:-1]), (idx[:-1], idx[1:]), (idx[:, 1:], idx[:, :-1]), (idx[:, :-1], idx[:, 1:])]
    keys = torch.sort(torch.cat([(r * (k * k) + c).reshape(-1) for r, c in pairs])).values
    off = torch.zeros(k * k + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // (k * k), minlength=k * k), 0)
    return "5-point grid 2000 x 2000", k * k, k * k, off.to(torch.int32), (keys % (k * k)).to(torch.int32)


def case_rmat(scale=22):
    a = G.rmat_csr(scale, 16 << scale, dtype=torch.float32)
    return f"R-MAT scale {scale}, {16 << scale} edges", a.rows, a.cols, a.row_offsets, a.column_indices


def case_one_row():
    n = 1 << 24
    return "2^24 entries in ONE row", 1, n, torch.tensor([0, n], device="cuda", dtype=torch.int32), torch.arange(n, device="cuda", dtype=torch.int32)


CASES = {"c2": case_c2, "grid": case_grid, "rmat": case_rmat, "onerow": case_one_row}


def entry_rows(off, rows):
    return torch.repeat_interleave(torch.arange(rows, device="cuda", dtype=torch.int64), torch.diff(off.to(torch.int64)))


def check(r, col, U, V, alpha, beta, old, got, what, reference=None):
    """got against the fp64 dot products (or against `reference`) within (k + 2) roundings of |alpha| sum|u v| + |beta c|"""
    k = U.shape[1]
    eps = 2.0 ** -53 if got.dtype == torch.float64 else 2.0 ** -24
    worst = 0.0
    for a in range(0, col.numel(), CHUNK):
        b = min(a + CHUNK, col.numel())
        p = U[r[a:b]].to(torch.float64) * V[col[a:b].to(torch.int64)].to(torch.float64)
        mag = abs(alpha) * p.abs().sum(1)
        want = alpha * p.sum(1)
        if beta != 0:
            want += beta * old[a:b].to(torch.float64)
            mag += (beta * old[a:b].to(torch.float64)).abs()
        if reference is not None:
            want = reference[a:b].to(torch.float64)
        err = (got[a:b].to(torch.float64) - want).abs()
        bound = (k + 2) * eps * mag
        assert bool((err <= bound).all()), f"{what}: an entry is off by more than (k + 2) roundings"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max().item()))
    return worst


def timed(fn, reps, warm=2):
    times = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if i >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times) * 100


def rocsparse_sddmm(off, col, U, V, rows, cols, alpha, beta, old, ours, r, reps, key):
    """(median ms, spread %) of rocsparse_sddmm (default algorithm) after buffer_size + preprocess, its result checked against ours"""
    L = R.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    in_type, c_type = DTYPES[key][2], (152 if ours.dtype == torch.float64 else 151)
    k = U.shape[1]
    ct = ctypes.c_double if ours.dtype == torch.float64 else ctypes.c_float
    a_, b_ = ct(alpha), ct(beta)
    out = old.clone() if beta else torch.zeros_like(old)         # (beta == 0: no NaN that a multiply by zero would keep)
    handle, dA, dB, dC = vp(), vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    p = lambda t: vp(t.data_ptr())
    row_major, none, transpose, default_alg = i32(0), i32(111), i32(112), i32(0)
    st = L.rocsparse_create_dnmat_descr(ctypes.byref(dA), i64(rows), i64(k), i64(k), p(U), i32(in_type), row_major)
    if st != 0 and key == "bf16":                                # (a rocSPARSE build whose descriptors do not take rocsparse_datatype_bf16_r)
        L.rocsparse_destroy_handle(handle)
        return None
    assert st == 0, f"rocsparse_create_dnmat_descr: {st}"
    assert L.rocsparse_create_dnmat_descr(ctypes.byref(dB), i64(cols), i64(k), i64(k), p(V), i32(in_type), row_major) == 0
    assert L.rocsparse_create_csr_descr(ctypes.byref(dC), i64(rows), i64(cols), i64(col.numel()), p(off), p(col), p(out), i32(2), i32(2), i32(0),
                                        i32(c_type)) == 0
    size = ctypes.c_size_t(0)
    args = (handle, none, transpose, ctypes.byref(a_), dA, dB, ctypes.byref(b_), dC, i32(c_type), default_alg)
    st = L.rocsparse_sddmm_buffer_size(*args, ctypes.byref(size))
    assert st == 0, f"rocsparse_sddmm_buffer_size: {st}"
    buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")
    st = L.rocsparse_sddmm_preprocess(*args, p(buf))
    assert st == 0, f"rocsparse_sddmm_preprocess: {st}"

    def call():
        st = L.rocsparse_sddmm(*args, p(buf))
        assert st == 0, f"rocsparse_sddmm: {st}"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record()
    torch.cuda.synchronize()
    reps = min(reps, max(3, int(2000 / max(e0.elapsed_time(e1), 1e-3))))       # (a call of seconds is timed 3 times, not --reps)
    check(r, col, U, V, alpha, beta, old, out, "rocsparse_sddmm against ours", reference=ours)
    ms = timed(call, reps, warm=1)
    L.rocsparse_destroy_spmat_descr(dC); L.rocsparse_destroy_dnmat_descr(dA); L.rocsparse_destroy_dnmat_descr(dB); L.rocsparse_destroy_handle(handle)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="c2,grid,rmat,onerow")
    ap.add_argument("--dtypes", default="f32,f64,bf16")
    ap.add_argument("--ks", default="16,64,128")
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--rocsparse-skip", default="", help="cases on which rocSPARSE is not run (its one-row case takes 13-48 s per call)")
    ap.add_argument("--no-header", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sddmm_bench needs a GPU"
    alpha, beta = 1.0, args.beta
    if not args.no_header:
        print(f"# sddmm_bench: {torch.cuda.get_device_name(0)}, median of {args.reps} calls, each between its own events; alpha = {alpha}, "
              f"beta = {beta}; GB/s of nnz x (4 + sizeof C x {2 if beta else 1}) + (rows + cols) x k x sizeof element; rocSPARSE = "
              f"rocsparse_sddmm, default algorithm, buffer_size + preprocess outside the timing, result checked against ours")
    for case in args.cases.split(","):
        name, rows, cols, off, col = CASES[case]()
        r = entry_rows(off, rows)
        nnz = col.numel()
        for key in args.dtypes.split(","):
            in_dt, out_dt, _ = DTYPES[key]
            for k in (int(x) for x in args.ks.split(",")):
                U, V = dense(rows, k, in_dt, 11), dense(cols, k, in_dt, 12)
                old = G.uniform_pm1(13, nnz, out_dt, "cuda") if beta else torch.full((nnz,), float("nan"), dtype=out_dt, device="cuda")
                out = old.clone()
                call = lambda: M.sddmm(off, col, U, V, out=out, alpha=alpha, beta=beta)
                call()
                torch.cuda.synchronize()
                worst = check(r, col, U, V, alpha, beta, old, out, "mspmv_sddmm")
                ours = out.clone()
                ms, spread = timed(call, args.reps)
                nbytes = nnz * (4 + out.element_size() * (2 if beta else 1)) + (rows + cols) * k * U.element_size()
                line = (f"{name:46s} {key:4s} k {k:3d}  nnz {nnz:9d}  {ms:9.3f} ms  spread {spread:4.1f} %  {nbytes / ms / 1e6:7.1f} GB/s  "
                        f"(worst error {worst:4.2f} of the bound)")
                if not args.no_rocsparse and case not in args.rocsparse_skip.split(","):
                    res = rocsparse_sddmm(off, col, U, V, rows, cols, alpha, beta, old, ours, r, args.reps, key)
                    if res is None:
                        line += "  | rocSPARSE: this build's dense descriptors refuse bf16"
                    else:
                        line += f"  | rocSPARSE {res[0]:9.3f} ms  spread {res[1]:4.1f} %  rocSPARSE / ours = {res[0] / ms:6.2f}"
                print(line, flush=True)
                del U, V, old, out, ours
                torch.cuda.empty_cache()
        del r, off, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
