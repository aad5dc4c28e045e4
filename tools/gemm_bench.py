"""Times C = A * B on the device (mspmv_csr_gemm_*) against rocSPARSE's csrgemm on the same arrays:
python tools/gemm_bench.py [--reps 10] > profiles/gemm_bench.txt

Cases: A A^T for a 5-point grid of 2000 x 2000 points; A A for a uniformly random matrix of 1 M rows with 8 entries per row; A A^T for
an R-MAT graph of scale 18 (long runs: a hot column of A meets itself); P A for a 0/1 aggregation matrix P that adds four neighbouring
rows of the grid (the multigrid shape); and one entry of A per row into ONE row of B with 2^24 entries (the balance case); fp32 and
fp64.  Per case: the median of --reps calls, each between its own events after a warm-up, the spread (max - min) / median, and
picoseconds per product.  The result of every case is checked before it is timed against a torch restatement: the products expanded
with repeat_interleave, the sorted unique keys row * cols + column compared exactly, the values against the products added in fp64 by
index_add_ within 2 (longest run + 1) roundings of the sum of the magnitudes (both sides round).  rocSPARSE (through ctypes, tools/rocsparse_ref.py)
runs rocsparse_[sd]csrgemm_buffer_size + rocsparse_csrgemm_nnz + rocsparse_[sd]csrgemm per call in DEVICE pointer mode, so that neither
side reads anything back on the host; its buffer is allocated once, outside the timing.  Its row pointers must equal ours and its
column indices, sorted within each row, must equal ours before it is timed (rocSPARSE does not sort the rows of C)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from merge_spmv_amd.generators import DeviceCsr
from tools import rocsparse_ref as R

MAX_PRODUCTS = 400_000_000                                       # (a case is shrunk until it stays below: about 26 / 34 GB of temp storage)


def values(n, dtype, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    return (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(dtype)


def from_keys(keys, rows, cols, dtype, seed):
    """a canonical CSR from sorted unique int64 keys row * cols + col"""
    off = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // cols, minlength=rows), 0)
    return DeviceCsr(rows, cols, off.to(torch.int32), (keys % cols).to(torch.int32), values(keys.numel(), dtype, seed))


def rows_of(m):
    return torch.repeat_interleave(torch.arange(m.rows, device="cuda", dtype=torch.int64), torch.diff(m.row_offsets.to(torch.int64)))


def transposed(a):
    vt, ot, ct, _ = M.csr_transpose(a.values, a.row_offsets, a.column_indices, a.cols)
    return DeviceCsr(a.cols, a.rows, ot, ct, vt)


def grid(k, dtype):
    idx = torch.arange(k * k, device="cuda", dtype=torch.int64).view(k, k)
    pairs = [(idx, idx), (idx[1:], idx[:-1]), (idx[:-1], idx[1:]), (idx[:, 1:], idx[:, :-1]), (idx[:, :-1], idx[:, 1:])]
    keys = torch.sort(torch.cat([(r * (k * k) + c).reshape(-1) for r, c in pairs])).values
    return from_keys(keys, k * k, k * k, dtype, 3)


def case_grid(dtype):
    a = grid(2000, dtype)
    return "5-point grid 2000 x 2000: A A^T", a, transposed(a)


def case_uniform(dtype):
    a = G.uniform_csr(1_000_000, 1_000_000, 8, dtype=dtype)
    return "uniform 1 M rows x 8 per row: A A", a, a


def case_rmat(dtype, scale=18):
    edges = 16 << scale
    while True:
        r, c = (t.to(torch.int32) for t in G.rmat_edges(scale, 0, edges, "cuda", G.SEED_C5)[:2])
        a = M.coo_to_csr(values(edges, dtype, 6), r, c, 1 << scale, 1 << scale, sum_duplicates=True)
        at = transposed(a)
        if M.csr_gemm_products(a, at) <= MAX_PRODUCTS:
            return f"R-MAT scale {scale}, {edges} edges merged: A A^T", a, at
        edges //= 2


def case_galerkin(dtype):
    a = grid(2000, dtype)
    n = a.rows
    p = DeviceCsr(n // 4, n, torch.arange(0, n + 1, 4, device="cuda", dtype=torch.int32), torch.arange(n, device="cuda", dtype=torch.int32),
                  torch.ones(n, device="cuda", dtype=dtype))
    return "aggregation P (4 rows into 1) times the grid: P A", p, a


def case_balance(dtype):
    rows, n = 8, 1 << 24
    a = DeviceCsr(rows, 1, torch.arange(rows + 1, device="cuda", dtype=torch.int32), torch.zeros(rows, device="cuda", dtype=torch.int32),
                  values(rows, dtype, 8))
    b = DeviceCsr(1, n, torch.tensor([0, n], device="cuda", dtype=torch.int32), torch.arange(n, device="cuda", dtype=torch.int32),
                  values(n, dtype, 9))
    return "8 rows of one entry into ONE row of 2^24 entries", a, b


CASES = {"grid": case_grid, "uniform": case_uniform, "rmat": case_rmat, "galerkin": case_galerkin, "balance": case_balance}


def check(a, b, c, products):
    """C against the torch restatement: keys exactly, values within 2 (longest run + 1) eps of the sum of the magnitudes"""
    lens = torch.diff(b.row_offsets.to(torch.int64))[a.column_indices.to(torch.int64)]
    assert int(lens.sum().item()) == products
    start = torch.cumsum(lens, 0) - lens
    e = torch.repeat_interleave(torch.arange(lens.numel(), device="cuda", dtype=torch.int64), lens)
    j = b.row_offsets.to(torch.int64)[a.column_indices.to(torch.int64)][e] + torch.arange(products, device="cuda", dtype=torch.int64) - start[e]
    key = rows_of(a)[e] * b.cols + b.column_indices.to(torch.int64)[j]
    want, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    got = rows_of(c) * c.cols + c.column_indices.to(torch.int64)
    assert torch.equal(got, want), "the pattern of C differs"
    del key, got
    p = a.values.to(torch.float64)[e] * b.values.to(torch.float64)[j]
    s = torch.zeros(want.numel(), dtype=torch.float64, device="cuda").index_add_(0, inverse, p)
    mag = torch.zeros(want.numel(), dtype=torch.float64, device="cuda").index_add_(0, inverse, p.abs())
    eps = 2.0 ** -24 if c.values.dtype == torch.float32 else 2.0 ** -53
    longest = int(counts.max().item())
    assert bool(((c.values.to(torch.float64) - s).abs() <= 2 * (longest + 1) * eps * mag).all()), "the values of C differ"
    return longest


def timed(fn, reps, warm=2):
    times = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times) * 100


def rocsparse_gemm(a, b, ours, reps):
    """(median ms, spread %) of csrgemm_buffer_size + csrgemm_nnz + csrgemm in device pointer mode, after its pattern was compared"""
    L = R.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    f32 = a.values.dtype == torch.float32
    size_fn = L.rocsparse_scsrgemm_buffer_size if f32 else L.rocsparse_dcsrgemm_buffer_size
    gemm = L.rocsparse_scsrgemm if f32 else L.rocsparse_dcsrgemm
    handle, descr, info = vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_set_pointer_mode(handle, i32(1)) == 0     # rocsparse_pointer_mode_device
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    assert L.rocsparse_create_mat_info(ctypes.byref(info)) == 0
    na, nb, count = a.column_indices.numel(), b.column_indices.numel(), ours.column_indices.numel()
    alpha = torch.ones(1, dtype=a.values.dtype, device="cuda")
    off = torch.empty(a.rows + 1, dtype=torch.int32, device="cuda")
    col = torch.empty(count, dtype=torch.int32, device="cuda")
    val = torch.empty(count, dtype=a.values.dtype, device="cuda")
    nnz = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: vp(t.data_ptr())
    none, op = vp(0), i32(111)                                   # rocsparse_operation_none
    size = ctypes.c_size_t(0)

    def query():
        st = size_fn(handle, op, op, i32(a.rows), i32(b.cols), i32(a.cols), p(alpha), descr, i32(na), p(a.row_offsets), p(a.column_indices),
                     descr, i32(nb), p(b.row_offsets), p(b.column_indices), none, descr, i32(0), none, none, info, ctypes.byref(size))
        assert st == 0, st
    query()
    buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")

    def call():
        query()
        assert size.value <= buf.numel()
        st = L.rocsparse_csrgemm_nnz(handle, op, op, i32(a.rows), i32(b.cols), i32(a.cols), descr, i32(na), p(a.row_offsets), p(a.column_indices),
                                     descr, i32(nb), p(b.row_offsets), p(b.column_indices), descr, i32(0), none, none, descr, p(off), p(nnz),
                                     info, p(buf))
        assert st == 0, st
        st = gemm(handle, op, op, i32(a.rows), i32(b.cols), i32(a.cols), p(alpha), descr, i32(na), p(a.values), p(a.row_offsets),
                  p(a.column_indices), descr, i32(nb), p(b.values), p(b.row_offsets), p(b.column_indices), none, descr, i32(0), none, none, none,
                  descr, p(val), p(off), p(col), info, p(buf))
        assert st == 0, st
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record()
    torch.cuda.synchronize()
    reps = min(reps, max(3, int(4000 / max(e0.elapsed_time(e1), 1e-3))))       # (a call of seconds is timed 3 times, not --reps)
    assert int(nnz.item()) == count and torch.equal(off, ours.row_offsets), "patterns differ"
    keys = rows_of(ours) * ours.cols
    assert torch.equal(torch.sort(keys + col.to(torch.int64)).values, keys + ours.column_indices.to(torch.int64)), "patterns differ"
    del keys
    out = timed(call, reps, warm=1)
    L.rocsparse_destroy_mat_info(info); L.rocsparse_destroy_mat_descr(descr); L.rocsparse_destroy_handle(handle)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="grid,uniform,rmat,galerkin,balance")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--no-header", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gemm_bench needs a GPU"
    if not args.no_header:
        print(f"# gemm_bench: {torch.cuda.get_device_name(0)}, median of {args.reps} calls, each between its own events; "
              f"rocSPARSE = csrgemm_buffer_size + csrgemm_nnz + csrgemm, device pointer mode")
    for dtype, vb in ((torch.float32, 4), (torch.float64, 8)):
        if f"f{vb * 8}" not in args.dtypes.split(","):
            continue
        for key in args.cases.split(","):
            name, a, b = CASES[key](dtype)
            products = M.csr_gemm_products(a, b)
            op = M.CsrGemm(a, b, products=products)
            c = op.trimmed()
            longest = check(a, b, c, products)
            ms, spread = timed(op, args.reps)
            nc = c.column_indices.numel()
            line = (f"{name:52s} fp{vb * 8}  nnz {op.nnz_a} x {op.nnz_b}  products {products} -> {nc} (longest run {longest})  {ms:9.3f} ms  "
                    f"spread {spread:4.1f} %  {ms * 1e9 / max(products, 1):6.1f} ps/product  temp {op.temp.numel() / 1e9:5.2f} GB")
            if not args.no_rocsparse:
                rms, rspread = rocsparse_gemm(a, b, c, args.reps)
                line += f"  | rocSPARSE {rms:9.3f} ms  spread {rspread:4.1f} %  (pattern equal)  ours / rocSPARSE = {ms / rms:5.2f}"
            print(line, flush=True)
            del op, c, a, b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
