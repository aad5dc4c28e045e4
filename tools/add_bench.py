"""Times C = alpha*A + beta*B on the device (mspmv_csr_add_*) against rocSPARSE's csrgeam_nnz + csrgeam on the same inputs:
python tools/add_bench.py [--reps 20] > profiles/add_bench.txt

Cases: a uniformly random 3.125 M x 3.125 M matrix of ~100 M entries plus its transpose (the symmetrisation), an R-MAT edge list
(scale 22, 64 M edges, duplicates merged) plus its transpose, a 5-point grid minus sigma I, one row of 2^26 entries plus a shifted
copy (the balance case), and the evenly spread case of the same entry count as the one-row case; fp32 and fp64.  Per case: the
median of --reps calls, each between its own events after a warm-up, the spread (max - min) / median, picoseconds per merged entry,
and the bytes of the model of DESIGN.md 4 "Addition" -- (8 + vb) n + (4 + vb) nnz_c + 20 rows, n = nnz_a + nnz_b: the column indices
and offsets are read by both passes -- over the time as a fraction of the HBM peak (8 TB/s).  The result of every case is checked
against torch (the sorted unique union of the two key lists) before it is timed.  rocSPARSE (through ctypes, tools/rocsparse_ref.py)
runs rocsparse_csrgeam_nnz + rocsparse_[sd]csrgeam per call in DEVICE pointer mode, so that neither side reads anything back on the
host; its row pointers and its first nnz_c column indices must equal ours before it is timed."""
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

PEAK = 8.0e12


def from_keys(keys, rows, cols, dtype, seed):
    """a canonical CSR from sorted unique int64 keys row * cols + col"""
    off = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // cols, minlength=rows), 0)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    vals = (torch.rand(keys.numel(), device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    return DeviceCsr(rows, cols, off.to(torch.int32), (keys % cols).to(torch.int32), vals)


def keys_of(m):
    r = torch.repeat_interleave(torch.arange(m.rows, device="cuda", dtype=torch.int64), torch.diff(m.row_offsets.to(torch.int64)))
    return r * m.cols + m.column_indices.to(torch.int64)


def transposed(a):
    vt, ot, ct, _ = M.csr_transpose(a.values, a.row_offsets, a.column_indices, a.cols)
    return DeviceCsr(a.cols, a.rows, ot, ct, vt)


def rmat(dtype, scale=22, edges=64_000_000, chunk=1 << 25):
    """the R-MAT edge list of the generators as a canonical CSR: built from the triples on the device, duplicates merged"""
    parts = [G.rmat_edges(scale, e0, min(e0 + chunk, edges), "cuda", G.SEED_C5) for e0 in range(0, edges, chunk)]
    r, c = (torch.cat([p[k] for p in parts]).to(torch.int32) for k in (0, 1))
    del parts
    g = torch.Generator(device="cuda"); g.manual_seed(6)
    v = (torch.rand(edges, device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    return M.coo_to_csr(v, r, c, 1 << scale, 1 << scale, sum_duplicates=True)


def cases(dtype, wanted):
    for key, make in (("uniform", case_uniform), ("rmat", case_rmat), ("grid", case_grid), ("spread", case_spread), ("onerow", case_onerow)):
        if key in wanted:
            yield make(dtype)


def case_rmat(dtype):
    a = rmat(dtype)
    return "R-MAT scale 22, 64 M edges merged + its transpose", a, transposed(a), 1.0, 1.0


def case_uniform(dtype):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n = 3_125_000
    a = from_keys(torch.unique(torch.randint(0, n * n, (100_000_000,), device="cuda", generator=g)), n, n, dtype, 2)
    return "uniform 3.125 M x 3.125 M + its transpose", a, transposed(a), 1.0, 1.0


def case_grid(dtype):
    k = 4000
    idx = torch.arange(k * k, device="cuda", dtype=torch.int64).view(k, k)
    pairs = [(idx, idx), (idx[1:], idx[:-1]), (idx[:-1], idx[1:]), (idx[:, 1:], idx[:, :-1]), (idx[:, :-1], idx[:, 1:])]
    keys = torch.sort(torch.cat([(r * (k * k) + c).reshape(-1) for r, c in pairs])).values
    grid = from_keys(keys, k * k, k * k, dtype, 3)
    eye = DeviceCsr(k * k, k * k, torch.arange(k * k + 1, device="cuda", dtype=torch.int32), torch.arange(k * k, device="cuda", dtype=torch.int32),
                    torch.ones(k * k, device="cuda", dtype=dtype))
    return "5-point grid 4000 x 4000 minus 0.5 I", grid, eye, 1.0, -0.5


def _row_keys():
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    m, cols = 1 << 26, 1 << 28
    return torch.unique(torch.randint(0, cols - 1, (m + (m >> 2),), device="cuda", generator=g))[:m].contiguous(), cols


def case_onerow(dtype):
    ka, cols = _row_keys()
    return "one row of 2^26 entries + the same shifted by one column", from_keys(ka, 1, cols, dtype, 4), from_keys(ka + 1, 1, cols, dtype, 5), 1.0, 1.0


def case_spread(dtype):
    ka, cols = _row_keys()
    rows = 1 << 21                                               # the same keys cut into 2^21 rows of 128 columns: 32 entries per row
    return ("the same 2^26 + 2^26 entries over 2^21 rows", from_keys(ka, rows, cols // rows, dtype, 4),
            from_keys(ka + 1, rows, cols // rows, dtype, 5), 1.0, 1.0)


def timed(fn, reps, warm=3):
    times = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times) * 100


def rocsparse_geam(a, b, alpha, beta, ours, count, reps):
    """(median ms, spread %) of csrgeam_nnz + csrgeam in device pointer mode, after its pattern was compared with ours"""
    L = R.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    f32 = a.values.dtype == torch.float32
    geam = L.rocsparse_scsrgeam if f32 else L.rocsparse_dcsrgeam
    handle, descr = vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_set_pointer_mode(handle, i32(1)) == 0     # rocsparse_pointer_mode_device
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    na, nb = a.column_indices.numel(), b.column_indices.numel()
    scal = torch.tensor([alpha, beta], dtype=a.values.dtype, device="cuda")
    off = torch.empty(a.rows + 1, dtype=torch.int32, device="cuda")
    col = torch.empty(na + nb, dtype=torch.int32, device="cuda")
    val = torch.empty(na + nb, dtype=a.values.dtype, device="cuda")
    nnz = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: vp(t.data_ptr())

    def call():
        st = L.rocsparse_csrgeam_nnz(handle, i32(a.rows), i32(a.cols), descr, i32(na), p(a.row_offsets), p(a.column_indices), descr, i32(nb),
                                     p(b.row_offsets), p(b.column_indices), descr, p(off), p(nnz))
        assert st == 0, st
        st = geam(handle, i32(a.rows), i32(a.cols), vp(scal.data_ptr()), descr, i32(na), p(a.values), p(a.row_offsets), p(a.column_indices),
                  vp(scal.data_ptr() + scal.element_size()), descr, i32(nb), p(b.values), p(b.row_offsets), p(b.column_indices), descr, p(val),
                  p(off), p(col))
        assert st == 0, st
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record()
    torch.cuda.synchronize()
    reps = min(reps, max(3, int(4000 / max(e0.elapsed_time(e1), 1e-3))))       # (a call of seconds is timed 3 times, not --reps)
    assert int(nnz.item()) == count and torch.equal(off, ours.row_offsets) and torch.equal(col[:count], ours.column_indices), "patterns differ"
    out = timed(call, reps, warm=1)
    L.rocsparse_destroy_mat_descr(descr); L.rocsparse_destroy_handle(handle)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="uniform,rmat,grid,onerow,spread")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--no-rocsparse", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "add_bench needs a GPU"
    print(f"# add_bench: {torch.cuda.get_device_name(0)}, median of {args.reps} calls, each between its own events; "
          f"rocSPARSE = csrgeam_nnz + csrgeam, device pointer mode")
    for dtype, vb in ((torch.float32, 4), (torch.float64, 8)):
        if f"f{vb * 8}" not in args.dtypes.split(","):
            continue
        for name, a, b, alpha, beta in cases(dtype, args.cases.split(",")):
            op = M.CsrAdd(a, b, alpha=alpha, beta=beta)
            torch.cuda.synchronize()
            c = op.trimmed()
            want = torch.unique(torch.cat([keys_of(a), keys_of(b)]))
            assert torch.equal(keys_of(c), want), name
            del want
            ms, spread = timed(op.add, args.reps)
            n, nc = op.nnz_a + op.nnz_b, c.column_indices.numel()
            model = (8 + vb) * n + (4 + vb) * nc + 20 * a.rows
            line = (f"{name:58s} fp{vb * 8}  nnz {op.nnz_a} + {op.nnz_b} -> {nc}  {ms:8.3f} ms  spread {spread:4.1f} %  "
                    f"{ms * 1e9 / n:6.1f} ps/entry  model {model / 1e9:6.2f} GB = {model / (ms * 1e-3) / PEAK * 100:4.1f} % of the HBM peak")
            if not args.no_rocsparse:
                rms, rspread = rocsparse_geam(a, b, alpha, beta, c, nc, args.reps)
                line += f"  | rocSPARSE {rms:8.3f} ms  spread {rspread:4.1f} %  (pattern equal)  ours / rocSPARSE = {ms / rms:5.2f}"
            print(line, flush=True)
            del op, c, a, b


if __name__ == "__main__":
    main()
