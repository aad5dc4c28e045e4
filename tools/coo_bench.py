"""tools/coo_bench.py -- the device COO -> CSR build against its yardsticks (profiles/coo_bench.txt).

Per input (uniformly shuffled triples): mspmv_coo_to_csr_* (values and permutation), the stateless mspmv_coomv_*,
mspmv_csr_sum_duplicates_* on the built CSR, and the yardsticks, none of which is the code under test: (a) the torch route
generators.rmat_csr uses (stable sort of the 64-bit key, bincount, cumsum, gathers) on the same triples, (b) mspmv_csr_transpose_*
on the built matrix (half as many passes of the same kernels), (c) rocSPARSE's coosort_by_row + coo2csr + gthr.  Every call is
timed on its own between two events on the stream after warm-up; the table gives the median and the spread (min .. max) of
`--reps` calls.  The bytes the build moves are computed from the shapes and set against 8 TB/s.  Development / reporting aid.

    python tools/coo_bench.py [--only c2_f32,rmat22,small] [--reps 15]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import merge_spmv_amd as M                                  # noqa: E402
from merge_spmv_amd import generators as G                  # noqa: E402
from tools import rocsparse_ref as R                        # noqa: E402

vp, i32 = ctypes.c_void_p, ctypes.c_int


def timed(fn, reps, warm=2, before=None):
    """[median, min, max] ms of `reps` calls, each between its own pair of events; `before` (untimed) runs ahead of every call"""
    times = []
    for k in range(warm + reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def passes_of(n):
    return -(-max(n - 1, 0).bit_length() // 8) if n > 1 else 0


def build_bytes(rows, cols, nnz, vb):
    """(the least a build can move: read the triples, write the CSR and the permutation; what this one moves: every pass reads its
    keys for the histogram, reads and writes one item -- the first reads no position --, the last kernel reads the rows and writes the offsets)"""
    least = nnz * (8 + vb) + nnz * (8 + vb) + 4 * (rows + 1)
    passes = max(1, passes_of(cols) + passes_of(rows))
    item = 12 + vb
    moved = passes * 4 * nnz + (2 * passes * item - 4) * nnz + 4 * nnz + 4 * (rows + 1)
    return least, moved, passes


def torch_route(r, c, v, rows, cols):
    key = r.to(torch.int64) * cols + c.to(torch.int64)
    order = torch.sort(key, stable=True).indices
    lens = torch.bincount(r.to(torch.int64), minlength=rows)
    off = torch.zeros(rows + 1, dtype=torch.int64, device=r.device)
    torch.cumsum(lens, 0, out=off[1:])
    return off.to(torch.int32), c[order], v[order]


def rocsparse_build(r, c, v, rows, cols, reps):
    L = R.lib()
    for name in ("rocsparse_coosort_buffer_size", "rocsparse_coosort_by_row", "rocsparse_coo2csr", "rocsparse_create_identity_permutation"):
        if not hasattr(L, name):
            return None
    handle = vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    nnz = r.numel()
    size = ctypes.c_size_t(0)
    assert L.rocsparse_coosort_buffer_size(handle, i32(rows), i32(cols), i32(nnz), vp(r.data_ptr()), vp(c.data_ptr()), ctypes.byref(size)) == 0
    buf = torch.empty(max(size.value, 1), dtype=torch.uint8, device="cuda")
    rr, cc, perm = torch.empty_like(r), torch.empty_like(c), torch.empty_like(r)
    off, val = torch.empty(rows + 1, dtype=torch.int32, device="cuda"), torch.empty_like(v)
    gthr = L.rocsparse_sgthr if v.dtype == torch.float32 else L.rocsparse_dgthr

    def call():
        assert L.rocsparse_create_identity_permutation(handle, i32(nnz), vp(perm.data_ptr())) == 0
        assert L.rocsparse_coosort_by_row(handle, i32(rows), i32(cols), i32(nnz), vp(rr.data_ptr()), vp(cc.data_ptr()), vp(perm.data_ptr()),
                                          vp(buf.data_ptr())) == 0
        assert L.rocsparse_coo2csr(handle, vp(rr.data_ptr()), i32(nnz), i32(rows), vp(off.data_ptr()), i32(0)) == 0
        assert gthr(handle, i32(nnz), vp(v.data_ptr()), vp(val.data_ptr()), vp(perm.data_ptr()), i32(0)) == 0
    ms = timed(call, reps, before=lambda: (rr.copy_(r), cc.copy_(c)))          # (it sorts in place: the copies are not timed)
    L.rocsparse_destroy_handle(handle)
    return ms


def run(label, rows, cols, r, c, v, reps):
    lib = M.load_library()
    vb, nnz, dev = v.element_size(), r.numel(), r.device
    sfx = "f32" if vb == 4 else "f64"
    out = {"input": label, "rows": rows, "cols": cols, "nnz": nnz, "dtype": sfx}
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    off = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    col, perm, val = torch.empty_like(c), torch.empty_like(c), torch.empty_like(v)
    fn = getattr(lib, "mspmv_coo_to_csr_" + sfx)
    args = (p(v), p(r), p(c), rows, cols, nnz, p(off), p(col), p(val), p(perm))
    size = ctypes.c_size_t(0)
    assert fn(None, ctypes.byref(size), *args, None, 0) == 0
    temp = torch.empty(size.value, dtype=torch.uint8, device=dev)
    out["coo_to_csr_ms"] = timed(lambda: fn(p(temp), ctypes.byref(size), *args, stream, 0), reps)
    least, moved, passes = build_bytes(rows, cols, nnz, vb)
    out.update(passes=passes, temp_bytes=int(size.value), bytes_least=least, bytes_moved=moved, ms_at_8tbs_least=round(least / 8e9, 4),
               ms_at_8tbs_moved=round(moved / 8e9, 4), moved_gbs=round(moved / out["coo_to_csr_ms"][0] / 1e6, 1))
    del temp
    # yardstick (a): the torch route on the same triples; it also checks the build (a stable sort of the same key)
    out["torch_route_ms"] = timed(lambda: torch_route(r, c, v, rows, cols), max(3, reps // 3))
    toff, tcol, tval = torch_route(r, c, v, rows, cols)
    out["same_as_torch_route"] = bool(torch.equal(toff, off) and torch.equal(tcol, col) and torch.equal(tval, val))
    del toff, tcol, tval
    # yardstick (b): the transpose of the built matrix (its column passes alone)
    tfn = getattr(lib, "mspmv_csr_transpose_" + sfx)
    off_t = torch.empty(cols + 1, dtype=torch.int32, device=dev)
    col_t, perm_t, val_t = torch.empty_like(c), torch.empty_like(c), torch.empty_like(v)
    targs = (p(val), p(off), p(col), rows, cols, nnz, p(val_t), p(off_t), p(col_t), p(perm_t))
    tsize = ctypes.c_size_t(0)
    assert tfn(None, ctypes.byref(tsize), *targs, None, 0) == 0
    ttemp = torch.empty(tsize.value, dtype=torch.uint8, device=dev)
    out["transpose_ms"] = timed(lambda: tfn(p(ttemp), ctypes.byref(tsize), *targs, stream, 0), reps)
    out["transpose_passes"] = max(1, passes_of(cols))
    del ttemp, off_t, col_t, perm_t, val_t
    # duplicates
    dfn = getattr(lib, "mspmv_csr_sum_duplicates_" + sfx)
    off2 = torch.empty_like(off); col2 = torch.empty_like(col); val2 = torch.empty_like(val)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    dargs = (p(val), p(off), p(col), rows, cols, nnz, p(val2), p(off2), p(col2), p(count))
    dsize = ctypes.c_size_t(0)
    assert dfn(None, ctypes.byref(dsize), *dargs, None, 0) == 0
    dtemp = torch.empty(dsize.value, dtype=torch.uint8, device=dev)
    out["sum_duplicates_ms"] = timed(lambda: dfn(p(dtemp), ctypes.byref(dsize), *dargs, stream, 0), reps)
    out["entries_after_merging"] = int(count.item())
    del dtemp, off2, col2, val2
    # the stateless COO SpMV, and the forward call on the built matrix for scale
    x = G.uniform_pm1(12345, cols, v.dtype, "cuda")
    y = torch.empty(rows, dtype=v.dtype, device=dev)
    ws = M.CsrMVWorkspace(rows, nnz, v.dtype)
    out["csrmv_on_built_ms"] = timed(lambda: M.csrmv(val, off, col, x, y, num_cols=cols, workspace=ws), reps)
    mfn = getattr(lib, "mspmv_coomv_" + sfx)
    ct = ctypes.c_float if vb == 4 else ctypes.c_double
    margs = (p(v), p(r), p(c), p(x), p(y), rows, cols, nnz, ct(1.0), ct(0.0))
    msize = ctypes.c_size_t(0)
    assert mfn(None, ctypes.byref(msize), *margs, None, 0) == 0
    mtemp = torch.empty(msize.value, dtype=torch.uint8, device=dev)
    out["coomv_ms"] = timed(lambda: mfn(p(mtemp), ctypes.byref(msize), *margs, stream, 0), reps)
    del mtemp
    # yardstick (c)
    try:
        ms = rocsparse_build(r, c, v, rows, cols, max(3, reps // 3))
        out["rocsparse_coosort_coo2csr_gthr_ms"] = ms if ms is not None else "not reachable"
    except (OSError, AttributeError, AssertionError) as e:
        out["rocsparse_coosort_coo2csr_gthr_ms"] = f"not reachable ({type(e).__name__})"
    print(json.dumps(out), flush=True)
    return out


def triples_of(A, seed):
    lens = (A.row_offsets[1:] - A.row_offsets[:-1]).to(torch.int64)
    r = torch.repeat_interleave(torch.arange(A.rows, dtype=torch.int32, device="cuda"), lens)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    sh = torch.randperm(A.nnz, device="cuda", generator=g)
    return r[sh].contiguous(), A.column_indices[sh].contiguous(), A.values[sh].contiguous()


def inputs(name):
    if name in ("c2_f32", "c2_f64"):
        A = G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float32 if name == "c2_f32" else torch.float64)
        return (A.rows, A.cols) + triples_of(A, 1)
    if name == "rmat22":                                         # the Orkut-sized edge list, in edge order (R-MAT edges arrive unsorted)
        n = 1 << G.C3_ORKUT_SCALE
        rs, cs = [], []
        for e0 in range(0, G.C3_ORKUT_EDGES, 1 << 25):
            r, c = G.rmat_edges(G.C3_ORKUT_SCALE, e0, min(e0 + (1 << 25), G.C3_ORKUT_EDGES), "cuda", G.SEED_C3)
            rs.append(r.to(torch.int32)); cs.append(c.to(torch.int32))
        r, c = torch.cat(rs), torch.cat(cs)
        return n, n, r, c, G.uniform_pm1(777, r.numel(), torch.float32, "cuda")
    if name == "small":
        A = G.uniform_csr(10_000, 10_000, 10, dtype=torch.float32)
        return (A.rows, A.cols) + triples_of(A, 2)
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c2_f32,c2_f64,rmat22,small")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    for name in a.only.split(","):
        rows, cols, r, c, v = inputs(name)
        run(name, rows, cols, r, c, v, a.reps)
        del r, c, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
