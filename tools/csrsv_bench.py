"""Times the level-scheduled triangular solve (mspmv_csrsv_*; merge_spmv_amd.CsrSv) against rocSPARSE's rocsparse_spsv on the same
arrays, analysis and solve separately:
python tools/csrsv_bench.py [--reps 10] > profiles/csrsv_bench.txt

Cases: the strict lower part plus the diagonal of a 5-point grid of 2000 x 2000 points; the ILU(0)-shaped factor pattern (lower part
plus diagonal) of a 3-D 7-point grid of 128^3 points; the strict lower and the strict upper triangle of an R-MAT graph of scale 20
(16 edges per vertex) with a unit diagonal; a bidiagonal chain of 2^16 rows.  The grids and the chain have mirror-image upper
triangles with the same levels, so only the lower one is timed.  Diagonal values in [1, 2), every other value in [-1, 1) divided by
the row length.  Per case: the levels, launches and largest level of the plan; the analysis (wall clock around the synchronous
mspmv_csrsv_plan_create, median of 3); the solve (median of --reps calls, each between its own events after a warm-up, and the
spread (max - min) / median).  The result is checked before it is timed: the residual |T x - b| through M.csrmv on the same
triangle, elementwise within (len + 1) * eps * (|T||x| + |b|).  rocSPARSE (through ctypes, the library of tools/rocsparse_ref.py)
runs rocsparse_spsv with its default algorithm; buffer_size and preprocess (its analysis, timed by wall clock) run outside the
solve timing; its x is compared with ours.
--sweep: W (info.narrow_rows) over a few values on the two grids, through the development library (MSPMV_CSRSV_NARROW_ROWS)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R


def entry_rows(off, rows):
    return torch.repeat_interleave(torch.arange(rows, device="cuda", dtype=torch.int64), torch.diff(off.to(torch.int64)))


def triangle(A, lower, diagonal):
    """(row_offsets, column_indices) of A's strict triangle, columns ascending, with the diagonal added when asked"""
    n = A.rows
    r, c = entry_rows(A.row_offsets, n), A.column_indices.to(torch.int64)
    keep = (c < r) if lower else (c > r)
    keys = r[keep] * n + c[keep]
    if diagonal:
        d = torch.arange(n, device="cuda", dtype=torch.int64)
        keys = torch.cat([keys, d * n + d])
    keys = torch.sort(keys).values
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return off.to(torch.int32), (keys % n).to(torch.int32)


def case_grid():
    off, col = triangle(G.grid2d_csr(2000, dtype=torch.float32), True, True)
    return "5-point grid 2000 x 2000, lower + diagonal", off, col, True, False


def case_grid3d():
    off, col = triangle(G.grid3d_csr(128, dtype=torch.float32), True, True)
    return "ILU(0) pattern of a 7-point grid 128^3, lower", off, col, True, False


def case_rmat_lower():
    off, col = triangle(G.rmat_csr(20, 16 << 20, dtype=torch.float32), True, False)
    return "R-MAT scale 20, strict lower, unit diagonal", off, col, True, True


def case_rmat_upper():
    off, col = triangle(G.rmat_csr(20, 16 << 20, dtype=torch.float32), False, False)
    return "R-MAT scale 20, strict upper, unit diagonal", off, col, False, True


def case_chain():
    n = 1 << 16
    r = torch.arange(n, device="cuda", dtype=torch.int64)
    keys = torch.sort(torch.cat([r * n + r, r[1:] * n + r[:-1]])).values
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return "bidiagonal chain of 2^16 rows", off.to(torch.int32), (keys % n).to(torch.int32), True, False


CASES = {"grid": case_grid, "grid3d": case_grid3d, "rmat_lower": case_rmat_lower, "rmat_upper": case_rmat_upper, "chain": case_chain}


def values_for(off, col, dtype):
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    lens = torch.diff(off.to(torch.int64)).clamp_min(1)[r].to(dtype)
    v = G.uniform_pm1(21, col.numel(), dtype, "cuda")
    return torch.where(col.to(torch.int64) == r, 1.5 + 0.5 * v, v / lens)


def check(off, col, val, b, x, unit, what):
    """|T x - b| <= (len + 1) eps (|T||x| + |b|) elementwise, T x through M.csrmv (plus x for a unit diagonal)"""
    rows = off.numel() - 1
    y = M.csrmv(val, off, col, x, num_cols=rows).to(torch.float64)
    mag = M.csrmv(val.abs(), off, col, x.abs(), num_cols=rows).to(torch.float64)
    if unit:
        y, mag = y + x.to(torch.float64), mag + x.abs().to(torch.float64)
    eps = 2.0 ** -52 if x.dtype == torch.float64 else 2.0 ** -23
    lens = torch.diff(off.to(torch.int64)).to(torch.float64) + (2 if unit else 1)
    bound = lens * eps * (mag + b.abs().to(torch.float64))
    ratio = ((y - b.to(torch.float64)).abs() / bound.clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, f"{what}: the residual is {ratio:.2f} of its bound"
    return ratio


def timed(fn, reps, warm=2):
    times = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if i >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times) * 100


def analysis_ms(off, col, lower, unit, times=3):
    out, plan = [], None
    for _ in range(times):
        if plan is not None:
            plan.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = M.CsrSv(off, col, lower=lower, unit_diagonal=unit)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), plan


def rocsparse_spsv(off, col, val, b, lower, unit, ours, reps):
    """(analysis ms, median solve ms, spread %, max |x - ours| / max |ours|) of rocsparse_spsv, default algorithm"""
    L = R.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    rows, nnz = off.numel() - 1, col.numel()
    dt = 152 if val.dtype == torch.float64 else 151
    ct = ctypes.c_double if val.dtype == torch.float64 else ctypes.c_float
    alpha = ct(1.0)
    x = torch.zeros_like(b)
    p = lambda t: vp(t.data_ptr())
    handle, dA, dB, dX = vp(), vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_create_csr_descr(ctypes.byref(dA), i64(rows), i64(rows), i64(nnz), p(off), p(col), p(val), i32(2), i32(2), i32(0), i32(dt)) == 0
    fill, diag = i32(0 if lower else 1), i32(1 if unit else 0)
    assert L.rocsparse_spmat_set_attribute(dA, i32(0), ctypes.byref(fill), ctypes.c_size_t(4)) == 0
    assert L.rocsparse_spmat_set_attribute(dA, i32(1), ctypes.byref(diag), ctypes.c_size_t(4)) == 0
    assert L.rocsparse_create_dnvec_descr(ctypes.byref(dB), i64(rows), p(b), i32(dt)) == 0
    assert L.rocsparse_create_dnvec_descr(ctypes.byref(dX), i64(rows), p(x), i32(dt)) == 0
    size = ctypes.c_size_t(0)
    head = (handle, i32(111), ctypes.byref(alpha), dA, dB, dX, i32(dt), i32(0))
    st = L.rocsparse_spsv(*head, i32(1), ctypes.byref(size), None)
    assert st == 0, f"rocsparse_spsv buffer_size: {st}"
    buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = L.rocsparse_spsv(*head, i32(2), ctypes.byref(size), p(buf))
    torch.cuda.synchronize()
    ana = (time.perf_counter() - t0) * 1e3
    assert st == 0, f"rocsparse_spsv preprocess: {st}"

    def call():
        st = L.rocsparse_spsv(*head, i32(3), ctypes.byref(size), p(buf))
        assert st == 0, f"rocsparse_spsv compute: {st}"
    call()
    torch.cuda.synchronize()
    diff = ((x.to(torch.float64) - ours.to(torch.float64)).abs().max() / ours.to(torch.float64).abs().max()).item()
    ms, spread = timed(call, reps, warm=1)
    L.rocsparse_destroy_dnvec_descr(dB); L.rocsparse_destroy_dnvec_descr(dX); L.rocsparse_destroy_spmat_descr(dA); L.rocsparse_destroy_handle(handle)
    return ana, ms, spread, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="grid,grid3d,rmat_lower,rmat_upper,chain")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--sweep", default="", help="comma-separated values of W tried on --sweep-cases through the development library")
    ap.add_argument("--sweep-cases", default="grid,grid3d")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "csrsv_bench needs a GPU"
    print(f"# csrsv_bench: {torch.cuda.get_device_name(0)}; analysis = wall clock of the synchronous call, median of 3; solve = median of "
          f"{args.reps} calls, each between its own events; alpha = 1; rocSPARSE = rocsparse_spsv, default algorithm, buffer_size + preprocess "
          f"outside the solve timing", flush=True)
    dts = {"f32": torch.float32, "f64": torch.float64}
    for case in args.cases.split(","):
        name, off, col, lower, unit = CASES[case]()
        rows, nnz = off.numel() - 1, col.numel()
        ana, plan = analysis_ms(off, col, lower, unit)
        info = plan.info
        print(f"{name}: rows {rows}  nnz {nnz}  levels {info['levels']}  launches {info['launches']}  largest level {info['max_level_rows']}  "
              f"W {info['narrow_rows']}  plan {info['device_bytes']} bytes  analysis {ana:9.3f} ms", flush=True)
        for key in args.dtypes.split(","):
            val = values_for(off, col, dts[key])
            b = G.uniform_pm1(22, rows, dts[key], "cuda")
            x = torch.empty_like(b)
            call = lambda: plan.solve(val, b, x=x)
            call()
            torch.cuda.synchronize()
            worst = check(off, col, val, b, x, unit, "mspmv_csrsv")
            ms, spread = timed(call, args.reps)
            line = f"    {key}  solve {ms:9.3f} ms  spread {spread:4.1f} %  (residual {worst:4.2f} of its bound)"
            if not args.no_rocsparse:
                try:
                    r_ana, r_ms, r_spread, diff = rocsparse_spsv(off, col, val, b, lower, unit, x, args.reps)
                    line += (f"  | rocSPARSE analysis {r_ana:9.3f} ms  solve {r_ms:9.3f} ms  spread {r_spread:4.1f} %  max |x - ours| / max |ours| {diff:.1e}  "
                             f"rocSPARSE / ours = {r_ms / ms:6.2f}")
                except AssertionError as e:
                    line += f"  | rocSPARSE: {e}"
            print(line, flush=True)
        plan.close()
        if args.sweep and case in args.sweep_cases.split(","):
            prev = M.use_library("dev")
            val = values_for(off, col, torch.float64)
            b = G.uniform_pm1(22, rows, torch.float64, "cuda")
            x = torch.empty_like(b)
            for w in (int(v) for v in args.sweep.split(",")):
                os.environ["MSPMV_CSRSV_NARROW_ROWS"] = str(w)
                p = M.CsrSv(off, col, lower=lower, unit_diagonal=unit)
                assert p.info["narrow_rows"] == w
                ms, spread = timed(lambda: p.solve(val, b, x=x), args.reps)
                print(f"    sweep f64  W {w:6d}  launches {p.info['launches']:5d}  solve {ms:9.3f} ms  spread {spread:4.1f} %", flush=True)
                p.close()
            del os.environ["MSPMV_CSRSV_NARROW_ROWS"]
            M.use_library(prev)
        del off, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
