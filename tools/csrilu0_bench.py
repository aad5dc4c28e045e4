"""Times ILU(0) on the device (mspmv_csrilu0_*; merge_spmv_amd.csrilu0) against rocSPARSE's rocsparse_csrilu0 on the same arrays, the
analysis outside the timing:
python tools/csrilu0_bench.py [--reps 15] [--sweep 1,2,4,8,16,32,64] > profiles/csrilu0_bench.txt

Cases: a 5-point grid of 2000 x 2000 points and a 7-point grid of 128^3 points (the lattice plus its diagonal); A + A^T + I of an
R-MAT graph of scale 18 (16 edges per vertex).  Diagonal values in [1, 2), every other value in [-1, 1) divided by the row length
(diagonally dominant: finite factors).  Per case and precision: the analysis (wall clock around the synchronous LOWER
mspmv_csrsv_plan_create, median of 3); the factorisation OUT OF PLACE (the prologue's copy of the values included), median of --reps
calls, each between its own events after a warm-up, and the spread (max - min) / median.  Checked before it is timed: the leading
--sample rows of the factor bit for bit against the numpy model of tests/csrilu0_model.py (the first m rows of an ILU(0) depend on
the first m rows of A alone), and the pivot.  rocSPARSE (through ctypes, the library of tools/rocsparse_ref.py): buffer_size and
analysis (wall clock) outside the timing; rocsparse_csrilu0 works in place, so the values are copied back before every call, outside
its events; the patterns are the same arrays, the values are compared with ours (largest difference relative to the largest entry).
A row is worked by ONE group of G lanes however long it is.  Before a case runs, the longest chain of dependent steps one group has
to make is estimated from the pattern (lower entries x owned entries x bisection steps); a case above --max-steps is NOT run by us
(a kernel of minutes on a shared device) and the line says so: rocSPARSE alone is timed there.
--sweep: G over the given values on the two grids, fp64, through the development library (MSPMV_CSRILU0_GROUP)."""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import csrilu0_model as model
import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R
from tools.csrsv_bench import entry_rows, timed


def with_diagonal(A, symmetrize=False):
    """(row_offsets, column_indices) of A's pattern plus the diagonal (plus A^T's), columns ascending, no column twice"""
    n = A.rows
    r, c = entry_rows(A.row_offsets, n), A.column_indices.to(torch.int64)
    d = torch.arange(n, device="cuda", dtype=torch.int64)
    keys = [r * n + c, d * n + d] + ([c * n + r] if symmetrize else [])
    keys = torch.unique(torch.cat(keys))
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return off.to(torch.int32), (keys % n).to(torch.int32)


def case_grid():
    return ("5-point grid 2000 x 2000",) + with_diagonal(G.grid2d_csr(2000, dtype=torch.float32))


def case_grid3d():
    return ("7-point grid 128^3",) + with_diagonal(G.grid3d_csr(128, dtype=torch.float32))


def case_rmat(scale=18):
    return (f"A + A^T + I of an R-MAT graph of scale {scale}",) + with_diagonal(G.rmat_csr(scale, 16 << scale, dtype=torch.float32), True)


CASES = {"grid": case_grid, "grid3d": case_grid3d, "rmat": case_rmat, "rmat14": lambda: case_rmat(14), "rmat16": lambda: case_rmat(16)}


def values_for(off, col, dtype):
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    lens = torch.diff(off.to(torch.int64)).clamp_min(1)[r].to(dtype)
    v = G.uniform_pm1(21, col.numel(), dtype, "cuda")
    return torch.where(col.to(torch.int64) == r, 1.5 + 0.5 * v, v / lens)


def serial_steps(off, col, lanes):
    """an upper estimate of the dependent steps the busiest group makes: (lower entries) x ceil(row length / G) x bisection steps"""
    rows = off.numel() - 1
    lens = torch.diff(off.to(torch.int64))
    lower = torch.bincount(entry_rows(off, rows)[col.to(torch.int64) < entry_rows(off, rows)], minlength=rows)
    per = lower * ((lens + lanes - 1) // lanes)
    return int(per.max().item()) * max(1, math.ceil(math.log2(int(lens.max().item()) + 1)))


def analysis_ms(off, col, times=3):
    out, plan = [], None
    for _ in range(times):
        if plan is not None:
            plan.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = M.CsrSv(off, col, lower=True, unit_diagonal=True)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), plan


def check_sample(off, col, val, lu, pivot, sample):
    """the first `sample` rows of the factor bit for bit against the model; the pivot"""
    m = min(sample, off.numel() - 1)
    h_off = off[: m + 1].cpu().numpy()
    n = int(h_off[-1])
    want, _ = model.ilu0(h_off, col[:n].cpu().numpy(), val[:n].cpu().numpy())
    bits = np.int32 if want.dtype == np.float32 else np.int64
    assert np.array_equal(want.view(bits), lu[:n].cpu().numpy().view(bits)), "the factor differs from the model's bits"
    assert int(pivot.item()) == -1, f"pivot {int(pivot.item())}"
    return m, n


def rocsparse_csrilu0(off, col, val, ours, reps):
    """(analysis ms, median ms, spread %, max |lu - ours| / max |ours|) of rocsparse_csrilu0, in place on a copy of val"""
    L = R.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    rows, nnz = off.numel() - 1, col.numel()
    f64 = val.dtype == torch.float64
    size_fn, ana_fn, fn = ((L.rocsparse_dcsrilu0_buffer_size, L.rocsparse_dcsrilu0_analysis, L.rocsparse_dcsrilu0) if f64 else
                           (L.rocsparse_scsrilu0_buffer_size, L.rocsparse_scsrilu0_analysis, L.rocsparse_scsrilu0))
    p = lambda t: vp(t.data_ptr())
    work = val.clone()
    handle, descr, info = vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    assert L.rocsparse_create_mat_info(ctypes.byref(info)) == 0
    size = ctypes.c_size_t(0)
    st = size_fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, ctypes.byref(size))
    assert st == 0, f"rocsparse_csrilu0_buffer_size: {st}"
    buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = ana_fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, i32(1), i32(0), p(buf))
    torch.cuda.synchronize()
    ana = (time.perf_counter() - t0) * 1e3
    assert st == 0, f"rocsparse_csrilu0_analysis: {st}"
    times = []
    for i in range(1 + reps):
        work.copy_(val)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, i32(0), p(buf))
        e1.record()
        e1.synchronize()
        assert st == 0, f"rocsparse_csrilu0: {st}"
        if i >= 1:
            times.append(e0.elapsed_time(e1))
    diff = float("nan")
    if ours is not None:
        diff = ((work.to(torch.float64) - ours.to(torch.float64)).abs().max() / ours.to(torch.float64).abs().max()).item()
    L.rocsparse_destroy_mat_info(info); L.rocsparse_destroy_mat_descr(descr); L.rocsparse_destroy_handle(handle)
    med = statistics.median(times)
    return ana, med, (max(times) - min(times)) / med * 100, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="grid,grid3d,rmat")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--sample", type=int, default=3000, help="leading rows compared with the model's bits")
    ap.add_argument("--max-steps", type=int, default=3_000_000, help="a case whose busiest group would make more dependent steps is not run by us")
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--sweep", default="", help="comma-separated values of G tried on --sweep-cases through the development library")
    ap.add_argument("--sweep-cases", default="grid,grid3d")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "csrilu0_bench needs a GPU"
    print(f"# csrilu0_bench: {torch.cuda.get_device_name(0)}; analysis = wall clock of the synchronous call, median of 3; factorisation = median of "
          f"{args.reps} calls, each between its own events, out of place (ours: the copy included; rocSPARSE: in place, the copy back outside "
          f"its events); rocSPARSE = rocsparse_csrilu0, buffer_size + analysis outside the timing", flush=True)
    dts = {"f32": torch.float32, "f64": torch.float64}
    for case in args.cases.split(","):
        name, off, col = CASES[case]()
        rows, nnz = off.numel() - 1, col.numel()
        lanes = M.csrilu0_group(rows, nnz)
        steps = serial_steps(off, col, lanes)
        run_ours = steps <= args.max_steps
        print(f"{name}: rows {rows}  nnz {nnz}  longest row {int(torch.diff(off).max().item())}  G {lanes}  busiest group <= {steps} dependent steps"
              + ("" if run_ours else f"  > {args.max_steps}: NOT RUN by mspmv_csrilu0 (one group of {lanes} lanes per row; a wave per long row is not built)"),
              flush=True)
        plan = None
        if run_ours:
            ana, plan = analysis_ms(off, col)
            info = plan.info
            print(f"    levels {info['levels']}  launches 1 + {info['launches']}  largest level {info['max_level_rows']}  W {info['narrow_rows']}  "
                  f"analysis {ana:9.3f} ms", flush=True)
        for key in args.dtypes.split(","):
            val = values_for(off, col, dts[key])
            lu, line = None, f"    {key}"
            if run_ours:
                lu = torch.empty_like(val)
                ilu_temp = torch.empty(M._ilu0_temp_bytes(plan), dtype=torch.uint8, device="cuda")
                pivot = torch.empty(1, dtype=torch.int32, device="cuda")
                call = lambda: M._ilu0_call(plan, ilu_temp, val, lu, off, col, pivot, None, False)
                call()
                torch.cuda.synchronize()
                sample = args.sample if int(torch.diff(off[: args.sample + 1]).max().item()) < 64 else 16
                m, n = check_sample(off, col, val, lu, pivot, sample)
                ms, spread = timed(call, args.reps)
                line += f"  factorisation {ms:9.3f} ms  spread {spread:4.1f} %  (first {m} rows, {n} entries: the model's bits)"
            if not args.no_rocsparse:
                try:
                    r_ana, r_ms, r_spread, diff = rocsparse_csrilu0(off, col, val, lu, args.reps)
                    line += f"  | rocSPARSE analysis {r_ana:9.3f} ms  factorisation {r_ms:9.3f} ms  spread {r_spread:4.1f} %"
                    if run_ours:
                        line += f"  max |lu - ours| / max |ours| {diff:.1e}  rocSPARSE / ours = {r_ms / ms:6.2f}"
                except AssertionError as e:
                    line += f"  | rocSPARSE: {e}"
            print(line, flush=True)
        if plan is not None:
            plan.close()
        if run_ours and args.sweep and case in args.sweep_cases.split(","):
            prev = M.use_library("dev")
            val = values_for(off, col, torch.float64)
            lu = torch.empty_like(val)
            pivot = torch.empty(1, dtype=torch.int32, device="cuda")
            p = M.CsrSv(off, col, lower=True, unit_diagonal=True)
            ilu_temp = torch.empty(M._ilu0_temp_bytes(p), dtype=torch.uint8, device="cuda")
            for g in (int(v) for v in args.sweep.split(",")):
                os.environ["MSPMV_CSRILU0_GROUP"] = str(g)
                assert M.csrilu0_group(rows, nnz) == g
                ms, spread = timed(lambda: M._ilu0_call(p, ilu_temp, val, lu, off, col, pivot, None, False), args.reps)
                print(f"    sweep f64  G {g:3d}  factorisation {ms:9.3f} ms  spread {spread:4.1f} %", flush=True)
            del os.environ["MSPMV_CSRILU0_GROUP"]
            p.close()
            M.use_library(prev)
        del off, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
