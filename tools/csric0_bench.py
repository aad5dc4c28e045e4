"""Times IC(0) on the device (mspmv_csric0_*; merge_spmv_amd.csric0) against rocSPARSE's rocsparse_csric0 and against this library's own
ILU(0) (mspmv_csrilu0_*) on the same arrays in the same run, the analysis outside the timing:
python tools/csric0_bench.py [--reps 15] [--sweep 1,2,4,8,16,32,64] > profiles/csric0_bench.txt
One case per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/csric0_bench.py --cases grid --sweep 1,2,4,8,16,32,64 > profiles/csric0_bench.txt && \\
timeout 600 python tools/csric0_bench.py --cases grid3d --sweep 1,2,4,8,16,32,64 >> profiles/csric0_bench.txt && ...

Cases: those of tools/csrilu0_bench.py: a 5-point grid of 2000 x 2000 points and a 7-point grid of 128^3 points (the lattice plus its
diagonal); A + A^T + I of an R-MAT graph (16 edges per vertex).  Diagonal values in [1, 2), every other value in [-1, 1) divided by
the longer of the two rows that meet at it (the symmetric matrix the lower triangle defines is diagonally dominant, and so is every
row of the stored one: finite factors for IC(0) and ILU(0) alike; the stored upper triangle holds other numbers than the lower one).
Per case and precision: the analysis (wall clock around the synchronous LOWER mspmv_csrsv_plan_create, median of 3); the
factorisation OUT OF PLACE (the prologue's copy of the values included) with mirror = 0 and with mirror = 1, median of --reps calls,
each between its own events after a warm-up, and the spread (max - min) / median; mspmv_csrilu0_* on the same plan and arrays, timed
the same way.  Checked before it is timed: the leading --sample rows of the factor (mirror = 0) bit for bit against the numpy model
of tests/csric0_model.py (the first m rows of an IC(0) depend on the lower triangle of the first m rows alone), and the pivot.
rocSPARSE (through ctypes, the library of tools/rocsparse_ref.py): buffer_size and analysis (wall clock) outside the timing;
rocsparse_csric0 works in place, so the values are copied back before every call, outside its events; the lower triangles are
compared with ours (largest difference relative to the largest entry).
A row is worked by ONE group of G lanes however long it is.  Before a case runs, the longest chain of dependent steps one group has
to make is estimated from the pattern: m * ceil((m + 1) / G) updates for a row of m lower entries, times the bisection steps; a case
above --max-steps (the bound of tools/csrilu0_bench.py) is NOT run by us (a kernel of minutes on a shared device) and the line says
so: rocSPARSE alone is timed there.
--sweep: G over the given values, fp64, mirror = 0, through the development library (MSPMV_CSRIC0_GROUP)."""
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

import csric0_model as model
import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R
from tools.csrilu0_bench import CASES, analysis_ms
from tools.csrsv_bench import entry_rows, timed


def values_for(off, col, dtype):
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    c = col.to(torch.int64)
    lens = torch.diff(off.to(torch.int64)).clamp_min(1)
    longer = torch.maximum(lens[r], lens[c]).to(dtype)
    v = G.uniform_pm1(21, col.numel(), dtype, "cuda")
    return torch.where(c == r, 1.5 + 0.5 * v, v / longer)


def serial_steps(off, col, lanes):
    """an upper estimate of the dependent steps the busiest group makes: m * ceil((m + 1) / G) for a row of m lower entries, times
    the bisection steps"""
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    lens = torch.diff(off.to(torch.int64))
    m = torch.bincount(r[col.to(torch.int64) < r], minlength=rows)
    per = m * ((m + 1 + lanes - 1) // lanes)
    return int(per.max().item()) * max(1, math.ceil(math.log2(int(lens.max().item()) + 1)))


def check_sample(off, col, val, l, pivot, sample):
    """the first `sample` rows of the factor (mirror = 0) bit for bit against the model; the pivot"""
    m = min(sample, off.numel() - 1)
    h_off = off[: m + 1].cpu().numpy()
    n = int(h_off[-1])
    want, _ = model.ic0(h_off, col[:n].cpu().numpy(), val[:n].cpu().numpy(), False)
    bits = np.int32 if want.dtype == np.float32 else np.int64
    assert np.array_equal(want.view(bits), l[:n].cpu().numpy().view(bits)), "the factor differs from the model's bits"
    assert int(pivot.item()) == -1, f"pivot {int(pivot.item())}"
    return m, n


def rocsparse_csric0(off, col, val, ours, reps):
    """(analysis ms, median ms, spread %, max |l - ours| / max |ours| over the lower triangle) of rocsparse_csric0, in place on a
    copy of val"""
    L = R.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    rows, nnz = off.numel() - 1, col.numel()
    f64 = val.dtype == torch.float64
    size_fn, ana_fn, fn = ((L.rocsparse_dcsric0_buffer_size, L.rocsparse_dcsric0_analysis, L.rocsparse_dcsric0) if f64 else
                           (L.rocsparse_scsric0_buffer_size, L.rocsparse_scsric0_analysis, L.rocsparse_scsric0))
    p = lambda t: vp(t.data_ptr())
    work = val.clone()
    handle, descr, info = vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    assert L.rocsparse_create_mat_info(ctypes.byref(info)) == 0
    size = ctypes.c_size_t(0)
    st = size_fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, ctypes.byref(size))
    assert st == 0, f"rocsparse_csric0_buffer_size: {st}"
    buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = ana_fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, i32(1), i32(0), p(buf))
    torch.cuda.synchronize()
    ana = (time.perf_counter() - t0) * 1e3
    assert st == 0, f"rocsparse_csric0_analysis: {st}"
    times = []
    for i in range(1 + reps):
        work.copy_(val)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = fn(handle, i32(rows), i32(nnz), descr, p(work), p(off), p(col), info, i32(0), p(buf))
        e1.record()
        e1.synchronize()
        assert st == 0, f"rocsparse_csric0: {st}"
        if i >= 1:
            times.append(e0.elapsed_time(e1))
    diff = float("nan")
    if ours is not None:
        low = col.to(torch.int64) <= entry_rows(off, rows)
        a, b = work[low].to(torch.float64), ours[low].to(torch.float64)
        diff = ((a - b).abs().max() / b.abs().max()).item()
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
    assert torch.cuda.is_available(), "csric0_bench needs a GPU"
    print(f"# csric0_bench: {torch.cuda.get_device_name(0)}; analysis = wall clock of the synchronous call, median of 3; factorisation = median of "
          f"{args.reps} calls, each between its own events, out of place (ours: the copy included; rocSPARSE: in place, the copy back outside "
          f"its events); rocSPARSE = rocsparse_csric0, buffer_size + analysis outside the timing; ILU(0) = mspmv_csrilu0 on the same plan and arrays",
          flush=True)
    dts = {"f32": torch.float32, "f64": torch.float64}
    for case in args.cases.split(","):
        name, off, col = CASES[case]()
        rows, nnz = off.numel() - 1, col.numel()
        lanes = M.csric0_group(rows, nnz)
        steps = serial_steps(off, col, lanes)
        run_ours = steps <= args.max_steps
        print(f"{name}: rows {rows}  nnz {nnz}  longest row {int(torch.diff(off).max().item())}  G {lanes} (ILU(0): {M.csrilu0_group(rows, nnz)})  "
              f"busiest group <= {steps} dependent steps"
              + ("" if run_ours else f"  > {args.max_steps}: NOT RUN by mspmv_csric0 (one group of {lanes} lanes per row; a wave per long row is not built)"),
              flush=True)
        plan = None
        if run_ours:
            ana, plan = analysis_ms(off, col)
            info = plan.info
            print(f"    levels {info['levels']}  launches 1 + {info['launches']} + mirror  largest level {info['max_level_rows']}  W {info['narrow_rows']}  "
                  f"analysis {ana:9.3f} ms", flush=True)
        for key in args.dtypes.split(","):
            val = values_for(off, col, dts[key])
            l, line = None, f"    {key}"
            if run_ours:
                l = torch.empty_like(val)
                temp = torch.empty(M._ic0_temp_bytes(plan), dtype=torch.uint8, device="cuda")
                pivot = torch.empty(1, dtype=torch.int32, device="cuda")
                call = lambda mirror=False: M._ic0_call(plan, temp, val, l, off, col, mirror, pivot, None, False)
                call()
                torch.cuda.synchronize()
                sample = args.sample if int(torch.diff(off[: args.sample + 1]).max().item()) < 64 else 16
                m, n = check_sample(off, col, val, l, pivot, sample)
                ms, spread = timed(call, args.reps)
                ms_m, spread_m = timed(lambda: call(True), args.reps)
                lu = torch.empty_like(val)
                ilu_temp = torch.empty(M._ilu0_temp_bytes(plan), dtype=torch.uint8, device="cuda")
                ms_ilu, spread_ilu = timed(lambda: M._ilu0_call(plan, ilu_temp, val, lu, off, col, pivot, None, False), args.reps)
                del lu
                call()
                torch.cuda.synchronize()
                line += (f"  factorisation {ms:9.3f} ms  spread {spread:4.1f} %  with the mirror {ms_m:9.3f} ms  spread {spread_m:4.1f} %  (first {m} rows, "
                         f"{n} entries: the model's bits)  | ILU(0) {ms_ilu:9.3f} ms  spread {spread_ilu:4.1f} %  ILU(0) / ours = {ms_ilu / ms:5.2f}")
            if not args.no_rocsparse:
                try:
                    r_ana, r_ms, r_spread, diff = rocsparse_csric0(off, col, val, l, args.reps)
                    line += f"  | rocSPARSE analysis {r_ana:9.3f} ms  factorisation {r_ms:9.3f} ms  spread {r_spread:4.1f} %"
                    if run_ours:
                        line += f"  max |l - ours| / max |ours| {diff:.1e}  rocSPARSE / ours = {r_ms / ms:6.2f}"
                except AssertionError as e:
                    line += f"  | rocSPARSE: {e}"
            print(line, flush=True)
        if plan is not None:
            plan.close()
        if run_ours and args.sweep and case in args.sweep_cases.split(","):
            prev = M.use_library("dev")
            val = values_for(off, col, torch.float64)
            l = torch.empty_like(val)
            pivot = torch.empty(1, dtype=torch.int32, device="cuda")
            p = M.CsrSv(off, col, lower=True, unit_diagonal=False)
            temp = torch.empty(M._ic0_temp_bytes(p), dtype=torch.uint8, device="cuda")
            for g in (int(v) for v in args.sweep.split(",")):
                os.environ["MSPMV_CSRIC0_GROUP"] = str(g)
                assert M.csric0_group(rows, nnz) == g
                ms, spread = timed(lambda: M._ic0_call(p, temp, val, l, off, col, False, pivot, None, False), args.reps)
                print(f"    sweep f64  G {g:3d}  factorisation {ms:9.3f} ms  spread {spread:4.1f} %", flush=True)
            del os.environ["MSPMV_CSRIC0_GROUP"]
            p.close()
            M.use_library(prev)
        del off, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
