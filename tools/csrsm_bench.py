"""Times the level-scheduled triangular solve for k right-hand sides (mspmv_csrsm_*; merge_spmv_amd.CsrSv.solve_many) against what a
caller had before it -- k calls of mspmv_csrsv_solve_* -- and against rocSPARSE's rocsparse_spsm on the same arrays:
python tools/csrsm_bench.py [--reps 10] [--sweep 64,128,256,512,1024,4096] > profiles/csrsm_bench.txt

Cases (those of tools/csrsv_bench.py): the strict lower part plus the diagonal of a 5-point grid of 2000 x 2000 points; the
ILU(0)-shaped factor pattern (lower part plus diagonal) of a 3-D 7-point grid of 128^3 points; the strict lower triangle of an R-MAT
graph of scale 20 (16 edges per vertex) with a unit diagonal.  k = 1, 4, 16, 64 in fp32 and fp64; B and X rows x k row-major, ld = k.
Per case, precision and k, the median of --reps solves, each between its own events after a warm-up, and the spread (max - min) /
median:
  (a) one mspmv_csrsm_solve_*;
  (b) k mspmv_csrsv_solve_* on the columns of B copied out to k vectors (the copies are made outside the timing); a (b) whose single
      solve exceeds a second is timed 3 times, one above --skip-seconds is "not run";
  (c) rocsparse_spsm (default algorithm, row-major B and C), buffer_size and preprocess (its analysis) outside the timing, or
      "not run" with the reason.
The result is checked before it is timed: every column of (a) equals the x of (b) on the bits, and (c) is compared with (a).
--sweep: the lane budget (info.narrow_lanes) over a few values on the two grids at k = 4 and k = 16, fp64, through the development
library (MSPMV_CSRSM_NARROW_LANES)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R
from tools.csrsv_bench import CASES, timed, values_for

KS = (1, 4, 16, 64)


def raw(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def rocsparse_spsm(off, col, val, B, lower, unit, ours, reps):
    """(analysis ms, median solve ms, spread %, max |X - ours| / max |ours|) of rocsparse_spsm, default algorithm"""
    import time
    L = R.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    rows, nnz, k = off.numel() - 1, col.numel(), B.shape[1]
    dt = 152 if val.dtype == torch.float64 else 151
    alpha = (ctypes.c_double if val.dtype == torch.float64 else ctypes.c_float)(1.0)
    X = torch.zeros_like(B)
    p = lambda t: vp(t.data_ptr())
    handle, dA, dB, dX = vp(), vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    try:
        assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
        assert L.rocsparse_create_csr_descr(ctypes.byref(dA), i64(rows), i64(rows), i64(nnz), p(off), p(col), p(val), i32(2), i32(2), i32(0), i32(dt)) == 0
        fill, diag = i32(0 if lower else 1), i32(1 if unit else 0)
        assert L.rocsparse_spmat_set_attribute(dA, i32(0), ctypes.byref(fill), ctypes.c_size_t(4)) == 0
        assert L.rocsparse_spmat_set_attribute(dA, i32(1), ctypes.byref(diag), ctypes.c_size_t(4)) == 0
        for d, t in ((dB, B), (dX, X)):                                  # rows x k, ld = k, rocsparse_order_row
            assert L.rocsparse_create_dnmat_descr(ctypes.byref(d), i64(rows), i64(k), i64(k), p(t), i32(dt), i32(0)) == 0
        size = ctypes.c_size_t(0)
        head = (handle, i32(111), i32(111), ctypes.byref(alpha), dA, dB, dX, i32(dt), i32(0))
        st = L.rocsparse_spsm(*head, i32(1), ctypes.byref(size), None)
        assert st == 0, f"rocsparse_spsm buffer_size: status {st}"
        buf = torch.empty(max(size.value, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = L.rocsparse_spsm(*head, i32(2), ctypes.byref(size), p(buf))
        torch.cuda.synchronize()
        ana = (time.perf_counter() - t0) * 1e3
        assert st == 0, f"rocsparse_spsm preprocess: status {st}"

        def call():
            st = L.rocsparse_spsm(*head, i32(3), ctypes.byref(size), p(buf))
            assert st == 0, f"rocsparse_spsm compute: status {st}"
        call()
        torch.cuda.synchronize()
        diff = ((X.to(torch.float64) - ours.to(torch.float64)).abs().max() / ours.to(torch.float64).abs().max()).item()
        ms, spread = timed(call, reps, warm=1)
        return ana, ms, spread, diff
    finally:
        for d, destroy in ((dB, L.rocsparse_destroy_dnmat_descr), (dX, L.rocsparse_destroy_dnmat_descr), (dA, L.rocsparse_destroy_spmat_descr)):
            if d.value:
                destroy(d)
        L.rocsparse_destroy_handle(handle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="grid,grid3d,rmat_lower")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--skip-seconds", type=float, default=6.0, help="a column (b) whose k solves would take longer than this is not run")
    ap.add_argument("--sweep", default="", help="comma-separated lane budgets tried on --sweep-cases through the development library")
    ap.add_argument("--sweep-cases", default="grid,grid3d")
    ap.add_argument("--sweep-ks", default="4,16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "csrsm_bench needs a GPU"
    print(f"# csrsm_bench: {torch.cuda.get_device_name(0)}; solve = median of {args.reps} calls, each between its own events; alpha = 1; ld = k; "
          f"(a) one mspmv_csrsm_solve; (b) k mspmv_csrsv_solve on the columns copied out to vectors (copies outside the timing); "
          f"(c) rocsparse_spsm, default algorithm, row-major, buffer_size + preprocess outside the timing", flush=True)
    dts = {"f32": torch.float32, "f64": torch.float64}
    ks = [int(k) for k in args.ks.split(",") if k]
    for case in args.cases.split(","):
        name, off, col, lower, unit = CASES[case]()
        rows, nnz = off.numel() - 1, col.numel()
        plan = M.CsrSv(off, col, lower=lower, unit_diagonal=unit)
        info = plan.info
        print(f"{name}: rows {rows}  nnz {nnz}  levels {info['levels']}  largest level {info['max_level_rows']}  csrsv launches {info['launches']} "
              f"(W {info['narrow_rows']})", flush=True)
        for key in args.dtypes.split(","):
            val = values_for(off, col, dts[key])
            for k in ks:
                mi = plan.many_info(k)
                B = G.uniform_pm1(22, rows * k, dts[key], "cuda").view(rows, k)
                X = torch.empty_like(B)
                bs = [B[:, j].contiguous() for j in range(k)]
                xs = [torch.empty(rows, dtype=dts[key], device="cuda") for _ in range(k)]
                many = lambda: plan.solve_many(val, B, X=X)

                def each():
                    for j in range(k):
                        plan.solve(val, bs[j], x=xs[j])
                many()
                plan.solve(val, bs[0], x=xs[0])
                torch.cuda.synchronize()
                assert torch.equal(raw(X[:, 0]), raw(xs[0])), "csrsm column 0 differs from csrsv"
                ms, spread = timed(many, args.reps)
                one_ms, _ = timed(lambda: plan.solve(val, bs[0], x=xs[0]), 1, warm=1)
                line = (f"    {key}  k {k:3d}  P {mi['lanes_per_row']:2d}  passes {mi['passes']}  launches {mi['launches']:5d}  (a) csrsm {ms:10.3f} ms  "
                        f"spread {spread:4.1f} %")
                if one_ms * k > args.skip_seconds * 1e3:
                    line += f"  | (b) not run: {k} csrsv solves of {one_ms:.0f} ms each take {one_ms * k / 1e3:.1f} s a time"
                else:
                    each()
                    torch.cuda.synchronize()
                    assert all(torch.equal(raw(X[:, j]), raw(xs[j])) for j in range(k)), "a csrsm column differs from csrsv"
                    reps_b = args.reps if one_ms * k < 1e3 else 3
                    b_ms, b_spread = timed(each, reps_b, warm=1)
                    line += f"  | (b) {k:3d} x csrsv {b_ms:10.3f} ms  spread {b_spread:4.1f} % ({reps_b} solves)  (b) / (a) = {b_ms / ms:6.2f}"
                if args.no_rocsparse:
                    line += "  | (c) rocsparse_spsm not run: --no-rocsparse"
                else:
                    try:
                        r_ana, r_ms, r_spread, diff = rocsparse_spsm(off, col, val, B, lower, unit, X, args.reps)
                        line += (f"  | (c) rocsparse_spsm analysis {r_ana:9.3f} ms  solve {r_ms:10.3f} ms  spread {r_spread:4.1f} %  "
                                 f"max |X - ours| / max |ours| {diff:.1e}  (c) / (a) = {r_ms / ms:6.2f}")
                    except (AssertionError, AttributeError, OSError) as e:
                        line += f"  | (c) rocsparse_spsm not run: {e}"
                print(line, flush=True)
                del B, X, bs, xs
        plan.close()
        if args.sweep and case in args.sweep_cases.split(","):
            prev = M.use_library("dev")
            p = M.CsrSv(off, col, lower=lower, unit_diagonal=unit)
            val = values_for(off, col, torch.float64)
            for k in (int(v) for v in args.sweep_ks.split(",")):
                B = G.uniform_pm1(22, rows * k, torch.float64, "cuda").view(rows, k)
                X = torch.empty_like(B)
                for w in (int(v) for v in args.sweep.split(",")):
                    os.environ["MSPMV_CSRSM_NARROW_LANES"] = str(w)
                    mi = p.many_info(k)
                    assert mi["narrow_lanes"] == w
                    ms, spread = timed(lambda: p.solve_many(val, B, X=X), args.reps)
                    print(f"    sweep f64  k {k:3d}  narrow_lanes {w:6d}  launches {mi['launches']:5d}  solve {ms:10.3f} ms  spread {spread:4.1f} %", flush=True)
                del os.environ["MSPMV_CSRSM_NARROW_LANES"]
            p.close()
            M.use_library(prev)
        del off, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
