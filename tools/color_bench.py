"""Times the multicolour ordering (mspmv_csr_color_*, mspmv_csr_permute_*; merge_spmv_amd.CsrColoring / csr_permute) and what it buys the
level-scheduled family, against rocSPARSE's rocsparse_csrcolor and against this library's own natural order in the same run:
python tools/color_bench.py [--reps 9] > profiles/color_bench.txt
One case per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/color_bench.py --cases grid > profiles/color_bench.txt && \\
timeout 600 python tools/color_bench.py --cases grid3d >> profiles/color_bench.txt && ...

Cases: those of tools/csrilu0_bench.py: a 5-point grid of 2000 x 2000 points and a 7-point grid of 128^3 points (the lattice plus its
diagonal); A + A^T + I of an R-MAT graph of scale 16 (16 edges per vertex).  Values, fp64: every off-diagonal entry -1, the diagonal
the row's length (symmetric and strictly diagonally dominant in any symmetric ordering: finite IC(0) and ILU(0) factors both ways).
Per case:
  colouring    wall clock around the synchronous constructor, median of 3; colours, rounds, the largest colour class; rocsparse_csrcolor
               on the same pattern (fraction 1.0; wall clock, median of 3) and ITS number of colours;
  permutation  P A P^T by csr_permute and mspmv_coo_to_csr_* on A's own triples (the same number of entries), median of --reps calls,
               each between its own events after a warm-up; the result is checked: every row sorted, the same multiset of values;
  pay-off      in natural and in multicolour order: the LOWER and UPPER mspmv_csrsv plans' levels and launches and the fp64 solve times;
               mspmv_csric0 (mirror = 1) and mspmv_csrilu0 out of place on the LOWER plan.  A case whose busiest group of lanes would make more
               than --max-steps dependent steps in a factorisation (the bound of tools/csrilu0_bench.py) is not factorised, in either order;
  pcg          (--pcg-cases) conjugate gradients on A preconditioned by Ic0.solve, to |r| <= --tol |b| by the recurrence, natural against
               multicolour order (b[order] in, x[inverse] out): iterations, wall clock, time per iteration, and the true residual of
               the mapped-back x in the original numbering.  The loop reads one norm back per iteration in both orders.
--sweep: the cap below which one workgroup finishes the colouring, over the given values, through the development library
(MSPMV_COLOR_CAP); the colours must not change.
For --pcg-cases grid the matrix is the 5-point Laplacian plus --shift times the identity (diagonal 4 + shift)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools import rocsparse_ref as R
from tools.csrilu0_bench import CASES, serial_steps
from tools.csrsv_bench import entry_rows, timed


def values_for(off, col, diagonal=None):
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    lens = torch.diff(off.to(torch.int64))[r].to(torch.float64)
    d = lens if diagonal is None else torch.full_like(lens, diagonal)
    return torch.where(col.to(torch.int64) == r, d, torch.full_like(lens, -1.0))


def wall_ms(fn, times=3):
    out, last = [], None
    for _ in range(times):
        if last is not None and hasattr(last, "close"):
            last.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), last


def rocsparse_csrcolor(off, col, val):
    """(median wall clock ms of 3, colours) of rocsparse_dcsrcolor, fraction_to_color = 1"""
    L = R.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    rows, nnz = off.numel() - 1, col.numel()
    p = lambda t: vp(t.data_ptr())
    handle, descr, info = vp(), vp(), vp()
    assert L.rocsparse_create_handle(ctypes.byref(handle)) == 0
    assert L.rocsparse_set_stream(handle, vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert L.rocsparse_create_mat_descr(ctypes.byref(descr)) == 0
    assert L.rocsparse_create_mat_info(ctypes.byref(info)) == 0
    coloring = torch.empty(rows, dtype=torch.int32, device="cuda")
    reordering = torch.empty(rows, dtype=torch.int32, device="cuda")
    fraction, ncolors = ctypes.c_double(1.0), ctypes.c_int(0)

    def call():
        st = L.rocsparse_dcsrcolor(handle, i32(rows), i32(nnz), descr, p(val), p(off), p(col), ctypes.byref(fraction), ctypes.byref(ncolors),
                                   p(coloring), p(reordering), info)
        assert st == 0, f"rocsparse_dcsrcolor: {st}"
    call()
    ms, _ = wall_ms(call)
    c = coloring.to(torch.int64)
    r = entry_rows(off, rows)
    proper = not bool(((c[r] == c[col.to(torch.int64)]) & (r != col.to(torch.int64))).any())
    L.rocsparse_destroy_mat_info(info); L.rocsparse_destroy_mat_descr(descr); L.rocsparse_destroy_handle(handle)
    return ms, int(ncolors.value), proper


def check_permuted(p, val, perm):
    rows = p.rows
    r = entry_rows(p.row_offsets, rows)
    key = r * rows + p.column_indices.to(torch.int64)
    assert bool((key[1:] > key[:-1]).all()), "the permuted matrix is not canonical"
    assert torch.equal(p.values, val[perm.to(torch.int64)]) and torch.equal(torch.sort(perm).values, torch.arange(perm.numel(), device="cuda", dtype=torch.int32))


def pay_off(label, off, col, val, reps, factorise):
    rows = off.numel() - 1
    b = G.uniform_pm1(23, rows, torch.float64, "cuda")
    line = f"    {label:11s}"
    plans = {}
    for name, lower in (("lower", True), ("upper", False)):
        plan = plans[name] = M.CsrSv(off, col, lower=lower, unit_diagonal=False)
        x = torch.empty_like(b)
        ms, spread = timed(lambda: plan.solve(val, b, x=x), reps)
        line += f"  csrsv {name} {plan.info['levels']:5d} levels {plan.info['launches']:5d} launches {ms:9.3f} ms ({spread:4.1f} %)"
    if factorise:
        plan = plans["lower"]
        out = torch.empty_like(val)
        pivot = torch.empty(1, dtype=torch.int32, device="cuda")
        temp = torch.empty(M._ic0_temp_bytes(plan), dtype=torch.uint8, device="cuda")
        ms, spread = timed(lambda: M._ic0_call(plan, temp, val, out, off, col, True, pivot, None, False), reps)
        assert int(pivot.item()) == -1
        line += f"  | csric0 {ms:9.3f} ms ({spread:4.1f} %)"
        temp = torch.empty(M._ilu0_temp_bytes(plan), dtype=torch.uint8, device="cuda")
        ms, spread = timed(lambda: M._ilu0_call(plan, temp, val, out, off, col, pivot, None, False), reps)
        assert int(pivot.item()) == -1
        line += f"  csrilu0 {ms:9.3f} ms ({spread:4.1f} %)"
    else:
        line += "  | csric0, csrilu0: NOT RUN (one group of lanes per row; the busiest would run for seconds)"
    print(line, flush=True)
    for plan in plans.values():
        plan.close()


def pcg(val, off, col, b, precondition, tol, limit):
    """the loop of tests/test_csric0.py; (x, iterations)"""
    n = b.numel()
    x = torch.zeros_like(b)
    r = b.clone()
    z = precondition(r).clone()
    p = z.clone()
    rz = torch.dot(r, z)
    stop = tol * float(torch.linalg.norm(b))
    for it in range(1, limit + 1):
        q = M.csrmv(val, off, col, p, num_cols=n)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            return x, it
        z = precondition(r)
        rz_new = torch.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, limit + 1


def pcg_both(off, col, val, coloring, p, tol, limit):
    rows = off.numel() - 1
    b = G.uniform_pm1(29, rows, torch.float64, "cuda")
    norm_b = float(torch.linalg.norm(b))
    for label, (o, c, v), rhs, back in (("natural", (off, col, val), b, lambda x: x),
                                        ("multicolour", (p.row_offsets, p.column_indices, p.values), coloring.permute_vector(b),
                                         lambda x: coloring.permute_vector(x, back=True))):
        ic = M.Ic0(o, c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert int(ic.factor(v).item()) == -1
        t_factor = (time.perf_counter() - t0) * 1e3
        pcg(v, o, c, rhs, ic.solve, tol, 2)                         # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, it = pcg(v, o, c, rhs, ic.solve, tol, limit)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        res = float(torch.linalg.norm(b - M.csrmv(val, off, col, back(x), num_cols=rows))) / norm_b
        print(f"    pcg {label:11s}  IC(0) factor {t_factor:9.3f} ms  {it:5d} iterations{' (NOT converged)' if it > limit else ''}  {total:10.3f} ms  "
              f"{total / max(it, 1):8.3f} ms per iteration  true |b - A x| / |b| {res:.2e}  "
              f"(lower {ic.lower.info['levels']} levels {ic.lower.info['launches']} launches, upper {ic.upper.info['launches']} launches)", flush=True)
        ic.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cases", default="grid,grid3d,rmat16")
    ap.add_argument("--pcg-cases", default="grid")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--shift", type=float, default=0.01, help="pcg on the grid: the diagonal is 4 + shift")
    ap.add_argument("--max-steps", type=int, default=3_000_000)
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--colouring-only", action="store_true", help="the colouring line (and the sweep) alone")
    ap.add_argument("--sweep", default="", help="comma-separated caps (uncoloured vertices one workgroup finishes) tried through the development library")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "color_bench needs a GPU"
    print(f"# color_bench: {torch.cuda.get_device_name(0)}; colouring = wall clock of the synchronous call, median of 3; permutation, solves and "
          f"factorisations = median of {args.reps} calls, each between its own events (spread = (max - min) / median); fp64", flush=True)
    for case in args.cases.split(","):
        name, off, col = CASES[case]()
        rows, nnz = off.numel() - 1, col.numel()
        val = values_for(off, col)
        print(f"{name}: rows {rows}  nnz {nnz}  longest row {int(torch.diff(off).max().item())}", flush=True)
        ms, coloring = wall_ms(lambda: M.CsrColoring(off, col))
        info = coloring.info
        c = coloring.colors.to(torch.int64)
        r = entry_rows(off, rows)
        assert not bool(((c[r] == c[col.to(torch.int64)]) & (r != col.to(torch.int64))).any()), "not a proper colouring"
        line = f"    colouring   {ms:9.3f} ms  {info['colors']} colours  {info['rounds']} rounds  largest class {info['max_color_rows']}  edges {info['edges']}"
        if not args.no_rocsparse:
            try:
                r_ms, r_colors, proper = rocsparse_csrcolor(off, col, val)
                line += f"  | rocsparse_csrcolor {r_ms:9.3f} ms  {r_colors} colours{'' if proper else ' (NOT proper)'}  rocSPARSE / ours = {r_ms / ms:5.2f}"
            except AssertionError as e:
                line += f"  | rocSPARSE: {e}"
        print(line, flush=True)
        if args.sweep:
            prev = M.use_library("dev")
            for cap in (int(v) for v in args.sweep.split(",")):
                os.environ["MSPMV_COLOR_CAP"] = str(cap)
                ms, swept = wall_ms(lambda: M.CsrColoring(off, col))
                assert torch.equal(swept.colors, coloring.colors)
                print(f"    sweep  cap {cap:7d}  colouring {ms:9.3f} ms  {swept.info['rounds']} rounds", flush=True)
                swept.close()
            del os.environ["MSPMV_COLOR_CAP"]
            M.use_library(prev)
        if args.colouring_only:
            coloring.close()
            continue
        p, perm = M.csr_permute(val, off, col, rows, row_perm=coloring.order, col_map=coloring.inverse, return_permutation=True)
        check_permuted(p, val, perm)
        ms_p, spread_p = timed(lambda: M.csr_permute(val, off, col, rows, row_perm=coloring.order, col_map=coloring.inverse, return_permutation=True), args.reps)
        r32 = r.to(torch.int32)
        ms_c, spread_c = timed(lambda: M.coo_to_csr(val, r32, col, rows, rows, return_permutation=True), args.reps)
        print(f"    permutation {ms_p:9.3f} ms ({spread_p:4.1f} %)  | mspmv_coo_to_csr on the same {nnz} entries {ms_c:9.3f} ms ({spread_c:4.1f} %)  "
              f"permutation / coo_to_csr = {ms_p / ms_c:5.2f}", flush=True)
        del r32, perm, c, r
        steps = serial_steps(off, col, M.csric0_group(rows, nnz))
        factorise = steps <= args.max_steps
        pay_off("natural", off, col, val, args.reps, factorise)
        pay_off("multicolour", p.row_offsets, p.column_indices, p.values, args.reps, factorise)
        if case in args.pcg_cases.split(","):
            diag = 4.0 + args.shift if case == "grid" else None
            val = values_for(off, col, diag)
            p = M.csr_permute(val, off, col, rows, row_perm=coloring.order, col_map=coloring.inverse)
            print(f"    pcg: {'the 5-point Laplacian + %g I' % args.shift if case == 'grid' else 'the values above'}, to |r| <= {args.tol:g} |b|, "
                  f"at most {args.limit} iterations", flush=True)
            pcg_both(off, col, val, coloring, p, args.tol, args.limit)
        coloring.close()
        del off, col, val, p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
