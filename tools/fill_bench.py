"""Times the level-of-fill pattern (mspmv_csr_fill_*; merge_spmv_amd.CsrFill) and what a stronger factor buys the solvers:
python tools/fill_bench.py [--reps 3] > profiles/fill_bench.txt
One case and one order per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/fill_bench.py --cases grid --orders multicolour > profiles/fill_bench.txt && timeout 900 python tools/fill_bench.py
--cases grid --orders natural >> ... && ... --cases grid3d ... && timeout 60 python tools/fill_bench.py --cases limit >> ...

Cases, fp64 (the matrices of tools/pcg_bench.py and tools/bicgstab_bench.py):
  grid     the 5-point stencil on 2000 x 2000 points; CG: the Laplacian + 0.01 I; BiCGStab: convection-diffusion, wind 0.5, shift 0.01
  grid3d   the 7-point stencil on 128^3 points; CG: the diagonal is the row's length; BiCGStab: wind 0.5, no shift
in natural order and in multicolour order (CsrColoring, csr_permute; the fill is then that of P A P^T), at fill levels 0, 1 and 2:
  symbolic    CsrFill(...): the wall clock of the whole analysis, the median (least .. most) of 2 x --reps, and as a multiple of ONE csrilu0 of the same
              matrix at level 0
  values      CsrFill.values: one launch between its own events
  plans       the levels and launches of the LOWER and UPPER plans on the filled pattern
  csric0 / csrilu0   one factorisation of the filled values between its own events
  sweeps      one pair (Ick.solve / Iluk.solve) between its own events
  Pcg / Bicgstab     to rr <= (tol |b|)^2: the iterations (found with check_every = 8), then the check_every = 0 solve of exactly those
              iterations, the median wall clock of --reps runs ending in a synchronisation: iterations x time per iteration = total.
  limit       the case of a fill beyond 2^31 - 65537: how long the refusal from the counts takes
x of every solve is checked: the true residual |b - A x| / |b| in the original numbering."""
import argparse
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
from tools.bicgstab_bench import values_for as convection_values
from tools.color_bench import values_for as laplacian_values
from tools.csrilu0_bench import CASES
from tools.csrsv_bench import timed
from tools.pcg_bench import wall

LEVELS = (0, 1, 2)


def symbolic_ms(off, col, level, reps):
    times, info = [], None
    for _ in range(2 * reps + 1):                                    # (the first run is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fill = M.CsrFill(off, col, level)
        times.append((time.perf_counter() - t0) * 1e3)
        info = fill.info
        fill.close()
    return statistics.median(times[1:]), min(times[1:]), max(times[1:]), info


def solve_line(label, solver, val, rhs, args, residual):
    x = torch.empty_like(rhs)
    x.zero_()
    solver.solve(val, rhs, x=x, rtol=args.tol, max_iterations=args.limit, check_every=8)      # finds the count (and warms up)
    state = solver.state
    needed = state["iterations"]

    def run():
        x.zero_()
        solver.solve(val, rhs, x=x, rtol=args.tol, max_iterations=needed, check_every=0)
    run()
    ms, spread, _ = wall(run, args.reps)
    state = solver.state
    print(f"        {label:9s} {needed:5d} iterations x {ms / max(needed, 1):9.4f} ms = {ms:10.3f} ms ({spread:4.1f} %)  {state['status']}  "
          f"true |b - A x| / |b| {residual(x):.2e}", flush=True)
    return needed, ms


def bench(case, order, args):
    name, off, col = CASES[case]()
    rows, nnz = off.numel() - 1, col.numel()
    spd = laplacian_values(off, col, 4.0 + args.shift if case == "grid" else None)
    wind = convection_values(off, col, args.wind, args.shift if case == "grid" else 0.0)
    b = G.uniform_pm1(29, rows, torch.float64, "cuda")
    norm_b = float(torch.linalg.norm(b))
    coloring = None
    o, c, v_spd, v_wind, rhs = off, col, spd, wind, b
    if order == "multicolour":
        coloring, p = M.multicolor_reorder(spd, off, col)
        o, c, v_spd = p.row_offsets, p.column_indices, p.values
        v_wind = M.csr_permute(wind, off, col, rows, row_perm=coloring.order, col_map=coloring.inverse).values
        rhs = coloring.permute_vector(b)
    print(f"{name}, {order} order{' (%d colours)' % coloring.num_colors if coloring else ''}: rows {rows}  nnz {nnz}  fp64  tol {args.tol:g}", flush=True)

    def residual_of(values):
        def residual(x):
            back = x if coloring is None else coloring.permute_vector(x, back=True)
            return float(torch.linalg.norm(b - M.csrmv(values, off, col, back, num_cols=rows))) / norm_b
        return residual

    z = torch.empty_like(rhs)
    ilu0_ms = None
    for level in LEVELS:
        sym, sym_lo, sym_hi, info = symbolic_ms(o, c, level, args.reps)
        ic, ilu = M.Ick(o, c, level), M.Iluk(o, c, level)
        assert int(ic.factor(v_spd).item()) == -1 and int(ilu.factor(v_wind).item()) == -1
        # the scatter and the factorisations alone, through the public calls, on arrays of their own
        f_spd, f_wind = ic.fill.values(v_spd), ilu.fill.values(v_wind)
        out = torch.empty_like(f_spd)
        val_ms, _ = timed(lambda: ic.fill.values(v_spd, out=out), 10, warm=3)
        ic_ms, _ = timed(lambda: M.csric0(f_spd, ic.row_offsets, ic.column_indices, plan=ic.lower, out=out, mirror=True), 5, warm=2)
        ilu_ms, _ = timed(lambda: M.csrilu0(f_wind, ilu.row_offsets, ilu.column_indices, plan=ilu.lower, out=out), 5, warm=2)
        if level == 0:
            ilu0_ms = ilu_ms
        del f_spd, f_wind, out
        sw_ic, _ = timed(lambda: ic.solve(rhs, out=z), 10, warm=3)
        sw_ilu, _ = timed(lambda: ilu.solve(rhs, out=z), 10, warm=3)
        lo, up = ic.lower.info, ic.upper.info
        print(f"    level {level}: nnz_filled {info['nnz_filled']} ({info['nnz_filled'] / nnz:4.2f} x), max level {info['max_level']}; symbolic "
              f"{sym:9.3f} ms ({sym_lo:.3f} .. {sym_hi:.3f}) = {sym / ilu0_ms:6.2f} x one csrilu0 at level 0; values {val_ms:7.4f} ms", flush=True)
        print(f"        plans: LOWER {lo['levels']} levels, {lo['launches']} launches; UPPER {up['levels']} levels, {up['launches']} launches; "
              f"csric0 {ic_ms:9.4f} ms, csrilu0 {ilu_ms:9.4f} ms; one sweep pair: IC {sw_ic:8.4f} ms, ILU {sw_ilu:8.4f} ms", flush=True)
        pcg = M.Pcg(o, c, torch.float64, preconditioner=ic)
        solve_line("Pcg", pcg, v_spd, rhs, args, residual_of(spd))
        pcg.close()
        bi = M.Bicgstab(o, c, torch.float64, preconditioner=ilu)
        solve_line("Bicgstab", bi, v_wind, rhs, args, residual_of(wind))
        bi.close()
        ic.close(); ilu.close()
        torch.cuda.empty_cache()
    if coloring is not None:
        coloring.close()


def bench_limit(reps):
    """the arrow with a dense first row and column, n = 46 400, at level 1: (n - 1)^2 > 2^31 pairs, refused from the counts"""
    n = 46400
    here = torch.arange(n, dtype=torch.int32, device="cuda")
    off = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), n + 2 * here]).contiguous()
    col = torch.cat([here, torch.stack([torch.zeros(n - 1, dtype=torch.int32, device="cuda"), here[1:]], dim=1).reshape(-1)]).contiguous()
    times = []
    for _ in range(reps + 1):                                        # (the first run is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            M.CsrFill(off, col, 1).close()
            refused = False
        except M.MspmvError:
            refused = True
        times.append((time.perf_counter() - t0) * 1e3)
    print(f"arrow with a dense first row and column, {n} rows, nnz {col.numel()}, level 1: {(n - 1) ** 2} pairs, "
          f"{'REFUSED from the counts' if refused else 'NOT refused'} after {statistics.median(times[1:]):7.3f} ms (the Python call included)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="grid,grid3d")
    ap.add_argument("--orders", default="multicolour,natural")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--wind", type=float, default=0.5)
    ap.add_argument("--shift", type=float, default=0.01)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fill_bench needs a GPU"
    print(f"# fill_bench: {torch.cuda.get_device_name(0)}; symbolic and solves = median wall clock of {args.reps} runs ending in a synchronisation, "
          f"after a warm-up run (spread = (max - min) / median); values, factorisations and sweeps = median of calls between their own events", flush=True)
    for case in [s for s in args.cases.split(",") if s]:
        if case == "limit":
            bench_limit(args.reps)
            continue
        for order in [s for s in args.orders.split(",") if s]:
            bench(case, order, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
