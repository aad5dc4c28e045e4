"""Times BiCGStab on the device (mspmv_bicgstab_*; merge_spmv_amd.Bicgstab) against the torch loop it replaces:
python tools/bicgstab_bench.py [--reps 5] > profiles/bicgstab_bench.txt
One case per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/bicgstab_bench.py --cases grid > profiles/bicgstab_bench.txt && timeout 600 python tools/bicgstab_bench.py --cases grid3d >> ...

Cases, fp64, NONSYMMETRIC convection-diffusion matrices in multicolour order (CsrColoring, csr_permute), preconditioned from the right by
ILU(0) of P A P^T, to rr <= (tol |b|)^2:
  grid     the 5-point stencil on 2000 x 2000 points: the diagonal is the row's length + --shift, -1 - --wind below the diagonal,
           -1 + --wind above it
  grid3d   the same 7-point stencil on 128^3 points, no shift
Per case, each the median wall clock of --reps runs that end in a device synchronisation, after a warm-up run:
  torch loop      `torch_bicgstab` below: the same M.csrmv and Ilu0.solve, four torch.dot, six elementwise passes and one float(norm)
                  per iteration
  Bicgstab.solve  check_every = 1, 8 and 0 (0: exactly the iterations the solve needs are enqueued, nothing is read back)
  graph replay    the check_every = 0 solve (x zeroed inside the graph) captured once, replayed
and, each between its own events, one product, one pair of sweeps and one iteration's launches of the solver's own (the rest of an
iteration of the replay after two products and four sweeps are taken out).  x of every variant is checked: the true residual
|b - A x| / |b| in the original numbering.  Iteration counts may differ from the torch loop's: its dots add in another order and it
does not test the half step."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import merge_spmv_amd as M
from merge_spmv_amd import generators as G
from tools.color_bench import entry_rows
from tools.csrilu0_bench import CASES
from tools.csrsv_bench import timed
from tools.pcg_bench import wall


def values_for(off, col, wind, shift):
    """convection-diffusion on the pattern: the row's length (+ shift) on the diagonal, -1 - wind below it, -1 + wind above it"""
    rows = off.numel() - 1
    r = entry_rows(off, rows)
    c = col.to(torch.int64)
    lens = torch.diff(off.to(torch.int64))[r].to(torch.float64)
    side = torch.where(c < r, torch.full_like(lens, -1.0 - wind), torch.full_like(lens, -1.0 + wind))
    return torch.where(c == r, lens + shift, side)


def torch_bicgstab(val, off, col, b, precondition, tol, limit):
    """right-preconditioned BiCGStab as a torch loop; (x, iterations)"""
    n = b.numel()
    x = torch.zeros_like(b)
    r = b.clone()
    rh = r.clone()
    p = r.clone()
    rho = torch.dot(r, r)
    stop = tol * float(torch.linalg.norm(b))
    for it in range(1, limit + 1):
        ph = precondition(p)
        v = M.csrmv(val, off, col, ph, num_cols=n)
        alpha = rho / torch.dot(rh, v)
        x += alpha * ph
        s = r - alpha * v
        sh = precondition(s)
        t = M.csrmv(val, off, col, sh, num_cols=n)
        omega = torch.dot(t, s) / torch.dot(t, t)
        x += omega * sh
        r = s - omega * t
        if float(torch.linalg.norm(r)) <= stop:
            return x, it
        rho_new = torch.dot(rh, r)
        p = r + (rho_new / rho) * (alpha / omega) * (p - omega * v)
        rho = rho_new
    return x, limit + 1


def bench_case(case, args):
    name, off, col = CASES[case]()
    rows, nnz = off.numel() - 1, col.numel()
    shift = args.shift if case == "grid" else 0.0
    val = values_for(off, col, args.wind, shift)
    print(f"{name} (convection-diffusion: wind {args.wind:g}, shift {shift:g}): rows {rows}  nnz {nnz}  fp64  tol {args.tol:g}", flush=True)
    coloring, p = M.multicolor_reorder(val, off, col)
    o, c, v = p.row_offsets, p.column_indices, p.values
    b = G.uniform_pm1(29, rows, torch.float64, "cuda")
    rhs = coloring.permute_vector(b)
    norm_b = float(torch.linalg.norm(b))
    ilu = M.Ilu0(o, c)
    assert int(ilu.factor(v).item()) == -1
    print(f"    {coloring.num_colors} colours; lower sweep {ilu.lower.info['launches']} launches, upper sweep {ilu.upper.info['launches']}", flush=True)

    def residual(x):
        return float(torch.linalg.norm(b - M.csrmv(val, off, col, coloring.permute_vector(x, back=True), num_cols=rows))) / norm_b

    def line(label, ms, spread, its, x, note=""):
        print(f"    {label:32s} {its:5d} iterations  {ms:10.3f} ms ({spread:4.1f} %)  {ms / max(its, 1):8.4f} ms per iteration  "
              f"true |b - A x| / |b| {residual(x):.2e}{note}", flush=True)

    torch_bicgstab(v, o, c, rhs, ilu.solve, args.tol, args.limit)                          # warm-up
    ms, spread, (x, its) = wall(lambda: torch_bicgstab(v, o, c, rhs, ilu.solve, args.tol, args.limit), args.reps)
    line("torch loop (torch_bicgstab)", ms, spread, its, x, " (NOT converged)" if its > args.limit else "")
    base = ms / max(its, 1)

    solver = M.Bicgstab(o, c, torch.float64, preconditioner=ilu)
    x = torch.empty(rows, dtype=torch.float64, device="cuda")
    needed = None
    for check_every in (1, 8, 0):
        limit = args.limit if check_every else needed

        def run():
            x.zero_()
            solver.solve(v, rhs, x=x, rtol=args.tol, max_iterations=limit, check_every=check_every)
        run()                                                                             # warm-up
        ms, spread, _ = wall(run, args.reps)
        state = solver.state
        needed = state["iterations"]
        line(f"Bicgstab.solve check_every = {check_every}", ms, spread, state["iterations"], x,
             f"  {state['status']} ({state['exit']})  loop / this per iteration = {base / (ms / max(needed, 1)):5.2f}")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.zero_()
        solver.solve(v, rhs, x=x, rtol=args.tol, max_iterations=needed, check_every=0)
    graph.replay()
    ms, spread, _ = wall(graph.replay, args.reps)
    state = solver.state
    line("graph replay", ms, spread, state["iterations"], x,
         f"  {state['status']} ({state['exit']})  loop / this per iteration = {base / (ms / max(needed, 1)):5.2f}")
    # where an iteration's time goes: one product and one pair of sweeps alone; an iteration has two of each
    q, z = torch.empty_like(rhs), torch.empty_like(rhs)
    ws = M.CsrMVWorkspace(rows, nnz, torch.float64)
    ws.prepare(o)
    mv, s_mv = timed(lambda: M.csrmv(v, o, c, rhs, y=q, num_cols=rows, workspace=ws), 20, warm=5)
    sw, s_sw = timed(lambda: ilu.solve(rhs, out=z), 20, warm=5)
    per = ms / max(needed, 1)
    print(f"    one iteration of the replay {per:8.4f} ms = two products 2 x {mv:7.4f} ms ({s_mv:4.1f} %) + four sweeps 2 x {sw:7.4f} ms ({s_sw:4.1f} %) + "
          f"{solver.launches_per_iteration} launches of the solver's own {per - 2 * mv - 2 * sw:7.4f} ms (by difference)", flush=True)
    solver.close(); ilu.close(); coloring.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="grid,grid3d")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--wind", type=float, default=0.5, help="the entries below the diagonal are -1 - wind, those above it -1 + wind")
    ap.add_argument("--shift", type=float, default=0.01, help="the grid case: the diagonal is the row's length + shift")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bicgstab_bench needs a GPU"
    print(f"# bicgstab_bench: {torch.cuda.get_device_name(0)}; solves = median wall clock of {args.reps} runs ending in a synchronisation, after a "
          f"warm-up run (spread = (max - min) / median)", flush=True)
    for case in [s for s in args.cases.split(",") if s]:
        bench_case(case, args)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
