"""Times restarted GMRES(m) on the device (mspmv_gmres_*; merge_spmv_amd.Gmres) against the torch loop it replaces and against Bicgstab:
python tools/gmres_bench.py [--reps 5] > profiles/gmres_bench.txt
One case per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/gmres_bench.py --cases grid > profiles/gmres_bench.txt && timeout 600 python tools/gmres_bench.py --cases grid3d >> ...
and the two block kernels alone, from a kernel trace taken in a run of its own:
timeout 600 rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gmres_bench.py --cases grid --block && python tools/gmres_bench.py --trace DIR --cases grid >> ...

Cases, fp64, the NONSYMMETRIC convection-diffusion matrices of tools/bicgstab_bench.py in multicolour order, preconditioned from the right
by ILU(0) of P A P^T, restart = --restart (30), to a true residual rr <= (tol |b|)^2:
  grid     the 5-point stencil on 2000 x 2000 points
  grid3d   the 7-point stencil on 128^3 points
Per case, each the median wall clock of --reps runs that end in a device synchronisation, after a warm-up run:
  torch loop      `torch_gmres` below: the same M.csrmv and Ilu0.solve, torch.mv on the basis for both Gram-Schmidt passes, a norm,
                  Givens rotations on the host and ONE read-back (the column and the norm) per iteration
  Gmres.solve     check_every = 1, restart and 0 (0: exactly the slots the solve needs are enqueued, nothing is read back)
  graph replay    the check_every = 0 solve (x zeroed inside the graph) captured once, replayed
  Bicgstab.solve  check_every = 0 at the iterations it needs: the time to solution of the other nonsymmetric solver
and, each between its own events, one product and one pair of sweeps.  x of every variant is checked: the true residual
|b - A x| / |b| in the original numbering.  Iteration counts may differ from the torch loop's: its dots add in another order.
--block runs nothing but four solves of exactly `restart` slots that cannot converge (rtol = 0), for the trace; --trace reads the
kernel trace back: of every solve's gmres_dots_kernel and gmres_orth_kernel launches the last ones (j = restart - 1), as bytes over
time against the 8 TB/s peak."""
import argparse
import csv
import glob
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TBS = 8.0


def torch_gmres(val, off, col, b, precondition, tol, restart, limit):
    """right-preconditioned GMRES(restart) with CGS2 as a torch loop; (x, iterations).  Convergence is declared on the true residual
    of a closing, as the device's is; the rotations' estimate closes a cycle early."""
    import torch
    import merge_spmv_amd as M
    n = b.numel()
    x = torch.zeros_like(b)
    stop = tol * float(torch.linalg.norm(b))
    V = torch.empty((restart + 1, n), dtype=b.dtype, device=b.device)
    r = b.clone()
    its = 0
    while its < limit:
        beta = float(torch.linalg.norm(r))
        if beta <= stop:
            return x, its
        V[0] = r / beta
        g = [beta]
        cs, sn, R = [], [], []
        cols = 0
        for j in range(min(restart, limit - its)):
            w = M.csrmv(val, off, col, precondition(V[j]), num_cols=n)
            basis = V[:j + 1]
            h1 = torch.mv(basis, w)
            w -= torch.mv(basis.t(), h1)
            h2 = torch.mv(basis, w)
            w -= torch.mv(basis.t(), h2)
            column = torch.cat([h1 + h2, torch.linalg.norm(w).reshape(1)]).tolist()     # the one read-back of the iteration
            h, hn = column[:-1], column[-1]
            for i in range(j):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], cs[i] * h[i + 1] - sn[i] * h[i]
            d = math.hypot(h[j], hn)
            if not d > 0:
                break
            cs.append(h[j] / d); sn.append(hn / d)
            R.append(h[:j] + [d])
            g.append(-sn[j] * g[j]); g[j] = cs[j] * g[j]
            its += 1; cols = j + 1
            if abs(g[j + 1]) <= stop or not hn > 0:
                break
            V[j + 1] = w / hn
        if cols == 0:
            return x, limit + 1
        y = [0.0] * cols
        for i in range(cols - 1, -1, -1):
            y[i] = (g[i] - sum(R[l][i] * y[l] for l in range(i + 1, cols))) / R[i][i]
        x += precondition(torch.mv(V[:cols].t(), torch.tensor(y, dtype=b.dtype, device=b.device)))
        r = b - M.csrmv(val, off, col, x, num_cols=n)
    return x, its if float(torch.linalg.norm(r)) <= stop else limit + 1


def system(case, args):
    import torch
    import merge_spmv_amd as M
    from merge_spmv_amd import generators as G
    from tools.bicgstab_bench import values_for
    from tools.csrilu0_bench import CASES
    name, off, col = CASES[case]()
    rows, nnz = off.numel() - 1, col.numel()
    shift = args.shift if case == "grid" else 0.0
    val = values_for(off, col, args.wind, shift)
    print(f"{name} (convection-diffusion: wind {args.wind:g}, shift {shift:g}): rows {rows}  nnz {nnz}  fp64  tol {args.tol:g}  restart {args.restart}",
          flush=True)
    coloring, p = M.multicolor_reorder(val, off, col)
    b = G.uniform_pm1(29, rows, torch.float64, "cuda")
    ilu = M.Ilu0(p.row_offsets, p.column_indices)
    assert int(ilu.factor(p.values).item()) == -1
    return name, (val, off, col), coloring, p, b, ilu


def bench_case(case, args):
    import torch
    import merge_spmv_amd as M
    from tools.csrsv_bench import timed
    from tools.pcg_bench import wall
    name, (val, off, col), coloring, p, b, ilu = system(case, args)
    rows, nnz = off.numel() - 1, col.numel()
    o, c, v = p.row_offsets, p.column_indices, p.values
    rhs = coloring.permute_vector(b)
    norm_b = float(torch.linalg.norm(b))
    print(f"    {coloring.num_colors} colours; lower sweep {ilu.lower.info['launches']} launches, upper sweep {ilu.upper.info['launches']}", flush=True)

    def residual(x):
        return float(torch.linalg.norm(b - M.csrmv(val, off, col, coloring.permute_vector(x, back=True), num_cols=rows))) / norm_b

    def line(label, ms, spread, its, x, note=""):
        print(f"    {label:32s} {its:5d} iterations  {ms:10.3f} ms ({spread:4.1f} %)  {ms / max(its, 1):8.4f} ms per iteration  "
              f"true |b - A x| / |b| {residual(x):.2e}{note}", flush=True)

    torch_gmres(v, o, c, rhs, ilu.solve, args.tol, args.restart, args.limit)               # warm-up
    ms, spread, (x, its) = wall(lambda: torch_gmres(v, o, c, rhs, ilu.solve, args.tol, args.restart, args.limit), args.reps)
    line("torch loop (torch_gmres)", ms, spread, its, x, " (NOT converged)" if its > args.limit else "")
    loop_ms = ms

    solver = M.Gmres(o, c, torch.float64, preconditioner=ilu, restart=args.restart)
    print(f"    the handle holds {solver.state['device_bytes'] / 2 ** 20:.0f} MiB on the device", flush=True)
    x = torch.empty(rows, dtype=torch.float64, device="cuda")
    needed = None
    for check_every in (1, args.restart, 0):
        limit = args.limit if check_every else needed

        def run():
            x.zero_()
            solver.solve(v, rhs, x=x, rtol=args.tol, max_iterations=limit, check_every=check_every)
        run()                                                                             # warm-up
        ms, spread, _ = wall(run, args.reps)
        state = solver.state
        needed = state["slots"]
        line(f"Gmres.solve check_every = {check_every}", ms, spread, state["iterations"], x,
             f"  {state['status']} ({state['exit']}), {state['cycles']} cycles, {state['slots']} slots  loop / this to solution = {loop_ms / ms:5.2f}")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.zero_()
        solver.solve(v, rhs, x=x, rtol=args.tol, max_iterations=needed, check_every=0)
    graph.replay()
    ms, spread, _ = wall(graph.replay, args.reps)
    state = solver.state
    line("graph replay", ms, spread, state["iterations"], x,
         f"  {state['status']} ({state['exit']}), {state['cycles']} cycles, {state['slots']} slots  loop / this to solution = {loop_ms / ms:5.2f}")
    gmres_ms, gmres_its = ms, state["iterations"]
    solver.close()

    other = M.Bicgstab(o, c, torch.float64, preconditioner=ilu)
    x.zero_()
    other.solve(v, rhs, x=x, rtol=args.tol, max_iterations=args.limit, check_every=1)
    its = other.state["iterations"]

    def run_other():
        x.zero_()
        other.solve(v, rhs, x=x, rtol=args.tol, max_iterations=its, check_every=0)
    run_other()
    ms, spread, _ = wall(run_other, args.reps)
    state = other.state
    line("Bicgstab.solve check_every = 0", ms, spread, state["iterations"], x,
         f"  {state['status']} ({state['exit']})  Bicgstab / Gmres replay to solution = {ms / gmres_ms:5.2f}")
    other.close()
    q, z = torch.empty_like(rhs), torch.empty_like(rhs)
    ws = M.CsrMVWorkspace(rows, nnz, torch.float64)
    ws.prepare(o)
    mv, s_mv = timed(lambda: M.csrmv(v, o, c, rhs, y=q, num_cols=rows, workspace=ws), 20, warm=5)
    sw, s_sw = timed(lambda: ilu.solve(rhs, out=z), 20, warm=5)
    per = gmres_ms / max(gmres_its, 1)
    print(f"    one iteration of the Gmres replay, cycle launches included, {per:8.4f} ms: one product {mv:7.4f} ms ({s_mv:4.1f} %) + two sweeps "
          f"{sw:7.4f} ms ({s_sw:4.1f} %) + the solver's own {per - mv - sw:7.4f} ms (by difference; an iteration of Bicgstab has two of each)", flush=True)
    ilu.close(); coloring.close()


def block_case(case, args):
    """four solves of exactly `restart` slots that cannot converge: what the kernel trace is taken of"""
    import torch
    import merge_spmv_amd as M
    _, _, coloring, p, b, ilu = system(case, args)
    rhs = coloring.permute_vector(b)
    solver = M.Gmres(p.row_offsets, p.column_indices, torch.float64, preconditioner=ilu, restart=args.restart)
    x = torch.empty_like(rhs)
    for _ in range(4):
        solver.solve(p.values, rhs, x=x, rtol=0.0, max_iterations=args.restart, check_every=0)
    state = solver.state
    print(f"    --block: four solves of {state['slots']} slots, {state['iterations']} iterations each, {state['status']}", flush=True)
    assert state["iterations"] == args.restart, "a column closed the cycle early: the last launches are not those of j = restart - 1"
    solver.close(); ilu.close(); coloring.close()


def read_trace(directory, case, args):
    """the launches of the two block kernels in the kernel trace under `directory`: every `restart`-th is that of j = restart - 1"""
    rows = {"grid": 2000 * 2000, "grid3d": 128 ** 3}[case]
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {directory}"
    found = {}
    for path in files:
        with open(path, newline="") as f:
            for rec in csv.DictReader(f):
                rec = {k.lower(): val for k, val in rec.items()}
                name = rec.get("kernel_name", "")
                for kernel in ("gmres_dots_kernel", "gmres_orth_kernel"):
                    if kernel in name:
                        found.setdefault(name, []).append((int(rec["start_timestamp"]), int(rec["end_timestamp"]) - int(rec["start_timestamp"])))
    assert found, "the trace holds no gmres_dots_kernel or gmres_orth_kernel launch"
    R, vec = args.restart, rows * 8
    print(f"    the block kernels alone at j = {R - 1} (kernel trace, {case}: vectors of {vec / 1e6:.1f} MB; peak {PEAK_TBS:g} TB/s):", flush=True)
    for name in sorted(found):
        launches = [d for _, d in sorted(found[name])]
        assert len(launches) % R == 0, (name, len(launches))
        last = [launches[i] for i in range(R - 1, len(launches), R)][1:] or launches[R - 1::R]     # (the first solve is the warm-up)
        us = statistics.median(last) / 1e3
        if "dots" in name:
            what, least, moved = "w . V", (R + 1) * vec, (R + 1) * vec
        elif "true" in name or "Lb1" in name:
            what, least, moved = "w -= V h1, then w . V", (R + 2) * vec, (2 * R + 2) * vec
        else:
            what, least, moved = "w -= V h2, then w . w", (R + 2) * vec, (R + 2) * vec
        print(f"      {name[:60]:60s} {what:24s} {us:9.1f} us (median of {len(last)}, {min(last) / 1e3:.1f} .. {max(last) / 1e3:.1f})  "
              f"requested {moved / 1e6:7.1f} MB = {moved / us / 1e6:5.2f} TB/s ({moved / us / 1e6 / PEAK_TBS:4.2f} of peak)  "
              f"least {least / 1e6:7.1f} MB = {least / us / 1e6:5.2f} TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="grid,grid3d")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--wind", type=float, default=0.5, help="the entries below the diagonal are -1 - wind, those above it -1 + wind")
    ap.add_argument("--shift", type=float, default=0.01, help="the grid case: the diagonal is the row's length + shift")
    ap.add_argument("--block", action="store_true", help="only the solves whose kernel trace --trace reads")
    ap.add_argument("--trace", default=None, help="a directory that holds rocprofv3's *kernel_trace.csv of a --block run (needs no GPU)")
    args = ap.parse_args()
    cases = [s for s in args.cases.split(",") if s]
    if args.trace:
        for case in cases:
            read_trace(args.trace, case, args)
        return
    import torch
    assert torch.cuda.is_available(), "gmres_bench needs a GPU"
    if not args.block:
        print(f"# gmres_bench: {torch.cuda.get_device_name(0)}; solves = median wall clock of {args.reps} runs ending in a synchronisation, after a "
              f"warm-up run (spread = (max - min) / median)", flush=True)
    for case in cases:
        block_case(case, args) if args.block else bench_case(case, args)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
