"""Times the conjugate gradients on the device (mspmv_pcg_*; merge_spmv_amd.Pcg) against the torch loop they replace, and the deterministic
dot product (mspmv_vec_dot_*) against torch.dot:
python tools/pcg_bench.py [--reps 5] > profiles/pcg_bench.txt
One case per process keeps every GPU step under a time limit of its own:
timeout 600 python tools/pcg_bench.py --cases grid > profiles/pcg_bench.txt && timeout 600 python tools/pcg_bench.py --cases grid3d --no-dot >> ...

Cases, fp64, in multicolour order (CsrColoring, csr_permute), preconditioned by IC(0) of P A P^T, to rr <= (tol |b|)^2:
  grid     the 5-point Laplacian + --shift I on 2000 x 2000 points (the PCG case of tools/color_bench.py)
  grid3d   the 7-point grid of 128^3 points, every off-diagonal entry -1, the diagonal the row's length
Per case, each the median wall clock of --reps runs that end in a device synchronisation, after a warm-up run:
  torch loop      `pcg` of tools/color_bench.py as it stands: two torch.dot, four elementwise passes and one float(norm) per iteration
  Pcg.solve       check_every = 1, 8 and 0 (0: exactly the iterations the solve needs are enqueued, nothing is read back)
  graph replay    the check_every = 0 solve (x zeroed inside the graph) captured once, replayed
and, each between its own events, one product, the two sweeps and one iteration's launches of the solver's own (the rest of the loop
after the product and the sweeps are taken out).  x of every variant is checked: the true residual |b - A x| / |b| in the original
numbering.  Iteration counts may differ by a few from the torch loop: the dots add in another order.
vec_dot: n = 4 * 10^6, fp64 and fp32, against torch.dot on the same vectors, after a warm-up, the median of --dot-reps of: one call between
its own events (which includes the host's enqueue: two launches through ctypes against one BLAS call), and 20 calls captured in one
graph, the replay between events, per call (the device's time alone)."""
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
from tools.color_bench import pcg as torch_pcg, values_for
from tools.csrilu0_bench import CASES
from tools.csrsv_bench import timed


CALLS = 20          # dot products per captured graph


def wall(fn, reps):
    """median wall clock in ms of reps calls, each ending in a synchronisation; the last call's result"""
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times) * 100, out


def bench_dot(reps):
    n = 4_000_000
    for dtype in (torch.float64, torch.float32):
        a, b = G.uniform_pm1(31, n, dtype, "cuda"), G.uniform_pm1(37, n, dtype, "cuda")
        out = torch.empty(1, dtype=dtype, device="cuda")
        temp = torch.empty(64 * 1024, dtype=torch.uint8, device="cuda")                  # (3907 partials)
        ours, s_ours = timed(lambda: M.vec_dot(a, b, out=out, temp=temp), reps, warm=5)
        ref = torch.empty((), dtype=dtype, device="cuda")
        theirs, s_theirs = timed(lambda: torch.dot(a, b, out=ref), reps, warm=5)
        sq, s_sq = timed(lambda: M.vec_dot(a, a, out=out, temp=temp), reps, warm=5)
        M.vec_dot(a, b, out=out, temp=temp)
        rel = abs(float(out.item()) - float(ref.item())) / abs(float(ref.item()))
        print(f"vec_dot {str(dtype):14s} n {n}, one call between events (the host's enqueue included): {ours * 1e3:8.1f} us ({s_ours:4.1f} %) | torch.dot "
              f"{theirs * 1e3:8.1f} us ({s_theirs:4.1f} %)  torch / ours = {theirs / ours:5.2f} | a == b {sq * 1e3:8.1f} us ({s_sq:4.1f} %) | "
              f"relative difference of the two sums {rel:.1e}", flush=True)
        # the device's time alone: CALLS calls captured in one graph, the replay between events, per call
        per = {}
        for label, fn in (("vec_dot", lambda: M.vec_dot(a, b, out=out, temp=temp)), ("torch.dot", lambda: torch.dot(a, b, out=ref))):
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    for _ in range(CALLS):
                        fn()
            except RuntimeError as e:                                 # (a BLAS call that cannot be captured: reported, not hidden)
                print(f"    {label}: not capturable ({str(e).splitlines()[0]})", flush=True)
                per[label] = (float("nan"), float("nan"))
                torch.cuda.synchronize()
                continue
            ms, spread = timed(graph.replay, reps, warm=5)
            per[label] = (ms / CALLS * 1e3, spread)
        gbs = 2 * n * a.element_size() / (per["vec_dot"][0] * 1e-6) / 1e9
        print(f"vec_dot {str(dtype):14s} n {n}, {CALLS} calls in a replayed graph, per call: {per['vec_dot'][0]:8.1f} us ({per['vec_dot'][1]:4.1f} %)  {gbs:6.0f} GB/s | "
              f"torch.dot {per['torch.dot'][0]:8.1f} us ({per['torch.dot'][1]:4.1f} %)  torch / ours = {per['torch.dot'][0] / per['vec_dot'][0]:5.2f}", flush=True)


def bench_case(case, args):
    name, off, col = CASES[case]()
    rows, nnz = off.numel() - 1, col.numel()
    val = values_for(off, col, 4.0 + args.shift if case == "grid" else None)
    print(f"{name}{' (+ %g I)' % args.shift if case == 'grid' else ''}: rows {rows}  nnz {nnz}  fp64  tol {args.tol:g}", flush=True)
    coloring, p = M.multicolor_reorder(val, off, col)
    o, c, v = p.row_offsets, p.column_indices, p.values
    b = G.uniform_pm1(29, rows, torch.float64, "cuda")
    rhs = coloring.permute_vector(b)
    norm_b = float(torch.linalg.norm(b))
    ic = M.Ic0(o, c)
    assert int(ic.factor(v).item()) == -1
    print(f"    {coloring.num_colors} colours; lower sweep {ic.lower.info['launches']} launches, upper sweep {ic.upper.info['launches']}", flush=True)

    def residual(x):
        return float(torch.linalg.norm(b - M.csrmv(val, off, col, coloring.permute_vector(x, back=True), num_cols=rows))) / norm_b

    def line(label, ms, spread, its, x, note=""):
        print(f"    {label:28s} {its:5d} iterations  {ms:10.3f} ms ({spread:4.1f} %)  {ms / max(its, 1):8.4f} ms per iteration  "
              f"true |b - A x| / |b| {residual(x):.2e}{note}", flush=True)

    torch_pcg(v, o, c, rhs, ic.solve, args.tol, args.limit)                              # warm-up
    ms, spread, (x, its) = wall(lambda: torch_pcg(v, o, c, rhs, ic.solve, args.tol, args.limit), args.reps)
    line("torch loop (color_bench.pcg)", ms, spread, its, x, " (NOT converged)" if its > args.limit else "")
    base = ms / max(its, 1)

    solver = M.Pcg(o, c, torch.float64, preconditioner=ic)
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
        line(f"Pcg.solve check_every = {check_every}", ms, spread, state["iterations"], x,
             f"  {state['status']}  loop / this per iteration = {base / (ms / max(needed, 1)):5.2f}")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.zero_()
        solver.solve(v, rhs, x=x, rtol=args.tol, max_iterations=needed, check_every=0)
    graph.replay()
    ms, spread, _ = wall(graph.replay, args.reps)
    state = solver.state
    line("graph replay", ms, spread, state["iterations"], x, f"  {state['status']}  loop / this per iteration = {base / (ms / max(needed, 1)):5.2f}")
    # where an iteration's time goes: the product and the sweeps alone
    q, z = torch.empty_like(rhs), torch.empty_like(rhs)
    ws = M.CsrMVWorkspace(rows, nnz, torch.float64)
    ws.prepare(o)
    mv, s_mv = timed(lambda: M.csrmv(v, o, c, rhs, y=q, num_cols=rows, workspace=ws), 20, warm=5)
    sw, s_sw = timed(lambda: ic.solve(rhs, out=z), 20, warm=5)
    per = ms / max(needed, 1)
    print(f"    one iteration of the replay {per:8.4f} ms = product {mv:7.4f} ms ({s_mv:4.1f} %) + two sweeps {sw:7.4f} ms ({s_sw:4.1f} %) + "
          f"{solver.launches_per_iteration} launches of the solver's own {per - mv - sw:7.4f} ms (by difference)", flush=True)
    solver.close(); ic.close(); coloring.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dot-reps", type=int, default=50)
    ap.add_argument("--cases", default="grid,grid3d")
    ap.add_argument("--no-dot", action="store_true")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--shift", type=float, default=0.01, help="the grid case: the diagonal is 4 + shift")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pcg_bench needs a GPU"
    print(f"# pcg_bench: {torch.cuda.get_device_name(0)}; solves = median wall clock of {args.reps} runs ending in a synchronisation, after a warm-up run "
          f"(spread = (max - min) / median); vec_dot = median of {args.dot_reps} calls, each between its own events", flush=True)
    if not args.no_dot:
        bench_dot(args.dot_reps)
    for case in [s for s in args.cases.split(",") if s]:
        bench_case(case, args)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
