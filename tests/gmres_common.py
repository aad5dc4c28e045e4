"""What the GMRES tests share (tests/test_gmres_model.py, tests/test_gmres.py) beside bicgstab_common and pcg_common: the table of
exits and the cases of the grids.  Nothing here calls the library."""
NAN, INF = float("nan"), float("inf")

RESTARTS = [1, 2, 5, 20, 30, 64]                # the model converges on both grids with each of these
BAND_RESTARTS = [1, 3, 30]
MISS = dict(grid=(24, 24), prec="f32", rtol=3e-7, restart=30)        # the estimate closes a cycle whose true residual misses

# name -> (A, b, restart, max_iterations, status, iterations, exit): small dense-stored systems on which the exit is taken in exact
# arithmetic too (fp32 and fp64 alike, with no preconditioner); all but "lucky" and "none" keep every intermediate exactly representable
EXIT_CASES = {
    "start": ([[1, 2], [3, 4]], [0, 0], 30, 10, "CONVERGED", 0, "start"),
    "beta-nan": ([[1, 2], [3, 4]], [NAN, 0], 30, 10, "BREAKDOWN", 0, "beta"),
    "beta-inf": ([[1, 2], [3, 4]], [INF, 0], 30, 10, "BREAKDOWN", 0, "beta"),
    "d-first": ([[0, 0], [0, 0]], [1, -1], 30, 10, "BREAKDOWN", 0, "d"),
    "d-second": ([[0, 1], [0, 0]], [0, 1], 30, 10, "BREAKDOWN", 1, "d"),
    "lucky": ([[3, 0], [0, 3]], [1, -2], 30, 10, "CONVERGED", 1, "rr"),
    "none": ([[4, -1, 0], [-2, 4, -1], [0, -2, 4]], [1, 2, 3], 2, 1, "RUNNING", 1, None),
    "stagnation": ([[0, 1], [-1, 0]], [1, 0], 1, 6, "RUNNING", 6, None),
    "stagnation-2": ([[0, 1], [-1, 0]], [1, 0], 2, 6, "CONVERGED", 2, "rr"),
}
