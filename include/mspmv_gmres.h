/* mspmv_gmres.h -- restarted GMRES(m) built ON TOP of the C ABI of mspmv.h (libmspmv_gmres.so; plain C99).
 *
 * The layer calls only what libmspmv.so exports -- mspmv_csrmv_prepare, mspmv_csrmv_prepared_*, mspmv_csrsv_solve_*,
 * mspmv_csrsv_plan_info -- and is linked against the libmspmv.so next to it, as libmspmv_krylov.so (mspmv_krylov.h: BiCGStab) is.  It
 * serves the NONSYMMETRIC case, for which mspmv_csrilu0_* makes the factor.
 *
 * ---- RIGHT-PRECONDITIONED RESTARTED GMRES(m) on the device (csrc/mspmv_gmres.hip): A x = b for a square A in CSR, as one call.
 * The orthogonalisation is classical Gram-Schmidt applied twice (CGS2): a fixed number of launches per iteration whatever the
 * column, on blocks of basis vectors.  The Hessenberg column is reduced by Givens rotations in a one-workgroup step.  The scalars,
 * the triangle R, the rotations and g live on the device; every dot is the deterministic reduction R(.) of mspmv.h
 * (mspmv_vec_dot_*), and the host reads nothing inside the loop unless asked to.
 * THE HANDLE is opaque and OWNS ITS STORAGE, as mspmv_bicgstab_t does.  mspmv_gmres_create ALLOCATES (one hipMalloc: the basis
 * vectors v_0 .. v_restart (restart + 1 of them), w, for JACOBI and FACTOR one more for M^-1 v, for FACTOR mid, the partial sums
 * (restart + 1 rows of level-1 partials, each row 16-byte aligned), R, the rotations, g, y, the column, the state block, the diagonal for JACOBI, and the temp storage of mspmv_csrmv_prepared_* in the size its query
 * states), runs mspmv_csrmv_prepare on d_row_offsets, for JACOBI finds every row's diagonal entry (one lane per row) and reads
 * state.bad_diagonal_row back; it is SYNCHRONOUS.  It depends on the pattern and on `restart` alone: new values need no new handle.
 * 1 <= restart <= MSPMV_GMRES_MAX_RESTART: the cap bounds the one-workgroup step's working set and the partial array; it is a
 * definition, not a tuning result.
 * PRECONDITIONER M, chosen at creation and applied from the right (A M^-1 y = b, x = M^-1 y; the residual is that of A x = b):
 *     MSPMV_GMRES_NONE     M^-1 v = v (an alias: nothing is copied)
 *     MSPMV_GMRES_JACOBI   (M^-1 v)[e] = v[e] / d[e], d[e] the stored diagonal entry of row e of d_values, taken once per solve; the
 *                          division is made by the pass that writes v.  A pattern with a row of no or of more than one diagonal
 *                          entry (state.bad_diagonal_row >= 0) is refused by the solve.
 *     MSPMV_GMRES_FACTOR   M^-1 v = second^-1 (first^-1 v): mspmv_csrsv_solve_* with first_plan into mid, then with second_plan,
 *                          alpha = 1, both on d_factor_values with ITS pattern arrays (mspmv_gmres_set_factor; none of them is copied
 *                          or owned: they live as long as solves use them).  ILU(0): first = LOWER + UNIT, second = UPPER + NON_UNIT
 *                          on the factor of mspmv_csrilu0_*.
 * ARITHMETIC, all in the value type T, every operation rounded on its own (no fused multiply-add), nothing flushed to zero, every
 * root the correctly rounded sqrt; fl(.) marks a rounding where a line holds more than one:
 *     x = +0.0, r = b            (use_x_as_guess: q = A x by mspmv_csrmv_prepared_*, r[e] = b[e] - q[e])
 *     bb = R(b o b);  rt = (T) rtol, at = (T) atol;  s0 = fl(fl(rt * rt) * bb), a2 = fl(at * at);  stop2 = s0 > a2 ? s0 : a2
 *     rr = R(r o r);  history[0] = rr;  iterations = 0;  slots = 0;  cycles = 0;  beta = 0
 *     rr <= stop2 and rr < +Inf  ->  CONVERGED (start)
 *     cycle, while RUNNING and slots < max_iterations:
 *         beta = sqrt(rr);     not (beta > 0 and beta < +Inf)  ->  BREAKDOWN (beta)        (a NaN or infinite residual ends here)
 *         v_0[e] = r[e] / beta;  g_0 = beta;  width = min(restart, max_iterations - slots);  slots += width;  cycles += 1;  cols = 0
 *         for j = 0 .. width - 1:                                                             (k = iterations + 1)
 *             z = M^-1 v_j;  w = A z
 *             h1_i = R(v_i o w), i = 0 .. j;      w[e] = w[e] - fl(h1_i * v_i[e]), i = 0 .. j in this order
 *             h2_i = R(v_i o w), i = 0 .. j;      w[e] = w[e] - fl(h2_i * v_i[e]), i = 0 .. j in this order
 *             h_i = h1_i + h2_i;  hn = sqrt(R(w o w));  h_{j+1} = hn
 *             for i = 0 .. j - 1:  t = fl(fl(c_i * h_i) + fl(s_i * h_{i+1}));  h_{i+1} = fl(fl(c_i * h_{i+1}) - fl(s_i * h_i));  h_i = t
 *             d = sqrt(fl(fl(h_j * h_j) + fl(hn * hn)))
 *             not (d > 0 and d < +Inf)  ->  the column is dropped (nothing of this iteration is written, iterations stays) and the
 *                                           cycle closes with BREAKDOWN (d) pending
 *             c_j = h_j / d;  s_j = hn / d;  R[.][j] = (h_0 .. h_{j-1}, d);  g_{j+1} = fl((-s_j) * g_j);  g_j = fl(c_j * g_j)
 *             gg = fl(g_{j+1} * g_{j+1});  history[k] = gg;  iterations = k;  cols = j + 1
 *             the cycle closes if gg <= stop2, or gg is NaN, or not (hn > 0), or j == width - 1;  otherwise v_{j+1}[e] = w[e] / hn
 *         closing, with cols columns (cols == 0: x, r and rr stay):
 *             y_i, i = cols - 1 .. 0:  acc = g_i;  acc = acc - fl(R[i][l] * y_l) for l = i + 1 .. cols - 1 ascending;  y_i = acc / R[i][i]
 *             u[e] = fl(y_0 * v_0[e]);  u[e] = u[e] + fl(y_i * v_i[e]), i = 1 .. cols - 1
 *             x[e] = x[e] + (M^-1 u)[e];  q = A x;  r[e] = b[e] - q[e];  rr = R(r o r);  history[iterations] = rr   (the TRUE residual)
 *             BREAKDOWN (d) pending  ->  BREAKDOWN (d);     rr <= stop2 and rr < +Inf  ->  CONVERGED (rr);     otherwise the next cycle
 * (stop2 with a NaN s0 is a2.  An infinite residual never converges, whatever stop2 is.)  CONSEQUENCES:
 *   - convergence is only ever declared on a TRUE residual; the estimate gg only closes a cycle early (and a cycle it closed whose
 *     true residual misses stop2 is followed by the next cycle);
 *   - history[iterations] always equals state.rr; the entries 1 .. iterations - 1 between two closings are estimates gg;
 *   - max_iterations counts iteration SLOTS: a cycle that closes early forfeits the rest of its width slots, so iterations <= slots
 *     <= max_iterations and a solve may end RUNNING (exit_test 0) with iterations < max_iterations.  This keeps the enqueued
 *     sequence a function of (restart, max_iterations) alone; graph capture and "the same bits for every check_every" rest on that;
 *   - x, iterations, slots, cycles, the status, exit_test and the history are functions of the inputs alone -- not of check_every,
 *     the grid or the alignment of b and x.  tests/gmres_model.py is this restatement in numpy.
 * LAUNCHES, all on one stream, ordered by the kernel boundary alone; no workgroup waits on another; no floating-point atomics.
 * Beside the product and (FACTOR) the two sweeps, an inner iteration launches state.launches_per_iteration = 7 kernels of the solver's
 * own, for every kind: the chunk sums of v_i o w for i = 0 .. j in one pass over w (gmres_dots_kernel); the step that folds them to
 * h1 (one workgroup per i); w -= sum h1_i v_i fused with the chunk sums of v_i o w on the new w (gmres_orth_kernel); the step that
 * folds them to h2 and h; w -= sum h2_i v_i fused with the chunk sums of w o w; the one-workgroup step of hn, the rotations, d, the
 * tests, g and the history; v_{j+1} = w / hn (JACOBI: and z = v_{j+1} / d) (gmres_scale_kernel).  A cycle adds
 * state.launches_per_cycle (5; FACTOR 6) beside one product and (FACTOR) two sweeps: the scale that makes v_0; the back substitution;
 * u = V y fused with x += (FACTOR: u alone, then the sweeps, then x +=); the residual fused with the chunk sums of r o r; the step
 * that folds rr, tests, writes the history and makes beta and g_0.  A solve starts with (a guess: the product,) the residual kernel
 * and a step.
 * THE FREEZE has two levels, both read from the state block.  Once the status is not RUNNING, every later kernel of the solver's own
 * returns at once.  Once a cycle has closed, the kernels of that cycle's remaining inner slots return at once; the closing kernels
 * still run, and the last of them clears the flag.  x, the state and the history entries beyond `iterations` stay as they are (the
 * products and the sweeps still run, on scratch).  Hence
 *     check_every = c > 0   the state block is read back (one small copy, one synchronisation) once c inner slots have been enqueued
 *                           since the last look: inside a cycle, where a closed cycle lets the call skip the rest of its inner slots
 *                           (they still count), or behind the closing launches, where a status other than RUNNING ends the call;
 *     check_every = 0       ceil(max_iterations / restart) cycles are enqueued and nothing is read back: the call is asynchronous,
 *                           allocates nothing and can be captured in a graph (one stream, no parallel branches);
 * with the same bits either way.
 * d_history: max_iterations + 1 values of T on the device, or NULL.  d_x and d_b may have any alignment of T; they must not overlap.
 * The matrix arrays passed to a solve hold the pattern the handle was made from.  mspmv_gmres_state reads the state block back on
 * `stream` and waits for it (rows == 0: host only).  debug_sync prints one line per launch (gmres_*_kernel, and the lines of the
 * products and the sweeps) and waits for each.
 * LIMITS, refused before anything is launched or allocated: create -- a NULL `solver`; rows, nnz < 0; rows + nnz > 2^31 - 65537; rows
 * > 2^30; nnz > 0 with rows == 0; value_bytes not 4 or 8; an unknown kind; restart < 1 or > MSPMV_GMRES_MAX_RESTART; NULL
 * d_row_offsets with rows > 0, NULL d_column_indices with nnz > 0.  set_factor -- a NULL handle or plan; a handle of another kind; a
 * plan whose rows (mspmv_csrsv_plan_info) differ from the handle's or whose bad_diagonal_row >= 0; NULL factor arrays with nnz > 0.
 * solve -- a NULL handle or one of the other value type; rtol or atol negative or NaN; max_iterations < 0; check_every < 0; FACTOR
 * without set_factor; JACOBI on a bad diagonal; NULL d_b, d_x or matrix arrays with rows > 0.  rows == 0 touches no device: create
 * gives a valid handle, a solve returns CONVERGED (start) at 0 iterations.  Every function returns 0 or a hipError_t, as mspmv.h's
 * do. ---- */
#ifndef MSPMV_GMRES_H
#define MSPMV_GMRES_H

#include "mspmv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSPMV_GMRES_NONE 0
#define MSPMV_GMRES_JACOBI 1
#define MSPMV_GMRES_FACTOR 2
#define MSPMV_GMRES_MAX_RESTART 128
/* status: MSPMV_PCG_RUNNING, MSPMV_PCG_CONVERGED, MSPMV_PCG_BREAKDOWN of mspmv.h */
#define MSPMV_GMRES_EXIT_NONE 0     /* still RUNNING: the slots of max_iterations are used up       */
#define MSPMV_GMRES_EXIT_START 1    /* CONVERGED before the first cycle                             */
#define MSPMV_GMRES_EXIT_RR 2       /* CONVERGED by the true residual of a closing                  */
#define MSPMV_GMRES_EXIT_BETA 3     /* BREAKDOWN: a cycle's starting residual is zero, Inf or NaN   */
#define MSPMV_GMRES_EXIT_D 4        /* BREAKDOWN: a column's d is zero, Inf or NaN                  */
typedef struct mspmv_gmres mspmv_gmres_t;
typedef struct mspmv_gmres_state {
    int32_t status;                  /* MSPMV_PCG_RUNNING (also: ended at max_iterations), _CONVERGED, _BREAKDOWN */
    int32_t iterations;              /* columns that entered the history                                           */
    int32_t slots;                   /* iteration slots taken by the cycles opened so far                          */
    int32_t cycles;                  /* cycles opened                                                              */
    int32_t restart;
    int32_t launches_per_iteration;  /* the solver's own, beside the product and the sweeps: 7                     */
    int32_t launches_per_cycle;      /* the solver's own, beside the product and the sweeps: 5, FACTOR 6           */
    int32_t precond_kind;
    int32_t bad_diagonal_row;        /* JACOBI: smallest row with no or more than one stored diagonal; -1          */
    int32_t exit_test;               /* MSPMV_GMRES_EXIT_*: the test that ended the solve                          */
    double rr, bb, stop2, beta;      /* the values of T, widened; beta: the last cycle's                           */
    uint64_t device_bytes;           /* what the handle holds on the device                                        */
} mspmv_gmres_state_t;
int mspmv_gmres_create(mspmv_gmres_t **solver, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                       int32_t value_bytes, int32_t precond_kind, int32_t restart, mspmv_stream_t stream, int debug_sync);
int mspmv_gmres_set_factor(mspmv_gmres_t *solver, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan,
                           const void *d_factor_values, const int32_t *d_row_offsets, const int32_t *d_column_indices);
int mspmv_gmres_solve_f32(mspmv_gmres_t *solver, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const float *d_b, float *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                          int32_t check_every, float *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream,
                          int debug_sync);
int mspmv_gmres_solve_f64(mspmv_gmres_t *solver, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const double *d_b, double *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                          int32_t check_every, double *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream,
                          int debug_sync);
int mspmv_gmres_state(mspmv_gmres_t *solver, mspmv_gmres_state_t *state, mspmv_stream_t stream);
int mspmv_gmres_destroy(mspmv_gmres_t *solver);

#ifdef __cplusplus
}
#endif
#endif /* MSPMV_GMRES_H */
