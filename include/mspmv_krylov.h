/* mspmv_krylov.h -- Krylov solvers built ON TOP of the C ABI of mspmv.h (libmspmv_krylov.so; plain C99).
 *
 * The layer calls only what libmspmv.so exports -- mspmv_csrmv_prepare, mspmv_csrmv_prepared_*, mspmv_csrsv_solve_*,
 * mspmv_csrsv_plan_info -- and is linked against the libmspmv.so next to it.  mspmv.h itself holds conjugate gradients
 * (mspmv_pcg_*), which need a symmetric positive definite matrix; what is here serves the NONSYMMETRIC case, for which
 * mspmv_csrilu0_* makes the factor.  GMRES(m) is mspmv_gmres.h.
 *
 * ---- RIGHT-PRECONDITIONED BiCGStab on the device (csrc/mspmv_bicgstab.hip): A x = b for a square A in CSR, as one call.  The
 * scalars of the iteration live in a state block on the device, every dot is the deterministic reduction R of mspmv.h
 * (mspmv_vec_dot_*), and the host reads nothing inside the loop unless asked to.
 * THE HANDLE is opaque and OWNS ITS STORAGE, as mspmv_pcg_t does.  mspmv_bicgstab_create ALLOCATES (one hipMalloc: the vectors p, v,
 * r, rh, t, for JACOBI and FACTOR one more for M^-1 p and M^-1 s, for FACTOR mid, the partials, the state block, the diagonal for
 * JACOBI, and the temp storage of mspmv_csrmv_prepared_* in the size its query states), runs mspmv_csrmv_prepare on d_row_offsets,
 * for JACOBI finds every row's diagonal entry (one lane per row) and reads state.bad_diagonal_row back; it is SYNCHRONOUS.  It
 * depends on the pattern alone: new values need no new handle.
 * PRECONDITIONER M, chosen at creation and applied from the right (A M^-1 y = b, x = M^-1 y; the residual is that of A x = b):
 *     MSPMV_BICGSTAB_NONE     M^-1 p = p (an alias: nothing is copied)
 *     MSPMV_BICGSTAB_JACOBI   (M^-1 p)[i] = p[i] / d[i], d[i] the stored diagonal entry of row i of d_values, taken once per solve.  A
 *                             pattern with a row of no or of more than one diagonal entry (state.bad_diagonal_row >= 0) is refused by
 *                             the solve.
 *     MSPMV_BICGSTAB_FACTOR   M^-1 p = second^-1 (first^-1 p): mspmv_csrsv_solve_* with first_plan into mid, then with second_plan,
 *                             alpha = 1, both on d_factor_values with ITS pattern arrays (mspmv_bicgstab_set_factor; none of them is
 *                             copied or owned: they live as long as solves use them).  ILU(0): first = LOWER + UNIT, second = UPPER +
 *                             NON_UNIT on the factor of mspmv_csrilu0_*.
 * ARITHMETIC, all in the value type T, every operation rounded on its own (no fused multiply-add), nothing flushed to zero:
 *     x = +0.0, r = b            (use_x_as_guess: q = A x by mspmv_csrmv_prepared_*, r[i] = b[i] - q[i])
 *     bb = R(b o b);  rt = (T) rtol, at = (T) atol;  s0 = fl(fl(rt * rt) * bb), a2 = fl(at * at);  stop2 = s0 > a2 ? s0 : a2
 *     rr = R(r o r);  history[0] = rr;  iterations = 0;      rr <= stop2 and rr < +Inf  ->  CONVERGED (start)
 *     rh = r (the shadow residual, kept for the whole solve);  rho = rr;  p = r
 *     iteration k = 1, 2, ...:
 *         ph = M^-1 p;  v = A ph;  rv = R(rh o v);        not (|rv| > 0)  ->  BREAKDOWN (rv): nothing of this iteration is written,
 *                                                                             iterations stays k - 1
 *         alpha = rho / rv
 *         x[i] = x[i] + fl(alpha * ph[i]);  s[i] = r[i] - fl(alpha * v[i]);  ss = R(s o s)
 *         ss <= stop2 and ss < +Inf  ->  rr = ss, history[k] = ss, iterations = k, CONVERGED (half)
 *         sh = M^-1 s;  t = A sh;  ts = R(t o s);  tt = R(t o t)
 *         not (tt > 0)  ->  rr = ss, history[k] = ss, iterations = k, BREAKDOWN (tt)      (x keeps the half step: s is its residual)
 *         omega = ts / tt
 *         x[i] = x[i] + fl(omega * sh[i]);  r[i] = s[i] - fl(omega * t[i]);  rr = R(r o r);  rho' = R(rh o r)
 *         history[k] = rr;  iterations = k;     rr <= stop2 and rr < +Inf  ->  CONVERGED (rr);     rr is NaN  ->  BREAKDOWN (rr-nan)
 *         not (|omega| > 0)  ->  BREAKDOWN (omega);     not (|rho'| > 0)  ->  BREAKDOWN (rho)       (tested in this order)
 *         beta = fl(fl(rho' / rho) * fl(alpha / omega));  rho = rho'
 *         p[i] = r[i] + fl(beta * fl(p[i] - fl(omega * v[i])))
 * (stop2 with a NaN s0 is a2.  An infinite residual never converges, whatever stop2 is.  A NaN fails every test written as
 * "not (... > 0)", so a NaN rv, tt, omega or rho' is a BREAKDOWN.)  The state keeps rho, alpha and omega as the solve leaves them: a
 * test that ends the solve comes before the assignment behind it.  A solve that ends at max_iterations leaves the status RUNNING and
 * exit_test 0.  x, iterations, the status, exit_test and the history are functions of the inputs alone -- not of check_every, the
 * grid or the alignment of b and x.  tests/bicgstab_model.py is this restatement in numpy.
 * LAUNCHES: beside the two products and (FACTOR) the four sweeps, an iteration launches state.launches_per_iteration = 9 kernels of
 * the solver's own, for every kind: the chunk sums of rh o v; a one-workgroup step that folds them, tests rv and makes alpha; the x
 * and s updates fused with the chunk sums of s o s (JACOBI: and sh = s / d); the step of the half-step test; the chunk sums of t o s
 * and t o t in one pass over t; the step that folds them, tests tt and makes omega; the x and r updates fused with the chunk sums of
 * r o r and rh o r; the step that folds them, writes the history, tests and makes beta; the p update (JACOBI: and ph = p / d).  s
 * lives in r's array.  All launches go on one stream, ordered by the kernel boundary alone; no workgroup waits on another; there are
 * no floating-point atomics.
 * THE FREEZE: once the status is not RUNNING, every later kernel of the solver's own reads the status and returns: x, the state and
 * the history entries beyond `iterations` stay as they are (the products and the sweeps still run, on scratch).  Hence
 *     check_every = c > 0   iterations are enqueued c at a time; after each group the state block is read back (one small copy, one
 *                           synchronisation) and the call returns at a status other than RUNNING or at max_iterations;
 *     check_every = 0       max_iterations iterations are enqueued and nothing is read back: the call is asynchronous, allocates
 *                           nothing and can be captured in a graph (one stream, no parallel branches);
 * with the same x, iterations, status, exit_test and history either way.
 * d_history: max_iterations + 1 values of T on the device, or NULL.  d_x and d_b may have any alignment of T; they must not overlap.
 * The matrix arrays passed to a solve hold the pattern the handle was made from.  mspmv_bicgstab_state reads the state block back on
 * `stream` and waits for it (rows == 0: host only).  debug_sync prints one line per launch (bicgstab_*_kernel, and the lines of the
 * products and the sweeps) and waits for each.
 * LIMITS, refused before anything is launched or allocated: create -- a NULL `solver`; rows, nnz < 0; rows + nnz > 2^31 - 65537; rows
 * > 2^30; nnz > 0 with rows == 0; value_bytes not 4 or 8; an unknown kind; NULL d_row_offsets with rows > 0, NULL d_column_indices
 * with nnz > 0.  set_factor -- a NULL handle or plan; a handle of another kind; a plan whose rows (mspmv_csrsv_plan_info) differ from
 * the handle's or whose bad_diagonal_row >= 0; NULL factor arrays with nnz > 0.  solve -- a NULL handle or one of the other value
 * type; rtol or atol negative or NaN; max_iterations < 0; check_every < 0; FACTOR without set_factor; JACOBI on a bad diagonal; NULL
 * d_b, d_x or matrix arrays with rows > 0.  rows == 0 touches no device: create gives a valid handle, a solve returns CONVERGED
 * (start) at 0 iterations.  Every function returns 0 or a hipError_t, as mspmv.h's do. ---- */
#ifndef MSPMV_KRYLOV_H
#define MSPMV_KRYLOV_H

#include "mspmv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSPMV_BICGSTAB_NONE 0
#define MSPMV_BICGSTAB_JACOBI 1
#define MSPMV_BICGSTAB_FACTOR 2
/* status: MSPMV_PCG_RUNNING, MSPMV_PCG_CONVERGED, MSPMV_PCG_BREAKDOWN of mspmv.h */
#define MSPMV_BICGSTAB_EXIT_NONE 0     /* still RUNNING: max_iterations                   */
#define MSPMV_BICGSTAB_EXIT_START 1    /* CONVERGED before the first iteration            */
#define MSPMV_BICGSTAB_EXIT_HALF 2     /* CONVERGED by ss, after the first half step      */
#define MSPMV_BICGSTAB_EXIT_RR 3       /* CONVERGED by rr                                 */
#define MSPMV_BICGSTAB_EXIT_RV 4       /* BREAKDOWN: rh . v is zero or NaN                */
#define MSPMV_BICGSTAB_EXIT_TT 5       /* BREAKDOWN: t . t is zero or NaN                 */
#define MSPMV_BICGSTAB_EXIT_RR_NAN 6   /* BREAKDOWN: rr is NaN                            */
#define MSPMV_BICGSTAB_EXIT_OMEGA 7    /* BREAKDOWN: omega is zero or NaN                 */
#define MSPMV_BICGSTAB_EXIT_RHO 8      /* BREAKDOWN: rh . r is zero or NaN                */
typedef struct mspmv_bicgstab mspmv_bicgstab_t;
typedef struct mspmv_bicgstab_state {
    int32_t status;                  /* MSPMV_PCG_RUNNING (also: ended at max_iterations), _CONVERGED, _BREAKDOWN */
    int32_t iterations;              /* iterations whose residual entered the history                              */
    int32_t launches_per_iteration;  /* the solver's own, beside the products and the sweeps: 9                    */
    int32_t precond_kind;
    int32_t bad_diagonal_row;        /* JACOBI: smallest row with no or more than one stored diagonal; -1          */
    int32_t exit_test;               /* MSPMV_BICGSTAB_EXIT_*: the test that ended the solve                       */
    double rr, bb, stop2, rho, alpha, omega;   /* the values of T, widened                                         */
    uint64_t device_bytes;           /* what the handle holds on the device                                        */
} mspmv_bicgstab_state_t;
int mspmv_bicgstab_create(mspmv_bicgstab_t **solver, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows,
                          int32_t nnz, int32_t value_bytes, int32_t precond_kind, mspmv_stream_t stream, int debug_sync);
int mspmv_bicgstab_set_factor(mspmv_bicgstab_t *solver, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan,
                              const void *d_factor_values, const int32_t *d_row_offsets, const int32_t *d_column_indices);
int mspmv_bicgstab_solve_f32(mspmv_bicgstab_t *solver, const float *d_values, const int32_t *d_row_offsets,
                             const int32_t *d_column_indices, const float *d_b, float *d_x, int32_t use_x_as_guess, double rtol,
                             double atol, int32_t max_iterations, int32_t check_every,
                             float *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream, int debug_sync);
int mspmv_bicgstab_solve_f64(mspmv_bicgstab_t *solver, const double *d_values, const int32_t *d_row_offsets,
                             const int32_t *d_column_indices, const double *d_b, double *d_x, int32_t use_x_as_guess, double rtol,
                             double atol, int32_t max_iterations, int32_t check_every,
                             double *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream, int debug_sync);
int mspmv_bicgstab_state(mspmv_bicgstab_t *solver, mspmv_bicgstab_state_t *state, mspmv_stream_t stream);
int mspmv_bicgstab_destroy(mspmv_bicgstab_t *solver);

#ifdef __cplusplus
}
#endif
#endif /* MSPMV_KRYLOV_H */
