// mspmv_krylov_op.hpp -- what the Krylov solvers (mspmv_pcg.hip, mspmv_bicgstab.hip, mspmv_gmres.hip) share: what a solver knows about
// A and M^-1, and nothing about any recurrence.  The operator (the prepared product, the preconditioner of one of three kinds), its
// refusals, its part of the one allocation a solver carves its arrays from, the read-back of a state block and the loop over groups of
// check_every iterations.  Every call into the library goes through what include/mspmv.h declares, so the layers built on the C ABI
// include this as mspmv_pcg.hip does.  Each solver keeps its own kernels, state block, Run and field-by-field state; GMRES its loop.
#pragma once
#include <new>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"     // lv_launched
#include "mspmv_vec.hpp"

namespace mspmv {
namespace {

enum { KRYLOV_NONE = 0, KRYLOV_JACOBI = 1, KRYLOV_FACTOR = 2 };     // every solver's three kinds (each file asserts its own against them)

struct KrylovOp {
    int32_t rows = 0, nnz = 0, value_bytes = 0, kind = 0, bad_diagonal_row = -1;
    long long m = 0;                                                // level-1 partials of a dot
    void *mv_temp = nullptr;                                        // the prepared product
    size_t mv_bytes = 0;
    void *mid = nullptr, *diag = nullptr;                           // FACTOR: between the two sweeps;  JACOBI: d
    int *dpos = nullptr;                                            // JACOBI: where each row's diagonal entry is
    mspmv_csrsv_plan_t *first = nullptr, *second = nullptr;         // FACTOR: the two sweeps (not owned)
    const void *f_vals = nullptr;
    const int32_t *f_off = nullptr, *f_cols = nullptr;
};

// one lane per row: where the row's diagonal entry is; the smallest row with none or more than one goes to *bad (all ones: none)
__global__ __launch_bounds__(256) void krylov_diag_kernel(const int *__restrict__ off, const int *__restrict__ cols, int rows, int *__restrict__ dpos,
                                                          unsigned *__restrict__ bad)
{
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= rows) return;
    const int r = (int) t;
    int at = 0, count = 0;
    for (int e = off[r]; e < off[r + 1]; ++e)
        if (cols[e] == r) { at = e; ++count; }
    dpos[r] = at;
    if (count != 1) atomicMin(bad, (unsigned) r);
}

// out = A in
template <typename T>
int krylov_product(const KrylovOp &op, const T *vals, const int32_t *off, const int32_t *cols, const T *in, T *out, hipStream_t stream, int dbg)
{
    size_t bytes = op.mv_bytes;
    const mspmv_stream_t s = reinterpret_cast<mspmv_stream_t>(stream);
    if constexpr (sizeof(T) == 4) return mspmv_csrmv_prepared_f32(op.mv_temp, &bytes, vals, off, cols, in, out, op.rows, op.rows, op.nnz, 1.0f, 0.0f, s, dbg);
    else return mspmv_csrmv_prepared_f64(op.mv_temp, &bytes, vals, off, cols, in, out, op.rows, op.rows, op.nnz, 1.0, 0.0, s, dbg);
}

// FACTOR: out = second^-1 (first^-1 in)
template <typename T>
int krylov_sweeps(const KrylovOp &op, const T *in, T *out, hipStream_t stream, int dbg)
{
    const mspmv_stream_t s = reinterpret_cast<mspmv_stream_t>(stream);
    const T *fv = static_cast<const T *>(op.f_vals);
    T *mid = static_cast<T *>(op.mid);
    if constexpr (sizeof(T) == 4) {
        if (int e = mspmv_csrsv_solve_f32(op.first, fv, op.f_off, op.f_cols, 1.0f, in, mid, s, dbg)) return e;
        return mspmv_csrsv_solve_f32(op.second, fv, op.f_off, op.f_cols, 1.0f, mid, out, s, dbg);
    } else {
        if (int e = mspmv_csrsv_solve_f64(op.first, fv, op.f_off, op.f_cols, 1.0, in, mid, s, dbg)) return e;
        return mspmv_csrsv_solve_f64(op.second, fv, op.f_off, op.f_cols, 1.0, mid, out, s, dbg);
    }
}

// the refusals of *_create, before anything is touched
static int krylov_refuse_create(const int32_t *off, const int32_t *cols, int32_t rows, int32_t nnz, int32_t value_bytes, int32_t kind)
{
    if (rows < 0 || nnz < 0 || (long long) rows + nnz > MAX_ITEMS || rows > VEC_MAX_N) return hipErrorInvalidValue;
    if ((value_bytes != 4 && value_bytes != 8) || kind < KRYLOV_NONE || kind > KRYLOV_FACTOR) return hipErrorInvalidValue;
    if (nnz > 0 && rows == 0) return hipErrorInvalidValue;
    if (rows > 0 && (!off || (nnz > 0 && !cols))) return hipErrorInvalidValue;
    return hipSuccess;
}

template <typename Solver>
int krylov_destroy(Solver *solver)
{
    if (!solver) return hipErrorInvalidValue;
    if (solver->base) (void) hipFree(solver->base);
    delete solver;
    return hipSuccess;
}

// *_create once nothing is refused: the solver with its operator described; build(solver) adds what is the solver's own to h_state and,
// where there are rows, makes the device part
template <typename Solver, typename Build>
int krylov_create(Solver **out, int32_t rows, int32_t nnz, int32_t value_bytes, int32_t kind, Build build)
{
    Solver *h = new (std::nothrow) Solver;
    if (!h) return hipErrorOutOfMemory;
    h->op.rows = rows; h->op.nnz = nnz; h->op.value_bytes = value_bytes; h->op.kind = kind;
    h->op.m = vec_partials(rows);
    h->h_state.precond_kind = kind;
    if (int e = build(*h)) {
        (void) hipGetLastError();
        (void) krylov_destroy(h);
        return e;
    }
    h->h_state.bad_diagonal_row = h->op.bad_diagonal_row;             // (-1 where nothing was built)
    *out = h;
    return hipSuccess;
}

// *_set_factor (op: NULL for no solver)
static int krylov_set_factor(KrylovOp *op, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan, const void *d_factor_values,
                             const int32_t *d_row_offsets, const int32_t *d_column_indices)
{
    if (!op || op->kind != KRYLOV_FACTOR || !first_plan || !second_plan) return hipErrorInvalidValue;
    for (const mspmv_csrsv_plan_t *plan : {first_plan, second_plan}) {
        mspmv_csrsv_info_t info;
        if (int e = mspmv_csrsv_plan_info(plan, &info)) return e;
        if (info.rows != op->rows || info.bad_diagonal_row >= 0) return hipErrorInvalidValue;
        if (info.nnz > 0 && (!d_factor_values || !d_row_offsets || !d_column_indices)) return hipErrorInvalidValue;
    }
    op->first = first_plan; op->second = second_plan;
    op->f_vals = d_factor_values; op->f_off = d_row_offsets; op->f_cols = d_column_indices;
    return hipSuccess;
}

// the refusals of *_solve (op: NULL for no solver); what the stopping test compares with: rtol^2 and atol^2, squared in T
template <typename T>
int krylov_refuse_solve(const KrylovOp *op, const T *vals, const int32_t *off, const int32_t *cols, const T *b, const T *x, double rtol, double atol,
                        int32_t max_iterations, int32_t check_every, T &rtol2, T &atol2)
{
    if (!op || op->value_bytes != (int32_t) sizeof(T)) return hipErrorInvalidValue;
    if (!(rtol >= 0) || !(atol >= 0) || max_iterations < 0 || check_every < 0) return hipErrorInvalidValue;       // (a NaN fails both)
    if (op->kind == KRYLOV_FACTOR && !op->first) return hipErrorInvalidValue;
    if (op->kind == KRYLOV_JACOBI && op->bad_diagonal_row >= 0) return hipErrorInvalidValue;
    if (op->rows > 0 && (!b || !x || !off || (op->nnz > 0 && (!vals || !cols)))) return hipErrorInvalidValue;
    const T rt = (T) rtol, at = (T) atol;
    rtol2 = rt * rt; atol2 = at * at;
    return hipSuccess;
}

// The carve of a solver's one allocation: offsets only, plain integer arithmetic.  A solver takes its state block first (256 bytes
// at offset 0; the diagonal probe's flag is its byte 128), then its own arrays in its own order, with precond() behind its vectors and
// product() last: device_bytes is pinned by tests/test_krylov_device_bytes.py, so the order and every size are part of the contract.
struct KrylovCarve {
    uint64_t size = 0, mid = 0, diag = 0, dpos = 0, mv = 0;
    uint64_t take(uint64_t bytes) { const uint64_t at = size; size += bytes; return at; }
    void precond(const KrylovOp &op, uint64_t vec)                  // vec: the bytes of one vector
    {
        mid = take(op.kind == KRYLOV_FACTOR ? vec : 0);
        diag = take(op.kind == KRYLOV_JACOBI ? vec : 0);
        dpos = take(op.kind == KRYLOV_JACOBI ? align256((uint64_t) op.rows * 4) : 0);
    }
    void product(const KrylovOp &op) { mv = take(align256(op.mv_bytes)); }
};

// before the carve: the size of the prepared product
static int krylov_query(KrylovOp &op) { return mspmv_csrmv_prepare(nullptr, &op.mv_bytes, nullptr, op.rows, op.nnz, op.value_bytes, nullptr, 0); }

// after it: the allocation, the operator's arrays, the state block zeroed, the product prepared, JACOBI: the diagonal located; synchronous
static int krylov_build(KrylovOp &op, char *&base, const KrylovCarve &c, const int32_t *off, const int32_t *cols, hipStream_t stream, int dbg)
{
    if (hipMalloc(reinterpret_cast<void **>(&base), c.size) != hipSuccess) return hipErrorOutOfMemory;
    const bool jacobi = op.kind == KRYLOV_JACOBI;
    op.mid = op.kind == KRYLOV_FACTOR ? base + c.mid : nullptr;
    op.diag = jacobi ? base + c.diag : nullptr;
    op.dpos = jacobi ? reinterpret_cast<int *>(base + c.dpos) : nullptr;
    op.mv_temp = base + c.mv;
    if (hipMemsetAsync(base, 0, 256, stream) != hipSuccess) return hipErrorInvalidValue;
    size_t bytes = op.mv_bytes;
    if (int e = mspmv_csrmv_prepare(op.mv_temp, &bytes, off, op.rows, op.nnz, op.value_bytes, reinterpret_cast<mspmv_stream_t>(stream), dbg)) return e;
    if (jacobi) {
        unsigned *bad = reinterpret_cast<unsigned *>(base + 128);
        if (hipMemsetAsync(bad, 0xff, 4, stream) != hipSuccess) return hipErrorInvalidValue;
        const unsigned grid = grid_for(op.rows, 256);
        hipLaunchKernelGGL(krylov_diag_kernel, dim3(grid), dim3(256), 0, stream, off, cols, (int) op.rows, op.dpos, bad);
        if (int e = lv_launched(stream, dbg, "krylov_diag_kernel", grid, 256)) return e;
        if (hipMemcpyAsync(&op.bad_diagonal_row, bad, 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return hipErrorInvalidValue;
    }
    return (int) hipStreamSynchronize(stream);
}

// the state block of the device, read back; synchronises
template <typename Dev>
int krylov_read(const void *state, Dev &d, hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(&d, state, sizeof(d), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return (int) e;
}

// max_iterations iterations in groups of check_every, the status read between two groups (check_every == 0: one group, nothing read)
template <typename Dev, typename Run>
int krylov_groups(const Run &run, int max_iterations, int check_every)
{
    for (int done = 0; done < max_iterations;) {
        const int group = check_every > 0 ? std::min(check_every, max_iterations - done) : max_iterations - done;
        for (int i = 0; i < group; ++i)
            if (int e = run.iteration()) return e;
        done += group;
        if (check_every > 0) {
            Dev now;
            if (int e = krylov_read(run.h->state, now, run.stream)) return e;
            if (now.status != MSPMV_PCG_RUNNING) break;
        }
    }
    return hipSuccess;
}

}  // namespace
}  // namespace mspmv
