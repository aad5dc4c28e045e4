// mspmv_pcg.hip -- preconditioned conjugate gradients on the device (mspmv_pcg_* of include/mspmv.h, which states the arithmetic).
//
// What one iteration launches, on one stream, ordered by the kernel boundary alone:
//     mspmv_csrmv_prepared_*          q = A p
//     pcg_dot_kernel                  the chunk sums of p.q                                          (one workgroup per 1024 elements)
//     pcg_step_kernel  PQ             folds them: pq, the breakdown test, alpha                      (ONE workgroup)
//     pcg_update_kernel               x += alpha p,  r -= alpha q,  the chunk sums of r.r;  JACOBI: z = r / d and the chunk sums of r.z
//     pcg_step_kernel  RR             folds: rr, history, iterations, the stopping tests;  NONE / JACOBI: rz', beta
//     FACTOR only:  two mspmv_csrsv_solve_* sweeps (z = second^-1 first^-1 r),  pcg_dot_kernel (r.z),  pcg_step_kernel RZ (rz', beta)
//     pcg_p_kernel                    p = z + beta p
// so the solver adds 5 launches per iteration (FACTOR: 7) to the product and the sweeps.  alpha, beta, rz, pq, rr, the status and the
// iteration counter live in a state block on the device (PcgDev); the host reads it only between groups of check_every iterations,
// and with check_every == 0 never.  THE FREEZE: every kernel here but the two that start a solve reads the status first and returns
// unless it is RUNNING, so iterations enqueued past the end change neither x nor the state nor the history.
// The dots are the defined reduction of mspmv_vec.hpp: chunk sums where the products are made, the fold in the one-workgroup step.
// What the solver knows about A and M^-1 (the product, the sweeps, the refusals, the operator's part of the carve) is
// mspmv_krylov_op.hpp, shared with BiCGStab and GMRES; the recurrence, its kernels and the state block are here.
#include <hip/hip_runtime.h>

#include "mspmv_krylov_op.hpp"

#pragma clang fp contract(off)

template <typename T>
struct PcgDev {                                                     // the state block on the device
    T alpha, beta, rz, pq, rr, bb, stop2, spare;
    int status, iterations, spare2[2];
};

struct mspmv_pcg {
    mspmv::KrylovOp op;                                             // A and M^-1
    char *base = nullptr;                                           // the one allocation the arrays below (and op's) are carved from
    void *q = nullptr, *z = nullptr, *p = nullptr, *r = nullptr, *part[3] = {}, *state = nullptr;
    mspmv_pcg_state_t h_state{};                                    // rows == 0: what a solve leaves (no device)
};

namespace {

using namespace mspmv;

static_assert(MSPMV_PCG_NONE == KRYLOV_NONE && MSPMV_PCG_JACOBI == KRYLOV_JACOBI && MSPMV_PCG_FACTOR == KRYLOV_FACTOR, "the kinds of mspmv_krylov_op.hpp");

enum { PCG_START = 0, PCG_PQ = 1, PCG_RR = 2, PCG_RZ = 3, PCG_RZ_FIRST = 4 };

static int pcg_launches_per_iteration(int kind) { return kind == MSPMV_PCG_FACTOR ? 7 : 5; }

// the start of a solve: r = b - q (q = A x for a guess; NULL: x = +0, r = b), the chunk sums of b.b and r.r; JACOBI: d, z = r / d, r.z
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void pcg_init_kernel(const T *__restrict__ b, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                             T *__restrict__ z, T *__restrict__ diag, const T *__restrict__ vals,
                                                             const int *__restrict__ dpos, long long n, T *__restrict__ part_bb,
                                                             T *__restrict__ part_rr, T *__restrict__ part_rz)
{
    __shared__ T s_w[4];
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vb[4], vr[4], s[4];
    vec_load4(b, i, n, vec_aligned16(b), vb);
    if (q) {
        T vq[4];
        vec_load4(q, i, n, true, vq);
#pragma unroll
        for (int j = 0; j < 4; ++j) vr[j] = vb[j] - vq[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { vr[j] = vb[j]; s[j] = (T) 0; }
        vec_store4(x, i, n, vec_aligned16(x), s);
    }
    vec_store4(r, i, n, true, vr);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vb[j] * vb[j];
    const T bb = vec_chunk_sum(s, s_w);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vr[j] * vr[j];
    const T rr = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) { part_bb[blockIdx.x] = bb; part_rr[blockIdx.x] = rr; }
    if (KIND == MSPMV_PCG_JACOBI) {
        T vd[4], vz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool have = i + j < n;
            vd[j] = have ? vals[dpos[i + j]] : (T) 0;
            vz[j] = have ? vr[j] / vd[j] : (T) 0;
            s[j] = vr[j] * vz[j];
        }
        vec_store4(diag, i, n, true, vd);
        vec_store4(z, i, n, true, vz);
        const T rz = vec_chunk_sum(s, s_w);
        if (threadIdx.x == 0) part_rz[blockIdx.x] = rz;
    }
}

// the chunk sums of a.b (p.q; FACTOR: r.z)
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void pcg_dot_kernel(const PcgDev<T> *__restrict__ st, const T *__restrict__ a, const T *__restrict__ b, long long n,
                                                            T *__restrict__ part)
{
    __shared__ T s_w[4];
    if (st->status != MSPMV_PCG_RUNNING) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T va[4], vb[4], s[4];
    vec_load4(a, i, n, true, va);
    vec_load4(b, i, n, true, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = va[j] * vb[j];
    const T sum = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// x[i] = x[i] + fl(alpha p[i]),  r[i] = r[i] - fl(alpha q[i]),  the chunk sums of r.r;  JACOBI: z[i] = r[i] / d[i] and those of r.z
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void pcg_update_kernel(const PcgDev<T> *__restrict__ st, const T *__restrict__ p, const T *__restrict__ q,
                                                               T *__restrict__ x, T *__restrict__ r, T *__restrict__ z, const T *__restrict__ diag,
                                                               long long n, T *__restrict__ part_rr, T *__restrict__ part_rz)
{
    __shared__ T s_w[4];
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T alpha = st->alpha;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    const bool x_aligned = vec_aligned16(x);
    T vp[4], vq[4], vx[4], vr[4], s[4];
    vec_load4(p, i, n, true, vp);
    vec_load4(q, i, n, true, vq);
    vec_load4(x, i, n, x_aligned, vx);
    vec_load4(r, i, n, true, vr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T ap = alpha * vp[j], aq = alpha * vq[j];
        vx[j] = vx[j] + ap;
        vr[j] = i + j < n ? vr[j] - aq : (T) 0;
        s[j] = vr[j] * vr[j];
    }
    vec_store4(x, i, n, x_aligned, vx);
    vec_store4(r, i, n, true, vr);
    const T rr = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = rr;
    if (KIND == MSPMV_PCG_JACOBI) {
        T vd[4], vz[4];
        vec_load4(diag, i, n, true, vd);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vz[j] = i + j < n ? vr[j] / vd[j] : (T) 0;
            s[j] = vr[j] * vz[j];
        }
        vec_store4(z, i, n, true, vz);
        const T rz = vec_chunk_sum(s, s_w);
        if (threadIdx.x == 0) part_rz[blockIdx.x] = rz;
    }
}

// p = z (first) or p[i] = z[i] + fl(beta p[i])
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void pcg_p_kernel(const PcgDev<T> *__restrict__ st, const T *__restrict__ z, T *__restrict__ p, long long n, int first)
{
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T beta = st->beta;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vz[4], vp[4];
    vec_load4(z, i, n, true, vz);
    if (!first) {
        vec_load4(p, i, n, true, vp);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const T bp = beta * vp[j]; vz[j] = vz[j] + bp; }
    }
    vec_store4(p, i, n, true, vz);
}

// ONE workgroup: the folds and the scalar arithmetic, once.  Every thread reads the status before thread 0 can write it (the folds'
// barriers lie between), so the early return is taken by all threads or by none.
template <typename T>
__global__ __launch_bounds__(VEC_FOLD_BLOCK) void pcg_step_kernel(PcgDev<T> *st, const T *__restrict__ part0, const T *__restrict__ part1,
                                                                  const T *__restrict__ part2, long long m, int mode, int kind, T rtol2, T atol2,
                                                                  T *__restrict__ history)
{
    __shared__ T s_p[VEC_CHUNK];
    __shared__ T s_w[16];
    const bool lead = threadIdx.x == 0;
    if (mode == PCG_START) {
        const T bb = vec_fold(part0, m, s_p, s_w), rr = vec_fold(part1, m, s_p, s_w);
        T rz = rr;                                                   // NONE: z is r, the same products in the same tree
        if (kind == MSPMV_PCG_JACOBI) rz = vec_fold(part2, m, s_p, s_w);
        if (lead) {
            const T scaled = rtol2 * bb, stop2 = scaled > atol2 ? scaled : atol2;
            st->alpha = 0; st->beta = 0; st->pq = 0; st->spare = 0;
            st->bb = bb; st->rr = rr; st->rz = rz; st->stop2 = stop2;
            st->iterations = 0;
            st->status = rr <= stop2 && rr < (T) INFINITY ? MSPMV_PCG_CONVERGED : MSPMV_PCG_RUNNING;       // (never on an infinite residual)
            if (history) history[0] = rr;
        }
        return;
    }
    if (st->status != MSPMV_PCG_RUNNING) return;
    if (mode == PCG_PQ) {
        const T pq = vec_fold(part0, m, s_p, s_w);
        if (lead) {
            st->pq = pq;
            if (!(pq > (T) 0)) st->status = MSPMV_PCG_BREAKDOWN;
            else st->alpha = st->rz / pq;
        }
        return;
    }
    T rr = 0, rz2 = 0;
    if (mode == PCG_RR) {
        rr = vec_fold(part0, m, s_p, s_w);
        rz2 = kind == MSPMV_PCG_JACOBI ? vec_fold(part1, m, s_p, s_w) : rr;
    } else {
        rz2 = vec_fold(part0, m, s_p, s_w);
    }
    if (!lead) return;
    bool next = mode != PCG_RR || kind != MSPMV_PCG_FACTOR;         // does this step hold rz'?
    if (mode == PCG_RR) {
        const int k = st->iterations + 1;
        st->rr = rr;
        st->iterations = k;
        if (history) history[k] = rr;
        if (rr <= st->stop2 && rr < (T) INFINITY) { st->status = MSPMV_PCG_CONVERGED; next = false; }
        else if (rr != rr) { st->status = MSPMV_PCG_BREAKDOWN; next = false; }
    }
    if (!next) return;
    if (mode == PCG_RZ_FIRST) { st->rz = rz2; return; }
    if (!(rz2 > (T) 0)) { st->status = MSPMV_PCG_BREAKDOWN; return; }
    st->beta = rz2 / st->rz;
    st->rz = rz2;
}

template <typename T>
struct PcgRun {
    mspmv_pcg *h;
    hipStream_t stream;
    int dbg;
    const T *vals;
    const int32_t *off, *cols;
    T *x;
    T rtol2, atol2;
    T *history;
    long long n;
    unsigned grid;

    T *arr(void *a) const { return static_cast<T *>(a); }
    PcgDev<T> *st() const { return static_cast<PcgDev<T> *>(h->state); }

    int product(const T *in, T *out) const { return krylov_product(h->op, vals, off, cols, in, out, stream, dbg); }
    int sweeps() const { return krylov_sweeps<T>(h->op, arr(h->r), arr(h->z), stream, dbg); }        // z = second^-1 (first^-1 r)
    int step(int mode) const
    {
        hipLaunchKernelGGL(pcg_step_kernel<T>, dim3(1), dim3(VEC_FOLD_BLOCK), 0, stream, st(), arr(h->part[0]), arr(h->part[1]), arr(h->part[2]), h->op.m,
                           mode, (int) h->op.kind, rtol2, atol2, history);
        return lv_launched(stream, dbg, "pcg_step_kernel", 1, VEC_FOLD_BLOCK);
    }
    int dot(const T *a, const T *b) const
    {
        hipLaunchKernelGGL(pcg_dot_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, st(), a, b, n, arr(h->part[0]));
        return lv_launched(stream, dbg, "pcg_dot_kernel", grid, VEC_BLOCK);
    }
    int new_p(int first) const
    {
        hipLaunchKernelGGL(pcg_p_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, st(), arr(h->z), arr(h->p), n, first);
        return lv_launched(stream, dbg, "pcg_p_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int init(const T *b, const T *q) const
    {
        hipLaunchKernelGGL((pcg_init_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, b, q, x, arr(h->r), arr(h->z), arr(h->op.diag), vals,
                           (const int *) h->op.dpos, n, arr(h->part[0]), arr(h->part[1]), arr(h->part[2]));
        return lv_launched(stream, dbg, "pcg_init_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int update() const
    {
        hipLaunchKernelGGL((pcg_update_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, (const PcgDev<T> *) st(), (const T *) arr(h->p),
                           (const T *) arr(h->q), x, arr(h->r), arr(h->z), (const T *) arr(h->op.diag), n, arr(h->part[0]), arr(h->part[1]));
        return lv_launched(stream, dbg, "pcg_update_kernel", grid, VEC_BLOCK);
    }

    int start(const T *b, int guess) const
    {
        const T *q = nullptr;
        if (guess) {
            if (int e = product(x, arr(h->q))) return e;
            q = arr(h->q);
        }
        if (int e = h->op.kind == MSPMV_PCG_JACOBI ? init<MSPMV_PCG_JACOBI>(b, q) : init<MSPMV_PCG_NONE>(b, q)) return e;
        if (int e = step(PCG_START)) return e;
        if (h->op.kind == MSPMV_PCG_FACTOR) {
            if (int e = sweeps()) return e;
            if (int e = dot(arr(h->r), arr(h->z))) return e;
            if (int e = step(PCG_RZ_FIRST)) return e;
        }
        return new_p(1);
    }
    int iteration() const
    {
        if (int e = product(arr(h->p), arr(h->q))) return e;
        if (int e = dot(arr(h->p), arr(h->q))) return e;
        if (int e = step(PCG_PQ)) return e;
        if (int e = h->op.kind == MSPMV_PCG_JACOBI ? update<MSPMV_PCG_JACOBI>() : update<MSPMV_PCG_NONE>()) return e;
        if (int e = step(PCG_RR)) return e;
        if (h->op.kind == MSPMV_PCG_FACTOR) {
            if (int e = sweeps()) return e;
            if (int e = dot(arr(h->r), arr(h->z))) return e;
            if (int e = step(PCG_RZ)) return e;
        }
        return new_p(0);
    }
};

template <typename T>
int pcg_read(const mspmv_pcg *h, mspmv_pcg_state_t *out, hipStream_t stream)
{
    PcgDev<T> d;
    if (int e = krylov_read(h->state, d, stream)) return e;
    out->status = d.status; out->iterations = d.iterations;
    out->rr = (double) d.rr; out->bb = (double) d.bb; out->stop2 = (double) d.stop2; out->rz = (double) d.rz;
    return hipSuccess;
}

template <typename T>
int pcg_solve(mspmv_pcg *h, const T *vals, const int32_t *off, const int32_t *cols, const T *b, T *x, int guess, double rtol, double atol,
              int32_t max_iterations, int32_t check_every, T *history, hipStream_t stream, int dbg)
{
    T rtol2, atol2;
    if (int e = krylov_refuse_solve(h ? &h->op : nullptr, vals, off, cols, b, x, rtol, atol, max_iterations, check_every, rtol2, atol2)) return e;
    if (h->op.rows == 0) {
        h->h_state.status = MSPMV_PCG_CONVERGED; h->h_state.iterations = 0;
        h->h_state.rr = 0; h->h_state.bb = 0; h->h_state.rz = 0; h->h_state.stop2 = (double) atol2;
        return hipSuccess;
    }
    const PcgRun<T> run{h, stream, dbg, vals, off, cols, x, rtol2, atol2, history, (long long) h->op.rows, (unsigned) h->op.m};
    if (int e = run.start(b, guess)) return e;
    return krylov_groups<PcgDev<T>>(run, max_iterations, check_every);
}

static int pcg_build(mspmv_pcg &h, const int32_t *off, const int32_t *cols, hipStream_t stream, int dbg)
{
    if (int e = krylov_query(h.op)) return e;
    const uint64_t vb = (uint64_t) h.op.value_bytes, vec = align256((uint64_t) h.op.rows * vb), part = align256((uint64_t) h.op.m * vb);
    const bool own_z = h.op.kind != MSPMV_PCG_NONE;                 // NONE: z is r
    KrylovCarve c;
    const uint64_t state_o = c.take(256), q_o = c.take(vec), p_o = c.take(vec), r_o = c.take(vec), z_o = c.take(own_z ? vec : 0);
    c.precond(h.op, vec);
    const uint64_t p0_o = c.take(part), p1_o = c.take(part), p2_o = c.take(part);
    c.product(h.op);
    if (int e = krylov_build(h.op, h.base, c, off, cols, stream, dbg)) return e;
    h.h_state.device_bytes = c.size;
    h.state = h.base + state_o; h.q = h.base + q_o; h.p = h.base + p_o; h.r = h.base + r_o;
    h.z = own_z ? h.base + z_o : h.r;
    h.part[0] = h.base + p0_o; h.part[1] = h.base + p1_o; h.part[2] = h.base + p2_o;
    return hipSuccess;
}

}  // namespace

extern "C" {

int mspmv_pcg_create(mspmv_pcg_t **pcg, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                     int32_t value_bytes, int32_t precond_kind, mspmv_stream_t stream, int debug_sync)
{
    if (!pcg) return hipErrorInvalidValue;
    *pcg = nullptr;
    if (int e = krylov_refuse_create(d_row_offsets, d_column_indices, rows, nnz, value_bytes, precond_kind)) return e;
    return krylov_create(pcg, rows, nnz, value_bytes, precond_kind, [&](mspmv_pcg &h) {
        h.h_state.launches_per_iteration = pcg_launches_per_iteration(precond_kind);
        return rows > 0 ? pcg_build(h, d_row_offsets, d_column_indices, reinterpret_cast<hipStream_t>(stream), debug_sync) : (int) hipSuccess;
    });
}

int mspmv_pcg_set_factor(mspmv_pcg_t *pcg, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan, const void *d_factor_values,
                         const int32_t *d_row_offsets, const int32_t *d_column_indices)
{
    return krylov_set_factor(pcg ? &pcg->op : nullptr, first_plan, second_plan, d_factor_values, d_row_offsets, d_column_indices);
}

int mspmv_pcg_solve_f32(mspmv_pcg_t *pcg, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices, const float *d_b,
                        float *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations, int32_t check_every,
                        float *d_history, mspmv_stream_t stream, int debug_sync)
{
    return pcg_solve<float>(pcg, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                            d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_pcg_solve_f64(mspmv_pcg_t *pcg, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices, const double *d_b,
                        double *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations, int32_t check_every,
                        double *d_history, mspmv_stream_t stream, int debug_sync)
{
    return pcg_solve<double>(pcg, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                             d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_pcg_state(mspmv_pcg_t *pcg, mspmv_pcg_state_t *state, mspmv_stream_t stream)
{
    if (!pcg || !state) return hipErrorInvalidValue;
    *state = pcg->h_state;
    if (pcg->op.rows == 0) return hipSuccess;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return pcg->op.value_bytes == 4 ? pcg_read<float>(pcg, state, s) : pcg_read<double>(pcg, state, s);
}

int mspmv_pcg_destroy(mspmv_pcg_t *pcg) { return krylov_destroy(pcg); }

}  // extern "C"
