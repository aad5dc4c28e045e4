// mspmv_gmres.hip -- right-preconditioned restarted GMRES(m) on the device (mspmv_gmres_* of include/mspmv_gmres.h, which states the
// arithmetic).  This file is libmspmv_gmres.so: a layer ON TOP of the C ABI, as mspmv_bicgstab.hip is.  The products and the sweeps
// are calls of what libmspmv.so exports (mspmv_csrmv_prepare, mspmv_csrmv_prepared_*, mspmv_csrsv_solve_*, mspmv_csrsv_plan_info);
// from the source tree it takes only header-only pieces: the deterministic vector layer (mspmv_vec.hpp), lv_launched
// (mspmv_levels.hpp) and what the three Krylov solvers know about A and M^-1 (mspmv_krylov_op.hpp: those calls, the refusals, the
// operator's part of the carve).  The loop over cycles and slots is this file's own.
//
// What inner slot j of a cycle launches, on one stream, ordered by the kernel boundary alone:
//     FACTOR: two mspmv_csrsv_solve_*     z = second^-1 first^-1 v_j     (NONE: z is v_j;  JACOBI: z = v_j / d was made with v_j)
//     mspmv_csrmv_prepared_*              w = A z
//  1  gmres_dots_kernel                   the chunk sums of v_i.w, i = 0 .. j: w's chunk in registers, one pass over the chunk's columns
//  2  gmres_step_kernel  H1               folds them: h1_i                                           (one workgroup per i)
//  3  gmres_orth_kernel  (dots)           w -= sum h1_i v_i in the stated order, then the chunk sums of v_i.w on the new w
//  4  gmres_step_kernel  H2               folds them: h2_i, h_i = h1_i + h2_i                         (one workgroup per i)
//  5  gmres_orth_kernel  (norm)           w -= sum h2_i v_i, the chunk sums of w.w
//  6  gmres_step_kernel  NORM             ONE workgroup: hn, the rotations, d, the tests, g, gg, the history, the counters, the flag
//  7  gmres_scale_kernel                  v_{j+1} = w / hn;  JACOBI: z = v_{j+1} / d
// and what a cycle adds (GMRES_CYCLE_LAUNCHES, + 1 for FACTOR):
//     gmres_scale_kernel                  v_0 = r / beta (r lives in w's array), before the cycle's first slot
//     gmres_step_kernel  SOLVE            the back substitution R y = g, thread 0
//     gmres_combine_kernel                u = V y;  NONE: x += u;  JACOBI: x += u / d;  FACTOR: u into w's array, two sweeps, gmres_xadd_kernel
//     mspmv_csrmv_prepared_*              q = A x (into w's array)
//     gmres_residual_kernel               r = b - q (in place), the chunk sums of r.r.  It also starts a solve (there: b.b too)
//     gmres_step_kernel  END              folds rr, the tests, history[iterations] = rr, opens the next cycle: beta, g_0, the counters
// The scalars live in a state block on the device (GmresDev).  THE FREEZE: every kernel here but the two that start a solve reads
// the status first and returns unless it is RUNNING; the kernels of an inner slot also return when the cycle has closed (closing),
// and the closing kernels but END return when the cycle holds no column.  The dots are the defined reduction of mspmv_vec.hpp.
#include <hip/hip_runtime.h>

#include "../../include/mspmv_gmres.h"
#include "mspmv_krylov_op.hpp"

#pragma clang fp contract(off)

template <typename T>
struct GmresDev {                                                   // the state block on the device
    T rr, bb, stop2, beta, scale;                                   // scale: what gmres_scale_kernel divides by (beta or hn)
    int status, iterations, slots, cycles, exit_test, closing, pending, cols;
};

template <typename T>
struct GmresSmall {                                                 // the small arrays of a cycle (ldr = restart)
    T *h1, *h2, *hcol, *R, *c, *s, *g, *y;                          // R[l * ldr + i] is R[i][l]
    int ldr;
};

struct mspmv_gmres {
    mspmv::KrylovOp op;                                             // A and M^-1
    int32_t restart = 0;
    long long pstride = 0, vstride = 0;                             // elements between two rows of partials, two basis vectors
    char *base = nullptr;                                           // the one allocation the arrays below (and op's) are carved from
    void *V = nullptr, *w = nullptr, *hat = nullptr, *part = nullptr, *small = nullptr, *state = nullptr;
    mspmv_gmres_state_t h_state{};                                  // rows == 0: what a solve leaves (no device)
};

namespace {

using namespace mspmv;

static_assert(MSPMV_GMRES_NONE == KRYLOV_NONE && MSPMV_GMRES_JACOBI == KRYLOV_JACOBI && MSPMV_GMRES_FACTOR == KRYLOV_FACTOR, "the kinds of mspmv_krylov_op.hpp");

enum { GMRES_START = 0, GMRES_H1 = 1, GMRES_H2 = 2, GMRES_NORM = 3, GMRES_SOLVE = 4, GMRES_END = 5 };
constexpr int GMRES_LAUNCHES = 7, GMRES_CYCLE_LAUNCHES = 5;

// The chunk sums of v_c o w for c = 0 .. cols - 1, w's chunk in vw: each is vec_chunk_sum's tree (the quad, six butterfly steps,
// (w0 + w1) + (w2 + w3)), but the waves' sums of all columns wait in s_w for ONE barrier.  Row c of `part` takes column c's.
// The columns go B at a time, all loads of a batch ahead of its sums (the compiler does not unroll a loop around a shuffle by itself).
template <typename T, int B>
__device__ __forceinline__ void gmres_dots_batch(const T *__restrict__ V, long long vstride, int c, const T (&vw)[4], long long i, long long n,
                                                 T (*s_w)[4])
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T vv[B][4];
#pragma unroll
    for (int b = 0; b < B; ++b) vec_load4(V + (c + b) * vstride, i, n, true, vv[b]);
#pragma unroll
    for (int b = 0; b < B; ++b) {
        T s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = vv[b][k] * vw[k];
        const T sum = vec_wave_sum(vec_quad(s));
        if (lane == 0) s_w[c + b][wave] = sum;
    }
}

// DOWN: the columns are taken from the last to the first -- behind a pass that read them first to last, the latest are the likeliest
// to be in a cache still.  The sums of the columns do not depend on one another, so the order moves no bit.
template <typename T, bool DOWN>
__device__ __forceinline__ void gmres_block_dots(const T *__restrict__ V, long long vstride, int cols, const T (&vw)[4], long long i, long long n,
                                                 T *__restrict__ part, long long pstride, T (*s_w)[4])
{
    if (DOWN) {
        int c = cols;
        for (; c >= 4; c -= 4) gmres_dots_batch<T, 4>(V, vstride, c - 4, vw, i, n, s_w);
        for (; c > 0; --c) gmres_dots_batch<T, 1>(V, vstride, c - 1, vw, i, n, s_w);
    } else {
        int c = 0;
        for (; c + 4 <= cols; c += 4) gmres_dots_batch<T, 4>(V, vstride, c, vw, i, n, s_w);
        for (; c < cols; ++c) gmres_dots_batch<T, 1>(V, vstride, c, vw, i, n, s_w);
    }
    __syncthreads();
    const int t = (int) threadIdx.x;
    if (t < cols) part[t * pstride + blockIdx.x] = (s_w[t][0] + s_w[t][1]) + (s_w[t][2] + s_w[t][3]);
}

// launch 1: the chunk sums of v_i o w, i = 0 .. j
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_dots_kernel(const GmresDev<T> *__restrict__ st, const T *__restrict__ V, long long vstride, int cols,
                                                               const T *__restrict__ w, long long n, T *__restrict__ part, long long pstride)
{
    __shared__ T s_w[MSPMV_GMRES_MAX_RESTART][4];
    if (st->status != MSPMV_PCG_RUNNING || st->closing) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vw[4];
    vec_load4(w, i, n, true, vw);
    gmres_block_dots<T, false>(V, vstride, cols, vw, i, n, part, pstride, s_w);
}

// launches 3 and 5: w[e] = w[e] - fl(coef_c * v_c[e]), c = 0 .. cols - 1 in this order; then DOTS: the chunk sums of v_c o w on the new w
// (a second sweep over the chunk's columns), or the chunk sums of w o w into `part_ww`
template <typename T, bool DOTS>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_orth_kernel(const GmresDev<T> *__restrict__ st, const T *__restrict__ V, long long vstride, int cols,
                                                               const T *__restrict__ coef, T *__restrict__ w, long long n, T *__restrict__ part,
                                                               long long pstride, T *__restrict__ part_ww)
{
    __shared__ T s_w[DOTS ? MSPMV_GMRES_MAX_RESTART : 1][4];
    if (st->status != MSPMV_PCG_RUNNING || st->closing) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vw[4];
    vec_load4(w, i, n, true, vw);
#pragma unroll 4
    for (int c = 0; c < cols; ++c) {
        const T h = coef[c];
        T vv[4];
        vec_load4(V + c * vstride, i, n, true, vv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T hv = h * vv[k];
            vw[k] = vw[k] - hv;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) vw[k] = i + k < n ? vw[k] : (T) 0;    // (what the last chunk lacks stays +0 whatever the coefficients are)
    vec_store4(w, i, n, true, vw);
    if (DOTS) {
        gmres_block_dots<T, true>(V, vstride, cols, vw, i, n, part, pstride, s_w);
    } else {
        T s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = vw[k] * vw[k];
        const T ww = vec_chunk_sum(s, s_w[0]);
        if (threadIdx.x == 0) part_ww[blockIdx.x] = ww;
    }
}

// launch 7, and the first of a cycle: v[e] = src[e] / scale (scale: hn, or beta for v_0);  JACOBI: z[e] = v[e] / d[e]
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_scale_kernel(const GmresDev<T> *__restrict__ st, const T *__restrict__ src, T *__restrict__ v,
                                                                T *__restrict__ z, const T *__restrict__ diag, long long n)
{
    if (st->status != MSPMV_PCG_RUNNING || st->closing) return;
    const T scale = st->scale;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vs[4], vv[4];
    vec_load4(src, i, n, true, vs);
#pragma unroll
    for (int k = 0; k < 4; ++k) vv[k] = i + k < n ? vs[k] / scale : (T) 0;
    vec_store4(v, i, n, true, vv);
    if (KIND == MSPMV_GMRES_JACOBI) {
        T vd[4], vz[4];
        vec_load4(diag, i, n, true, vd);
#pragma unroll
        for (int k = 0; k < 4; ++k) vz[k] = i + k < n ? vv[k] / vd[k] : (T) 0;
        vec_store4(z, i, n, true, vz);
    }
}

// closing: u[e] = fl(y_0 v_0[e]), u[e] = u[e] + fl(y_c v_c[e]), c = 1 .. cols - 1;  NONE: x[e] = x[e] + u[e];  JACOBI: x[e] = x[e] +
// u[e] / d[e];  FACTOR: u goes to `u` (the sweeps and gmres_xadd_kernel follow)
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_combine_kernel(const GmresDev<T> *__restrict__ st, const T *__restrict__ V, long long vstride,
                                                                  const T *__restrict__ y, T *__restrict__ x, T *__restrict__ u,
                                                                  const T *__restrict__ diag, long long n)
{
    if (st->status != MSPMV_PCG_RUNNING) return;
    const int cols = st->cols;
    if (cols == 0) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vu[4], vv[4];
    vec_load4(V, i, n, true, vv);
    const T y0 = y[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) vu[k] = y0 * vv[k];
#pragma unroll 4
    for (int c = 1; c < cols; ++c) {
        const T yc = y[c];
        vec_load4(V + c * vstride, i, n, true, vv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T yv = yc * vv[k];
            vu[k] = vu[k] + yv;
        }
    }
    if (KIND == MSPMV_GMRES_FACTOR) {
        vec_store4(u, i, n, true, vu);
        return;
    }
    if (KIND == MSPMV_GMRES_JACOBI) {
        T vd[4];
        vec_load4(diag, i, n, true, vd);
#pragma unroll
        for (int k = 0; k < 4; ++k) vu[k] = i + k < n ? vu[k] / vd[k] : (T) 0;
    }
    const bool x_aligned = vec_aligned16(x);
    T vx[4];
    vec_load4(x, i, n, x_aligned, vx);
#pragma unroll
    for (int k = 0; k < 4; ++k) vx[k] = vx[k] + vu[k];
    vec_store4(x, i, n, x_aligned, vx);
}

// closing, FACTOR: x[e] = x[e] + z[e]
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_xadd_kernel(const GmresDev<T> *__restrict__ st, const T *__restrict__ z, T *__restrict__ x, long long n)
{
    if (st->status != MSPMV_PCG_RUNNING || st->cols == 0) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    const bool x_aligned = vec_aligned16(x);
    T vx[4], vz[4];
    vec_load4(z, i, n, true, vz);
    vec_load4(x, i, n, x_aligned, vx);
#pragma unroll
    for (int k = 0; k < 4; ++k) vx[k] = vx[k] + vz[k];
    vec_store4(x, i, n, x_aligned, vx);
}

// r[e] = b[e] - q[e] and the chunk sums of r o r.  q and r are one array (every lane reads its q before it writes its r), so neither
// is __restrict__.  `first`: the start of a solve -- no state is read, q may be NULL (x = +0, r = b), the chunk sums of b o b go to
// part_bb, and JACOBI takes d.
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void gmres_residual_kernel(const GmresDev<T> *__restrict__ st, int first, const T *__restrict__ b, const T *q,
                                                                   T *__restrict__ x, T *r, T *__restrict__ diag, const T *__restrict__ vals,
                                                                   const int *__restrict__ dpos, long long n, T *__restrict__ part_bb,
                                                                   T *__restrict__ part_rr)
{
    __shared__ T s_w[4];
    if (!first && (st->status != MSPMV_PCG_RUNNING || st->cols == 0)) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vb[4], vr[4], s[4];
    vec_load4(b, i, n, vec_aligned16(b), vb);
    if (q) {
        T vq[4];
        vec_load4(q, i, n, true, vq);
#pragma unroll
        for (int k = 0; k < 4; ++k) vr[k] = vb[k] - vq[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { vr[k] = vb[k]; s[k] = (T) 0; }
        vec_store4(x, i, n, vec_aligned16(x), s);
    }
    vec_store4(r, i, n, true, vr);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = vr[k] * vr[k];
    const T rr = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = rr;
    if (!first) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = vb[k] * vb[k];
    const T bb = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part_bb[blockIdx.x] = bb;
    if (KIND == MSPMV_GMRES_JACOBI) {
        T vd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) vd[k] = i + k < n ? vals[dpos[i + k]] : (T) 0;
        vec_store4(diag, i, n, true, vd);
    }
}

// opens a cycle of `width` slots on the residual rr (thread 0 of a step that leaves the status RUNNING)
template <typename T>
__device__ __forceinline__ void gmres_open(GmresDev<T> *st, const GmresSmall<T> &a, T rr, int width)
{
    const T beta = sqrt(rr);
    st->beta = beta;
    if (!(beta > (T) 0 && beta < (T) INFINITY)) { st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_GMRES_EXIT_BETA; return; }
    a.g[0] = beta;
    st->scale = beta;
    st->slots += width; st->cycles += 1; st->cols = 0;
}

// The folds and the scalar arithmetic.  H1 and H2: one workgroup per column i = blockIdx.x of the Hessenberg column; the other modes:
// ONE workgroup.  Every thread reads the state before thread 0 can write it (the folds' barriers lie between), so an early return is
// taken by all threads of a workgroup or by none.  part: row i of the partials is part + i * pstride, row `ldr` holds w o w or r o r.
// j: the column (H1, H2, NORM);  arg: NORM -- whether j is the cycle's last slot;  START, END -- the next cycle's width, 0 for none.
template <typename T>
__global__ __launch_bounds__(VEC_FOLD_BLOCK) void gmres_step_kernel(GmresDev<T> *st, const T *__restrict__ part, long long pstride, long long m, int mode,
                                                                    int j, int arg, T rtol2, T atol2, T *__restrict__ history, GmresSmall<T> a)
{
    __shared__ T s_p[VEC_CHUNK];
    __shared__ T s_w[16];
    const bool lead = threadIdx.x == 0;
    const T *last_row = part + (long long) a.ldr * pstride;
    if (mode == GMRES_START) {
        const T bb = vec_fold(part, m, s_p, s_w), rr = vec_fold(last_row, m, s_p, s_w);
        if (lead) {
            const T scaled = rtol2 * bb, stop2 = scaled > atol2 ? scaled : atol2;
            const bool done = rr <= stop2 && rr < (T) INFINITY;         // (never on an infinite residual)
            st->bb = bb; st->rr = rr; st->stop2 = stop2; st->beta = 0; st->scale = 0;
            st->iterations = 0; st->slots = 0; st->cycles = 0; st->closing = 0; st->pending = 0; st->cols = 0;
            st->exit_test = done ? MSPMV_GMRES_EXIT_START : MSPMV_GMRES_EXIT_NONE;
            st->status = done ? MSPMV_PCG_CONVERGED : MSPMV_PCG_RUNNING;
            if (history) history[0] = rr;
            if (!done && arg > 0) gmres_open(st, a, rr, arg);
        }
        return;
    }
    if (st->status != MSPMV_PCG_RUNNING) return;
    if (mode == GMRES_H1 || mode == GMRES_H2) {
        if (st->closing) return;
        const int i = (int) blockIdx.x;
        const T h = vec_fold(part + (long long) i * pstride, m, s_p, s_w);
        if (!lead) return;
        if (mode == GMRES_H1) a.h1[i] = h;
        else { a.h2[i] = h; a.hcol[i] = a.h1[i] + h; }
        return;
    }
    if (mode == GMRES_NORM) {
        if (st->closing) return;
        const T ww = vec_fold(last_row, m, s_p, s_w);
        if (!lead) return;
        const T hn = sqrt(ww);
        T hj = a.hcol[0];
        for (int i = 0; i < j; ++i) {                                // the earlier rotations: hj is h_i, next is h_{i+1}
            const T next = a.hcol[i + 1], c = a.c[i], s = a.s[i];
            const T ch = c * hj, sn = s * next, cn = c * next, sh = s * hj;
            a.hcol[i] = ch + sn;
            hj = cn - sh;
        }
        const T hh = hj * hj, nn = hn * hn;
        const T d = sqrt(hh + nn);
        if (!(d > (T) 0 && d < (T) INFINITY)) { st->pending = 1; st->closing = 1; return; }      // the column is dropped
        const T c = hj / d, s = hn / d;
        a.c[j] = c; a.s[j] = s;
        T *col = a.R + (long long) j * a.ldr;
        for (int i = 0; i < j; ++i) col[i] = a.hcol[i];
        col[j] = d;
        const T gj = a.g[j];
        const T gn = (-s) * gj;
        a.g[j + 1] = gn; a.g[j] = c * gj;
        const T gg = gn * gn;
        const int k = st->iterations + 1;
        if (history) history[k] = gg;
        st->iterations = k; st->cols = j + 1;
        st->scale = hn;
        if (gg <= st->stop2 || gg != gg || !(hn > (T) 0) || arg) st->closing = 1;
        return;
    }
    const int cols = st->cols;
    if (mode == GMRES_SOLVE) {
        if (!lead) return;
        T *y = s_p;                                                  // (thread 0 alone: no barrier is needed)
        for (int i = cols - 1; i >= 0; --i) {
            T acc = a.g[i];
            for (int l = i + 1; l < cols; ++l) {
                const T ry = a.R[(long long) l * a.ldr + i] * y[l];
                acc = acc - ry;
            }
            y[i] = acc / a.R[(long long) i * a.ldr + i];
            a.y[i] = y[i];
        }
        return;
    }
    // GMRES_END
    const T folded = vec_fold(last_row, m, s_p, s_w);
    if (!lead) return;
    T rr = st->rr;
    if (cols > 0) {
        rr = folded;
        st->rr = rr;
        if (history) history[st->iterations] = rr;
    }
    st->closing = 0;
    if (st->pending) { st->pending = 0; st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_GMRES_EXIT_D; return; }
    if (rr <= st->stop2 && rr < (T) INFINITY) { st->status = MSPMV_PCG_CONVERGED; st->exit_test = MSPMV_GMRES_EXIT_RR; return; }
    if (arg > 0) gmres_open(st, a, rr, arg);
}

template <typename T>
struct GmresRun {
    mspmv_gmres *h;
    hipStream_t stream;
    int dbg;
    const T *vals;
    const int32_t *off, *cols;
    T *x;
    T rtol2, atol2;
    T *history;
    long long n;
    unsigned grid;
    GmresSmall<T> small;

    T *arr(void *a) const { return static_cast<T *>(a); }
    GmresDev<T> *st() const { return static_cast<GmresDev<T> *>(h->state); }
    const GmresDev<T> *cst() const { return st(); }
    T *v(int j) const { return arr(h->V) + (long long) j * h->vstride; }
    T *z(int j) const { return h->op.kind == MSPMV_GMRES_NONE ? v(j) : arr(h->hat); }
    T *part(int row) const { return arr(h->part) + (long long) row * h->pstride; }

    int product(const T *in, T *out) const { return krylov_product(h->op, vals, off, cols, in, out, stream, dbg); }
    int sweeps(const T *in) const { return krylov_sweeps<T>(h->op, in, arr(h->hat), stream, dbg); }  // hat = second^-1 (first^-1 in)
    int step(int mode, int j, int arg) const
    {
        const unsigned blocks = mode == GMRES_H1 || mode == GMRES_H2 ? (unsigned) j + 1 : 1;
        hipLaunchKernelGGL(gmres_step_kernel<T>, dim3(blocks), dim3(VEC_FOLD_BLOCK), 0, stream, st(), (const T *) arr(h->part), h->pstride, h->op.m, mode, j, arg,
                           rtol2, atol2, history, small);
        return lv_launched(stream, dbg, "gmres_step_kernel", blocks, VEC_FOLD_BLOCK);
    }
    int dots(int j) const
    {
        hipLaunchKernelGGL(gmres_dots_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->V), h->vstride, j + 1,
                           (const T *) arr(h->w), n, arr(h->part), h->pstride);
        return lv_launched(stream, dbg, "gmres_dots_kernel", grid, VEC_BLOCK);
    }
    template <bool DOTS>
    int orth(int j) const
    {
        hipLaunchKernelGGL((gmres_orth_kernel<T, DOTS>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->V), h->vstride, j + 1,
                           (const T *) (DOTS ? small.h1 : small.h2), arr(h->w), n, arr(h->part), h->pstride, part(h->restart));
        return lv_launched(stream, dbg, "gmres_orth_kernel", grid, VEC_BLOCK);
    }
    int scale(int j) const                                           // v_j = w / scale
    {
        if (h->op.kind == MSPMV_GMRES_JACOBI)
            hipLaunchKernelGGL((gmres_scale_kernel<T, MSPMV_GMRES_JACOBI>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->w), v(j),
                               arr(h->hat), (const T *) arr(h->op.diag), n);
        else
            hipLaunchKernelGGL((gmres_scale_kernel<T, MSPMV_GMRES_NONE>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->w), v(j),
                               (T *) nullptr, (const T *) nullptr, n);
        return lv_launched(stream, dbg, "gmres_scale_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int combine_as() const
    {
        hipLaunchKernelGGL((gmres_combine_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->V), h->vstride,
                           (const T *) small.y, x, arr(h->w), (const T *) arr(h->op.diag), n);
        return lv_launched(stream, dbg, "gmres_combine_kernel", grid, VEC_BLOCK);
    }
    int combine() const
    {
        if (h->op.kind == MSPMV_GMRES_NONE) return combine_as<MSPMV_GMRES_NONE>();
        if (h->op.kind == MSPMV_GMRES_JACOBI) return combine_as<MSPMV_GMRES_JACOBI>();
        if (int e = combine_as<MSPMV_GMRES_FACTOR>()) return e;
        if (int e = sweeps(arr(h->w))) return e;
        hipLaunchKernelGGL(gmres_xadd_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), (const T *) arr(h->hat), x, n);
        return lv_launched(stream, dbg, "gmres_xadd_kernel", grid, VEC_BLOCK);
    }
    int residual(int first, const T *b, const T *q) const
    {
        if (h->op.kind == MSPMV_GMRES_JACOBI)
            hipLaunchKernelGGL((gmres_residual_kernel<T, MSPMV_GMRES_JACOBI>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), first, b, q, x, arr(h->w),
                               arr(h->op.diag), vals, (const int *) h->op.dpos, n, part(0), part(h->restart));
        else
            hipLaunchKernelGGL((gmres_residual_kernel<T, MSPMV_GMRES_NONE>), dim3(grid), dim3(VEC_BLOCK), 0, stream, cst(), first, b, q, x, arr(h->w),
                               (T *) nullptr, vals, (const int *) nullptr, n, part(0), part(h->restart));
        return lv_launched(stream, dbg, "gmres_residual_kernel", grid, VEC_BLOCK);
    }

    int start(const T *b, int guess, int width) const
    {
        const T *q = nullptr;
        if (guess) {
            if (int e = product(x, arr(h->w))) return e;
            q = arr(h->w);
        }
        if (int e = residual(1, b, q)) return e;
        return step(GMRES_START, 0, width);
    }
    int inner(int j, int width) const
    {
        if (h->op.kind == MSPMV_GMRES_FACTOR)
            if (int e = sweeps(v(j))) return e;
        if (int e = product(z(j), arr(h->w))) return e;
        if (int e = dots(j)) return e;
        if (int e = step(GMRES_H1, j, 0)) return e;
        if (int e = orth<true>(j)) return e;
        if (int e = step(GMRES_H2, j, 0)) return e;
        if (int e = orth<false>(j)) return e;
        if (int e = step(GMRES_NORM, j, j == width - 1)) return e;
        return scale(j + 1);                                         // (returns at once where NORM closed the cycle, as slot restart - 1 always does)
    }
    int closing(const T *b, int next_width) const
    {
        if (int e = step(GMRES_SOLVE, 0, 0)) return e;
        if (int e = combine()) return e;
        if (int e = product(x, arr(h->w))) return e;
        if (int e = residual(0, b, arr(h->w))) return e;
        return step(GMRES_END, 0, next_width);
    }
};

template <typename T>
int gmres_read(const mspmv_gmres *h, mspmv_gmres_state_t *out, hipStream_t stream, int *closing = nullptr)
{
    GmresDev<T> d;
    if (int e = krylov_read(h->state, d, stream)) return e;
    out->status = d.status; out->iterations = d.iterations; out->slots = d.slots; out->cycles = d.cycles; out->exit_test = d.exit_test;
    out->rr = (double) d.rr; out->bb = (double) d.bb; out->stop2 = (double) d.stop2; out->beta = (double) d.beta;
    if (closing) *closing = d.closing;
    return hipSuccess;
}

template <typename T>
int gmres_solve(mspmv_gmres *h, const T *vals, const int32_t *off, const int32_t *cols, const T *b, T *x, int guess, double rtol, double atol,
                int32_t max_iterations, int32_t check_every, T *history, hipStream_t stream, int dbg)
{
    T rtol2, atol2;
    if (int e = krylov_refuse_solve(h ? &h->op : nullptr, vals, off, cols, b, x, rtol, atol, max_iterations, check_every, rtol2, atol2)) return e;
    if (h->op.rows == 0) {
        h->h_state.status = MSPMV_PCG_CONVERGED; h->h_state.iterations = 0; h->h_state.slots = 0; h->h_state.cycles = 0;
        h->h_state.exit_test = MSPMV_GMRES_EXIT_START;
        h->h_state.rr = 0; h->h_state.bb = 0; h->h_state.beta = 0; h->h_state.stop2 = (double) atol2;
        return hipSuccess;
    }
    T *sm = static_cast<T *>(h->small);
    const int R = h->restart;
    GmresSmall<T> small;
    small.h1 = sm; small.h2 = sm + R; small.hcol = sm + 2 * R; small.c = sm + 3 * R; small.s = sm + 4 * R; small.y = sm + 5 * R;
    small.g = sm + 6 * R;                                            // (restart + 1 entries)
    small.R = sm + 7 * R + 1;
    small.ldr = R;
    const GmresRun<T> run{h, stream, dbg, vals, off, cols, x, rtol2, atol2, history, (long long) h->op.rows, (unsigned) h->op.m, small};
    if (int e = run.start(b, guess, std::min(R, max_iterations))) return e;
    int since = 0;                                                   // inner slots since the host last looked
    for (int done = 0; done < max_iterations;) {
        const int width = std::min(R, max_iterations - done);
        if (int e = run.scale(0)) return e;
        bool closed = false;
        for (int j = 0; j < width; ++j) {
            if (!closed)
                if (int e = run.inner(j, width)) return e;
            ++since;
            if (check_every > 0 && since >= check_every && !closed && j + 1 < width) {
                mspmv_gmres_state_t now{};
                int flag = 0;
                if (int e = gmres_read<T>(h, &now, stream, &flag)) return e;
                since = 0;
                if (now.status != MSPMV_PCG_RUNNING) return hipSuccess;
                closed = flag != 0;                                  // the rest of the cycle's slots would return at once: they count, but are not enqueued
            }
        }
        done += width;
        if (int e = run.closing(b, std::min(R, max_iterations - done))) return e;
        if (check_every > 0 && since >= check_every) {
            mspmv_gmres_state_t now{};
            if (int e = gmres_read<T>(h, &now, stream)) return e;
            since = 0;
            if (now.status != MSPMV_PCG_RUNNING) break;
        }
    }
    return hipSuccess;
}

static int gmres_build(mspmv_gmres &h, const int32_t *off, const int32_t *cols, hipStream_t stream, int dbg)
{
    if (int e = krylov_query(h.op)) return e;
    const uint64_t vb = (uint64_t) h.op.value_bytes, vec = align256((uint64_t) h.op.rows * vb), R = (uint64_t) h.restart;
    h.vstride = (long long) (vec / vb);
    h.pstride = (long long) (((uint64_t) h.op.m * vb + 15) / 16 * 16 / vb);                                         // rows of partials 16-byte aligned
    const bool own_hat = h.op.kind != MSPMV_GMRES_NONE;             // NONE: z is v_j itself
    KrylovCarve c;
    const uint64_t state_o = c.take(256), V_o = c.take((R + 1) * vec), w_o = c.take(vec), hat_o = c.take(own_hat ? vec : 0);
    c.precond(h.op, vec);
    const uint64_t part_o = c.take(align256((R + 1) * (uint64_t) h.pstride * vb)), small_o = c.take(align256((R * R + 7 * R + 1) * vb));
    c.product(h.op);
    if (int e = krylov_build(h.op, h.base, c, off, cols, stream, dbg)) return e;
    h.h_state.device_bytes = c.size;
    h.state = h.base + state_o; h.V = h.base + V_o; h.w = h.base + w_o;
    h.hat = own_hat ? h.base + hat_o : nullptr;
    h.part = h.base + part_o; h.small = h.base + small_o;
    return hipSuccess;
}

}  // namespace

extern "C" {

int mspmv_gmres_create(mspmv_gmres_t **solver, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                       int32_t value_bytes, int32_t precond_kind, int32_t restart, mspmv_stream_t stream, int debug_sync)
{
    if (!solver) return hipErrorInvalidValue;
    *solver = nullptr;
    if (int e = krylov_refuse_create(d_row_offsets, d_column_indices, rows, nnz, value_bytes, precond_kind)) return e;
    if (restart < 1 || restart > MSPMV_GMRES_MAX_RESTART) return hipErrorInvalidValue;
    return krylov_create(solver, rows, nnz, value_bytes, precond_kind, [&](mspmv_gmres &h) {
        h.restart = restart;
        h.h_state.restart = restart;
        h.h_state.launches_per_iteration = GMRES_LAUNCHES;
        h.h_state.launches_per_cycle = GMRES_CYCLE_LAUNCHES + (precond_kind == MSPMV_GMRES_FACTOR ? 1 : 0);
        return rows > 0 ? gmres_build(h, d_row_offsets, d_column_indices, reinterpret_cast<hipStream_t>(stream), debug_sync) : (int) hipSuccess;
    });
}

int mspmv_gmres_set_factor(mspmv_gmres_t *solver, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan, const void *d_factor_values,
                           const int32_t *d_row_offsets, const int32_t *d_column_indices)
{
    return krylov_set_factor(solver ? &solver->op : nullptr, first_plan, second_plan, d_factor_values, d_row_offsets, d_column_indices);
}

int mspmv_gmres_solve_f32(mspmv_gmres_t *solver, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const float *d_b, float *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                          int32_t check_every, float *d_history, mspmv_stream_t stream, int debug_sync)
{
    return gmres_solve<float>(solver, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                              d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_gmres_solve_f64(mspmv_gmres_t *solver, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const double *d_b, double *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                          int32_t check_every, double *d_history, mspmv_stream_t stream, int debug_sync)
{
    return gmres_solve<double>(solver, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                               d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_gmres_state(mspmv_gmres_t *solver, mspmv_gmres_state_t *state, mspmv_stream_t stream)
{
    if (!solver || !state) return hipErrorInvalidValue;
    *state = solver->h_state;
    if (solver->op.rows == 0) return hipSuccess;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return solver->op.value_bytes == 4 ? gmres_read<float>(solver, state, s) : gmres_read<double>(solver, state, s);
}

int mspmv_gmres_destroy(mspmv_gmres_t *solver) { return krylov_destroy(solver); }

}  // extern "C"
