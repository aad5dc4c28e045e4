// mspmv_bicgstab.hip -- right-preconditioned BiCGStab on the device (mspmv_bicgstab_* of include/mspmv_krylov.h, which states the
// arithmetic).  This file is libmspmv_krylov.so: a layer ON TOP of the C ABI.  The products and the sweeps are calls of what
// libmspmv.so exports (mspmv_csrmv_prepare, mspmv_csrmv_prepared_*, mspmv_csrsv_solve_*, mspmv_csrsv_plan_info); from the source tree
// it takes only header-only pieces: the deterministic vector layer (mspmv_vec.hpp), lv_launched (mspmv_levels.hpp) and what the three
// Krylov solvers know about A and M^-1 (mspmv_krylov_op.hpp: those calls, the refusals, the operator's part of the carve).
//
// What one iteration launches, on one stream, ordered by the kernel boundary alone:
//     FACTOR: two mspmv_csrsv_solve_*     ph = second^-1 first^-1 p      (NONE: ph is p;  JACOBI: ph = p / d was made with p)
//     mspmv_csrmv_prepared_*              v = A ph
//  1  bicgstab_dot_kernel                 the chunk sums of rh.v                                     (one workgroup per 1024 elements)
//  2  bicgstab_step_kernel  RV            folds them: rv, the breakdown test, alpha                  (ONE workgroup)
//  3  bicgstab_s_kernel                   x += alpha ph,  s = r - alpha v (into r's array),  the chunk sums of s.s;  JACOBI: sh = s / d
//  4  bicgstab_step_kernel  SS            folds: ss, the half-step test
//     FACTOR: two mspmv_csrsv_solve_*     sh = second^-1 first^-1 s      (NONE: sh is s)
//     mspmv_csrmv_prepared_*              t = A sh
//  5  bicgstab_dot2_kernel                the chunk sums of t.s and t.t in one pass over t
//  6  bicgstab_step_kernel  TT            folds: ts, tt, the breakdown test, omega
//  7  bicgstab_update_kernel              x += omega sh,  r = s - omega t,  the chunk sums of r.r and rh.r
//  8  bicgstab_step_kernel  RR            folds: rr, rho', history, iterations, the tests, beta
//  9  bicgstab_p_kernel                   p = r + beta (p - omega v);  JACOBI: ph = p / d
// so the solver adds 9 launches per iteration to the two products and the four sweeps, for every kind.  ph and sh share one array
// (ph is dead once x has taken alpha ph).  The scalars live in a state block on the device (BicgDev); the host reads it only between
// groups of check_every iterations, and with check_every == 0 never.  THE FREEZE: every kernel here but the two that start a solve
// reads the status first and returns unless it is RUNNING, so iterations enqueued past the end change neither x nor the state nor
// the history.  The dots are the defined reduction of mspmv_vec.hpp: chunk sums where the products are made, the fold in the
// one-workgroup step.
#include <hip/hip_runtime.h>

#include "../../include/mspmv_krylov.h"
#include "mspmv_krylov_op.hpp"

#pragma clang fp contract(off)

template <typename T>
struct BicgDev {                                                    // the state block on the device
    T rho, alpha, omega, beta, rr, bb, stop2, ss;
    int status, iterations, exit_test, spare;
};

struct mspmv_bicgstab {
    mspmv::KrylovOp op;                                             // A and M^-1
    char *base = nullptr;                                           // the one allocation the arrays below (and op's) are carved from
    void *p = nullptr, *v = nullptr, *r = nullptr, *rh = nullptr, *t = nullptr, *hat = nullptr, *part[2] = {}, *state = nullptr;
    mspmv_bicgstab_state_t h_state{};                               // rows == 0: what a solve leaves (no device)
};

namespace {

using namespace mspmv;

static_assert(MSPMV_BICGSTAB_NONE == KRYLOV_NONE && MSPMV_BICGSTAB_JACOBI == KRYLOV_JACOBI && MSPMV_BICGSTAB_FACTOR == KRYLOV_FACTOR,
              "the kinds of mspmv_krylov_op.hpp");

enum { BICG_START = 0, BICG_RV = 1, BICG_SS = 2, BICG_TT = 3, BICG_RR = 4 };
constexpr int BICG_LAUNCHES = 9;

// the start of a solve: r = b - q (q = A x for a guess; NULL: x = +0, r = b), rh = r, p = r, the chunk sums of b.b and r.r;
// JACOBI: d, ph = p / d
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_init_kernel(const T *__restrict__ b, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                                  T *__restrict__ rh, T *__restrict__ p, T *__restrict__ hat, T *__restrict__ diag,
                                                                  const T *__restrict__ vals, const int *__restrict__ dpos, long long n,
                                                                  T *__restrict__ part_bb, T *__restrict__ part_rr)
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
    vec_store4(rh, i, n, true, vr);
    vec_store4(p, i, n, true, vr);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vb[j] * vb[j];
    const T bb = vec_chunk_sum(s, s_w);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vr[j] * vr[j];
    const T rr = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) { part_bb[blockIdx.x] = bb; part_rr[blockIdx.x] = rr; }
    if (KIND == MSPMV_BICGSTAB_JACOBI) {
        T vd[4], vh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool have = i + j < n;
            vd[j] = have ? vals[dpos[i + j]] : (T) 0;
            vh[j] = have ? vr[j] / vd[j] : (T) 0;
        }
        vec_store4(diag, i, n, true, vd);
        vec_store4(hat, i, n, true, vh);
    }
}

// the chunk sums of a.b (rh.v)
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_dot_kernel(const BicgDev<T> *__restrict__ st, const T *__restrict__ a, const T *__restrict__ b,
                                                                 long long n, T *__restrict__ part)
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

// the chunk sums of t.s and t.t
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_dot2_kernel(const BicgDev<T> *__restrict__ st, const T *__restrict__ t, const T *__restrict__ sv,
                                                                  long long n, T *__restrict__ part_ts, T *__restrict__ part_tt)
{
    __shared__ T s_w[4];
    if (st->status != MSPMV_PCG_RUNNING) return;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vt[4], vs[4], s[4];
    vec_load4(t, i, n, true, vt);
    vec_load4(sv, i, n, true, vs);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vt[j] * vs[j];
    const T ts = vec_chunk_sum(s, s_w);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vt[j] * vt[j];
    const T tt = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) { part_ts[blockIdx.x] = ts; part_tt[blockIdx.x] = tt; }
}

// x[i] = x[i] + fl(alpha ph[i]),  s[i] = r[i] - fl(alpha v[i]) (in r's array),  the chunk sums of s.s;  JACOBI: sh[i] = s[i] / d[i].
// ph and sh may be one array (every lane reads its ph before it writes its sh), so neither is __restrict__.
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_s_kernel(const BicgDev<T> *__restrict__ st, const T *ph, const T *__restrict__ v, T *__restrict__ x,
                                                               T *__restrict__ r, T *sh, const T *__restrict__ diag, long long n, T *__restrict__ part_ss)
{
    __shared__ T s_w[4];
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T alpha = st->alpha;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    const bool x_aligned = vec_aligned16(x);
    T vp[4], vv[4], vx[4], vr[4], s[4];
    vec_load4(ph, i, n, true, vp);
    vec_load4(v, i, n, true, vv);
    vec_load4(x, i, n, x_aligned, vx);
    vec_load4(r, i, n, true, vr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T ap = alpha * vp[j], av = alpha * vv[j];
        vx[j] = vx[j] + ap;
        vr[j] = i + j < n ? vr[j] - av : (T) 0;
        s[j] = vr[j] * vr[j];
    }
    vec_store4(x, i, n, x_aligned, vx);
    vec_store4(r, i, n, true, vr);
    const T ss = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part_ss[blockIdx.x] = ss;
    if (KIND == MSPMV_BICGSTAB_JACOBI) {
        T vd[4], vh[4];
        vec_load4(diag, i, n, true, vd);
#pragma unroll
        for (int j = 0; j < 4; ++j) vh[j] = i + j < n ? vr[j] / vd[j] : (T) 0;
        vec_store4(sh, i, n, true, vh);
    }
}

// x[i] = x[i] + fl(omega sh[i]),  r[i] = s[i] - fl(omega t[i]) (s is what r's array holds),  the chunk sums of r.r and rh.r.
// NONE: sh is r's array itself (every lane reads before it writes), so sh and r are not __restrict__.
template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_update_kernel(const BicgDev<T> *__restrict__ st, const T *sh, const T *__restrict__ t,
                                                                    const T *__restrict__ rh, T *__restrict__ x, T *r, long long n,
                                                                    T *__restrict__ part_rr, T *__restrict__ part_rho)
{
    __shared__ T s_w[4];
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T omega = st->omega;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    const bool x_aligned = vec_aligned16(x);
    T vh[4], vt[4], vx[4], vr[4], vs[4], s[4];
    vec_load4(sh, i, n, true, vh);
    vec_load4(t, i, n, true, vt);
    vec_load4(x, i, n, x_aligned, vx);
    vec_load4(r, i, n, true, vr);
    vec_load4(rh, i, n, true, vs);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T oh = omega * vh[j], ot = omega * vt[j];
        vx[j] = vx[j] + oh;
        vr[j] = i + j < n ? vr[j] - ot : (T) 0;
        s[j] = vr[j] * vr[j];
    }
    vec_store4(x, i, n, x_aligned, vx);
    vec_store4(r, i, n, true, vr);
    const T rr = vec_chunk_sum(s, s_w);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = vs[j] * vr[j];
    const T rho = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) { part_rr[blockIdx.x] = rr; part_rho[blockIdx.x] = rho; }
}

// p[i] = r[i] + fl(beta fl(p[i] - fl(omega v[i])));  JACOBI: ph[i] = p[i] / d[i]
template <typename T, int KIND>
__global__ __launch_bounds__(VEC_BLOCK) void bicgstab_p_kernel(const BicgDev<T> *__restrict__ st, const T *__restrict__ r, const T *__restrict__ v,
                                                               T *__restrict__ p, T *__restrict__ hat, const T *__restrict__ diag, long long n)
{
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T beta = st->beta, omega = st->omega;
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T vr[4], vv[4], vp[4];
    vec_load4(r, i, n, true, vr);
    vec_load4(v, i, n, true, vv);
    vec_load4(p, i, n, true, vp);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T ov = omega * vv[j];
        const T d = vp[j] - ov;
        const T bd = beta * d;
        vp[j] = vr[j] + bd;
    }
    vec_store4(p, i, n, true, vp);
    if (KIND == MSPMV_BICGSTAB_JACOBI) {
        T vd[4], vh[4];
        vec_load4(diag, i, n, true, vd);
#pragma unroll
        for (int j = 0; j < 4; ++j) vh[j] = i + j < n ? vp[j] / vd[j] : (T) 0;
        vec_store4(hat, i, n, true, vh);
    }
}

// ONE workgroup: the folds and the scalar arithmetic, once.  Every thread reads the status before thread 0 can write it (the folds'
// barriers lie between), so the early return is taken by all threads or by none.
template <typename T>
__global__ __launch_bounds__(VEC_FOLD_BLOCK) void bicgstab_step_kernel(BicgDev<T> *st, const T *__restrict__ part0, const T *__restrict__ part1, long long m,
                                                                       int mode, T rtol2, T atol2, T *__restrict__ history)
{
    __shared__ T s_p[VEC_CHUNK];
    __shared__ T s_w[16];
    const bool lead = threadIdx.x == 0;
    if (mode == BICG_START) {
        const T bb = vec_fold(part0, m, s_p, s_w), rr = vec_fold(part1, m, s_p, s_w);
        if (lead) {
            const T scaled = rtol2 * bb, stop2 = scaled > atol2 ? scaled : atol2;
            const bool done = rr <= stop2 && rr < (T) INFINITY;         // (never on an infinite residual)
            st->alpha = 0; st->omega = 0; st->beta = 0; st->ss = 0;
            st->bb = bb; st->rr = rr; st->rho = rr; st->stop2 = stop2;
            st->iterations = 0; st->spare = 0;
            st->exit_test = done ? MSPMV_BICGSTAB_EXIT_START : MSPMV_BICGSTAB_EXIT_NONE;
            st->status = done ? MSPMV_PCG_CONVERGED : MSPMV_PCG_RUNNING;
            if (history) history[0] = rr;
        }
        return;
    }
    if (st->status != MSPMV_PCG_RUNNING) return;
    const T a = vec_fold(part0, m, s_p, s_w);
    const T b = mode == BICG_TT || mode == BICG_RR ? vec_fold(part1, m, s_p, s_w) : (T) 0;
    if (!lead) return;
    const int k = st->iterations + 1;
    if (mode == BICG_RV) {
        if (!(a > (T) 0 || a < (T) 0)) { st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_BICGSTAB_EXIT_RV; }
        else st->alpha = st->rho / a;
    } else if (mode == BICG_SS) {
        st->ss = a;
        if (a <= st->stop2 && a < (T) INFINITY) {
            st->rr = a; st->iterations = k;
            if (history) history[k] = a;
            st->status = MSPMV_PCG_CONVERGED; st->exit_test = MSPMV_BICGSTAB_EXIT_HALF;
        }
    } else if (mode == BICG_TT) {                                    // a = ts, b = tt
        if (!(b > (T) 0)) {
            const T ss = st->ss;
            st->rr = ss; st->iterations = k;
            if (history) history[k] = ss;
            st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_BICGSTAB_EXIT_TT;
        } else {
            st->omega = a / b;
        }
    } else {                                                         // a = rr, b = rho'
        const T omega = st->omega;
        st->rr = a; st->iterations = k;
        if (history) history[k] = a;
        if (a <= st->stop2 && a < (T) INFINITY) { st->status = MSPMV_PCG_CONVERGED; st->exit_test = MSPMV_BICGSTAB_EXIT_RR; }
        else if (a != a) { st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_BICGSTAB_EXIT_RR_NAN; }
        else if (!(omega > (T) 0 || omega < (T) 0)) { st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_BICGSTAB_EXIT_OMEGA; }
        else if (!(b > (T) 0 || b < (T) 0)) { st->status = MSPMV_PCG_BREAKDOWN; st->exit_test = MSPMV_BICGSTAB_EXIT_RHO; }
        else {
            const T rho_ratio = b / st->rho, step_ratio = st->alpha / omega;
            st->beta = rho_ratio * step_ratio;
            st->rho = b;
        }
    }
}

template <typename T>
struct BicgRun {
    mspmv_bicgstab *h;
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
    BicgDev<T> *st() const { return static_cast<BicgDev<T> *>(h->state); }
    T *ph() const { return arr(h->op.kind == MSPMV_BICGSTAB_NONE ? h->p : h->hat); }
    T *sh() const { return arr(h->op.kind == MSPMV_BICGSTAB_NONE ? h->r : h->hat); }

    int product(const T *in, T *out) const { return krylov_product(h->op, vals, off, cols, in, out, stream, dbg); }
    int sweeps(const T *in) const { return krylov_sweeps<T>(h->op, in, arr(h->hat), stream, dbg); }  // hat = second^-1 (first^-1 in)
    int step(int mode) const
    {
        hipLaunchKernelGGL(bicgstab_step_kernel<T>, dim3(1), dim3(VEC_FOLD_BLOCK), 0, stream, st(), (const T *) arr(h->part[0]), (const T *) arr(h->part[1]),
                           h->op.m, mode, rtol2, atol2, history);
        return lv_launched(stream, dbg, "bicgstab_step_kernel", 1, VEC_FOLD_BLOCK);
    }
    int dot(const T *a, const T *b) const
    {
        hipLaunchKernelGGL(bicgstab_dot_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, (const BicgDev<T> *) st(), a, b, n, arr(h->part[0]));
        return lv_launched(stream, dbg, "bicgstab_dot_kernel", grid, VEC_BLOCK);
    }
    int dot2() const
    {
        hipLaunchKernelGGL(bicgstab_dot2_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, (const BicgDev<T> *) st(), (const T *) arr(h->t),
                           (const T *) arr(h->r), n, arr(h->part[0]), arr(h->part[1]));
        return lv_launched(stream, dbg, "bicgstab_dot2_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int init(const T *b, const T *q) const
    {
        hipLaunchKernelGGL((bicgstab_init_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, b, q, x, arr(h->r), arr(h->rh), arr(h->p), arr(h->hat),
                           arr(h->op.diag), vals, (const int *) h->op.dpos, n, arr(h->part[0]), arr(h->part[1]));
        return lv_launched(stream, dbg, "bicgstab_init_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int s_update() const
    {
        hipLaunchKernelGGL((bicgstab_s_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, (const BicgDev<T> *) st(), (const T *) ph(),
                           (const T *) arr(h->v), x, arr(h->r), arr(h->hat), (const T *) arr(h->op.diag), n, arr(h->part[0]));
        return lv_launched(stream, dbg, "bicgstab_s_kernel", grid, VEC_BLOCK);
    }
    int update() const
    {
        hipLaunchKernelGGL(bicgstab_update_kernel<T>, dim3(grid), dim3(VEC_BLOCK), 0, stream, (const BicgDev<T> *) st(), (const T *) sh(),
                           (const T *) arr(h->t), (const T *) arr(h->rh), x, arr(h->r), n, arr(h->part[0]), arr(h->part[1]));
        return lv_launched(stream, dbg, "bicgstab_update_kernel", grid, VEC_BLOCK);
    }
    template <int KIND>
    int new_p() const
    {
        hipLaunchKernelGGL((bicgstab_p_kernel<T, KIND>), dim3(grid), dim3(VEC_BLOCK), 0, stream, (const BicgDev<T> *) st(), (const T *) arr(h->r),
                           (const T *) arr(h->v), arr(h->p), arr(h->hat), (const T *) arr(h->op.diag), n);
        return lv_launched(stream, dbg, "bicgstab_p_kernel", grid, VEC_BLOCK);
    }

    int start(const T *b, int guess) const
    {
        const T *q = nullptr;
        if (guess) {
            if (int e = product(x, arr(h->v))) return e;
            q = arr(h->v);
        }
        if (int e = h->op.kind == MSPMV_BICGSTAB_JACOBI ? init<MSPMV_BICGSTAB_JACOBI>(b, q) : init<MSPMV_BICGSTAB_NONE>(b, q)) return e;
        return step(BICG_START);
    }
    int iteration() const
    {
        const bool jacobi = h->op.kind == MSPMV_BICGSTAB_JACOBI, factor = h->op.kind == MSPMV_BICGSTAB_FACTOR;
        if (factor)
            if (int e = sweeps(arr(h->p))) return e;
        if (int e = product(ph(), arr(h->v))) return e;
        if (int e = dot(arr(h->rh), arr(h->v))) return e;
        if (int e = step(BICG_RV)) return e;
        if (int e = jacobi ? s_update<MSPMV_BICGSTAB_JACOBI>() : s_update<MSPMV_BICGSTAB_NONE>()) return e;
        if (int e = step(BICG_SS)) return e;
        if (factor)
            if (int e = sweeps(arr(h->r))) return e;
        if (int e = product(sh(), arr(h->t))) return e;
        if (int e = dot2()) return e;
        if (int e = step(BICG_TT)) return e;
        if (int e = update()) return e;
        if (int e = step(BICG_RR)) return e;
        return jacobi ? new_p<MSPMV_BICGSTAB_JACOBI>() : new_p<MSPMV_BICGSTAB_NONE>();
    }
};

template <typename T>
int bicg_read(const mspmv_bicgstab *h, mspmv_bicgstab_state_t *out, hipStream_t stream)
{
    BicgDev<T> d;
    if (int e = krylov_read(h->state, d, stream)) return e;
    out->status = d.status; out->iterations = d.iterations; out->exit_test = d.exit_test;
    out->rr = (double) d.rr; out->bb = (double) d.bb; out->stop2 = (double) d.stop2;
    out->rho = (double) d.rho; out->alpha = (double) d.alpha; out->omega = (double) d.omega;
    return hipSuccess;
}

template <typename T>
int bicg_solve(mspmv_bicgstab *h, const T *vals, const int32_t *off, const int32_t *cols, const T *b, T *x, int guess, double rtol, double atol,
               int32_t max_iterations, int32_t check_every, T *history, hipStream_t stream, int dbg)
{
    T rtol2, atol2;
    if (int e = krylov_refuse_solve(h ? &h->op : nullptr, vals, off, cols, b, x, rtol, atol, max_iterations, check_every, rtol2, atol2)) return e;
    if (h->op.rows == 0) {
        h->h_state.status = MSPMV_PCG_CONVERGED; h->h_state.iterations = 0; h->h_state.exit_test = MSPMV_BICGSTAB_EXIT_START;
        h->h_state.rr = 0; h->h_state.bb = 0; h->h_state.rho = 0; h->h_state.alpha = 0; h->h_state.omega = 0; h->h_state.stop2 = (double) atol2;
        return hipSuccess;
    }
    const BicgRun<T> run{h, stream, dbg, vals, off, cols, x, rtol2, atol2, history, (long long) h->op.rows, (unsigned) h->op.m};
    if (int e = run.start(b, guess)) return e;
    return krylov_groups<BicgDev<T>>(run, max_iterations, check_every);
}

static int bicg_build(mspmv_bicgstab &h, const int32_t *off, const int32_t *cols, hipStream_t stream, int dbg)
{
    if (int e = krylov_query(h.op)) return e;
    const uint64_t vb = (uint64_t) h.op.value_bytes, vec = align256((uint64_t) h.op.rows * vb), part = align256((uint64_t) h.op.m * vb);
    const bool own_hat = h.op.kind != MSPMV_BICGSTAB_NONE;          // NONE: ph is p and sh is s, which lives in r
    KrylovCarve c;
    const uint64_t state_o = c.take(256), p_o = c.take(vec), v_o = c.take(vec), r_o = c.take(vec), rh_o = c.take(vec), t_o = c.take(vec),
                   hat_o = c.take(own_hat ? vec : 0);
    c.precond(h.op, vec);
    const uint64_t p0_o = c.take(part), p1_o = c.take(part);
    c.product(h.op);
    if (int e = krylov_build(h.op, h.base, c, off, cols, stream, dbg)) return e;
    h.h_state.device_bytes = c.size;
    h.state = h.base + state_o; h.p = h.base + p_o; h.v = h.base + v_o; h.r = h.base + r_o; h.rh = h.base + rh_o; h.t = h.base + t_o;
    h.hat = own_hat ? h.base + hat_o : nullptr;
    h.part[0] = h.base + p0_o; h.part[1] = h.base + p1_o;
    return hipSuccess;
}

}  // namespace

extern "C" {

int mspmv_bicgstab_create(mspmv_bicgstab_t **solver, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                          int32_t value_bytes, int32_t precond_kind, mspmv_stream_t stream, int debug_sync)
{
    if (!solver) return hipErrorInvalidValue;
    *solver = nullptr;
    if (int e = krylov_refuse_create(d_row_offsets, d_column_indices, rows, nnz, value_bytes, precond_kind)) return e;
    return krylov_create(solver, rows, nnz, value_bytes, precond_kind, [&](mspmv_bicgstab &h) {
        h.h_state.launches_per_iteration = BICG_LAUNCHES;
        return rows > 0 ? bicg_build(h, d_row_offsets, d_column_indices, reinterpret_cast<hipStream_t>(stream), debug_sync) : (int) hipSuccess;
    });
}

int mspmv_bicgstab_set_factor(mspmv_bicgstab_t *solver, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan, const void *d_factor_values,
                              const int32_t *d_row_offsets, const int32_t *d_column_indices)
{
    return krylov_set_factor(solver ? &solver->op : nullptr, first_plan, second_plan, d_factor_values, d_row_offsets, d_column_indices);
}

int mspmv_bicgstab_solve_f32(mspmv_bicgstab_t *solver, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                             const float *d_b, float *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                             int32_t check_every, float *d_history, mspmv_stream_t stream, int debug_sync)
{
    return bicg_solve<float>(solver, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                             d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_bicgstab_solve_f64(mspmv_bicgstab_t *solver, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                             const double *d_b, double *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                             int32_t check_every, double *d_history, mspmv_stream_t stream, int debug_sync)
{
    return bicg_solve<double>(solver, d_values, d_row_offsets, d_column_indices, d_b, d_x, use_x_as_guess, rtol, atol, max_iterations, check_every,
                              d_history, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_bicgstab_state(mspmv_bicgstab_t *solver, mspmv_bicgstab_state_t *state, mspmv_stream_t stream)
{
    if (!solver || !state) return hipErrorInvalidValue;
    *state = solver->h_state;
    if (solver->op.rows == 0) return hipSuccess;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return solver->op.value_bytes == 4 ? bicg_read<float>(solver, state, s) : bicg_read<double>(solver, state, s);
}

int mspmv_bicgstab_destroy(mspmv_bicgstab_t *solver) { return krylov_destroy(solver); }

}  // extern "C"
