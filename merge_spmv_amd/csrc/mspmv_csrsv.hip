// mspmv_csrsv.hip -- the sparse triangular solve on the device (mspmv_csrsv_* of include/mspmv.h): op(A) x = alpha * b for one
// right-hand side, A rows x rows in CSR, the triangle and the diagonal chosen by uplo / diag, everything else in A ignored.
//
// Scheme: level scheduling.  level[r] = 0 for a row without entries in the strict triangle, else 1 + the largest level among the rows
// those entries name.  The rows of one level depend only on rows of lower levels, so a level is solved by independent lanes, and the
// levels are ordered by launch order or, inside one workgroup, by a workgroup barrier -- by nothing else.  No flags, no spinning, no
// cooperative launch: no workgroup ever depends on another one's progress.
//
// Analysis (mspmv_csrsv_plan_create; the pattern alone).
//   1. A^T's pattern by the structure-only device transpose (mspmv_csr_transpose_*): for a row c, the rows that name c.
//   2. One lane per row counts the row's strict-triangle entries (the in-degree; a repeated column counts twice, here and in A^T)
//      and its stored diagonals; rows of in-degree 0 are the first frontier.
//   3. Peeling: every row c of the frontier takes one from the count of every row r > c (LOWER; r < c for UPPER) that names it; the
//      row whose count reaches 0 gets level + 1 and joins the next frontier.  Integer atomics; the order in which rows arrive in a
//      frontier is discarded.  While the frontier has at most SV_PEEL_CAP rows, ONE workgroup peels level after level with a barrier
//      between them (a chain of 65536 rows is one launch, not 65536 launches and read-backs); a larger frontier is one launch of many
//      workgroups, after which the host reads the next frontier's size back (32 bytes per step).
//   4. order[] = the rows sorted stably by level and level_offsets[] are the transpose of the rows x levels pattern that has the one
//      entry (r, level[r]) in row r: the same radix passes, so both are functions of the pattern alone.
//   5. The host reads level_offsets once and cuts the levels into segments (below); the scratch is freed.
//
// Solve.  One lane adds one row's sum, left to right in stored order, every operation rounded on its own; x[r] is a function of the
// row's entries, the x of its dependencies, alpha and b[r] alone.  A maximal run of levels of at most W rows each is one launch of ONE
// workgroup that walks its levels (mspmv_levels.hpp: lv_walk_ahead; a thread takes rows tid, tid + 1024, ...); every other level is
// one launch of ceil(rows of the level / 256) workgroups.  x is read and written by the same kernel: it is not __restrict__ and goes
// through the ordinary loads.  A solve allocates nothing, reads nothing back and launches the same kernels whatever the values.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"

#include "mspmv_radix.hpp"     // tr_fill_kernel

constexpr int SV_PEEL_CAP = 4096;           // analysis: a frontier of at most this many rows is peeled inside one workgroup
// W, the rows up to which a level is narrow.  Measured (profiles/csrsv_bench.txt, the sweep; DESIGN.md 4 "Triangular solve"), fp64, W =
// 64 / 256 / 1024 / 2048 / 4096: the lower part of a 5-point grid of 2000 x 2000 16.6 / 16.2 / 18.9 / 39.0 / 39.0 ms, of a 7-point grid of
// 128^3 2.15 / 2.12 / 2.23 / 2.79 / 4.72 ms: a level of a few hundred rows is cheaper as a launch of its own than as one more barrier
// of one workgroup, whose lanes then take several rows each on one CU.
constexpr int SV_NARROW_ROWS = 256;

enum { ST_COUNT = 0, ST_BAD = 1, ST_USED = 2 /* and 3 */, ST_NEXT = 4, ST_LEVEL = 5, ST_WHICH = 6, ST_WORDS = 8 };

// ---- analysis ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sv_iota_kernel(int *__restrict__ out, long long n)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int) i;
}

// one lane per row: the strict-triangle entries (in-degree) and the stored diagonals; rows of in-degree 0 are level 0
__global__ __launch_bounds__(256) void sv_count_kernel(const int *__restrict__ off, const int *__restrict__ cols, int rows, int upper,
                                                       int nonunit, int *__restrict__ indeg, int *__restrict__ level,
                                                       int *__restrict__ frontier, int *__restrict__ state)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int r = (int) i;
    int deg = 0, dg = 0;
    for (int e = off[r], e1 = off[r + 1]; e < e1; ++e) {
        const int c = cols[e];
        deg += lv_strict(upper, r, c) ? 1 : 0;
        dg += c == r ? 1 : 0;
    }
    indeg[r] = deg;
    if (deg == 0) {
        level[r] = 0;
        frontier[atomicAdd(&state[ST_COUNT], 1)] = r;
    } else {
        atomicAdd(reinterpret_cast<unsigned long long *>(state + ST_USED), (unsigned long long) deg);
    }
    if (nonunit && dg != 1) atomicMin(reinterpret_cast<unsigned *>(state + ST_BAD), (unsigned) r);
}

__device__ __forceinline__ void sv_release_one(int r, int c, int upper, int *__restrict__ indeg, int *__restrict__ level, int lvl,
                                               int *next, int *next_count)
{
    if (!lv_strict(upper, r, c)) return;
    if (atomicSub(&indeg[r], 1) == 1) {
        level[r] = lvl + 1;
        next[atomicAdd(next_count, 1)] = r;
    }
}

// All 64 lanes of a wave come here together, each with a finished row c of level lvl (or none): every row that names c in its strict
// triangle loses one from its count, and the one whose count reaches 0 joins the next frontier.  A row of A^T of 64 entries or more
// is walked by the whole wave (lanes taking turns by ballot), so that a hub column costs no single lane a long loop.
__device__ __forceinline__ void sv_release(bool have, int c, const int *__restrict__ off_t, const int *__restrict__ cols_t, int upper,
                                           int *__restrict__ indeg, int *__restrict__ level, int lvl, int *next,
                                           int *next_count)
{
    const int lane = (int) threadIdx.x & 63;
    int e0 = 0, e1 = 0;
    if (have) { e0 = off_t[c]; e1 = off_t[c + 1]; }
    const bool longrow = e1 - e0 >= 64;
    if (!longrow)
        for (int e = e0; e < e1; ++e) sv_release_one(cols_t[e], c, upper, indeg, level, lvl, next, next_count);
    unsigned long long todo = __ballot(longrow);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int sc = __shfl(c, src, 64), s0 = __shfl(e0, src, 64), s1 = __shfl(e1, src, 64);
        for (int e = s0 + lane; e < s1; e += 64) sv_release_one(cols_t[e], sc, upper, indeg, level, lvl, next, next_count);
    }
}

// one level, many workgroups: the frontier `cur` of n rows at level lvl -> `next`, counted in *next_count (zero on entry)
__global__ __launch_bounds__(256) void sv_peel_wide_kernel(const int *__restrict__ off_t, const int *__restrict__ cols_t, int upper,
                                                           int *__restrict__ indeg, int *__restrict__ level,
                                                           const int *__restrict__ cur, int *__restrict__ next, int n, int lvl,
                                                           int *__restrict__ next_count)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    sv_release(have, have ? cur[i] : 0, off_t, cols_t, upper, indeg, level, lvl, next, next_count);
}

// ONE workgroup: level after level, while the frontier is neither empty nor larger than cap; a barrier between two levels.  On exit
// state[ST_NEXT] = the size of the frontier it stopped at, state[ST_LEVEL] = that frontier's level, state[ST_WHICH] = 1 when it lies
// in f1.  The frontier arrays are not __restrict__: what one level writes the next one reads.
__global__ __launch_bounds__(LV_NARROW_BLOCK) void sv_peel_narrow_kernel(const int *__restrict__ off_t, const int *__restrict__ cols_t,
                                                                         int upper, int *__restrict__ indeg, int *__restrict__ level,
                                                                         int *f0, int *f1, int n, int lvl, int cap,
                                                                         int *__restrict__ state)
{
    __shared__ int s_next;
    const int tid = (int) threadIdx.x;
    int *cur = f0, *next = f1;
    do {                                                            // (n and lvl are the same in every thread)
        if (tid == 0) s_next = 0;
        __syncthreads();
        for (int base = 0; base < n; base += LV_NARROW_BLOCK) {
            const bool have = base + tid < n;
            sv_release(have, have ? cur[base + tid] : 0, off_t, cols_t, upper, indeg, level, lvl, next, &s_next);
        }
        __threadfence_block();
        __syncthreads();
        n = s_next;
        ++lvl;
        int *t = cur; cur = next; next = t;
        __syncthreads();                                            // (everyone has read s_next before it is cleared)
    } while (n > 0 && n <= cap);
    if (tid == 0) { state[ST_NEXT] = n; state[ST_LEVEL] = lvl; state[ST_WHICH] = cur == f1 ? 1 : 0; }
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------
// row r, its entries [e0, e1): s = +0; s = s + a[e] * x[c] over the strict triangle in stored order; x[r] = (alpha * b[r] - s) [/ d]
template <typename V>
__device__ __forceinline__ void sv_row(int r, int e0, int e1, const V *__restrict__ vals, const int *__restrict__ cols, V alpha, const V *b,
                                       V *x, int upper, int unit)
{
    V s = V(0), d = V(1);
    for (int e = e0; e < e1; ++e) {
        const int c = cols[e];
        if (lv_strict(upper, r, c)) {
            const V p = vals[e] * x[c];
            s = s + p;
        } else if (c == r) {
            d = vals[e];
        }
    }
    const V t = alpha * b[r];
    V v = t - s;
    if (!unit) v = v / d;
    x[r] = v;
}

// one level (or a stretch of one), one lane per row: rows order[0 .. n)
template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void sv_level_kernel(const int *__restrict__ order, int n, const V *__restrict__ vals,
                                                            const int *__restrict__ off, const int *__restrict__ cols, V alpha, const V *b,
                                                            V *x, int upper, int unit)
{
    const long long i = (long long) blockIdx.x * LV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int r = order[i];
    int e0, e1;
    lv_bounds(off, r, e0, e1);
    sv_row<V>(r, e0, e1, vals, cols, alpha, b, x, upper, unit);
}

// levels [level_lo, level_hi), every one of at most W rows: ONE workgroup, a barrier between two levels.  Every trip count that
// encloses a barrier is the same in every thread.
template <typename V>
__global__ __launch_bounds__(LV_NARROW_BLOCK) void sv_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
                                                                    int level_lo, int level_hi, const V *__restrict__ vals,
                                                                    const int *__restrict__ off, const int *__restrict__ cols, V alpha,
                                                                    const V *b, V *x, int upper, int unit)
{
    const int tid = (int) threadIdx.x;
    lv_walk_ahead(order, level_offsets, level_lo, level_hi, off, tid, LV_NARROW_BLOCK,
                  [=](int r, int e0, int e1) { sv_row<V>(r, e0, e1, vals, cols, alpha, b, x, upper, unit); });
}

static int sv_read(void *h, const void *d, size_t bytes, hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return (int) e;
}

static int sv_narrow_rows()
{
#ifdef MSPMV_TUNING
    // development library only: the sweep of tools/csrsv_bench.py
    if (const char *e = getenv("MSPMV_CSRSV_NARROW_ROWS")) { const int w = atoi(e); if (w > 0) return w; }
#endif
    return SV_NARROW_ROWS;
}

// the launches of one solve from the level offsets: the cut for one lane per row and W rows
static void sv_segments(mspmv_csrsv_plan &p, const std::vector<int32_t> &lo)
{
    p.segments.clear();
    p.info.max_level_rows = 0;
    (void) mspmv_levels_cut(lo, 0, p.info.narrow_rows, [&](int l, int m, bool narrow) {
        p.segments.push_back({l, m, lo[l], lo[m], narrow});
        return 0;
    });
    for (int l = 0; l < p.info.levels; ++l) p.info.max_level_rows = std::max(p.info.max_level_rows, lo[l + 1] - lo[l]);
    p.info.launches = (int32_t) p.segments.size();
}

struct SvScratch {
    char *base = nullptr;
    ~SvScratch() { if (base) (void) hipFree(base); }
};

static int sv_analyse(mspmv_csrsv_plan &p, const int32_t *d_off, const int32_t *d_cols, hipStream_t stream, int debug_sync)
{
    const int rows = p.info.rows, nnz = p.info.nnz, upper = p.info.uplo == MSPMV_CSRSV_UPPER, nonunit = p.info.diag == MSPMV_CSRSV_NON_UNIT;
    mspmv_stream_t cstream = reinterpret_cast<mspmv_stream_t>(stream);
    const unsigned rgrid = grid_for(rows, 256);
    if (hipMalloc(reinterpret_cast<void **>(&p.d_order), (size_t) rows * 4) != hipSuccess) return hipErrorOutOfMemory;
    p.info.device_bytes = (uint64_t) rows * 4;
    std::vector<int32_t> h_lo;
    if (nnz == 0) {
        // every row is level 0; without a stored diagonal, row 0 is already a bad one
        hipLaunchKernelGGL(sv_iota_kernel, dim3(rgrid), dim3(256), 0, stream, p.d_order, (long long) rows);
        if (int e = lv_launched(stream, debug_sync, "sv_iota_kernel", rgrid, 256)) return e;
        p.info.levels = 1;
        p.info.bad_diagonal_row = nonunit ? 0 : -1;
        h_lo = {0, rows};
    } else {
        size_t tb1 = 0, tb2 = 0;
        if (int e = mspmv_csr_transpose_f32(nullptr, &tb1, nullptr, nullptr, nullptr, rows, rows, nnz, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) return e;
        if (int e = mspmv_csr_transpose_f32(nullptr, &tb2, nullptr, nullptr, nullptr, rows, rows, rows, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) return e;
        const uint64_t n4 = align256((uint64_t) rows * 4 + 4);
        uint64_t o = 0;
        const uint64_t state_off = o; o += 256;
        const uint64_t offt_off = o; o += n4;
        const uint64_t colst_off = o; o += align256((uint64_t) nnz * 4);
        const uint64_t indeg_off = o; o += n4;
        const uint64_t level_off = o; o += n4;
        const uint64_t f0_off = o; o += n4;
        const uint64_t f1_off = o; o += n4;
        const uint64_t iota_off = o; o += n4;
        const uint64_t temp_off = o; o += align256(std::max(tb1, tb2));
        SvScratch S;
        if (hipMalloc(reinterpret_cast<void **>(&S.base), o) != hipSuccess) return hipErrorOutOfMemory;
        int *state = reinterpret_cast<int *>(S.base + state_off), *off_t = reinterpret_cast<int *>(S.base + offt_off);
        int *cols_t = reinterpret_cast<int *>(S.base + colst_off), *indeg = reinterpret_cast<int *>(S.base + indeg_off);
        int *level = reinterpret_cast<int *>(S.base + level_off), *iota = reinterpret_cast<int *>(S.base + iota_off);
        int *f[2] = {reinterpret_cast<int *>(S.base + f0_off), reinterpret_cast<int *>(S.base + f1_off)};
        void *temp = S.base + temp_off;
        // 1. the pattern of A^T
        size_t tb = tb1;
        if (int e = mspmv_csr_transpose_f32(temp, &tb, nullptr, d_off, d_cols, rows, rows, nnz, nullptr, off_t, cols_t, nullptr, cstream, debug_sync)) return e;
        // 2. in-degrees, diagonals, the first frontier
        if (hipMemsetAsync(state, 0, ST_WORDS * 4, stream) != hipSuccess) return hipErrorInvalidValue;
        if (hipMemsetAsync(state + ST_BAD, 0xff, 4, stream) != hipSuccess) return hipErrorInvalidValue;
        hipLaunchKernelGGL(sv_count_kernel, dim3(rgrid), dim3(256), 0, stream, d_off, d_cols, rows, upper, nonunit, indeg, level, f[0], state);
        if (int e = lv_launched(stream, debug_sync, "sv_count_kernel", rgrid, 256)) return e;
        int h[ST_WORDS];
        if (int e = sv_read(h, state, sizeof(h), stream)) return e;
        p.info.bad_diagonal_row = (unsigned) h[ST_BAD] == 0xffffffffu ? -1 : h[ST_BAD];
        p.info.used_entries = (int64_t) ((uint64_t) (unsigned) h[ST_USED] | (uint64_t) (unsigned) h[ST_USED + 1] << 32);
        // 3. peel
        int n = h[ST_COUNT], lvl = 0, which = 0;
        long long done = 0;
        while (n > 0) {
            done += n;
            if (n <= SV_PEEL_CAP) {
                hipLaunchKernelGGL(sv_peel_narrow_kernel, dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, off_t, cols_t, upper, indeg, level, f[which],
                                   f[which ^ 1], n, lvl, SV_PEEL_CAP, state);
                if (int e = lv_launched(stream, debug_sync, "sv_peel_narrow_kernel", 1, LV_NARROW_BLOCK)) return e;
                if (int e = sv_read(h, state, sizeof(h), stream)) return e;
                n = h[ST_NEXT]; lvl = h[ST_LEVEL]; which ^= h[ST_WHICH];
            } else {
                const unsigned g = grid_for(n, 256);
                if (hipMemsetAsync(state + ST_NEXT, 0, 4, stream) != hipSuccess) return hipErrorInvalidValue;
                hipLaunchKernelGGL(sv_peel_wide_kernel, dim3(g), dim3(256), 0, stream, off_t, cols_t, upper, indeg, level, f[which], f[which ^ 1], n,
                                   lvl, state + ST_NEXT);
                if (int e = lv_launched(stream, debug_sync, "sv_peel_wide_kernel", g, 256)) return e;
                if (int e = sv_read(h, state, sizeof(h), stream)) return e;
                n = h[ST_NEXT]; ++lvl; which ^= 1;
            }
        }
        (void) done;
        p.info.levels = lvl;
        // 4. the rows sorted stably by level, and where each level starts: the transpose of the pattern {(r, level[r])}
        if (hipMalloc(reinterpret_cast<void **>(&p.d_level_offsets), ((size_t) lvl + 1) * 4) != hipSuccess) return hipErrorOutOfMemory;
        p.info.device_bytes += ((uint64_t) lvl + 1) * 4;
        const unsigned igrid = grid_for((long long) rows + 1, 256);
        hipLaunchKernelGGL(sv_iota_kernel, dim3(igrid), dim3(256), 0, stream, iota, (long long) rows + 1);
        if (int e = lv_launched(stream, debug_sync, "sv_iota_kernel", igrid, 256)) return e;
        tb = tb2;
        if (int e = mspmv_csr_transpose_f32(temp, &tb, nullptr, iota, level, rows, lvl, rows, nullptr, p.d_level_offsets, p.d_order, nullptr, cstream,
                                            debug_sync))
            return e;
        h_lo.resize((size_t) lvl + 1);
        if (int e = sv_read(h_lo.data(), p.d_level_offsets, h_lo.size() * 4, stream)) return e;
    }
    if (!p.d_level_offsets) {
        if (hipMalloc(reinterpret_cast<void **>(&p.d_level_offsets), h_lo.size() * 4) != hipSuccess) return hipErrorOutOfMemory;
        p.info.device_bytes += h_lo.size() * 4;
        if (hipMemcpyAsync(p.d_level_offsets, h_lo.data(), h_lo.size() * 4, hipMemcpyHostToDevice, stream) != hipSuccess) return hipErrorInvalidValue;
    }
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorInvalidValue;
    sv_segments(p, h_lo);
    p.h_level_offsets = std::move(h_lo);                            // (kept for mspmv_csrsm_*, whose cut depends on k)
    return hipSuccess;
}

template <typename V>
int sv_solve(mspmv_csrsv_plan *p, const V *vals, const int32_t *off, const int32_t *cols, V alpha, const V *b, V *x, hipStream_t stream,
             int debug_sync)
{
    if (!p || p->info.bad_diagonal_row >= 0) return hipErrorInvalidValue;
    if (p->info.rows == 0) return hipSuccess;
    if (!b || !x || (p->info.nnz > 0 && (!vals || !off || !cols))) return hipErrorInvalidValue;
    const int upper = p->info.uplo == MSPMV_CSRSV_UPPER, unit = p->info.diag == MSPMV_CSRSV_UNIT;
    if (p->info.nnz == 0) { vals = nullptr; off = nullptr; cols = nullptr; }
    for (const mspmv_csrsv_plan::Segment &s : p->segments) {
        if (s.narrow) {
            hipLaunchKernelGGL((sv_narrow_kernel<V>), dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, s.level_lo,
                               s.level_hi, vals, off, cols, alpha, b, x, upper, unit);
            if (int e = lv_launched(stream, debug_sync, "sv_narrow_kernel", 1, LV_NARROW_BLOCK)) return e;
        } else {
            const int n = s.row_hi - s.row_lo;
            const unsigned g = grid_for(n, LV_BLOCK);
            hipLaunchKernelGGL((sv_level_kernel<V>), dim3(g), dim3(LV_BLOCK), 0, stream, p->d_order + s.row_lo, n, vals, off, cols, alpha, b, x, upper,
                               unit);
            if (int e = lv_launched(stream, debug_sync, "sv_level_kernel", g, LV_BLOCK)) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int mspmv_csrsv_plan_create(mspmv_csrsv_plan_t **plan, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                            int32_t uplo, int32_t diag, mspmv_stream_t stream, int debug_sync)
{
    if (!plan) return hipErrorInvalidValue;
    *plan = nullptr;
    if (rows < 0 || nnz < 0 || (long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    if ((uplo != MSPMV_CSRSV_LOWER && uplo != MSPMV_CSRSV_UPPER) || (diag != MSPMV_CSRSV_NON_UNIT && diag != MSPMV_CSRSV_UNIT)) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || !d_row_offsets || !d_column_indices)) return hipErrorInvalidValue;
    mspmv_csrsv_plan *p = new (std::nothrow) mspmv_csrsv_plan;
    if (!p) return hipErrorOutOfMemory;
    p->info.rows = rows; p->info.nnz = nnz; p->info.uplo = uplo; p->info.diag = diag;
    p->info.narrow_rows = sv_narrow_rows();
    p->info.bad_diagonal_row = -1;
    if (rows > 0) {
        if (int e = sv_analyse(*p, d_row_offsets, d_column_indices, reinterpret_cast<hipStream_t>(stream), debug_sync)) {
            (void) hipGetLastError();
            (void) mspmv_csrsv_plan_destroy(p);
            return e;
        }
    }
    *plan = p;
    return hipSuccess;
}

int mspmv_csrsv_plan_info(const mspmv_csrsv_plan_t *plan, mspmv_csrsv_info_t *info)
{
    if (!plan || !info) return hipErrorInvalidValue;
    *info = plan->info;
    return hipSuccess;
}

const int32_t *mspmv_csrsv_plan_order(const mspmv_csrsv_plan_t *plan) { return plan ? plan->d_order : nullptr; }
const int32_t *mspmv_csrsv_plan_level_offsets(const mspmv_csrsv_plan_t *plan) { return plan ? plan->d_level_offsets : nullptr; }

int mspmv_csrsv_solve_f32(mspmv_csrsv_plan_t *plan, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          float alpha, const float *d_b, float *d_x, mspmv_stream_t stream, int debug_sync)
{
    return sv_solve<float>(plan, d_values, d_row_offsets, d_column_indices, alpha, d_b, d_x, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csrsv_solve_f64(mspmv_csrsv_plan_t *plan, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          double alpha, const double *d_b, double *d_x, mspmv_stream_t stream, int debug_sync)
{
    return sv_solve<double>(plan, d_values, d_row_offsets, d_column_indices, alpha, d_b, d_x, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_csrsv_plan_destroy(mspmv_csrsv_plan_t *plan)
{
    if (!plan) return hipErrorInvalidValue;
    if (plan->d_order) (void) hipFree(plan->d_order);
    if (plan->d_level_offsets) (void) hipFree(plan->d_level_offsets);
    delete plan;
    return hipSuccess;
}

}  // extern "C"
