// mspmv_csrsm.hip -- the sparse triangular solve for k right-hand sides (mspmv_csrsm_* of include/mspmv.h): op(A) X = alpha * B, A rows x
// rows in CSR, B and X rows x k row-major (the layout of Y in mspmv_csrmm_*).  The plan is a mspmv_csrsv_plan_t, used as made: the
// levels, order[] and level_offsets[] of mspmv_csrsv.hip; no analysis of its own.
//
// Values.  Column j of X is, bit for bit, what mspmv_csrsv_solve_* gives for column j of B: one lane adds one (row, right-hand side)
// sum, left to right in stored order, every operation rounded on its own.  Nothing depends on k, the leading dimensions, P or the
// schedule.
//
// Mapping.  P = the smallest power of two >= min(k, 64) adjacent lanes of one wave work one row; lane j of the group takes the
// right-hand sides j, j + 64, ... (each a pass of its own over the row); a lane with j >= k idles.  The group reads cols[e] and vals[e]
// at one address and gathers X[c, j .. j + P) in one coalesced request.  All index arithmetic on B and X is 64-bit.
//
// Schedule.  A level of n rows is narrow for this k when n * P <= narrow_lanes.  A maximal run of consecutive narrow levels is one
// launch of ONE workgroup that walks its levels (mspmv_levels.hpp: lv_walk_ahead; a thread takes the pairs (row, j) numbered tid,
// tid + 1024, ...: 1024 is a multiple of P, so its j never changes); every other level is one launch of ceil(n * P / 256) workgroups.
// The cut depends on P, so it is made from the plan's host copy of the level offsets while the solve walks them.  X is read and
// written by the same kernel: it is not __restrict__ and goes through the ordinary loads.  A solve allocates nothing, reads nothing
// back and launches the same kernels whatever the values.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

constexpr int SM_MAX_LANES = 64;            // the lanes of one row at most: one wave
// The lane budget up to which a level is narrow: the 256 lanes of csrsv's W = 256, so that k = 1 launches what csrsv launches.
// DESIGN.md 4 "Triangular solve, several right-hand sides" holds the sweep.
constexpr int SM_NARROW_LANES = 256;

// row r, its entries [e0, e1), the right-hand sides j, j + 64, ... < k, one pass each:
// s = +0; s = s + a[e] * X[c, jj] over the strict triangle in stored order; X[r, jj] = (alpha * B[r, jj] - s) [/ d]
template <typename V>
__device__ __forceinline__ void sm_row(int r, int e0, int e1, const V *__restrict__ vals, const int *__restrict__ cols, V alpha, const V *b,
                                       long long ldb, V *x, long long ldx, int j, int k, int upper, int unit)
{
    for (int jj = j; jj < k; jj += SM_MAX_LANES) {
        V s = V(0), d = V(1);
        for (int e = e0; e < e1; ++e) {
            const int c = cols[e];
            if (lv_strict(upper, r, c)) {
                const V p = vals[e] * x[(long long) c * ldx + jj];
                s = s + p;
            } else if (c == r) {
                d = vals[e];
            }
        }
        const V t = alpha * b[(long long) r * ldb + jj];
        V v = t - s;
        if (!unit) v = v / d;
        x[(long long) r * ldx + jj] = v;
    }
}

// one level, P = 1 << logp lanes per row: rows order[0 .. n)
template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void sm_level_kernel(const int *__restrict__ order, int n, const V *__restrict__ vals,
                                                            const int *__restrict__ off, const int *__restrict__ cols, V alpha, const V *b,
                                                            long long ldb, V *x, long long ldx, int k, int logp, int upper, int unit)
{
    const long long t = (long long) blockIdx.x * LV_BLOCK + threadIdx.x;
    const long long i = t >> logp;
    if (i >= n) return;
    const int j = (int) (t & ((1 << logp) - 1));
    const int r = order[i];
    int e0, e1;
    lv_bounds(off, r, e0, e1);
    sm_row<V>(r, e0, e1, vals, cols, alpha, b, ldb, x, ldx, j, k, upper, unit);
}

// levels [level_lo, level_hi), every one of at most narrow_lanes / P rows: ONE workgroup, a barrier between two levels.  Every trip
// count that encloses a barrier is the same in every thread, and no thread leaves early (a lane with j >= k has no pass to make).
template <typename V>
__global__ __launch_bounds__(LV_NARROW_BLOCK) void sm_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
                                                                    int level_lo, int level_hi, const V *__restrict__ vals,
                                                                    const int *__restrict__ off, const int *__restrict__ cols, V alpha,
                                                                    const V *b, long long ldb, V *x, long long ldx, int k, int logp, int upper,
                                                                    int unit)
{
    // pair tid + m * 1024 of a level is (row (tid >> logp) + m * (1024 >> logp), right-hand side tid & (P - 1))
    const int tid = (int) threadIdx.x, j = tid & ((1 << logp) - 1);
    lv_walk_ahead(order, level_offsets, level_lo, level_hi, off, tid >> logp, LV_NARROW_BLOCK >> logp,
                  [=](int r, int e0, int e1) { sm_row<V>(r, e0, e1, vals, cols, alpha, b, ldb, x, ldx, j, k, upper, unit); });
}

static int sm_narrow_lanes()
{
#ifdef MSPMV_TUNING
    // development library only: the sweep of tools/csrsm_bench.py
    if (const char *e = getenv("MSPMV_CSRSM_NARROW_LANES")) { const int w = atoi(e); if (w > 0) return w; }
#endif
    return SM_NARROW_LANES;
}

static int sm_log2_lanes(int k)
{
    int logp = 0;
    while ((1 << logp) < k && (1 << logp) < SM_MAX_LANES) ++logp;
    return logp;
}

template <typename V>
int sm_solve(mspmv_csrsv_plan *p, const V *vals, const int32_t *off, const int32_t *cols, V alpha, const V *b, int32_t ldb, V *x, int32_t ldx,
             int32_t k, hipStream_t stream, int debug_sync)
{
    if (!p || p->info.bad_diagonal_row >= 0) return hipErrorInvalidValue;
    if (k < 1 || ldb < k || ldx < k) return hipErrorInvalidValue;
    if (p->info.rows == 0) return hipSuccess;
    if (!b || !x || (p->info.nnz > 0 && (!vals || !off || !cols))) return hipErrorInvalidValue;
    const int upper = p->info.uplo == MSPMV_CSRSV_UPPER, unit = p->info.diag == MSPMV_CSRSV_UNIT;
    if (p->info.nnz == 0) { vals = nullptr; off = nullptr; cols = nullptr; }
    const int logp = sm_log2_lanes(k);
    const std::vector<int32_t> &lo = p->h_level_offsets;
    return mspmv_levels_cut(lo, logp, sm_narrow_lanes(), [&](int l, int m, bool narrow) -> int {
        if (narrow) {
            hipLaunchKernelGGL((sm_narrow_kernel<V>), dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, l, m, vals, off,
                               cols, alpha, b, (long long) ldb, x, (long long) ldx, k, logp, upper, unit);
            return lv_launched(stream, debug_sync, "sm_narrow_kernel", 1, LV_NARROW_BLOCK);
        }
        const int n = lo[m] - lo[l];
        const unsigned g = (unsigned) ((((long long) n << logp) + LV_BLOCK - 1) / LV_BLOCK);
        hipLaunchKernelGGL((sm_level_kernel<V>), dim3(g), dim3(LV_BLOCK), 0, stream, p->d_order + lo[l], n, vals, off, cols, alpha, b,
                           (long long) ldb, x, (long long) ldx, k, logp, upper, unit);
        return lv_launched(stream, debug_sync, "sm_level_kernel", g, LV_BLOCK);
    });
}

}  // namespace

extern "C" {

int mspmv_csrsm_info(const mspmv_csrsv_plan_t *plan, int32_t k, mspmv_csrsm_info_t *info)
{
    if (!plan || !info || k < 1) return hipErrorInvalidValue;
    const int logp = sm_log2_lanes(k);
    int launches = 0;
    info->k = k;
    info->lanes_per_row = 1 << logp;
    info->passes = (k + SM_MAX_LANES - 1) / SM_MAX_LANES;
    info->narrow_lanes = sm_narrow_lanes();
    (void) mspmv_levels_cut(plan->h_level_offsets, logp, info->narrow_lanes, [&](int, int, bool) -> int { ++launches; return 0; });
    info->launches = launches;
    return hipSuccess;
}

int mspmv_csrsm_solve_f32(mspmv_csrsv_plan_t *plan, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          float alpha, const float *d_b, int32_t ldb, float *d_x, int32_t ldx, int32_t k, mspmv_stream_t stream, int debug_sync)
{
    return sm_solve<float>(plan, d_values, d_row_offsets, d_column_indices, alpha, d_b, ldb, d_x, ldx, k, reinterpret_cast<hipStream_t>(stream),
                           debug_sync);
}
int mspmv_csrsm_solve_f64(mspmv_csrsv_plan_t *plan, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          double alpha, const double *d_b, int32_t ldb, double *d_x, int32_t ldx, int32_t k, mspmv_stream_t stream, int debug_sync)
{
    return sm_solve<double>(plan, d_values, d_row_offsets, d_column_indices, alpha, d_b, ldb, d_x, ldx, k, reinterpret_cast<hipStream_t>(stream),
                            debug_sync);
}

}  // extern "C"
