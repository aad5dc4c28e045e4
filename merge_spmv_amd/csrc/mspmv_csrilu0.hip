// mspmv_csrilu0.hip -- the incomplete LU factorisation without fill-in on the device (mspmv_csrilu0_* of include/mspmv.h): A ~ L U on
// A's own pattern, L's unit diagonal implied, "nothing extracted": the layout the LOWER+UNIT and UPPER+NON_UNIT solves of
// mspmv_csrsv_* sweep.
//
// Scheme: the level schedule of the LOWER triangular solve.  Row i of the row-wise (IKJ) elimination needs the FINISHED rows k whose
// column is stored in its strict lower part -- the dependency graph of L x = b -- so a LOWER mspmv_csrsv_plan_t already holds the
// analysis: order[], level_offsets[] and the segments.  A maximal run of narrow levels is ONE workgroup of 1024 threads that walks its
// levels with __syncthreads() between them; every other level is one launch of many workgroups.  mspmv_levels.hpp holds what is not
// ILU(0)'s own: the prologue that finds the diagonals (dpos), the lane-group body of a wide level and the host path.
//
// A row is worked by a GROUP of G consecutive lanes of one wave (G a power of two, a function of rows and nnz alone).  Lane l of the
// group OWNS the entries e0 + l, e0 + l + G, ... of the row: only that lane ever reads or writes them while the row is worked, so no
// lane needs to see another lane's store and no memory-ordering question arises inside a level.  For each strict-lower entry e, in
// stored order, the owning lane divides by the pivot (the final diagonal of row k = col[e], read from memory: row k belongs to an
// earlier level) and stores the quotient; the group gets it by __shfl(q, e - e0, G); then every lane looks each of its owned entries
// behind e up in row k's sorted upper part by bisection and subtracts on a hit.  Every update of an entry a[g] comes from a different e,
// and they arrive in ascending e: the order the definition states.
// The loop over the lower entries holds a shuffle, so EVERY lane of the wave stays in it: its trip count is the wave's largest (a
// ballot), a lane whose row is shorter -- or that has no row -- runs it with `on` false.  No lane returns early anywhere.
// The values are read and written by the same kernel: they are not __restrict__ and go through the ordinary loads.
//
// On input that is not sorted the values are unspecified, but every position used is one a bisection inside [off[r], off[r + 1]]
// returned, so nothing outside the arrays is touched and every loop ends.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

// All 64 lanes of a wave come here together; the G lanes of a group share `have` and the row i.  gl = the lane's place in its group.
template <typename V>
__device__ __forceinline__ void ilu_row(bool have, int i, int G, int gl, const int *__restrict__ off, const int *__restrict__ cols,
                                        const int *__restrict__ dpos, V *a, unsigned *__restrict__ pivot)
{
    int e0 = 0, e1 = 0, lo_end = 0;
    bool diag = false;
    if (have && off) {
        e0 = off[i]; e1 = off[i + 1];
        const int d = dpos[i];
        diag = d >= 0;
        lo_end = diag ? d : ~d;
    }
    const int nlow = lo_end - e0;
    for (int t = 0; __ballot(t < nlow) != 0ull; ++t) {               // (the same trip count in every lane of the wave)
        const bool on = t < nlow;
        const int e = e0 + t;
        V q = V(0);
        int u0 = 0, u1 = 0;
        if (on) {
            const int k = cols[e];
            const int dk = dpos[k];
            u0 = dk >= 0 ? dk + 1 : ~dk;                             // row k's entries behind its diagonal
            u1 = off[k + 1];
            if ((t & (G - 1)) == gl) {                               // the owner of a[e]
                const V piv = dk >= 0 ? a[dk] : V(0);
                q = a[e] / piv;
                a[e] = q;
            }
        }
        q = __shfl(q, t & (G - 1), G);
        if (on && u0 < u1) {
            // this lane's entries behind e: e0 + r for r = gl (mod G), r > t
            for (int g = e + 1 + ((gl - t - 1) & (G - 1)); g < e1; g += G) {
                const int j = cols[g];
                const int f = lv_lower_bound(cols, u0, u1, j);
                if (f < u1 && cols[f] == j) {
                    const V p = q * a[f];
                    a[g] = a[g] - p;
                }
            }
        }
    }
    if (pivot && diag && (nlow & (G - 1)) == gl && a[lo_end] == V(0)) atomicMin(pivot, (unsigned) i);
}

template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void ilu0_prologue_kernel(const V *vals, V *lu, const int *__restrict__ off, const int *__restrict__ cols,
                                                                 int rows, int nnz, int *__restrict__ dpos, unsigned *__restrict__ pivot)
{
    lv_prologue<V>(vals, lu, off, cols, rows, nnz, dpos, pivot);
}

template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void ilu0_level_kernel(const int *__restrict__ order, int n, int G, const int *__restrict__ off,
                                                              const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                              unsigned *__restrict__ pivot)
{
    lv_level_groups(order, n, G, [=](bool have, int i, int gl) { ilu_row<V>(have, i, G, gl, off, cols, dpos, a, pivot); });
}

// levels [level_lo, level_hi), every one narrow: ONE workgroup, a barrier between two levels.  Every trip count that encloses a
// barrier or a shuffle is the same in every thread.  (The twin of ic0_narrow_kernel of mspmv_csric0.hip:
// mspmv_levels.hpp says why the two are not one.)
template <typename V>
__global__ __launch_bounds__(LV_NARROW_BLOCK) void ilu0_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
                                                                      int level_lo, int level_hi, int G, const int *__restrict__ off,
                                                                      const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                                      unsigned *__restrict__ pivot)
{
    __shared__ int s_lo[LV_LEVEL_CHUNK + 1];
    const int tid = (int) threadIdx.x, grp = tid / G, gl = tid & (G - 1), per_pass = LV_NARROW_BLOCK / G;
    for (int base = level_lo; base < level_hi; base += LV_LEVEL_CHUNK) {
        const int n = min(LV_LEVEL_CHUNK, level_hi - base);
        for (int i = tid; i <= n; i += LV_NARROW_BLOCK) s_lo[i] = level_offsets[base + i];
        __syncthreads();
        for (int l = 0; l < n; ++l) {
            const int hi = s_lo[l + 1];
            for (int first = s_lo[l]; first < hi; first += per_pass) {
                const int idx = first + grp;
                const bool have = idx < hi;
                ilu_row<V>(have, have ? order[idx] : 0, G, gl, off, cols, dpos, a, pivot);
            }
            __syncthreads();                                        // level l's rows are finished before level l + 1 reads them
        }
        // (the barrier that ended the last level also ends the reads of s_lo)
    }
}

// G for the mean row length.  Measured (profiles/csrilu0_bench.txt, the sweep; DESIGN.md 4 "ILU(0)"), fp64, G = 1 / 2 / 4 / 8 / 16 / 32 / 64:
// a 5-point grid of 2000 x 2000 (the rule: 8) 45.9 / 30.4 / 26.3 / 26.7 / 28.4 / 32.0 / 40.9 ms, a 7-point grid of 128^3 (the rule: 8)
// 6.53 / 4.13 / 3.33 / 3.12 / 3.35 / 3.88 / 5.49 ms.
static int ilu_group(int32_t rows, int32_t nnz)
{
    return lv_group(rows > 0 ? ((long long) nnz + rows - 1) / rows : 1, "MSPMV_CSRILU0_GROUP");
}

template <typename V>
int ilu_factor(const mspmv_csrsv_plan *p, void *d_temp, size_t *temp_bytes, const V *vals, V *lu, const int32_t *off, const int32_t *cols,
               int32_t *d_pivot, hipStream_t stream, int debug_sync)
{
    return lv_factor<V>(
        p, d_temp, temp_bytes, vals, lu, off, cols, d_pivot, stream, ilu_group,
        [&](const LvFactor<V> &f, unsigned grid) {
            hipLaunchKernelGGL((ilu0_prologue_kernel<V>), dim3(grid), dim3(LV_BLOCK), 0, stream, f.vals, f.out, f.off, f.cols, f.rows, f.nnz, f.dpos,
                               f.pivot);
            return lv_launched(stream, debug_sync, "ilu0_prologue_kernel", grid, LV_BLOCK, f.G);
        },
        [&](const LvFactor<V> &f, const mspmv_csrsv_plan::Segment &s) {
            hipLaunchKernelGGL((ilu0_narrow_kernel<V>), dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, s.level_lo,
                               s.level_hi, f.G, f.off, f.cols, f.dpos, f.out, f.pivot);
            return lv_launched(stream, debug_sync, "ilu0_narrow_kernel", 1, LV_NARROW_BLOCK, f.G);
        },
        [&](const LvFactor<V> &f, const mspmv_csrsv_plan::Segment &s, unsigned grid) {
            hipLaunchKernelGGL((ilu0_level_kernel<V>), dim3(grid), dim3(LV_BLOCK), 0, stream, p->d_order + s.row_lo, s.row_hi - s.row_lo, f.G, f.off,
                               f.cols, f.dpos, f.out, f.pivot);
            return lv_launched(stream, debug_sync, "ilu0_level_kernel", grid, LV_BLOCK, f.G);
        },
        [](const LvFactor<V> &) { return 0; });
}

}  // namespace

extern "C" {

int mspmv_csrilu0_group(int32_t rows, int32_t nnz, int32_t *lanes_per_row)
{
    if (rows < 0 || nnz < 0 || !lanes_per_row) return hipErrorInvalidValue;
    *lanes_per_row = ilu_group(rows, nnz);
    return hipSuccess;
}

int mspmv_csrilu0_f32(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const float *d_values, float *d_values_lu,
                      const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t *d_pivot, mspmv_stream_t stream, int debug_sync)
{
    return ilu_factor<float>(lower_plan, d_temp, temp_bytes, d_values, d_values_lu, d_row_offsets, d_column_indices, d_pivot,
                             reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csrilu0_f64(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const double *d_values, double *d_values_lu,
                      const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t *d_pivot, mspmv_stream_t stream, int debug_sync)
{
    return ilu_factor<double>(lower_plan, d_temp, temp_bytes, d_values, d_values_lu, d_row_offsets, d_column_indices, d_pivot,
                              reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
