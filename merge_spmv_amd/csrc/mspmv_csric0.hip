// mspmv_csric0.hip -- the incomplete Cholesky factorisation without fill-in on the device (mspmv_csric0_* of include/mspmv.h): A ~ L L^T
// on the pattern of A's lower triangle, L in the lower triangle and on the diagonal of A's own layout; with mirror == 1 one more launch
// writes L^T into the upper triangle, so that the array is L\L^T and the LOWER + NON_UNIT and UPPER + NON_UNIT solves of mspmv_csrsv_*
// sweep it with nothing extracted and nothing transposed.
//
// Scheme: the level schedule of the LOWER triangular solve, as in mspmv_csrilu0.hip.  Row i of the row-wise Cholesky needs the FINISHED
// rows whose column is stored in its strict lower part -- the dependency graph of L x = b -- so a LOWER mspmv_csrsv_plan_t already
// holds the analysis.  A maximal run of narrow levels is ONE workgroup of 1024 threads that walks its levels with __syncthreads()
// between them; every other level is one launch of many workgroups.  mspmv_levels.hpp holds what is not IC(0)'s own: the prologue
// that finds the diagonals (dpos), the lane-group body of a wide level and the host path.
//
// A row is worked by a GROUP of G consecutive lanes of one wave (G a power of two, a function of rows and nnz alone).  Lane l of the
// group OWNS the entries e0 + l, e0 + l + G, ... of the row UP TO AND INCLUDING THE DIAGONAL: only that lane ever reads or writes them
// while the row is worked, so no lane needs to see another lane's store and no memory-ordering question arises inside a level.  For
// each strict-lower entry e (column j), in stored order, the owning lane divides by the pivot (the final, rooted diagonal of row j, read
// from memory: row j belongs to an earlier level) and stores the quotient; the group gets it by __shfl(q, e - e0, G); then every lane
// takes its owned entries g behind e: the diagonal loses q * q, an entry of column k < i looks column j up in row k's strict lower
// part [off[k], dpos(k)) by bisection and loses q * a[f] on a hit.  Every update of an entry a[g] comes from a different e, and they
// arrive in ascending e: the order the definition states.  After the loop the diagonal's owner tests <= 0 for the pivot and takes the
// root.  Entries behind the diagonal are never touched here.
// The loop over the lower entries holds a shuffle, so EVERY lane of the wave stays in it: its trip count is the wave's largest (a
// ballot), a lane whose row is shorter -- or that has no row -- runs it with `on` false.  No lane returns early anywhere.
// The values are read and written by the same kernel: they are not __restrict__ and go through the ordinary loads.
//
// Mirror epilogue (one launch, mirror == 1): a group per row walks the entries behind the diagonal; entry (i, j), j > i, bisects row
// j's strict lower part for column i and receives that value, or +0.0 when row j does not store it.  It reads only lower entries and
// writes only upper ones, so the order of its rows does not matter.
//
// On input that is not sorted the values are unspecified, but every position used is one a bisection inside [off[r], off[r + 1]]
// returned, so nothing outside the arrays is touched and every loop ends.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

// the compiler's correctly rounded roots (no fast-math in this file)
__device__ __forceinline__ float ic_root(float v) { return sqrtf(v); }
__device__ __forceinline__ double ic_root(double v) { return sqrt(v); }

// All 64 lanes of a wave come here together; the G lanes of a group share `have` and the row i.  gl = the lane's place in its group.
template <typename V>
__device__ __forceinline__ void ic_row(bool have, int i, int G, int gl, const int *__restrict__ off, const int *__restrict__ cols,
                                       const int *__restrict__ dpos, V *a, unsigned *__restrict__ pivot)
{
    int e0 = 0, lo_end = 0;
    bool diag = false;
    if (have && off) {
        e0 = off[i];
        const int d = dpos[i];
        diag = d >= 0;
        lo_end = diag ? d : ~d;
    }
    const int nlow = lo_end - e0;
    const int own_end = lo_end + (diag ? 1 : 0);                     // the owned entries: the strict lower part and the diagonal
    for (int t = 0; __ballot(t < nlow) != 0ull; ++t) {               // (the same trip count in every lane of the wave)
        const bool on = t < nlow;
        const int e = e0 + t;
        V q = V(0);
        int j = 0;
        if (on) {
            j = cols[e];
            if ((t & (G - 1)) == gl) {                               // the owner of a[e]
                const int dj = dpos[j];
                const V piv = dj >= 0 ? a[dj] : V(0);
                q = a[e] / piv;
                a[e] = q;
            }
        }
        q = __shfl(q, t & (G - 1), G);
        if (on) {
            // this lane's entries behind e: e0 + r for r = gl (mod G), r > t
            for (int g = e + 1 + ((gl - t - 1) & (G - 1)); g < own_end; g += G) {
                const int k = cols[g];
                if (k == i) {
                    const V p = q * q;
                    a[g] = a[g] - p;
                } else {
                    const int dk = dpos[k];
                    const int l1 = dk >= 0 ? dk : ~dk;               // row k's strict lower part ends here
                    const int f = lv_lower_bound(cols, off[k], l1, j);
                    if (f < l1 && cols[f] == j) {
                        const V p = q * a[f];
                        a[g] = a[g] - p;
                    }
                }
            }
        }
    }
    if (diag && (nlow & (G - 1)) == gl) {                            // the owner of the diagonal
        const V v = a[lo_end];
        if (pivot && v <= V(0)) atomicMin(pivot, (unsigned) i);
        a[lo_end] = ic_root(v);
    }
}

template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void ic0_prologue_kernel(const V *vals, V *l, const int *__restrict__ off, const int *__restrict__ cols,
                                                                int rows, int nnz, int *__restrict__ dpos, unsigned *__restrict__ pivot)
{
    lv_prologue<V>(vals, l, off, cols, rows, nnz, dpos, pivot);
}

template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void ic0_level_kernel(const int *__restrict__ order, int n, int G, const int *__restrict__ off,
                                                             const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                             unsigned *__restrict__ pivot)
{
    lv_level_groups(order, n, G, [=](bool have, int i, int gl) { ic_row<V>(have, i, G, gl, off, cols, dpos, a, pivot); });
}

// levels [level_lo, level_hi), every one narrow: ONE workgroup, a barrier between two levels.  Every trip count that encloses a
// barrier or a shuffle is the same in every thread.  (The twin of ilu0_narrow_kernel of mspmv_csrilu0.hip:
// mspmv_levels.hpp says why the two are not one.)
template <typename V>
__global__ __launch_bounds__(LV_NARROW_BLOCK) void ic0_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
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
                ic_row<V>(have, have ? order[idx] : 0, G, gl, off, cols, dpos, a, pivot);
            }
            __syncthreads();                                        // level l's rows are finished before level l + 1 reads them
        }
        // (the barrier that ended the last level also ends the reads of s_lo)
    }
}

// rows [0, rows), LV_BLOCK / G of them per workgroup: entry (i, j) behind the diagonal receives entry (j, i), or +0.0
template <typename V>
__global__ __launch_bounds__(LV_BLOCK) void ic0_mirror_kernel(int rows, int G, const int *__restrict__ off, const int *__restrict__ cols,
                                                              const int *__restrict__ dpos, V *a)
{
    const int tid = (int) threadIdx.x;
    const long long idx = (long long) blockIdx.x * (LV_BLOCK / G) + tid / G;
    if (idx >= rows) return;                                         // (no shuffle and no barrier below)
    const int i = (int) idx;
    const int d = dpos[i];
    const int e1 = off[i + 1];
    for (int g = (d >= 0 ? d + 1 : ~d) + (tid & (G - 1)); g < e1; g += G) {
        const int j = cols[g];
        if (j <= i) continue;                                        // (unsorted input: only upper entries are written)
        const int dj = dpos[j];
        const int l1 = dj >= 0 ? dj : ~dj;
        const int f = lv_lower_bound(cols, off[j], l1, i);
        a[g] = (f < l1 && cols[f] == i) ? a[f] : V(0);
    }
}

// G for the mean length of a row's lower-plus-diagonal part under a symmetric pattern, ceil((nnz + rows) / (2 rows)).
// Measured (profiles/csric0_bench.txt, the sweep; DESIGN.md 4 "IC(0)"), fp64, G = 1 / 2 / 4 / 8 / 16 / 32 / 64: a 5-point grid of 2000 x 2000
// (the rule: 4) 33.9 / 26.2 / 25.6 / 26.1 / 27.5 / 31.1 / 39.1 ms, a 7-point grid of 128^3 (the rule: 4) 4.37 / 3.28 / 3.01 / 3.11 / 3.33 / 3.87 /
// 5.46 ms: the rule's choice is the fastest on both, so the starting rule stays.
static int ic_group(int32_t rows, int32_t nnz)
{
    return lv_group(rows > 0 ? ((long long) nnz + rows + 2ll * rows - 1) / (2ll * rows) : 1, "MSPMV_CSRIC0_GROUP");
}

template <typename V>
int ic_factor(const mspmv_csrsv_plan *p, void *d_temp, size_t *temp_bytes, const V *vals, V *l, const int32_t *off, const int32_t *cols,
              int32_t mirror, int32_t *d_pivot, hipStream_t stream, int debug_sync)
{
    if (mirror != 0 && mirror != 1) return hipErrorInvalidValue;
    return lv_factor<V>(
        p, d_temp, temp_bytes, vals, l, off, cols, d_pivot, stream, ic_group,
        [&](const LvFactor<V> &f, unsigned grid) {
            hipLaunchKernelGGL((ic0_prologue_kernel<V>), dim3(grid), dim3(LV_BLOCK), 0, stream, f.vals, f.out, f.off, f.cols, f.rows, f.nnz, f.dpos,
                               f.pivot);
            return lv_launched(stream, debug_sync, "ic0_prologue_kernel", grid, LV_BLOCK, f.G);
        },
        [&](const LvFactor<V> &f, const mspmv_csrsv_plan::Segment &s) {
            hipLaunchKernelGGL((ic0_narrow_kernel<V>), dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, s.level_lo,
                               s.level_hi, f.G, f.off, f.cols, f.dpos, f.out, f.pivot);
            return lv_launched(stream, debug_sync, "ic0_narrow_kernel", 1, LV_NARROW_BLOCK, f.G);
        },
        [&](const LvFactor<V> &f, const mspmv_csrsv_plan::Segment &s, unsigned grid) {
            hipLaunchKernelGGL((ic0_level_kernel<V>), dim3(grid), dim3(LV_BLOCK), 0, stream, p->d_order + s.row_lo, s.row_hi - s.row_lo, f.G, f.off,
                               f.cols, f.dpos, f.out, f.pivot);
            return lv_launched(stream, debug_sync, "ic0_level_kernel", grid, LV_BLOCK, f.G);
        },
        [&](const LvFactor<V> &f) {
            if (!mirror) return 0;
            // (no entries: the launch stays, over no rows -- the same launches whatever the matrix)
            const unsigned grid = f.nnz > 0 ? grid_for(f.rows, LV_BLOCK / f.G) : 1u;
            hipLaunchKernelGGL((ic0_mirror_kernel<V>), dim3(grid), dim3(LV_BLOCK), 0, stream, f.nnz > 0 ? f.rows : 0, f.G, f.off, f.cols, f.dpos, f.out);
            return lv_launched(stream, debug_sync, "ic0_mirror_kernel", grid, LV_BLOCK, f.G);
        });
}

}  // namespace

extern "C" {

int mspmv_csric0_group(int32_t rows, int32_t nnz, int32_t *lanes_per_row)
{
    if (rows < 0 || nnz < 0 || !lanes_per_row) return hipErrorInvalidValue;
    *lanes_per_row = ic_group(rows, nnz);
    return hipSuccess;
}

int mspmv_csric0_f32(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const float *d_values, float *d_values_l,
                     const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t mirror, int32_t *d_pivot, mspmv_stream_t stream,
                     int debug_sync)
{
    return ic_factor<float>(lower_plan, d_temp, temp_bytes, d_values, d_values_l, d_row_offsets, d_column_indices, mirror, d_pivot,
                            reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csric0_f64(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const double *d_values, double *d_values_l,
                     const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t mirror, int32_t *d_pivot, mspmv_stream_t stream,
                     int debug_sync)
{
    return ic_factor<double>(lower_plan, d_temp, temp_bytes, d_values, d_values_l, d_row_offsets, d_column_indices, mirror, d_pivot,
                             reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
