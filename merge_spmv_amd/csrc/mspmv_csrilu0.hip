// mspmv_csrilu0.hip -- the incomplete LU factorisation without fill-in on the device (mspmv_csrilu0_* of include/mspmv.h): A ~ L U on
// A's own pattern, L's unit diagonal implied, "nothing extracted": the layout the LOWER+UNIT and UPPER+NON_UNIT solves of
// mspmv_csrsv_* sweep.
//
// Scheme: the level schedule of the LOWER triangular solve.  Row i of the row-wise (IKJ) elimination needs the FINISHED rows k whose
// column is stored in its strict lower part -- the dependency graph of L x = b -- so a LOWER mspmv_csrsv_plan_t already holds the
// analysis: order[], level_offsets[] and the segments.  A maximal run of narrow levels is ONE workgroup of 1024 threads that walks its
// levels with __syncthreads() between them; every other level is one launch of many workgroups.  Nothing else orders two levels: no
// flags, no spinning, no cooperative launch.
//
// Prologue (one launch): a lane per row finds, by bisection, the first entry whose column is >= the row (the end of the strict lower
// part) and writes it to temp: the position p itself when that entry is the diagonal, ~p (negative) when the row stores none, which
// also goes to *d_pivot by atomicMin; a lane per entry copies d_values to d_values_lu when they differ.
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

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"
#include "mspmv_csrsv_plan.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

constexpr int ILU_BLOCK = 256;              // a wide level: ILU_BLOCK / G rows per workgroup
constexpr int ILU_NARROW_BLOCK = 1024;      // a run of narrow levels: one workgroup
constexpr int ILU_LEVEL_CHUNK = 1024;       // level offsets staged in LDS at a time

static unsigned ilu_grid(long long n, int per_block) { return (unsigned) std::max<long long>(1, (n + per_block - 1) / per_block); }

// first position in [lo, hi) whose column is >= c (hi when none)
__device__ __forceinline__ int ilu_lower_bound(const int *__restrict__ cols, int lo, int hi, int c)
{
    while (lo < hi) {
        const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// lane t < rows: the diagonal position of row t; lane t < nnz: one value copied (out of place only)
template <typename V>
__global__ __launch_bounds__(256) void ilu0_prologue_kernel(const V *vals, V *lu, const int *__restrict__ off, const int *__restrict__ cols,
                                                            int rows, int nnz, int *__restrict__ dpos, unsigned *__restrict__ pivot)
{
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t < nnz && lu != vals) lu[t] = vals[t];
    if (t < rows) {
        const int r = (int) t;
        int e0 = 0, e1 = 0;
        if (off) { e0 = off[r]; e1 = off[r + 1]; }                   // (off may be NULL only when the matrix has no entries)
        const int p = ilu_lower_bound(cols, e0, e1, r);
        const bool stored = p < e1 && cols[p] == r;
        dpos[r] = stored ? p : ~p;
        if (!stored && pivot) atomicMin(pivot, (unsigned) r);
    }
}

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
                const int f = ilu_lower_bound(cols, u0, u1, j);
                if (f < u1 && cols[f] == j) {
                    const V p = q * a[f];
                    a[g] = a[g] - p;
                }
            }
        }
    }
    if (pivot && diag && (nlow & (G - 1)) == gl && a[lo_end] == V(0)) atomicMin(pivot, (unsigned) i);
}

// one level (or a stretch of one): rows order[0 .. n), ILU_BLOCK / G of them per workgroup
template <typename V>
__global__ __launch_bounds__(ILU_BLOCK) void ilu0_level_kernel(const int *__restrict__ order, int n, int G, const int *__restrict__ off,
                                                               const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                               unsigned *__restrict__ pivot)
{
    const int tid = (int) threadIdx.x;
    const long long idx = (long long) blockIdx.x * (ILU_BLOCK / G) + tid / G;
    const bool have = idx < n;
    ilu_row<V>(have, have ? order[idx] : 0, G, tid & (G - 1), off, cols, dpos, a, pivot);
}

// levels [level_lo, level_hi), every one narrow: ONE workgroup, a barrier between two levels.  Every trip count that encloses a
// barrier or a shuffle is the same in every thread.
template <typename V>
__global__ __launch_bounds__(ILU_NARROW_BLOCK) void ilu0_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
                                                                       int level_lo, int level_hi, int G, const int *__restrict__ off,
                                                                       const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                                       unsigned *__restrict__ pivot)
{
    __shared__ int s_lo[ILU_LEVEL_CHUNK + 1];
    const int tid = (int) threadIdx.x, grp = tid / G, gl = tid & (G - 1), per_pass = ILU_NARROW_BLOCK / G;
    for (int base = level_lo; base < level_hi; base += ILU_LEVEL_CHUNK) {
        const int n = min(ILU_LEVEL_CHUNK, level_hi - base);
        for (int i = tid; i <= n; i += ILU_NARROW_BLOCK) s_lo[i] = level_offsets[base + i];
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

static int ilu_launched(hipStream_t stream, int debug_sync, const char *name, unsigned grid, int block, int G)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int) e;
    if (debug_sync) {
        printf("mspmv: %s<<<%u, %d>>> %d lanes per row\n", name, grid, block, G);
        fflush(stdout);
        e = hipStreamSynchronize(stream);
    }
    return (int) e;
}

// G: the smallest power of two that is at least the mean row length, within [1, 64].  Measured (profiles/csrilu0_bench.txt, the sweep;
// DESIGN.md 4 "ILU(0)"), fp64, G = 1 / 2 / 4 / 8 / 16 / 32 / 64: a 5-point grid of 2000 x 2000 (the rule: 8) 45.9 / 30.4 / 26.3 / 26.7 / 28.4 /
// 32.0 / 40.9 ms, a 7-point grid of 128^3 (the rule: 8) 6.53 / 4.13 / 3.33 / 3.12 / 3.35 / 3.88 / 5.49 ms.
static int ilu_group(int32_t rows, int32_t nnz)
{
#ifdef MSPMV_TUNING
    // development library only: the sweep of tools/csrilu0_bench.py
    if (const char *e = getenv("MSPMV_CSRILU0_GROUP")) {
        const int g = atoi(e);
        if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) return g;
    }
#endif
    if (rows <= 0) return 1;
    const long long mean = ((long long) nnz + rows - 1) / rows;
    int g = 1;
    while (g < 64 && g < mean) g <<= 1;
    return g;
}

static size_t ilu_temp_bytes(int32_t rows) { return std::max<size_t>(16, ((size_t) rows * 4 + 15) & ~size_t(15)); }

template <typename V>
int ilu_factor(const mspmv_csrsv_plan *p, void *d_temp, size_t *temp_bytes, const V *vals, V *lu, const int32_t *off, const int32_t *cols,
               int32_t *d_pivot, hipStream_t stream, int debug_sync)
{
    if (!p || p->info.uplo != MSPMV_CSRSV_LOWER || !temp_bytes) return hipErrorInvalidValue;
    const int rows = p->info.rows, nnz = p->info.nnz;
    const size_t need = ilu_temp_bytes(rows);
    if (!d_temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15) != 0) return hipErrorInvalidValue;
    if (nnz > 0 && (!vals || !lu || !off || !cols)) return hipErrorInvalidValue;
    unsigned *pivot = reinterpret_cast<unsigned *>(d_pivot);
    if (pivot && hipMemsetAsync(pivot, 0xff, 4, stream) != hipSuccess) return hipErrorInvalidValue;      // all ones: -1, no row yet
    if (rows == 0) return hipSuccess;
    if (nnz == 0) { vals = nullptr; lu = nullptr; off = nullptr; cols = nullptr; }
    const int G = ilu_group(rows, nnz);
    int *dpos = static_cast<int *>(d_temp);
    const unsigned pgrid = ilu_grid(std::max(rows, nnz), 256);
    hipLaunchKernelGGL((ilu0_prologue_kernel<V>), dim3(pgrid), dim3(256), 0, stream, vals, lu, off, cols, rows, nnz, dpos, pivot);
    if (int e = ilu_launched(stream, debug_sync, "ilu0_prologue_kernel", pgrid, 256, G)) return e;
    for (const mspmv_csrsv_plan::Segment &s : p->segments) {
        if (s.narrow) {
            hipLaunchKernelGGL((ilu0_narrow_kernel<V>), dim3(1), dim3(ILU_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, s.level_lo,
                               s.level_hi, G, off, cols, dpos, lu, pivot);
            if (int e = ilu_launched(stream, debug_sync, "ilu0_narrow_kernel", 1, ILU_NARROW_BLOCK, G)) return e;
        } else {
            const int n = s.row_hi - s.row_lo;
            const unsigned g = ilu_grid(n, ILU_BLOCK / G);
            hipLaunchKernelGGL((ilu0_level_kernel<V>), dim3(g), dim3(ILU_BLOCK), 0, stream, p->d_order + s.row_lo, n, G, off, cols, dpos, lu, pivot);
            if (int e = ilu_launched(stream, debug_sync, "ilu0_level_kernel", g, ILU_BLOCK, G)) return e;
        }
    }
    return hipSuccess;
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
