// mspmv_csric0.hip -- the incomplete Cholesky factorisation without fill-in on the device (mspmv_csric0_* of include/mspmv.h): A ~ L L^T
// on the pattern of A's lower triangle, L in the lower triangle and on the diagonal of A's own layout; with mirror == 1 one more launch
// writes L^T into the upper triangle, so that the array is L\L^T and the LOWER + NON_UNIT and UPPER + NON_UNIT solves of mspmv_csrsv_*
// sweep it with nothing extracted and nothing transposed.
//
// Scheme: the level schedule of the LOWER triangular solve, exactly as in mspmv_csrilu0.hip.  Row i of the row-wise Cholesky needs the
// FINISHED rows whose column is stored in its strict lower part -- the dependency graph of L x = b -- so a LOWER mspmv_csrsv_plan_t
// already holds the analysis.  A maximal run of narrow levels is ONE workgroup of 1024 threads that walks its levels with
// __syncthreads() between them; every other level is one launch of many workgroups.  Nothing else orders two levels: no flags, no
// spinning, no cooperative launch.
//
// Prologue (one launch; the same work as ILU(0)'s, duplicated here so that that file's launches and lines stay as they are): a lane per
// row finds, by bisection, the first entry whose column is >= the row and writes it to temp: the position p itself when that entry is
// the diagonal, ~p (negative) when the row stores none, which also goes to *d_pivot by atomicMin; a lane per entry copies d_values to
// d_values_l when they differ.
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

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"
#include "mspmv_csrsv_plan.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

constexpr int IC_BLOCK = 256;               // a wide level and the mirror: IC_BLOCK / G rows per workgroup
constexpr int IC_NARROW_BLOCK = 1024;       // a run of narrow levels: one workgroup
constexpr int IC_LEVEL_CHUNK = 1024;        // level offsets staged in LDS at a time

static unsigned ic_grid(long long n, int per_block) { return (unsigned) std::max<long long>(1, (n + per_block - 1) / per_block); }

// first position in [lo, hi) whose column is >= c (hi when none)
__device__ __forceinline__ int ic_lower_bound(const int *__restrict__ cols, int lo, int hi, int c)
{
    while (lo < hi) {
        const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the compiler's correctly rounded roots (no fast-math in this file)
__device__ __forceinline__ float ic_root(float v) { return sqrtf(v); }
__device__ __forceinline__ double ic_root(double v) { return sqrt(v); }

// lane t < rows: the diagonal position of row t; lane t < nnz: one value copied (out of place only)
template <typename V>
__global__ __launch_bounds__(256) void ic0_prologue_kernel(const V *vals, V *l, const int *__restrict__ off, const int *__restrict__ cols,
                                                           int rows, int nnz, int *__restrict__ dpos, unsigned *__restrict__ pivot)
{
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t < nnz && l != vals) l[t] = vals[t];
    if (t < rows) {
        const int r = (int) t;
        int e0 = 0, e1 = 0;
        if (off) { e0 = off[r]; e1 = off[r + 1]; }                   // (off may be NULL only when the matrix has no entries)
        const int p = ic_lower_bound(cols, e0, e1, r);
        const bool stored = p < e1 && cols[p] == r;
        dpos[r] = stored ? p : ~p;
        if (!stored && pivot) atomicMin(pivot, (unsigned) r);
    }
}

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
                    const int f = ic_lower_bound(cols, off[k], l1, j);
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

// one level (or a stretch of one): rows order[0 .. n), IC_BLOCK / G of them per workgroup
template <typename V>
__global__ __launch_bounds__(IC_BLOCK) void ic0_level_kernel(const int *__restrict__ order, int n, int G, const int *__restrict__ off,
                                                             const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                             unsigned *__restrict__ pivot)
{
    const int tid = (int) threadIdx.x;
    const long long idx = (long long) blockIdx.x * (IC_BLOCK / G) + tid / G;
    const bool have = idx < n;
    ic_row<V>(have, have ? order[idx] : 0, G, tid & (G - 1), off, cols, dpos, a, pivot);
}

// levels [level_lo, level_hi), every one narrow: ONE workgroup, a barrier between two levels.  Every trip count that encloses a
// barrier or a shuffle is the same in every thread.
template <typename V>
__global__ __launch_bounds__(IC_NARROW_BLOCK) void ic0_narrow_kernel(const int *__restrict__ order, const int *__restrict__ level_offsets,
                                                                     int level_lo, int level_hi, int G, const int *__restrict__ off,
                                                                     const int *__restrict__ cols, const int *__restrict__ dpos, V *a,
                                                                     unsigned *__restrict__ pivot)
{
    __shared__ int s_lo[IC_LEVEL_CHUNK + 1];
    const int tid = (int) threadIdx.x, grp = tid / G, gl = tid & (G - 1), per_pass = IC_NARROW_BLOCK / G;
    for (int base = level_lo; base < level_hi; base += IC_LEVEL_CHUNK) {
        const int n = min(IC_LEVEL_CHUNK, level_hi - base);
        for (int i = tid; i <= n; i += IC_NARROW_BLOCK) s_lo[i] = level_offsets[base + i];
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

// rows [0, rows), IC_BLOCK / G of them per workgroup: entry (i, j) behind the diagonal receives entry (j, i), or +0.0
template <typename V>
__global__ __launch_bounds__(IC_BLOCK) void ic0_mirror_kernel(int rows, int G, const int *__restrict__ off, const int *__restrict__ cols,
                                                              const int *__restrict__ dpos, V *a)
{
    const int tid = (int) threadIdx.x;
    const long long idx = (long long) blockIdx.x * (IC_BLOCK / G) + tid / G;
    if (idx >= rows) return;                                         // (no shuffle and no barrier below)
    const int i = (int) idx;
    const int d = dpos[i];
    const int e1 = off[i + 1];
    for (int g = (d >= 0 ? d + 1 : ~d) + (tid & (G - 1)); g < e1; g += G) {
        const int j = cols[g];
        if (j <= i) continue;                                        // (unsorted input: only upper entries are written)
        const int dj = dpos[j];
        const int l1 = dj >= 0 ? dj : ~dj;
        const int f = ic_lower_bound(cols, off[j], l1, i);
        a[g] = (f < l1 && cols[f] == i) ? a[f] : V(0);
    }
}

static int ic_launched(hipStream_t stream, int debug_sync, const char *name, unsigned grid, int block, int G)
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

// G: the smallest power of two that is at least the mean length of a row's lower-plus-diagonal part under a symmetric pattern,
// ceil((nnz + rows) / (2 rows)), within [1, 64].
// Measured (profiles/csric0_bench.txt, the sweep; DESIGN.md 4 "IC(0)"), fp64, G = 1 / 2 / 4 / 8 / 16 / 32 / 64: a 5-point grid of 2000 x 2000
// (the rule: 4) 33.9 / 26.2 / 25.6 / 26.1 / 27.5 / 31.1 / 39.1 ms, a 7-point grid of 128^3 (the rule: 4) 4.37 / 3.28 / 3.01 / 3.11 / 3.33 / 3.87 /
// 5.46 ms: the rule's choice is the fastest on both, so the starting rule stays.
static int ic_group(int32_t rows, int32_t nnz)
{
#ifdef MSPMV_TUNING
    // development library only: the sweep of tools/csric0_bench.py
    if (const char *e = getenv("MSPMV_CSRIC0_GROUP")) {
        const int g = atoi(e);
        if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) return g;
    }
#endif
    if (rows <= 0) return 1;
    const long long mean = ((long long) nnz + rows + 2ll * rows - 1) / (2ll * rows);
    int g = 1;
    while (g < 64 && g < mean) g <<= 1;
    return g;
}

static size_t ic_temp_bytes(int32_t rows) { return std::max<size_t>(16, ((size_t) rows * 4 + 15) & ~size_t(15)); }

template <typename V>
int ic_factor(const mspmv_csrsv_plan *p, void *d_temp, size_t *temp_bytes, const V *vals, V *l, const int32_t *off, const int32_t *cols,
              int32_t mirror, int32_t *d_pivot, hipStream_t stream, int debug_sync)
{
    if (!p || p->info.uplo != MSPMV_CSRSV_LOWER || !temp_bytes || (mirror != 0 && mirror != 1)) return hipErrorInvalidValue;
    const int rows = p->info.rows, nnz = p->info.nnz;
    const size_t need = ic_temp_bytes(rows);
    if (!d_temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15) != 0) return hipErrorInvalidValue;
    if (nnz > 0 && (!vals || !l || !off || !cols)) return hipErrorInvalidValue;
    unsigned *pivot = reinterpret_cast<unsigned *>(d_pivot);
    if (pivot && hipMemsetAsync(pivot, 0xff, 4, stream) != hipSuccess) return hipErrorInvalidValue;      // all ones: -1, no row yet
    if (rows == 0) return hipSuccess;
    if (nnz == 0) { vals = nullptr; l = nullptr; off = nullptr; cols = nullptr; }
    const int G = ic_group(rows, nnz);
    int *dpos = static_cast<int *>(d_temp);
    const unsigned pgrid = ic_grid(std::max(rows, nnz), 256);
    hipLaunchKernelGGL((ic0_prologue_kernel<V>), dim3(pgrid), dim3(256), 0, stream, vals, l, off, cols, rows, nnz, dpos, pivot);
    if (int e = ic_launched(stream, debug_sync, "ic0_prologue_kernel", pgrid, 256, G)) return e;
    for (const mspmv_csrsv_plan::Segment &s : p->segments) {
        if (s.narrow) {
            hipLaunchKernelGGL((ic0_narrow_kernel<V>), dim3(1), dim3(IC_NARROW_BLOCK), 0, stream, p->d_order, p->d_level_offsets, s.level_lo,
                               s.level_hi, G, off, cols, dpos, l, pivot);
            if (int e = ic_launched(stream, debug_sync, "ic0_narrow_kernel", 1, IC_NARROW_BLOCK, G)) return e;
        } else {
            const int n = s.row_hi - s.row_lo;
            const unsigned g = ic_grid(n, IC_BLOCK / G);
            hipLaunchKernelGGL((ic0_level_kernel<V>), dim3(g), dim3(IC_BLOCK), 0, stream, p->d_order + s.row_lo, n, G, off, cols, dpos, l, pivot);
            if (int e = ic_launched(stream, debug_sync, "ic0_level_kernel", g, IC_BLOCK, G)) return e;
        }
    }
    if (mirror) {                                                    // (no entries: the launch stays, over no rows -- the same launches whatever the matrix)
        const unsigned g = nnz > 0 ? ic_grid(rows, IC_BLOCK / G) : 1u;
        hipLaunchKernelGGL((ic0_mirror_kernel<V>), dim3(g), dim3(IC_BLOCK), 0, stream, nnz > 0 ? rows : 0, G, off, cols, dpos, l);
        if (int e = ic_launched(stream, debug_sync, "ic0_mirror_kernel", g, IC_BLOCK, G)) return e;
    }
    return hipSuccess;
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
