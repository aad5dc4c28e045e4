// mspmv_levels.hpp -- what the kernel families that run along a level schedule (mspmv_csrsv_plan.hpp) share: mspmv_csrsv.hip and
// mspmv_csrsm.hip (the solves), mspmv_csrilu0.hip and mspmv_csric0.hip (the factorisations).  Each of them keeps its own __global__
// kernels and its own row body; here are the bodies those kernels call with the row body as a callable, the small device pieces, and
// the host code of a launch and of a factorisation.  Plain function templates, nothing with state.
// (ilu0_narrow_kernel and ic0_narrow_kernel hold their walk themselves: behind a shared one the compiler swapped two instructions
// of theirs, and this layer was made under the rule that the factorisation kernels stay instruction for instruction what they were.)
//
// The schedule: the rows of one level depend only on rows of earlier levels.  A maximal run of narrow levels is ONE workgroup of
// LV_NARROW_BLOCK threads that walks its levels with __syncthreads() between them; every other level is one launch of many workgroups
// of LV_BLOCK threads.  Nothing else orders two levels: no flags, no spinning, no cooperative launch.
//
// The rule of every loop here: a trip count that encloses a barrier or a shuffle is the same in every thread of the workgroup (of the
// wave, for a shuffle), and no thread leaves such a loop early; a thread without a row goes round with `have` false.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"
#include "mspmv_csrsv_plan.hpp"

namespace mspmv {

constexpr int LV_BLOCK = 256;               // a wide level (and the prologue): many workgroups
constexpr int LV_NARROW_BLOCK = 1024;       // a run of narrow levels: one workgroup
constexpr int LV_LEVEL_CHUNK = 1024;        // level offsets staged in LDS at a time

// ---- device: small pieces ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lv_strict(int upper, int r, int c) { return upper ? c > r : c < r; }

__device__ __forceinline__ void lv_bounds(const int *__restrict__ off, int r, int &e0, int &e1)
{
    e0 = 0; e1 = 0;
    if (off) { e0 = off[r]; e1 = off[r + 1]; }                      // (off may be NULL only when the matrix has no entries)
}

// first position in [lo, hi) whose column is >= c (hi when none)
__device__ __forceinline__ int lv_lower_bound(const int *__restrict__ cols, int lo, int hi, int c)
{
    while (lo < hi) {
        const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The prologue of a factorisation, LV_BLOCK threads per workgroup.  Lane t < rows finds, by bisection, the first entry of row t whose
// column is >= t (the end of the strict lower part) and writes it to dpos: the position p itself when that entry is the diagonal, ~p
// (negative) when the row stores none, which also goes to *pivot by atomicMin; lane t < nnz copies one value (out of place only).
template <typename V>
__device__ __forceinline__ void lv_prologue(const V *vals, V *out, const int *__restrict__ off, const int *__restrict__ cols, int rows, int nnz,
                                            int *__restrict__ dpos, unsigned *__restrict__ pivot)
{
    const long long t = (long long) blockIdx.x * LV_BLOCK + threadIdx.x;
    if (t < nnz && out != vals) out[t] = vals[t];
    if (t < rows) {
        const int r = (int) t;
        int e0, e1;
        lv_bounds(off, r, e0, e1);
        const int p = lv_lower_bound(cols, e0, e1, r);
        const bool stored = p < e1 && cols[p] == r;
        dpos[r] = stored ? p : ~p;
        if (!stored && pivot) atomicMin(pivot, (unsigned) r);
    }
}

// ---- device: a row per lane (or per P lanes), the solves ------------------------------------------------------------------------------
// Levels [level_lo, level_hi), every one narrow: ONE workgroup, a barrier between two levels.  Of the rows order[lo .. hi) of a level a
// thread takes lo + sub, lo + sub + step, ...: (tid, LV_NARROW_BLOCK) for a lane per row, (tid >> logp, LV_NARROW_BLOCK >> logp) for
// 1 << logp lanes per row.  row(r, e0, e1) solves row r, whose entries are [e0, e1).
template <typename Row>
__device__ __forceinline__ void lv_walk_ahead(const int *order, const int *level_offsets, int level_lo, int level_hi, const int *off, int sub,
                                              int step, Row row)
{
    __shared__ int s_lo[LV_LEVEL_CHUNK + 1];
    const int tid = (int) threadIdx.x;
    for (int base = level_lo; base < level_hi; base += LV_LEVEL_CHUNK) {
        const int n = min(LV_LEVEL_CHUNK, level_hi - base);
        for (int i = tid; i <= n; i += LV_NARROW_BLOCK) s_lo[i] = level_offsets[base + i];
        __syncthreads();
        // this thread's first row of the level and its bounds: loaded one level ahead (they do not depend on the solution)
        int i = s_lo[0] + sub, r = 0, e0 = 0, e1 = 0;
        bool have = i < s_lo[1];
        if (have) { r = order[i]; lv_bounds(off, r, e0, e1); }
        for (int l = 0; l < n; ++l) {
            const int hi = s_lo[l + 1];
            if (have) {
                row(r, e0, e1);
                for (i += step; i < hi; i += step) {
                    r = order[i];
                    lv_bounds(off, r, e0, e1);
                    row(r, e0, e1);
                }
            }
            have = false;
            if (l + 1 < n) {
                i = hi + sub;
                have = i < s_lo[l + 2];
                if (have) { r = order[i]; lv_bounds(off, r, e0, e1); }
            }
            __syncthreads();                                        // level l's solution is written before level l + 1 reads it
        }
        // (the barrier that ended the last level also ends the reads of s_lo)
    }
}

// ---- device: a row per group of G lanes, the factorisations ---------------------------------------------------------------------------
// A row is worked by G consecutive lanes of one wave (G a power of two).  All 64 lanes of a wave reach row(have, i, gl) together; the
// lanes of a group share `have` and the row i, gl is the lane's place in its group.
// One level (or a stretch of one): rows order[0 .. n), LV_BLOCK / G of them per workgroup
template <typename Row>
__device__ __forceinline__ void lv_level_groups(const int *order, int n, int G, Row row)
{
    const int tid = (int) threadIdx.x;
    const long long idx = (long long) blockIdx.x * (LV_BLOCK / G) + tid / G;
    const bool have = idx < n;
    row(have, have ? order[idx] : 0, tid & (G - 1));
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// after every launch: its error; with debug_sync the line "mspmv: NAME<<<grid, block>>>[ G lanes per row]" and a synchronisation
static int lv_launched(hipStream_t stream, int debug_sync, const char *name, unsigned grid, int block, int G = 0)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int) e;
    if (debug_sync) {
        if (G) printf("mspmv: %s<<<%u, %d>>> %d lanes per row\n", name, grid, block, G);
        else printf("mspmv: %s<<<%u, %d>>>\n", name, grid, block);
        fflush(stdout);
        e = hipStreamSynchronize(stream);
    }
    return (int) e;
}

// G, the lanes of a row of a factorisation: the smallest power of two that is at least `mean`, within [1, 64]
static int lv_group(long long mean, const char *tuning_env)
{
#ifdef MSPMV_TUNING
    // development library only: the sweeps of tools/csrilu0_bench.py and tools/csric0_bench.py
    if (const char *e = getenv(tuning_env)) {
        const int g = atoi(e);
        if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) return g;
    }
#endif
    (void) tuning_env;
    int g = 1;
    while (g < 64 && g < mean) g <<= 1;
    return g;
}

// what the launches of one factorisation work on (the matrix arrays are NULL when it has no entries)
template <typename V>
struct LvFactor {
    const V *vals;
    V *out;
    const int32_t *off, *cols;
    int *dpos;
    unsigned *pivot;
    int rows, nnz, G;
};

// A factorisation along a LOWER plan: the checks, the size query (temp: rows * 4 bytes, 16-byte aligned, at least 16), *d_pivot = -1,
// the prologue, then the plan's segments in order, then the epilogue.  group(rows, nnz) gives G.  Each callable launches its kernel and
// returns lv_launched(...): prologue(f, grid), narrow(f, segment), level(f, segment, grid), epilogue(f).
template <typename V, typename Prologue, typename Narrow, typename Level, typename Epilogue>
int lv_factor(const mspmv_csrsv_plan *p, void *d_temp, size_t *temp_bytes, const V *vals, V *out, const int32_t *off, const int32_t *cols,
              int32_t *d_pivot, hipStream_t stream, int (*group)(int32_t, int32_t), Prologue prologue, Narrow narrow, Level level, Epilogue epilogue)
{
    if (!p || p->info.uplo != MSPMV_CSRSV_LOWER || !temp_bytes) return hipErrorInvalidValue;
    const int rows = p->info.rows, nnz = p->info.nnz;
    const size_t need = std::max<size_t>(16, ((size_t) rows * 4 + 15) & ~size_t(15));
    if (!d_temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15) != 0) return hipErrorInvalidValue;
    if (nnz > 0 && (!vals || !out || !off || !cols)) return hipErrorInvalidValue;
    unsigned *pivot = reinterpret_cast<unsigned *>(d_pivot);
    if (pivot && hipMemsetAsync(pivot, 0xff, 4, stream) != hipSuccess) return hipErrorInvalidValue;      // all ones: -1, no row yet
    if (rows == 0) return hipSuccess;
    if (nnz == 0) { vals = nullptr; out = nullptr; off = nullptr; cols = nullptr; }
    const LvFactor<V> f{vals, out, off, cols, static_cast<int *>(d_temp), pivot, rows, nnz, group(rows, nnz)};
    if (int e = prologue(f, grid_for(std::max(rows, nnz), LV_BLOCK))) return e;
    for (const mspmv_csrsv_plan::Segment &s : p->segments)
        if (int e = s.narrow ? narrow(f, s) : level(f, s, grid_for(s.row_hi - s.row_lo, LV_BLOCK / f.G))) return e;
    return epilogue(f);
}

}  // namespace mspmv
