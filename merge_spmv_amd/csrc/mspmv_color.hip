// mspmv_color.hip -- a deterministic graph colouring on the device (mspmv_csr_color_* of include/mspmv.h): the colours, the vertices
// sorted stably by colour, that order's inverse and where each colour starts.  With row_perm = order and col_map = inverse,
// mspmv_csr_permute_* gives P A P^T, whose LOWER level schedule (mspmv_csrsv_plan_create) has at most as many levels as there are colours.
//
// Definition (the pattern and the priorities alone).  Vertices are the rows of a rows x rows pattern; u and v are neighbours when u != v
// and A[u,v] or A[v,u] is stored.  key(v) = (uint64) prio(v) << 32 | v, prio(v) = d_priority[v] or, without priorities, fmix32(v).
// color[v] = the smallest non-negative integer that no neighbour u with key(u) > key(v) holds: sequential greedy colouring in descending
// key order, a total function of its input.
//
// Scheme: Jones-Plassmann in rounds.  A vertex is coloured once every neighbour of larger key holds a colour >= 0; it then takes the
// smallest colour free among those neighbours.  color[v] goes from -1 to its final value in ONE 32-bit store and never changes again, so
// a reader in another workgroup of the same launch sees -1 (the vertex waits one more round) or the final value (what the next launch
// would show): the result is the definition whatever the timing.  A colour that reads as -1 anywhere in a vertex's scan, a rescan
// included, defers the vertex.  Nothing but the kernel boundary and, inside one workgroup, the barrier orders two rounds: no flags, no
// spinning, no workgroup that waits on another.  Every round colours at least the uncoloured vertex of the largest key.
//
// Analysis (mspmv_csr_color_create).
//   1. A^T's pattern by the structure-only device transpose (mspmv_csr_transpose_*): a vertex's neighbour slots are row v of A and row v
//      of A^T (a neighbour may sit in both, or twice in one; the diagonal is skipped).
//   2. Rounds over the compacted list of uncoloured vertices.  While more than COLOR_CAP remain, a round is one launch of many workgroups,
//      after which the host reads the remaining count back (32 bytes); at or below it ONE workgroup finishes all remaining rounds with a
//      barrier between them (a path of 4096 vertices in index order is one launch, not 4096).  A vertex of 64 or more neighbour slots is
//      scanned by its whole wave (lanes taking turns by ballot, the colour mask OR-reduced across the lanes), so that a hub costs no single
//      lane a long loop.  The free colour is the lowest clear bit of a 64-bit mask over the colours [base, base + 64); a full window
//      moves on by 64 and the vertex is scanned again.
//   3. order[] and offsets[] are the transpose of the rows x colours pattern that has the one entry (v, color[v]) in row v: the same
//      radix passes, so both are functions of the colours alone; inverse[order[i]] = i.
//   4. The host reads offsets once (for max_color_rows); the scratch is freed.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"     // lv_launched, LV_NARROW_BLOCK

struct mspmv_csr_color {
    mspmv_csr_color_info_t info{};
    int32_t *d_colors = nullptr, *d_order = nullptr, *d_inverse = nullptr, *d_offsets = nullptr;
};

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range

#include "mspmv_radix.hpp"     // tr_fill_kernel

// At most this many uncoloured vertices: one workgroup finishes (as SV_PEEL_CAP).  Measured (profiles/color_bench.txt, the sweep; DESIGN.md
// 4 "Multicolour ordering"), cap = 256 / 1024 / 4096 / 16384 / 65536: a 5-point grid of 2000 x 2000 6.17 / 6.07 / 6.10 / 6.13 / 6.41 ms, a
// 7-point grid of 128^3 5.05 / 5.01 / 5.02 / 5.20 / 6.53 ms, A + A^T + I of an R-MAT graph of scale 16 169 / 166 / 171 / 250 / 438 ms: flat up
// to 4096, then one workgroup is given more than it should have.
constexpr int COLOR_CAP = 4096;
constexpr int COLOR_CHUNK = 1024;           // entries per block of the edge count (one row-range search per block)

enum { CS_NEXT = 0, CS_MAXC = 1, CS_EDGES = 2 /* and 3 */, CS_WORDS = 8 };

__device__ __forceinline__ unsigned col_fmix32(unsigned h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ unsigned long long col_key(const unsigned *__restrict__ prio, int v)
{
    return (unsigned long long) (prio ? prio[v] : col_fmix32((unsigned) v)) << 32 | (unsigned) v;
}

__global__ __launch_bounds__(256) void color_iota_kernel(int *__restrict__ out, long long n)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int) i;
}

// the stored off-diagonal entries, duplicates counted: one 64-bit atomic per block of COLOR_CHUNK entries
__global__ __launch_bounds__(256) void color_edges_kernel(const int *__restrict__ off, const int *__restrict__ cols, int rows, int nnz,
                                                          int *__restrict__ state)
{
    __shared__ int s_range[2];
    __shared__ int s_count;
    if (threadIdx.x == 0) s_count = 0;
    const long long j0 = (long long) blockIdx.x * COLOR_CHUNK;
    const int j1 = (int) std::min<long long>(j0 + COLOR_CHUNK, nnz) - 1;
    block_row_range(off, rows, (int) j0, j1, s_range);              // (syncs)
    int n = 0;
    for (int j = (int) j0 + (int) threadIdx.x; j <= j1; j += 256) n += cols[j] != row_of(off, s_range[0], s_range[1], j) ? 1 : 0;
    if (n) atomicAdd(&s_count, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(reinterpret_cast<unsigned long long *>(state + CS_EDGES), (unsigned long long) s_count);
}

struct ColorGraph {                                                  // a vertex's neighbour slots: row v of A, then row v of A^T
    const int *off, *cols, *off_t, *cols_t;
    const unsigned *prio;
};

// The slots first, first + step, ... of vertex v (n of them, the first nA in A's row at e0, the others in A^T's at t0): ORs the colours
// of the neighbours of larger key that lie in [base, base + 64) into mask; false as soon as one of them is uncoloured.
__device__ __forceinline__ bool col_scan(const ColorGraph &g, const int *color, int v, unsigned long long kv, int e0, unsigned nA, int t0,
                                         unsigned n, unsigned first, unsigned step, int base, unsigned long long &mask)
{
    for (unsigned s = first; s < n; s += step) {
        const int u = s < nA ? g.cols[e0 + s] : g.cols_t[t0 + (s - nA)];
        if (u == v || col_key(g.prio, u) < kv) continue;
        const int c = color[u];
        if (c < 0) return false;
        const unsigned d = (unsigned) (c - base);
        if (d < 64u) mask |= 1ull << d;
    }
    return true;
}

__device__ __forceinline__ unsigned long long col_wave_or(unsigned long long m)
{
    unsigned lo = (unsigned) m, hi = (unsigned) (m >> 32);
    for (int d = 1; d < 64; d <<= 1) { lo |= __shfl_xor(lo, d, 64); hi |= __shfl_xor(hi, d, 64); }
    return (unsigned long long) hi << 32 | lo;
}

// All 64 lanes of a wave come here together, each with an uncoloured vertex v (or none): the vertex's colour, or -1 when a neighbour of
// larger key is still uncoloured.  A vertex of 64 slots or more is scanned by the whole wave; what decides a trip of its loop (ready,
// the mask) is made the same in every lane first.
__device__ __forceinline__ int col_pick(bool have, int v, const ColorGraph &g, const int *color)
{
    const unsigned lane = threadIdx.x & 63u;
    int e0 = 0, t0 = 0;
    unsigned nA = 0, n = 0;
    unsigned long long kv = 0;
    if (have) {
        e0 = g.off[v]; nA = (unsigned) (g.off[v + 1] - e0);
        t0 = g.off_t[v]; n = nA + (unsigned) (g.off_t[v + 1] - t0);
        kv = col_key(g.prio, v);
    }
    const bool longv = n >= 64u;
    int result = -1;
    if (have && !longv) {
        for (int base = 0;; base += 64) {
            unsigned long long mask = 0;
            if (!col_scan(g, color, v, kv, e0, nA, t0, n, 0u, 1u, base, mask)) break;
            if (~mask) { result = base + __builtin_ctzll(~mask); break; }
        }
    }
    unsigned long long todo = __ballot(longv);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int sv = __shfl(v, src, 64), se0 = __shfl(e0, src, 64), st0 = __shfl(t0, src, 64);
        const unsigned snA = __shfl(nA, src, 64), sn = __shfl(n, src, 64);
        const unsigned long long skv = (unsigned long long) __shfl((unsigned) (kv >> 32), src, 64) << 32 | __shfl((unsigned) kv, src, 64);
        int res = -1;
        for (int base = 0;; base += 64) {
            unsigned long long mask = 0;
            const bool ready = col_scan(g, color, sv, skv, se0, snA, st0, sn, lane, 64u, base, mask);
            if (__ballot(!ready)) break;
            mask = col_wave_or(mask);
            if (~mask) { res = base + __builtin_ctzll(~mask); break; }
        }
        if ((int) lane == src) result = res;
    }
    return result;
}

// All 64 lanes together: a coloured vertex stores its colour (the one transition of color[v]); the others join the next list, one
// atomic per wave.  The order in which vertices arrive in a list is discarded.
__device__ __forceinline__ void col_commit(bool have, int v, int c, int *color, int *next, int *next_count, int *max_color)
{
    const unsigned lane = threadIdx.x & 63u;
    if (have && c >= 0) color[v] = c;
    int m = have ? c : -1;
    for (int d = 1; d < 64; d <<= 1) m = max(m, __shfl_xor(m, d, 64));
    if (lane == 0 && m > 0) atomicMax(max_color, m);
    const unsigned long long waiting = __ballot(have && c < 0);
    if (!waiting) return;
    int at = 0;
    if (lane == 0) at = atomicAdd(next_count, __popcll(waiting));
    at = __shfl(at, 0, 64);
    if (have && c < 0) next[at + __popcll(waiting & ((1ull << lane) - 1))] = v;
}

// one round, many workgroups: the n uncoloured vertices `cur` (NULL: the vertices 0 .. n) -> those still uncoloured in `next`, counted in
// state[CS_NEXT] (zero on entry).  color is read and written by the same launch: not __restrict__.
__global__ __launch_bounds__(256) void color_wide_kernel(ColorGraph g, int *color, const int *__restrict__ cur, int *__restrict__ next, int n,
                                                         int *state)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    const int v = have ? (cur ? cur[i] : (int) i) : 0;
    const int c = col_pick(have, v, g, color);
    col_commit(have, v, c, color, next, state + CS_NEXT, state + CS_MAXC);
}

// ONE workgroup: round after round until no vertex is left, a barrier between two rounds.  The list arrays are not __restrict__: what
// one round writes the next one reads.  (n is the same in every thread.)
__global__ __launch_bounds__(LV_NARROW_BLOCK) void color_narrow_kernel(ColorGraph g, int *color, int *f0, int *f1, int n, int *state)
{
    __shared__ int s_next;
    const int tid = (int) threadIdx.x;
    int *cur = f0, *next = f1;
    while (n > 0) {
        if (tid == 0) s_next = 0;
        __syncthreads();
        for (int base = 0; base < n; base += LV_NARROW_BLOCK) {
            const bool have = base + tid < n;
            const int v = have ? cur[base + tid] : 0;
            const int c = col_pick(have, v, g, color);
            col_commit(have, v, c, color, next, &s_next, state + CS_MAXC);
        }
        __threadfence_block();
        __syncthreads();
        n = s_next;
        int *t = cur; cur = next; next = t;
        __syncthreads();                                            // (everyone has read s_next before it is cleared)
    }
}

__global__ __launch_bounds__(256) void color_inverse_kernel(const int *__restrict__ order, int rows, int *__restrict__ inverse)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < rows) inverse[order[i]] = (int) i;
}

static int color_read(void *h, const void *d, size_t bytes, hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return (int) e;
}

static int color_cap()
{
#ifdef MSPMV_TUNING
    // development library only: the sweep of tools/color_bench.py
    if (const char *e = getenv("MSPMV_COLOR_CAP")) { const int c = atoi(e); if (c > 0) return c; }
#endif
    return COLOR_CAP;
}

struct ColorScratch {
    char *base = nullptr;
    ~ColorScratch() { if (base) (void) hipFree(base); }
};

static int color_analyse(mspmv_csr_color &p, const int32_t *d_off, const int32_t *d_cols, const uint32_t *d_prio, hipStream_t stream,
                         int debug_sync)
{
    const int rows = p.info.rows, nnz = p.info.nnz;
    mspmv_stream_t cstream = reinterpret_cast<mspmv_stream_t>(stream);
    const unsigned rgrid = grid_for(rows, 256);
    for (int32_t **a : {&p.d_colors, &p.d_order, &p.d_inverse})
        if (hipMalloc(reinterpret_cast<void **>(a), (size_t) rows * 4) != hipSuccess) return hipErrorOutOfMemory;
    p.info.device_bytes = 3 * (uint64_t) rows * 4;
    std::vector<int32_t> h_co;
    if (nnz == 0) {
        // no edges: colour 0 everywhere, the identity order
        hipLaunchKernelGGL(tr_fill_kernel, dim3(rgrid), dim3(256), 0, stream, p.d_colors, (long long) rows, 0);
        if (int e = lv_launched(stream, debug_sync, "tr_fill_kernel", rgrid, 256)) return e;
        for (int32_t *a : {p.d_order, p.d_inverse}) {
            hipLaunchKernelGGL(color_iota_kernel, dim3(rgrid), dim3(256), 0, stream, a, (long long) rows);
            if (int e = lv_launched(stream, debug_sync, "color_iota_kernel", rgrid, 256)) return e;
        }
        p.info.colors = 1;
        h_co = {0, rows};
        if (hipMalloc(reinterpret_cast<void **>(&p.d_offsets), 8) != hipSuccess) return hipErrorOutOfMemory;
        if (hipMemcpyAsync(p.d_offsets, h_co.data(), 8, hipMemcpyHostToDevice, stream) != hipSuccess) return hipErrorInvalidValue;
    } else {
        size_t tb1 = 0, tb2 = 0;
        if (int e = mspmv_csr_transpose_f32(nullptr, &tb1, nullptr, nullptr, nullptr, rows, rows, nnz, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) return e;
        if (int e = mspmv_csr_transpose_f32(nullptr, &tb2, nullptr, nullptr, nullptr, rows, rows, rows, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) return e;
        const uint64_t n4 = align256((uint64_t) rows * 4 + 4);
        uint64_t o = 0;
        const uint64_t state_off = o; o += 256;
        const uint64_t offt_off = o; o += n4;
        const uint64_t colst_off = o; o += align256((uint64_t) nnz * 4);
        const uint64_t f0_off = o; o += n4;
        const uint64_t f1_off = o; o += n4;
        const uint64_t iota_off = o; o += n4;
        const uint64_t temp_off = o; o += align256(std::max(tb1, tb2));
        ColorScratch S;
        if (hipMalloc(reinterpret_cast<void **>(&S.base), o) != hipSuccess) return hipErrorOutOfMemory;
        int *state = reinterpret_cast<int *>(S.base + state_off), *off_t = reinterpret_cast<int *>(S.base + offt_off);
        int *cols_t = reinterpret_cast<int *>(S.base + colst_off), *iota = reinterpret_cast<int *>(S.base + iota_off);
        int *f[2] = {reinterpret_cast<int *>(S.base + f0_off), reinterpret_cast<int *>(S.base + f1_off)};
        void *temp = S.base + temp_off;
        // 1. the pattern of A^T
        size_t tb = tb1;
        if (int e = mspmv_csr_transpose_f32(temp, &tb, nullptr, d_off, d_cols, rows, rows, nnz, nullptr, off_t, cols_t, nullptr, cstream, debug_sync)) return e;
        // 2. every vertex uncoloured; the edge count; the rounds
        if (hipMemsetAsync(state, 0, CS_WORDS * 4, stream) != hipSuccess) return hipErrorInvalidValue;
        hipLaunchKernelGGL(tr_fill_kernel, dim3(rgrid), dim3(256), 0, stream, p.d_colors, (long long) rows, -1);
        if (int e = lv_launched(stream, debug_sync, "tr_fill_kernel", rgrid, 256)) return e;
        const unsigned egrid = grid_for(nnz, COLOR_CHUNK);
        hipLaunchKernelGGL(color_edges_kernel, dim3(egrid), dim3(256), 0, stream, d_off, d_cols, rows, nnz, state);
        if (int e = lv_launched(stream, debug_sync, "color_edges_kernel", egrid, 256)) return e;
        const ColorGraph g{d_off, d_cols, off_t, cols_t, d_prio};
        const int cap = color_cap();
        int h[CS_WORDS];
        int n = rows, which = 0;
        const int *cur = nullptr;                                   // (the first list is every vertex)
        while (n > cap) {
            const unsigned wgrid = grid_for(n, 256);
            if (hipMemsetAsync(state + CS_NEXT, 0, 4, stream) != hipSuccess) return hipErrorInvalidValue;
            hipLaunchKernelGGL(color_wide_kernel, dim3(wgrid), dim3(256), 0, stream, g, p.d_colors, cur, f[which], n, state);
            if (int e = lv_launched(stream, debug_sync, "color_wide_kernel", wgrid, 256)) return e;
            if (int e = color_read(h, state, sizeof(h), stream)) return e;
            n = h[CS_NEXT]; cur = f[which]; which ^= 1;
            ++p.info.rounds;
        }
        if (n > 0) {
            if (!cur) {
                hipLaunchKernelGGL(color_iota_kernel, dim3(rgrid), dim3(256), 0, stream, f[which ^ 1], (long long) rows);
                if (int e = lv_launched(stream, debug_sync, "color_iota_kernel", rgrid, 256)) return e;
            }
            hipLaunchKernelGGL(color_narrow_kernel, dim3(1), dim3(LV_NARROW_BLOCK), 0, stream, g, p.d_colors, f[which ^ 1], f[which], n, state);
            if (int e = lv_launched(stream, debug_sync, "color_narrow_kernel", 1, LV_NARROW_BLOCK)) return e;
            ++p.info.rounds;
        }
        if (int e = color_read(h, state, sizeof(h), stream)) return e;
        const int colors = h[CS_MAXC] + 1;
        p.info.colors = colors;
        p.info.edges = (int64_t) ((uint64_t) (unsigned) h[CS_EDGES] | (uint64_t) (unsigned) h[CS_EDGES + 1] << 32);
        // 3. the vertices sorted stably by colour, and where each colour starts: the transpose of the pattern {(v, color[v])}
        if (hipMalloc(reinterpret_cast<void **>(&p.d_offsets), ((size_t) colors + 1) * 4) != hipSuccess) return hipErrorOutOfMemory;
        const unsigned igrid = grid_for((long long) rows + 1, 256);
        hipLaunchKernelGGL(color_iota_kernel, dim3(igrid), dim3(256), 0, stream, iota, (long long) rows + 1);
        if (int e = lv_launched(stream, debug_sync, "color_iota_kernel", igrid, 256)) return e;
        tb = tb2;
        if (int e = mspmv_csr_transpose_f32(temp, &tb, nullptr, iota, p.d_colors, rows, colors, rows, nullptr, p.d_offsets, p.d_order, nullptr, cstream,
                                            debug_sync))
            return e;
        hipLaunchKernelGGL(color_inverse_kernel, dim3(rgrid), dim3(256), 0, stream, p.d_order, rows, p.d_inverse);
        if (int e = lv_launched(stream, debug_sync, "color_inverse_kernel", rgrid, 256)) return e;
        h_co.resize((size_t) colors + 1);
        if (int e = color_read(h_co.data(), p.d_offsets, h_co.size() * 4, stream)) return e;
    }
    p.info.device_bytes += h_co.size() * 4;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorInvalidValue;
    for (int c = 0; c < p.info.colors; ++c) p.info.max_color_rows = std::max(p.info.max_color_rows, h_co[c + 1] - h_co[c]);
    return hipSuccess;
}

}  // namespace

extern "C" {

int mspmv_csr_color_create(mspmv_csr_color_t **coloring, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows,
                           int32_t nnz, const uint32_t *d_priority, mspmv_stream_t stream, int debug_sync)
{
    if (!coloring) return hipErrorInvalidValue;
    *coloring = nullptr;
    if (rows < 0 || nnz < 0 || (long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || !d_row_offsets || !d_column_indices)) return hipErrorInvalidValue;
    mspmv_csr_color *p = new (std::nothrow) mspmv_csr_color;
    if (!p) return hipErrorOutOfMemory;
    p->info.rows = rows; p->info.nnz = nnz;
    if (rows > 0) {
        if (int e = color_analyse(*p, d_row_offsets, d_column_indices, d_priority, reinterpret_cast<hipStream_t>(stream), debug_sync)) {
            (void) hipGetLastError();
            (void) mspmv_csr_color_destroy(p);
            return e;
        }
    }
    *coloring = p;
    return hipSuccess;
}

int mspmv_csr_color_info(const mspmv_csr_color_t *coloring, mspmv_csr_color_info_t *info)
{
    if (!coloring || !info) return hipErrorInvalidValue;
    *info = coloring->info;
    return hipSuccess;
}

const int32_t *mspmv_csr_color_colors(const mspmv_csr_color_t *coloring) { return coloring ? coloring->d_colors : nullptr; }
const int32_t *mspmv_csr_color_order(const mspmv_csr_color_t *coloring) { return coloring ? coloring->d_order : nullptr; }
const int32_t *mspmv_csr_color_inverse(const mspmv_csr_color_t *coloring) { return coloring ? coloring->d_inverse : nullptr; }
const int32_t *mspmv_csr_color_offsets(const mspmv_csr_color_t *coloring) { return coloring ? coloring->d_offsets : nullptr; }

int mspmv_csr_color_destroy(mspmv_csr_color_t *coloring)
{
    if (!coloring) return hipErrorInvalidValue;
    for (int32_t *a : {coloring->d_colors, coloring->d_order, coloring->d_inverse, coloring->d_offsets})
        if (a) (void) hipFree(a);
    delete coloring;
    return hipSuccess;
}

}  // extern "C"
