// mspmv_coords.hpp -- the merge-path search, the detection of column-band candidates and the three coordinate kernels.
#pragma once
#include "mspmv_types.hpp"

namespace mspmv {

// ---------------------------------------------------------------------------
// Merge-path diagonal search (reference
// cub/thread/thread_search.cuh:53-84), wave-cooperative.
//   smallest p in [lo, hi] with p == hi or row_end[p] + p + 1 > diagonal.
// row_end[p] + p is strictly increasing, so the predicate is monotone; each
// round the wave's 64 lanes probe the last element of 64 equal chunks of the
// candidate range and a ballot picks the chunk: range / 64 per dependent load.
// All lanes return the same coordinate.
// ---------------------------------------------------------------------------
__device__ __forceinline__ Coord wave_merge_path_search(int diagonal, const int *__restrict__ row_end,
                                                        int rows, int nnz)
{
    const int lane = threadIdx.x & (WAVE - 1);
    int lo = diagonal - nnz; lo = lo < 0 ? 0 : lo;
    int hi = diagonal < rows ? diagonal : rows;
    while (lo < hi) {
        const int n = hi - lo;
        const int step = (n + WAVE - 1) / WAVE;
        const int chunk_lo = lo + lane * step;          // may exceed hi for trailing lanes
        int q = chunk_lo + step; q = (q < hi ? q : hi) - 1;
        bool pred = false;                               // lanes whose chunk is empty abstain
        if (chunk_lo < hi) pred = (row_end[q] + q + 1 > diagonal);
        const unsigned long long mask = __ballot(pred);
        if (mask == 0ull) { lo = hi; break; }            // no row-end beyond the diagonal in range
        const int f = __ffsll((long long) mask) - 1;     // first chunk whose last element is past
        const int new_lo = lo + f * step;
        int new_hi = new_lo + step; new_hi = (new_hi < hi ? new_hi : hi) - 1;
        lo = new_lo; hi = new_hi;                        // answer in [new_lo, q_f]
    }
    Coord c; c.x = lo < rows ? lo : rows; c.y = diagonal - lo;
    return c;
}

// The same search as the self-searching tiles of small problems do it: round 1 probes 64 FIXED samples
// (k + 1) * rows / 64 -- the same addresses for every block, so they come from L2 --, round 2 probes 64 CONSECUTIVE
// rows around the point linear interpolation inside that bracket predicts (two cache lines); on a matrix whose row
// lengths vary smoothly that finishes it: two dependent loads instead of four, ~1.5 us less before a block's first
// nonzero is requested.  Whatever is left of the bracket goes through 64-ary rounds.  Exact; all lanes return the
// same coordinate.  M(p) = row_end[p] + p + 1 (strictly increasing), M(rows) = +inf; the point of diagonal d is
// (p, d - p) for the first p with M(p) > d.
__device__ __forceinline__ Coord wave_merge_path_search_interp(int diagonal, const int *__restrict__ row_end, int rows, int nnz)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int inf = rows + nnz + 1;                              // < 2^31
    auto m_of = [&](int p) { return p < rows ? row_end[p] + p + 1 : inf; };
    const int pk = (int) ((long long) (lane + 1) * rows / WAVE);  // lane 63: rows
    const int mk = m_of(pk);
    unsigned long long mask = __ballot(mk > diagonal);            // monotone; lane 63 is always set
    int f = __ffsll((long long) mask) - 1;
    int b = __shfl(pk, f, WAVE);
    const int m_hi = __shfl(mk, f, WAVE);
    const int p_lo = f == 0 ? -1 : __shfl(pk, f - 1, WAVE);
    const int m_lo = f == 0 ? 0 : __shfl(mk, f - 1, WAVE);
    int a = p_lo + 1;                                             // M(p) <= diagonal for p < a;  M(b) > diagonal
    if (a < b) {
        const long long g = p_lo + 1 + (long long) ((double) (diagonal - m_lo) * (double) (b - p_lo - 1) / (double) (m_hi - m_lo));
        int w0 = (int) g - WAVE / 2;
        const int w_max = b - (WAVE - 1) > a ? b - (WAVE - 1) : a;
        w0 = w0 < a ? a : w0 > w_max ? w_max : w0;               // window [w0, w0 + 63], inside [a, b] where possible
        const int p = w0 + lane;
        const bool pred = p >= b ? true : m_of(p) > diagonal;
        mask = __ballot(pred);
        f = __ffsll((long long) mask) - 1;
        if (mask == 0ull) a = w0 + WAVE;                          // the answer lies beyond the window
        else if (f == 0 && w0 > a) b = w0;                        // ... at or before its first row
        else a = b = w0 + f;                                      // found
        while (a < b) {                                           // 64-ary rounds over [a, b), M(b) > diagonal
            const int n = b - a;
            const int step = (n + WAVE - 1) / WAVE;
            const int chunk_lo = a + lane * step;
            int q = chunk_lo + step; q = (q < b ? q : b) - 1;
            bool pr = false;
            if (chunk_lo < b) pr = m_of(q) > diagonal;
            const unsigned long long mm = __ballot(pr);
            if (mm == 0ull) { a = b; break; }
            const int ff = __ffsll((long long) mm) - 1;
            const int na = a + ff * step;
            int nb = na + step; nb = (nb < b ? nb : b) - 1;
            a = na; b = nb;
        }
    }
    Coord c; c.x = b < rows ? b : rows; c.y = diagonal - b;
    return c;
}

// ref: DeviceSpmvSearchKernel, dispatch_spmv_orig.cuh:104-143 (there: one
// thread per boundary, binary search).  coords has num_tiles+1 entries.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void search_kernel(const int *__restrict__ row_end, int rows, int nnz,
                                                       int tile_items, int num_tiles, BoundaryOut out)
{
    const int wave_in_block = threadIdx.x / WAVE;
    const int boundary = blockIdx.x * (BLOCK / WAVE) + wave_in_block;
    if (boundary > num_tiles) return;
    const long long total = (long long) rows + nnz;
    long long d = (long long) boundary * tile_items;
    const int diagonal = (int) (d < total ? d : total);
    const Coord c = wave_merge_path_search(diagonal, row_end, rows, nnz);
    if ((threadIdx.x & (WAVE - 1)) == 0) emit_boundary(out, boundary, c.x, c.y, c.x > 0 ? row_end[c.x - 1] : 0);
}

// ---------------------------------------------------------------------------
// Column-band passes (no counterpart in the reference).  A matrix whose columns are spread
// uniformly over an x several times the 4 MiB of an XCD's L2 is gather-bound at the Infinity-Cache rate
// (C2: 100 M gathers in 1.2 ms, the CSR stream alone takes 0.14 ms).  Streaming the matrix B times, each
// pass multiplying only the nonzeros of one column band -- an x slice that stays in L2 -- is faster: C2
// fp32 0.83 ms with B = 3.  Whether the columns ARE spread like that is not known to the host, and a
// stateless, asynchronous call cannot wait for the answer: 64 extra blocks of the coordinate pass sample 64
// windows of 2048 consecutive nonzeros, and the tile kernel (its BAND variant) reads the 64 verdicts and runs
// either its ordinary body or the passes (run_band_passes).
// ---------------------------------------------------------------------------
constexpr int BAND_WINDOWS = WAVE;         // one verdict per lane of the wave that reads them
constexpr int BAND_WINDOW = 2048;          // consecutive nonzeros per window
constexpr int BAND_MAJORITY = 56;          // windows that must look uniform
constexpr int BAND_BITMAP_WORDS = 2048;    // 65 536 bits, one per 128-byte line of x modulo 8 MiB
// set bits expected from d distinct lines hashed uniformly: m (1 - exp(-d / m)); d = 0.93 * 2048 -> 1877
constexpr int BAND_MIN_BITS = 1877;
constexpr int BAND_COUNTER_STRIDE = 64;    // ints between the 8 claim counters of run_band_passes (they follow the verdicts)

__device__ __forceinline__ bool band_mode(const int *__restrict__ verdict)      // wave-uniform
{
    const int v = verdict[threadIdx.x & (WAVE - 1)];
    return __popcll(__ballot(v != 0)) >= BAND_MAJORITY;
}

struct BandDetectArgs {
    const int *cols; int nnz, num_cols;
    int line_shift;            // column index -> 128-byte line of x: 5 (fp32), 4 (fp64)
    int *verdict;              // BAND_WINDOWS verdicts, then the claim counters
};

// verdict[w] = 1 when window w touches (almost) as many distinct 128-byte lines of x as it has nonzeros -- no
// short-range reuse for a cache to exploit: R-MAT windows reach 0.6-0.88 of that, stencils and bands a few percent,
// uniform columns 0.975-0.99 -- AND spans at least 3/4 of the columns.  Block `w` of BAND_WINDOWS; BLOCK threads.
template <int BLOCK>
__device__ __forceinline__ void band_detect_block(const BandDetectArgs &a, int w)
{
    constexpr int NW = BLOCK / WAVE;
    __shared__ unsigned s_bits[BAND_BITMAP_WORDS];
    __shared__ int s_red[3][NW];
    const int tid = threadIdx.x;
    for (int i = tid; i < BAND_BITMAP_WORDS; i += BLOCK) s_bits[i] = 0u;
    __syncthreads();
    const long long start = a.nnz > BAND_WINDOW ? (long long) w * (a.nnz - BAND_WINDOW) / (BAND_WINDOWS - 1) : 0;
    const int len = a.nnz < BAND_WINDOW ? a.nnz : BAND_WINDOW;
    int fresh = 0, lo = 0x7fffffff, hi = -1;
    for (int j = tid; j < len; j += BLOCK) {
        const int c = a.cols[start + j];
        lo = c < lo ? c : lo; hi = c > hi ? c : hi;
        const unsigned line = ((unsigned) c >> a.line_shift) & (BAND_BITMAP_WORDS * 32u - 1u);
        const unsigned bit = 1u << (line & 31u);
        fresh += (atomicOr(&s_bits[line >> 5], bit) & bit) ? 0 : 1;
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        fresh += __shfl_xor(fresh, d, WAVE);
        const int l2 = __shfl_xor(lo, d, WAVE), h2 = __shfl_xor(hi, d, WAVE);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if ((tid & (WAVE - 1)) == 0) { s_red[0][tid / WAVE] = fresh; s_red[1][tid / WAVE] = lo; s_red[2][tid / WAVE] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < NW; ++k) {
            fresh += s_red[0][k];
            lo = s_red[1][k] < lo ? s_red[1][k] : lo; hi = s_red[2][k] > hi ? s_red[2][k] : hi;
        }
        const bool wide = 4LL * ((long long) hi - lo) >= 3LL * a.num_cols;
        a.verdict[w] = (len == BAND_WINDOW && fresh >= BAND_MIN_BITS && wide) ? 1 : 0;
        if (w < 8) a.verdict[BAND_WINDOWS + w * BAND_COUNTER_STRIDE] = 0;        // the claim counters of run_band_passes
    }
}

// stand-alone form (calls that do not run the scatter coordinate pass: prepared calls, >= 10 M rows)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void band_detect_kernel(BandDetectArgs a)
{
    band_detect_block<BLOCK>(a, (int) blockIdx.x);
}

// ---------------------------------------------------------------------------
// The same coordinates by ONE coalesced pass over the row offsets instead of
// num_tiles independent searches (each 4 dependent, scattered loads): the
// merge position of row-end r is m_r = r + row_end[r] (r row-ends and
// row_end[r] nonzeros precede it -- ties go to the row end, Appendix B.1), and
// the point of diagonal d has x(d) = #{r : m_r < d}.  So thread r owns exactly
// the tile boundaries d = t*tile_items with m_{r-1} < d <= m_r and writes
// (r, d - r) for them; thread `rows` owns the boundaries past the last row end.
// Usually a thread owns 0 or 1 boundary; a row longer than a tile owns many, and
// a wave then fills one such row's run of boundaries cooperatively (a giant row
// of 2^26 nonzeros owns ~37 000 of them).  Measured on MI355X: 3-15 us where
// the search kernel took 27-52 us.
// ---------------------------------------------------------------------------
template <int BLOCK, int TILE_ITEMS, bool VEC>
__device__ __forceinline__ void coords_scatter_block(const int *__restrict__ row_offsets, int rows, int nnz, int num_tiles,
                                                     const BoundaryOut &out, unsigned block)
{
    // With M(i) = (i - 1) + row_offsets[i] (i >= 1; the merge position of row-end i - 1) and
    // M(0) = -1, row r owns the boundaries t with M(r) < t*TILE_ITEMS <= M(r + 1); row index
    // `rows` owns the ones past M(rows).  A thread takes 4 consecutive r (one 16-byte load).
    // A boundary owned by row r lies INSIDE row r (r row-ends consumed, between row_offsets[r] and
    // row_offsets[r + 1] nonzeros), so the row's first nonzero is o[j] -- what tile_kernel_snap wants to know.
    const int lane = threadIdx.x & (WAVE - 1);
    const long long gid = (long long) block * BLOCK + threadIdx.x;
    const int total = rows + nnz;                              // < 2^31
    const long long base = gid * 4;                            // first r of this thread
    int o[5];                                                  // row_offsets[base .. base + 4]
    if (VEC && base + 4 <= rows) {
        const int4v v = *reinterpret_cast<const int4v *>(row_offsets + base);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; o[4] = row_offsets[base + 4];
    } else {
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = base + j <= rows ? row_offsets[base + j] : 0;
    }
    int t_lo[4], t_hi[4];
    bool any_long = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long r = base + j;
        t_lo[j] = 1; t_hi[j] = 0;
        if (r <= rows) {
            const int m_lo = r == 0 ? -1 : (int) r - 1 + o[j];
            t_lo[j] = m_lo < 0 ? 0 : m_lo / TILE_ITEMS + 1;
            t_hi[j] = r < rows ? ((int) r + o[j + 1]) / TILE_ITEMS : num_tiles;
            const int count = t_hi[j] - t_lo[j] + 1;
            if (count > 0 && count <= 2) {
                for (int t = t_lo[j]; t <= t_hi[j]; ++t) {
                    const long long d = (long long) t * TILE_ITEMS;
                    emit_boundary(out, t, (int) r, (int) (d < total ? d : total) - (int) r, o[j]);
                }
            }
            any_long |= count > 2;
        }
    }
    // rows longer than two tiles: the wave fills each such run of boundaries together
    if (__ballot(any_long) == 0ull) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long pending = __ballot(t_hi[j] - t_lo[j] + 1 > 2);
        while (pending) {
            const int src = __ffsll((long long) pending) - 1;
            pending &= pending - 1;
            const int lo = __shfl(t_lo[j], src, WAVE), hi = __shfl(t_hi[j], src, WAVE);
            const int rr = (int) __shfl((int) base, src, WAVE) + j;
            const int rs = __shfl(o[j], src, WAVE);
            for (int t = lo + lane; t <= hi; t += WAVE) {
                const long long d = (long long) t * TILE_ITEMS;
                emit_boundary(out, t, rr, (int) (d < total ? d : total) - rr, rs);
            }
        }
    }
}

template <int BLOCK, int TILE_ITEMS, bool VEC, bool DETECT = false>
__global__ __launch_bounds__(BLOCK) void coords_scatter_kernel(const int *__restrict__ row_offsets, int rows, int nnz,
                                                               int num_tiles, BoundaryOut out, BandDetectArgs da)
{
    // DETECT: the first BAND_WINDOWS blocks of the grid sample the column windows (column-band passes, above) -- first, so
    // that their two dependent memory round trips run under the coordinate work instead of after it
    if constexpr (DETECT) {
        if ((int) blockIdx.x < BAND_WINDOWS) { band_detect_block<BLOCK>(da, (int) blockIdx.x); return; }
    }
    coords_scatter_block<BLOCK, TILE_ITEMS, VEC>(row_offsets, rows, nnz, num_tiles, out, DETECT ? blockIdx.x - BAND_WINDOWS : blockIdx.x);
}

// ---------------------------------------------------------------------------
// The same coordinates WITHOUT reading every row offset: one THREAD per tile boundary, interpolation search.
// With M(p) = row_end[p] + p + 1 (the merge position just past row-end p; strictly increasing) and
// M(rows) = +inf, the point of diagonal d is (p, d - p) for the first p in [0, rows] with M(p) > d (for
// p > d or p < d - nnz the predicate holds / fails by itself, so the search bounds of Appendix B.2 are implied).
//   1. every block loads the same K + 1 samples M(k * rows / K) into LDS (L2 hits after the first block);
//   2. a thread finds its bracket among them (10 LDS steps) and runs up to four secant steps -- evaluate M at the
//      linearly interpolated point, shrink the bracket -- then a short walk; on a matrix whose row lengths vary
//      smoothly (grids, bands, dense blocks, uniform random rows) that ends within a row or two of the first guess;
//   3. otherwise (a giant row, a power-law neighbourhood) an exact binary search over what is left of the bracket.
// Always exact -- the result is bit for bit the scatter pass's.  The kernel is latency-bound: its time is that of
// its slowest thread, ~2-8 us on regular matrices and <= 17 us (a full binary search of a bracket) on any matrix,
// whatever the row count, where the scatter pass reads all of row_offsets: 8 us at 3 M rows, 12 at 8 M, 20-23 at
// 16.8 M.  The dispatcher therefore uses it from 10 M rows up (measured: band5 19.1 -> 7.5 us, C4 22.7 -> 11.5,
// grid2d-4096 20.3 -> 16.5; below that size the scatter pass is at least as fast on irregular matrices).
// ---------------------------------------------------------------------------
constexpr int INTERP_SAMPLES = 1024;
// s_m: SAMPLES + 1 ints of LDS (M values fit 32 bits: rows + nnz + 1 < 2^31); has a barrier inside
template <int BLOCK, int SAMPLES = INTERP_SAMPLES>
__device__ __forceinline__ void coords_interp_block(const int *__restrict__ row_end, int rows, int nnz, int tile_items, int num_tiles,
                                                    const BoundaryOut &out, unsigned block, int *s_m)
{
    static_assert(SAMPLES % BLOCK == 0, "whole rounds of sample loads");
    const int total = rows + nnz;
    auto sample_pos = [&](int k) { return (int) ((long long) k * rows / SAMPLES); };
    auto m_of = [&](int p) { return p < rows ? row_end[p] + p + 1 : total + 1; };
    for (int k = threadIdx.x; k < SAMPLES; k += BLOCK) s_m[k] = m_of(sample_pos(k));
    if (threadIdx.x == 0) s_m[SAMPLES] = total + 1;          // M(rows) = +inf
    __syncthreads();
    const long long boundary_ll = (long long) block * BLOCK + threadIdx.x;
    if (boundary_ll > num_tiles) return;
    const int boundary = (int) boundary_ll;
    long long dl = (long long) boundary * tile_items;
    const int d = (int) (dl < total ? dl : total);
    // bracket: first sample k with M(p_k) > d  (k = SAMPLES always qualifies)
    int klo = 0, khi = SAMPLES;
    while (klo < khi) { const int mid = (klo + khi) >> 1; if (s_m[mid] > d) khi = mid; else klo = mid + 1; }
    int b = sample_pos(klo);                                       // M(b) = m_hi > d
    int m_hi = s_m[klo];
    int p_lo = klo == 0 ? -1 : sample_pos(klo - 1);                // M(p_lo) = m_lo <= d   (p_lo = -1: nothing below)
    int m_lo = klo == 0 ? 0 : s_m[klo - 1];
    // secant steps: evaluate M at the interpolated point, keep the half that holds the answer
    for (int it = 0; it < 4 && b - p_lo > 1; ++it) {
        long long g = p_lo + 1 + (long long) ((double) (d - m_lo) * (double) (b - p_lo - 1) / (double) (m_hi - m_lo));
        const int p = (int) (g <= p_lo ? p_lo + 1 : g >= b ? b - 1 : g);
        const int mp = m_of(p);
        if (mp > d) { b = p; m_hi = mp; } else { p_lo = p; m_lo = mp; }
    }
    // short walk from both ends, then an exact binary search over what is left (nothing, on a smooth matrix)
    int a = p_lo + 1;                                              // M(p) <= d for p < a;  M(b) > d
    for (int step = 0; step < 2 && a < b; ++step) { if (m_of(a) > d) b = a; else ++a; }
    for (int step = 0; step < 2 && a < b; ++step) { if (m_of(b - 1) > d) --b; else a = b; }
    while (a < b) { const int mid = (int) (((long long) a + b) >> 1); if (m_of(mid) > d) b = mid; else a = mid + 1; }
    const int x = b < rows ? b : rows;
    emit_boundary(out, boundary, x, d - b, x > 0 ? row_end[x - 1] : 0);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void coords_interp_kernel(const int *__restrict__ row_end, int rows, int nnz, int tile_items,
                                                              int num_tiles, BoundaryOut out)
{
    __shared__ int s_m[INTERP_SAMPLES + 1];
    coords_interp_block<BLOCK>(row_end, rows, nnz, tile_items, num_tiles, out, blockIdx.x, s_m);
}

}  // namespace mspmv
