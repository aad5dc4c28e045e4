// mspmv_radix.hpp -- one pass of the stable least-significant-digit radix sort that rebuilds a matrix on the device, shared by the
// transpose (mspmv_transpose.hip: A's nonzeros sorted by column) and the COO build (mspmv_coo.hip: triples sorted by column digits,
// then row digits).  D = 8 bits per pass over tiles of 2048 items carrying (key, other index, original position, value) as sequential
// traffic.  A pass is three steps, none of which waits on another workgroup:
//   upsweep    per tile, the digit histogram (integer atomics in LDS) -> counts[digit * tiles + tile];
//   scan       exclusive scan of that table (mspmv_scan.hpp) -> where digit d of tile t starts in the pass's output;
//   downsweep  each item's stable rank inside its tile: per wave, rounds of 64 consecutive items; the lanes holding the same digit are
//              the AND of D ballots, the rank is the popcount of those in lower lanes plus the wave's running count of the digit
//              (LDS, item order); then the waves' counts are scanned per digit, the tile is staged in LDS in digit order and written
//              out so that every digit's run is one contiguous store stream.
// Every output position is a function of the input alone.  Also here: the finishing kernel that turns sorted keys into offsets by
// boundary detection, and the small fill / gather kernels both users launch.  Included inside an anonymous namespace of each
// translation unit, after mspmv_scan.hpp and `using namespace mspmv` (grid_for is mspmv_internal.hpp's).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

constexpr int TR_BLOCK = 256, TR_WAVES = TR_BLOCK / 64, TR_IPT = 8, TR_TILE = TR_BLOCK * TR_IPT;
constexpr int TR_BITS = 8, TR_DIGITS = 1 << TR_BITS;
constexpr int TR_WAVE_ITEMS = TR_TILE / TR_WAVES;     // a wave's contiguous share of a tile: TR_IPT rounds of 64 items

// where a downsweep's items come from: a set written by the previous pass; the CSR arrays (key = column, the row by search, k = the
// position); or two plain index arrays in input order (in.key, in.row; k = the position, values from csr_vals)
enum { SRC_ITEMS = 0, SRC_CSR = 1, SRC_COO = 2 };

static int key_bits(int n)                              // bits of the largest index below n, n - 1
{
    int b = 0;
    for (unsigned v = n > 1 ? (unsigned) (n - 1) : 0u; v; v >>= 1) ++b;
    return b;
}
static int radix_passes(int n) { return std::max(1, (key_bits(n) + TR_BITS - 1) / TR_BITS); }

// (the set's size with the alignment of its four arrays)
static uint64_t set_bytes(int nnz, int value_bytes)
{
    const uint64_t n = (uint64_t) std::max(nnz, 1);
    return 3 * align256(n * 4) + align256(n * value_bytes);
}

template <typename V>
struct Items {                                          // one set of arrays of the sort (n entries each)
    int *key, *row, *k; V *val;
};
template <typename V>
static Items<V> items_at(char *base, uint64_t off, int nnz)
{
    const uint64_t n = (uint64_t) std::max(nnz, 1);
    Items<V> s;
    s.key = reinterpret_cast<int *>(base + off);
    s.row = reinterpret_cast<int *>(base + off + align256(n * 4));
    s.k = reinterpret_cast<int *>(base + off + 2 * align256(n * 4));
    s.val = reinterpret_cast<V *>(base + off + 3 * align256(n * 4));
    return s;
}
// ---- upsweep: digit histogram of one tile ----------------------------------------------------------------------------------
__global__ __launch_bounds__(TR_BLOCK) void tr_upsweep_kernel(const int *__restrict__ keys, int nnz, int shift, long long tiles,
                                                              int *__restrict__ counts)
{
    __shared__ int s_hist[TR_DIGITS];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long) blockIdx.x * TR_TILE;
    for (int i = 0; i < TR_IPT; ++i) {
        const long long j = base + i * TR_BLOCK + threadIdx.x;
        if (j < nnz) atomicAdd(&s_hist[(keys[j] >> shift) & (TR_DIGITS - 1)], 1);
    }
    __syncthreads();
    counts[(long long) threadIdx.x * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

// ---- downsweep: stable rank by ballots, staged in LDS, contiguous runs per digit ---------------------------------------------
// SRC: where the items come from (above).  VALS: values travel.
template <typename V, int SRC, bool VALS>
__global__ __launch_bounds__(TR_BLOCK) void tr_downsweep_kernel(const int *__restrict__ off, const int *__restrict__ csr_cols,
                                                                const V *__restrict__ csr_vals, int rows, Items<V> in, int nnz,
                                                                int shift, long long tiles, const int *__restrict__ digit_offs,
                                                                int *__restrict__ out_key, int *__restrict__ out_row,
                                                                int *__restrict__ out_k, V *__restrict__ out_val)
{
    __shared__ int s_wc[TR_WAVES][TR_DIGITS];           // per wave: running count of each digit, then the wave's offset in the digit
    __shared__ int s_goff[TR_DIGITS], s_lstart[TR_DIGITS];
    __shared__ int s_key[TR_TILE], s_row[TR_TILE], s_k[TR_TILE];
    __shared__ V s_val[VALS ? TR_TILE : 1];
    __shared__ int s_range[2], s_tmp[TR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile_base = (long long) blockIdx.x * TR_TILE;
    const int tile_n = (int) std::min<long long>(TR_TILE, nnz - tile_base);
    for (int w = 0; w < TR_WAVES; ++w) s_wc[w][threadIdx.x] = 0;
    s_goff[threadIdx.x] = digit_offs[(long long) threadIdx.x * tiles + blockIdx.x];
    int r_lo = 0, r_hi = 0;
    if constexpr (SRC == SRC_CSR) {
        block_row_range(off, rows, (int) tile_base, (int) tile_base + tile_n - 1, s_range);     // (syncs)
        r_lo = s_range[0]; r_hi = s_range[1];
    } else {
        __syncthreads();
    }
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;      // lanes below this one
    int key[TR_IPT], row[TR_IPT], kk[TR_IPT], rank[TR_IPT];
    V val[TR_IPT];
    for (int i = 0; i < TR_IPT; ++i) {
        const int t = wave * TR_WAVE_ITEMS + i * 64 + lane;                   // item index inside the tile (item order = input order)
        const bool valid = t < tile_n;
        const int j = (int) tile_base + t;
        key[i] = 0; row[i] = 0; kk[i] = j; val[i] = (V) 0;
        if (valid) {
            if constexpr (SRC == SRC_CSR) {
                key[i] = csr_cols[j];
                row[i] = row_of(off, r_lo, r_hi, j);
                if constexpr (VALS) val[i] = csr_vals[j];
            } else if constexpr (SRC == SRC_COO) {
                key[i] = in.key[j]; row[i] = in.row[j];
                if constexpr (VALS) val[i] = csr_vals[j];
            } else {
                key[i] = in.key[j]; row[i] = in.row[j]; kk[i] = in.k[j];
                if constexpr (VALS) val[i] = in.val[j];
            }
        }
        const int d = (key[i] >> shift) & (TR_DIGITS - 1);
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < TR_BITS; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? m : ~m;
        }
        // the wave's count of digit d so far; the lowest lane of the group adds the group (all lanes read before it writes)
        const int before = valid ? s_wc[wave][d] : 0;
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & lt) == 0) s_wc[wave][d] = before + __popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rank[i] = before + __popcll(peers & lt);
    }
    __syncthreads();
    {   // per digit (thread = digit): the waves' offsets inside the digit's run, and the run's start in the tile
        const int d = threadIdx.x;
        int sum = 0;
        for (int w = 0; w < TR_WAVES; ++w) { const int c = s_wc[w][d]; s_wc[w][d] = sum; sum += c; }
        const int incl = block_inclusive_scan(sum, s_tmp);                    // (syncs)
        s_lstart[d] = incl - sum;
    }
    __syncthreads();
    for (int i = 0; i < TR_IPT; ++i) {
        const int t = wave * TR_WAVE_ITEMS + i * 64 + lane;
        if (t < tile_n) {
            const int d = (key[i] >> shift) & (TR_DIGITS - 1);
            const int p = s_lstart[d] + s_wc[wave][d] + rank[i];
            s_key[p] = key[i]; s_row[p] = row[i]; s_k[p] = kk[i];
            if constexpr (VALS) s_val[p] = val[i];
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tile_n; t += TR_BLOCK) {
        const int k = s_key[t];
        const int d = (k >> shift) & (TR_DIGITS - 1);
        const int p = s_goff[d] + (t - s_lstart[d]);
        out_key[p] = k; out_row[p] = s_row[t];
        if (out_k) out_k[p] = s_k[t];
        if constexpr (VALS) out_val[p] = s_val[t];
    }
}

// ---- finishing: offsets[c] = the number of entries with key < c, by boundary detection ---------------------------------------
// Entry j (0 <= j <= nnz, key[-1] = -1, key[nnz] = cols) writes j at columns key[j-1]+1 .. key[j].  A span longer than a wave is
// written by the whole wave (lanes taking turns by ballot) so that a long run of empty columns costs no single lane a long loop.
__global__ __launch_bounds__(256) void tr_offsets_kernel(const int *__restrict__ keys, int nnz, int cols, int *__restrict__ offsets_t)
{
    const long long j = (long long) blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = -1;
    if (j <= nnz) {
        lo = j == 0 ? 0 : keys[j - 1] + 1;
        hi = j == nnz ? cols : keys[j];
    }
    const bool longspan = hi - lo >= 64;
    if (!longspan) for (int c = lo; c <= hi; ++c) offsets_t[c] = (int) j;
    unsigned long long todo = __ballot(longspan);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int slo = __shfl(lo, src, 64), shi = __shfl(hi, src, 64);
        const int sj = __shfl((int) j, src, 64);
        for (long long c = (long long) slo + lane; c <= shi; c += 64) offsets_t[c] = sj;
    }
}

__global__ __launch_bounds__(256) void tr_fill_kernel(int *__restrict__ out, long long n, int v)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

template <typename V>
__global__ __launch_bounds__(256) void tr_values_kernel(const V *__restrict__ vals, const int *__restrict__ perm, V *__restrict__ vals_t,
                                                        int nnz)
{
    const long long j = (long long) blockIdx.x * 256 + threadIdx.x;
    if (j < nnz) vals_t[j] = vals[perm[j]];
}

static int launched(hipStream_t stream, int debug_sync, const char *name, unsigned grid)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int) e;
    if (debug_sync) { printf("mspmv: %s<<<%u, 256>>>\n", name, grid); fflush(stdout); e = hipStreamSynchronize(stream); }
    return (int) e;
}

// the three launches that turn the digit x tile table of a pass into its exclusive scan
static int scan_table(const int *counts, long long table, int *bsum, int *offs, hipStream_t stream, int debug_sync)
{
    const unsigned sblocks = grid_for(table, SCAN_CHUNK);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(sblocks), dim3(SCAN_BLOCK), 0, stream, counts, table, bsum);
    if (int e = launched(stream, debug_sync, "scan_reduce_kernel", sblocks)) return e;
    hipLaunchKernelGGL(scan_blocksums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, stream, bsum, (int) sblocks);
    if (int e = launched(stream, debug_sync, "scan_blocksums_kernel", 1)) return e;
    hipLaunchKernelGGL(scan_apply_kernel, dim3(sblocks), dim3(SCAN_BLOCK), 0, stream, counts, table, bsum, offs);
    return launched(stream, debug_sync, "scan_apply_kernel", sblocks);
}
