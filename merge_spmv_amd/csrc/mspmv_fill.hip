// mspmv_fill.hip -- the level-of-fill pattern of a square CSR pattern on the device: the symbolic phase of ILU(p) / IC(p)
// (mspmv_csr_fill_* of include/mspmv_fill.h; libmspmv_fill.so).
//
// Definition.  Every stored entry has level 0, every other position +inf, and lev(i, j) = min(lev(i, j), lev(i, m) + lev(m, j) + 1)
// over m < min(i, j).  F_p holds every position of level <= p, in canonical CSR, with its level and its index in A's arrays (-1: fill).
//
// Scheme: a LEVELLED PRODUCT, one round per level -- the expand - sort - compress of mspmv_gemm.hip with (min, +) for (+, x).
// After round l the state S is F_l exactly.  Round l pairs every entry (i, m) of the strict lower part of S with every entry (m, j)
// of the strict upper part of row m; the pair is a candidate of level a + b + 1.  An entry of final level l >= 1 has a pair with
// a + b + 1 = l, whose two members have final levels below l and so stand in F_(l-1) with those levels: round l keeps the pairs with
// a + b + 1 == l and no others, and every candidate it keeps is a true path, so nothing is ever entered above its level.
//   upper    one lane per row: where the row's entries right of the diagonal start;
//   rows     the row of every entry of S, in equal tiles whatever the row lengths (a block's row range, a search inside it);
//   lengths  len[e] = the entries right of the diagonal in row col[e], for e below the diagonal; per block their 64-bit sum;
//   total    one block adds the sums; the host reads the total (8 bytes) and REFUSES, before anything proportional to it is allocated,
//            a round whose entries + candidates + rows exceed MAX_ITEMS;
//   keep     the candidates cut into tiles of FILL_TILE whatever the row lengths: a tile finds the entries of its first and last
//            candidate by a search of the scanned lengths and every lane the entry of its candidate inside that range -- one row of a
//            million entries is no single lane's loop.  keep[q] = 1 for a pair of this round's level; the flags are scanned and the
//            host reads how many pairs are kept (4 bytes).  None kept: the round ends, S stays;
//   expand   the same tiles again: a kept pair writes its triple behind S's entries, at the place the scan gave it.  A pair of
//            another level is written nowhere: it is neither sorted nor compacted;
//   sort     S's entries, then the kept pairs, sorted STABLY by (row, column) (coo_run, mspmv_coo.hpp), the value a 64-bit word
//            level << 32 | source;
//   compact  runs of equal (row, column) flagged and scanned (dup_flags_kernel, scan_table); the host reads the count (4 bytes) and
//            allocates the next S; the head of a run writes ITS word and no lane walks a run: the sort is stable and S's entries
//            come first, so the head is S's own entry where the position stood in S (its level is below the round's), and
//            otherwise one of the run's kept pairs, which all hold the same word (the round's level, no source).
// No atomics on global memory, no workgroup waits on another, integer arithmetic only.  The analysis is synchronous and owns its
// storage; mspmv_csr_fill_values_* is one launch that allocates nothing and reads nothing back.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/mspmv_fill.h"
#include "mspmv_internal.hpp"

struct mspmv_csr_fill {
    mspmv_csr_fill_info_t info{};
    int32_t *d_off = nullptr, *d_col = nullptr, *d_lev = nullptr, *d_src = nullptr;
};

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range, the three scan kernels

#include "mspmv_radix.hpp"     // launched, scan_table, tr_fill_kernel, TR_TILE

#include "mspmv_coo.hpp"       // coo_layout, coo_temp_bytes, coo_run, dup_flags_kernel, dup_offsets_kernel, DUP_CHUNK

typedef long long Packed;                                            // level << 32 | (uint32) source: the smaller word is the better entry

constexpr int FILL_BLOCK = 256, FILL_TILE = TR_TILE;                 // 2048 entries or candidates per block
constexpr int FILL_MAX_LEVEL = 32;
constexpr int FILL_MAX_ROWS = 1 << 30;

__device__ __forceinline__ Packed fill_pack(int level, int source) { return (Packed) level << 32 | (Packed) (unsigned) source; }
__device__ __forceinline__ int fill_level(Packed w) { return (int) (w >> 32); }

// S = A: entry e has level 0 and source e
__global__ __launch_bounds__(FILL_BLOCK) void fill_init_kernel(Packed *__restrict__ pk, int nnz)
{
    const long long e = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (e < nnz) pk[e] = fill_pack(0, (int) e);
}

__global__ __launch_bounds__(FILL_BLOCK) void fill_copy_kernel(const int *__restrict__ src, int *__restrict__ dst, long long words)
{
    const long long i = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (i < words) dst[i] = src[i];
}

// ustart[r] = the first entry of row r whose column is above r (the row's end if there is none)
__global__ __launch_bounds__(FILL_BLOCK) void fill_upper_kernel(const int *__restrict__ off, const int *__restrict__ col, int rows,
                                                                int *__restrict__ ustart)
{
    const long long r = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (r >= rows) return;
    int lo = off[r], hi = off[r + 1];
    while (lo < hi) {
        const int mid = (int) (((long long) lo + hi) >> 1);
        if (col[mid] > r) hi = mid; else lo = mid + 1;
    }
    ustart[r] = lo;
}

// erow[e] = the row of entry e; len[e] = the candidates under e; partial[block] = the block's 64-bit sum of them
__global__ __launch_bounds__(FILL_BLOCK) void fill_lengths_kernel(const int *__restrict__ off, const int *__restrict__ col, int rows, int nnz,
                                                                  const int *__restrict__ ustart, int *__restrict__ erow,
                                                                  int *__restrict__ len, long long *__restrict__ partial)
{
    __shared__ long long s_sum[FILL_BLOCK];
    __shared__ int s_range[2];
    const long long e0 = (long long) blockIdx.x * FILL_TILE;
    const int e1 = (int) std::min<long long>(e0 + FILL_TILE, nnz) - 1;
    block_row_range(off, rows, (int) e0, e1, s_range);
    long long t = 0;
    for (int e = (int) e0 + (int) threadIdx.x; e <= e1; e += FILL_BLOCK) {
        const int r = row_of(off, s_range[0], s_range[1], e), m = col[e];
        const int l = m >= 0 && m < r ? off[m + 1] - ustart[m] : 0;      // (a column outside [0, rows) has no pairs: nothing is read through it)
        erow[e] = r; len[e] = l;
        t += l;
    }
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int d = FILL_BLOCK / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}

__global__ __launch_bounds__(FILL_BLOCK) void fill_total_kernel(const long long *__restrict__ partial, long long blocks,
                                                                long long *__restrict__ total)
{
    __shared__ long long s_sum[FILL_BLOCK];
    long long t = 0;
    for (long long i = threadIdx.x; i < blocks; i += FILL_BLOCK) t += partial[i];
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int d = FILL_BLOCK / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_sum[0];
}

// candidate q belongs to the LAST entry e with start[e] <= q (entries of no candidates are skipped by the search), the pair of e =
// (r, m) with entry ustart[m] + q - start[e] of row m.  Returns whether the pair has the round's level; e and j are the two entries.
__device__ __forceinline__ bool fill_pair(const int *__restrict__ start, const int *__restrict__ col, const Packed *__restrict__ pk, int nnz,
                                          const int *__restrict__ ustart, int e_lo, int e_hi, int q, int round, int &e, int &j)
{
    e = row_of(start, e_lo, e_hi, q);
    j = min(max(ustart[col[e]] + (q - start[e]), 0), nnz - 1);
    return fill_level(pk[e]) + fill_level(pk[j]) + 1 == round;
}

// keep[q] = 1 when candidate q has the round's level
__global__ __launch_bounds__(FILL_BLOCK) void fill_keep_kernel(const int *__restrict__ start, const int *__restrict__ col,
                                                               const Packed *__restrict__ pk, int nnz, const int *__restrict__ ustart,
                                                               int products, int round, int *__restrict__ keep)
{
    __shared__ int s_e[2];
    const int q0 = (int) blockIdx.x * FILL_TILE;                     // (nnz + products <= MAX_ITEMS: no wrap, here or in q0 + FILL_TILE)
    const int q1 = min(q0 + FILL_TILE, products);
    block_row_range(start, nnz, q0, q1 - 1, s_e);                    // (syncs)
    for (int q = q0 + (int) threadIdx.x; q < q1; q += FILL_BLOCK) {
        int e, j;
        keep[q] = fill_pair(start, col, pk, nnz, ustart, s_e[0], s_e[1], q, round, e, j) ? 1 : 0;
    }
}

// a kept candidate writes (row of e, column of j, the round's level and no source) at pos[q]: behind S's own entries
__global__ __launch_bounds__(FILL_BLOCK) void fill_expand_kernel(const int *__restrict__ start, const int *__restrict__ erow,
                                                                 const int *__restrict__ col, const Packed *__restrict__ pk, int nnz,
                                                                 const int *__restrict__ ustart, int products, int round,
                                                                 const int *__restrict__ pos, int *__restrict__ out_row,
                                                                 int *__restrict__ out_col, Packed *__restrict__ out_pk)
{
    __shared__ int s_e[2];
    const int q0 = (int) blockIdx.x * FILL_TILE;
    const int q1 = min(q0 + FILL_TILE, products);
    block_row_range(start, nnz, q0, q1 - 1, s_e);                    // (syncs)
    for (int q = q0 + (int) threadIdx.x; q < q1; q += FILL_BLOCK) {
        const int p = pos[q];
        if (pos[q + 1] == p) continue;                               // not kept
        int e, j;
        (void) fill_pair(start, col, pk, nnz, ustart, s_e[0], s_e[1], q, round, e, j);
        out_row[p] = erow[e]; out_col[p] = col[j]; out_pk[p] = fill_pack(round, -1);
    }
}

// the head of a run of equal (row, column) writes the run's column and its own word at pos[j] (S's entry, or one of equal pairs)
__global__ __launch_bounds__(FILL_BLOCK) void fill_compact_kernel(const int *__restrict__ pos, const int *__restrict__ cols,
                                                                  const Packed *__restrict__ pk, int n, int *__restrict__ cols_out,
                                                                  Packed *__restrict__ pk_out)
{
    const long long j = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int p = pos[j];
    if (pos[j + 1] == p) return;                                     // not a head
    cols_out[p] = cols[j];
    pk_out[p] = pk[j];
}

// levels and sources out of the words; present[l] = 1 for the largest level l of every block
__global__ __launch_bounds__(FILL_BLOCK) void fill_unpack_kernel(const Packed *__restrict__ pk, int n, int *__restrict__ lev,
                                                                 int *__restrict__ src, int *__restrict__ present)
{
    __shared__ int s_max[FILL_BLOCK];
    const long long e = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    int l = 0;
    if (e < n) {
        const Packed w = pk[e];
        l = fill_level(w);
        lev[e] = l; src[e] = (int) (unsigned) (w & 0xffffffffLL);
    }
    s_max[threadIdx.x] = l;
    __syncthreads();
    for (int d = FILL_BLOCK / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) present[s_max[0]] = 1;
}

// filled[e] = values[source[e]], +0.0 for a fill entry: moved, never recomputed
template <typename V>
__global__ __launch_bounds__(FILL_BLOCK) void fill_values_kernel(const int *__restrict__ src, const V *__restrict__ values,
                                                                 V *__restrict__ filled, int n)
{
    const long long e = (long long) blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int s = src[e];
    filled[e] = s >= 0 ? values[s] : V(0);
}

struct DevBuf {                                                      // device memory that leaves with its scope unless released
    char *p = nullptr;
    ~DevBuf() { if (p) (void) hipFree(p); }
    bool alloc(uint64_t bytes) { return hipMalloc(reinterpret_cast<void **>(&p), (size_t) std::max<uint64_t>(bytes, 256)) == hipSuccess; }
    template <typename T> T *as(uint64_t off = 0) const { return reinterpret_cast<T *>(p + off); }
    template <typename T> T *release() { T *r = reinterpret_cast<T *>(p); p = nullptr; return r; }
    void swap(DevBuf &o) { std::swap(p, o.p); }
};

static int fill_read(void *h, const void *d, size_t bytes, hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return (int) e;
}

// a copy on the device by a kernel of this file: the runtime's own device-to-device copy at times held the calling thread for 360-500
// ms between two copies of a few hundred MB (a kernel trace of analyses of the 2000 x 2000 grid: 6.5 ms of kernels in a span of 372 ms)
static int fill_copy(void *dst, const void *src, uint64_t bytes, hipStream_t stream, int debug_sync)
{
    if (bytes == 0) return hipSuccess;
    const long long words = (long long) (bytes / 4);                 // (every array here is of 4- or 8-byte items)
    const unsigned g = grid_for(words, FILL_BLOCK);
    hipLaunchKernelGGL(fill_copy_kernel, dim3(g), dim3(FILL_BLOCK), 0, stream, static_cast<const int *>(src), static_cast<int *>(dst), words);
    return launched(stream, debug_sync, "fill_copy_kernel", g);
}

static int fill_analyse(mspmv_csr_fill &f, const int32_t *d_off, const int32_t *d_cols, hipStream_t stream, int debug_sync)
{
    const int rows = f.info.rows, level = f.info.level;
    int n = f.info.nnz;                                              // the entries of S
    const uint64_t rbytes = ((uint64_t) rows + 1) * 4;
    DevBuf s_off, s_col, s_pk;                                       // S
    if (!s_off.alloc(rbytes) || !s_col.alloc((uint64_t) n * 4) || !s_pk.alloc((uint64_t) n * 8)) return hipErrorOutOfMemory;
    if (int e = fill_copy(s_off.p, d_off, rbytes, stream, debug_sync)) return e;
    if (int e = fill_copy(s_col.p, d_cols, (uint64_t) n * 4, stream, debug_sync)) return e;
    if (n > 0) {
        const unsigned g = grid_for(n, FILL_BLOCK);
        hipLaunchKernelGGL(fill_init_kernel, dim3(g), dim3(FILL_BLOCK), 0, stream, s_pk.as<Packed>(), n);
        if (int e = launched(stream, debug_sync, "fill_init_kernel", g)) return e;
    }
    const unsigned rgrid = grid_for(rows, FILL_BLOCK), ogrid = grid_for((long long) rows + 1, 256);
    for (int round = 1; round <= level && n > 0; ++round) {
        // ---- 1. the candidates of every entry, and their count
        const long long blocks = ((long long) n + FILL_TILE - 1) / FILL_TILE;
        uint64_t o = 0;
        const uint64_t total_off = o; o += 256;
        const uint64_t partial_off = o; o = align256(o + (uint64_t) blocks * 8);
        const uint64_t ustart_off = o; o = align256(o + (uint64_t) rows * 4);
        const uint64_t erow_off = o; o = align256(o + (uint64_t) n * 4);
        const uint64_t len_off = o; o = align256(o + (uint64_t) n * 4);
        const uint64_t start_off = o; o = align256(o + ((uint64_t) n + 1) * 4);
        const uint64_t bsum_off = o; o = align256(o + (uint64_t) (((long long) n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
        DevBuf pre;
        if (!pre.alloc(o)) return hipErrorOutOfMemory;
        int *ustart = pre.as<int>(ustart_off), *erow = pre.as<int>(erow_off), *len = pre.as<int>(len_off), *start = pre.as<int>(start_off);
        hipLaunchKernelGGL(fill_upper_kernel, dim3(rgrid), dim3(FILL_BLOCK), 0, stream, s_off.as<int>(), s_col.as<int>(), rows, ustart);
        if (int e = launched(stream, debug_sync, "fill_upper_kernel", rgrid)) return e;
        hipLaunchKernelGGL(fill_lengths_kernel, dim3((unsigned) blocks), dim3(FILL_BLOCK), 0, stream, s_off.as<int>(), s_col.as<int>(), rows, n,
                           ustart, erow, len, pre.as<long long>(partial_off));
        if (int e = launched(stream, debug_sync, "fill_lengths_kernel", (unsigned) blocks)) return e;
        hipLaunchKernelGGL(fill_total_kernel, dim3(1), dim3(FILL_BLOCK), 0, stream, pre.as<long long>(partial_off), blocks,
                           pre.as<long long>(total_off));
        if (int e = launched(stream, debug_sync, "fill_total_kernel", 1)) return e;
        long long products = 0;
        if (int e = fill_read(&products, pre.as<long long>(total_off), 8, stream)) return e;
        if (products == 0) break;                                    // (no pair at all: nothing of any level can follow)
        if (products < 0 || (long long) rows + n + products > MAX_ITEMS) return hipErrorInvalidValue;      // the count limit
        if (int e = scan_table(len, n, pre.as<int>(bsum_off), start, stream, debug_sync)) return e;
        // ---- 2. which candidates have this round's level, and how many
        o = 0;
        const uint64_t keep_off = o; o = align256(o + (uint64_t) products * 4);
        const uint64_t kpos_off = o; o = align256(o + ((uint64_t) products + 1) * 4);
        const uint64_t kbsum_off = o; o = align256(o + (uint64_t) ((products + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
        DevBuf kept_buf;
        if (!kept_buf.alloc(o)) return hipErrorOutOfMemory;
        int *keep = kept_buf.as<int>(keep_off), *kpos = kept_buf.as<int>(kpos_off);
        const unsigned egrid = grid_for(products, FILL_TILE);
        hipLaunchKernelGGL(fill_keep_kernel, dim3(egrid), dim3(FILL_BLOCK), 0, stream, start, s_col.as<int>(), s_pk.as<Packed>(), n, ustart,
                           (int) products, round, keep);
        if (int e = launched(stream, debug_sync, "fill_keep_kernel", egrid)) return e;
        if (int e = scan_table(keep, products, kept_buf.as<int>(kbsum_off), kpos, stream, debug_sync)) return e;
        int kept = 0;
        if (int e = fill_read(&kept, kpos + products, 4, stream)) return e;
        if (kept < 0 || kept > products) return hipErrorUnknown;
        if (kept == 0) continue;                                     // (nothing of this level: S stays; a later level may still have pairs)
        const int T = n + kept;
        // ---- 3. S's entries and the kept candidates as triples
        const CooLayout C = coo_layout(rows, rows, T, (int) sizeof(Packed));
        const DupLayout D = dup_layout(T);
        o = 0;
        const uint64_t trow_off = o; o = align256(o + (uint64_t) T * 4);
        const uint64_t tcol_off = o; o = align256(o + (uint64_t) T * 4);
        const uint64_t tpk_off = o; o = align256(o + (uint64_t) T * 8);
        const uint64_t coo_off = o; o = align256(o + coo_temp_bytes(rows, rows, T, (int) sizeof(Packed)));
        const uint64_t soff_off = o; o = align256(o + rbytes);
        const uint64_t scol_off = o; o = align256(o + (uint64_t) T * 4);
        const uint64_t spk_off = o; o = align256(o + (uint64_t) T * 8);
        const uint64_t dup_off = o; o = align256(o + D.total);
        DevBuf work;
        if (!work.alloc(o)) return hipErrorOutOfMemory;
        int *trow = work.as<int>(trow_off), *tcol = work.as<int>(tcol_off);
        Packed *tpk = work.as<Packed>(tpk_off);
        if (int e = fill_copy(trow, erow, (uint64_t) n * 4, stream, debug_sync)) return e;
        if (int e = fill_copy(tcol, s_col.p, (uint64_t) n * 4, stream, debug_sync)) return e;
        if (int e = fill_copy(tpk, s_pk.p, (uint64_t) n * 8, stream, debug_sync)) return e;
        hipLaunchKernelGGL(fill_expand_kernel, dim3(egrid), dim3(FILL_BLOCK), 0, stream, start, erow, s_col.as<int>(), s_pk.as<Packed>(), n, ustart,
                           (int) products, round, kpos, trow + n, tcol + n, tpk + n);
        if (int e = launched(stream, debug_sync, "fill_expand_kernel", egrid)) return e;
        // ---- 4. sorted by (row, column), runs flagged and counted
        int *soff = work.as<int>(soff_off), *scol = work.as<int>(scol_off);
        Packed *spk = work.as<Packed>(spk_off);
        if (int e = coo_run<Packed, true>(work.p + coo_off, C, tpk, trow, tcol, rows, T, soff, scol, spk, nullptr, stream, debug_sync)) return e;
        int *flags = work.as<int>(dup_off + D.flags_off), *pos = work.as<int>(dup_off + D.pos_off);
        const unsigned fgrid = grid_for(T, DUP_CHUNK), cgrid = grid_for(T, FILL_BLOCK);
        hipLaunchKernelGGL(dup_flags_kernel, dim3(fgrid), dim3(256), 0, stream, soff, scol, rows, T, flags);
        if (int e = launched(stream, debug_sync, "dup_flags_kernel", fgrid)) return e;
        if (int e = scan_table(flags, T, work.as<int>(dup_off + D.bsum_off), pos, stream, debug_sync)) return e;
        int count = 0;
        if (int e = fill_read(&count, pos + T, 4, stream)) return e;
        if (count < n || count > T) return hipErrorUnknown;          // (cannot be: every entry of S heads or joins a run)
        // ---- 5. the next S
        DevBuf n_off, n_col, n_pk;
        if (!n_off.alloc(rbytes) || !n_col.alloc((uint64_t) count * 4) || !n_pk.alloc((uint64_t) count * 8)) return hipErrorOutOfMemory;
        hipLaunchKernelGGL(fill_compact_kernel, dim3(cgrid), dim3(FILL_BLOCK), 0, stream, pos, scol, spk, T, n_col.as<int>(), n_pk.as<Packed>());
        if (int e = launched(stream, debug_sync, "fill_compact_kernel", cgrid)) return e;
        hipLaunchKernelGGL(dup_offsets_kernel, dim3(ogrid), dim3(256), 0, stream, soff, pos, rows, n_off.as<int>());
        if (int e = launched(stream, debug_sync, "dup_offsets_kernel", ogrid)) return e;
        if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;      // (before this round's storage goes)
        s_off.swap(n_off); s_col.swap(n_col); s_pk.swap(n_pk);
        n = count;
    }
    // ---- levels and sources; the largest level present
    DevBuf lev, src, present;
    if (!lev.alloc((uint64_t) n * 4) || !src.alloc((uint64_t) n * 4) || !present.alloc((FILL_MAX_LEVEL + 1) * 4)) return hipErrorOutOfMemory;
    int h_present[FILL_MAX_LEVEL + 1] = {0};
    if (n > 0) {
        if (hipMemsetAsync(present.p, 0, sizeof(h_present), stream) != hipSuccess) return hipErrorInvalidValue;
        const unsigned g = grid_for(n, FILL_BLOCK);
        hipLaunchKernelGGL(fill_unpack_kernel, dim3(g), dim3(FILL_BLOCK), 0, stream, s_pk.as<Packed>(), n, lev.as<int>(), src.as<int>(),
                           present.as<int>());
        if (int e = launched(stream, debug_sync, "fill_unpack_kernel", g)) return e;
        if (int e = fill_read(h_present, present.p, sizeof(h_present), stream)) return e;
    } else if (hipStreamSynchronize(stream) != hipSuccess) {
        return hipErrorUnknown;
    }
    for (int l = 0; l <= FILL_MAX_LEVEL; ++l) if (h_present[l]) f.info.max_level = l;
    f.info.nnz_filled = n;
    f.info.device_bytes = rbytes + 3 * (uint64_t) n * 4;
    f.d_off = s_off.release<int32_t>(); f.d_col = s_col.release<int32_t>();
    f.d_lev = lev.release<int32_t>(); f.d_src = src.release<int32_t>();
    return hipSuccess;
}

template <typename V>
int fill_values_impl(const mspmv_csr_fill *f, const V *d_values, V *d_filled, hipStream_t stream, int debug_sync)
{
    if (!f) return hipErrorInvalidValue;
    const int n = f->info.nnz_filled;
    if (n == 0) return hipSuccess;
    if (!d_filled || (f->info.nnz > 0 && !d_values)) return hipErrorInvalidValue;
    const unsigned g = grid_for(n, FILL_BLOCK);
    hipLaunchKernelGGL(fill_values_kernel<V>, dim3(g), dim3(FILL_BLOCK), 0, stream, f->d_src, d_values, d_filled, n);
    return launched(stream, debug_sync, "fill_values_kernel", g);
}

}  // namespace

extern "C" {

int mspmv_csr_fill_create(mspmv_csr_fill_t **fill, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                          int32_t level, mspmv_stream_t stream, int debug_sync)
{
    if (!fill) return hipErrorInvalidValue;
    *fill = nullptr;
    if (rows < 0 || nnz < 0 || rows > FILL_MAX_ROWS || (long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    if (level < 0 || level > FILL_MAX_LEVEL) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || !d_column_indices)) return hipErrorInvalidValue;
    if (rows > 0 && !d_row_offsets) return hipErrorInvalidValue;
    mspmv_csr_fill *f = new (std::nothrow) mspmv_csr_fill;
    if (!f) return hipErrorOutOfMemory;
    f->info.rows = rows; f->info.nnz = nnz; f->info.level = level;
    if (rows > 0) {
        if (int e = fill_analyse(*f, d_row_offsets, d_column_indices, reinterpret_cast<hipStream_t>(stream), debug_sync)) {
            (void) hipGetLastError();
            (void) mspmv_csr_fill_destroy(f);
            return e;
        }
    }
    *fill = f;
    return hipSuccess;
}

int mspmv_csr_fill_info(const mspmv_csr_fill_t *fill, mspmv_csr_fill_info_t *info)
{
    if (!fill || !info) return hipErrorInvalidValue;
    *info = fill->info;
    return hipSuccess;
}

const int32_t *mspmv_csr_fill_row_offsets(const mspmv_csr_fill_t *fill) { return fill ? fill->d_off : nullptr; }
const int32_t *mspmv_csr_fill_column_indices(const mspmv_csr_fill_t *fill) { return fill ? fill->d_col : nullptr; }
const int32_t *mspmv_csr_fill_levels(const mspmv_csr_fill_t *fill) { return fill ? fill->d_lev : nullptr; }
const int32_t *mspmv_csr_fill_source(const mspmv_csr_fill_t *fill) { return fill ? fill->d_src : nullptr; }

int mspmv_csr_fill_values_f32(const mspmv_csr_fill_t *fill, const float *d_values, float *d_values_filled, mspmv_stream_t stream, int debug_sync)
{
    return fill_values_impl<float>(fill, d_values, d_values_filled, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_fill_values_f64(const mspmv_csr_fill_t *fill, const double *d_values, double *d_values_filled, mspmv_stream_t stream,
                              int debug_sync)
{
    return fill_values_impl<double>(fill, d_values, d_values_filled, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_csr_fill_destroy(mspmv_csr_fill_t *fill)
{
    if (!fill) return hipErrorInvalidValue;
    for (int32_t *a : {fill->d_off, fill->d_col, fill->d_lev, fill->d_src})
        if (a) (void) hipFree(a);
    delete fill;
    return hipSuccess;
}

}  // extern "C"
