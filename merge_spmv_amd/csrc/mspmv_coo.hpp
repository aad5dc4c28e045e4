// mspmv_coo.hpp -- the two passes that mspmv_coo.hip (CSR from COO triples, duplicate merging) and mspmv_gemm.hip (the sparse product:
// expanded triples sorted, then runs of equal (row, column) added) share: coo_run, the stable radix sort of triples by (row, column)
// into CSR arrays with its temp layout, and sum_duplicates_impl, the merging of runs of equal (row, column) of a sorted CSR.  What
// they do and why is told in mspmv_coo.hip.  Included inside an anonymous namespace of each translation unit, after mspmv_scan.hpp and
// mspmv_radix.hpp.
#pragma once
#include <hip/hip_runtime.h>

struct CooLayout {
    int col_passes, row_passes, passes, sets;
    long long tiles, table;                             // tiles of TR_TILE entries; digit x tile entries
    uint64_t counts_off, offs_off, bsum_off, keys_off, set_off[2], total;
};

// temp storage of one build: the digit table and its scan, the scan's block sums, the sorted rows, and up to two sets of
// (column, row, position, value) arrays between passes (passes - 1 of them, at most two: the last pass writes the caller's arrays)
static CooLayout coo_layout(int rows, int cols, int nnz, int value_bytes)
{
    CooLayout L{};
    L.col_passes = cols > 1 ? radix_passes(cols) : 0;
    L.row_passes = rows > 1 ? radix_passes(rows) : 0;
    if (L.col_passes + L.row_passes == 0) L.row_passes = 1;
    L.passes = L.col_passes + L.row_passes;
    L.sets = std::min(L.passes - 1, 2);
    L.tiles = ((long long) nnz + TR_TILE - 1) / TR_TILE;
    L.table = L.tiles * TR_DIGITS;
    uint64_t off = 0;
    L.counts_off = off; off = align256(off + (uint64_t) std::max(L.table, 1LL) * 4);
    L.offs_off = off; off = align256(off + (uint64_t) (L.table + 1) * 4);
    L.bsum_off = off; off = align256(off + (uint64_t) ((L.table + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
    L.keys_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    for (int s = 0; s < 2; ++s) {
        L.set_off[s] = off;
        if (s < L.sets) off += set_bytes(nnz, value_bytes);
    }
    L.total = off;
    return L;
}

static uint64_t coo_temp_bytes(int rows, int cols, int nnz, int value_bytes)
{
    return std::max<uint64_t>(coo_layout(rows, cols, nnz, value_bytes).total, 256);
}

template <typename V, bool VALS>
int coo_run(char *base, const CooLayout &L, const V *d_values, const int32_t *d_rows, const int32_t *d_cols, int32_t rows, int32_t nnz,
            int32_t *d_off, int32_t *d_cols_csr, V *d_values_csr, int32_t *d_perm, hipStream_t stream, int debug_sync)
{
    if (nnz == 0) {
        const unsigned g = grid_for((long long) rows + 1, 256);
        hipLaunchKernelGGL(tr_fill_kernel, dim3(g), dim3(256), 0, stream, d_off, (long long) rows + 1, 0);
        return launched(stream, debug_sync, "tr_fill_kernel", g);
    }
    int *counts = reinterpret_cast<int *>(base + L.counts_off);
    int *offs = reinterpret_cast<int *>(base + L.offs_off);
    int *bsum = reinterpret_cast<int *>(base + L.bsum_off);
    int *keys = reinterpret_cast<int *>(base + L.keys_off);            // the sorted rows (the last pass writes them)
    // in a set, .key holds the columns and .row the rows, whichever of them a pass sorts by
    const Items<V> set[2] = {items_at<V>(base, L.set_off[0], nnz), items_at<V>(base, L.set_off[1], nnz)};
    const Items<V> coo = {const_cast<int *>(d_cols), const_cast<int *>(d_rows), nullptr, nullptr};      // (only read)
    const Items<V> csr = {d_cols_csr, keys, d_perm, d_values_csr};
    const unsigned tgrid = (unsigned) L.tiles;
    for (int p = 0; p < L.passes; ++p) {
        const bool by_col = p < L.col_passes, last = p == L.passes - 1;
        const int shift = (by_col ? p : p - L.col_passes) * TR_BITS;
        const Items<V> &s = p == 0 ? coo : set[(p + 1) & 1];           // pass p reads what pass p - 1 wrote (set (p - 1) % 2)
        const Items<V> &d = last ? csr : set[p & 1];
        const Items<V> in = {by_col ? s.key : s.row, by_col ? s.row : s.key, s.k, s.val};      // key first, the other index second
        hipLaunchKernelGGL(tr_upsweep_kernel, dim3(tgrid), dim3(TR_BLOCK), 0, stream, in.key, nnz, shift, L.tiles, counts);
        if (int e = launched(stream, debug_sync, "tr_upsweep_kernel", tgrid)) return e;
        if (int e = scan_table(counts, L.table, bsum, offs, stream, debug_sync)) return e;
        int *ok = by_col ? d.key : d.row, *oo = by_col ? d.row : d.key;
        if (p == 0)
            hipLaunchKernelGGL((tr_downsweep_kernel<V, SRC_COO, VALS>), dim3(tgrid), dim3(TR_BLOCK), 0, stream, nullptr, nullptr, d_values, rows, in,
                               nnz, shift, L.tiles, offs, ok, oo, d.k, d.val);
        else
            hipLaunchKernelGGL((tr_downsweep_kernel<V, SRC_ITEMS, VALS>), dim3(tgrid), dim3(TR_BLOCK), 0, stream, nullptr, nullptr, d_values, rows,
                               in, nnz, shift, L.tiles, offs, ok, oo, d.k, d.val);
        if (int e = launched(stream, debug_sync, "tr_downsweep_kernel", tgrid)) return e;
    }
    const unsigned ogrid = grid_for((long long) nnz + 1, 256);
    hipLaunchKernelGGL(tr_offsets_kernel, dim3(ogrid), dim3(256), 0, stream, keys, nnz, rows, d_off);
    return launched(stream, debug_sync, "tr_offsets_kernel", ogrid);
}

// ---- duplicates ------------------------------------------------------------------------------------------------------------
constexpr int DUP_CHUNK = 1024;                          // entries per block of the flag kernel (one row-range search per block)

// flag[j] = 1 when entry j starts a run of equal (row, column): the first entry of its row, or another column than entry j - 1
__global__ __launch_bounds__(256) void dup_flags_kernel(const int *__restrict__ off, const int *__restrict__ cols, int rows, int nnz,
                                                        int *__restrict__ flags)
{
    __shared__ int s_range[2];
    const long long j0 = (long long) blockIdx.x * DUP_CHUNK;
    const int j1 = (int) std::min<long long>(j0 + DUP_CHUNK, nnz) - 1;
    block_row_range(off, rows, (int) j0, j1, s_range);
    for (int j = (int) j0 + (int) threadIdx.x; j <= j1; j += 256) {
        const int r = row_of(off, s_range[0], s_range[1], j);
        const int left = j > 0 ? cols[j - 1] : -1;
        flags[j] = (off[r] == j || cols[j] != left) ? 1 : 0;
    }
}

// pos = the exclusive scan of the flags (pos[nnz] = the number of runs).  The head of a run writes the merged entry at pos[j]:
// its column and the run's values added left to right.  Thread 0 of the grid writes the count.  The output arrays hold `capacity`
// entries: a count above it leaves them untouched (the count still tells how much room is needed).
template <typename V, bool VALS>
__global__ __launch_bounds__(256) void dup_compact_kernel(const int *__restrict__ pos, const int *__restrict__ cols, const V *__restrict__ vals,
                                                          int nnz, int capacity, int *__restrict__ cols_out,
                                                          V *__restrict__ vals_out, int *__restrict__ nnz_out)
{
    const long long j = (long long) blockIdx.x * 256 + threadIdx.x;
    const int count = pos[nnz];
    if (j == 0) *nnz_out = count;
    if (j >= nnz || count > capacity) return;
    const int p = pos[j];
    if (pos[j + 1] == p) return;                         // not a head
    cols_out[p] = cols[j];
    if constexpr (VALS) {
        V s = vals[j];
        for (long long q = j + 1; q < nnz && pos[q + 1] == pos[q]; ++q) s += vals[q];
        vals_out[p] = s;
    }
}

// row_offsets_out[r] = the number of runs that start before row r's first entry
__global__ __launch_bounds__(256) void dup_offsets_kernel(const int *__restrict__ off, const int *__restrict__ pos, int rows,
                                                          int *__restrict__ off_out)
{
    const long long r = (long long) blockIdx.x * 256 + threadIdx.x;
    if (r <= rows) off_out[r] = pos[off[r]];
}

__global__ void dup_empty_kernel(int *__restrict__ nnz_out) { *nnz_out = 0; }

struct DupLayout {
    uint64_t flags_off, pos_off, bsum_off, total;
};
static DupLayout dup_layout(int nnz)
{
    DupLayout D{};
    uint64_t off = 0;
    D.flags_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    D.pos_off = off; off = align256(off + ((uint64_t) nnz + 1) * 4);
    D.bsum_off = off; off = align256(off + (uint64_t) (((long long) nnz + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
    D.total = off;
    return D;
}

template <typename V>
int sum_duplicates_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_off, const int32_t *d_cols, int32_t rows,
                        int32_t cols, int32_t nnz, int32_t capacity, V *d_values_out, int32_t *d_off_out, int32_t *d_cols_out,
                        int32_t *d_nnz_out, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0 || capacity < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    const DupLayout D = dup_layout(nnz);
    if (d_temp == nullptr) { *temp_bytes = (size_t) D.total; return hipSuccess; }
    if (*temp_bytes < D.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!d_off_out || !d_nnz_out) return hipErrorInvalidValue;
    // (output arrays of no capacity have no say: nothing is written to them)
    if (nnz > 0 && (!d_off || !d_cols)) return hipErrorInvalidValue;
    if (nnz > 0 && capacity > 0 && (!d_cols_out || (d_values == nullptr) != (d_values_out == nullptr))) return hipErrorInvalidValue;
    if (nnz == 0) {
        const unsigned g = grid_for((long long) rows + 1, 256);
        hipLaunchKernelGGL(tr_fill_kernel, dim3(g), dim3(256), 0, stream, d_off_out, (long long) rows + 1, 0);
        if (int e = launched(stream, debug_sync, "tr_fill_kernel", g)) return e;
        hipLaunchKernelGGL(dup_empty_kernel, dim3(1), dim3(1), 0, stream, d_nnz_out);
        return launched(stream, debug_sync, "dup_empty_kernel", 1);
    }
    char *base = static_cast<char *>(d_temp);
    int *flags = reinterpret_cast<int *>(base + D.flags_off), *pos = reinterpret_cast<int *>(base + D.pos_off);
    int *bsum = reinterpret_cast<int *>(base + D.bsum_off);
    const unsigned fgrid = grid_for(nnz, DUP_CHUNK), cgrid = grid_for(nnz, 256), ogrid = grid_for((long long) rows + 1, 256);
    hipLaunchKernelGGL(dup_flags_kernel, dim3(fgrid), dim3(256), 0, stream, d_off, d_cols, rows, nnz, flags);
    if (int e = launched(stream, debug_sync, "dup_flags_kernel", fgrid)) return e;
    if (int e = scan_table(flags, nnz, bsum, pos, stream, debug_sync)) return e;
    if (d_values && d_values_out)
        hipLaunchKernelGGL((dup_compact_kernel<V, true>), dim3(cgrid), dim3(256), 0, stream, pos, d_cols, d_values, nnz, capacity, d_cols_out,
                           d_values_out, d_nnz_out);
    else
        hipLaunchKernelGGL((dup_compact_kernel<V, false>), dim3(cgrid), dim3(256), 0, stream, pos, d_cols, d_values, nnz, capacity, d_cols_out,
                           d_values_out, d_nnz_out);
    if (int e = launched(stream, debug_sync, "dup_compact_kernel", cgrid)) return e;
    hipLaunchKernelGGL(dup_offsets_kernel, dim3(ogrid), dim3(256), 0, stream, d_off, pos, rows, d_off_out);
    return launched(stream, debug_sync, "dup_offsets_kernel", ogrid);
}
