// mspmv_transpose.hip -- the device CSR transpose of include/mspmv.h (mspmv_csr_transpose_*, mspmv_csr_transpose_values_*) and the
// stateless y = alpha * A^T * x + beta * y built on it (mspmv_csrmv_transpose_*).
//
// What.  A^T as CSR is A's nonzeros sorted STABLY by column: row_offsets_t from the sorted keys, column_indices_t = the original rows,
// values_t the values, permutation = the original positions.  The sort is a least-significant-digit radix sort over the bits of
// cols - 1, D = 8 bits per pass (C2's 3.1 M columns: 22 bits, 3 passes), carrying (key, row, k, value) through every pass as sequential
// traffic.  A pass is three steps, none of which waits on another workgroup:
//   upsweep    per tile of TILE nonzeros, the digit histogram (integer atomics in LDS) -> counts[digit * tiles + tile];
//   scan       exclusive scan of that table (mspmv_scan.hpp) -> where digit d of tile t starts in the pass's output;
//   downsweep  each item's stable rank inside its tile: per wave, rounds of 64 consecutive items; the lanes holding the same digit are
//              the AND of D ballots, the rank is the popcount of those in lower lanes plus the wave's running count of the digit
//              (LDS, item order); then the waves' counts are scanned per digit, the tile is staged in LDS in digit order and written
//              out so that every digit's run is one contiguous store stream.
// The first pass reads the CSR arrays directly (no key-copy pass): a tile finds its row range as plan_count_kernel does and every item
// its row by a binary search inside it.  The last pass writes column_indices_t / values_t / permutation and the sorted keys, from which
// the finishing kernel writes row_offsets_t by boundary detection (entry j writes the offsets of the columns key[j-1]+1 .. key[j]; no
// atomics, empty columns come out right).  nnz == 0 and cols == 1 (A's order is already sorted) go straight to finishing kernels.
//
// Deterministic by construction: every position is a function of the input alone, so the output is the canonical stable transpose.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range, the three scan kernels

#include "mspmv_radix.hpp"     // the pass kernels (upsweep, downsweep), the offsets / fill / gather kernels, Items, launched

struct TrLayout {
    int passes, sets;
    long long tiles, table;                             // tiles of TR_TILE nonzeros; digit x tile entries
    uint64_t counts_off, offs_off, bsum_off, keys_off, set_off[2], total;
};

// temp storage of one transpose: the digit table and its scan, the scan's block sums, the sorted keys, and up to two sets of
// (key, row, k, value) arrays between passes (passes - 1 of them, at most two: the last pass writes the caller's arrays)
static TrLayout tr_layout(int cols, int nnz, int value_bytes)
{
    TrLayout L{};
    L.passes = radix_passes(cols);
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

// cols == 1: A's order is already sorted by column -- column_indices_t = the rows, values_t = the values, permutation = identity
template <typename V, bool VALS>
__global__ __launch_bounds__(256) void tr_identity_kernel(const int *__restrict__ off, const V *__restrict__ vals, int rows, int nnz,
                                                          int *__restrict__ cols_t, V *__restrict__ vals_t, int *__restrict__ perm)
{
    __shared__ int s_range[2];
    const int j0 = blockIdx.x * 1024;
    const int j1 = min(j0 + 1024, nnz) - 1;
    block_row_range(off, rows, j0, j1, s_range);
    for (int j = j0 + (int) threadIdx.x; j <= j1; j += 256) {
        cols_t[j] = row_of(off, s_range[0], s_range[1], j);
        if constexpr (VALS) vals_t[j] = vals[j];
        if (perm) perm[j] = j;
    }
}

template <typename V, bool VALS>
int transpose_run(char *base, const TrLayout &L, const V *d_values, const int32_t *d_off, const int32_t *d_cols, int32_t rows,
                  int32_t cols, int32_t nnz, V *d_values_t, int32_t *d_off_t, int32_t *d_cols_t, int32_t *d_perm, hipStream_t stream,
                  int debug_sync)
{
    if (nnz == 0) {
        hipLaunchKernelGGL(tr_fill_kernel, dim3(grid_for((long long) cols + 1, 256)), dim3(256), 0, stream, d_off_t, (long long) cols + 1, 0);
        return launched(stream, debug_sync, "tr_fill_kernel", grid_for((long long) cols + 1, 256));
    }
    const unsigned ogrid = grid_for((long long) nnz + 1, 256);
    if (cols == 1) {
        const unsigned g = grid_for(nnz, 1024);
        hipLaunchKernelGGL((tr_identity_kernel<V, VALS>), dim3(g), dim3(256), 0, stream, d_off, d_values, rows, nnz, d_cols_t, d_values_t, d_perm);
        if (int e = launched(stream, debug_sync, "tr_identity_kernel", g)) return e;
        hipLaunchKernelGGL(tr_offsets_kernel, dim3(ogrid), dim3(256), 0, stream, d_cols, nnz, cols, d_off_t);
        return launched(stream, debug_sync, "tr_offsets_kernel", ogrid);
    }
    int *counts = reinterpret_cast<int *>(base + L.counts_off);
    int *offs = reinterpret_cast<int *>(base + L.offs_off);
    int *bsum = reinterpret_cast<int *>(base + L.bsum_off);
    int *keys = reinterpret_cast<int *>(base + L.keys_off);
    Items<V> set[2] = {items_at<V>(base, L.set_off[0], nnz), items_at<V>(base, L.set_off[1], nnz)};
    const unsigned tgrid = (unsigned) L.tiles;
    for (int p = 0; p < L.passes; ++p) {
        const int shift = p * TR_BITS;
        const bool last = p == L.passes - 1;
        const Items<V> &src = set[(p + 1) & 1];          // pass p reads what pass p - 1 wrote (set (p - 1) % 2)
        hipLaunchKernelGGL(tr_upsweep_kernel, dim3(tgrid), dim3(TR_BLOCK), 0, stream, p == 0 ? d_cols : src.key, nnz, shift, L.tiles, counts);
        if (int e = launched(stream, debug_sync, "tr_upsweep_kernel", tgrid)) return e;
        if (int e = scan_table(counts, L.table, bsum, offs, stream, debug_sync)) return e;
        int *ok = last ? keys : set[p & 1].key, *orow = last ? d_cols_t : set[p & 1].row, *okk = last ? d_perm : set[p & 1].k;
        V *oval = last ? d_values_t : set[p & 1].val;
        if (p == 0)
            hipLaunchKernelGGL((tr_downsweep_kernel<V, SRC_CSR, VALS>), dim3(tgrid), dim3(TR_BLOCK), 0, stream, d_off, d_cols, d_values, rows, src,
                               nnz, shift, L.tiles, offs, ok, orow, okk, oval);
        else
            hipLaunchKernelGGL((tr_downsweep_kernel<V, SRC_ITEMS, VALS>), dim3(tgrid), dim3(TR_BLOCK), 0, stream, d_off, d_cols, d_values, rows,
                               src, nnz, shift, L.tiles, offs, ok, orow, okk, oval);
        if (int e = launched(stream, debug_sync, "tr_downsweep_kernel", tgrid)) return e;
    }
    hipLaunchKernelGGL(tr_offsets_kernel, dim3(ogrid), dim3(256), 0, stream, keys, nnz, cols, d_off_t);
    return launched(stream, debug_sync, "tr_offsets_kernel", ogrid);
}

// bytes of temp storage a transpose of these sizes needs (the same for both precisions' structure-only mode)
static uint64_t transpose_temp_bytes(int32_t cols, int32_t nnz, int value_bytes)
{
    return std::max<uint64_t>(tr_layout(cols, nnz, value_bytes).total, 256);
}

template <typename V>
int transpose_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_off, const int32_t *d_cols, int32_t rows,
                   int32_t cols, int32_t nnz, V *d_values_t, int32_t *d_off_t, int32_t *d_cols_t, int32_t *d_perm, hipStream_t stream,
                   int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    const TrLayout L = tr_layout(cols, nnz, (int) sizeof(V));
    const uint64_t need = transpose_temp_bytes(cols, nnz, (int) sizeof(V));
    if (d_temp == nullptr) { *temp_bytes = (size_t) need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!d_off_t) return hipErrorInvalidValue;
    if (nnz > 0 && (!d_off || !d_cols || !d_cols_t || (d_values == nullptr) != (d_values_t == nullptr))) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    if (d_values) return transpose_run<V, true>(base, L, d_values, d_off, d_cols, rows, cols, nnz, d_values_t, d_off_t, d_cols_t, d_perm, stream, debug_sync);
    return transpose_run<V, false>(base, L, d_values, d_off, d_cols, rows, cols, nnz, d_values_t, d_off_t, d_cols_t, d_perm, stream, debug_sync);
}

template <typename V>
int transpose_values_impl(const V *d_values, const int32_t *d_perm, V *d_values_t, int32_t nnz, hipStream_t stream, int debug_sync)
{
    if (nnz < 0 || (nnz > 0 && (!d_values || !d_perm || !d_values_t))) return hipErrorInvalidValue;
    if (nnz == 0) return hipSuccess;
    const unsigned g = grid_for(nnz, 256);
    hipLaunchKernelGGL((tr_values_kernel<V>), dim3(g), dim3(256), 0, stream, d_values, d_perm, d_values_t, nnz);
    return launched(stream, debug_sync, "tr_values_kernel", g);
}

// the stateless A^T x: temp = [the transpose's temp | values_t | row_offsets_t | column_indices_t | the forward call's temp]
struct TmvLayout {
    uint64_t tr_bytes, vals_off, off_off, cols_off, inner_off, inner_bytes, total;
};

template <typename V>
int csrmv_transpose_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_off, const int32_t *d_cols, const V *d_x,
                         V *d_y, int32_t rows, int32_t cols, int32_t nnz, V alpha, V beta, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) cols + nnz > MAX_ITEMS) return hipErrorInvalidValue;           // A^T's rows + nnz: the forward call's bound
    TmvLayout T{};
    T.tr_bytes = transpose_temp_bytes(cols, nnz, (int) sizeof(V));
    uint64_t off = align256(T.tr_bytes);
    T.vals_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * sizeof(V));
    T.off_off = off; off = align256(off + ((uint64_t) cols + 1) * 4);
    T.cols_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    T.inner_off = off;
    size_t inner = 0;
    const int q = sizeof(V) == 4 ? mspmv_csrmv_axpby_f32(nullptr, &inner, nullptr, nullptr, nullptr, nullptr, nullptr, cols, rows, nnz, 1.0f, 0.0f,
                                                         nullptr, 0)
                                 : mspmv_csrmv_axpby_f64(nullptr, &inner, nullptr, nullptr, nullptr, nullptr, nullptr, cols, rows, nnz, 1.0, 0.0,
                                                         nullptr, 0);
    if (q != 0) return q;
    T.inner_bytes = inner;
    T.total = off + inner;
    if (d_temp == nullptr) { *temp_bytes = (size_t) T.total; return hipSuccess; }
    if (*temp_bytes < T.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (cols == 0) return hipSuccess;                   // y has no entries
    if (!d_y || (nnz > 0 && (!d_values || !d_off || !d_cols || !d_x))) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    V *vals_t = reinterpret_cast<V *>(base + T.vals_off);
    int32_t *off_t = reinterpret_cast<int32_t *>(base + T.off_off), *cols_t = reinterpret_cast<int32_t *>(base + T.cols_off);
    size_t tb = (size_t) T.tr_bytes;
    if (int e = transpose_impl<V>(d_temp, &tb, d_values, d_off, d_cols, rows, cols, nnz, nnz > 0 ? vals_t : nullptr, off_t, cols_t, nullptr,
                                  stream, debug_sync))
        return e;
    size_t ib = (size_t) T.inner_bytes;
    if constexpr (sizeof(V) == 4)
        return mspmv_csrmv_axpby_f32(base + T.inner_off, &ib, vals_t, off_t, cols_t, d_x, d_y, cols, rows, nnz, alpha, beta, stream, debug_sync);
    else
        return mspmv_csrmv_axpby_f64(base + T.inner_off, &ib, vals_t, off_t, cols_t, d_x, d_y, cols, rows, nnz, alpha, beta, stream, debug_sync);
}

}  // namespace

extern "C" {

int mspmv_csr_transpose_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_offsets,
                            const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, float *d_values_t,
                            int32_t *d_row_offsets_t, int32_t *d_column_indices_t, int32_t *d_permutation, mspmv_stream_t stream,
                            int debug_sync)
{
    return transpose_impl<float>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, d_values_t, d_row_offsets_t,
                                 d_column_indices_t, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_transpose_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_offsets,
                            const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, double *d_values_t,
                            int32_t *d_row_offsets_t, int32_t *d_column_indices_t, int32_t *d_permutation, mspmv_stream_t stream,
                            int debug_sync)
{
    return transpose_impl<double>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, d_values_t, d_row_offsets_t,
                                  d_column_indices_t, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_transpose_values_f32(const float *d_values, const int32_t *d_permutation, float *d_values_t, int32_t nnz, mspmv_stream_t stream,
                                   int debug_sync)
{
    return transpose_values_impl<float>(d_values, d_permutation, d_values_t, nnz, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_transpose_values_f64(const double *d_values, const int32_t *d_permutation, double *d_values_t, int32_t nnz,
                                   mspmv_stream_t stream, int debug_sync)
{
    return transpose_values_impl<double>(d_values, d_permutation, d_values_t, nnz, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csrmv_transpose_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_offsets,
                              const int32_t *d_column_indices, const float *d_x, float *d_y, int32_t rows, int32_t cols, int32_t nnz,
                              float alpha, float beta, mspmv_stream_t stream, int debug_sync)
{
    return csrmv_transpose_impl<float>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, d_x, d_y, rows, cols, nnz, alpha, beta,
                                       reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csrmv_transpose_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_offsets,
                              const int32_t *d_column_indices, const double *d_x, double *d_y, int32_t rows, int32_t cols, int32_t nnz,
                              double alpha, double beta, mspmv_stream_t stream, int debug_sync)
{
    return csrmv_transpose_impl<double>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, d_x, d_y, rows, cols, nnz, alpha, beta,
                                        reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
