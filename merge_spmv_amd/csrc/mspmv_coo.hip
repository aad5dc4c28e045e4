// mspmv_coo.hip -- CSR built on the device from unsorted COO triples (mspmv_coo_to_csr_*, mspmv_coo_to_csr_values_*), the merging of
// duplicate entries of a sorted CSR (mspmv_csr_sum_duplicates_*) and the stateless y = alpha * A * x + beta * y from COO
// (mspmv_coomv_*) of include/mspmv.h.  The sort (coo_run) and the duplicate pass (sum_duplicates_impl) live in mspmv_coo.hpp, which
// the sparse product (mspmv_gemm.hip) includes too.
//
// What.  The CSR of a COO matrix is its entries sorted STABLY by (row, column), duplicates kept: the reference's CsrMatrix(coo).  The
// sort is the transpose's least-significant-digit radix sort (mspmv_radix.hpp) over a two-part key: first the 8-bit digits of the
// column index (ceil(bits(cols - 1) / 8) passes, none for one column), then those of the row index (likewise; none for one row --
// a 1 x 1 matrix still runs one pass, which copies).  C2's 3.1 M x 3.1 M: 3 + 3 passes.  An item is (column, row, input position,
// value); a column pass sorts by the first and carries the second, a row pass the other way round, which is a swap of pointers on
// the host.  The first pass reads the caller's COO arrays (the position is the item's index), the last writes the caller's CSR arrays
// and the sorted rows, from which tr_offsets_kernel writes row_offsets by boundary detection.  The host launches the same kernels
// whatever the data and never reads device memory, so a call can be captured in a graph.
//
// Duplicates.  In the built CSR equal (row, column) entries are neighbours in input order.  mspmv_csr_sum_duplicates_* flags the
// head of every run (the first entry of a row, or a column that differs from its left neighbour's), scans the flags (mspmv_scan.hpp)
// and lets the thread of each head add its run left to right and write the merged entry at the scan's position; the new offset of a
// row is the scan's value at its old offset.  No atomics on global memory anywhere in this file; every output position and every
// value is a function of the input alone.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range, the three scan kernels

#include "mspmv_radix.hpp"     // the pass kernels (upsweep, downsweep), the offsets / fill / gather kernels, Items, launched

#include "mspmv_coo.hpp"       // CooLayout, coo_temp_bytes, coo_run; the duplicate kernels, sum_duplicates_impl

template <typename V>
int coo_to_csr_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_rows, const int32_t *d_cols, int32_t rows,
                    int32_t cols, int32_t nnz, int32_t *d_off, int32_t *d_cols_csr, V *d_values_csr, int32_t *d_perm, hipStream_t stream,
                    int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;             // what this builds can be multiplied
    const CooLayout L = coo_layout(rows, cols, nnz, (int) sizeof(V));
    const uint64_t need = coo_temp_bytes(rows, cols, nnz, (int) sizeof(V));
    if (d_temp == nullptr) { *temp_bytes = (size_t) need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!d_off) return hipErrorInvalidValue;
    if (nnz > 0 && (!d_rows || !d_cols || !d_cols_csr || (d_values == nullptr) != (d_values_csr == nullptr))) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    if (d_values) return coo_run<V, true>(base, L, d_values, d_rows, d_cols, rows, nnz, d_off, d_cols_csr, d_values_csr, d_perm, stream, debug_sync);
    return coo_run<V, false>(base, L, d_values, d_rows, d_cols, rows, nnz, d_off, d_cols_csr, d_values_csr, d_perm, stream, debug_sync);
}

template <typename V>
int coo_values_impl(const V *d_values, const int32_t *d_perm, V *d_values_csr, int32_t nnz, hipStream_t stream, int debug_sync)
{
    if (nnz < 0 || (nnz > 0 && (!d_values || !d_perm || !d_values_csr))) return hipErrorInvalidValue;
    if (nnz == 0) return hipSuccess;
    const unsigned g = grid_for(nnz, 256);
    hipLaunchKernelGGL((tr_values_kernel<V>), dim3(g), dim3(256), 0, stream, d_values, d_perm, d_values_csr, nnz);
    return launched(stream, debug_sync, "tr_values_kernel", g);
}

// ---- the stateless A x from COO: temp = [the build's temp | values | row_offsets | column_indices | the forward call's temp] ------
template <typename V>
int coomv_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_rows, const int32_t *d_cols, const V *d_x, V *d_y,
               int32_t rows, int32_t cols, int32_t nnz, V alpha, V beta, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    const uint64_t build_bytes = coo_temp_bytes(rows, cols, nnz, (int) sizeof(V));
    uint64_t off = align256(build_bytes);
    const uint64_t vals_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * sizeof(V));
    const uint64_t off_off = off; off = align256(off + ((uint64_t) rows + 1) * 4);
    const uint64_t cols_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    const uint64_t inner_off = off;
    size_t inner = 0;
    const int q = sizeof(V) == 4 ? mspmv_csrmv_axpby_f32(nullptr, &inner, nullptr, nullptr, nullptr, nullptr, nullptr, rows, cols, nnz, 1.0f, 0.0f,
                                                         nullptr, 0)
                                 : mspmv_csrmv_axpby_f64(nullptr, &inner, nullptr, nullptr, nullptr, nullptr, nullptr, rows, cols, nnz, 1.0, 0.0,
                                                         nullptr, 0);
    if (q != 0) return q;
    const uint64_t total = off + inner;
    if (d_temp == nullptr) { *temp_bytes = (size_t) total; return hipSuccess; }
    if (*temp_bytes < total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;                   // y has no entries
    if (!d_y || (nnz > 0 && (!d_values || !d_rows || !d_cols || !d_x))) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    V *vals = reinterpret_cast<V *>(base + vals_off);
    int32_t *roff = reinterpret_cast<int32_t *>(base + off_off), *ccols = reinterpret_cast<int32_t *>(base + cols_off);
    size_t bb = (size_t) build_bytes;
    if (int e = coo_to_csr_impl<V>(d_temp, &bb, d_values, d_rows, d_cols, rows, cols, nnz, roff, ccols, nnz > 0 ? vals : nullptr, nullptr, stream,
                                   debug_sync))
        return e;
    size_t ib = inner;
    if constexpr (sizeof(V) == 4)
        return mspmv_csrmv_axpby_f32(base + inner_off, &ib, vals, roff, ccols, d_x, d_y, rows, cols, nnz, alpha, beta, stream, debug_sync);
    else
        return mspmv_csrmv_axpby_f64(base + inner_off, &ib, vals, roff, ccols, d_x, d_y, rows, cols, nnz, alpha, beta, stream, debug_sync);
}

}  // namespace

extern "C" {

int mspmv_coo_to_csr_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_indices,
                         const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, int32_t *d_row_offsets,
                         int32_t *d_column_indices_csr, float *d_values_csr, int32_t *d_permutation, mspmv_stream_t stream, int debug_sync)
{
    return coo_to_csr_impl<float>(d_temp, temp_bytes, d_values, d_row_indices, d_column_indices, rows, cols, nnz, d_row_offsets,
                                  d_column_indices_csr, d_values_csr, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_coo_to_csr_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_indices,
                         const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, int32_t *d_row_offsets,
                         int32_t *d_column_indices_csr, double *d_values_csr, int32_t *d_permutation, mspmv_stream_t stream, int debug_sync)
{
    return coo_to_csr_impl<double>(d_temp, temp_bytes, d_values, d_row_indices, d_column_indices, rows, cols, nnz, d_row_offsets,
                                   d_column_indices_csr, d_values_csr, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_coo_to_csr_values_f32(const float *d_values, const int32_t *d_permutation, float *d_values_csr, int32_t nnz, mspmv_stream_t stream,
                                int debug_sync)
{
    return coo_values_impl<float>(d_values, d_permutation, d_values_csr, nnz, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_coo_to_csr_values_f64(const double *d_values, const int32_t *d_permutation, double *d_values_csr, int32_t nnz, mspmv_stream_t stream,
                                int debug_sync)
{
    return coo_values_impl<double>(d_values, d_permutation, d_values_csr, nnz, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_sum_duplicates_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_offsets,
                                 const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, float *d_values_out,
                                 int32_t *d_row_offsets_out, int32_t *d_column_indices_out, int32_t *d_nnz_out, mspmv_stream_t stream,
                                 int debug_sync)
{
    return sum_duplicates_impl<float>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, nnz, d_values_out,
                                      d_row_offsets_out, d_column_indices_out, d_nnz_out, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_sum_duplicates_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_offsets,
                                 const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, double *d_values_out,
                                 int32_t *d_row_offsets_out, int32_t *d_column_indices_out, int32_t *d_nnz_out, mspmv_stream_t stream,
                                 int debug_sync)
{
    return sum_duplicates_impl<double>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, nnz, d_values_out,
                                       d_row_offsets_out, d_column_indices_out, d_nnz_out, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_coomv_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_indices, const int32_t *d_column_indices,
                    const float *d_x, float *d_y, int32_t rows, int32_t cols, int32_t nnz, float alpha, float beta, mspmv_stream_t stream,
                    int debug_sync)
{
    return coomv_impl<float>(d_temp, temp_bytes, d_values, d_row_indices, d_column_indices, d_x, d_y, rows, cols, nnz, alpha, beta,
                             reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_coomv_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_indices, const int32_t *d_column_indices,
                    const double *d_x, double *d_y, int32_t rows, int32_t cols, int32_t nnz, double alpha, double beta, mspmv_stream_t stream,
                    int debug_sync)
{
    return coomv_impl<double>(d_temp, temp_bytes, d_values, d_row_indices, d_column_indices, d_x, d_y, rows, cols, nnz, alpha, beta,
                              reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
