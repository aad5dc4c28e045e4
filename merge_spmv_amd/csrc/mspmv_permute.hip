// mspmv_permute.hip -- B = A[row_perm, :] with the columns renumbered by col_map, canonical (mspmv_csr_permute_* of include/mspmv.h).
//
// What.  Row i of B holds the entries of A's row row_perm[i], each column c replaced by col_map[c], sorted STABLY by the new column:
// entries that map to one column keep their stored order.  B entry j is A entry permutation[j]; values are moved, never recomputed.
// That is, bit for bit, what mspmv_coo_to_csr_* gives on the triples (inverse_row(r), col_map[c], v) listed in A's stored order -- and
// it is computed that way:
//   1. inv[row_perm[i]] = i                                   (one lane per row; skipped for the identity);
//   2. every entry j of A -> (inv[row of j], col_map[column of j]) in equal tiles of PM_CHUNK entries whatever the row lengths: a tile
//      finds its row range as the transpose's first pass does and every entry its row by a binary search inside it, so that one row of
//      2^20 entries is no single lane's loop;
//   3. the COO build's stable radix sort over (new column digits, then new row digits) (mspmv_coo.hpp: coo_run), which reads the
//      values from A's array in its first pass and writes B's three arrays, the permutation and B's row offsets in its last.
// No atomics on global memory, no workgroup waits on another, the host launches the same kernels whatever the data and reads nothing
// back: the result is a function of the input alone and the call can be captured in a graph.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range, the three scan kernels

#include "mspmv_radix.hpp"     // the pass kernels (upsweep, downsweep), the offsets / fill kernels, Items, launched

#include "mspmv_coo.hpp"       // CooLayout, coo_temp_bytes, coo_run

constexpr int PM_CHUNK = 1024;                          // entries per block of the expansion (one row-range search per block)

__global__ __launch_bounds__(256) void pm_inverse_kernel(const int *__restrict__ perm, int rows, int *__restrict__ inv)
{
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < rows) inv[perm[i]] = (int) i;
}

// entry j of A -> its new row and its new column (inv, col_map: NULL = identity)
__global__ __launch_bounds__(256) void pm_expand_kernel(const int *__restrict__ off, const int *__restrict__ cols, int rows, int nnz,
                                                        const int *__restrict__ inv, const int *__restrict__ col_map,
                                                        int *__restrict__ rows_new, int *__restrict__ cols_new)
{
    __shared__ int s_range[2];
    const long long j0 = (long long) blockIdx.x * PM_CHUNK;
    const int j1 = (int) std::min<long long>(j0 + PM_CHUNK, nnz) - 1;
    block_row_range(off, rows, (int) j0, j1, s_range);
    for (int j = (int) j0 + (int) threadIdx.x; j <= j1; j += 256) {
        const int r = row_of(off, s_range[0], s_range[1], j), c = cols[j];
        rows_new[j] = inv ? inv[r] : r;
        cols_new[j] = col_map ? col_map[c] : c;
    }
}

// temp storage of one call: inv[rows], the new rows and columns of A's entries, and the sort's own temp
struct PmLayout {
    uint64_t inv_off, rows_off, cols_off, sort_off, total;
};
static PmLayout pm_layout(int rows, int cols, int nnz, int value_bytes)
{
    PmLayout P{};
    uint64_t off = 0;
    P.inv_off = off; off = align256(off + (uint64_t) std::max(rows, 1) * 4);
    P.rows_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    P.cols_off = off; off = align256(off + (uint64_t) std::max(nnz, 1) * 4);
    P.sort_off = off; off += align256(coo_temp_bytes(rows, cols, nnz, value_bytes));
    P.total = off;
    return P;
}

template <typename V>
int permute_impl(void *d_temp, size_t *temp_bytes, const V *d_values, const int32_t *d_off, const int32_t *d_cols, int32_t rows, int32_t cols,
                 int32_t nnz, const int32_t *d_row_perm, const int32_t *d_col_map, V *d_values_b, int32_t *d_off_b, int32_t *d_cols_b,
                 int32_t *d_perm, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || nnz < 0) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    const PmLayout P = pm_layout(rows, cols, nnz, (int) sizeof(V));
    if (d_temp == nullptr) { *temp_bytes = (size_t) P.total; return hipSuccess; }
    if (*temp_bytes < P.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!d_off_b) return hipErrorInvalidValue;
    if (nnz > 0 && (!d_off || !d_cols || !d_cols_b || (d_values == nullptr) != (d_values_b == nullptr))) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    const CooLayout L = coo_layout(rows, cols, nnz, (int) sizeof(V));
    int *inv = reinterpret_cast<int *>(base + P.inv_off), *rows_new = reinterpret_cast<int *>(base + P.rows_off);
    int *cols_new = reinterpret_cast<int *>(base + P.cols_off);
    if (nnz > 0) {
        if (d_row_perm) {
            const unsigned g = grid_for(rows, 256);
            hipLaunchKernelGGL(pm_inverse_kernel, dim3(g), dim3(256), 0, stream, d_row_perm, rows, inv);
            if (int e = launched(stream, debug_sync, "pm_inverse_kernel", g)) return e;
        }
        const unsigned g = grid_for(nnz, PM_CHUNK);
        hipLaunchKernelGGL(pm_expand_kernel, dim3(g), dim3(256), 0, stream, d_off, d_cols, rows, nnz, d_row_perm ? inv : nullptr, d_col_map, rows_new,
                           cols_new);
        if (int e = launched(stream, debug_sync, "pm_expand_kernel", g)) return e;
    }
    if (d_values)
        return coo_run<V, true>(base + P.sort_off, L, d_values, rows_new, cols_new, rows, nnz, d_off_b, d_cols_b, d_values_b, d_perm, stream, debug_sync);
    return coo_run<V, false>(base + P.sort_off, L, d_values, rows_new, cols_new, rows, nnz, d_off_b, d_cols_b, d_values_b, d_perm, stream, debug_sync);
}

}  // namespace

extern "C" {

int mspmv_csr_permute_f32(void *d_temp, size_t *temp_bytes, const float *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, const int32_t *d_row_perm,
                          const int32_t *d_col_map, float *d_values_b, int32_t *d_row_offsets_b, int32_t *d_column_indices_b,
                          int32_t *d_permutation, mspmv_stream_t stream, int debug_sync)
{
    return permute_impl<float>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, d_row_perm, d_col_map, d_values_b,
                               d_row_offsets_b, d_column_indices_b, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_permute_f64(void *d_temp, size_t *temp_bytes, const double *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz, const int32_t *d_row_perm,
                          const int32_t *d_col_map, double *d_values_b, int32_t *d_row_offsets_b, int32_t *d_column_indices_b,
                          int32_t *d_permutation, mspmv_stream_t stream, int debug_sync)
{
    return permute_impl<double>(d_temp, temp_bytes, d_values, d_row_offsets, d_column_indices, rows, cols, nnz, d_row_perm, d_col_map, d_values_b,
                                d_row_offsets_b, d_column_indices_b, d_permutation, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
