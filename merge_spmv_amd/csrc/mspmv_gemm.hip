// mspmv_gemm.hip -- C = A * B for two CSR matrices on the device (mspmv_csr_gemm_products, mspmv_csr_gemm_* of include/mspmv.h).
//
// What.  Expand - sort - compress.  Every pair (a_ik, b_kj) becomes a triple (i, j, a * b); the triples are sorted STABLY by
// (row, column) (coo_run, mspmv_coo.hpp) and every run of equal (i, j) is added left to right (sum_duplicates_impl).  The triples
// are expanded in the order of A's entries and, under one entry of A, in the order of B's row, and the sort is stable: the order in
// which the products of one entry of C are added is a function of the two inputs alone, and C is defined bit for bit.
//   lengths  one thread per entry e of A: len[e] = the length of B's row column_indices_a[e]; per block the 64-bit sum of them;
//   scan     start[e] = len[0] + ... + len[e - 1] (mspmv_scan.hpp, int32);
//   total    one block adds the per-block sums in 64 bits and compares the total with the caller's `products`: the verdict.  The
//            64-bit total cannot wrap, so a count of 2^32 + products is told from products, which start[nnz_a] alone could not;
//   expand   the list of products is cut into tiles of GEMM_TILE whatever the row lengths -- one entry of A that hits a row of B
//            with a million entries costs what a million short rows cost.  A tile finds the entries of A of its first and last
//            product by a search of start (the LAST entry that starts at or before the product: entries whose B row is empty are
//            skipped by the search, not walked), stages start, the row, the offset into B and A's value of its entries in LDS, and
//            every thread finds the entry of its products by a search there.  Consecutive lanes take consecutive products: the
//            stores, and the loads of B under one entry of A, are consecutive.  A tile whose slice of A is longer than GEMM_TILE
//            (long stretches of empty B rows inside it) searches in global memory instead.  When the verdict is "wrong", the tiles
//            write (0, 0, 0) and read neither matrix: whatever `products` says, every index is in range;
//   sort, compress, and a last thread that overwrites *d_nnz_c with -1 when the verdict is "wrong".
// No atomics on global memory, no workgroup waits on another, the host sizes every launch from its arguments and never reads device
// memory: the call launches the same kernels whatever the data and can be captured in a graph.
//
// Values.  a * b rounded on its own, then the sums: contraction into fused multiply-adds is switched off for this file, as in
// mspmv_add.hip.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range, the three scan kernels

#include "mspmv_radix.hpp"     // launched, scan_table, tr_fill_kernel, TR_TILE

#include "mspmv_coo.hpp"       // coo_layout, coo_temp_bytes, coo_run, dup_layout, sum_duplicates_impl

constexpr int GEMM_BLOCK = 256, GEMM_IPT = 8, GEMM_TILE = GEMM_BLOCK * GEMM_IPT;      // 2048 products, the radix tile
static_assert(GEMM_TILE == TR_TILE, "an expansion tile is a tile of the sort");

struct GemmVerdict { long long total; int ok, pad; };

// ---- lengths: len[e] = the length of B's row cola[e] (LEN), and the block's 64-bit sum of them -------------------------------
template <bool LEN>
__global__ __launch_bounds__(GEMM_BLOCK) void gemm_lengths_kernel(const int *__restrict__ cola, int nnz_a, const int *__restrict__ offb,
                                                                  int *__restrict__ len, long long *__restrict__ partial)
{
    __shared__ long long s_sum[GEMM_BLOCK];
    const long long base = (long long) blockIdx.x * GEMM_TILE;
    long long t = 0;
    for (int i = 0; i < GEMM_IPT; ++i) {
        const long long e = base + i * GEMM_BLOCK + threadIdx.x;
        if (e < nnz_a) {
            const int c = cola[e];
            const int l = offb[c + 1] - offb[c];
            if constexpr (LEN) len[e] = l;
            t += l;
        }
    }
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int d = GEMM_BLOCK / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}

// one block adds the per-block sums; with a verdict to write, compares the total with what the caller stated
__global__ __launch_bounds__(GEMM_BLOCK) void gemm_total_kernel(const long long *__restrict__ partial, long long blocks, long long stated,
                                                                long long *__restrict__ total_out, GemmVerdict *__restrict__ verdict)
{
    __shared__ long long s_sum[GEMM_BLOCK];
    long long t = 0;
    for (long long i = threadIdx.x; i < blocks; i += GEMM_BLOCK) t += partial[i];
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int d = GEMM_BLOCK / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (total_out) *total_out = s_sum[0];
        if (verdict) { verdict->total = s_sum[0]; verdict->ok = s_sum[0] == stated ? 1 : 0; verdict->pad = 0; }
    }
}

// ---- expand: product p of the tile -> (row of A's entry, column of B's entry, a * b) ----------------------------------------------
// Runs the real expansion only under a verdict of "right": then start is non-decreasing, start[nnz_a] == products, and product p
// belongs to the LAST entry e with start[e] <= p, at position p - start[e] < len[e] of B's row.
template <typename V, bool VALS>
__global__ __launch_bounds__(GEMM_BLOCK) void gemm_expand_kernel(const GemmVerdict *__restrict__ verdict, const int *__restrict__ start,
                                                                 const int *__restrict__ offa, const int *__restrict__ cola,
                                                                 const V *__restrict__ vala, int rows, int nnz_a,
                                                                 const int *__restrict__ offb, const int *__restrict__ colb,
                                                                 const V *__restrict__ valb, int nnz_b, int products,
                                                                 int *__restrict__ out_row, int *__restrict__ out_col, V *__restrict__ out_val)
{
    __shared__ int s_start[GEMM_TILE], s_row[GEMM_TILE], s_delta[GEMM_TILE];
    __shared__ V s_val[VALS ? GEMM_TILE : 1];
    __shared__ int s_e[2], s_range[2];
    const int tid = (int) threadIdx.x;
    const int p0 = (int) blockIdx.x * GEMM_TILE;                     // (products < 2^31 - 65536: no wrap, here or in p0 + GEMM_TILE)
    const int p1 = min(p0 + GEMM_TILE, products);
    bool wrong = verdict->ok != 1;
    if (!wrong) {
        block_row_range(start, nnz_a, p0, p1 - 1, s_e);              // A's entries of the tile's first and last product (syncs)
        wrong = s_e[1] < s_e[0];                                     // (only with row offsets of B that decrease: not a CSR)
    }
    if (wrong) {                                                     // (the same for every thread of the block)
        for (int p = p0 + tid; p < p1; p += GEMM_BLOCK) {
            out_row[p] = 0; out_col[p] = 0;
            if constexpr (VALS) out_val[p] = V(0);
        }
        return;
    }
    const int e0 = s_e[0], e1 = s_e[1];
    block_row_range(offa, rows, e0, e1, s_range);                    // ... and their rows (syncs)
    const int r_lo = s_range[0], r_hi = s_range[1];
    const int last_b = max(nnz_b - 1, 0);
    const long long span = (long long) e1 - e0 + 1;
    if (span <= GEMM_TILE) {
        for (int k = tid; k < (int) span; k += GEMM_BLOCK) {
            const int e = e0 + k, st = start[e];
            s_start[k] = st;
            s_delta[k] = offb[cola[e]] - st;                         // product p of entry e is B's entry p + delta
            s_row[k] = row_of(offa, r_lo, r_hi, e);
            if constexpr (VALS) s_val[k] = vala[e];
        }
        __syncthreads();
        for (int p = p0 + tid; p < p1; p += GEMM_BLOCK) {
            int lo = 0, hi = (int) span - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_start[mid] <= p) lo = mid; else hi = mid - 1;
            }
            const int j = min(max(p + s_delta[lo], 0), last_b);
            out_row[p] = s_row[lo]; out_col[p] = colb[j];
            if constexpr (VALS) out_val[p] = s_val[lo] * valb[j];
        }
    } else {
        for (int p = p0 + tid; p < p1; p += GEMM_BLOCK) {
            const int e = row_of(start, e0, e1, p);
            const int j = min(max(offb[cola[e]] + (p - start[e]), 0), last_b);
            out_row[p] = row_of(offa, r_lo, r_hi, e); out_col[p] = colb[j];
            if constexpr (VALS) out_val[p] = vala[e] * valb[j];
        }
    }
}

__global__ void gemm_count_kernel(int *__restrict__ nnz_out, int v) { *nnz_out = v; }

__global__ void gemm_verdict_kernel(const GemmVerdict *__restrict__ verdict, int *__restrict__ nnz_out)
{
    if (verdict->ok != 1) *nnz_out = -1;
}

// ---- temp storage -------------------------------------------------------------------------------------------------------------------
struct CountLayout {
    long long blocks;
    uint64_t partial_off, total;
};
static CountLayout count_layout(int nnz_a)
{
    CountLayout L{};
    L.blocks = std::max<long long>(1, ((long long) nnz_a + GEMM_TILE - 1) / GEMM_TILE);
    L.partial_off = 0;
    L.total = align256((uint64_t) L.blocks * 8);
    return L;
}

struct GemmLayout {
    CountLayout count;
    uint64_t count_off, verdict_off, len_off, start_off, bsum_off, trow_off, tcol_off, tval_off, coo_off, soff_off, scol_off, sval_off,
             dup_off, total;
    size_t coo_bytes, dup_bytes;
};
// the per-block sums and the verdict; len, start and the scan's block sums; the triples; the sort's temp; the sorted CSR with its
// duplicates; the duplicate pass's temp
static GemmLayout gemm_layout(int rows, int cols, int nnz_a, int products, int value_bytes)
{
    GemmLayout L{};
    L.count = count_layout(nnz_a);
    const uint64_t n = (uint64_t) std::max(products, 1);
    uint64_t off = 0;
    L.count_off = off; off += L.count.total;
    L.verdict_off = off; off = align256(off + sizeof(GemmVerdict));
    L.len_off = off; off = align256(off + (uint64_t) std::max(nnz_a, 1) * 4);
    L.start_off = off; off = align256(off + ((uint64_t) nnz_a + 1) * 4);
    L.bsum_off = off; off = align256(off + (uint64_t) (((long long) nnz_a + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
    if (products > 0) {
        L.trow_off = off; off = align256(off + n * 4);
        L.tcol_off = off; off = align256(off + n * 4);
        L.tval_off = off; off = align256(off + n * value_bytes);
        L.coo_bytes = (size_t) coo_temp_bytes(rows, cols, products, value_bytes);
        L.coo_off = off; off = align256(off + L.coo_bytes);
        L.soff_off = off; off = align256(off + ((uint64_t) rows + 1) * 4);
        L.scol_off = off; off = align256(off + n * 4);
        L.sval_off = off; off = align256(off + n * value_bytes);
        L.dup_bytes = (size_t) dup_layout(products).total;
        L.dup_off = off; off = align256(off + L.dup_bytes);
    }
    L.total = off;
    return L;
}

// the sizes both entry points take: refused before anything else is looked at
static bool gemm_sizes_ok(long long rows, long long inner, long long nnz_a, long long nnz_b)
{
    if (rows < 0 || inner < 0 || nnz_a < 0 || nnz_b < 0) return false;
    if ((nnz_a > 0 || nnz_b > 0) && (rows == 0 || inner == 0)) return false;
    return rows + nnz_a <= MAX_ITEMS && inner + nnz_b <= MAX_ITEMS;
}

int gemm_products_impl(void *d_temp, size_t *temp_bytes, const int32_t *oa, const int32_t *ca, int32_t rows, int32_t inner, int32_t nnz_a,
                       const int32_t *ob, int32_t nnz_b, int64_t *d_products, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || !gemm_sizes_ok(rows, inner, nnz_a, nnz_b)) return hipErrorInvalidValue;
    const CountLayout L = count_layout(nnz_a);
    if (d_temp == nullptr) { *temp_bytes = (size_t) L.total; return hipSuccess; }
    if (*temp_bytes < L.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!d_products || (nnz_a > 0 && (!ca || !ob))) return hipErrorInvalidValue;
    long long *partial = reinterpret_cast<long long *>(static_cast<char *>(d_temp) + L.partial_off);
    const unsigned grid = (unsigned) L.blocks;
    hipLaunchKernelGGL(gemm_lengths_kernel<false>, dim3(grid), dim3(GEMM_BLOCK), 0, stream, ca, nnz_a, ob, nullptr, partial);
    if (int e = launched(stream, debug_sync, "gemm_lengths_kernel", grid)) return e;
    hipLaunchKernelGGL(gemm_total_kernel, dim3(1), dim3(GEMM_BLOCK), 0, stream, partial, L.blocks, 0LL, reinterpret_cast<long long *>(d_products),
                       nullptr);
    return launched(stream, debug_sync, "gemm_total_kernel", 1);
}

template <typename V>
int csr_gemm_impl(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t inner, int32_t cols, const V *va, const int32_t *oa,
                  const int32_t *ca, int32_t nnz_a, const V *vb, const int32_t *ob, const int32_t *cb, int32_t nnz_b, int32_t products,
                  int32_t capacity, V *vc, int32_t *oc, int32_t *cc, int32_t *d_nnz_c, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || cols < 0 || products < 0 || capacity < 0 || !gemm_sizes_ok(rows, inner, nnz_a, nnz_b)) return hipErrorInvalidValue;
    if ((nnz_a > 0 || nnz_b > 0) && cols == 0) return hipErrorInvalidValue;
    if ((long long) rows + products > MAX_ITEMS) return hipErrorInvalidValue;
    if (products > 0 && (rows == 0 || inner == 0 || cols == 0)) return hipErrorInvalidValue;
    const GemmLayout L = gemm_layout(rows, cols, nnz_a, products, (int) sizeof(V));
    if (d_temp == nullptr) { *temp_bytes = (size_t) L.total; return hipSuccess; }
    if (*temp_bytes < L.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!oc || !d_nnz_c) return hipErrorInvalidValue;
    // values for every matrix or for none (an array of no entries, or of no capacity, has no say)
    const bool with_values = (capacity > 0 && vc != nullptr) || (nnz_a > 0 && va != nullptr) || (nnz_b > 0 && vb != nullptr);
    if (with_values && ((capacity > 0 && !vc) || (nnz_a > 0 && !va) || (nnz_b > 0 && !vb))) return hipErrorInvalidValue;
    if (nnz_a > 0 && (!oa || !ca || !ob)) return hipErrorInvalidValue;
    if (nnz_b > 0 && !cb) return hipErrorInvalidValue;
    if (products > 0 && capacity > 0 && !cc) return hipErrorInvalidValue;
    const bool values = with_values && capacity > 0;                 // (without room for C's entries no value is ever written)

    char *base = static_cast<char *>(d_temp);
    const unsigned rgrid = grid_for((long long) rows + 1, 256);
    const bool can_hold = nnz_a > 0 && nnz_b > 0;                    // (else the true count is 0)
    if (products == 0 || !can_hold) {
        hipLaunchKernelGGL(tr_fill_kernel, dim3(rgrid), dim3(256), 0, stream, oc, (long long) rows + 1, 0);
        if (int e = launched(stream, debug_sync, "tr_fill_kernel", rgrid)) return e;
        hipLaunchKernelGGL(gemm_count_kernel, dim3(1), dim3(1), 0, stream, d_nnz_c, products == 0 ? 0 : -1);
        if (int e = launched(stream, debug_sync, "gemm_count_kernel", 1)) return e;
        if (!can_hold) return hipSuccess;
    }
    // ---- 1. lengths, their scan, the verdict
    long long *partial = reinterpret_cast<long long *>(base + L.count_off + L.count.partial_off);
    GemmVerdict *verdict = reinterpret_cast<GemmVerdict *>(base + L.verdict_off);
    int *len = reinterpret_cast<int *>(base + L.len_off), *start = reinterpret_cast<int *>(base + L.start_off);
    int *bsum = reinterpret_cast<int *>(base + L.bsum_off);
    const unsigned lgrid = (unsigned) L.count.blocks;
    hipLaunchKernelGGL(gemm_lengths_kernel<true>, dim3(lgrid), dim3(GEMM_BLOCK), 0, stream, ca, nnz_a, ob, len, partial);
    if (int e = launched(stream, debug_sync, "gemm_lengths_kernel", lgrid)) return e;
    hipLaunchKernelGGL(gemm_total_kernel, dim3(1), dim3(GEMM_BLOCK), 0, stream, partial, L.count.blocks, (long long) products, nullptr, verdict);
    if (int e = launched(stream, debug_sync, "gemm_total_kernel", 1)) return e;
    if (products > 0) {
        if (int e = scan_table(len, nnz_a, bsum, start, stream, debug_sync)) return e;
        // ---- 2. expand
        int *trow = reinterpret_cast<int *>(base + L.trow_off), *tcol = reinterpret_cast<int *>(base + L.tcol_off);
        V *tval = reinterpret_cast<V *>(base + L.tval_off);
        const unsigned egrid = grid_for(products, GEMM_TILE);
        if (values)
            hipLaunchKernelGGL((gemm_expand_kernel<V, true>), dim3(egrid), dim3(GEMM_BLOCK), 0, stream, verdict, start, oa, ca, va, rows, nnz_a, ob,
                               cb, vb, nnz_b, products, trow, tcol, tval);
        else
            hipLaunchKernelGGL((gemm_expand_kernel<V, false>), dim3(egrid), dim3(GEMM_BLOCK), 0, stream, verdict, start, oa, ca, va, rows, nnz_a, ob,
                               cb, vb, nnz_b, products, trow, tcol, tval);
        if (int e = launched(stream, debug_sync, "gemm_expand_kernel", egrid)) return e;
        // ---- 3. sort
        int *soff = reinterpret_cast<int *>(base + L.soff_off), *scol = reinterpret_cast<int *>(base + L.scol_off);
        V *sval = reinterpret_cast<V *>(base + L.sval_off);
        const CooLayout C = coo_layout(rows, cols, products, (int) sizeof(V));
        const int st = values ? coo_run<V, true>(base + L.coo_off, C, tval, trow, tcol, rows, products, soff, scol, sval, nullptr, stream, debug_sync)
                              : coo_run<V, false>(base + L.coo_off, C, nullptr, trow, tcol, rows, products, soff, scol, nullptr, nullptr, stream,
                                                  debug_sync);
        if (st) return st;
        // ---- 4. compress
        size_t dup_bytes = L.dup_bytes;
        if (int e = sum_duplicates_impl<V>(base + L.dup_off, &dup_bytes, values ? sval : nullptr, soff, scol, rows, cols, products, capacity,
                                           values ? vc : nullptr, oc, cc, d_nnz_c, stream, debug_sync))
            return e;
    }
    // ---- 5. the verdict
    hipLaunchKernelGGL(gemm_verdict_kernel, dim3(1), dim3(1), 0, stream, verdict, d_nnz_c);
    return launched(stream, debug_sync, "gemm_verdict_kernel", 1);
}

}  // namespace

extern "C" {

int mspmv_csr_gemm_products(void *d_temp, size_t *temp_bytes, const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t rows,
                            int32_t inner, int32_t nnz_a, const int32_t *d_row_offsets_b, int32_t nnz_b, int64_t *d_products,
                            mspmv_stream_t stream, int debug_sync)
{
    return gemm_products_impl(d_temp, temp_bytes, d_row_offsets_a, d_column_indices_a, rows, inner, nnz_a, d_row_offsets_b, nnz_b, d_products,
                              reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_gemm_f32(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t inner, int32_t cols, const float *d_values_a,
                       const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a, const float *d_values_b,
                       const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b, int32_t products, int32_t capacity_c,
                       float *d_values_c, int32_t *d_row_offsets_c, int32_t *d_column_indices_c, int32_t *d_nnz_c, mspmv_stream_t stream,
                       int debug_sync)
{
    return csr_gemm_impl<float>(d_temp, temp_bytes, rows, inner, cols, d_values_a, d_row_offsets_a, d_column_indices_a, nnz_a, d_values_b,
                                d_row_offsets_b, d_column_indices_b, nnz_b, products, capacity_c, d_values_c, d_row_offsets_c, d_column_indices_c,
                                d_nnz_c, reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_gemm_f64(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t inner, int32_t cols, const double *d_values_a,
                       const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a, const double *d_values_b,
                       const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b, int32_t products, int32_t capacity_c,
                       double *d_values_c, int32_t *d_row_offsets_c, int32_t *d_column_indices_c, int32_t *d_nnz_c, mspmv_stream_t stream,
                       int debug_sync)
{
    return csr_gemm_impl<double>(d_temp, temp_bytes, rows, inner, cols, d_values_a, d_row_offsets_a, d_column_indices_a, nnz_a, d_values_b,
                                 d_row_offsets_b, d_column_indices_b, nnz_b, products, capacity_c, d_values_c, d_row_offsets_c, d_column_indices_c,
                                 d_nnz_c, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
