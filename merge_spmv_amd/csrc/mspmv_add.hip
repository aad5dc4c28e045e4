// mspmv_add.hip -- C = alpha * A + beta * B for two CSR matrices on the device (mspmv_csr_add_* of include/mspmv.h).
//
// What.  A and B are canonical (every row sorted by column, no column twice), so each is a sorted sequence of the key (row, column)
// and C's pattern is the union of the two sequences: a MERGE.  The merge of the nnz_a + nnz_b entries (ties: A's entry first) is cut
// into tiles of ADD_TILE merged entries at equally spaced diagonals, whatever the row lengths -- one row holding every entry costs
// what a million short ones cost.  The key of an entry is never stored.  Where diagonal d crosses the merge is found in two steps:
// the row, by binary search over S[r] = row_offsets_a[r] + row_offsets_b[r] (every key of an earlier row precedes merged position
// S[r], none of row r does), then the split of the d - S[r] entries of that row between A and B by a merge-path search over the two
// column lists of the row alone.  A merged entry is a HEAD unless it is B's entry right behind A's entry of the same key.
//   count   each tile finds its start and end (two threads search concurrently; the start goes to temp storage, 16 bytes per tile),
//           stages its A and B ranges of column indices in LDS -- with A's entry before the range (the predecessor of the tile's
//           first entry) and one entry of look-ahead past either range --, gives every thread ADD_IPT consecutive merged entries by
//           the same two-step search (rows from the offsets, columns in LDS), and counts the heads;
//   scan    exclusive scan of the tile counts (mspmv_scan.hpp); its total is *d_nnz_c;
//   fill    the same staging and walk, now with the values: a head writes its column and value at tile base + its rank among the
//           tile's heads (block scan), through LDS so that consecutive lanes write consecutive entries of C.  A head of A whose
//           partner in B sits behind a thread or tile boundary reads it from the next position (the look-ahead); the partner, not
//           being a head, writes nothing.  row_offsets_c[r] = the heads in front of merged position S[r]; every such position lies
//           in exactly one tile (those equal to nnz_a + nnz_b go to the last one), whose threads take the rows in a strided loop
//           and read the rank off the per-thread scan and head masks -- a run of empty rows costs a coalesced store like any other.
// No atomics on global memory, no workgroup waits on another, the host launches the same kernels whatever the data and never reads
// device memory: every output position and value is a function of the input alone, and the call can be captured in a graph.
//
// Values.  alpha * a, beta * b, (alpha * a) + (beta * b), each operation rounded on its own: contraction into fused multiply-adds is
// switched off for this file (the pragma below), because hipcc contracts by default.
//
// Robustness.  Column indices are only ever COMPARED: on rows that are not sorted or hold a column twice the result is unspecified,
// but the searches stay inside the row's range of either array, every LDS index is clamped to the staged range, the count and the
// fill pass take the same decisions (so the ranks stay below the counts), and every loop is bounded.  Row offsets must be valid, as
// for every call of the library.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // block_inclusive_scan, the three scan kernels

#include "mspmv_radix.hpp"     // launched, scan_table, tr_fill_kernel

// 256 threads x 7 merged entries.  An odd count per thread keeps the lanes' walks through the two staged column lists (a stride of
// up to ADD_IPT words between neighbouring lanes) off a common bank; 7 x 256 entries need 7 KiB of LDS for the columns and 7 / 14
// KiB for the staged values of C.
constexpr int ADD_BLOCK = 256, ADD_IPT = 7, ADD_TILE = ADD_BLOCK * ADD_IPT;
constexpr int ADD_SENTINEL = 0x7fffffff;
enum { ADD_COUNT = 0, ADD_FILL = 1, ADD_FILL_VALUES = 2 };

// where a diagonal crosses the merge: A's share i of the d entries in front of it (B's is d - i), the row that position lies in
// (the LAST r with S[r] <= d) and the FIRST r with S[r] >= d (the rows whose offsets this position starts with)
struct AddSplit { int i, row, row_first, pad; };

// the largest r in [lo, hi] with S[r] <= d (true for lo)
__device__ __forceinline__ int add_row_last(const int *__restrict__ offa, const int *__restrict__ offb, int lo, int hi, int d)
{
    while (lo < hi) {
        const int mid = (int) (((long long) lo + hi + 1) >> 1);
        if (offa[mid] + offb[mid] <= d) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the smallest r in [lo, hi] with S[r] >= d (true for hi)
__device__ __forceinline__ int add_row_first(const int *__restrict__ offa, const int *__restrict__ offb, int lo, int hi, int d)
{
    while (lo < hi) {
        const int mid = (int) (((long long) lo + hi) >> 1);
        if (offa[mid] + offb[mid] >= d) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the split of diagonal d, 0 <= d <= nnz_a + nnz_b, from global memory (rows >= 1)
__device__ AddSplit add_split(const int *__restrict__ offa, const int *__restrict__ cola, const int *__restrict__ offb,
                              const int *__restrict__ colb, int rows, int d)
{
    const int r = add_row_last(offa, offb, 0, rows - 1, d);
    const int sa = offa[r], ea = offa[r + 1], sb = offb[r], eb = offb[r + 1];
    const int e = d - (sa + sb);                                    // entries of row r in front of the diagonal
    int lo = max(0, e - (eb - sb)), hi = min(e, ea - sa);           // A's share of them
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);                      // (lo + hi may pass 2^31: one row can hold every entry)
        if (cola[sa + mid] <= colb[sb + e - 1 - mid]) lo = mid + 1; else hi = mid;       // (ties: A first)
    }
    AddSplit s;
    s.i = sa + lo; s.row = r; s.pad = 0;
    s.row_first = sa + sb == d ? add_row_first(offa, offb, 0, r, d) : r + 1;
    return s;
}

template <typename V, int MODE>
__global__ __launch_bounds__(ADD_BLOCK) void add_tile_kernel(const int *__restrict__ offa, const int *__restrict__ cola,
                                                             const V *__restrict__ vala, int na, const int *__restrict__ offb,
                                                             const int *__restrict__ colb, const V *__restrict__ valb, int nb, int rows,
                                                             V alpha, V beta, AddSplit *__restrict__ splits, int *__restrict__ counts,
                                                             const int *__restrict__ pos, int *__restrict__ colc, V *__restrict__ valc,
                                                             int *__restrict__ offc, int *__restrict__ nnzc)
{
    __shared__ int s_cols[ADD_TILE + 4];            // A[i0 - 1 .. i1], then B[j0 .. j1]; the fill pass reuses it for C's columns
    __shared__ V s_vals[MODE == ADD_FILL_VALUES ? ADD_TILE : 1];
    __shared__ int s_rank[ADD_BLOCK + 1];
    __shared__ unsigned s_mask[ADD_BLOCK + 1];
    __shared__ int s_tmp[4];
    __shared__ AddSplit s_split[2];
    const int tid = (int) threadIdx.x, t = (int) blockIdx.x, tiles = (int) gridDim.x;
    const int n = na + nb;
    const int d0 = t * ADD_TILE, d1 = min(d0 + ADD_TILE, n), items = d1 - d0;

    // ---- the tile's start and end
    if (tid == 0 || tid == 64) {
        const int which = tid >> 6;
        AddSplit s;
        if (which == 1 && t + 1 == tiles) { s.i = na; s.row = rows - 1; s.row_first = rows + 1; s.pad = 0; }
        else if (MODE == ADD_COUNT) s = add_split(offa, cola, offb, colb, rows, which ? d1 : d0);
        else s = splits[t + which];
        if (MODE == ADD_COUNT && which == 0) splits[t] = s;
        s_split[which] = s;
    }
    __syncthreads();
    const int i0 = s_split[0].i, j0 = d0 - i0, r0 = s_split[0].row, r1 = min(s_split[1].row, rows - 1);
    const int cnta = min(max(s_split[1].i - i0, 0), items), cntb = items - cnta;
    const int i1 = i0 + cnta, j1 = j0 + cntb;
    int *s_b = s_cols + cnta + 2;

    // ---- stage the column indices: A[i0 - 1, i1] and B[j0, j1] (what lies outside an array is never compared on canonical input)
    for (int k = tid; k < cnta + 2; k += ADD_BLOCK) {
        const int g = i0 - 1 + k;
        s_cols[k] = g >= 0 && g < na ? cola[g] : ADD_SENTINEL;
    }
    for (int k = tid; k < cntb + 1; k += ADD_BLOCK) {
        const int g = j0 + k;
        s_b[k] = g >= 0 && g < nb ? colb[g] : ADD_SENTINEL;
    }
    __syncthreads();
    auto col_a = [&](int i) { return s_cols[min(max(i - i0 + 1, 0), cnta + 1)]; };
    auto col_b = [&](int j) { return s_b[min(max(j - j0, 0), cntb)]; };

    // ---- this thread's ADD_IPT merged entries from position p on
    const int first = tid * ADD_IPT, mine = min(max(items - first, 0), ADD_IPT);
    int c[ADD_IPT];
    V v[ADD_IPT];
    unsigned heads = 0;
    if (mine > 0) {
        int p = d0 + first;
        int r = add_row_last(offa, offb, r0, r1, p);
        int sa = offa[r], ea = offa[r + 1], sb = offb[r], eb = offb[r + 1];
        int lo = max(max(sa, p - eb), max(i0, p - j1)), hi = min(min(ea, p - sb), min(i1, p - j0));
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);                  // (positions in A, up to 2^31: lo + hi would wrap)
            if (col_a(mid) <= col_b(p - 1 - mid)) lo = mid + 1; else hi = mid;
        }
        int i = min(max(lo, sa), ea);
        int j = min(max(p - i, sb), eb);
#pragma unroll
        for (int k = 0; k < ADD_IPT; ++k) {
            c[k] = 0; v[k] = V(0);
            if (k < mine) {
                if (i >= ea && j >= eb) {                            // the row is used up: on to the next row that has entries
                    int rn = min(r + 1, rows - 1);
                    if (rn < r1 && offa[rn + 1] + offb[rn + 1] <= p) rn = add_row_last(offa, offb, rn, r1, p);
                    r = rn;
                    sa = offa[r]; ea = offa[r + 1]; sb = offb[r]; eb = offb[r + 1];
                    i = sa; j = sb;
                }
                if (i < ea && (j >= eb || col_a(i) <= col_b(j))) {   // A's entry: always a head
                    c[k] = col_a(i);
                    heads |= 1u << k;
                    if constexpr (MODE == ADD_FILL_VALUES) {
                        const V x = alpha * vala[i];
                        if (j < eb && col_b(j) == c[k]) { const V y = beta * valb[j]; v[k] = x + y; }
                        else v[k] = x;
                    }
                    ++i;
                } else if (j < eb) {                                 // B's entry: a head unless A's entry of the same key is in front
                    c[k] = col_b(j);
                    if (!(i > sa && col_a(i - 1) == c[k])) {
                        heads |= 1u << k;
                        if constexpr (MODE == ADD_FILL_VALUES) v[k] = beta * valb[j];
                    }
                    ++j;
                }
                ++p;
            }
        }
    }
    const int nheads = __popc(heads);
    const int incl = block_inclusive_scan(nheads, s_tmp);            // (two barriers: every walk has ended behind it)
    if constexpr (MODE == ADD_COUNT) {
        if (tid == ADD_BLOCK - 1) counts[t] = incl;
        return;
    } else {
        // ---- C's entries through LDS, then consecutive lanes write consecutive entries
        s_rank[tid] = incl - nheads;
        s_mask[tid] = heads;
        if (tid == ADD_BLOCK - 1) { s_rank[ADD_BLOCK] = incl; s_mask[ADD_BLOCK] = 0; }
        int rank = incl - nheads;
#pragma unroll
        for (int k = 0; k < ADD_IPT; ++k)
            if (heads >> k & 1u) {
                s_cols[rank] = c[k];
                if constexpr (MODE == ADD_FILL_VALUES) s_vals[rank] = v[k];
                ++rank;
            }
        __syncthreads();
        const int total = s_rank[ADD_BLOCK];
        const long long base = pos[t];
        for (int k = tid; k < total; k += ADD_BLOCK) {
            colc[base + k] = s_cols[k];
            if constexpr (MODE == ADD_FILL_VALUES) valc[base + k] = s_vals[k];
        }
        // ---- C's offsets of the rows whose merged position S[r] lies in this tile
        const int rfirst = s_split[0].row_first, rend = min(s_split[1].row_first, rows + 1);
        for (long long r = (long long) rfirst + tid; r < rend; r += ADD_BLOCK) {
            const int q = min(max(offa[r] + offb[r] - d0, 0), items);
            const int owner = q / ADD_IPT, within = q - owner * ADD_IPT;
            offc[r] = (int) base + s_rank[owner] + __popc(s_mask[owner] & ((1u << within) - 1u));
        }
        if (t == 0 && tid == 0) *nnzc = pos[tiles];
    }
}

__global__ void add_empty_kernel(int *__restrict__ nnz_out) { *nnz_out = 0; }

struct AddLayout {
    long long tiles;
    uint64_t splits_off, counts_off, pos_off, bsum_off, total;
};
// temp storage: per tile its split (16 bytes), its head count and the count's scan (4 + 4), and the scan's block sums
static AddLayout add_layout(long long n)
{
    AddLayout L{};
    L.tiles = (n + ADD_TILE - 1) / ADD_TILE;
    uint64_t off = 0;
    L.splits_off = off; off = align256(off + (uint64_t) std::max(L.tiles, 1LL) * sizeof(AddSplit));
    L.counts_off = off; off = align256(off + (uint64_t) std::max(L.tiles, 1LL) * 4);
    L.pos_off = off; off = align256(off + (uint64_t) (L.tiles + 1) * 4);
    L.bsum_off = off; off = align256(off + (uint64_t) ((L.tiles + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4);
    L.total = off;
    return L;
}

template <typename V>
int csr_add_impl(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t cols, V alpha, const V *va, const int32_t *oa, const int32_t *ca,
                 int32_t na, V beta, const V *vb, const int32_t *ob, const int32_t *cb, int32_t nb, V *vc, int32_t *oc, int32_t *cc,
                 int32_t *d_nnz_c, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || rows < 0 || cols < 0 || na < 0 || nb < 0) return hipErrorInvalidValue;
    const long long n = (long long) na + nb;
    if (n > 0 && (rows == 0 || cols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + n > MAX_ITEMS) return hipErrorInvalidValue;
    const AddLayout L = add_layout(n);
    if (d_temp == nullptr) { *temp_bytes = (size_t) L.total; return hipSuccess; }
    if (*temp_bytes < L.total || (reinterpret_cast<uintptr_t>(d_temp) & 15)) return hipErrorInvalidValue;
    if (!oc || !d_nnz_c) return hipErrorInvalidValue;
    // values for every matrix or for none (an array of no entries has no say)
    const bool with_values = vc != nullptr || (na > 0 && va != nullptr) || (nb > 0 && vb != nullptr);
    if (with_values && ((n > 0 && !vc) || (na > 0 && !va) || (nb > 0 && !vb))) return hipErrorInvalidValue;
    if (n == 0) {
        const unsigned g = grid_for((long long) rows + 1, 256);
        hipLaunchKernelGGL(tr_fill_kernel, dim3(g), dim3(256), 0, stream, oc, (long long) rows + 1, 0);
        if (int e = launched(stream, debug_sync, "tr_fill_kernel", g)) return e;
        hipLaunchKernelGGL(add_empty_kernel, dim3(1), dim3(1), 0, stream, d_nnz_c);
        return launched(stream, debug_sync, "add_empty_kernel", 1);
    }
    if (!oa || !ob || !cc || (na > 0 && !ca) || (nb > 0 && !cb)) return hipErrorInvalidValue;
    char *base = static_cast<char *>(d_temp);
    AddSplit *splits = reinterpret_cast<AddSplit *>(base + L.splits_off);
    int *counts = reinterpret_cast<int *>(base + L.counts_off), *pos = reinterpret_cast<int *>(base + L.pos_off);
    int *bsum = reinterpret_cast<int *>(base + L.bsum_off);
    const unsigned grid = (unsigned) L.tiles;
    hipLaunchKernelGGL((add_tile_kernel<V, ADD_COUNT>), dim3(grid), dim3(ADD_BLOCK), 0, stream, oa, ca, va, na, ob, cb, vb, nb, rows, alpha, beta,
                       splits, counts, pos, cc, vc, oc, d_nnz_c);
    if (int e = launched(stream, debug_sync, "add_tile_kernel<count>", grid)) return e;
    if (int e = scan_table(counts, L.tiles, bsum, pos, stream, debug_sync)) return e;
    if (with_values)
        hipLaunchKernelGGL((add_tile_kernel<V, ADD_FILL_VALUES>), dim3(grid), dim3(ADD_BLOCK), 0, stream, oa, ca, va, na, ob, cb, vb, nb, rows, alpha,
                           beta, splits, counts, pos, cc, vc, oc, d_nnz_c);
    else
        hipLaunchKernelGGL((add_tile_kernel<V, ADD_FILL>), dim3(grid), dim3(ADD_BLOCK), 0, stream, oa, ca, va, na, ob, cb, vb, nb, rows, alpha, beta,
                           splits, counts, pos, cc, vc, oc, d_nnz_c);
    return launched(stream, debug_sync, "add_tile_kernel<fill>", grid);
}

}  // namespace

extern "C" {

int mspmv_csr_add_f32(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t cols, float alpha, const float *d_values_a,
                      const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a, float beta, const float *d_values_b,
                      const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b, float *d_values_c,
                      int32_t *d_row_offsets_c, int32_t *d_column_indices_c, int32_t *d_nnz_c, mspmv_stream_t stream, int debug_sync)
{
    return csr_add_impl<float>(d_temp, temp_bytes, rows, cols, alpha, d_values_a, d_row_offsets_a, d_column_indices_a, nnz_a, beta, d_values_b,
                               d_row_offsets_b, d_column_indices_b, nnz_b, d_values_c, d_row_offsets_c, d_column_indices_c, d_nnz_c,
                               reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_csr_add_f64(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t cols, double alpha, const double *d_values_a,
                      const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a, double beta, const double *d_values_b,
                      const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b, double *d_values_c,
                      int32_t *d_row_offsets_c, int32_t *d_column_indices_c, int32_t *d_nnz_c, mspmv_stream_t stream, int debug_sync)
{
    return csr_add_impl<double>(d_temp, temp_bytes, rows, cols, alpha, d_values_a, d_row_offsets_a, d_column_indices_a, nnz_a, beta, d_values_b,
                                d_row_offsets_b, d_column_indices_b, nnz_b, d_values_c, d_row_offsets_c, d_column_indices_c, d_nnz_c,
                                reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
