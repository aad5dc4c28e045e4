// mspmv_sddmm.hip -- the sampled dense-dense product on the device (mspmv_sddmm_* of include/mspmv.h): for every stored entry e of a
// CSR pattern, in row r and column c,
//     s = +0.0;  for t = 0 .. k-1:  s = s + U[r*ldu + t] * V[c*ldv + t];      C[e] = alpha * s + (beta == 0 ? +0.0 : beta * C[e])
// with U rows x k and V cols x k row-major -- the value gradient of SpMM (U = dY, V = X), edge scores of a graph (U = V = H).
//
// Balance.  Every entry costs the same k multiply-adds, so the entries are cut into tiles of SDDMM_TILE whatever the row lengths:
// one row holding every entry costs what a million short ones cost.  One block takes one tile, finds the rows of its first and last
// entry (block_row_range), stages that slice of the row offsets in LDS, and every lane finds the row of its entry by a search there;
// a tile whose slice is longer than the tile (long stretches of empty rows inside it) searches in global memory instead, as
// gemm_expand_kernel does.  Consecutive lanes take consecutive entries: the column indices, the old C and the new C are consecutive
// streams.  One launch, no temp storage, no atomics, no workgroup waits on another.
//
// Data movement.  The sum of one entry is sequential, so one lane owns one entry's accumulator.  A lane that walked its own row of V
// in 16-byte steps would make the wave touch 64 different cache lines per load and come back for the rest of each line after the
// 32 KB L1 has lost it.  So V is loaded cooperatively: k is cut into chunks of 128 bytes (32 fp32, 16 fp64, 64 bf16 elements, one
// cache line when the row is aligned to one); for each chunk, 8 neighbouring lanes read one entry's slice of V[c, :] as 8
// consecutive 16-byte words (8 passes cover the wave's 64 entries, 8 loads in flight per lane) and store it in the wave's own LDS
// image, one row of 9 words (144 bytes) per entry.  Then each lane reads its own row back in 16-byte words and accumulates left to
// right.  The stride of 9 words makes those reads conflict-free: a 16-byte LDS read is served in groups of 16 lanes whose lane
// numbers are distinct mod 16, and 9 * l mod 16 is a permutation, so the 16 words of a group fall on 16 different quadruples of the
// 64 banks; the stores of 8 lanes are 128 contiguous bytes.  The image belongs to one wave (9 KB; 36 KB per block, 4 blocks per
// CU), so the hand-over inside a chunk needs no workgroup barrier: LDS operations of one wave execute in order.  Rows of U are
// read directly in 16-byte words: the lanes of one row of the pattern read the same address and coalesce.
//
// Rows of V shorter than 64 bytes skip the LDS (each lane reads its own row in 16-byte words): measured, below.
//
// Alignment.  The 16-byte path needs U and V 16-byte aligned and ldu, ldv multiples of 16 bytes; anything else runs the
// element-wise kernel (one lane, one entry, scalar loads).  Elements past the last full word of a row (k need not be a multiple of
// the word) are loaded one by one in either path: nothing outside [row, row + k) is read.  The two paths, every chunk width and
// every position in a tile add the same products in the same order: C[e] is a function of U's row, V's row, k, alpha, beta and the
// old C[e] alone.
//
// Values.  Every multiply and every add rounded on its own in the compute type: contraction into fused multiply-adds is switched
// off for this file, as in mspmv_gemm.hip and mspmv_add.hip.  bf16 is the upper half of an fp32 and is widened in registers.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_internal.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

#include "mspmv_scan.hpp"      // row_of, block_row_range

#include "mspmv_radix.hpp"     // launched

constexpr int SDDMM_BLOCK = 256, SDDMM_WAVES = SDDMM_BLOCK / 64, SDDMM_IPT = 2, SDDMM_TILE = SDDMM_BLOCK * SDDMM_IPT;
constexpr int SDDMM_WORDS = 8;                          // 16-byte words per chunk of k: 128 bytes
constexpr int SDDMM_ROW = SDDMM_WORDS + 1;              // words per entry in the LDS image (the pad that spreads the banks)
enum { SDDMM_ELEMENTWISE = 0, SDDMM_STAGED = 1, SDDMM_DIRECT = 2 };

// one 16-byte word of a row of U or V
template <typename S>
union SddmmWord {
    uint4 q;
    S e[16 / sizeof(S)];
};

template <typename S, typename C> __device__ __forceinline__ C sddmm_widen(S x) { return x; }
template <> __device__ __forceinline__ float sddmm_widen<uint16_t, float>(uint16_t x) { return __uint_as_float((unsigned) x << 16); }

// word j of a chunk that starts at p: a 16-byte load when all its n elements exist, else the n that do, one by one
template <typename S>
__device__ __forceinline__ SddmmWord<S> sddmm_load(const S *__restrict__ p, int n)
{
    constexpr int EPW = 16 / (int) sizeof(S);
    SddmmWord<S> w;
    if (n >= EPW) {
        w.q = *reinterpret_cast<const uint4 *>(p);
    } else {
        w.q = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int i = 0; i < EPW - 1; ++i)
            if (i < n) w.e[i] = p[i];
    }
    return w;
}

// s = s + u[i] * v[i] for the first n elements of a word, left to right
template <typename S, typename C>
__device__ __forceinline__ void sddmm_accumulate(C &s, const SddmmWord<S> &u, const SddmmWord<S> &v, int n)
{
    constexpr int EPW = 16 / (int) sizeof(S);
#pragma unroll
    for (int i = 0; i < EPW; ++i)
        if (i < n) {
            const C p = sddmm_widen<S, C>(u.e[i]) * sddmm_widen<S, C>(v.e[i]);
            s = s + p;
        }
}

// one chunk of w <= CH elements from element t0 on (FULL: w == CH, every word whole).  All 64 lanes of the wave come here together.
template <typename S, typename C, int MODE, bool FULL>
__device__ __forceinline__ void sddmm_chunk(C &s, const S *__restrict__ urow, const S *__restrict__ v, int ldv, int col,
                                            unsigned long long valid_mask, bool valid, int t0, int w, uint4 *__restrict__ image)
{
    constexpr int EPW = 16 / (int) sizeof(S);
    const int lane = (int) threadIdx.x & 63;
    const int words = FULL ? SDDMM_WORDS : (w + EPW - 1) / EPW;
    SddmmWord<S> uw[SDDMM_WORDS];
#pragma unroll
    for (int j = 0; j < SDDMM_WORDS; ++j)
        if (valid && j < words) uw[j] = sddmm_load<S>(urow + t0 + j * EPW, FULL ? EPW : w - j * EPW);
    if constexpr (MODE == SDDMM_STAGED) {
        // lanes 8g .. 8g+7 load the 8 words of entry 8p + g's slice of its row of V
        const int word = lane & 7, n = FULL ? EPW : w - word * EPW;
        SddmmWord<S> vw[SDDMM_WORDS];
#pragma unroll
        for (int p = 0; p < SDDMM_WORDS; ++p) {
            const int src = p * 8 + (lane >> 3);
            const int c = __shfl(col, src, 64);
            if ((valid_mask >> src & 1ull) && n > 0) vw[p] = sddmm_load<S>(v + (long long) c * ldv + t0 + word * EPW, n);
        }
#pragma unroll
        for (int p = 0; p < SDDMM_WORDS; ++p) {
            const int src = p * 8 + (lane >> 3);
            if ((valid_mask >> src & 1ull) && n > 0) image[src * SDDMM_ROW + word] = vw[p].q;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int j = 0; j < SDDMM_WORDS; ++j)
            if (valid && j < words) {
                SddmmWord<S> x;
                x.q = image[lane * SDDMM_ROW + j];
                sddmm_accumulate<S, C>(s, uw[j], x, FULL ? EPW : w - j * EPW);
            }
        // (the next chunk's stores come behind these reads: one wave's LDS operations execute in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        const S *vrow = v + (long long) col * ldv;
#pragma unroll
        for (int j = 0; j < SDDMM_WORDS; ++j)
            if (valid && j < words) {
                const SddmmWord<S> x = sddmm_load<S>(vrow + t0 + j * EPW, FULL ? EPW : w - j * EPW);
                sddmm_accumulate<S, C>(s, uw[j], x, FULL ? EPW : w - j * EPW);
            }
    }
}

template <typename S, typename C, int MODE>
__global__ __launch_bounds__(SDDMM_BLOCK) void sddmm_kernel(const int *__restrict__ off, const int *__restrict__ cols,
                                                            const S *__restrict__ u, int ldu, const S *__restrict__ v, int ldv,
                                                            C *__restrict__ out, int rows, int nnz, int k, C alpha, C beta)
{
    constexpr int CH = SDDMM_WORDS * 16 / (int) sizeof(S);          // elements per chunk
    __shared__ int s_off[SDDMM_TILE];
    __shared__ int s_range[2];
    __shared__ uint4 s_image[MODE == SDDMM_STAGED ? SDDMM_WAVES * 64 * SDDMM_ROW : 1];
    const int tid = (int) threadIdx.x, wave = tid >> 6;
    const int e0 = (int) blockIdx.x * SDDMM_TILE;                   // (nnz < 2^31 - 65536: no wrap, here or in e0 + SDDMM_TILE)
    const int e1 = min(e0 + SDDMM_TILE, nnz);
    block_row_range(off, rows, e0, e1 - 1, s_range);                // (syncs)
    const int r_lo = s_range[0], r_hi = max(s_range[1], r_lo);
    const long long span = (long long) r_hi - r_lo + 1;
    const bool staged_rows = span <= SDDMM_TILE;
    if (staged_rows) {
        for (int i = tid; i < (int) span; i += SDDMM_BLOCK) s_off[i] = off[r_lo + i];
        __syncthreads();
    }
    uint4 *image = s_image + (MODE == SDDMM_STAGED ? wave * 64 * SDDMM_ROW : 0);
    for (int i = 0; i < SDDMM_IPT; ++i) {
        const int e = e0 + i * SDDMM_BLOCK + tid;
        const bool valid = e < e1;
        const unsigned long long valid_mask = __ballot(valid);
        if (valid_mask == 0) break;                                  // (the same for the whole wave)
        int col = 0, r = r_lo;
        if (valid) {
            col = cols[e];
            r = staged_rows ? r_lo + row_of(s_off, 0, (int) span - 1, e) : row_of(off, r_lo, r_hi, e);
        }
        const S *urow = u + (long long) r * ldu;
        C s = C(0);
        if constexpr (MODE == SDDMM_ELEMENTWISE) {
            if (valid) {
                const S *vrow = v + (long long) col * ldv;
                for (int t = 0; t < k; ++t) {
                    const C p = sddmm_widen<S, C>(urow[t]) * sddmm_widen<S, C>(vrow[t]);
                    s = s + p;
                }
            }
        } else {
            int t0 = 0;
            for (; t0 + CH <= k; t0 += CH) sddmm_chunk<S, C, MODE, true>(s, urow, v, ldv, col, valid_mask, valid, t0, CH, image);
            if (t0 < k) sddmm_chunk<S, C, MODE, false>(s, urow, v, ldv, col, valid_mask, valid, t0, k - t0, image);
        }
        if (valid) {
            const C a = alpha * s;
            C b = C(0);
            if (beta != C(0)) b = beta * out[e];
            out[e] = a + b;
        }
    }
}

// The form of the 16-byte path.  Measured (profiles/sddmm_bench.txt, the A/B section): through LDS is the faster form from rows of V of
// 64 bytes on (1.7 - 4.4 x on config 2 at k = 128); rows shorter than that (bf16 with k < 32) lie inside one half of a cache line, a
// wave's few loads come back to it at once and the staging only costs -- there every lane walks its own row (1.4 - 2.9 x faster at
// 32 bytes).  The choice depends on k alone, and both forms give the same bits.  -DMSPMV_SDDMM_DIRECT builds the library with the
// direct form for every k (the other side of that A/B).
#ifdef MSPMV_SDDMM_DIRECT
constexpr int SDDMM_LONG_ROWS = SDDMM_DIRECT;
#else
constexpr int SDDMM_LONG_ROWS = SDDMM_STAGED;
#endif
constexpr int SDDMM_STAGE_FROM_BYTES = 64;

template <typename S, typename C>
int sddmm_impl(const int32_t *off, const int32_t *cols, const S *u, int32_t ldu, const S *v, int32_t ldv, C *out, int32_t rows, int32_t ncols,
               int32_t nnz, int32_t k, C alpha, C beta, hipStream_t stream, int debug_sync)
{
    if (rows < 0 || ncols < 0 || nnz < 0 || k < 0 || ldu < k || ldv < k) return hipErrorInvalidValue;
    if (nnz > 0 && (rows == 0 || ncols == 0)) return hipErrorInvalidValue;
    if ((long long) rows + nnz > MAX_ITEMS) return hipErrorInvalidValue;
    if (nnz == 0) return hipSuccess;
    if (!off || !cols || !out || (k > 0 && (!u || !v))) return hipErrorInvalidValue;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v) | (uintptr_t) ((uint64_t) ldu * sizeof(S)) |
                           (uintptr_t) ((uint64_t) ldv * sizeof(S));
    const bool wide = (bits & 15) == 0;
    const bool staged = wide && SDDMM_LONG_ROWS == SDDMM_STAGED && (long long) k * (long long) sizeof(S) >= SDDMM_STAGE_FROM_BYTES;
    const unsigned grid = grid_for(nnz, SDDMM_TILE);
    if (staged)
        hipLaunchKernelGGL((sddmm_kernel<S, C, SDDMM_STAGED>), dim3(grid), dim3(SDDMM_BLOCK), 0, stream, off, cols, u, ldu, v, ldv, out, rows, nnz,
                           k, alpha, beta);
    else if (wide)
        hipLaunchKernelGGL((sddmm_kernel<S, C, SDDMM_DIRECT>), dim3(grid), dim3(SDDMM_BLOCK), 0, stream, off, cols, u, ldu, v, ldv, out, rows, nnz,
                           k, alpha, beta);
    else
        hipLaunchKernelGGL((sddmm_kernel<S, C, SDDMM_ELEMENTWISE>), dim3(grid), dim3(SDDMM_BLOCK), 0, stream, off, cols, u, ldu, v, ldv, out, rows,
                           nnz, k, alpha, beta);
    return launched(stream, debug_sync, staged ? "sddmm_kernel<16-byte, through LDS>" : wide ? "sddmm_kernel<16-byte>" : "sddmm_kernel<element-wise>",
                    grid);
}

}  // namespace

extern "C" {

int mspmv_sddmm_f32(const int32_t *d_row_offsets, const int32_t *d_column_indices, const float *d_u, int32_t ldu, const float *d_v, int32_t ldv,
                    float *d_values_c, int32_t rows, int32_t cols, int32_t nnz, int32_t k, float alpha, float beta, mspmv_stream_t stream,
                    int debug_sync)
{
    return sddmm_impl<float, float>(d_row_offsets, d_column_indices, d_u, ldu, d_v, ldv, d_values_c, rows, cols, nnz, k, alpha, beta,
                                    reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_sddmm_f64(const int32_t *d_row_offsets, const int32_t *d_column_indices, const double *d_u, int32_t ldu, const double *d_v, int32_t ldv,
                    double *d_values_c, int32_t rows, int32_t cols, int32_t nnz, int32_t k, double alpha, double beta, mspmv_stream_t stream,
                    int debug_sync)
{
    return sddmm_impl<double, double>(d_row_offsets, d_column_indices, d_u, ldu, d_v, ldv, d_values_c, rows, cols, nnz, k, alpha, beta,
                                      reinterpret_cast<hipStream_t>(stream), debug_sync);
}
int mspmv_sddmm_bf16_f32(const int32_t *d_row_offsets, const int32_t *d_column_indices, const uint16_t *d_u, int32_t ldu, const uint16_t *d_v,
                         int32_t ldv, float *d_values_c, int32_t rows, int32_t cols, int32_t nnz, int32_t k, float alpha, float beta,
                         mspmv_stream_t stream, int debug_sync)
{
    return sddmm_impl<uint16_t, float>(d_row_offsets, d_column_indices, d_u, ldu, d_v, ldv, d_values_c, rows, cols, nnz, k, alpha, beta,
                                       reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
