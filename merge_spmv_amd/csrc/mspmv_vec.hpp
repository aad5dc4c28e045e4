// mspmv_vec.hpp -- the deterministic vector layer: the reduction R(.) of include/mspmv.h ("the deterministic reduction") as device
// pieces.  mspmv_vec.hip (mspmv_vec_dot_*) and mspmv_pcg.hip (the conjugate gradients' dots, fused into their vector passes) build
// their kernels from them, so both add in the one defined order.
//
// The tree.  The summands are cut into chunks of VEC_CHUNK = 1024 consecutive ones; summands the last chunk lacks are +0.0.
//   chunk sum:  lane t of 256 adds its four consecutive summands  q[t] = ((s[4t] + s[4t+1]) + s[4t+2]) + s[4t+3]  (what it holds after
//               one 16-byte load, two for fp64), then the 256 q's are added pairwise, neighbours first:  q <- q[0::2] + q[1::2],
//               eight times.  On the device that is six xor-butterfly steps inside each wave (every lane ends with the wave's sum:
//               IEEE addition is commutative, so both partners of a step compute the same bits) and (w0 + w1) + (w2 + w3) over the
//               four waves' sums through LDS.
//   level 1:    one chunk sum per chunk of the n summands: m = max(1, ceil(n / 1024)) partials (vec_chunk_sum, one workgroup each).
//   fold:       ONE workgroup (vec_fold).  If m > 1024, the partials are treated like summands once more: ceil(m / 1024) chunk sums.
//               Then ALWAYS one final chunk sum over what is left (at most 1024 values, padded with +0.0): the result.
// n <= 2^30 keeps the fold at two levels (m <= 2^20); larger n is refused.  Nothing here depends on the grid, on alignment (an
// unaligned array is read element by element into the same registers) or on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "mspmv_wave.hpp"      // Vec4, ld_stream4

#pragma clang fp contract(off)

namespace mspmv {

constexpr int VEC_CHUNK = 1024;             // summands per chunk
constexpr int VEC_BLOCK = 256;              // a chunk's workgroup: four summands per lane
constexpr int VEC_FOLD_BLOCK = 1024;        // the folding workgroup: four chunks at a time
constexpr long long VEC_MAX_N = 1LL << 30;  // (m <= 2^20 partials: the fold's second level fits LDS)

static inline long long vec_partials(long long n) { return std::max<long long>(1, (n + VEC_CHUNK - 1) / VEC_CHUNK); }

__device__ __forceinline__ bool vec_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a[i .. i + 4) of a[0 .. n), i a multiple of 4; elements at or beyond n are +0.0.  `aligned`: a is 16-byte aligned.
template <typename T>
__device__ __forceinline__ void vec_load4(const T *__restrict__ a, long long i, long long n, bool aligned, T (&v)[4])
{
    if (aligned && i + 4 <= n) {
        const Vec4<T> q = ld_stream4<false>(a + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q.get(j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < n ? a[i + j] : (T) 0;
    }
}

template <typename T>
__device__ __forceinline__ void vec_store4(T *__restrict__ a, long long i, long long n, bool aligned, const T (&v)[4])
{
    if (aligned && i + 4 <= n) {
        Vec4<T> q;
        if constexpr (sizeof(T) == 4) {
            q.v = float4v{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<float4v *>(a + i) = q.v;
        } else {
            q.a = double2v{v[0], v[1]}; q.b = double2v{v[2], v[3]};
            reinterpret_cast<double2v *>(a + i)[0] = q.a;
            reinterpret_cast<double2v *>(a + i)[1] = q.b;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < n) a[i + j] = v[j];
    }
}

template <typename T>
__device__ __forceinline__ T vec_quad(const T (&s)[4]) { return ((s[0] + s[1]) + s[2]) + s[3]; }

// six butterfly steps: every lane ends with the pairwise (neighbours first) sum of the wave's 64 values
template <typename T>
__device__ __forceinline__ T vec_wave_sum(T s)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s = s + __shfl_xor(s, d, 64);
    return s;
}

// The chunk sum of the 256 x 4 summands that the lanes of a VEC_BLOCK workgroup hold, in every thread.  s_w: 4 values of LDS.
// (Two barriers: the first ends the reads of an earlier use of s_w.)
template <typename T>
__device__ __forceinline__ T vec_chunk_sum(const T (&s)[4], T *s_w)
{
    const T w = vec_wave_sum(vec_quad(s));
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = w;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// The fold of m <= 2^20 level-1 partials (16-byte aligned), in every thread of ONE workgroup of VEC_FOLD_BLOCK threads; m is the same
// in every thread.  s_p: VEC_CHUNK values of LDS, s_w: 16.  The four groups of 256 threads each take a chunk of the partials at a
// time; with m <= 1024 they all hold the one, final chunk.
template <typename T>
__device__ __forceinline__ T vec_fold(const T *__restrict__ part, long long m, T *s_p, T *s_w)
{
    const int tid = (int) threadIdx.x, g = tid >> 8, t = tid & 255;
    const int chunks = (int) ((m + VEC_CHUNK - 1) / VEC_CHUNK);
    T v[4];
    if (chunks <= 1) {
        vec_load4(part, 4ll * t, m, true, v);
    } else {
        for (int base = 0; base < chunks; base += 4) {
            const int c = base + g;                                  // (a group beyond the last chunk adds zeros and stores nothing)
            vec_load4(part, (long long) c * VEC_CHUNK + 4ll * t, m, true, v);
            const T w = vec_wave_sum(vec_quad(v));
            __syncthreads();
            if ((tid & 63) == 0) s_w[tid >> 6] = w;
            __syncthreads();
            if (t == 0 && c < chunks) s_p[c] = (s_w[4 * g] + s_w[4 * g + 1]) + (s_w[4 * g + 2] + s_w[4 * g + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 4 * t + j < chunks ? s_p[4 * t + j] : (T) 0;
    }
    const T w = vec_wave_sum(vec_quad(v));
    __syncthreads();
    if ((tid & 63) == 0) s_w[tid >> 6] = w;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);                    // (the waves of group 0; the other groups hold the same)
}

}  // namespace mspmv
