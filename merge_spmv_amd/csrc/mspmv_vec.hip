// mspmv_vec.hip -- mspmv_vec_dot_* of include/mspmv.h: the dot product of two device vectors, ONE value left ON THE DEVICE, added in the
// defined order of mspmv_vec.hpp.  Two launches, ordered by the kernel boundary alone: one workgroup per chunk of 1024 products writes
// the chunk's sum to temp storage; one workgroup folds them.  No atomics, nothing read back, nothing allocated.
#include <hip/hip_runtime.h>

#include "../../include/mspmv.h"
#include "mspmv_levels.hpp"     // lv_launched
#include "mspmv_vec.hpp"

#pragma clang fp contract(off)

namespace {

using namespace mspmv;

template <typename T>
__global__ __launch_bounds__(VEC_BLOCK) void vec_dot_kernel(const T *__restrict__ a, const T *__restrict__ b, long long n, T *__restrict__ part)
{
    __shared__ T s_w[4];
    const long long i = (long long) blockIdx.x * VEC_CHUNK + 4ll * threadIdx.x;
    T va[4], vb[4], s[4];
    vec_load4(a, i, n, vec_aligned16(a), va);
    vec_load4(b, i, n, vec_aligned16(b), vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = va[j] * vb[j];               // (absent elements are +0.0: so are their products)
    const T sum = vec_chunk_sum(s, s_w);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

template <typename T>
__global__ __launch_bounds__(VEC_FOLD_BLOCK) void vec_fold_kernel(const T *__restrict__ part, long long m, T *__restrict__ result)
{
    __shared__ T s_p[VEC_CHUNK];
    __shared__ T s_w[16];
    const T sum = vec_fold(part, m, s_p, s_w);
    if (threadIdx.x == 0) *result = sum;
}

template <typename T>
int vec_dot(void *d_temp, size_t *temp_bytes, const T *a, const T *b, int64_t n, T *result, hipStream_t stream, int debug_sync)
{
    if (!temp_bytes || n < 0 || n > VEC_MAX_N) return hipErrorInvalidValue;
    const long long m = vec_partials(n);
    const size_t need = ((size_t) m * sizeof(T) + 15) & ~size_t(15);
    if (!d_temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need || (reinterpret_cast<uintptr_t>(d_temp) & 15) != 0) return hipErrorInvalidValue;
    if (!result || (n > 0 && (!a || !b))) return hipErrorInvalidValue;
    T *part = static_cast<T *>(d_temp);
    hipLaunchKernelGGL(vec_dot_kernel<T>, dim3((unsigned) m), dim3(VEC_BLOCK), 0, stream, a, b, (long long) n, part);
    if (int e = lv_launched(stream, debug_sync, "vec_dot_kernel", (unsigned) m, VEC_BLOCK)) return e;
    hipLaunchKernelGGL(vec_fold_kernel<T>, dim3(1), dim3(VEC_FOLD_BLOCK), 0, stream, part, m, result);
    return lv_launched(stream, debug_sync, "vec_fold_kernel", 1, VEC_FOLD_BLOCK);
}

}  // namespace

extern "C" {

int mspmv_vec_dot_f32(void *d_temp, size_t *temp_bytes, const float *d_a, const float *d_b, int64_t n, float *d_result,
                      mspmv_stream_t stream, int debug_sync)
{
    return vec_dot<float>(d_temp, temp_bytes, d_a, d_b, n, d_result, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

int mspmv_vec_dot_f64(void *d_temp, size_t *temp_bytes, const double *d_a, const double *d_b, int64_t n, double *d_result,
                      mspmv_stream_t stream, int debug_sync)
{
    return vec_dot<double>(d_temp, temp_bytes, d_a, d_b, n, d_result, reinterpret_cast<hipStream_t>(stream), debug_sync);
}

}  // extern "C"
