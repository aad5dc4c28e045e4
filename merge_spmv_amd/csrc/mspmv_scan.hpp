// mspmv_scan.hpp -- device pieces shared by the passes that rebuild a matrix on the device (the band-major plan, mspmv_plan.hip;
// the transpose, mspmv_transpose.hip): the row of a nonzero by binary search over the row offsets, a block's row range, and the
// three-kernel exclusive scan of an int array (per-block sums, one block scanning them, per-block apply).  Nothing here waits on
// another workgroup.  Included inside an anonymous namespace of each translation unit.
#pragma once
#include <hip/hip_runtime.h>

constexpr int SCAN_BLOCK = 256, SCAN_IPT = 16, SCAN_CHUNK = SCAN_BLOCK * SCAN_IPT;

// the row holding nonzero j: the largest r in [lo, hi] with row_offsets[r] <= j
__device__ __forceinline__ int row_of(const int *__restrict__ off, int lo, int hi, int j)
{
    while (lo < hi) {
        const int mid = (int) (((long long) lo + hi + 1) >> 1);
        if (off[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// block-wide: the rows of the block's first and last nonzero (two waves search concurrently)
__device__ __forceinline__ void block_row_range(const int *__restrict__ off, int rows, int j0, int j1, int *s_range)
{
    if (threadIdx.x == 0) s_range[0] = row_of(off, 0, rows - 1, j0);
    if (threadIdx.x == 64) s_range[1] = row_of(off, 0, rows - 1, j1);
    __syncthreads();
}

// ---- exclusive scan of n ints: out[0] = 0, out[i + 1] = in[0] + ... + in[i] ------------------------------------
__device__ __forceinline__ int block_inclusive_scan(int v, int *s_tmp)      // 256 threads
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d, 64); if (lane >= d) v += u; }
    if (lane == 63) s_tmp[wave] = v;
    __syncthreads();
    int add = 0;
    for (int w = 0; w < wave; ++w) add += s_tmp[w];
    __syncthreads();
    return v + add;
}
__global__ __launch_bounds__(SCAN_BLOCK) void scan_reduce_kernel(const int *__restrict__ in, long long n, int *__restrict__ bsum)
{
    __shared__ int s_tmp[4];
    const long long base = (long long) blockIdx.x * SCAN_CHUNK + (long long) threadIdx.x * SCAN_IPT;
    int t = 0;
    for (int k = 0; k < SCAN_IPT; ++k) if (base + k < n) t += in[base + k];
    const int incl = block_inclusive_scan(t, s_tmp);
    if (threadIdx.x == SCAN_BLOCK - 1) bsum[blockIdx.x] = incl;
}
__global__ __launch_bounds__(SCAN_BLOCK) void scan_blocksums_kernel(int *__restrict__ bsum, int nblocks)
{
    __shared__ int s_tmp[4];
    __shared__ int s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += SCAN_BLOCK) {
        const int i = base + (int) threadIdx.x;
        const int v = i < nblocks ? bsum[i] : 0;
        const int incl = block_inclusive_scan(v, s_tmp);
        const int carry = s_carry;
        if (i < nblocks) bsum[i] = carry + incl - v;          // exclusive
        __syncthreads();
        if (threadIdx.x == SCAN_BLOCK - 1) s_carry = carry + incl;
        __syncthreads();
    }
}
__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(const int *__restrict__ in, long long n, const int *__restrict__ bsum,
                                                                int *__restrict__ out)
{
    __shared__ int s_tmp[4];
    const long long base = (long long) blockIdx.x * SCAN_CHUNK + (long long) threadIdx.x * SCAN_IPT;
    int v[SCAN_IPT]; int t = 0;
    for (int k = 0; k < SCAN_IPT; ++k) { v[k] = base + k < n ? in[base + k] : 0; t += v[k]; }
    int run = block_inclusive_scan(t, s_tmp) - t + bsum[blockIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
    for (int k = 0; k < SCAN_IPT; ++k) { run += v[k]; if (base + k < n) out[base + k + 1] = run; }
}
