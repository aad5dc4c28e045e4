// mspmv_wave.hpp -- wave primitives (DPP segmented scan, block reduce-by-key) and the streaming loads (Vec4, widen, ld_stream4*).
#pragma once
#include "mspmv_coords.hpp"

namespace mspmv {

// ---------------------------------------------------------------------------
// wave64 inclusive segmented (reduce-by-key) scan over one (key, value) pair
// per lane.  Keys are non-decreasing across lanes (rows along the merge
// path), so "same key" == "same segment"; the combine is the reference's
// ReduceByKeyOp<Sum> (thread_operators.cuh:291-301).
// ---------------------------------------------------------------------------
// Data-parallel-primitive (DPP) moves: cross-lane operands delivered inside the VALU
// instead of through the LDS crossbar (__shfl_up lowers to ds_bpermute_b32, ~100 cycles
// of dependent latency per step; a DPP move costs a VALU slot).  Lanes that receive
// nothing (out of the row for row_shr, rows masked off for the broadcasts) keep `old`.
//   row_shr:n   = 0x110 + n   shift right by n inside each row of 16 lanes
//   row_bcast15 = 0x142       lane 15 of each row -> all lanes of the next row
//   row_bcast31 = 0x143       lane 31 -> lanes 32..63
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_move(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float old, float src)
{
    return __builtin_bit_cast(float, dpp_move<CTRL, ROW_MASK>(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double old, double src)
{
    const long long o = __builtin_bit_cast(long long, old), v = __builtin_bit_cast(long long, src);
    const int lo = dpp_move<CTRL, ROW_MASK>((int) o, (int) v);
    const int hi = dpp_move<CTRL, ROW_MASK>((int) (o >> 32), (int) (v >> 32));
    return __builtin_bit_cast(double, ((long long) hi << 32) | (unsigned) lo);
}

template <typename V, int CTRL, int ROW_MASK>
__device__ __forceinline__ void rbk_step(int key, V &val)
{
    const int k2 = dpp_move<CTRL, ROW_MASK>(-1, key);       // -1: "no source lane", never equals a key
    const V v2 = dpp_move<CTRL, ROW_MASK>((V) 0, val);
    val += k2 == key ? v2 : (V) 0;
}

template <typename V>
__device__ __forceinline__ V wave_segmented_inclusive_sum(int key, V val)
{
    // keys are >= 0 and non-decreasing across lanes: equal key == same segment
    rbk_step<V, 0x111, 0xf>(key, val);      // row_shr:1
    rbk_step<V, 0x112, 0xf>(key, val);      // row_shr:2
    rbk_step<V, 0x114, 0xf>(key, val);      // row_shr:4
    rbk_step<V, 0x118, 0xf>(key, val);      // row_shr:8   -> inclusive within each 16-lane row
    rbk_step<V, 0x142, 0xa>(key, val);      // row_bcast15 into rows 1 and 3
    rbk_step<V, 0x143, 0xc>(key, val);      // row_bcast31 into rows 2 and 3
    return val;
}

// Block-wide exclusive reduce-by-key scan of one pair per thread.
//   in : (key, val) of this thread, keys non-decreasing with threadIdx.x
//   out: carry_in  = sum of val over preceding threads whose key equals the
//                    key of the thread just before this one, restricted to
//                    that trailing equal-key run (0 for thread 0);
//        returns the block aggregate (key, sum) in agg_* for the LAST thread.
// s_wave_key/s_wave_val: LDS scratch, one slot per wave.
template <typename V, int BLOCK>
__device__ __forceinline__ void block_exclusive_rbk(int key, V val, int *s_wave_key, V *s_wave_val,
                                                    int &prev_key, V &carry_in, int &agg_key, V &agg_val)
{
    constexpr int NW = BLOCK / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const V incl = wave_segmented_inclusive_sum<V>(key, val);
    if (lane == WAVE - 1) { s_wave_key[wave] = key; s_wave_val[wave] = incl; }
    __syncthreads();
    // fold the aggregates of the preceding waves, in order
    int pk = -1; V pv = 0; bool have = false;
#pragma unroll
    for (int w = 0; w < NW - 1; ++w) {
        if (w < wave) {
            const int k = s_wave_key[w]; const V v = s_wave_val[w];
            pv = (have && pk == k) ? pv + v : v; pk = k; have = true;
        }
    }
    // exclusive within the wave
    int ek = __shfl_up(key, 1, WAVE);
    V ev = __shfl_up(incl, 1, WAVE);
    if (lane == 0) { prev_key = pk; carry_in = have ? pv : (V) 0; }
    else { prev_key = ek; carry_in = (have && pk == ek) ? pv + ev : ev; }
    // aggregate as seen by this thread (meaningful for the last thread)
    agg_key = key; agg_val = (have && pk == key) ? pv + incl : incl;
}

// ---------------------------------------------------------------------------
// Streaming loads.  The nonzero arrays and the row offsets are read exactly
// once per SpMV: load them non-temporally so they do not evict x from the
// XCD's 4 MiB L2 (measured: -7 % time on the 12.5 MB-x gather), 16 bytes per
// lane (a dword-per-lane stream tops out at 4.0 TB/s on MI355X, 16 B/lane at
// 6.4 TB/s).
// ---------------------------------------------------------------------------
// NT = false: ordinary loads.  A matrix that fits the 256 MB Infinity Cache stays there
// between SpMVs of an iterative solver when it is read with ordinary loads (measured +9-10 %
// at 58 MB and 272 MB), while for larger matrices the non-temporal form wins (+3-6 %): the
// dispatcher picks per call from the matrix's byte size.
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p) { return NT ? __builtin_nontemporal_load(p) : *p; }

template <typename T> struct Vec4;
template <> struct Vec4<int> { int4v v; __device__ __forceinline__ int get(int i) const { return v[i]; } };
template <> struct Vec4<float> { float4v v; __device__ __forceinline__ float get(int i) const { return v[i]; } };
template <> struct Vec4<double> { double2v a, b; __device__ __forceinline__ double get(int i) const { return i < 2 ? a[i] : b[i - 2]; } };

template <> struct Vec4<bf16> {
    int2v v;
    __device__ __forceinline__ bf16 get(int i) const { bf16 r; r.bits = (unsigned short) ((unsigned) v[i >> 1] >> (16 * (i & 1))); return r; }
};
// matrix value -> compute type: exact (every fp32 is an fp64, every bf16 an fp32), so a mixed call's products are those of the widened matrix
template <typename V> __device__ __forceinline__ V widen(V v) { return v; }
template <typename V> __device__ __forceinline__ V widen(bf16 v) { return __builtin_bit_cast(float, (unsigned) v.bits << 16); }
template <typename V, typename = typename std::enable_if<sizeof(V) == 8>::type> __device__ __forceinline__ V widen(float v) { return (V) v; }

template <bool NT>
__device__ __forceinline__ bf16 ld_stream(const bf16 *p) { bf16 r; r.bits = ld_stream<NT>(&p->bits); return r; }
template <bool NT>
__device__ __forceinline__ Vec4<bf16> ld_stream4(const bf16 *p)       // 8 bytes per chunk
{
    Vec4<bf16> r; const int2v *q = reinterpret_cast<const int2v *>(p);
    r.v = NT ? __builtin_nontemporal_load(q) : *q; return r;
}
template <bool NT>
__device__ __forceinline__ Vec4<int> ld_stream4(const int *p)
{
    Vec4<int> r; const int4v *q = reinterpret_cast<const int4v *>(p);
    r.v = NT ? __builtin_nontemporal_load(q) : *q; return r;
}
template <bool NT>
__device__ __forceinline__ Vec4<float> ld_stream4(const float *p)
{
    Vec4<float> r; const float4v *q = reinterpret_cast<const float4v *>(p);
    r.v = NT ? __builtin_nontemporal_load(q) : *q; return r;
}
template <bool NT>
__device__ __forceinline__ Vec4<double> ld_stream4(const double *p)
{
    Vec4<double> r; const double2v *q = reinterpret_cast<const double2v *>(p);
    r.a = NT ? __builtin_nontemporal_load(q) : q[0];
    r.b = NT ? __builtin_nontemporal_load(q + 1) : q[1];
    return r;
}
__device__ __forceinline__ void zero4(Vec4<float> &r) { r.v = float4v{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void zero4(Vec4<double> &r) { r.a = double2v{0.0, 0.0}; r.b = r.a; }
__device__ __forceinline__ void st_lds4(float *p, const float (&v)[4])
{ float4v w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3]; *reinterpret_cast<float4v *>(p) = w; }
__device__ __forceinline__ void st_lds4(double *p, const double (&v)[4])
{
    double2v a, b; a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
    *reinterpret_cast<double2v *>(p) = a; *(reinterpret_cast<double2v *>(p) + 1) = b;
}
__device__ __forceinline__ void st_lds4(int *p, const int (&v)[4])
{ int4v w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3]; *reinterpret_cast<int4v *>(p) = w; }
// Tile-relative row ends as the flag/scan reduction keeps them: 16 bits each (a tile has < 65536
// nonzeros; entries of rows outside the tile are never read, so truncating them is harmless).
// LDS is what limits the resident blocks per CU, and residency is worth more than anything else
// here: 6 KB per 256x11 tile.
typedef unsigned short end16_t;
__device__ __forceinline__ void st_lds4(end16_t *p, const int (&v)[4])
{
    int2v w;
    w.x = (v[0] & 0xffff) | (v[1] << 16);
    w.y = (v[2] & 0xffff) | (v[3] << 16);
    *reinterpret_cast<int2v *>(p) = w;
}
template <bool FL> struct EndType { typedef int type; };
template <> struct EndType<true> { typedef end16_t type; };

// LDS index swizzle of the staged products.  Thread t of the walk reads products around index
// t*IPT - (rows before it); when rows have a regular length the per-lane stride resonates with
// the 32 banks (dense 32-nnz rows, IPT = 11: lanes l, l+3, l+6 ... hit one bank, an 11-way
// conflict: SQ_LDS_BANK_CONFLICT was 56 % of all LDS cycles).  XOR-ing index bits 2..4 with
// bits 5..7 keeps every 4-element chunk contiguous and 16-byte aligned (the staging writes
// whole chunks) and moves indices 32 apart to different banks.
__device__ __forceinline__ int swz_prod(int i) { return i ^ (((i >> 5) & 7) << 2); }

}  // namespace mspmv
