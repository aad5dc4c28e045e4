// mspmv_stage.hpp -- how a tile gets into LDS: tile_kernel (dword per lane, the fallback kernel, whole), then the 16-byte staging
// of every other tile kernel: tile_waves_per_simd, TileRegs, issue_nonzero_loads, stage_tile*, a tiny x in LDS, the block -> tile maps.
#pragma once
#include "mspmv_reduce.hpp"

namespace mspmv {

// ---------------------------------------------------------------------------
// One block per tile, dword-per-lane staging: the fallback for CSR arrays
// whose base addresses are not 16-byte aligned and for tiny matrices.
// ref: DeviceSpmvKernel / AgentSpmv::ConsumeTile, dispatch_spmv_orig.cuh:157-186,
// agent_spmv_orig.cuh:413-639,856-914.
// ---------------------------------------------------------------------------
template <typename V, int BLOCK, int IPT, typename OUT, typename MV = V>
__global__ __launch_bounds__(BLOCK) void tile_kernel(Params<V, MV> p, const Coord *__restrict__ coords,
                                                     Carry<V> *__restrict__ carries, int num_tiles)
{
    constexpr bool AXPBY = OUT::AXPBY;
    constexpr int TILE = BLOCK * IPT;
    constexpr int NW = BLOCK / WAVE;
    constexpr int PAD = IPT + 4;
    __shared__ int s_end[TILE + PAD];
    __shared__ V s_prod[TILE + PAD];
    __shared__ int s_wave_key[NW];
    __shared__ V s_wave_val[NW];

    const int tile = blockIdx.x;
    const int tid = threadIdx.x;
    const Coord c0 = coords[tile];
    const Coord c1 = coords[tile + 1];
    const int tile_rows = c1.x - c0.x;
    const int tile_nnz = c1.y - c0.y;

    const int *__restrict__ cols = p.cols + c0.y;
    const MV *__restrict__ vals = p.values + c0.y;
    int col_r[IPT];
    MV val_r[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = tid + k * BLOCK;
        if (j < tile_nnz) { col_r[k] = cols[j]; val_r[k] = vals[j]; }
    }
    const int *__restrict__ row_end = p.row_end + c0.x;
    for (int r = tid; r < TILE + PAD; r += BLOCK) s_end[r] = r < tile_rows ? row_end[r] - c0.y : 0x3fffffff;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = tid + k * BLOCK;
        s_prod[j] = j < tile_nnz ? widen<V>(val_r[k]) * p.x[col_r[k]] : (V) 0;
    }
    if (tid < PAD) s_prod[TILE + tid] = (V) 0;
    __syncthreads();
    consume_tile_lds<V, BLOCK, IPT, AXPBY>(p, c0, tile_rows, tile_nnz, s_end, s_prod, s_prod, s_wave_key, s_wave_val,
                                           carries + tile);
}

// ---------------------------------------------------------------------------
// The production kernel: 16-byte streaming loads, LDS-staged products, flag/segmented-scan
// reduction (consume_tile_flags).  PERSIST = false (default): one tile per block; the
// hardware's block scheduler balances the load and de-phases the blocks of a CU.
// PERSIST = true (tuning flags): a block walks tiles blockIdx.x, +gridDim.x, ... and requests
// the NEXT tile's nonzeros (into the registers the current tile has just drained into LDS)
// before the LDS phases of the current one.  The persistent form was the faster one while the
// in-tile reduction was the per-thread path walk; measured with the present reduction a resident
// grid is 7-10 % slower on streaming matrices and 2-4 tiles per block are within +-3 % of one
// (tools/sweep.py with SWEEP_FLAGS=0x100000..0x800000), so the simpler launch is the default.
// What bounds the kernel is the CU's vector-memory pipeline: cycle stamps (tools/trace_tiles.py)
// show ~70 % of a block's life spent issuing into / waiting on it, and throughput follows the
// number of cache lines requested per tile, not the instruction count of the LDS phases.
//
// Staging works on 4-element chunks aligned in ARRAY index space (the CSR
// arrays are 16-byte aligned -- checked by the dispatcher -- but a tile starts
// anywhere): chunk addresses are clamped to the last full chunk of the array
// instead of being branched around, so every load is unconditional,
// straight-line code (a branch per chunk made hipcc wait for each load before
// issuing the next); elements outside the tile are predicated off, and the
// <= 3 elements of a ragged array tail are read by scalar loads in a rarely
// taken branch.  Nothing outside [0,nnz) / [0,rows] is ever read.
// ---------------------------------------------------------------------------
// Resident blocks per CU the vectorised tile kernels are compiled for: what their LDS
// footprint admits (160 KiB per CU), at most 32 waves per CU.  Passed to __launch_bounds__ as
// waves per SIMD: left alone, hipcc spent 92-104 VGPRs on these kernels (4-5 waves/SIMD); told
// the target it fits 64-80 without spilling, which is what actually sets the residency.
template <typename V, int BLOCK, int IPT, bool WIDE_ENDS = false>
constexpr int tile_blocks_per_cu()
{
    constexpr int slots = (IPT / 4 + 1) * BLOCK * 4;
    constexpr int lds = slots * ((WIDE_ENDS ? 4 : 2) + (int) sizeof(V)) + slots / 8 + 256;      // products, row ends (16-bit; 32 for the walk), flag bits
    constexpr int by_lds = 163840 / lds;
    constexpr int by_waves = 2048 / BLOCK;
    return by_lds < by_waves ? (by_lds < 1 ? 1 : by_lds) : by_waves;
}
template <typename V, int BLOCK, int IPT, bool RELAX = false, bool WIDE_ENDS = false>
constexpr int tile_waves_per_simd()
{
    // one wave less than the LDS footprint admits (never more than 6 for fp64): with both
    // staging paths in the kernel the tighter budget spills 3 registers per lane, and the
    // measured difference between the two choices is within noise
    int w = (tile_blocks_per_cu<V, BLOCK, IPT, WIDE_ENDS>() * BLOCK + 255) / 256;
    if (sizeof(V) == 8 && w > 6) w = 6;
    if (w > 4 && (!RELAX || WIDE_ENDS)) w -= WIDE_ENDS && w > 5 ? 2 : 1;
    return w;
}

// Column-band passes, fp64: the values of a chunk are fetched only when one of its four columns lies in the pass's band
// (with sorted columns a band's nonzeros are a run inside each row: C2 fp64 skips 57 % of the 32-byte value loads per pass,
// 1.447 -> 1.342 ms).  Not for fp32: the extra live state spills there (0.87 -> 0.95 ms, and the scratch set-up costs the
// ordinary body of the same kernel 20 %).
template <typename V, bool BAND> constexpr bool band_lazy_values() { return BAND && sizeof(V) == 8; }

template <typename V, int BLOCK, int IPT, typename MV = V>
struct TileRegs {
    static constexpr int CPT = IPT / 4 + 1;   // 4-element chunks per thread: covers TILE + 3
    Vec4<int> col[CPT];
    Vec4<MV> val[CPT];                        // as stored: 16 bytes (fp32), 32 (fp64) or 8 (bf16) per chunk
};

// fp64 values of a 4-element chunk are 32 bytes: fetched as two 16-byte loads per lane, each load instruction of a wave would
// touch every 128-byte line of the wave's 2 KB twice, half a line at a time -- and the second touch of a line read with a
// non-temporal load is another request to L2 (measured: making the second half an ordinary load, which then hits the CU's
// cache, is worth 5-9 % on dense32 / 7-point-grid streams, but gives the lines ordinary retention and costs the
// gather-bound matrices 2-3 % of their x hits).  Instead the two loads are laid out line by line: in the first, lanes 0-31
// fetch the first half of their own chunk and lanes 32-63 the SECOND half of the chunk of lane - 32 (8 whole lines); in the
// second, lanes 0-31 fetch the first half of the chunk of lane + 32 and lanes 32-63 their own second half; four
// v_permlane32_swap (gfx950) then hand every lane its own 32 bytes.  Wave-uniform control flow required.
// (The swaps are a separate step, linewise_own, done by the staging right before the products: next to the loads the compiler
//  waits for each pair before it requests the next one.)
template <bool NT>
__device__ __forceinline__ Vec4<double> ld_stream4_linewise(const double *base, int e_own, int e_partner, int tid)
{
    const bool hi = (tid & 32) != 0;
    const double2v *pa = reinterpret_cast<const double2v *>(base + (hi ? e_partner + 2 : e_own));
    const double2v *pb = reinterpret_cast<const double2v *>(base + (hi ? e_own + 2 : e_partner));
    Vec4<double> r;
    r.a = NT ? __builtin_nontemporal_load(pa) : *pa;
    r.b = NT ? __builtin_nontemporal_load(pb) : *pb;
    return r;
}
// what ld_stream4_linewise fetched -> every lane's own four values.  Wave-uniform control flow required.
__device__ __forceinline__ Vec4<double> linewise_own(const Vec4<double> &w)
{
    typedef unsigned uint4v __attribute__((ext_vector_type(4)));
    uint4v ua = __builtin_bit_cast(uint4v, w.a), ub = __builtin_bit_cast(uint4v, w.b);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        // lanes 32-63 of the first operand <-> lanes 0-31 of the second
        const auto sw = __builtin_amdgcn_permlane32_swap(ua[d], ub[d], false, false);
        ua[d] = sw[0]; ub[d] = sw[1];
    }
    Vec4<double> r; r.a = __builtin_bit_cast(double2v, ua); r.b = __builtin_bit_cast(double2v, ub);
    return r;
}
__device__ __forceinline__ Vec4<float> linewise_own(const Vec4<float> &w) { return w; }
__device__ __forceinline__ Vec4<bf16> linewise_own(const Vec4<bf16> &w) { return w; }
// values as issue_nonzero_loads left them in the tile's registers -> the values of the lane's own chunk k
// (MV: 8-byte STORED values only -- fp32 values of an fp64 product are one 16-byte load per chunk, the fp32 path's)
template <typename V, bool NT, bool LAZY, typename MV = V>
constexpr bool vals_linewise() { return sizeof(MV) == 8 && NT && !LAZY; }
// WIRE staging (the production kernels): the values stay as ld_stream4_linewise fetched them -- val.a = the first half of the own chunk
// (lanes 0-31) / the second half of the chunk 32 lanes down (lanes 32-63), val.b = the first half of the chunk 32 lanes up / the own
// second half -- and the COLUMNS are swapped to match (two v_permlane32_swap instead of four): every lane then multiplies two pairs that
// belong to two different chunks, and writes each pair where it belongs in the LDS tile.  Lanes 0-31 and 32-63 of one store
// instruction together cover 1 KB of consecutive 16-byte units (a lane writing its own 32 bytes as two stores 32 bytes apart
// collided two-way with the lane four further on).  cols[0..1] belong to val.a, cols[2..3] to val.b.
__device__ __forceinline__ void wire_cols(const Vec4<int> &col, int (&c)[4])
{
    const auto s0 = __builtin_amdgcn_permlane32_swap((unsigned) col.v.x, (unsigned) col.v.z, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap((unsigned) col.v.y, (unsigned) col.v.w, false, false);
    c[0] = (int) s0[0]; c[1] = (int) s1[0]; c[2] = (int) s0[1]; c[3] = (int) s1[1];
}
// chunk index (in units of 4 elements, relative to the tile's first chunk) and element offset inside it of the pair in val.a / val.b
struct WirePos { int qa, qb, off; };
__device__ __forceinline__ WirePos wire_pos(int q, int tid)
{
    const bool hi = (tid & 32) != 0;
    WirePos w; w.qa = hi ? q - 32 : q; w.qb = hi ? q : q + 32; w.off = hi ? 2 : 0;
    return w;
}

// (A wave-uniform skip of chunks that lie past the tile altogether -- one or two of the four waves of a short-row tile -- was built for
//  the interior staging in round 5 and not kept: every branch around a group of loads makes the compiler wait at the join, and the
//  result was mixed -- grid3d-200 -2.3 %, band5 -3 %, but the circuit-shaped matrix +8 %, dense32 fp64 +3.5 %, dense5 +2 %:
//  profiles/r05_ab_wave_skip_general_kernel.txt.  The compact front end, whose loads are few and whose tiles share a CU in small
//  numbers, keeps it.)
template <typename V, int BLOCK, int IPT, bool NT, bool VALS = true, bool LINEWISE_OK = true, typename MV = V>
__device__ __forceinline__ void issue_nonzero_loads(const Params<V, MV> &p, const Coord c0, const Coord c1,
                                                    TileRegs<V, BLOCK, IPT, MV> &r, int tid_in = -1)
{
    const int tid = tid_in < 0 ? (int) threadIdx.x : tid_in;
    constexpr int CPT = IPT / 4 + 1;
    const int a0 = c0.y & ~3;
    const int last_full = (p.nnz & ~3) - 4;        // first element of the array's last full chunk (nnz >= 4)
    const int safe = a0 < last_full ? a0 : last_full;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        int e0 = a0 + 4 * (tid + k * BLOCK);
        // a chunk past the tile (it belongs to the next tile) or past the last full chunk of
        // the array is not fetched: those lanes re-read the tile's first chunk instead (one
        // cached address), so no byte of HBM traffic is spent on data this tile does not use
        e0 = (e0 < c1.y && e0 <= last_full) ? e0 : safe;
        r.col[k] = ld_stream4<NT>(p.cols + e0);
        if constexpr (VALS && LINEWISE_OK && vals_linewise<V, NT, false, MV>()) {     // (ordinary loads: the second half hits the CU's cache anyway, and the swaps cost 3 % on dense5)
            int e1 = a0 + 4 * ((tid ^ 32) + k * BLOCK);          // the chunk of the lane 32 away, by the same rule
            e1 = (e1 < c1.y && e1 <= last_full) ? e1 : safe;
            r.val[k] = ld_stream4_linewise<NT>(p.values, e0, e1, tid);
        } else if constexpr (VALS) r.val[k] = ld_stream4<NT>(p.values + e0);      // (!VALS: column-band passes fetch the values later, by band)
    }
}

// Stage one tile whose nonzeros are already in `regs` (requested earlier): row offsets
// and x gathers are issued, tile-relative row ends and products land in LDS (every slot of
// both arrays is written: +inf / 0 outside the tile), the ragged array tails are patched,
// and the block is synchronised.
// (after_gather: called once the x gathers have been requested -- scalar work of the caller that then runs in the shadow of their
//  latency instead of after the staging barrier: the hint verdict of tile_kernel_snap)
struct NoAfterGather { __device__ __forceinline__ void operator()() const {} };
template <typename V, int BLOCK, int IPT, bool NT, bool FL, bool XL = false, bool BAND = false, typename AG = NoAfterGather, typename MV = V>
__device__ __forceinline__ void stage_tile_careful(const Params<V, MV> &p, const Coord c0, const Coord c1,
                                           const TileRegs<V, BLOCK, IPT, MV> &regs, typename EndType<FL>::type *s_end_raw, V *s_prod_raw,
                                           int last_full_nz, int last_full_ro, unsigned *s_flag, const V *s_x = nullptr, int tid_in = -1,
                                           bool lean = false, AG after_gather = AG())
{
    // lean (block-uniform; FL only): the tile will be reduced row by row (consume_tile_rows) -- no row-start bits, products at their raw positions
    constexpr int CPT = IPT / 4 + 1;
    const int tid = tid_in < 0 ? (int) threadIdx.x : tid_in;
    const int *__restrict__ row_offsets = p.row_end - 1;
    const int tile_rows = c1.x - c0.x;
    const int tile_nnz = c1.y - c0.y;
    const int a0 = c0.y & ~3;
    const int first = c0.x + 1;                // d_row_offsets index of the tile's first row end
    const int i0 = first & ~3;
    const int eshift = first - i0;
    // ---- row ends of the current tile -> LDS (chunks of d_row_offsets)
    Vec4<int> ro[CPT];
    const int ro_chunks = (tile_rows + eshift + 3) / 4;           // chunks holding a row end of this tile
    const int ro_safe = i0 < last_full_ro ? i0 : last_full_ro;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int q = tid + k * BLOCK;
        int i = i0 + 4 * q;
        i = (q < ro_chunks && i <= last_full_ro) ? i : ro_safe;
        ro[k] = ld_stream4<NT>(row_offsets + i);
    }
    // ---- gather x for the current tile (its nonzeros were requested one iteration ago)
    V xv[CPT][4];
    unsigned in_band = 0u;                     // BAND: one bit per staged nonzero of this thread (its column lies in the pass's band)
    constexpr bool LAZY = band_lazy_values<V, BAND>();
    Vec4<MV> bval[LAZY ? CPT : 1];              // LAZY: the values, fetched here and only for chunks with a nonzero of the band
    constexpr bool WIRE = vals_linewise<V, NT, LAZY, MV>() && FL;
    unsigned wire_in = 0u;                     // WIRE: one bit per held nonzero that lies in the tile
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e0 = a0 + 4 * (tid + k * BLOCK);
        if constexpr (WIRE) {
            int gc[4]; wire_cols(regs.col[k], gc);
            const WirePos wp = wire_pos(tid + k * BLOCK, tid);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int eb = a0 + 4 * (i < 2 ? wp.qa : wp.qb);             // first element of the chunk this value belongs to
                const bool in = (unsigned) (eb + wp.off + (i & 1) - c0.y) < (unsigned) tile_nnz && eb <= last_full_nz;
                wire_in |= in ? 1u << (4 * k + i) : 0u;
                xv[k][i] = XL ? s_x[in ? gc[i] : 0] : p.x[in ? gc[i] : 0];
            }
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = (unsigned) (e0 + i - c0.y) < (unsigned) tile_nnz && e0 <= last_full_nz;
            if (BAND) {
                xv[k][i] = (V) 0;
                if (in && (unsigned) (regs.col[k].get(i) - p.band_lo) < (unsigned) p.band_len) { xv[k][i] = p.x[regs.col[k].get(i)]; in_band |= 1u << (4 * k + i); }
            } else xv[k][i] = XL ? s_x[in ? regs.col[k].get(i) : 0] : p.x[in ? regs.col[k].get(i) : 0];
        }
        if constexpr (LAZY) {
            zero4(bval[k]);
            if ((in_band >> (4 * k)) & 0xfu) bval[k] = ld_stream4<NT>(p.values + e0);     // (a bit set => a chunk of this tile, <= last_full_nz)
        }
    }
    after_gather();
    // ---- stage row ends
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int q = tid + k * BLOCK;
        const int i = i0 + 4 * q;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 4 * q - eshift + j;
            const bool in = r >= 0 && r < tile_rows && i <= last_full_ro;
            v[j] = in ? ro[k].get(j) - c0.y : 0x3fffffff;
            if (FL && !lean && (unsigned) v[j] < (unsigned) tile_nnz) {
                const int b = (c0.y - a0) + v[j];
                atomicOr(&s_flag[b >> 5], 1u << (b & 31));
            }
        }
        st_lds4(&s_end_raw[4 * q], v);
    }
    if (FL && !lean && tid == 0) atomicOr(&s_flag[0], 1u << (c0.y - a0));
    // ---- stage products
    Vec4<MV> own_val[LAZY || WIRE ? 1 : CPT];
    if constexpr (!LAZY && !WIRE) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) own_val[k] = vals_linewise<V, NT, LAZY, MV>() ? linewise_own(regs.val[k]) : regs.val[k];
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int chunk = tid + k * BLOCK;
        const int e0 = a0 + 4 * chunk;
        if constexpr (WIRE) {
            const WirePos wp = wire_pos(chunk, tid);
            const V w[4] = {regs.val[k].get(0), regs.val[k].get(1), regs.val[k].get(2), regs.val[k].get(3)};
            V pa[2], pb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                pa[i] = ((wire_in >> (4 * k + i)) & 1u) ? w[i] * xv[k][i] : (V) 0;
                pb[i] = ((wire_in >> (4 * k + 2 + i)) & 1u) ? w[2 + i] * xv[k][2 + i] : (V) 0;
            }
            st_unit(&s_prod_raw[2 * prod_unit<V, CPT>(2 * wp.qa + (wp.off >> 1), lean)], pa);
            st_unit(&s_prod_raw[2 * prod_unit<V, CPT>(2 * wp.qb + (wp.off >> 1), lean)], pb);
            continue;
        }
        V prod[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = BAND ? ((in_band >> (4 * k + i)) & 1u) != 0u
                                 : (unsigned) (e0 + i - c0.y) < (unsigned) tile_nnz && e0 <= last_full_nz;
            if constexpr (LAZY) prod[i] = in ? bval[k].get(i) * xv[k][i] : (V) 0;
            else prod[i] = in ? widen<V>(own_val[k].get(i)) * xv[k][i] : (V) 0;
        }
        if (FL) st_prod_chunk<CPT>(s_prod_raw, chunk, prod, lean);
        else st_lds4(&s_prod_raw[swz_prod(4 * chunk)], prod);
    }
    // ---- ragged array tails (at most 3 elements each; only the tile that reaches the array
    //      end).  Block-uniform branch; the barrier orders these writes after the zeros /
    //      sentinels the chunk owners stored into the same slots above.
    const bool nz_tail = c1.y > last_full_nz + 4;
    const bool ro_tail = first + tile_rows > last_full_ro + 4;
    if (nz_tail || ro_tail) {
        __syncthreads();
        const int j = last_full_nz + 4 + tid;                       // absolute nonzero index
        if (nz_tail && j < c1.y && j >= c0.y) {
            const int c = ld_stream<NT>(p.cols + j);
            const bool inb = !BAND || (unsigned) (c - p.band_lo) < (unsigned) p.band_len;
            s_prod_raw[FL ? prod_slot<V, CPT>(j - a0, lean) : swz_prod(j - a0)] = inb ? widen<V>(ld_stream<NT>(p.values + j)) * (XL ? s_x[c] : p.x[c]) : (V) 0;
        }
        const int i = last_full_ro + 4 + tid;                       // absolute d_row_offsets index
        const int r = i - first;
        if (ro_tail && r >= 0 && r < tile_rows) {
            const int v = ld_stream<NT>(row_offsets + i) - c0.y;
            s_end_raw[r + eshift] = (typename EndType<FL>::type) v;
            if (FL && !lean && (unsigned) v < (unsigned) tile_nnz) atomicOr(&s_flag[((c0.y - a0) + v) >> 5], 1u << (((c0.y - a0) + v) & 31));
        }
    }
    __syncthreads();
}

// Interior tiles (all but the handful whose chunk loads would touch the last, ragged chunk of
// an array -- the matrix's final tile in particular): no per-element predicates at all.
//  * every column index in a loaded chunk is a valid index even when the element belongs to
//    the neighbouring tile, so x is gathered unconditionally;
//  * products of elements outside the tile land in LDS slots the walk never reads as
//    nonzeros (an item past the tile's nonzeros is always a row end there, and a row end's
//    product slot is read but discarded by a select, so even a NaN cannot leak);
//  * row offsets past the tile's last row are REAL offsets (>= the tile's nonzero count), which
//    serve as the "+inf" the search and the walk need: a row end of a later tile lies at
//    least IPT path items past every thread of a full tile.
// Only whole chunks beyond the needed range are redirected to a cached address (no HBM bytes
// for data the tile does not use).  This removes ~200 of the ~1100 instructions per wave per tile.
template <typename V, int BLOCK, int IPT, bool NT, bool FL, bool XL = false, bool BAND = false, typename AG = NoAfterGather, typename MV = V>
__device__ __forceinline__ void stage_tile_interior(const Params<V, MV> &p, const Coord c0, const Coord c1,
                                                    const TileRegs<V, BLOCK, IPT, MV> &regs,
                                                    typename EndType<FL>::type *s_end_raw, V *s_prod_raw, unsigned *s_flag,
                                                    const V *s_x = nullptr, int tid_in = -1, bool lean = false, AG after_gather = AG())
{
    constexpr int CPT = IPT / 4 + 1;
    const int tid = tid_in < 0 ? (int) threadIdx.x : tid_in;
    const int *__restrict__ row_offsets = p.row_end - 1;
    const int tile_rows = c1.x - c0.x;
    const int first = c0.x + 1;
    const int i0 = first & ~3;
    const int eshift = first - i0;
    Vec4<int> ro[CPT];
    // row ends of the tile (+ the IPT the per-thread walk may peek at)
    const int ro_chunks = (tile_rows + eshift + (FL ? 0 : IPT) + 3) / 4;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        // block-uniform: a tile of long rows needs one chunk per thread at most; every vector-memory
        // instruction spared is a slot in the CU's memory pipeline, which is what this kernel queues on
        if (k == 0 || k * BLOCK < ro_chunks) {
            const int q = tid + k * BLOCK;
            const int i = q < ro_chunks ? i0 + 4 * q : i0;
            ro[k] = ld_stream4<NT>(row_offsets + (unsigned) i);
        }
    }
    V xv[CPT][4];
    unsigned in_band = 0u;                     // BAND: one bit per staged nonzero of this thread
    constexpr bool LAZY = band_lazy_values<V, BAND>();
    Vec4<MV> bval[LAZY ? CPT : 1];              // LAZY: the values, fetched here and only for chunks with a nonzero of the band
    constexpr bool WIRE = vals_linewise<V, NT, LAZY, MV>() && FL;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        if constexpr (WIRE) {
            int gc[4]; wire_cols(regs.col[k], gc);
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[k][i] = XL ? s_x[(unsigned) gc[i]] : p.x[(unsigned) gc[i]];
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (BAND) {
                xv[k][i] = (V) 0;
                if ((unsigned) (regs.col[k].get(i) - p.band_lo) < (unsigned) p.band_len) { xv[k][i] = p.x[(unsigned) regs.col[k].get(i)]; in_band |= 1u << (4 * k + i); }
            } else xv[k][i] = XL ? s_x[(unsigned) regs.col[k].get(i)] : p.x[(unsigned) regs.col[k].get(i)];
        }
        if constexpr (LAZY) {
            zero4(bval[k]);
            if ((in_band >> (4 * k)) & 0xfu) {
                // the address issue_nonzero_loads used for this chunk's columns (a chunk past the tile re-reads the tile's first)
                const int a0 = c0.y & ~3, last_full = (p.nnz & ~3) - 4;
                int e0 = a0 + 4 * (tid + k * BLOCK);
                e0 = (e0 < c1.y && e0 <= last_full) ? e0 : (a0 < last_full ? a0 : last_full);
                bval[k] = ld_stream4<NT>(p.values + e0);
            }
        }
    }
    after_gather();
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int q = tid + k * BLOCK;
        if (q < ro_chunks) {
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ro[k].get(j) - c0.y;
            st_lds4(&s_end_raw[4 * q], v);
            if (FL && !lean) {
                // row starts inside the tile (rows before the tile give v <= 0, rows after it
                // v >= tile_nnz; v == 0 is the tile's first nonzero, flagged anyway)
                const int tile_nnz = c1.y - c0.y, pshift = c0.y - (c0.y & ~3);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned) v[j] < (unsigned) tile_nnz) atomicOr(&s_flag[(pshift + v[j]) >> 5], 1u << ((pshift + v[j]) & 31));
            }
        }
    }
    if (FL && !lean && tid == 0) atomicOr(&s_flag[0], 1u << (c0.y - (c0.y & ~3)));
    Vec4<MV> own_val[LAZY || WIRE ? 1 : CPT];
    if constexpr (!LAZY && !WIRE) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) own_val[k] = vals_linewise<V, NT, LAZY, MV>() ? linewise_own(regs.val[k]) : regs.val[k];
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int chunk = tid + k * BLOCK;
        if constexpr (WIRE) {
            const WirePos wp = wire_pos(chunk, tid);
            V pa[2], pb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) { pa[i] = regs.val[k].get(i) * xv[k][i]; pb[i] = regs.val[k].get(2 + i) * xv[k][2 + i]; }
            st_unit(&s_prod_raw[2 * prod_unit<V, CPT>(2 * wp.qa + (wp.off >> 1), lean)], pa);
            st_unit(&s_prod_raw[2 * prod_unit<V, CPT>(2 * wp.qb + (wp.off >> 1), lean)], pb);
            continue;
        }
        V prod[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (LAZY) prod[i] = ((in_band >> (4 * k + i)) & 1u) ? bval[k].get(i) * xv[k][i] : (V) 0;
            else if constexpr (BAND) prod[i] = ((in_band >> (4 * k + i)) & 1u) ? own_val[k].get(i) * xv[k][i] : (V) 0;
            else prod[i] = widen<V>(own_val[k].get(i)) * xv[k][i];
        }
        if (FL) st_prod_chunk<CPT>(s_prod_raw, chunk, prod, lean);
        else st_lds4(&s_prod_raw[swz_prod(4 * chunk)], prod);
    }
    __syncthreads();
}

// true when every vector load of the interior path stays inside full chunks of the arrays
template <int IPT>
__device__ __forceinline__ bool tile_is_interior(const Coord c0, const Coord c1, int tile, int num_tiles,
                                                 int last_full_nz, int last_full_ro)
{
    const int first = c0.x + 1;
    const int i0 = first & ~3;
    const int ro_chunks = ((c1.x - c0.x) + (first - i0) + IPT + 3) / 4;
    return tile != num_tiles - 1 && c1.y <= last_full_nz + 4 && i0 + 4 * ro_chunks <= last_full_ro + 4;
}

template <typename V, int BLOCK, int IPT, bool NT, bool FL, bool BAND = false, typename AG = NoAfterGather, typename MV = V>
__device__ __forceinline__ void stage_tile(const Params<V, MV> &p, const Coord c0, const Coord c1, int tile, int num_tiles,
                                           const TileRegs<V, BLOCK, IPT, MV> &regs, typename EndType<FL>::type *s_end_raw,
                                           V *s_prod_raw, int last_full_nz, int last_full_ro, unsigned *s_flag, const V *s_x = nullptr, int tid_in = -1,
                                           bool lean = false, AG after_gather = AG())
{
    const bool interior = tile_is_interior<IPT>(c0, c1, tile, num_tiles, last_full_nz, last_full_ro);      // block-uniform
    if constexpr (BAND) {              // (a banded pass is for an x beyond L2: never the LDS copy)
        if (interior) stage_tile_interior<V, BLOCK, IPT, NT, FL, false, true>(p, c0, c1, regs, s_end_raw, s_prod_raw, s_flag, nullptr, tid_in);
        else stage_tile_careful<V, BLOCK, IPT, NT, FL, false, true>(p, c0, c1, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, nullptr, tid_in);
    } else if (MSPMV_LIKELY((layout_hints<V, IPT>()), s_x == nullptr)) {
        // (the likelihoods order the code of the SMALL tile shapes: x in memory, interior tile, usable hints, lean reduction first and in
        //  one piece -- a block that runs alone, i.e. a small problem, waits for every stretch of instructions it jumps to:
        //  instruction-cache misses per 28-tile launch 169 -> 87, wave-cycles -21 %, profiles/r04_small_call_counters.txt; a full
        //  device has them all in its caches, and the large fp32 shape sits at its register limit: the hints cost it spills)
        if (MSPMV_LIKELY((layout_hints<V, IPT>()), interior)) stage_tile_interior<V, BLOCK, IPT, NT, FL, false, false, AG>(p, c0, c1, regs, s_end_raw, s_prod_raw, s_flag, nullptr, -1, lean, after_gather);
        else stage_tile_careful<V, BLOCK, IPT, NT, FL, false, false, AG>(p, c0, c1, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, nullptr, -1, lean, after_gather);
    } else {                                  // block-uniform: x lives in LDS (tiny x only)
        if (MSPMV_LIKELY((layout_hints<V, IPT>()), interior)) stage_tile_interior<V, BLOCK, IPT, NT, FL, true, false, AG>(p, c0, c1, regs, s_end_raw, s_prod_raw, s_flag, s_x, -1, lean, after_gather);
        else stage_tile_careful<V, BLOCK, IPT, NT, FL, true, false, AG>(p, c0, c1, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, s_x, -1, lean, after_gather);
    }
}

// x -> LDS (dynamic shared memory, p.x_lds entries) at block start; nullptr when the call does not use it.
// The copy is visible after the block's first barrier.
template <typename V, typename MV = V>
__device__ __forceinline__ const V *stage_x_in_lds(const Params<V, MV> &p, unsigned char *s_dyn, int block)
{
    if (p.x_lds <= 0) return nullptr;
    V *s_x = reinterpret_cast<V *>(s_dyn);
    for (int i = threadIdx.x; i < p.x_lds; i += block) s_x[i] = p.x[i];
    return s_x;
}

// The same copy in two steps (tile_kernel_snap, scalar-hint shapes): the loads are REQUESTED at the very head of the block --
// before the hints are waited for, before the tile's streams -- and WRITTEN to LDS after the streams have been requested
// (vector loads return in order: waiting for the oldest does not wait for the streams).  In one step the block sat through
// hint latency + x latency with nothing else in flight: 0.5 us of a 5.7 us block life on the reference's --dense inputs.
template <typename V, int BLOCK> struct XRegs { static constexpr int N = X_LDS_MAX_BYTES / (int) sizeof(V) / BLOCK; V v[N]; };
template <typename V, int BLOCK, typename MV = V>
__device__ __forceinline__ void request_x_for_lds(const Params<V, MV> &p, XRegs<V, BLOCK> &xr)
{
    static_assert(XRegs<V, BLOCK>::N >= 1, "x_lds entries per thread");
#pragma unroll
    for (int j = 0; j < XRegs<V, BLOCK>::N; ++j) {
        const int i = (int) threadIdx.x + j * BLOCK;
        xr.v[j] = i < p.x_lds ? p.x[i] : (V) 0;
    }
}
template <typename V, int BLOCK, typename MV = V>
__device__ __forceinline__ void commit_x_to_lds(const Params<V, MV> &p, const XRegs<V, BLOCK> &xr, unsigned char *s_dyn)
{
    V *s_x = reinterpret_cast<V *>(s_dyn);
#pragma unroll
    for (int j = 0; j < XRegs<V, BLOCK>::N; ++j) {
        const int i = (int) threadIdx.x + j * BLOCK;
        if (i < p.x_lds) s_x[i] = xr.v[j];
    }
}

// Block -> tile mapping of the one-tile-per-block launches.  Blocks are dealt round-robin to the 8
// XCDs (block b runs on XCD b % 8: observed; only speed depends on it).  Inside every group of 8*G
// blocks, XCD k takes G CONSECUTIVE tiles: neighbouring tiles gather neighbouring x (which then stays in
// that XCD's private L2) and each XCD reads longer contiguous pieces of the CSR arrays, while the XCDs
// still advance through the matrix together.  Bijective for any num_tiles; log2 G = 0 turns it off.
constexpr int TILE_MAP_CONTIGUOUS = 30;       // chunk_log2 value selecting one contiguous tile range per XCD
__device__ __forceinline__ int xcd_chunked_tile(int b, int num_tiles, int chunk_log2)
{
    if (chunk_log2 == TILE_MAP_CONTIGUOUS) {
        // XCD k takes tiles [k*T/8, (k+1)*T/8): what the band-major prepared plan wants (each XCD's L2
        // then only ever sees the x slice of the band(s) its range covers); bijective for any T
        const int q = num_tiles / 8, r = num_tiles % 8;
        const int xcd = b & 7, idx = b >> 3;
        return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    if (chunk_log2 > 0) {
        // groups of span = 8 * 2^chunk_log2 blocks; shifts, not divisions (the compiler does not see that span is a power of
        // two, and this sits at the very head of every block, before its first load can be requested); b, num_tiles >= 0
        const int sh = chunk_log2 + 3;
        if (b < ((num_tiles >> sh) << sh)) {
            const int q = b >> sh, r = b & ((1 << sh) - 1);
            return (((q << 3) | (r & 7)) << chunk_log2) + (r >> 3);
        }
    }
    return b;
}

// the same map without a branch (the head of tile_kernel_snap: scalar selects, nothing between the wave's start and its hint request)
__device__ __forceinline__ int xcd_chunked_tile_flat(int b, int num_tiles, int chunk_log2)
{
    const int q8 = num_tiles >> 3, r8 = num_tiles & 7, xcd = b & 7;
    const int contiguous = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
    const int sh = (chunk_log2 & 15) + 3, cl = chunk_log2 & 15;                     // (& 15: the shifts stay defined when chunk_log2 is the contiguous code)
    const int q = b >> sh, r = b & ((1 << sh) - 1);
    const int chunked = b < ((num_tiles >> sh) << sh) ? (((q << 3) | (r & 7)) << cl) + (r >> 3) : b;
    return chunk_log2 == TILE_MAP_CONTIGUOUS ? contiguous : chunk_log2 > 0 ? chunked : b;
}

// The compact launches (small problems: up to 2304 tiles): ONE CONTIGUOUS TILE RANGE PER XCD (map != 0), the same range in every call.
// Blocks are dealt round-robin to the XCDs (block b -> XCD b % 8), so with tile = block index neighbouring tiles sit on eight different
// XCDs and each fetches the x window of its rows for itself (a 5-point grid of 500^2: 10.9 KB of x beside the 17 KB of the tile's own
// streams); with one range per XCD the window is fetched once per XCD, the lines that straddle tile boundaries once instead of twice
// -- and a matrix of up to ~4 MB per XCD appears to be still in that XCD's L2 at the next call of a solver's loop (where the advantage
// ends: 2300-2800 tiles, 4-6 MB per XCD; mspmv_api.hip: compact_max_tiles).  Measured (tools/ab_driver, interleaved with the block-index map, fp64 / fp32 5-point grids):
// 697 tiles 4.35 -> 4.13 / 3.29 -> 3.27 us per call, 1003 tiles 5.31 -> 4.69 / 3.75 -> 3.53, 1366 tiles 7.05 -> 6.09 / 4.64 -> 4.07.
// Forward progress is not a matter of order here either: a tile that needs another workgroup's record (a long row ending in it) polls a
// bounded number of times and then computes the sum itself; inside a range a lower-numbered tile sits on an earlier block, only the
// first tiles of a range (and group leaders at a range's edge) look at blocks dispatched after them.
__device__ __forceinline__ int compact_tile(int b, int num_tiles, int map)
{
    const int q8 = num_tiles >> 3, r8 = num_tiles & 7, xcd = b & 7;
    const int contiguous = xcd * q8 + (xcd < r8 ? xcd : r8) + (b >> 3);
    return map ? contiguous : b;                  // (scalar arithmetic and a select: nothing between the wave's start and its hint request)
}

}  // namespace mspmv
