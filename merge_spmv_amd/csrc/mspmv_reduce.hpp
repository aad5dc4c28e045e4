// mspmv_reduce.hpp -- the in-tile reductions: consume_tile_lds (the reference's path walk), LookBack, consume_tile_flags (row-start
// bits + segmented scan, swizzled LDS), consume_tile_rows (lean rows) and CompactChain.
#pragma once
#include "mspmv_wave.hpp"

namespace mspmv {

// ---------------------------------------------------------------------------
// The reference's in-tile algorithm (agent_spmv_orig.cuh:539-634,906-913), tuned for CDNA4:
// per-thread merge-path search on diagonal tid*IPT, the IPT-step path walk, the block-wide
// carry scan, the y stores and the tile's carry-out.  Used by the dword-per-lane fallback
// kernel (tile_kernel) and selectable in tile_kernel_vec for comparison (tuning flag 0x70000);
// the production kernels use consume_tile_flags below.  Everything is tile-relative
// (row 0 == c0.x, nonzero 0 == c0.y).
//   s_end[r]  = tile-relative nonzero index where tile row r ends (r <
//               tile_rows), +inf for the row left open at the tile end (the
//               reference instead loads row_end[tile_rows] -- one past the
//               array for the last tile);
//   s_prod[j] = values[j] * x[cols[j]] for the tile's nonzeros.
// ---------------------------------------------------------------------------
template <typename V, int BLOCK, int IPT, bool AXPBY, bool SWZ = false, typename MV = V>
__device__ __forceinline__ void consume_tile_lds(const Params<V, MV> &p, const Coord c0, int tile_rows, int tile_nnz,
                                                 const int *s_end, const V *s_prod, V *s_y, int *s_wave_key,
                                                 V *s_wave_val, Carry<V> *__restrict__ carry_out, int pshift = 0)
{
    // s_y (tile_rows entries) may alias the memory behind s_prod.  SWZ: s_prod is the raw
    // (unshifted) array, product j lives at swz_prod(pshift + j).
    // Straight-line code throughout: divergent branches in the search and the walk made
    // every wave execute both sides of each step (measured 15-23 % of the kernel on
    // short-row matrices).  Requirements on the staging: s_end[r] = +inf for every
    // r >= tile_rows and s_prod[j] = 0 for every j >= tile_nnz, up to TILE + IPT + 3.
    const int tid = threadIdx.x;
    const int tile_items = tile_rows + tile_nnz;
    int diag = tid * IPT; diag = diag < tile_items ? diag : tile_items;

    // ---- in-tile merge-path search: x(diag) = #{r < tile_rows : s_end[r] + r < diag}
    // (the predicate is monotone in r, Appendix B.2; the bounds max(diag - nnz, 0) and
    // min(diag, rows) of the reference's search are implied by it).  Uniform trip count.
    int row = 0;
    for (int step = 1 << (31 - __builtin_clz(tile_rows | 1)); step > 0; step >>= 1) {
        const int q = row + step;                      // candidate count
        const int e = s_end[q - 1 < tile_rows ? q - 1 : tile_rows];   // clamped: slot tile_rows holds +inf
        row = (q <= tile_rows && e + (q - 1) < diag) ? q : row;
    }
    const int first_row = row;                         // the row this thread starts in
    const int nz = diag - row;

    // ---- walk IPT path items, latency-free form.
    // The reference's walk (agent_spmv_orig.cuh:557-578) reads LDS once per step with the
    // address depending on the previous step: IPT dependent LDS round trips.  Here the
    // <= IPT row ends this thread can reach are read in one batch; row-end j sits at path
    // item (s_end[first_row + j] - nz) + j of this thread, which gives a bit mask of the
    // items that are row ends; the k-th item is then nonzero nz + k - popcount(mask below
    // k), so all products are read in a second batch and the segmented sum runs in registers.
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const int pos = s_end[row + j] - nz + j;       // +inf sentinel (2^30) stays out of range
        mask |= pos < IPT ? 1u << pos : 0u;
    }
    V prod[IPT];
    {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            prod[k] = SWZ ? s_prod[swz_prod(pshift + nz + k - cnt)] : s_prod[nz + k - cnt];
            cnt += (mask >> k) & 1u;
        }
    }
    // segmented sum in registers: ended[k] = total of the row that ends at item k
    V ended[IPT];
    V total = 0;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const bool end = (mask >> k) & 1u;
        ended[k] = total;
        total = end ? (V) 0 : total + prod[k];
    }
    const int done_all = __builtin_popcount(mask);
    // ---- carry between threads: block-wide exclusive reduce-by-key scan (has a barrier
    //      inside: after it every thread has finished reading s_prod, which s_y aliases)
    int prev_key, agg_key; V carry_in, agg_val;
    block_exclusive_rbk<V, BLOCK>(row + done_all, total, s_wave_key, s_wave_val, prev_key, carry_in, agg_key, agg_val);
    // ---- row totals -> LDS (scattered 4/8-byte LDS writes are cheap; scattered global
    //      stores were not: ~1.3 rows per L2 write request, as many requests as the
    //      whole read stream on a 5-nnz/row matrix), then one coalesced copy to y.
    {
        // prev_key == first_row whenever tid > 0 (the previous thread ended in the row this
        // thread started in); thread 0 has no in-tile carry.
        const V first_carry = (tid > 0 && prev_key == first_row) ? carry_in : (V) 0;
        int done = 0;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            if ((mask >> k) & 1u) {
                s_y[row + done] = done == 0 ? ended[k] + first_carry : ended[k];
                ++done;
            }
        }
    }
    if (tid == BLOCK - 1) {
        // the row left open at the tile end (ref: agent_spmv_orig.cuh:906-913)
        Carry<V> c; c.key = c0.x + agg_key; c.value = agg_val;
        *carry_out = c;
    }
    __syncthreads();
    V *__restrict__ y = p.y + c0.x;
    for (int r = tid; r < tile_rows; r += BLOCK) {
        if (AXPBY) y[r] = p.alpha * s_y[r] + (p.beta == (V) 0 ? (V) 0 : p.beta * y[r]);
        else y[r] = s_y[r];
    }
}

// ---------------------------------------------------------------------------
// Carries without a second launch (tile_kernel_snap, for the rows its boundary snapping leaves open).  The per-tile carries
// are LOCAL partial sums -- no tile needs another tile's result to compute its own -- so the fix-up "y[row] += carries of
// the tiles before the one in which the row ends" can be done by that tile itself.  A tile that leaves a row open PUBLISHES
// its partial sum as soon as its scan is done.  The tile in which the row ENDS knows exactly which earlier tiles hold
// pieces of it: the row's first nonzero is path item r + row_offsets[r], i.e. it lies in tile (r + row_offsets[r]) / TILE,
// so the pieces are the carries of tiles [that tile, this tile).  It takes exactly those records (one lane each: up to 64 by
// wave 0 alone while the other waves run the row phase, longer lists by the whole block), adds them to its first row in a
// fixed order and clears them.  There is no chain of waits (a waiting tile waits for blocks that wait for nobody before
// publishing), and workgroups are dispatched in order: an awaited block is running or done (mspmv_api.hip:
// safe_chunk_log2 keeps that true under the XCD-chunked tile order).  The reference's fp64 fix-up relies on the same
// property (decoupled look-back, agent_segment_fixup.cuh:262-341 with single_pass_scan_operators.cuh); unlike it,
// nothing here spins on a chain -- and when the property does not hold (fewer resident blocks than assumed) the waiting
// tile computes the sum itself after a bounded poll (recompute_row_head).  Records: rec_store / rec_take above.
// ---------------------------------------------------------------------------
struct LookBack {
    unsigned long long *rec;      // 2 words per tile; nullptr = off (the fix-up launch adds the carries)
    unsigned tag_a, tag_b;        // tag_a is never 0 (a cleared word is never valid)
    int *error;                   // two words of the call's temp storage: [0] receives call_tag when a poll ran out and the consumer computed the
                                  // sum itself (a diagnostic: debug_sync reports it), [1] counts such episodes (was: an epoch mixed into the tags)
    unsigned call_tag;            // what the host compares word [0] with
    int max_polls;                // how often a consumer looks for a record before it computes the sum itself (REC_MAX_POLLS; tests: 1, or 0 = never looks)
    int group_base;               // record index of the first GROUP record (= the launch's number of tiles): see LB_GROUP
};
// GROUP RECORDS: a row spanning thousands of tiles (BASELINE config 4: one row of 67 M nonzeros = 23 800 tiles) left its last tile
// 23 800 records to take -- 24 rounds of memory latency by ONE block, 50 us at the end of a 130 us launch while the chip idles.
// So every LB_GROUP-th piece of a long row is a group LEADER: a tile without a row end, tile % LB_GROUP == LB_GROUP - 1, whose row
// began at or before the group's first tile.  The leader takes its LB_GROUP - 1 predecessors' records (one wave, one round), adds its
// own partial sum and publishes the total as group record tile / LB_GROUP -- instead of a record of its own.  The tile in which
// the row ends derives the same set of leaders from the same two numbers (the row's first piece, its own index) and takes the
// group records of the complete groups plus the single records before the first and after the last of them: at most
// 2 * (LB_GROUP - 1) + pieces / LB_GROUP records.  Every record still has exactly one taker, which clears it; the order of the
// additions is fixed by the tile indices alone; and nothing depends on a record arriving -- a leader whose poll runs out
// computes its group's sum from the matrix, like any consumer.
constexpr int LB_GROUP = 64;
template <typename V> struct LbBits;
template <> struct LbBits<float> {
    static __device__ __forceinline__ void split(float v, unsigned &p0, unsigned &p1) { p0 = __builtin_bit_cast(unsigned, v); p1 = 0u; }
    static __device__ __forceinline__ float join(unsigned p0, unsigned) { return __builtin_bit_cast(float, p0); }
};
template <> struct LbBits<double> {
    static __device__ __forceinline__ void split(double v, unsigned &p0, unsigned &p1)
    { const unsigned long long b = __builtin_bit_cast(unsigned long long, v); p0 = (unsigned) (b >> 32); p1 = (unsigned) b; }
    static __device__ __forceinline__ double join(unsigned p0, unsigned p1)
    { return __builtin_bit_cast(double, ((unsigned long long) p0 << 32) | p1); }
};
template <typename V>
__device__ __forceinline__ void lb_publish(const LookBack &lb, int slot, V value, unsigned long long announced)
{
    unsigned p0, p1; LbBits<V>::split(value, p0, p1);
    rec_store(lb.rec + 2 * (size_t) slot, lb.tag_a, lb.tag_b, p0, p1, announced);
}
__device__ __forceinline__ unsigned long long lb_announce(const LookBack &lb, int slot) { return rec_announce(lb.rec + 2 * (size_t) slot, lb.tag_a); }
// the carry tile s published: waits (bounded) until both words carry this call's tag, then clears the record
template <typename V>
__device__ __forceinline__ V lb_take(const LookBack &lb, int s, bool &ok)
{
    unsigned p0, p1;
    if (rec_take(lb.rec + 2 * (size_t) s, lb.tag_a, lb.tag_b, p0, p1, lb.max_polls)) return LbBits<V>::join(p0, p1);
    ok = false;                             // the caller computes the sum itself (recompute_row_head)
    return (V) 0;
}
// Sum of the carries of tiles [tile - count, tile) -- the pieces of this tile's first row held by earlier tiles --
// taken by the lanes of ONE wave (count <= 64), nearest tile on lane 0; fixed butterfly order; wave-uniform result.
template <typename V>
__device__ __forceinline__ V lb_take_wave(const LookBack &lb, int tile, int count, bool &ok)
{
    const int lane = threadIdx.x & (WAVE - 1);
    V part = lane < count ? lb_take<V>(lb, tile - 1 - lane, ok) : (V) 0;
    if (count > 1) {
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) part += __shfl_xor(part, d, WAVE);
    } else part = __shfl(part, 0, WAVE);
    return part;
}
// The same for a long list (a row spanning more than 64 tiles), by the whole block: thread j takes tiles tile-1-j,
// tile-1-j-BLOCK, ... in that order; wave butterflies; the wave partials in wave order.  Block-uniform call (it has a
// barrier); the result is valid on thread 0.
template <typename V, int BLOCK, int U, typename SlotOf>
__device__ __forceinline__ V lb_take_block(const LookBack &lb, int count, V *s_wave_val, bool &ok, SlotOf slot_of)
{   // (slot_of(i): the record index of the i-th of the `count` records to take)
    // U records per thread and round are requested before any is looked at (a round costs one memory latency whatever its
    // width: with U = 4 a row spanning 37 000 tiles is 37 rounds); one that is not there yet -- only ever among the nearest
    // tiles -- is then polled for.  The order of the additions is fixed by (thread, round, slot).  (U is what the register
    // budget of the calling kernel allows.)
    V part = 0;
    for (int i0 = threadIdx.x; i0 < count; i0 += U * BLOCK) {
        unsigned long long w0[U], w1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * BLOCK;
            w0[u] = w1[u] = 0ull;
            if (i < count) {
                unsigned long long *r = lb.rec + 2 * (size_t) slot_of(i);
                w0[u] = __hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                w1[u] = __hip_atomic_load(r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * BLOCK;
            if (i < count) {
                if (lb.max_polls > 0 && (unsigned) (w0[u] >> 32) == lb.tag_a && (unsigned) (w1[u] >> 32) == lb.tag_b) {
                    unsigned long long *r = lb.rec + 2 * (size_t) slot_of(i);
                    __hip_atomic_store(r, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(r + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    part += LbBits<V>::join((unsigned) w0[u], (unsigned) w1[u]);
                } else part += lb_take<V>(lb, slot_of(i), ok);
            }
        }
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) part += __shfl_xor(part, d, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_wave_val[threadIdx.x / WAVE] = part;
    __syncthreads();
    V total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / WAVE; ++w) total += s_wave_val[w];
    return total;
}

// What the records of tiles [first piece, this tile) add up to, computed from the matrix instead: the products of the
// nonzeros [j0, j1) of the row that ends in this tile (from the row's first nonzero to the tile's first) -- the path of a
// consumer whose poll ran out.  Whole block (barriers inside); fixed order; the result on every thread.
template <typename V, int BLOCK, typename MV = V>
__device__ __forceinline__ V recompute_row_head(const Params<V, MV> &p, int j0, int j1, V *s_wave_val)
{
    V part = 0;
    for (int j = j0 + (int) threadIdx.x; j < j1; j += BLOCK) part += widen<V>(p.values[j]) * p.x[p.cols[j]];
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) part += __shfl_xor(part, d, WAVE);
    __syncthreads();                                   // (s_wave_val may still be read by a take that preceded)
    if ((threadIdx.x & (WAVE - 1)) == 0) s_wave_val[threadIdx.x / WAVE] = part;
    __syncthreads();
    V total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / WAVE; ++w) total += s_wave_val[w];
    return total;
}

// ---------------------------------------------------------------------------
// In-tile reduction of the production kernels: head flags + segmented scan.
//
// The reference walks the tile's merge path thread by thread (a binary search per
// thread, then ITEMS dependent LDS reads, agent_spmv_orig.cuh:539-578); consume_tile_lds
// above is that algorithm.  On CDNA4 it costs ~100 instructions per path item, which is what
// bounds a streaming CsrMV here (39 lane-operations per fp32 nonzero are available at the HBM
// peak).  The same tile result is obtained with no per-thread search and no dependent walk:
//   * staging sets one bit per row START in a bit array over the tile's nonzeros (row r ends
//     at tile-relative nonzero e => the next row starts at e: bit e, when e < tile_nnz; several
//     empty rows set the same bit), plus the bit of the tile's first nonzero;
//   * NONZERO PHASE: thread t owns the NPT consecutive staged products [t*NPT, (t+1)*NPT) (16-byte
//     LDS reads), runs the segmented inclusive sum over them in registers, one block-wide
//     segmented scan of (has-flag, running-sum) supplies the sum flowing in from the threads
//     before it, and S[j] = "sum of the row containing nonzero j, up to j" is written back in place;
//   * ROW PHASE: thread r of the tile's rows reads S at its row's last nonzero (0 for an empty
//     row) and stores y[r] straight from registers, coalesced.  The row left open at the tile
//     end is S at the tile's last nonzero: the carry.
// Path items still bound a tile (rows + nonzeros <= BLOCK*IPT), tiles/carries/fix-up are
// unchanged; only the association order inside a tile differs (sequential inside a thread's
// NPT nonzeros, scan tree across threads), as it already did from the reference's.
// Raw LDS positions outside [pshift, pshift + tile_nnz) may hold anything (the interior
// staging path does not clear them): the bit at pshift isolates what precedes the tile and
// nothing reads S past the tile's last nonzero.
// ---------------------------------------------------------------------------
// 16-byte units of the staged products are XOR-swizzled when a thread of the nonzero phase
// owns 2 or 4 of them (lanes 8 or 4 apart would otherwise start in the same banks).
template <typename V, int CPT>
__device__ __forceinline__ int prod_unit(int u)
{
    constexpr int UPT = CPT * 4 * (int) sizeof(V) / 16;
    // UPT == 6 (fp64, 12 products per thread): lanes 8 apart start 48 units apart = the same banks
    return UPT == 4 ? u ^ ((u >> 4) & 3) : UPT == 2 ? u ^ ((u >> 4) & 1) : UPT == 6 ? u ^ ((u / 48) & 1) : u;
}
template <typename V, int CPT>
__device__ __forceinline__ int prod_slot(int e)      // element index (>= 0) in raw order -> LDS element index
{
    constexpr int EPU = 16 / (int) sizeof(V);
    return prod_unit<V, CPT>(e / EPU) * EPU + (e % EPU);
}
// (plain: the lean row phase of short-row tiles, consume_tile_rows, reads the products of a row at consecutive addresses)
template <typename V, int CPT>
__device__ __forceinline__ int prod_unit(int u, bool plain) { return plain ? u : prod_unit<V, CPT>(u); }
template <typename V, int CPT>
__device__ __forceinline__ int prod_slot(int e, bool plain) { return plain ? e : prod_slot<V, CPT>(e); }
template <int CPT>
__device__ __forceinline__ void st_prod_chunk(float *s_prod_raw, int chunk, const float (&v)[4], bool plain = false)
{
    st_lds4(&s_prod_raw[4 * prod_unit<float, CPT>(chunk, plain)], v);
}
template <int CPT>
__device__ __forceinline__ void st_prod_chunk(double *s_prod_raw, int chunk, const double (&v)[4], bool plain = false)
{
    double2v a, b; a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
    *reinterpret_cast<double2v *>(&s_prod_raw[2 * prod_unit<double, CPT>(2 * chunk, plain)]) = a;
    *reinterpret_cast<double2v *>(&s_prod_raw[2 * prod_unit<double, CPT>(2 * chunk + 1, plain)]) = b;
}
__device__ __forceinline__ void ld_unit(const float *p, float *out)
{ const float4v w = *reinterpret_cast<const float4v *>(p); out[0] = w.x; out[1] = w.y; out[2] = w.z; out[3] = w.w; }
__device__ __forceinline__ void ld_unit(const double *p, double *out)
{ const double2v w = *reinterpret_cast<const double2v *>(p); out[0] = w.x; out[1] = w.y; }
__device__ __forceinline__ void st_unit(float *p, const float *in)
{ float4v w; w.x = in[0]; w.y = in[1]; w.z = in[2]; w.w = in[3]; *reinterpret_cast<float4v *>(p) = w; }
__device__ __forceinline__ void st_unit(double *p, const double *in)
{ double2v w; w.x = in[0]; w.y = in[1]; *reinterpret_cast<double2v *>(p) = w; }

// one Kogge-Stone step of the wave's inclusive segmented sum over (flag, value) pairs
template <typename V, int CTRL, int ROW_MASK>
__device__ __forceinline__ void seg_step(int &f, V &v)
{
    const int f2 = dpp_move<CTRL, ROW_MASK>(0, f);
    const V v2 = dpp_move<CTRL, ROW_MASK>((V) 0, v);
    v += f ? (V) 0 : v2;
    f |= f2;
}
// Block-wide EXCLUSIVE segmented sum: returns the sum of `val` over the threads before this
// one back to (and including) the nearest preceding thread with flag set.  One barrier inside.
template <typename V, int BLOCK>
__device__ __forceinline__ V block_exclusive_segsum(bool flag, V val, int *s_wave_flag, V *s_wave_val, int tid_in = -1)
{
    constexpr int NW = BLOCK / WAVE;
    const unsigned tidu = tid_in < 0 ? threadIdx.x : (unsigned) tid_in;       // (tid_in: see tile_kernel_band)
    const int lane = tidu & (WAVE - 1);
    const int wave = tidu / WAVE;
    int f = flag ? 1 : 0;
    V v = val;
    seg_step<V, 0x111, 0xf>(f, v);      // row_shr:1
    seg_step<V, 0x112, 0xf>(f, v);      // row_shr:2
    seg_step<V, 0x114, 0xf>(f, v);      // row_shr:4
    seg_step<V, 0x118, 0xf>(f, v);      // row_shr:8
    seg_step<V, 0x142, 0xa>(f, v);      // row_bcast15 into rows 1 and 3
    seg_step<V, 0x143, 0xc>(f, v);      // row_bcast31 into rows 2 and 3
    if (lane == WAVE - 1) { s_wave_flag[wave] = f; s_wave_val[wave] = v; }
    __syncthreads();
    V pv = 0;                           // segmented sum of the preceding waves, in order
#pragma unroll
    for (int w = 0; w < NW - 1; ++w) {
        if (w < wave) { const V wv = s_wave_val[w]; pv = s_wave_flag[w] ? wv : pv + wv; }
    }
    const int ef = __shfl_up(f, 1, WAVE);
    const V ev = __shfl_up(v, 1, WAVE);
    return lane == 0 ? pv : (ef ? ev : pv + ev);
}

template <typename V, int BLOCK, int IPT, bool AXPBY, int LB_BATCH = 1, typename MV = V>
__device__ __forceinline__ void consume_tile_flags(const Params<V, MV> &p, const Coord c0, int tile_rows, int tile_nnz,
                                                   const end16_t *s_end, V *s_prod_raw, unsigned *s_flag,
                                                   int *s_wave_flag, V *s_wave_val, Carry<V> *__restrict__ carry_out,
                                                   int pshift, unsigned long long *tr = nullptr, const LookBack *lb = nullptr,
                                                   int tile = 0, bool publish = false, int first_row_tile = 0, int tid_in = -1,
                                                   int first_row_start = 0)
{
    constexpr int TAKE_BATCH = LB_BATCH;
    constexpr int CPT = IPT / 4 + 1;
    constexpr int NPT = CPT * 4;                  // staged products per thread
    constexpr int EPU = 16 / (int) sizeof(V);     // elements per 16-byte unit
    constexpr int UPT = NPT / EPU;
    constexpr int FLAG_WORDS = CPT * BLOCK * 4 / 32 + 1;
    static_assert(NPT <= 16 && FLAG_WORDS <= BLOCK, "flag word handling");
    const int tid = tid_in < 0 ? (int) threadIdx.x : tid_in;

    // one-launch path: a tile that will publish ANNOUNCES itself now -- the thread that will store the record exchanges a marker into
    // the slot; the answer is looked at when the sum is there (rec_store), by then it has long arrived ("EVERY RECORD SLOT IS CLEAN")
    // (a group leader -- "GROUP RECORDS"; first_row_tile < tile only when the tile begins inside a row that began in an earlier one --
    //  publishes the group's slot, by thread 0; a piece without a row end its own, by the thread that holds its last nonzero; a tile
    //  with row ends its own, by the last thread)
    const bool leader = lb != nullptr && publish && tile_rows == 0 && tile % LB_GROUP == LB_GROUP - 1 && first_row_tile <= tile - (LB_GROUP - 1);
    unsigned long long announced = 0ull;
    if (lb != nullptr && publish) {
        const int pub_thread = tile_rows > 0 ? BLOCK - 1 : leader ? 0 : tile_nnz > 0 ? (pshift + tile_nnz - 1) / NPT : 0;
        if (tid == pub_thread) announced = lb_announce(*lb, leader ? lb->group_base + tile / LB_GROUP : tile);
    }

    // ---- nonzero phase
    V s[NPT];
#pragma unroll
    for (int u = 0; u < UPT; ++u) ld_unit(&s_prod_raw[prod_unit<V, CPT>(tid * UPT + u) * EPU], &s[u * EPU]);
    const int base = tid * NPT;
    const unsigned lo = s_flag[base >> 5], hi = s_flag[(base >> 5) + 1];
    const unsigned m = (unsigned) ((((unsigned long long) hi << 32) | lo) >> (base & 31)) & ((1u << NPT) - 1u);
    V run = 0;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        run = ((m >> k) & 1u) ? s[k] : run + s[k];
        s[k] = run;
    }
    if (tr && tid == 0) tr[6] = clock64();
    const V carry_in = block_exclusive_segsum<V, BLOCK>(m != 0u, run, s_wave_flag, s_wave_val, tid_in);
    const unsigned lead = (m & (0u - m)) - 1u;    // bits below the first row start (all ones when none)
#pragma unroll
    for (int k = 0; k < NPT; ++k) s[k] += ((lead >> k) & 1u) ? carry_in : (V) 0;
    if (tile_rows == 0) {
        // block-uniform: no row ends in this tile (a slice of one long row): only the running sum
        // at the tile's last nonzero is needed -- the carry.  No write-back, no third barrier.
        if (tid < FLAG_WORDS) s_flag[tid] = 0u;
        const int last = pshift + tile_nnz - 1;
        if (tile_nnz > 0 ? tid == last / NPT : tid == 0) {
            V v = 0;
#pragma unroll
            for (int k = 0; k < NPT; ++k) v = (tile_nnz > 0 && k == last % NPT) ? s[k] : v;
            Carry<V> c; c.key = c0.x; c.value = v;
            if (p.band_pass > 0) c.value += carry_out->value;      // later column-band pass: same tile, same key
            *carry_out = c;
            if (lb && publish && !leader) lb_publish<V>(*lb, tile, v, announced);   // (only when some tile will take it)
            if (leader) s_wave_val[0] = v;
        }
        if (leader) {
            // (block-uniform) the group's total: the LB_GROUP - 1 records before this tile, by one wave, + this tile's own sum
            __syncthreads();
            const V own = s_wave_val[0];
            bool ok = true;
            V before = 0;
            if (tid < WAVE) before = lb_take_wave<V>(*lb, tile, LB_GROUP - 1, ok);
            if (__syncthreads_or(ok ? 0 : 1)) {
                // a poll ran out: the nonzeros of the group's earlier tiles, from the matrix (they are the row's, one tile's worth each --
                // or from the row's first nonzero, when the group begins with the row's first piece)
                const int j0 = first_row_tile == tile - (LB_GROUP - 1) ? first_row_start : c0.y - (LB_GROUP - 1) * (BLOCK * IPT);
                before = recompute_row_head<V, BLOCK>(p, j0, c0.y, s_wave_val);
                if (tid == 0 && lb->error) {
                    __hip_atomic_store(lb->error, (int) lb->call_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(lb->error + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (tid == 0) lb_publish<V>(*lb, lb->group_base + tile / LB_GROUP, before + own, announced);
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < UPT; ++u) st_unit(&s_prod_raw[prod_unit<V, CPT>(tid * UPT + u) * EPU], &s[u * EPU]);
    __syncthreads();
    if (tr && tid == 0) tr[7] = clock64();
    if (tid < FLAG_WORDS) s_flag[tid] = 0u;       // clean for the next tile's staging (after the loop's barrier)

    // ---- the row left open at the tile end (ref: agent_spmv_orig.cuh:906-913): the carry.  Written -- and, on the
    //      single-launch path, published for the tile in which that row ends -- BEFORE the row phase, as early as it exists
    if (tid == BLOCK - 1) {
        const int e_last = tile_rows > 0 ? s_end[tile_rows - 1] : 0;
        Carry<V> c; c.key = c0.x + tile_rows;
        c.value = tile_nnz > e_last ? s_prod_raw[prod_slot<V, CPT>(pshift + tile_nnz - 1)] : (V) 0;
        if (p.band_pass > 0) c.value += carry_out->value;
        *carry_out = c;
        if (lb && publish) lb_publish<V>(*lb, tile, c.value, announced);
    }
    // single-launch path: the pieces of this tile's first row held by tiles [first_row_tile, tile) (thread 0 stores row 0).
    // Up to 64 of them: wave 0 alone, while the other waves go on with the row phase; more: the whole block.
    V first_row_carry = 0;
    if (lb) {
        const int pieces = tile - first_row_tile;            // block-uniform
        if (pieces > 0) {
            bool ok = true;
            // the complete groups among the pieces [first_row_tile, tile): their leaders folded them into group records
            const int g_first = (first_row_tile + LB_GROUP - 1) / LB_GROUP, g_end = tile / LB_GROUP;
            if (g_first < g_end) {
                const int n_tail = tile - g_end * LB_GROUP, n_groups = g_end - g_first, n_head = g_first * LB_GROUP - first_row_tile;
                const int gb = lb->group_base;
                // nearest first: the single records after the last complete group, the group records, the singles before the first
                first_row_carry = lb_take_block<V, BLOCK, TAKE_BATCH>(*lb, n_tail + n_groups + n_head, s_wave_val, ok, [=](int i) {
                    return i < n_tail ? tile - 1 - i : i < n_tail + n_groups ? gb + g_end - 1 - (i - n_tail) : g_first * LB_GROUP - 1 - (i - n_tail - n_groups); });
            } else if (pieces > WAVE) first_row_carry = lb_take_block<V, BLOCK, TAKE_BATCH>(*lb, pieces, s_wave_val, ok, [=](int i) { return tile - 1 - i; });
            else if (tid < WAVE) first_row_carry = lb_take_wave<V>(*lb, tile, pieces, ok);
            // a poll ran out (see "NOTHING DEPENDS ON A RECORD ARRIVING" above): the whole block computes the sum from the
            // matrix -- the row's nonzeros before this tile (its cancelled slots are wiped by their publishers when those come)
            if (__syncthreads_or(ok ? 0 : 1)) {
                first_row_carry = recompute_row_head<V, BLOCK>(p, first_row_start, c0.y, s_wave_val);
                if (tid == 0 && lb->error) {
                    __hip_atomic_store(lb->error, (int) lb->call_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(lb->error + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }

    // ---- row phase
    V *__restrict__ y = p.y + c0.x;
    for (int r = tid; r < tile_rows; r += BLOCK) {
        const int e = s_end[r];
        const int e0 = r > 0 ? s_end[r - 1] : 0;
        V sum = e > e0 ? s_prod_raw[prod_slot<V, CPT>(pshift + e - 1)] : (V) 0;
        if (r == 0) sum += first_row_carry;
        if (AXPBY) y[r] = p.alpha * sum + (p.beta == (V) 0 ? (V) 0 : p.beta * y[r]);
        else y[r] = sum;
    }
}

// ---------------------------------------------------------------------------
// LEAN in-tile reduction for tiles of short rows (tile_kernel_snap): when a row-snapped tile is CLOSED -- it starts at the
// first nonzero of a row and ends with the last nonzero of a row: nothing flows in, nothing is left open -- and its rows
// are short on average, the flag bits, the per-thread running sums, the block-wide segmented scan, the write-back of the
// running sums and two of the three barriers of consume_tile_flags buy nothing: a thread takes a whole row and adds
// up its products straight from LDS.  What bounds a matrix of 4-7 nonzeros per row that lives in the Infinity Cache (the
// reference's --dense=5, the 5/7-point grids) is VALU issue, not bytes (profiles/r03_short_rows/): the general reduction
// costs ~290 vector instructions per wave and tile, this one ~60 on such a tile.
//   * products were staged at their RAW positions (prod_unit(u, plain = true)), so row r's products are the consecutive
//     LDS elements [pshift + e0, pshift + e1), read with immediate offsets from one address per row;
//   * summation order: strictly left to right from +0.0 -- for every row of at most LEAN_SERIAL nonzeros that IS the order of
//     the reference's SpmvGold (gpu_spmv.cu:262-278: partial = 0; partial += v * x, one product at a time), so such rows
//     are bit for bit the sequential definition's; longer rows (rare in a tile that qualifies) are summed by the 16 lanes
//     of a DPP row, strided, then folded: another fixed order;
//   * which reduction a tile takes depends only on its boundaries (closed, nonzeros <= lean_avg * rows), i.e. on the
//     matrix and the tile shape -- never on hints, timing or the device.
// ---------------------------------------------------------------------------
// which tile shapes take the branch likelihoods below: the small ones (what a small problem runs on).  In the fp64 256x11 kernel the
// same hints changed nothing on a full device (dense5, the grids, dense32, circuit, Orkut-sized within +-0.5 %), in the fp32 one
// they cost spills.
template <typename V, int IPT> constexpr bool layout_hints() { return IPT <= 7; }
#define MSPMV_LIKELY(on, c) ((on) ? __builtin_expect(!!(c), 1) : !!(c))      // (on: a constant -- which tile shapes take the hint)
#define MSPMV_UNLIKELY(on, c) ((on) ? __builtin_expect(!!(c), 0) : !!(c))
// acc += v[j] for j < len - base, j = 0 .. 7, left to right, under a SHRINKING EXEC MASK: v_cmpx + v_add per product -- the lanes
// leave as their row ends -- instead of compare + select(s) + add (3 instructions per product in fp32, 4 in fp64).  The same additions
// in the same order as `acc = j < len ? acc + v[j] : acc`; EXEC is restored.  (The lean reductions of short-row tiles are bound by
// VALU issue, not bytes: profiles/r04_short_rows/.)
template <typename V> struct CompactChain;
template <> struct CompactChain<double> {
    // the first half alone: rows of at most four products (the caller knows that no lane of the wave has more)
    static __device__ __forceinline__ void add4(double &acc, const double (&v)[4], int len)
    {
        unsigned long long sv;
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 0, %[l]\n\tv_add_f64 %[a], %[a], %[v0]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 1, %[l]\n\tv_add_f64 %[a], %[a], %[v1]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 2, %[l]\n\tv_add_f64 %[a], %[a], %[v2]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 3, %[l]\n\tv_add_f64 %[a], %[a], %[v3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(sv)
                     : [l] "v"(len), [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3])
                     : "vcc");
    }
    // acc (+0.0 on entry) += v[j] for j < len, left to right, lanes leaving as their row ends (EXEC restored)
    static __device__ __forceinline__ void add8(double &acc, const double (&v)[8], int len, int base)
    {
        unsigned long long sv;
        const int l = len - base;
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 0, %[l]\n\tv_add_f64 %[a], %[a], %[v0]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 1, %[l]\n\tv_add_f64 %[a], %[a], %[v1]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 2, %[l]\n\tv_add_f64 %[a], %[a], %[v2]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 3, %[l]\n\tv_add_f64 %[a], %[a], %[v3]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 4, %[l]\n\tv_add_f64 %[a], %[a], %[v4]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 5, %[l]\n\tv_add_f64 %[a], %[a], %[v5]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 6, %[l]\n\tv_add_f64 %[a], %[a], %[v6]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 7, %[l]\n\tv_add_f64 %[a], %[a], %[v7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(sv)
                     : [l] "v"(l), [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [v4] "v"(v[4]), [v5] "v"(v[5]), [v6] "v"(v[6]), [v7] "v"(v[7])
                     : "vcc");
    }
};
template <> struct CompactChain<float> {
    // the first half alone: rows of at most four products (the caller knows that no lane of the wave has more)
    static __device__ __forceinline__ void add4(float &acc, const float (&v)[4], int len)
    {
        unsigned long long sv;
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 0, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v0]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 1, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v1]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 2, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v2]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 3, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v3]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(sv)
                     : [l] "v"(len), [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3])
                     : "vcc");
    }
    static __device__ __forceinline__ void add8(float &acc, const float (&v)[8], int len, int base)
    {
        unsigned long long sv;
        const int l = len - base;
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 0, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v0]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 1, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v1]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 2, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v2]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 3, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v3]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 4, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v4]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 5, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v5]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 6, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v6]\n\t"
                     "v_cmpx_lt_i32_e32 vcc, 7, %[l]\n\tv_add_f32_e32 %[a], %[a], %[v7]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [a] "+v"(acc), [sv] "=&s"(sv)
                     : [l] "v"(l), [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]), [v4] "v"(v[4]), [v5] "v"(v[5]), [v6] "v"(v[6]), [v7] "v"(v[7])
                     : "vcc");
    }
};
constexpr int LEAN_SERIAL = 16;        // rows up to this long are summed by one thread
constexpr int LEAN_GROUP_MAX = 256;    // rows up to this long (and longer than LEAN_SERIAL) are summed by the 16 lanes of one DPP row; longer ones by the wave
// Rows of a lean tile that are longer than LEAN_SERIAL -- every lane of the wave calls this with ITS row's first product position
// `pos` (LDS element index), length `len` (0: no row) and running sum `acc`; the owners of such rows get their row's total in `acc`.
//   * LEAN_SERIAL < len <= LEAN_GROUP_MAX: four rows at a time, each by the 16 lanes of one DPP row -- lane j adds products j, j + 16, ...
//     from +0.0, the 16 partial sums are folded left to right (row_shr 1, 2, 4, 8): summation depth <= len / 16 + 4 <= 20;
//   * longer rows (a closed lean tile can hold ONE row of ~2000-3000 nonzeros next to hundreds of empty ones): one at a time by the
//     whole wave -- lane j keeps FOUR running sums, over products j + 64 u + 256 r (u = 0 .. 3), adds them pairwise, and the 64
//     totals are folded by row_shr 1, 2, 4, 8, row_bcast 15 and 31: depth <= len / 256 + 2 + 6 <= 20 for any row a tile can hold.
//     (Until round 5 these rows went to a 16-lane group as well: depth len / 16 + 4, ~150 for such a row -- beyond the
//      2 (ceil(log2(len + 1)) + items_per_thread + 8) of the stated bound, which the tests then only met statistically.)
// A fixed order either way; shared by consume_tile_rows and the compact front end, so the two write the same bits.
template <typename V>
__device__ __forceinline__ void lean_long_rows(const V *s_prod, int pos, int len, int lane, V &acc)
{
    unsigned long long pending = __ballot(len > LEAN_SERIAL && len <= LEAN_GROUP_MAX);
    while (pending != 0ull) {                                           // wave-uniform
        int owner[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            owner[g] = pending != 0ull ? __ffsll((long long) pending) - 1 : -1;
            pending &= pending - 1ull;                                  // (0 stays 0)
        }
        const int grp = lane >> 4, j = lane & 15;
        const int own = grp == 0 ? owner[0] : grp == 1 ? owner[1] : grp == 2 ? owner[2] : owner[3];
        // (both shuffles by ALL lanes, the selection afterwards: a lane switched off by a branch cannot be read from)
        const int g_pos = __shfl(pos, own < 0 ? 0 : own, WAVE);
        const int g_len_any = __shfl(len, own < 0 ? 0 : own, WAVE);
        const int g_len = own < 0 ? 0 : g_len_any;
        const V *gsrc = s_prod + g_pos;
        V part = (V) 0;
        for (int k = j; __ballot(k < g_len) != 0ull; k += 64) {
            V u4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) u4[u] = k + 16 * u < g_len ? gsrc[k + 16 * u] : (V) 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) part += u4[u];
        }
        part += dpp_move<0x111, 0xf>((V) 0, part);                     // row_shr:1
        part += dpp_move<0x112, 0xf>((V) 0, part);                     // row_shr:2
        part += dpp_move<0x114, 0xf>((V) 0, part);                     // row_shr:4
        part += dpp_move<0x118, 0xf>((V) 0, part);                     // row_shr:8  -> lane 15 of every row holds its total
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const V total = __shfl(part, 16 * g + 15, WAVE);
            if (lane == owner[g]) acc = total;
        }
    }
    pending = __ballot(len > LEAN_GROUP_MAX);
    while (pending != 0ull) {                                           // wave-uniform: one row per round, by the whole wave
        const int own = __ffsll((long long) pending) - 1;
        pending &= pending - 1ull;
        const int g_pos = __shfl(pos, own, WAVE), g_len = __shfl(len, own, WAVE);
        const V *gsrc = s_prod + g_pos;
        V a4[4] = {(V) 0, (V) 0, (V) 0, (V) 0};
        for (int k = lane; k < g_len; k += 4 * WAVE) {                  // (the lanes leave as the row runs out: no ballot needed, nothing is exchanged inside)
#pragma unroll
            for (int u = 0; u < 4; ++u) a4[u] += k + WAVE * u < g_len ? gsrc[k + WAVE * u] : (V) 0;
        }
        V part = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        part += dpp_move<0x111, 0xf>((V) 0, part);                     // row_shr:1
        part += dpp_move<0x112, 0xf>((V) 0, part);                     // row_shr:2
        part += dpp_move<0x114, 0xf>((V) 0, part);                     // row_shr:4
        part += dpp_move<0x118, 0xf>((V) 0, part);                     // row_shr:8  -> lane 15 of every row of 16 holds that row's total
        part += dpp_move<0x142, 0xa>((V) 0, part);                     // row_bcast15 into rows 1 and 3
        part += dpp_move<0x143, 0xc>((V) 0, part);                     // row_bcast31 into rows 2 and 3 -> lane 63 holds the total
        const V total = __shfl(part, WAVE - 1, WAVE);
        if (lane == own) acc = total;
    }
}

constexpr int LEAN_BATCH = 8;          // products of a row requested before any is looked at
template <typename V, int BLOCK, int IPT, bool AXPBY, typename MV = V>
__device__ __forceinline__ void consume_tile_rows(const Params<V, MV> &p, const Coord c0, int tile_rows, const end16_t *s_end,
                                                  const V *s_prod_raw, int pshift, Carry<V> *__restrict__ carry_out,
                                                  unsigned long long *tr = nullptr)
{
    const int tid = threadIdx.x;
#ifdef MSPMV_DEV
#define MSPMV_LEAN_TR(i) do { if (tr && tid == 0) tr[i] = wall_clock64(); } while (0)
#else
#define MSPMV_LEAN_TR(i) do { } while (0)
#endif
    MSPMV_LEAN_TR(8);
    if (tid == BLOCK - 1) { Carry<V> c; c.key = c0.x + tile_rows; c.value = (V) 0; *carry_out = c; }     // (nothing open: what mspmv_debug_read_tiles reports)
    V *__restrict__ y = p.y + c0.x;
    // Two rows per thread and iteration (r, r + BLOCK), and every LDS read of a step requested before the first is waited for:
    // the row ends of both rows, then the first LEAN_BATCH products of both (read whether the row has them or not: they lie
    // inside the LDS arrays for any lane, pshift + e0 + 15 < SLOTS) -- two LDS round trips per pair of rows instead of six.
    for (int r0 = 0; r0 < tile_rows; r0 += 2 * BLOCK) {           // block-uniform trip count
        int e0[2], len[2]; bool valid[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = r0 + h * BLOCK + tid;
            valid[h] = r < tile_rows;
            const int rr = valid[h] ? r : 0;                       // (row 0 exists: tile_rows > 0 here)
            const int e1 = s_end[rr];
            const int ep = s_end[rr > 0 ? rr - 1 : 0];             // (read whatever rr is: a select afterwards, not a branch around a second LDS round trip)
            e0[h] = rr > 0 ? ep : 0;
            len[h] = valid[h] ? e1 - e0[h] : 0;
        }
        if (r0 == 0) MSPMV_LEAN_TR(9);
        // (a wave none of whose rows -- of this pair of rounds -- has more than four products reads and adds the first four of each only: the
        //  row-strided product reads are bank-conflict-laden, 57 % of the LDS cycles of a 5-point grid's launch, and the LDS is busy for more
        //  than half of such a kernel: profiles/r05_lds_counters.txt)
        const bool more = __ballot(len[0] > LEAN_BATCH / 2 || len[1] > LEAN_BATCH / 2) != 0ull;      // wave-uniform
        V v[2][LEAN_BATCH];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < LEAN_BATCH / 2; ++j) v[h][j] = s_prod_raw[pshift + e0[h] + j];
        V acc[2] = {(V) 0, (V) 0};
        static_assert(LEAN_BATCH == 8, "CompactChain adds eight");
        if (more) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = LEAN_BATCH / 2; j < LEAN_BATCH; ++j) v[h][j] = s_prod_raw[pshift + e0[h] + j];
            // (all of them requested here, in one go: without this the compiler sinks a read into the branch of the first addition that uses it)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < LEAN_BATCH; ++j) asm volatile("" : "+v"(v[h][j]));
#pragma unroll
            for (int h = 0; h < 2; ++h) CompactChain<V>::add8(acc[h], v[h], len[h], 0);
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < LEAN_BATCH / 2; ++j) asm volatile("" : "+v"(v[h][j]));
#pragma unroll
            for (int h = 0; h < 2; ++h) { const V q[4] = {v[h][0], v[h][1], v[h][2], v[h][3]}; CompactChain<V>::add4(acc[h], q, len[h]); }
        }
        if (r0 == 0) MSPMV_LEAN_TR(10);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const V *src = s_prod_raw + (pshift + e0[h]);
            // rows of LEAN_BATCH + 1 ... LEAN_SERIAL nonzeros: the same left-to-right order, continued
            if (MSPMV_UNLIKELY((layout_hints<V, IPT>()), __ballot(len[h] > LEAN_BATCH) != 0ull)) {
                V w[LEAN_SERIAL - LEAN_BATCH];
#pragma unroll
                for (int j = 0; j < LEAN_SERIAL - LEAN_BATCH; ++j) w[j] = src[LEAN_BATCH + j];
                CompactChain<V>::add8(acc[h], w, len[h], LEAN_BATCH);
            }
            // rows longer than that: by 16-lane groups, the longest by the whole wave (lean_long_rows)
            if (MSPMV_UNLIKELY((layout_hints<V, IPT>()), __ballot(len[h] > LEAN_SERIAL) != 0ull))
                lean_long_rows<V>(s_prod_raw, pshift + e0[h], len[h], tid & (WAVE - 1), acc[h]);
            if (r0 == 0 && h == 0) MSPMV_LEAN_TR(11);
            if (valid[h]) {
                const int r = r0 + h * BLOCK + tid;
                if (AXPBY) y[r] = p.alpha * acc[h] + (p.beta == (V) 0 ? (V) 0 : p.beta * y[r]);
                else y[r] = acc[h];
            }
        }
    }
    MSPMV_LEAN_TR(12);
#undef MSPMV_LEAN_TR
}

}  // namespace mspmv
