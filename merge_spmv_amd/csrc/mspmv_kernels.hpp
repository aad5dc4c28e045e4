// mspmv_kernels.hpp -- hand-written CDNA4 (gfx950, wave64) kernels of the
// merge-based CsrMV.  Replaces the reference's cub/agent/agent_spmv_orig.cuh,
// agent_segment_fixup.cuh and the kernels of
// cub/device/dispatch/dispatch_spmv_orig.cuh:68-224; none of that code (nor
// any CUB/hipCUB/rocPRIM primitive) is used.  The algorithm contract is
// SURVEY.md Appendix B.
//
// What a SpMV runs, all on the caller's stream (mspmv_api.hip picks):
//   ONE launch, the default: tile_kernel_snap -- one 256-thread block per merge tile (XCD-chunked tile order).  The tile's
//                      two boundaries are HINTS read from the caller's temp storage and verified against four row offsets
//                      (wrong: two waves search them -- wave_merge_path_guess -- and store the repaired hints); boundaries
//                      that fall a short way into a row are snapped to the row's first nonzero, so there are no carries
//                      and no fix-up for short rows; rows longer than that hand their pieces over as tagged records
//                      (LookBack).  Inside the tile: 16-byte streaming of (col, val) and row offsets, gather of x (from a
//                      per-block LDS copy when x is <= 4 KB), products and 16-bit tile-relative row ends staged in LDS, one
//                      bit per row start; segmented running sums over 12 consecutive products per thread + one block-wide
//                      DPP segmented scan (consume_tile_flags), y stored per row from registers  (ref: DeviceSpmvKernel);
//                      closed tiles of short rows: a thread per row straight from LDS instead (consume_tile_rows);
//                      fp64 values read non-temporally are fetched line by line over the wave (ld_stream4_linewise)
//   the classic three launches (column-band candidates, the band-major plan's tile order, unaligned arrays, tuning options):
//   1. tile boundaries of the merge path -> coords[tile]            (ref: DeviceSpmvSearchKernel)
//        coords_scatter_kernel : ONE coalesced pass over row_offsets (row end r sits at path position
//                      r + row_end[r]); the default below 10 M rows;
//        coords_interp_kernel  : one THREAD per boundary -- bracket in an LDS table of 1025 samples, secant steps,
//                      exact binary search of what is left; latency-bound, the default from 10 M rows up;
//        search_kernel : one WAVE per boundary, 64-ary search (option)
//      (the same kernels fill in the hints of tile_kernel_snap ahead of time: mspmv_csrmv_prepare)
//   2. tile_kernel_vec : the same tile body on stored coordinates, one (row, partial) carry per tile
//      tile_kernel_vec<.., Bands> : the same kernel with the column-band passes compiled in (run_band_passes): when 64
//                      sampled windows of column indices (band_detect_block, riding on the coordinate launch) say the
//                      columns are spread uniformly over an x several times L2, the first 4-5 blocks per CU stream the
//                      matrix once per band of x instead (C2 fp32: 1.22 -> 0.83 ms); otherwise the ordinary body runs
//      tile_kernel     : dword-per-lane fallback for unaligned arrays, with the reference's
//                      per-thread search + path walk (consume_tile_lds)
//   3. fixup_onepass_kernel : deterministic reduce-by-key over the per-tile carries in one
//                      launch (every run of equal keys has one owner block), y[row] += sum;
//                      no decoupled look-back, no spin-waits, no atomics: bitwise reproducible
//                      (ref: DeviceSegmentFixupKernel).  fixup_kernel / fixup_atomic_kernel:
//                      multi-level and atomic options.
// Development variants of tile_kernel_vec (persistent grid, ablations, cycle stamps) compile only with -DMSPMV_DEV.
// mspmv_spmm.hpp builds the SpMM kernels on the same pieces.
// Which variant of a tile kernel runs is spelled by tag types (mspmv_types.hpp), so a launch site and a profile both say it:
//   tile_kernel_vec<float, 256, 11, Clocked, Assign, Streamed>     body Sweep | Bands | Clocked (-DMSPMV_DEV: DevSweep<..>)
//   tile_kernel_snap<double, 256, 7, Compact, Axpby, Cached>       body General | Compact
//   output Assign (y = A x) | Axpby (y = alpha A x + beta y); streams Cached | Streamed (non-temporal loads of the CSR arrays)
//
// This header is the map.  What the kernels are built from lies in the headers below, each including the one before it:
//   mspmv_types.hpp     Coord, Carry, Params, the variant tags, the tagged records (rec_announce, rec_store, rec_take), BoundaryOut
//   mspmv_coords.hpp    merge-path search, band detection, search_kernel / coords_scatter_kernel / coords_interp_kernel
//   mspmv_wave.hpp      wave primitives (DPP segmented scan, block reduce-by-key); streaming loads (Vec4, widen, ld_stream4*)
//   mspmv_reduce.hpp    in-tile reductions: consume_tile_lds, LookBack, consume_tile_flags, consume_tile_rows, CompactChain
//   mspmv_stage.hpp     tile_kernel; 16-byte staging: TileRegs, issue_nonzero_loads, stage_tile*, x in LDS, block -> tile maps
//   mspmv_tdm.hpp       TdmArgs, stage_tile_tdm: the staging of the clock-scheduled column bands (on mspmv_stage.hpp)
// and below them, here: BandArgs, run_band_passes, tile_kernel_vec; the fix-up kernels; wave_merge_path_guess, the compact front
// end, tile_kernel_snap; probe_read_kernel, launch_exact, mg_apply_kernel.
#pragma once
#include "mspmv_types.hpp"
#include "mspmv_coords.hpp"
#include "mspmv_wave.hpp"
#include "mspmv_reduce.hpp"
#include "mspmv_stage.hpp"
#include "mspmv_tdm.hpp"

namespace mspmv {

// What the tile kernel needs to know about the column bands (the Bands and Clocked variants of tile_kernel_vec; verdict == nullptr otherwise)
struct BandArgs {
    const int *verdict;        // BAND_WINDOWS verdicts of band_detect_block
    int *counters;             // 8 claim counters, BAND_COUNTER_STRIDE ints apart, zeroed by band_detect_block
    int *next;                 // num_tiles ints: next[t] = the tile the block that ran t in pass 0 took after it
    int grid;                  // blocks that run the passes (4-5 per CU, a multiple of 8); the others return
    int bands, band_cols;
    int force;                 // 1: passes whatever the verdicts say (mspmv_set_band_passes)
    TdmArgs tdm;               // band_shift > 0: clock-scheduled bands instead of the passes
};

// The column-band passes of one call, run by the first `grid` blocks of the tile kernel's launch.
// Pass 0 hands out the tiles dynamically -- as the hardware's block dispatcher does for the one-tile-per-block form; a
// static split measured 18 % slower, and so did anything that lets the blocks work far apart in the matrix -- in
// ascending order: block b starts with tile b, then takes tile 8 * n + (b & 7) for the next n of counter (b & 7)
// (8 counters 256 bytes apart: one device-scope atomic per tile on ONE word serialises at ~10 ns, 0.3 ms for C2;
// b & 7 is the block's XCD, and when its own sequence runs out a block helps with the others').  The claim for the
// next tile is issued before the current tile is staged.  Each block chains what it took in next[] and the later
// passes walk the block's own chain, so y[r] and carries[tile] are re-read by the very thread that wrote them: nothing
// travels between CUs or XCDs (next[] is written and read by thread 0 of the same block, past the caches).
// Pass 0 applies the caller's alpha and beta, the later ones add to y and to the stored carries; the ordinary fix-up
// launch follows.  Blocks drift from one band to the next without a barrier: two slices share L2 only while they do.
template <typename V, int BLOCK, int IPT, bool NT>
__device__ __forceinline__ void run_band_passes(Params<V> p, const Coord *__restrict__ coords, Carry<V> *__restrict__ carries,
                                                int num_tiles, const BandArgs &ba, end16_t *s_end_raw, V *s_prod_raw, unsigned *s_flag,
                                                int *s_wave_key, V *s_wave_val)
{
    constexpr int CPT = IPT / 4 + 1;
    constexpr int SLOTS = CPT * BLOCK * 4;
    __shared__ int s_next, s_first;
    const int tid = threadIdx.x;
    if (tid < SLOTS / 32 + 1) s_flag[tid] = 0u;
    // (the block's index is needed again at the head of every pass; kept in LDS, not in a register across the tile loop -- the
    //  fp32 kernel sits at its 64-VGPR cap there, and what does not fit went to scratch memory: .vgpr_spill_count 1-2 until round 6)
    __shared__ V s_beta0;
    if (tid == 0) { s_first = blockIdx.x; s_beta0 = p.beta; }
    const int last_full_nz = (p.nnz & ~3) - 4;
    const int last_full_ro = ((p.rows + 1) & ~3) - 4;
    const int first_n = ba.grid / 8;           // sequence positions the blocks' first tiles used up (grid: a multiple of 8, or < 8 = all the tiles)
    int seq = (int) blockIdx.x & 7;            // thread 0: the sequence it claims from (moves on when one is exhausted)
    for (int b = 0; b < ba.bands; ++b) {
        p.band_lo = b * ba.band_cols; p.band_len = ba.band_cols; p.band_pass = b;
        __syncthreads();
        if (tid == 0) s_next = s_first;        // every pass starts with the block's own first tile: no claim
        __syncthreads();
        p.beta = b == 0 ? s_beta0 : (V) 1;
        for (;;) {
            // (s_next: written before the barrier that ended the previous tile, or the one above)
            const int tile = s_next;
            if (tile >= num_tiles) break;
            int following = num_tiles;
            if (tid == 0) {
                // the tile after this one: the atomic / the load is in flight while this tile is staged
                if (b > 0) following = __hip_atomic_load(ba.next + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (ba.grid >= 8)
                    for (int tries = 0; tries < 8; ++tries) {
                        const int n = first_n + atomicAdd(ba.counters + seq * BAND_COUNTER_STRIDE, 1);
                        following = 8 * n + seq;
                        if (following < num_tiles) break;
                        following = num_tiles; seq = (seq + 1) & 7;
                    }
            }
            // the thread index goes through an empty asm once per tile: what the tile body derives from it (LDS addresses,
            // lane offsets) is then recomputed per tile instead of being hoisted out of the loop and kept live across it,
            // which costs ~40 registers per lane and with them a quarter of the resident waves.
            int t = tid;
            asm volatile("" : "+v"(t));
            __builtin_assume(t >= 0 && t < BLOCK);
            const Coord c0 = coords[tile];
            const Coord c1 = coords[tile + 1];
            TileRegs<V, BLOCK, IPT> regs;
            constexpr bool FL = true, BAND = true, AXPBY = true;      // (16-bit row ends and flags; this band's columns only; every pass with alpha and beta)
            issue_nonzero_loads<V, BLOCK, IPT, NT, !band_lazy_values<V, BAND>()>(p, c0, c1, regs, t);     // (fp64: columns now, values by band in the staging)
            stage_tile<V, BLOCK, IPT, NT, FL, BAND>(p, c0, c1, tile, num_tiles, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, nullptr, t);
            const int pshift = c0.y - (c0.y & ~3);
            const int eshift = (c0.x + 1) - ((c0.x + 1) & ~3);
            consume_tile_flags<V, BLOCK, IPT, AXPBY>(p, c0, c1.x - c0.x, c1.y - c0.y, s_end_raw + eshift, s_prod_raw, s_flag,
                                                    s_wave_key, s_wave_val, carries + tile, pshift, nullptr, nullptr, 0, false, 0, t);
            if (tid == 0) {
                s_next = following;
                if (b == 0) __hip_atomic_store(ba.next + tile, following, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();          // all LDS reads of this tile done before the next tile's staging writes; s_next visible
        }
    }
}

#ifdef MSPMV_DEV
// development: per-phase cycle stamps of the first 16 tiles of every block (ABLATE == 6 variant)
__device__ unsigned long long *g_mspmv_trace = nullptr;
#endif

template <typename V, int BLOCK, int IPT, typename BODY, typename OUT, typename STREAMS, typename MV = V>
__global__ __launch_bounds__(BLOCK, (tile_waves_per_simd<V, BLOCK, IPT, !BODY::PERSIST, BODY::ABLATE == 7>())) void tile_kernel_vec(Params<V, MV> p, const Coord *__restrict__ coords,
                                                                Carry<V> *__restrict__ carries, int num_tiles, int xcd_chunk_log2,
                                                                BandArgs ba)
{
    constexpr bool AXPBY = OUT::AXPBY, NT = STREAMS::NT, BAND = BODY::BAND, TDM = BODY::TDM, PERSIST = BODY::PERSIST, XCD_REMAP = BODY::XCD_REMAP;
    constexpr int ABLATE = BODY::ABLATE;
    constexpr int NW = BLOCK / WAVE;
    constexpr int CPT = IPT / 4 + 1;
    constexpr int SLOTS = CPT * BLOCK * 4;         // >= TILE + 8
    constexpr bool FL = ABLATE != 7;

    __shared__ __attribute__((aligned(16))) typename EndType<FL>::type s_end_raw[SLOTS];
    __shared__ __attribute__((aligned(16))) V s_prod_raw[SLOTS];
    __shared__ unsigned s_flag[SLOTS / 32 + 1];
    __shared__ int s_wave_key[NW];
    __shared__ V s_wave_val[NW];               // ABLATE 7 (development): the per-thread path walk instead
    // BAND: a call that the column-band passes may serve better; the sampled windows decide, here, on the device.  The
    // verdicts are requested now and looked at once the tile's coordinates are there too (one load latency, not two:
    // with the residency capped by LDS every microsecond a block waits before streaming is throughput lost)
    static_assert(std::is_same<V, MV>::value || (!BAND && !TDM), "mixed precision: never the column bands");
    int band_v = 0;
    if constexpr (BAND) {
        static_assert(FL && !PERSIST && ABLATE == 0 && !XCD_REMAP, "band passes: production variant only");
    static_assert(BAND || !TDM, "clock-scheduled bands: a BAND variant");
        band_v = ba.force ? 1 : ba.verdict[threadIdx.x & (WAVE - 1)];
    }
    constexpr bool TRACE = ABLATE == 6;
    int trace_iter = 0;
#ifdef MSPMV_DEV
    unsigned long long *const trace = TRACE ? g_mspmv_trace : nullptr;
#else
    static_assert(ABLATE == 0 && !PERSIST && !XCD_REMAP, "development variants need -DMSPMV_DEV");
    unsigned long long *const trace = nullptr;
#endif
#define MSPMV_TR(i) do { if (TRACE && trace && threadIdx.x == 0 && trace_iter < 16) trace[((size_t) blockIdx.x * 16 + trace_iter) * 8 + (i)] = clock64(); } while (0)

    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];     // x, when it is tiny (p.x_lds)
    const int tid = threadIdx.x;
    if (tid < SLOTS / 32 + 1) s_flag[tid] = 0u;
    const V *const s_x = stage_x_in_lds<V>(p, s_dyn, BLOCK);
    __syncthreads();
    // XCD_REMAP: blocks are dealt round-robin to the 8 XCDs (block b -> XCD
    // b % 8, observed; only speed depends on it); give each XCD's private L2 a
    // contiguous range of tiles.  Bijective for any num_tiles.
    auto physical = [&](int t) {
        if (XCD_REMAP) {
            const int q = num_tiles / 8, r = num_tiles % 8;
            const int xcd = t % 8, idx = t / 8;
            return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        }
        return xcd_chunked_tile(t, num_tiles, xcd_chunk_log2);
    };
    int seq = blockIdx.x;
    if (seq >= num_tiles) return;
    int tile = physical(seq);
    Coord c0 = coords[tile];
    Coord c1 = coords[tile + 1];
    if constexpr (BAND) {
        // (the empty asm pins the order: coordinates requested, THEN the verdict awaited -- left alone the compiler
        // compares it the moment it is loaded, a full memory latency at the head of every block.  Measured on a banded
        // 99 M-nonzero matrix the passes do not serve: +8 us per call that way, +2 us this way.)
        asm volatile("" : "+s"(c0.x), "+v"(band_v));
        if (__popcll(__ballot(band_v != 0)) >= BAND_MAJORITY) {
            if constexpr (TDM) {
                // clock-scheduled column bands (mspmv_tdm.hpp): one tile per block as in the ordinary body, the x gathers band by band
                // (a kernel of its own, chosen by the host: with the passes in the same kernel the scalar registers do not go round)
                __shared__ int s_tdm_start[TDM_MAX_BANDS + 1];
                p.x_lds = 0;
                TileRegs<V, BLOCK, IPT> tregs;
                // (values by plain 16-byte loads, also where the ordinary body fetches them line by line: the two bodies then share no
                //  loads, the ordinary one compiles as it does in the kernel of the passes, and this one needs no lane swaps)
                asm volatile("" : "+s"(p.nnz));       // (nothing of this body is merged with the ordinary one's)
                constexpr bool VALS = true, LINEWISE_OK = false;
#ifdef MSPMV_DEV
                // development: eight wall-clock stamps per block (the buffer of mspmv_dev_set_trace: 8 words per tile; tools/trace_tiles.py clocked)
                unsigned long long *const tdm_tr = g_mspmv_trace ? g_mspmv_trace + (size_t) blockIdx.x * 8 : nullptr;
                if (tdm_tr && threadIdx.x == 0) tdm_tr[0] = wall_clock64();
#else
                unsigned long long *const tdm_tr = nullptr;
#endif
                issue_nonzero_loads<V, BLOCK, IPT, NT, VALS, LINEWISE_OK>(p, c0, c1, tregs);
                stage_tile_tdm<V, BLOCK, IPT, NT>(p, c0, c1, tregs, s_end_raw, s_prod_raw, (p.nnz & ~3) - 4, ((p.rows + 1) & ~3) - 4, s_flag,
                                                  s_tdm_start, s_wave_key, ba.tdm, (int) threadIdx.x, tdm_tr);
                consume_tile_flags<V, BLOCK, IPT, AXPBY>(p, c0, c1.x - c0.x, c1.y - c0.y, s_end_raw + ((c0.x + 1) - ((c0.x + 1) & ~3)), s_prod_raw, s_flag,
                                                         s_wave_key, s_wave_val, carries + tile, c0.y - (c0.y & ~3));
                if (tdm_tr && threadIdx.x == 0) tdm_tr[7] = wall_clock64();
                return;
            } else {
                // the passes instead: run by the first ba.grid blocks of this launch, the others return
                if ((int) blockIdx.x < ba.grid) {
                    if (!AXPBY) { p.alpha = (V) 1; p.beta = (V) 0; }
                    p.x_lds = 0;
                    run_band_passes<V, BLOCK, IPT, NT>(p, coords, carries, num_tiles, ba, s_end_raw, s_prod_raw, s_flag, s_wave_key, s_wave_val);
                }
                return;
            }
        }
    }
    TileRegs<V, BLOCK, IPT, MV> regs;
    issue_nonzero_loads<V, BLOCK, IPT, NT>(p, c0, c1, regs);
    const int last_full_nz = (p.nnz & ~3) - 4;
    const int last_full_ro = ((p.rows + 1) & ~3) - 4;   // rows + 1 >= 4

    for (;;) {
        const int tile_rows = c1.x - c0.x;
        const int tile_nnz = c1.y - c0.y;
        const int a0 = c0.y & ~3;
        const int pshift = c0.y - a0;
        const int first = c0.x + 1;                // d_row_offsets index of the tile's first row end
        const int i0 = first & ~3;
        const int eshift = first - i0;

        // ---- next tile's coordinates (scalar loads, in flight during the staging)
        const int next_seq = seq + (int) gridDim.x;
        const bool has_next = PERSIST ? next_seq < num_tiles : false;
        const int next = has_next ? physical(next_seq) : tile;
        const Coord n0 = coords[next];
        const Coord n1 = coords[next + 1];
        MSPMV_TR(0);
        if (TRACE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        MSPMV_TR(1);
        stage_tile<V, BLOCK, IPT, NT, FL>(p, c0, c1, tile, num_tiles, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, s_x);
        MSPMV_TR(2);
        // ---- the next tile's nonzero stream goes in flight, then the LDS phases of this tile
        if (has_next) issue_nonzero_loads<V, BLOCK, IPT, NT>(p, n0, n1, regs);
        MSPMV_TR(3);
        if constexpr (ABLATE == 1) {
            // ablation (development): staging only -- keep the LDS data live, skip search/walk/scan
            if (s_prod_raw[tid] == (V) 12345.678 && s_end_raw[tid] == 77) carries[tile].key = 1;
        } else if constexpr (FL)
            consume_tile_flags<V, BLOCK, IPT, AXPBY>(p, c0, tile_rows, tile_nnz, s_end_raw + eshift, s_prod_raw, s_flag,
                                                     s_wave_key, s_wave_val, carries + tile, pshift,
                                                     (TRACE && trace && trace_iter < 16) ? trace + ((size_t) blockIdx.x * 16 + trace_iter) * 8 : nullptr);
        else
            consume_tile_lds<V, BLOCK, IPT, AXPBY, true>(p, c0, tile_rows, tile_nnz, s_end_raw + eshift, s_prod_raw,
                                                            s_prod_raw, s_wave_key, s_wave_val, carries + tile, pshift);
        MSPMV_TR(4);
        if (!has_next) break;
        __syncthreads();          // all LDS reads of this tile done before the next tile's staging writes
        MSPMV_TR(5);
        ++trace_iter;
        seq = next_seq; tile = next; c0 = n0; c1 = n1;
    }
}

// ---------------------------------------------------------------------------
// Fix-up: reduce-by-key over n carry pairs whose keys are non-decreasing;
// y[key] += alpha * sum for key < rows (the guard the reference lacks,
// agent_segment_fixup.cuh:257-259).  ref: DeviceSegmentFixupKernel,
// dispatch_spmv_orig.cuh:198-224.
// Each block owns CHUNK = BLOCK*IPT consecutive pairs.  A segment (run of
// equal keys) lying strictly inside the chunk has a unique owner and is
// applied with a plain read-modify-write.  With more than one block, the
// chunk's first and last segments may continue in the neighbours: they are
// written to out[2*chunk], out[2*chunk+1] (keys stay non-decreasing) and the
// kernel is run again on `out`; the final level has a single block.
// Fixed association order => bitwise reproducible results.
// ---------------------------------------------------------------------------
template <typename V, int BLOCK, int IPT>
__device__ __forceinline__ void fixup_chunk(const Carry<V> *in, int n, int chunk, bool multi, Carry<V> *out, V *y,
                                            int rows, V alpha, int *s_wave_key, V *s_wave_val)
{
    constexpr int CHUNK = BLOCK * IPT;
    const int tid = threadIdx.x;
    const int base = chunk * CHUNK;
    const int key0 = in[base].key;           // base < n by construction of the grid

    int keys[IPT]; V vals[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int i = base + tid * IPT + k;
        if (i < n) { const Carry<V> c = in[i]; keys[k] = c.key; vals[k] = c.value; }
        else { keys[k] = 0x7fffffff; vals[k] = 0; }
    }
    // Thread-local fold.  A thread conceptually starts inside the segment its
    // predecessor ended in (start_key = key of the item just before its range),
    // so that a segment ending exactly at a thread boundary is closed -- with
    // the carry-in of the preceding threads -- by the thread that follows.
    const int first_i = base + tid * IPT;
    int cur = (tid > 0 && first_i - 1 < n) ? in[first_i - 1].key : keys[0];
    if (tid > 0 && first_i - 1 >= n) cur = 0x7fffffff;
    V total = 0;
    int first_key = -1; V first_total = 0; bool have_first = false;
    // Segments this thread closes are collected (slot k = item index that closed them) and
    // applied afterwards in one batch of independent loads followed by the stores: a
    // load-add-store per segment in sequence made each thread wait for up to IPT dependent
    // memory round trips.
    int ekey[IPT]; V esum[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        ekey[k] = -1; esum[k] = 0;
        if (keys[k] != cur) {
            if (!have_first) { have_first = true; first_key = cur; first_total = total; }
            else { ekey[k] = cur; esum[k] = total; }
            cur = keys[k]; total = vals[k];
        } else total += vals[k];
    }
    int prev_key, agg_key; V carry_in, agg_val;
    block_exclusive_rbk<V, BLOCK>(cur, total, s_wave_key, s_wave_val, prev_key, carry_in, agg_key, agg_val);
    int fkey = -1; V fsum = 0;
    if (have_first) { fkey = first_key; fsum = first_total + ((tid > 0 && prev_key == first_key) ? carry_in : (V) 0); }
    // threads whose whole range is one key contributed through the scan only.
    int lkey = -1; V lsum = 0;                         // the chunk's open last segment (last thread)
    if (tid == BLOCK - 1) {
        if (multi) {
            Carry<V> c; c.key = agg_key; c.value = agg_val; out[2 * chunk + 1] = c;
            if (agg_key == key0) { Carry<V> z; z.key = key0; z.value = 0; out[2 * chunk] = z; }
        } else { lkey = agg_key; lsum = agg_val; }
    }
    // a segment with the chunk's first key may continue from the previous chunk: next level
    if (multi && fkey == key0) { Carry<V> c; c.key = fkey; c.value = fsum; out[2 * chunk] = c; fkey = -1; }
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (multi && ekey[k] == key0) { Carry<V> c; c.key = ekey[k]; c.value = esum[k]; out[2 * chunk] = c; ekey[k] = -1; }
    // batched y[key] += alpha * sum (keys of one thread are distinct)
    V old[IPT], fold = 0, lold = 0;
#pragma unroll
    for (int k = 0; k < IPT; ++k) { const bool ok = ekey[k] >= 0 && ekey[k] < rows; old[k] = ok ? y[ekey[k]] : (V) 0; }
    if (fkey >= 0 && fkey < rows) fold = y[fkey];
    if (lkey >= 0 && lkey < rows && lkey != fkey) lold = y[lkey];
#pragma unroll
    for (int k = 0; k < IPT; ++k) if (ekey[k] >= 0 && ekey[k] < rows) y[ekey[k]] = old[k] + alpha * esum[k];
    if (fkey >= 0 && fkey < rows) { fold += alpha * fsum; if (lkey == fkey) fold += alpha * lsum; y[fkey] = fold; }
    if (lkey >= 0 && lkey < rows && lkey != fkey) y[lkey] = lold + alpha * lsum;
}

template <typename V, int BLOCK, int IPT>
__global__ __launch_bounds__(BLOCK) void fixup_kernel(const Carry<V> *__restrict__ in, int n,
                                                      Carry<V> *__restrict__ out, V *__restrict__ y, int rows,
                                                      V alpha)
{
    constexpr int NW = BLOCK / WAVE;
    __shared__ int s_wave_key[NW];
    __shared__ V s_wave_val[NW];
    fixup_chunk<V, BLOCK, IPT>(in, n, blockIdx.x, gridDim.x > 1, out, y, rows, alpha, s_wave_key, s_wave_val);
}

// ---------------------------------------------------------------------------
// One-launch fix-up.  Same reduce-by-key over the carry pairs, but every segment (maximal run of
// equal keys) is owned by the block whose chunk holds its FIRST pair: that block sums the part
// inside its chunk (thread-local fold + one block scan, as above) and, when the run continues
// past the chunk end, reads on until the key changes -- keys are non-decreasing, so the run is
// contiguous; this only happens for rows that span several tiles.  A block skips the leading
// pairs of its chunk that continue a run begun earlier.  Every y[key] therefore has exactly one
// writer and a fixed association order (bitwise reproducible), with no second level: one launch
// instead of two or three, ~5 us less on every call.
// ---------------------------------------------------------------------------
template <typename V, int BLOCK, int IPT>
__global__ __launch_bounds__(BLOCK) void fixup_onepass_kernel(const Carry<V> *__restrict__ in, int n, V *__restrict__ y,
                                                              int rows, V alpha)
{
    constexpr int CHUNK = BLOCK * IPT;
    constexpr int NW = BLOCK / WAVE;
    __shared__ int s_wave_key[NW];
    __shared__ V s_wave_val[NW];
    __shared__ int s_need;
    const int tid = threadIdx.x;
    const int base = blockIdx.x * CHUNK;
    const int key_before = base > 0 ? in[base - 1].key : -1;       // -1: no run continues into this chunk (keys are >= 0)

    int keys[IPT]; V vals[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int i = base + tid * IPT + k;
        if (i < n) { const Carry<V> c = in[i]; keys[k] = c.key; vals[k] = c.value; }
        else { keys[k] = 0x7fffffff; vals[k] = 0; }
    }
    const int first_i = base + tid * IPT;
    int cur = tid == 0 ? key_before : (first_i - 1 < n ? in[first_i - 1].key : 0x7fffffff);   // the run this thread starts inside
    if (tid == BLOCK - 1) {
        // does the chunk's last run continue in the next chunk, and is it ours (begun in this chunk)?
        const int last_key = keys[IPT - 1];
        const int next_i = base + CHUNK;
        s_need = (next_i < n && last_key != key_before && last_key < rows && in[next_i].key == last_key) ? 1 : 0;
    }
    V total = 0;
    int first_key = -1; V first_total = 0; bool have_first = false;
    int ekey[IPT]; V esum[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        ekey[k] = -1; esum[k] = 0;
        if (keys[k] != cur) {
            if (!have_first) { have_first = true; first_key = cur; first_total = total; }
            else { ekey[k] = cur; esum[k] = total; }
            cur = keys[k]; total = vals[k];
        } else total += vals[k];
    }
    int prev_key, agg_key; V carry_in, agg_val;
    block_exclusive_rbk<V, BLOCK>(cur, total, s_wave_key, s_wave_val, prev_key, carry_in, agg_key, agg_val);
    int fkey = -1; V fsum = 0;
    if (have_first) { fkey = first_key; fsum = first_total + ((tid > 0 && prev_key == first_key) ? carry_in : (V) 0); }
    if (fkey == key_before) fkey = -1;                 // that run began in an earlier chunk: its owner adds these pairs
    // the chunk's open last run (last thread); its continuation beyond the chunk, if any
    int lkey = -1; V lsum = 0;
    if (tid == BLOCK - 1 && agg_key != key_before) { lkey = agg_key; lsum = agg_val; }
    if (s_need) {                                      // block-uniform (written before the scan's barrier)
        const int akey = in[base + CHUNK].key;
        V part = 0;
        // 16 independent loads per thread and round (a round costs one memory latency whatever
        // its width): a run of 24 000 pairs -- one row spanning 24 000 tiles -- takes 6 rounds
        constexpr int U = 16;
        for (int pos = base + CHUNK;; pos += U * BLOCK) {
            Carry<V> c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = pos + tid + u * BLOCK;
                if (i < n) c[u] = in[i]; else { c[u].key = -2; c[u].value = 0; }
            }
            bool ended = false;
#pragma unroll
            for (int u = 0; u < U; ++u) { if (c[u].key == akey) part += c[u].value; else ended = true; }
            if (__syncthreads_or(ended ? 1 : 0)) break;
        }
        // block sum in a fixed order: wave scan, then the wave totals in wave order
        const V wsum = wave_segmented_inclusive_sum<V>(0, part);
        __syncthreads();                               // s_wave_val is free again
        if ((tid & (WAVE - 1)) == WAVE - 1) s_wave_val[tid / WAVE] = wsum;
        __syncthreads();
        if (tid == BLOCK - 1) {
            V ext = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) ext += s_wave_val[w];
            lsum += ext;
        }
    }
    // batched y[key] += alpha * sum (the keys of one thread are distinct; every key has one owner)
    V old[IPT], fold = 0, lold = 0;
#pragma unroll
    for (int k = 0; k < IPT; ++k) { const bool ok = ekey[k] >= 0 && ekey[k] < rows; old[k] = ok ? y[ekey[k]] : (V) 0; }
    if (fkey >= 0 && fkey < rows) fold = y[fkey];
    if (lkey >= 0 && lkey < rows) lold = y[lkey];
#pragma unroll
    for (int k = 0; k < IPT; ++k) if (ekey[k] >= 0 && ekey[k] < rows) y[ekey[k]] = old[k] + alpha * esum[k];
    if (fkey >= 0 && fkey < rows) y[fkey] = fold + alpha * fsum;
    if (lkey >= 0 && lkey < rows) y[lkey] = lold + alpha * lsum;
}

// ---------------------------------------------------------------------------
// ONE launch for problems of any size: tile_kernel_snap (the default of every call that the vectorised staging can serve,
// and that is not a candidate for the column-band passes).  No coordinate launch,
// no fix-up launch, no dependency between workgroups except for rows longer than HEAD_MAX.
//  * COORDINATES ARE HINTS, VERIFIED.  The point (x, y) of a tile boundary is characterised by two row offsets:
//    row_offsets[x] <= y <= row_offsets[x + 1].  A tile therefore takes whatever the caller's temp storage holds for its
//    two boundaries -- left there by an earlier call on the same matrix, by mspmv_csrmv_prepare, or garbage --, starts
//    streaming on that assumption, and checks the four row offsets that decide it (requested first, so they are back
//    before the nonzeros).  Right (every call but the first on a given temp buffer): the tile has paid what a stored
//    coordinate costs, one cached load, and the call has no coordinate pass at all.  Wrong: waves 0 and 1 search the two
//    boundaries (wave_merge_path_guess: one window of row offsets around the arithmetic guess on a regular matrix, the
//    64-ary sampled search on any other), the tile is staged again, and the corrected hints are stored for the next call.
//    Nothing depends on the hints being right, so the call stays stateless in the reference's sense (temp storage is
//    scratch); what a second call on the same buffer saves is the search, 8-19 us per call as a launch of its own.
//  * ROW-SNAPPED TILES: no carries, every y[r] written exactly once.  A merge-path boundary falls inside some row x,
//    `head` nonzeros after the row's first one.  When head <= HEAD_MAX the boundary is moved back to the row's first
//    nonzero: the tile BEFORE it stops at the end of its last complete row and the tile AFTER it also multiplies those
//    <= HEAD_MAX nonzeros -- both sides decide from the same two numbers, so they agree.  Tiles stay merge-path tiles
//    (their work differs by at most HEAD_MAX items, 5-10 % of a tile; LDS has that much room in every compiled shape), but
//    a matrix of short rows -- every grid, band, dense-block or FEM matrix -- has no row left open at any tile end:
//    nothing to publish, nothing to wait for, nothing to fix up.
//  * Long rows (head > HEAD_MAX): the tiles holding a piece of the row publish their partial sums
//    as tagged records and the tile in which the row ENDS takes exactly those (up to 64 by wave 0 alone, longer lists by
//    the whole block, 8 records per thread and round), adds them in a fixed order and clears them.  A publisher never
//    waits before it publishes, so there are no chains; a waiting tile needs lower-numbered TILES to have been dispatched,
//    which the block -> tile mapping guarantees as long as one of its XCD runs fits the resident blocks twice over
//    (mspmv_api.hip: safe_chunk_log2) -- and otherwise recomputes the missing sum itself after a bounded poll, so the call
//    never depends on another workgroup's progress.  Deterministic and bitwise reproducible (a recomputed sum is the one
//    re-association that can differ): the result does not depend on whether the hints were right.
//  * Closed tiles of short rows take the lean row-by-row reduction (consume_tile_rows) instead of flags + scan.
// ---------------------------------------------------------------------------
// Merge-path point of a diagonal WITHOUT a coordinate pass and, on a regular matrix, at the price of the one memory round
// trip that loading a stored coordinate costs: the row is guessed arithmetically -- x ~ diagonal * rows / (rows + nnz),
// exact when every row has the same length -- and the wave looks at the 64 rows around the guess (two cache lines of
// row_offsets, which the tile is about to read anyway).  M(p) = row_end[p] + p + 1 is strictly increasing and the point
// is the first p with M(p) > diagonal, so the window holds the answer iff its first row fails the test (or the window
// starts at row 0) and some row passes it.  Otherwise the window's own slope gives a second guess (a matrix whose row
// lengths vary smoothly: grids, bands, FEM meshes), and if that window misses as well the 64-ary search over fixed
// samples runs (wave_merge_path_search_interp: any matrix, 3-4 dependent loads).  Exact; all lanes return the same
// point; row_start = row_offsets[x], the first nonzero of the row the point falls in.
__device__ __forceinline__ Coord wave_merge_path_guess(int diagonal, const int *__restrict__ row_end, int rows, int nnz, int &row_start)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int inf = rows + nnz + 1;                                  // < 2^31
    long long g = (long long) diagonal * rows / ((long long) rows + nnz);
    for (int attempt = 0; attempt < 2; ++attempt) {
        int w0 = (int) g - WAVE / 2;
        const int w_max = rows - (WAVE - 1) > 0 ? rows - (WAVE - 1) : 0;
        w0 = w0 < 0 ? 0 : w0 > w_max ? w_max : w0;
        const int p = w0 + lane;
        const int e = p < rows ? row_end[p] : 0;
        const int m = p < rows ? e + p + 1 : inf;                    // (p == rows: M = +inf)
        const unsigned long long mask = __ballot(m > diagonal);
        const bool first_fails = !(mask & 1ull);
        if (mask != 0ull && (first_fails || w0 == 0)) {
            const int f = __ffsll((long long) mask) - 1;
            const int x = w0 + f;                                    // <= rows
            // row_offsets[x] = row_end[x - 1]: in the window unless x == w0 (then w0 == 0: row 0 starts at 0)
            row_start = f > 0 ? __shfl(e, f - 1, WAVE) : 0;
            Coord c; c.x = x < rows ? x : rows; c.y = diagonal - c.x;
            if (x >= rows) row_start = nnz;
            return c;
        }
        if (mask == 0ull && w0 + WAVE >= rows) break;                // (cannot happen: lane of p == rows always passes) -- fall back
        // second guess from the window's slope
        const int m_a = __shfl(m, 0, WAVE), m_b = __shfl(m, WAVE - 1, WAVE);
        if (m_b >= inf || m_b <= m_a) break;
        g = w0 + (long long) ((double) (diagonal - m_a) * (double) (WAVE - 1) / (double) (m_b - m_a));
        if (g < 0) g = 0; if (g > rows) g = rows;
    }
    const Coord c = wave_merge_path_search_interp(diagonal, row_end, rows, nnz);
    row_start = c.x >= rows ? nnz : c.x > 0 ? row_end[c.x - 1] : 0;
    return c;
}

template <int BLOCK, int IPT>
constexpr int snap_head_max()
{
    constexpr int slack = (IPT / 4 + 1) * BLOCK * 4 - BLOCK * IPT - 16;
    return slack < 192 ? slack : 192;
}

// ---------------------------------------------------------------------------
// COMPACT FRONT END of the one-launch kernel, for problems of ONE BLOCK GENERATION (mspmv_api.hip: compact_max_tiles).
// The reference special-cases small problems too (dispatch_spmv_orig.cuh:674-679: one tile -> no search, no fix-up;
// agent_spmv_orig.cuh:867-891).  Below a few hundred tiles a call is one generation of blocks that each run alone on their CU:
// what it costs is the block's dependent memory trips (hints -> streams -> x) PLUS ONE INSTRUCTION PER ~5 CYCLES of a lone wave and
// every stretch of code the block has to fetch -- the general kernel issues ~440 instructions per wave on its likeliest path
// (hints, checks for every shape of tile, 16-bit row ends, row-start bits, the two-rows-at-a-time lean reduction) out of 19-37 KB
// of code.  This front end is that likeliest path and nothing else, written for instruction count (~200 per wave, ~2 KB of
// straight-line code at the head of the kernel):
//   * the tile is the block index (no XCD chunking: a generation that is resident all at once gains nothing from it);
//   * hints by two scalar loads; the tile is taken here only if they describe a CLOSED LEAN tile (exactly the tiles the general
//     kernel hands to consume_tile_rows) whose every speculative access stays inside the arrays and LDS -- anything else (no usable
//     hints yet, a long row, x in LDS, hints that fail the four-word verification) returns false BEFORE anything but LDS and registers
//     was touched, and the block runs the general body from its start: the compact kernel is complete, this is only its fast lane;
//   * CSR chunks are clamped to the last full chunk of their array (min, no branch); the one ragged chunk an array can end with is
//     re-aligned in a wave-uniform, rarely taken branch -- so the LAST tile of a problem stays in the fast lane (a launch is as slow
//     as its slowest block);
//   * row offsets go to LDS as they are (32 bits, x0 .. x1: a row's start and end are ONE ds_read2_b32), products at their raw
//     positions; ONE barrier;
//   * a thread sums a row left to right from +0.0 -- the first eight products under a shrinking EXEC mask (v_cmpx + v_add per
//     product instead of compare + select + add), nine to sixteen the same way in a second batch, longer rows by the 16 lanes of a
//     DPP row exactly as consume_tile_rows does: THE SAME ADDITIONS IN THE SAME ORDER, so y is bit for bit what the general kernel
//     writes (tests/test_gpu_parity.py: the `compact` paths; tools/fuzz.py).
// ---------------------------------------------------------------------------
constexpr int COMPACT_BLOCK = 256, COMPACT_IPT = 7;
// element i of a chunk that was loaded `s` elements too early (the last, ragged chunk of an array is fetched at n - 4): what
// belongs at position i is what was loaded at position i + s (positions that fall off the end are never used)
template <typename T>
__device__ __forceinline__ void compact_realign(Vec4<T> &c, int s)
{
    T l[4], o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) l[i] = c.get(i);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int j = i + s; o[i] = j <= 0 ? l[0] : j == 1 ? l[1] : j == 2 ? l[2] : l[3]; }
    if constexpr (sizeof(T) == 8) { c.a[0] = o[0]; c.a[1] = o[1]; c.b[0] = o[2]; c.b[1] = o[3]; }
    else { c.v[0] = o[0]; c.v[1] = o[1]; c.v[2] = o[2]; c.v[3] = o[3]; }
}
// (the ragged chunk sits at n - 4, which need not be 16-byte aligned: dword-aligned 16-byte global loads are fine on gfx9; the
//  packed attribute keeps the compiler from assuming more)
typedef int int4v_u __attribute__((ext_vector_type(4), aligned(4)));
typedef float float4v_u __attribute__((ext_vector_type(4), aligned(4)));
typedef double double2v_u __attribute__((ext_vector_type(2), aligned(8)));
typedef int int2v_u __attribute__((ext_vector_type(2), aligned(4)));

// loads through a 32-bit unsigned BYTE offset from a uniform base (global_load ... v_off, s[base]: one shift, no 64-bit address
// arithmetic per lane).  The dispatcher takes the compact kernel only when every array is < 4 GB (mspmv_api.hip).
template <typename T>
__device__ __forceinline__ T compact_ld(const void *base, unsigned byte_off)
{
    return *reinterpret_cast<const T *>(static_cast<const char *>(base) + byte_off);
}
__device__ __forceinline__ Vec4<int> compact_ld4(const int *base, int e) { Vec4<int> r; r.v = compact_ld<int4v_u>(base, (unsigned) e << 2); return r; }
__device__ __forceinline__ Vec4<float> compact_ld4(const float *base, int e) { Vec4<float> r; r.v = compact_ld<float4v_u>(base, (unsigned) e << 2); return r; }
__device__ __forceinline__ Vec4<double> compact_ld4(const double *base, int e)
{
    Vec4<double> r; r.a = compact_ld<double2v_u>(base, (unsigned) e << 3); r.b = compact_ld<double2v_u>(base, ((unsigned) e << 3) + 16u); return r;
}

// Written for the ORDER OF ITS CODE as much as for its instruction count: the translation unit that instantiates the compact kernel
// (mspmv_compact.hip) is compiled with the block placement pass off, so the machine code keeps the order of this source -- the
// fast lane from the hint request to its s_endpgm in one piece, what is rarely needed (the ragged end of the nonzero arrays, tiles
// of more than 511 rows, rows of more than 8 nonzeros) behind it, reached by `goto` and left by `goto`.
template <typename V, bool AXPBY>
__device__ __forceinline__ void compact_front(const Coord *coords, const int *rstart, int num_tiles, const Params<V> &p,
                                              Carry<V> *__restrict__ carries, int lean_avg, int tile, V *s_prod, int *s_ro, int4v &hc, int2v &hr)
{
    constexpr int BLOCK = COMPACT_BLOCK, IPT = COMPACT_IPT, TILE = BLOCK * IPT, CPT = IPT / 4 + 1;
    constexpr int HEAD_MAX = snap_head_max<BLOCK, IPT>();
    constexpr int RO_ROUNDS = (TILE + 1 + BLOCK - 1) / BLOCK;         // row offsets x0 .. x1, one per lane and round: <= 8 rounds
    static_assert(CPT == 2 && TILE + HEAD_MAX + 16 <= CPT * BLOCK * 4 && RO_ROUNDS * BLOCK <= CPT * BLOCK * 4, "two chunks per thread; room for the snapped rows");
    static_assert(LEAN_SERIAL == 2 * LEAN_BATCH && LEAN_BATCH == 8, "two batches of eight");
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    // (everything the cold sections at the end touch is declared up here: a goto may not jump past an initialisation)
    Vec4<int> col[CPT]; Vec4<V> val[CPT];
    int rov[RO_ROUNDS];
    int r0, r, start, len; bool valid; V acc; const V *src;
    int2v vw0 = {0, 0}, vw1 = {0, 0};
    __shared__ int s_verdict;
    // ---- hints (scalar cache; the tile index is uniform).  Request and wait in ONE asm statement (see tile_kernel_snap).  They go
    // back to the caller: a tile that is not taken runs the general body on THESE registers instead of waiting for the same 24 bytes again
    asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(hc), "=&s"(hr) : "s"(coords + tile), "s"(rstart + tile) : "memory");
    // (used in this very basic block: the kernel-argument loads are requested before the wait above)
    asm volatile("" :: "s"(p.row_end), "s"(p.cols), "s"(p.values), "s"(p.x), "s"(p.y), "s"(p.rows), "s"(p.nnz), "s"(p.x_lds), "s"(lean_avg), "s"(carries));
    const int x0 = hc.x, x1 = hc.z, rs0 = hr.x, rs1 = hr.y;
    const int total = p.rows + p.nnz;                                  // < 2^31
    const int d0 = tile * TILE, d1 = d0 + TILE < total ? d0 + TILE : total;
    const int y0 = d0 - x0, y1 = d1 - x1;
    const int tile_rows = x1 - x0, tile_nnz = rs1 - rs0;
    // A closed lean tile (exactly the general kernel's `lean`: both boundaries snap, nonzeros <= lean_avg * rows) -- judged on the HINTS,
    // which may hold anything: what keeps every access before the verdict inside the arrays is 0 <= x0, x1 <= rows and 0 <= rs0 <= nnz
    // (chunk addresses are clamped from above, row-offset indices lie in [x0, x1], LDS is written at thread positions only); the
    // verdict then either proves the hints to be THE merge-path points of d0 and d1 -- and with them everything else assumed here:
    // x0 <= x1, rs0 <= rs1 <= nnz, the tile's sizes -- or sends the block to the general body before LDS is read or y written.
    // (x in memory and more than one tile: the dispatcher launches this variant only then)
    const bool take = ((unsigned) (y0 - rs0) <= (unsigned) HEAD_MAX) & ((unsigned) (y1 - rs1) <= (unsigned) HEAD_MAX) &
                      ((unsigned) x0 <= (unsigned) p.rows) & ((unsigned) x1 <= (unsigned) p.rows) & ((unsigned) rs0 <= (unsigned) p.nnz) &
                      ((unsigned) tile_nnz <= (unsigned) lean_avg * (unsigned) tile_rows);
    // ONE way out to the general body (the caller's code behind this function): `go` stays 0 when the tile is not taken or its hints
    // fail the verification, and is tested once, after the staging -- two exits would be merged by the compiler through flag
    // variables and a common block at the far end of the kernel, which puts two far jumps into the fast lane
    int go = 0;
    const int *__restrict__ row_offsets = p.row_end - 1;
    const int a0 = rs0 & ~3;
    const int nz4 = p.nnz - 4;                                          // (nnz >= 4 on this path)
    const int a0c = a0 < nz4 ? a0 : nz4;
    const int n_ro = tile_rows + 1;
    const int wave_base = __builtin_amdgcn_readfirstlane(tid) & ~(WAVE - 1);
    const bool live1 = a0 + 4 * (wave_base + BLOCK) < rs1;             // wave-uniform (scalar): see the nonzero loads below
    if (__builtin_expect(!take, 0)) goto staged;
    // ---- the four row offsets that decide whether (x0, rs0), (x1, rs1) are the points of diagonals d0, d1: two scalar loads of the
    // pairs row_end[x - 1], row_end[x] (uniform addresses; row_end[-1] = row_offsets[0] exists, and a boundary at x == rows reads
    // the pair one lower), requested first, looked at in the shadow of the gathers
    // (by the block's FIRST WAVE alone: its verdict reaches the others through one LDS word behind the staging barrier that is there
    //  anyway -- two vector-memory requests and ~25 scalar instructions fewer in three of the four waves)
    if (wave_base == 0) {
        const int b0 = x0 - 1 < p.rows - 2 ? x0 - 1 : p.rows - 2, b1 = x1 - 1 < p.rows - 2 ? x1 - 1 : p.rows - 2;      // (rows >= 3)
        // (plain loads on uniform addresses of memory the kernel has not written: the compiler makes them s_load_dwordx2 and keeps
        //  track of them itself -- a hand-issued scalar load whose wait sits in another asm statement leaves its destination
        //  registers open to copies while the load is in flight)
        vw0 = *reinterpret_cast<const int2v_u *>(p.row_end + b0);
        vw1 = *reinterpret_cast<const int2v_u *>(p.row_end + b1);
    }
    // ---- the tile's nonzeros: 4-element chunks aligned in array index space, clamped to the array's last full chunk.
    // A WAVE whose second chunk lies past the tile altogether (a tile of 5-point rows fills 1500 of the 2048 slots: waves 2 and 3)
    // issues nothing for it -- no stream loads, no gathers, no products: a redirected load costs no bytes, but it costs the CU's
    // vector-memory pipeline the same cycles, and that pipeline is what several tiles on one CU queue on
    {
        const int e = a0 + 4 * tid;
        const int ee = e < rs1 ? (e < nz4 ? e : nz4) : a0c;             // (a chunk past the tile re-reads the tile's first: no bytes for data it does not use)
        col[0] = compact_ld4(p.cols, ee);
        val[0] = compact_ld4(p.values, ee);
    }
    if (live1) {
        const int e = a0 + 4 * (tid + BLOCK);
        const int ee = e < rs1 ? (e < nz4 ? e : nz4) : a0c;
        col[1] = compact_ld4(p.cols, ee);
        val[1] = compact_ld4(p.values, ee);
    }
    // ---- row offsets x0 .. x1 (a row's start and end both come from here), one per lane and round: no alignment, no ragged end
    rov[0] = compact_ld<int>(row_offsets, (unsigned) (x0 + (tid < n_ro ? tid : 0)) << 2);
    // (a round is taken by the waves that have entries in it: a tile of 300 rows has 45 in the second round, all in the first wave)
    if (wave_base + BLOCK < n_ro) rov[1] = compact_ld<int>(row_offsets, (unsigned) (x0 + (tid + BLOCK < n_ro ? tid + BLOCK : 0)) << 2);      // wave-uniform
    if (__builtin_expect(2 * BLOCK < n_ro, 0)) goto more_row_offsets;
have_row_offsets:
    // the one ragged chunk the nonzero arrays can end with was fetched at nnz - 4: its elements are put where they belong
    if (__builtin_expect(((rs1 + 3) & ~3) > p.nnz, 0)) goto ragged_end;
aligned:
    {
        // ---- x gathers
        V xv[CPT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[0][i] = compact_ld<V>(p.x, (unsigned) col[0].get(i) * (unsigned) sizeof(V));
        if (live1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[1][i] = compact_ld<V>(p.x, (unsigned) col[1].get(i) * (unsigned) sizeof(V));
        }
        // ---- the verdict on the hints, in the shadow of the gathers (scalar: v_readlane).  Acted upon after the barrier -- a branch
        // here would hold the gathers back behind it --: until then nothing but registers and LDS is touched
        if (wave_base == 0) {
        const int before0 = x0 == p.rows ? vw0.y : vw0.x, at0 = vw0.y, before1 = x1 == p.rows ? vw1.y : vw1.x, at1 = vw1.y;
        // (x, rs) is the point of diagonal d  <=>  rs == row_offsets[x] <= y = d - x  and  (x == rows ? d == total : y <= row_offsets[x + 1])
        // (written with integer selects: the tests stay on the scalar unit); and the stored y's are the derived ones (what
        //  mspmv_debug_read_tiles reports)
        const int lim0 = x0 < p.rows ? at0 : (d0 == total ? 0x7fffffff : -1);
        const int lim1 = x1 < p.rows ? at1 : (d1 == total ? 0x7fffffff : -1);
        const bool verdict = ((x0 > 0 ? before0 : 0) == rs0) & (y0 <= lim0) & ((x1 > 0 ? before1 : 0) == rs1) & (y1 <= lim1) & (hc.y == y0) & (hc.w == y1);
        if (lane == 0) s_verdict = verdict ? 1 : 0;
        }
        // (nothing open at the end of a closed tile: what mspmv_debug_read_tiles reports.  By the last wave, here in the shadow of the
        //  gathers; a tile that fails the verdict has it overwritten by the general body)
        if (__builtin_amdgcn_readfirstlane(tid) >= BLOCK - WAVE) { if (tid == BLOCK - 1) { Carry<V> c; c.key = x1; c.value = (V) 0; carries[tile] = c; } }
        // ---- LDS: row offsets as they are, products at their raw positions (element e of the array -> slot e - a0)
        s_ro[tid] = rov[0];
        if (wave_base + BLOCK < n_ro) s_ro[tid + BLOCK] = rov[1];
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (k == 0 || live1) {                                      // (slots of a chunk nobody staged are never a row's products: reads past a row's end are discarded)
                V prod[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) prod[i] = val[k].get(i) * xv[k][i];
                st_lds4(&s_prod[4 * (tid + k * BLOCK)], prod);
            }
        __syncthreads();
        go = s_verdict;
    }
staged:
    asm volatile("" : "+v"(go));                                       // (opaque: the test below is not threaded back into the two places `go` comes from)
    go = __builtin_amdgcn_readfirstlane(go);
    if (__builtin_expect(go == 0, 0)) return;                          // (every wave alike; the general body starts from scratch)
    // ---- row by row: consume_tile_rows' arithmetic (left to right from +0.0; > LEAN_SERIAL: 16-lane groups), one row per thread and round
    r0 = wave_base;                                                    // (the wave's first row of the round: scalar -- the compiler has to SEE that the test below is wave-uniform)
next_round:
    // (the wave's program ENDS here -- s_endpgm, not a return: a return value is merged with the general body's exit and the
    //  reduction then sits behind two far jumps.  The test has to be visibly wave-uniform for the same reason: an exit the compiler
    //  takes for divergent is routed through flag variables and a common exit block)
    if (r0 >= tile_rows) __builtin_amdgcn_endpgm();                    // this wave's rows are done
    r = r0 + lane;
    valid = r < tile_rows;
    {
        const int rr = valid ? r : 0;                                   // (row 0 exists: tile_rows > 0 here)
        start = s_ro[rr]; const int end = s_ro[rr + 1];
        len = valid ? end - start : 0;
        src = s_prod + (start - a0);                                   // (start - a0 + 15 < SLOTS for any lane)
        // THE PRODUCT READS ARE WHAT THE LANE WAITS FOR: lanes a row apart read 8-byte words 32 bytes (rows of 4) or 64 bytes (rows of 8)
        // apart, 4 or 2 distinct bank groups for the 16 lanes of an LDS cycle -- SQ_LDS_BANK_CONFLICT is 65 % of the LDS cycles of a
        // 5-point grid's call, and the LDS is busy for ~3/4 of such a kernel (profiles/r05_lds_counters.txt).  So a wave none of whose rows
        // has more than four products (wave-uniform: one ballot) reads and adds the first four only.  (A third level -- six -- for rows of
        // 5 and 6, whose strides conflict far less, measured no gain: profiles/r05_ab_half_batch.txt.)
        V v[LEAN_BATCH];
        const bool more = __ballot(len > LEAN_BATCH / 2) != 0ull;
#pragma unroll
        for (int j = 0; j < LEAN_BATCH / 2; ++j) v[j] = src[j];
        acc = (V) 0;
        if (more) {
#pragma unroll
            for (int j = LEAN_BATCH / 2; j < LEAN_BATCH; ++j) v[j] = src[j];
            CompactChain<V>::add8(acc, v, len, 0);
        } else {
            const V h[4] = {v[0], v[1], v[2], v[3]};
            CompactChain<V>::add4(acc, h, len);
        }
    }
    if (__builtin_expect(__ballot(len > LEAN_BATCH) != 0ull, 0)) goto longer_rows;
store_row:
    if (valid) {
        V *__restrict__ y = p.y + x0;
        if (AXPBY) y[r] = p.alpha * acc + (p.beta == (V) 0 ? (V) 0 : p.beta * y[r]);
        else y[r] = acc;
    }
    r0 += BLOCK;
    goto next_round;

    // ======== what is rarely needed ========
more_row_offsets:                                                      // tiles of more than 511 rows (rows that average < 3.5 nonzeros)
#pragma unroll
    for (int k = 2; k < RO_ROUNDS; ++k)
        if (k * BLOCK < n_ro) rov[k] = compact_ld<int>(row_offsets, (unsigned) (x0 + (tid + k * BLOCK < n_ro ? tid + k * BLOCK : 0)) << 2);
#pragma unroll
    for (int k = 2; k < RO_ROUNDS; ++k)
        if (k * BLOCK < n_ro) s_ro[tid + k * BLOCK] = rov[k];           // (the barrier of the fast lane follows)
    goto have_row_offsets;
ragged_end:
#pragma unroll
    for (int k = 0; k < CPT; ++k)
        if (k == 0 || live1) {
            const int e = a0 + 4 * (tid + k * BLOCK);
            const int s = (e < rs1 && e > nz4) ? e - nz4 : 0;
            if (__ballot(s != 0) != 0ull) { compact_realign(col[k], s); compact_realign(val[k], s); }
        }
    goto aligned;
longer_rows:
    {
        // (a lane index the compiler cannot hoist out of the round loop: everything derived from it -- the DPP groups' bookkeeping --
        //  stays down here instead of being computed ahead of the fast lane's loop)
        int lane_c = tid; asm volatile("" : "+v"(lane_c)); lane_c &= WAVE - 1;
        V w[LEAN_BATCH];
#pragma unroll
        for (int j = 0; j < LEAN_BATCH; ++j) w[j] = src[LEAN_BATCH + j];
        CompactChain<V>::add8(acc, w, len, LEAN_BATCH);
        // rows longer than LEAN_SERIAL: the code consume_tile_rows runs for them
        if (__ballot(len > LEAN_SERIAL) != 0ull) lean_long_rows<V>(s_prod, start - a0, len, lane_c, acc);
    }
    goto store_row;
}

template <typename V, int BLOCK, int IPT, typename BODY, typename OUT, typename STREAMS, typename MV = V>
__global__ __launch_bounds__(BLOCK, (BODY::COMPACT ? 4 : tile_waves_per_simd<V, BLOCK, IPT, true>())) void tile_kernel_snap(Coord *__restrict__ coords, int *__restrict__ rstart,
                                                           int num_tiles, int xcd_chunk_log2,
                                                           Params<V, MV> p, Carry<V> *__restrict__ carries, LookBack lb, int lean_avg)
{
    constexpr bool AXPBY = OUT::AXPBY, NT = STREAMS::NT, COMPACT = BODY::COMPACT;
    constexpr int TILE = BLOCK * IPT;
    constexpr int NW = BLOCK / WAVE;
    constexpr int CPT = IPT / 4 + 1;
    constexpr int SLOTS = CPT * BLOCK * 4;
    constexpr int HEAD_MAX = snap_head_max<BLOCK, IPT>();
    static_assert(HEAD_MAX >= 64 && TILE + HEAD_MAX + 16 <= SLOTS, "room for the snapped rows");
    // (COMPACT: the fast lane's 32-bit row offsets and the general body's 16-bit row ends share one array -- a block uses one of the two)
    __shared__ __attribute__((aligned(16))) int s_end_words[COMPACT ? SLOTS : SLOTS / 2];
    end16_t *const s_end_raw = reinterpret_cast<end16_t *>(s_end_words);
    __shared__ __attribute__((aligned(16))) V s_prod_raw[SLOTS];
    __shared__ unsigned s_flag[SLOTS / 32 + 1];
    __shared__ int s_wave_key[NW];
    __shared__ V s_wave_val[NW];
    __shared__ int s_bnd[6];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];     // x, when it is tiny (p.x_lds)
    // COMPACT (small problems, mspmv_api.hip: compact_max_tiles): the fast lane for closed lean tiles on good hints comes first -- its own LDS layout
    // (32-bit row offsets) in an array of its own, the product array shared --; a tile it does not take runs the general body below
    // from the start, on the hints the front end loaded.  Same tile (compact_tile) in both.
    int4v front_hc = {0, 0, 0, 0}; int2v front_hr = {0, 0};
    if constexpr (COMPACT) {
        static_assert(std::is_same<V, MV>::value, "mixed precision: never the compact front end");
        static_assert(BLOCK == COMPACT_BLOCK && IPT == COMPACT_IPT && !NT, "the compact front end is written for the small tile shape");
        compact_front<V, AXPBY>(coords, rstart, num_tiles, p, carries, lean_avg, compact_tile((int) blockIdx.x, num_tiles, xcd_chunk_log2), s_prod_raw, s_end_words,
                                front_hc, front_hr);      // (a tile it takes ends there)
    }

    const int tid = threadIdx.x;
#ifdef MSPMV_DEV
    // development (tools/trace_snap.py): 100 MHz wall-clock stamps of this block's phases, 8 words per block
    const unsigned long long t_entry = wall_clock64();           // (before the load of the trace pointer: that is a memory round trip)
    unsigned long long *const snap_tr = g_mspmv_trace ? g_mspmv_trace + (size_t) blockIdx.x * 16 : nullptr;     // (8 words of the block + 8 of the lean reduction)
#define MSPMV_SNAP_TR(i) do { if (snap_tr && tid == 0) snap_tr[i] = wall_clock64(); } while (0)
    if (snap_tr && tid == 0) { snap_tr[6] = __builtin_amdgcn_s_getreg(63492); snap_tr[7] = __builtin_amdgcn_s_getreg(6164); }
#else
#define MSPMV_SNAP_TR(i) do { } while (0)
#endif
#ifdef MSPMV_DEV
    if (snap_tr && tid == 0) snap_tr[0] = t_entry;
#endif
    static_assert(sizeof(coords) + sizeof(rstart) + sizeof(num_tiles) + sizeof(xcd_chunk_log2) <= 32, "the four leading arguments lie inside the 8 preloaded dwords");
    // THE FIRST FOUR ARGUMENTS -- all the hint request needs -- are in SGPRs when the wave starts (kernel-argument preload, 8 dwords:
    // the Makefile's -amdgpu-kernarg-preload-count=8), the tile index below is branch-free scalar arithmetic on them, and the other
    // arguments are pinned behind the hint request: the block's first memory round trip is the hints AND the rest of the kernel
    // arguments together, where the arguments (in three batches, as the compiler sank them to their uses) came first.
    const int tile = COMPACT ? compact_tile((int) blockIdx.x, num_tiles, xcd_chunk_log2) : xcd_chunked_tile_flat((int) blockIdx.x, num_tiles, xcd_chunk_log2);
    // the hints: the tile's two boundaries (x, y) and their row starts, read THROUGH THE SCALAR
    // CACHE -- the tile index is uniform, and a scalar load neither queues behind the vector-memory traffic of the CU's other
    // blocks nor needs an LDS hop to reach every wave: 2-6 % on matrices streamed from HBM (grid2d-4096, dense32, band5, C4;
    // same-box A/B in profiles/r03_scalar_hints.txt), and since round 4 in the small tile shape as well (two lanes' vector
    // loads + an LDS broadcast until then): 4.1-4.2 -> 3.8-4.0 us per call below 1 M nonzeros, 19.9 -> 18.0 us at 5.8 M, with
    // the rest of this prologue in 32-bit, branch-free scalar code.  (The hints were written by vector stores of an earlier
    // launch; the scalar cache is invalidated at every kernel start.)  Request and wait are ONE asm statement: the compiler never
    // sees destination registers whose load is still in flight, so it cannot copy, spill or re-assign them under the load (a
    // later, separate s_waitcnt left exactly that open).  What used to sit between the two -- clearing the flag words,
    // requesting a tiny x -- comes first; the block has nothing else to do until its hints are there anyway.
    const bool single = num_tiles == 1;                             // one tile: its boundaries are (0, 0) and (rows, nnz)
    int4v hint_c; int2v hint_r;
    if constexpr (COMPACT) { hint_c = front_hc; hint_r = front_hr; }          // (the compact front end's: it requested them)
    else asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                      : "=&s"(hint_c), "=&s"(hint_r) : "s"(coords + tile), "s"(rstart + tile) : "memory");
    // (uses in this very basic block: the loads of these arguments stay up here, requested before the wait above)
    asm volatile("" :: "s"(p.row_end), "s"(p.cols), "s"(p.values), "s"(p.x), "s"(p.y), "s"(p.rows), "s"(p.nnz), "s"(p.x_lds), "s"(lean_avg),
                 "s"(carries), "s"(lb.rec), "s"(lb.tag_a), "s"(lb.tag_b), "s"(lb.error), "s"(lb.call_tag), "s"(lb.max_polls), "s"(p.band_pass));
    if (tid < SLOTS / 32 + 1) s_flag[tid] = 0u;                     // (the row-start bits)
    // a tiny x goes to LDS: requested now, written after the streams have been requested
    XRegs<V, BLOCK> xr;
    const V *s_x = nullptr;
    if (MSPMV_UNLIKELY((layout_hints<V, IPT>()), p.x_lds > 0)) { request_x_for_lds<V, BLOCK>(p, xr); s_x = reinterpret_cast<const V *>(s_dyn); }
    // (With a tiny x being copied into LDS, every wave requests its share of the streams first and the barrier -- which waits for
    //  that copy -- comes after the requests: dense32 fp32 -3 %, fp64 -6.5 %; without the copy the early barrier is the better
    //  place, by 1-2 %)
    const bool late_barrier = s_x != nullptr;                       // block-uniform
    if constexpr (!layout_hints<V, IPT>()) { if (!late_barrier) __syncthreads(); }      // (the large shapes: see below)
    const LookBack &lbe = lb;
    MSPMV_SNAP_TR(1);
    const int total = p.rows + p.nnz;                               // < 2^31
    // (32-bit: tile < num_tiles = ceil(total / TILE), so tile * TILE < total <= 2^31 - 65537 and adding TILE cannot overflow)
    const int d0 = tile * TILE, d1 = d0 + TILE < total ? d0 + TILE : total;
    const int last_full_nz = (p.nnz & ~3) - 4;
    const int last_full_ro = ((p.rows + 1) & ~3) - 4;
    int x0 = single ? 0 : hint_c.x, rs0 = single ? 0 : hint_r.x, x1 = single ? p.rows : hint_c.z, rs1 = single ? p.nnz : hint_r.y;
    const int hint_y0 = single ? 0 : hint_c.y, hint_y1 = single ? p.nnz : hint_c.w;
    int y0 = d0 - x0, y1 = d1 - x1;
    bool snap0 = y0 - rs0 <= HEAD_MAX, snap1 = y1 - rs1 <= HEAD_MAX;
    Coord c0, c1;
    c0.x = x0; c0.y = snap0 ? rs0 : y0;
    c1.x = x1; c1.y = snap1 ? rs1 : y1;
    // closed tile of short rows (block-uniform; consume_tile_rows): no row-start bits, raw product positions, one LDS phase
    // (unsigned: with garbage hints the product may wrap -- harmless, `lean` is only used once the hints have passed `good`,
    //  and then a tile has at most TILE rows)
    bool lean = snap0 && snap1 && (unsigned) (c1.y - c0.y) <= (unsigned) lean_avg * (unsigned) (c1.x - c0.x);
    // the clearing of the row-start bits is fenced from the staging's ORs by a barrier only in a tile that will use them -- a lean
    // tile neither sets nor reads them, and spares its waves the meeting (3.5-3.7 -> 3.4-3.6 us per small call).  As early as `lean`
    // is known (whatever the hints are worth: hints that fail the checks below send the block through the search, which clears
    // and fences for itself).  In the small shapes only: in the large one the circuit-shaped matrix, a mix of lean and other tiles,
    // was 1 % slower in every variant tried and dense5 / the grids as much faster (same-box A/B, profiles/r04_small_call_lean_barrier.txt)
    if constexpr (layout_hints<V, IPT>()) { if (!lean && !late_barrier) __syncthreads(); }
    // hints: anything may be in there.  Only values that keep every speculative access inside the arrays and the LDS tile
    // are tried at all (block-uniform)
    // 0 <= x0 <= x1 <= rows, 0 <= y0 <= y1 <= nnz, 0 <= rs0 <= y0, rs0 <= rs1 <= y1, as unsigned comparisons without branches (each
    // chain's last link bounds the earlier ones from below by zero); the last: the snapped boundaries in order
    bool good = ((unsigned) x0 <= (unsigned) x1) & ((unsigned) x1 <= (unsigned) p.rows) & ((unsigned) y0 <= (unsigned) y1) &
                ((unsigned) y1 <= (unsigned) p.nnz) & ((unsigned) rs0 <= (unsigned) y0) & ((unsigned) rs0 <= (unsigned) rs1) &
                ((unsigned) rs1 <= (unsigned) y1) & (c1.y >= c0.y);
    // the hints of the next call on this temp storage (and what mspmv_debug_read_tiles returns): stored when they were not there
    auto store_hints = [&](bool found_here) {
        if (tid == 0) {
            if (found_here || single || hint_y0 != y0) { Coord h; h.x = x0; h.y = y0; coords[tile] = h; rstart[tile] = rs0; }
            if (tile == num_tiles - 1 && (found_here || single || hint_y1 != y1)) { Coord h; h.x = x1; h.y = y1; coords[num_tiles] = h; rstart[num_tiles] = rs1; }
        }
    };
    if (MSPMV_LIKELY((layout_hints<V, IPT>()), good)) {
        // the four row offsets that decide whether (x0, rs0) and (x1, rs1) are the points of diagonals d0 and d1: requested
        // BEFORE the tile's streams, so they are back first
        // (by four lanes of EVERY wave: each wave then decides for itself -- all from the same four words, so all alike --
        //  and the verdict needs neither an LDS word nor a barrier of its own)
        int vre = 0;
        const int lane = tid & (WAVE - 1);
        if (lane < 4) {
            int idx = (lane < 2 ? x0 : x1) - 1 + (lane & 1);        // x0 - 1, x0, x1 - 1, x1
            idx = idx < 0 ? 0 : idx >= p.rows ? p.rows - 1 : idx;   // (rows >= 3 on this path)
            vre = p.row_end[idx];
        }
        TileRegs<V, BLOCK, IPT, MV> regs;
        issue_nonzero_loads<V, BLOCK, IPT, NT>(p, c0, c1, regs);
        MSPMV_SNAP_TR(2);
        if (MSPMV_UNLIKELY((layout_hints<V, IPT>()), late_barrier)) { commit_x_to_lds<V, BLOCK>(p, xr, s_dyn); __syncthreads(); }
        // The verdict on the hints: looked at once the tile's x gathers have been requested -- the four words came back before the
        // streams did, and the scalar arithmetic on them runs in the shadow of the gathers (after the staging barrier it was ~100
        // instructions of a lone wave's critical path; before the staging it would hold the wave's share of the streams back).
        // (v_readlane: the four words and everything derived from them are scalars -- a shuffle goes through LDS and leaves vectors)
        bool verdict = true;
        auto check_hints = [&]() {
            const int before0 = __builtin_amdgcn_readlane(vre, 0), at0 = __builtin_amdgcn_readlane(vre, 1), before1 = __builtin_amdgcn_readlane(vre, 2), at1 = __builtin_amdgcn_readlane(vre, 3);
            // (x, rs) is the point of diagonal d  <=>  rs == row_offsets[x] <= y = d - x  and  (x == rows ? d == total : y <= row_offsets[x + 1])
            const bool ok0 = (x0 > 0 ? before0 == rs0 : rs0 == 0) & (x0 < p.rows ? y0 <= at0 : d0 == total);
            const bool ok1 = (x1 > 0 ? before1 == rs1 : rs1 == 0) & (x1 < p.rows ? y1 <= at1 : d1 == total);
            verdict = single | (ok0 & ok1);
        };
        constexpr bool FL = true, BAND = false;         // (16-bit row ends and row-start bits; every column)
        stage_tile<V, BLOCK, IPT, NT, FL, BAND, decltype(check_hints)>(p, c0, c1, tile, num_tiles, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, s_x, -1, lean, check_hints);
        MSPMV_SNAP_TR(3);
        good = verdict;
    }
    if (MSPMV_UNLIKELY((layout_hints<V, IPT>()), !good)) {
        // no usable hints (the first call on this temp storage, or another matrix since): find the two boundaries, stage (again)
        // (after a failed check every wave is past the staging barrier, which touched nothing but LDS; the bits are cleared whatever
        //  was done to them, and the barrier below comes before the new staging)
        if (tid < SLOTS / 32 + 1) s_flag[tid] = 0u;
        if (late_barrier) commit_x_to_lds<V, BLOCK>(p, xr, s_dyn);      // (again, or for the first time: same values)
        __syncthreads();
        const int wave = tid / WAVE;
        if (wave < 2) {
            int rs = 0;
            const Coord c = wave_merge_path_guess(wave == 0 ? d0 : d1, p.row_end, p.rows, p.nnz, rs);
            if ((tid & (WAVE - 1)) == 0) { s_bnd[3 * wave] = c.x; s_bnd[3 * wave + 1] = rs; }
        }
        __syncthreads();
        x0 = s_bnd[0]; rs0 = s_bnd[1]; x1 = s_bnd[3]; rs1 = s_bnd[4];
        y0 = d0 - x0; y1 = d1 - x1;
        snap0 = y0 - rs0 <= HEAD_MAX; snap1 = y1 - rs1 <= HEAD_MAX;
        c0.x = x0; c0.y = snap0 ? rs0 : y0;
        c1.x = x1; c1.y = snap1 ? rs1 : y1;
        lean = snap0 && snap1 && (unsigned) (c1.y - c0.y) <= (unsigned) lean_avg * (unsigned) (c1.x - c0.x);
        TileRegs<V, BLOCK, IPT, MV> regs;
        issue_nonzero_loads<V, BLOCK, IPT, NT>(p, c0, c1, regs);
        constexpr bool FL = true;
        stage_tile<V, BLOCK, IPT, NT, FL>(p, c0, c1, tile, num_tiles, regs, s_end_raw, s_prod_raw, last_full_nz, last_full_ro, s_flag, s_x, -1, lean);
    }
    store_hints(!good);
    // the tiles that hold published pieces of this tile's first row (only when the row ends here and began > HEAD_MAX
    // nonzeros before the tile): from the tile of its first nonzero (path item x0 + rs0) -- or the one after, if that one
    // handed its short piece on by the rule above -- up to this tile
    int first_piece = tile;
    if (!snap0) {                                                   // (also for a tile without a row end: a group leader needs it)
        const unsigned item = (unsigned) x0 + (unsigned) rs0;         // (<= rows + nnz < 2^31)
        const int ft = (int) (item / (unsigned) TILE);
        const unsigned tail_ft = (unsigned) (ft + 1) * (unsigned) TILE - item;
        first_piece = ft + (tail_ft <= (unsigned) HEAD_MAX ? 1 : 0);
    }
    const int pshift = c0.y - (c0.y & ~3);
    const int eshift = (c0.x + 1) - ((c0.x + 1) & ~3);
#ifdef MSPMV_DEV
#define MSPMV_SNAP_END() do { MSPMV_SNAP_TR(4); if (snap_tr) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); MSPMV_SNAP_TR(5); } } while (0)    // (5: y stores acknowledged)
    unsigned long long *const lean_tr = snap_tr;
#else
#define MSPMV_SNAP_END() do { } while (0)
    unsigned long long *const lean_tr = nullptr;
#endif
    if (MSPMV_LIKELY((layout_hints<V, IPT>()), lean)) {
        consume_tile_rows<V, BLOCK, IPT, AXPBY>(p, c0, c1.x - c0.x, s_end_raw + eshift, s_prod_raw, pshift, carries + tile, lean_tr);
        MSPMV_SNAP_END();
        return;                                                     // (the program ends HERE, not after a jump over the general reduction)
    }
    consume_tile_flags<V, BLOCK, IPT, AXPBY, 4>(p, c0, c1.x - c0.x, c1.y - c0.y, s_end_raw + eshift, s_prod_raw, s_flag,
                                                s_wave_key, s_wave_val, carries + tile, pshift, nullptr, &lbe, tile, !snap1, first_piece, -1, rs0);
    MSPMV_SNAP_END();
#undef MSPMV_SNAP_END
#undef MSPMV_SNAP_TR
}

// mspmv_probe_read_stream: a bare 16-byte-per-lane read stream over a buffer, one 256 x 11-chunk piece per block like a tile's
// nonzero stream, ordinary or non-temporal loads -- the rate a measured kernel's algorithmic bytes are to be read against when
// its arrays live in the Infinity Cache (bench.py: records whose matrix fits 256 MB), where the HBM peak is not the bound.
__device__ int g_probe_sink;
template <bool NT>
__global__ __launch_bounds__(256) void probe_read_kernel(const int4v *__restrict__ p, unsigned long long n16)
{
    constexpr int PER = 11;
    const unsigned long long base = (unsigned long long) blockIdx.x * (256ull * PER) + threadIdx.x;
    int4v acc = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const unsigned long long i = base + 256ull * k;
        if (i < n16) { const int4v v = NT ? __builtin_nontemporal_load(p + i) : p[i]; acc ^= v; }
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x5a5a5a5a) g_probe_sink = 1;        // (keeps the loads; practically never true)
}

// ONE runtime call per launch.  `kernel<<<...>>>(...)` / hipLaunchKernelGGL is three (push the launch configuration, pop it in the stub,
// hipLaunchKernel) and leaves its status to a fourth (hipGetLastError); every entry into the HIP runtime costs the calling thread
// 50-100 ns, and the reference's timing loop is bound by the enqueueing thread below a few hundred tiles (tools/ab_driver: host
// enqueue time per call == loop time per call there).  The arguments are converted to the kernel's exact parameter types.
template <typename... P, typename... A, size_t... I>
static inline hipError_t launch_exact_impl(void (*kernel)(P...), dim3 grid, dim3 block, size_t dyn_lds, hipStream_t stream, std::index_sequence<I...>, A &&...a)
{
    std::tuple<P...> vals{static_cast<P>(a)...};
    void *ptrs[] = {static_cast<void *>(&std::get<I>(vals))...};
    return hipLaunchKernel(reinterpret_cast<const void *>(kernel), grid, block, ptrs, dyn_lds, stream);
}
template <typename... P, typename... A>
static inline hipError_t launch_exact(void (*kernel)(P...), dim3 grid, dim3 block, size_t dyn_lds, hipStream_t stream, A &&...a)
{
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    return launch_exact_impl(kernel, grid, block, dyn_lds, stream, std::index_sequence_for<P...>{}, static_cast<A &&>(a)...);
}

// host side of the compact variant (defined and instantiated in mspmv_compact.hip, the translation unit compiled for it)
template <typename V>
hipError_t launch_snap_compact(bool axpby, unsigned grid, size_t dyn_lds, hipStream_t stream, Coord *coords, int *rstart, int num_tiles,
                         const Params<V> &p, Carry<V> *carries, const LookBack &lb, int lean_avg, int tile_map);

// Single-launch alternative (MSPMV_TUNE_ATOMIC_FIX): one atomicAdd per carry,
// like the reference's fp32 path (agent_segment_fixup.cuh:226-260); order of
// the additions, hence the rounding, varies from run to run.
template <typename V, int BLOCK>
__global__ __launch_bounds__(BLOCK) void fixup_atomic_kernel(const Carry<V> *__restrict__ in, int n,
                                                             V *__restrict__ y, int rows, V alpha)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const Carry<V> c = in[i];
    if (c.key < rows && c.value != (V) 0) atomicAdd(&y[c.key], alpha * c.value);
}

// y_local[0] += sum of the carries of earlier parts that belong to it
// (multi-GPU, mspmv.h: mspmv_mg_apply_carries).  take_mask bit j set => add
// carries[j]; rank order => deterministic.
template <typename V>
__global__ void mg_apply_kernel(V *__restrict__ y_local, const V *__restrict__ carries, unsigned long long take_mask,
                                int parts)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    V acc = y_local[0];
    for (int j = 0; j < parts; ++j)
        if ((take_mask >> j) & 1ull) acc += carries[j];
    y_local[0] = acc;
}

}  // namespace mspmv
