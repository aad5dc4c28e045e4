// mspmv_types.hpp -- what every CsrMV kernel shares (mspmv_kernels.hpp is the map): vector types, Coord, Carry, Params, the variant tags,
// the tagged records that blocks of one launch hand each other, where a coordinate pass puts a tile boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <tuple>
#include <type_traits>
#include <utility>

namespace mspmv {

constexpr int WAVE = 64;

typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef double double2v __attribute__((ext_vector_type(2)));

struct Coord {
    int x;  // row-ends consumed   (list A index)
    int y;  // nonzeros consumed   (list B index)
};

template <typename V> struct Carry;
template <> struct alignas(8) Carry<float> { int key; float value; };
template <> struct alignas(16) Carry<double> { int key; int pad; double value; };

// MV: the type the matrix values are STORED in (mixed precision: float values in a double product, bf16 values in a float one).  Every
// value is widened to V in registers right before its multiply (widen<V>); x, y, alpha, beta, the products and every sum are V.
struct bf16 { unsigned short bits; };         // the upper 16 bits of an IEEE fp32
template <typename V, typename MV = V>
struct Params {
    const MV *__restrict__ values;
    const int *__restrict__ row_end;  // d_row_offsets + 1 (device_spmv.cuh:148)
    const int *__restrict__ cols;
    const V *__restrict__ x;
    V *__restrict__ y;
    int rows;
    int nnz;
    V alpha;
    V beta;
    int x_lds;                        // > 0: x has this many entries and the tile kernels gather it from LDS
    // column-band passes (BAND kernels only): this launch multiplies the nonzeros whose column lies in
    // [band_lo, band_lo + band_len) and treats the others as zeros; band_pass > 0 adds its carries to the stored ones
    int band_lo, band_len, band_pass;
};

// Variant tags: WHICH tile kernel an instantiation is, as words in the source and in the symbol (tile_kernel, tile_kernel_vec,
// tile_kernel_snap, spmm_tile_kernel, spmm_lane_kernel).  Each carries the constants the kernel unpacks at its top.
struct Assign { static constexpr bool AXPBY = false; };        // output: y = A x
struct Axpby { static constexpr bool AXPBY = true; };          //         y = alpha A x + beta y
struct Cached { static constexpr bool NT = false; };           // streams: the CSR arrays by ordinary loads
struct Streamed { static constexpr bool NT = true; };          //          non-temporally (ld_stream*)
// body of tile_kernel_vec: one sweep over the tile; the column-band passes compiled in (run_band_passes); the clock-scheduled bands (stage_tile_tdm)
struct Production { static constexpr bool PERSIST = false, XCD_REMAP = false; static constexpr int ABLATE = 0; };
struct Sweep : Production { static constexpr bool BAND = false, TDM = false; };
struct Bands : Production { static constexpr bool BAND = true, TDM = false; };
struct Clocked : Production { static constexpr bool BAND = true, TDM = true; };
#ifdef MSPMV_DEV
// development: the persistent sweep, with one contiguous tile range per XCD (REMAP) or an ablation (ABL: 1, 6, 7; tile_kernel_vec)
template <bool REMAP, int ABL>
struct DevSweep { static constexpr bool BAND = false, TDM = false, PERSIST = true, XCD_REMAP = REMAP; static constexpr int ABLATE = ABL; };
#endif
// body of tile_kernel_snap: the general one alone, or behind the compact front end
struct General { static constexpr bool COMPACT = false; };
struct Compact { static constexpr bool COMPACT = true; };
// the tags a launch's runtime choices select (mspmv_api.hip: with_bools hands the launch lambdas the choices as constants)
template <bool AXPBY> using OutputIf = std::conditional_t<AXPBY, Axpby, Assign>;
template <bool NT> using StreamsIf = std::conditional_t<NT, Streamed, Cached>;
template <bool TDM> using BandsIf = std::conditional_t<TDM, Clocked, Bands>;

// ---------------------------------------------------------------------------
// Tagged records: how blocks of ONE launch hand each other 64 bits (tile_kernel_snap).  A record is two
// 64-bit words, each carrying half of a per-call tag beside 32 bits of payload, written and read with relaxed agent-scope
// atomics (visible across the XCDs' L2s without a cache flush).  A word is valid when its tag half matches, so no ordering
// between the two is needed, and stale or uninitialised memory is told apart by the 63 tag bits.
// EVERY RECORD SLOT IS CLEAN (0, 0) WHEN THE LAUNCH ENDS -- whoever acts on a slot LAST leaves it clean -- so no record outlives
// its call and a captured call replays with the same tags, even after the matrix changed.  A slot goes through
//     (anything) --publisher ANNOUNCES--> PENDING --publisher stores the record--> RECORD --consumer takes it--> (0, 0)
//   * a publisher ANNOUNCES itself as soon as it knows it will publish -- an atomic exchange of a marker into word 0, issued before
//     the tile's reduction, its answer looked at only when the sum is there: nothing waits for it -- and later stores the record
//     with two plain atomic stores;
//   * the one consumer every record has takes it (both tags match) and clears it;
//   * NOTHING DEPENDS ON ANOTHER WORKGROUP BEING DISPATCHED -- only on workgroups that HAVE STARTED running to their stores (a block that
//     has announced itself and is then preempted for good or faults hangs its consumer, as it would hang any kernel).  Polling for a
//     publisher that has not started is bounded; a consumer whose poll runs out -- the awaited block
//     has not been dispatched: possible only when far fewer blocks are resident than mspmv_api.hip assumed (a CU-masked stream, a
//     long kernel beside this one, several processes on the device) AND the resident ones are all waiting -- CANCELS the slot by an
//     atomic exchange.  What comes back decides: the RECORD (it arrived between the last look and now) -> taken like any other;
//     PENDING -> the publisher is RUNNING (it announced itself); a plain publisher waits for nothing, a group LEADER (below) only --
//     bounded, or for plain publishers that have started -- for its 63 predecessors: a chain of depth two, no cycle, so the record
//     comes in finite time whatever else the device does: the consumer goes on polling for it WITHOUT a bound; anything else -> the publisher has not
//     started: the cancellation stays, the block computes the missing sum itself from the matrix (recompute_row_head), and the
//     publisher, whose announcement brings the cancellation back, wipes the slot instead of publishing.
// (Until round 5 a cancelled slot's late record stayed where it was and an EPOCH word, bumped by the recomputing consumer and mixed
//  into the tags, was to keep a replayed launch from mistaking it for its own.  That left two holes: a publisher dispatched AFTER the
//  bump tagged its record with the NEW epoch -- the one the next replay reads at its start --, and blocks of one launch that read the
//  epoch before and after a bump disagreed about every tag between them, each such pair costing a full poll budget.  A publisher
//  that EXCHANGES its record in and cleans up when it finds a cancellation was measured first: correct, but the answer of the
//  exchange sits on the critical path of a tile that does nothing after publishing -- BASELINE config 4, 23 800 such tiles: +7.5 %.)
// The reference's fp64 fix-up spins without bound on the same residency assumption (single_pass_scan_operators.cuh:620-639);
// here a broken assumption costs time, never the result.  Every interleaving of these operations under relaxed ordering -- one
// publisher and one consumer, and the publisher -> leader -> consumer chain, every poll budget, clean and stale slots -- is
// enumerated by tests/test_record_protocol_model.py (payload or recompute; slot (0, 0) at the end; no wait that nothing ends;
// the unbounded wait only for a publisher that has started).  What the invariant excludes: a slot that already holds THIS call's
// marker when the launch starts (a launch killed between announce and store, then replayed with the same tags).
// ---------------------------------------------------------------------------
constexpr int REC_MAX_POLLS = 1 << 17;      // x ~1 us: ~0.1 s before a consumer gives up on a record and computes the sum itself
// (markers carry the call's tag with its low bit CLEARED: never a valid record tag, tag_a | 1)
__device__ __forceinline__ unsigned long long rec_cancel_word(unsigned tag_a) { return ((unsigned long long) (tag_a & ~1u) << 32) | 0x0CA9CE11ull; }
__device__ __forceinline__ unsigned long long rec_pending_word(unsigned tag_a) { return ((unsigned long long) (tag_a & ~1u) << 32) | 0x9E0D1D61ull; }
// the publisher's announcement; the returned word goes to rec_store when the sum is there
__device__ __forceinline__ unsigned long long rec_announce(unsigned long long *rec, unsigned tag_a)
{
    return __hip_atomic_exchange(rec, rec_pending_word(tag_a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rec_store(unsigned long long *rec, unsigned tag_a, unsigned tag_b, unsigned p0, unsigned p1, unsigned long long announced)
{
    if (announced == rec_cancel_word(tag_a)) {      // the one consumer of this slot gave up before this block started: nobody will take the record
        __hip_atomic_store(rec, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(rec + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __hip_atomic_store(rec + 1, ((unsigned long long) tag_b << 32) | p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(rec, ((unsigned long long) tag_a << 32) | p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waits (bounded) until both words carry this call's tag, clears the record; false = the slot is cancelled (payload undefined)
__device__ __forceinline__ bool rec_take(unsigned long long *rec, unsigned tag_a, unsigned tag_b, unsigned &p0, unsigned &p1, int max_polls)
{
    for (int polls = 0; polls < max_polls; ++polls) {
        const unsigned long long w0 = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long w1 = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned) (w0 >> 32) == tag_a && (unsigned) (w1 >> 32) == tag_b) {
            __hip_atomic_store(rec, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(rec + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            p0 = (unsigned) w0; p1 = (unsigned) w1;
            return true;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    // give up on this slot: cancel it -- unless its publisher has at least started
    unsigned long long w0 = __hip_atomic_exchange(rec, rec_cancel_word(tag_a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned) (w0 >> 32) != tag_a && w0 != rec_pending_word(tag_a)) return false;       // not started: the publisher will find the cancellation
    // The record's word 0 (its word 1 was stored before it by the same thread and is on its way), or the announcement of a publisher
    // that is running and waits for nothing (its record overwrites the cancellation): a wait for stores of a block that HAS started
    // (the exchange REPLACED word 0: a record's word 0 is the one it brought back; after an announcement the publisher's store will
    //  overwrite the cancellation)
    const bool have_w0 = (unsigned) (w0 >> 32) == tag_a;
    unsigned long long w1;
    for (;;) {
        if (!have_w0) w0 = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w1 = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned) (w0 >> 32) == tag_a && (unsigned) (w1 >> 32) == tag_b) break;
        __builtin_amdgcn_s_sleep(2);
    }
    __hip_atomic_store(rec, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(rec + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p0 = (unsigned) w0; p1 = (unsigned) w1;
    return max_polls > 0;                   // (max_polls == 0, the "never look" testing aid: the slot is cleaned, the record discarded -- every such tile recomputes)
}

// Where a coordinate pass puts what it finds about tile boundary t -- the merge-path point (x, y) of diagonal t * TILE:
//   coords[t] = (x, y)                       what the tile kernels read; mspmv_debug_read_tiles
//   rstart[t] = row_offsets[x]               the first nonzero of the row the boundary falls in (tile_kernel_snap; nullptr: not wanted)
struct BoundaryOut {
    Coord *coords;
    int *rstart;
};
__device__ __forceinline__ void emit_boundary(const BoundaryOut &o, int t, int x, int y, int row_start)
{
    Coord c; c.x = x; c.y = y;
    o.coords[t] = c;
    if (o.rstart) o.rstart[t] = row_start;
}

// A tiny x (the reference's --dense=<cols> inputs: 5 or 32 entries) is copied to LDS once per block and
// gathered there: the x gather then costs LDS reads instead of 12 vector-memory instructions per thread --
// as many as the whole CSR stream needs.  Bounded so that residency barely changes.
constexpr int X_LDS_MAX_BYTES = 4096;

}  // namespace mspmv
