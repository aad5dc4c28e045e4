// mspmv_csrsv_plan.hpp -- what a level-scheduling plan (mspmv_csrsv_plan_t of include/mspmv.h) holds, and the cut of its levels into
// launches.  mspmv_csrsv.hip makes and solves with it; mspmv_csrsm.hip solves for several right-hand sides with it; mspmv_csrilu0.hip
// and mspmv_csric0.hip factorise along the same levels (the dependency graph of a row-wise factorisation is the LOWER solve's).
// mspmv_levels.hpp holds the walk along the levels that the four share.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/mspmv.h"

struct mspmv_csrsv_plan {
    struct Segment { int32_t level_lo, level_hi, row_lo, row_hi; bool narrow; };
    mspmv_csrsv_info_t info{};
    int32_t *d_order = nullptr, *d_level_offsets = nullptr;
    std::vector<Segment> segments;          // the launches of one solve, in order
    std::vector<int32_t> h_level_offsets;   // the host's copy of level_offsets[]: mspmv_csrsm.hip cuts its own segments, which depend on k
};

// The launches of one pass over the levels `lo` (level l holds the rows order[lo[l] .. lo[l + 1])) with 1 << logp lanes per row: a level is
// narrow when its lanes fit the budget; a maximal run of narrow levels is one launch, every other level its own.
// launch(first level, one past the last, narrow) returns 0 or an error, which ends the walk.
template <typename F>
static int mspmv_levels_cut(const std::vector<int32_t> &lo, int logp, int budget, F launch)
{
    const int L = lo.empty() ? 0 : (int) lo.size() - 1;
    auto narrow = [&](int l) { return ((long long) (lo[l + 1] - lo[l]) << logp) <= (long long) budget; };
    for (int l = 0; l < L;) {
        int m = l + 1;
        const bool nar = narrow(l);
        if (nar)
            while (m < L && narrow(m)) ++m;
        if (int e = launch(l, m, nar)) return e;
        l = m;
    }
    return 0;
}
