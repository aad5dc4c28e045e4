// mspmv_csrsv_plan.hpp -- what a level-scheduling plan (mspmv_csrsv_plan_t of include/mspmv.h) holds.  mspmv_csrsv.hip makes and solves
// with it; mspmv_csrilu0.hip factorises along the same levels (the dependency graph of row-wise ILU(0) is the LOWER solve's);
// mspmv_csrsm.hip solves for several right-hand sides with it.
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
