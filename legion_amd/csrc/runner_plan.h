// runner_plan.h -- how GPURunner (server.hip) sizes what it serves from: the rows of a lane's and a pipe slot's feature buffer
// (runner_rows), and the lanes, the groups in flight, their arena and the overflow buffers behind it (runner_group_plan).  Host-only, no
// HIP: the runner measures the free HBM and allocates what the plan says, tests/cpu/runner_plan_test.cpp pins every condition.
#pragma once

#include <algorithm>
#include <cstdint>

#include "pool_plan.h"

struct RunnerRows {
    int32_t lane_rule_rows;      // the lanes: 1.2 x the PreSC maximum, scaled and clamped
    int64_t slot_rows;           // the pipe slots: the worst case of a batch where that is cheap, else the rule
};
// presc_max_ids: the largest TRAINING batch PreSC saw (server.cu:277 sizes by 1.2 x that).  Validation / test batches can be larger than
// the raw batch: the rule is scaled by that ratio, never beyond num_ids, never below one row.  The pipe_slots pipe-slot buffers -- what
// a trainer end that does not take views reads its rows from, and what the operator-by-operator Runner gathers into -- take the worst
// case of a batch, num_ids rows, whenever together they cost at most a tenth of the free HBM: no batch is ever truncated there (the
// reference sizes them by the rule and overruns).  runner_overflow = 0 keeps the rule for them too.
static inline RunnerRows runner_rows(int32_t presc_max_ids, int32_t batch_size, int32_t raw_batch_size, int64_t num_ids, int64_t float_feature_len,
                                     int32_t feature_out_dtype, int64_t free_bytes, int32_t pipe_slots, int32_t runner_overflow)
{
    RunnerRows r;
    int64_t rows = (int64_t)int32_t(presc_max_ids * 1.2) * ((batch_size + raw_batch_size - 1) / raw_batch_size);
    if (rows > num_ids) rows = num_ids;
    if (rows < 1) rows = 1;
    r.lane_rule_rows = (int32_t)rows;
    const int64_t worst_bytes = num_ids * float_feature_len * lg_feature_out_bytes(feature_out_dtype);
    r.slot_rows = runner_overflow != 0 && pipe_slots * worst_bytes <= free_bytes / 10 ? num_ids : rows;
    return r;
}

// What a lane was reckoned to cost beyond its trainer-visible arrays when the lanes are halved against the free HBM.  It predates the
// exact plan (pool_private_plan's sum) and differs from it; it stays because the exact sum would change how many lanes a tight GPU gets.
static inline int64_t runner_lane_private_estimate(int64_t num_ids, int64_t max_slots) { return num_ids * 40 + max_slots * 28; }

struct RunnerGroupPlan {
    int32_t slots, lanes;            // groups in flight, lanes per group
    bool lane_features;              // rows land in the lanes (false: forced `gather` hand-over, or no features at all)
    int32_t lane_feature_rows;
    int64_t arena_lane;              // a lane's trainer-visible bytes
    int64_t overflow_bytes;          // of ONE overflow buffer (there is one per pipe slot), 0: none
    int64_t arena_bytes;             // the lanes and the overflow buffers behind them
};
// Groups as large as bench.py's (524288 / B rounded down to a power of two, at most 512: the launch tails and the per-kernel floors are
// paid once per group), never larger than the schedule can fill (largest_group(cap)), halved while the lanes of the groups in flight
// would take more than 0.6 of the HBM that is free now (tables and caches are in place).  Three groups in flight: one being handed over,
// one running, one queued behind it -- with two, the GPU could only start group g+2 after the trainer had taken the first batch of g+1,
// and the next group's head never ran under the current group's heavy kernels (measured at RMAT-26, views: 132 k batches/s with two,
// see DESIGN.md).  One overflow buffer per pipe slot behind the lanes, inside the arena (a trainer end that takes views maps the whole
// arena): the worst case of a batch, num_ids rows -- unless they cost more than a tenth of the free HBM or would not leave the lanes
// their memory (then an oversized batch stops the server as before).  handover: LegionTuning.runner_handover (1: forced `gather`).
template <class LargestGroup>
static inline RunnerGroupPlan runner_group_plan(int64_t batch_size, int64_t num_ids, int64_t max_slots, int64_t float_feature_len, int32_t feature_out_dtype,
                                                int32_t lane_rule_rows, int64_t free_bytes, int32_t handover, int32_t runner_slots, int32_t runner_lanes,
                                                int32_t runner_overflow, LargestGroup largest_group, int32_t pipe_slots)
{
    RunnerGroupPlan p{};
    const int64_t feature_rows = std::max<int64_t>(1, std::min<int64_t>(lane_rule_rows, num_ids));
    p.slots = runner_slots >= 2 ? std::min(runner_slots, 4) : 3;
    p.lanes = 1;
    while (p.lanes * 2 <= 512 && (int64_t)p.lanes * 2 * batch_size <= 524288) p.lanes *= 2;
    if (runner_lanes > 0) p.lanes = runner_lanes;
    p.lanes = std::min(p.lanes, (int32_t)largest_group(p.lanes));
    p.lane_features = handover != 1 && float_feature_len > 0;        // forced `gather`: rows never land in a lane
    p.arena_lane = pool_visible_bytes(batch_size, num_ids, p.lane_features ? feature_rows : 0, float_feature_len, feature_out_dtype);
    const int64_t lane_bytes = p.arena_lane + runner_lane_private_estimate(num_ids, max_slots);
    while (p.lanes > 1 && (int64_t)p.lanes * p.slots * lane_bytes > free_bytes / 10 * 6) p.lanes /= 2;
    p.arena_bytes = p.arena_lane * p.lanes * p.slots;
    p.lane_feature_rows = p.lane_features ? (int32_t)feature_rows : 0;
    if (p.lane_features && handover == 0 && feature_rows < num_ids && runner_overflow != 0) {
        p.overflow_bytes = ((num_ids * float_feature_len * lg_feature_out_bytes(feature_out_dtype)) + 4095) & ~(int64_t)4095;
        if (pipe_slots * p.overflow_bytes > free_bytes / 10 || (int64_t)p.lanes * p.slots * lane_bytes + pipe_slots * p.overflow_bytes > free_bytes / 10 * 7)
            p.overflow_bytes = 0;
    }
    p.arena_bytes += pipe_slots * p.overflow_bytes;
    return p;
}
