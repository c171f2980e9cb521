// walk_rule.h -- the arguments of a random walk and of PinSAGE's neighbour sampler (legion_random_walk, legion_pinsage_neighbors,
// include/legion_hip.h): the one place that says which are legal, and the checks every walk op shares (node2vec_rule.h uses them).
// Host-only, no HIP: operators.hip asks here before it enqueues anything, tests/cpu/walk_rule_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

// the shared checks.  count, per >= 0 and count * per < 2^62: base above the last index is asked first, so the sum cannot overflow
constexpr bool walk_draw_index_past(int64_t base, int64_t count, int64_t per)
{
    return base > (int64_t)0x7FFFFFFF || base + count * per > (int64_t)0x7FFFFFFF;
}
constexpr bool walk_flag(int32_t weighted) { return weighted == 0 || weighted == 1; }
constexpr bool walk_lacks_table(int32_t weighted, bool graph_has_table) { return weighted == 1 && !graph_has_table; }
constexpr bool walk_probability(float prob) { return prob >= 0.0f && prob <= 1.0f; }      // (NaN fails both comparisons)

enum class WalkRefusal { Ok, Count, Visits, DrawIndex, Weighted, NoTable, Prob };

constexpr WalkRefusal walk_refusal(int32_t num_walks, int32_t length, int64_t base, int32_t weighted, bool graph_has_table, float restart_prob)
{
    if (num_walks < 0 || length < 1 || base < 0) return WalkRefusal::Count;
    if (walk_draw_index_past(base, num_walks, length)) return WalkRefusal::DrawIndex;
    if (!walk_flag(weighted)) return WalkRefusal::Weighted;
    if (walk_lacks_table(weighted, graph_has_table)) return WalkRefusal::NoTable;
    if (!walk_probability(restart_prob)) return WalkRefusal::Prob;
    return WalkRefusal::Ok;
}

constexpr WalkRefusal pinsage_refusal(int32_t num_seeds, int32_t walks_per_seed, int32_t walk_length, int32_t num_neighbors, int64_t base,
                                      int32_t weighted, bool graph_has_table, float termination_prob)
{
    if (num_seeds < 0 || walks_per_seed < 1 || walk_length < 1 || num_neighbors < 1 || base < 0) return WalkRefusal::Count;
    const int64_t visits = (int64_t)walks_per_seed * (int64_t)walk_length;
    if (visits > LEGION_PINSAGE_MAX_VISITS || num_neighbors > LEGION_PINSAGE_MAX_VISITS) return WalkRefusal::Visits;
    if (walk_draw_index_past(base, num_seeds, visits)) return WalkRefusal::DrawIndex;      // (num_seeds * visits < 2^41)
    if (!walk_flag(weighted)) return WalkRefusal::Weighted;
    if (walk_lacks_table(weighted, graph_has_table)) return WalkRefusal::NoTable;
    if (!walk_probability(termination_prob)) return WalkRefusal::Prob;
    return WalkRefusal::Ok;
}

static_assert(LEGION_PINSAGE_MAX_VISITS == 1024, "walk_refusal_text spells the limit out");
constexpr const char* walk_refusal_text(WalkRefusal r)
{
    switch (r) {
    case WalkRefusal::Ok: return "ok";
    case WalkRefusal::Count: return "the counts are >= 0, the lengths >= 1 and base >= 0";
    case WalkRefusal::Visits: return "walks per seed * walk length and num_neighbors are at most 1024";
    case WalkRefusal::DrawIndex: return "base + the number of steps is past the last draw index, 2^31 - 1";
    case WalkRefusal::Weighted: return "weighted is 0 or 1";
    case WalkRefusal::NoTable: return "a weighted walk needs the graph's edge weights (legion_graph_set_edge_weights)";
    case WalkRefusal::Prob: return "the restart / termination probability lies in [0, 1]";
    }
    return "";
}
