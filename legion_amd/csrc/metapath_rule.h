// metapath_rule.h -- the rule of metapath walks and of PinSAGE over a metapath (legion_metapath_walk, legion_pinsage_metapath_neighbors,
// include/legion_hip.h): which type a step uses, how the metapath travels to the kernels, where PinSAGE's termination draw and its
// visit fall, which arguments are legal and in which order they are refused.  Host-only constexpr text, no HIP, and no floating point
// beyond the walk's own unit draw: kernels_metapath.hip evaluates it on the device, operators.hip asks it before it enqueues anything,
// tests/cpu/metapath_rule_test.cpp pins it over a literal table with g++.  The shared checks are walk_rule.h's.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "walk_rule.h"

// step j = 1 .. length uses metapath[(j - 1) mod L]; the kernels keep a running index instead: metapath_next from 0
constexpr int32_t metapath_index(int64_t j, int32_t L) { return (int32_t)((j - 1) % (int64_t)L); }
constexpr int32_t metapath_next(int32_t i, int32_t L) { return i + 1 == L ? 0 : i + 1; }

// The metapath as kernel arguments: entry i is byte i & 7 of word i >> 3, 64 bytes in eight 64-bit words.  A kernel copies the words
// once into LDS with constant indices: no argument array is indexed dynamically.
struct MetapathWords {
    uint64_t w[LEGION_METAPATH_MAX_PERIOD / 8];
};
constexpr MetapathWords metapath_pack(const uint8_t* metapath, int32_t period)
{
    MetapathWords p{};
    for (int32_t i = 0; i < period && i < LEGION_METAPATH_MAX_PERIOD; i++) p.w[i >> 3] |= (uint64_t)metapath[i] << (8 * (i & 7));
    return p;
}
constexpr int32_t metapath_type(const MetapathWords& p, int32_t i) { return (int32_t)((p.w[i >> 3] >> (8 * (i & 7))) & 0xFFu); }

// the entry of the segment [lo, hi) of a row that the unit draw r in [0, 1) picks (rule step 4): in [lo, hi) for hi > lo
constexpr int32_t metapath_pick(int32_t lo, int32_t hi, double r) { return lo + (int32_t)(r * (double)(hi - lo)); }

// PinSAGE over a metapath, step j = 1 .. Q * L of a walk: the termination draw is taken before the first step of traversals 2 .. Q,
// and a visit is recorded at the end of a traversal
constexpr bool metapath_terminates_before(int32_t j, int32_t L) { return j > 1 && (j - 1) % L == 0; }
constexpr bool metapath_visit_at(int32_t j, int32_t L) { return j % L == 0; }

enum class MetapathRefusal { Ok, Count, Period, Visits, DrawIndex, Untyped, Type, Prob, Pointer };

constexpr bool metapath_types_legal(const uint8_t* metapath, int32_t period, int32_t num_types)
{
    if (metapath == nullptr) return true;                            // (a null pointer is refused in its own place)
    for (int32_t i = 0; i < period; i++)
        if ((int32_t)metapath[i] >= num_types) return false;
    return true;
}

// what the two calls check, in this order.  num_types: the graph's, 0 for an untyped or a null graph; pointers: every required one,
// the metapath among them, is given
constexpr MetapathRefusal metapath_tail_refusal(const uint8_t* metapath, int32_t period, int32_t num_types, float prob, bool pointers)
{
    if (num_types < 1) return MetapathRefusal::Untyped;
    if (!metapath_types_legal(metapath, period, num_types)) return MetapathRefusal::Type;
    if (!walk_probability(prob)) return MetapathRefusal::Prob;
    if (!pointers || metapath == nullptr) return MetapathRefusal::Pointer;
    return MetapathRefusal::Ok;
}

constexpr MetapathRefusal metapath_walk_refusal(int32_t num_walks, const uint8_t* metapath, int32_t period, int32_t length, int64_t base,
                                                int32_t num_types, float restart_prob, bool pointers)
{
    if (num_walks < 0 || length < 1 || base < 0) return MetapathRefusal::Count;
    if (period < 1 || period > LEGION_METAPATH_MAX_PERIOD) return MetapathRefusal::Period;
    if (walk_draw_index_past(base, num_walks, length)) return MetapathRefusal::DrawIndex;
    return metapath_tail_refusal(metapath, period, num_types, restart_prob, pointers);
}

constexpr MetapathRefusal pinsage_metapath_refusal(int32_t num_seeds, const uint8_t* metapath, int32_t period, int32_t walks_per_seed,
                                                   int32_t num_traversals, int32_t num_neighbors, int64_t base, int32_t num_types,
                                                   float termination_prob, bool pointers)
{
    if (num_seeds < 0 || walks_per_seed < 1 || num_traversals < 1 || num_neighbors < 1 || base < 0) return MetapathRefusal::Count;
    if (period < 1 || period > LEGION_METAPATH_MAX_PERIOD) return MetapathRefusal::Period;
    const int64_t visits = (int64_t)walks_per_seed * (int64_t)num_traversals;
    if (visits > LEGION_PINSAGE_MAX_VISITS || num_neighbors > LEGION_PINSAGE_MAX_VISITS) return MetapathRefusal::Visits;
    if (walk_draw_index_past(base, num_seeds, visits * period)) return MetapathRefusal::DrawIndex;      // (num_seeds * steps < 2^47)
    return metapath_tail_refusal(metapath, period, num_types, termination_prob, pointers);
}

static_assert(LEGION_METAPATH_MAX_PERIOD == 64 && LEGION_PINSAGE_MAX_VISITS == 1024, "metapath_refusal_text spells the limits out");
constexpr const char* metapath_refusal_text(MetapathRefusal r)
{
    switch (r) {
    case MetapathRefusal::Ok: return "ok";
    case MetapathRefusal::Count: return "the counts are >= 0, the lengths >= 1 and base >= 0";
    case MetapathRefusal::Period: return "the metapath has 1 to 64 entries";
    case MetapathRefusal::Visits: return "walks per seed * traversals and num_neighbors are at most 1024";
    case MetapathRefusal::DrawIndex: return "base + the number of steps is past the last draw index, 2^31 - 1";
    case MetapathRefusal::Untyped: return "the graph has edge types (legion_graph_set_edge_types)";
    case MetapathRefusal::Type: return "every metapath entry is below the graph's number of edge types";
    case MetapathRefusal::Prob: return "the restart / termination probability lies in [0, 1]";
    case MetapathRefusal::Pointer: return "a required pointer is null";
    }
    return "";
}
