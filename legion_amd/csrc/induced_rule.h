// induced_rule.h -- the rule of the vertex set and of induced subgraphs (legion_node_set_build, legion_node_set_lookup,
// legion_induced_count, legion_induced_edges, legion_dst_offsets, include/legion_hip.h): how large the set's table is and where a key's
// probe starts (id_table_rule.h's, under the set's names), which arguments are legal, and how large the scratch is (kept_rule.h's
// formula behind this op's limit).  No HIP, all constexpr: kernels_induced.hip evaluates this text on the device, operators.hip asks it
// before it enqueues anything, tests/cpu/induced_rule_test.cpp pins it over a literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "id_table_rule.h"
#include "kept_rule.h"

// the set's table is the id table (id_table_rule.h) of its k nodes
constexpr int32_t NODE_SET_EMPTY_KEY = ID_TABLE_EMPTY_KEY;
constexpr int64_t node_set_slots(int32_t k) { return id_table_slots(k); }
constexpr int32_t node_set_shift(int64_t slots) { return id_table_shift(slots); }
constexpr uint32_t node_set_home(int32_t v, int32_t shift) { return id_table_home(v, shift); }

// int32 keys[S] then uint32 first[S]
constexpr int64_t node_set_bytes(int32_t k)
{
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return -1;
    return id_table_bytes(id_table_slots(k));
}

enum class InducedRefusal { Ok, Count, Slots, SetSize, SetBytes, Capacity, Scratch };

constexpr InducedRefusal node_set_build_refusal(int32_t k, int64_t set_bytes)
{
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return InducedRefusal::SetSize;
    if (set_bytes < node_set_bytes(k)) return InducedRefusal::SetBytes;
    return InducedRefusal::Ok;
}

// m: the ids to look up
constexpr InducedRefusal node_set_lookup_refusal(int32_t k, int64_t set_bytes, int64_t m)
{
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return InducedRefusal::SetSize;
    if (set_bytes < node_set_bytes(k)) return InducedRefusal::SetBytes;
    if (m < 0 || m > (int64_t)0x7FFFFFFF) return InducedRefusal::Slots;
    return InducedRefusal::Ok;
}

// the compaction's scratch (kept_rule.h) for a legal m
constexpr int64_t induced_scratch_bytes(int64_t m)
{
    if (m < 0 || m > LEGION_INDUCED_MAX_SLOTS) return -1;
    return kept_scratch_bytes(m);
}

// what both calls check, in this order
constexpr InducedRefusal induced_count_refusal(int32_t n, int64_t m, int32_t k, int64_t set_bytes, int64_t scratch_bytes)
{
    if (n < 0 || n > LEGION_IN_EDGES_MAX_ROWS) return InducedRefusal::Count;
    if (m < 0 || m > LEGION_INDUCED_MAX_SLOTS) return InducedRefusal::Slots;
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return InducedRefusal::SetSize;
    if (set_bytes < node_set_bytes(k)) return InducedRefusal::SetBytes;
    if (scratch_bytes < induced_scratch_bytes(m)) return InducedRefusal::Scratch;
    return InducedRefusal::Ok;
}

constexpr InducedRefusal induced_edges_refusal(int32_t n, int64_t m, int32_t k, int64_t set_bytes, int64_t scratch_bytes, int64_t cap)
{
    if (n < 0 || n > LEGION_IN_EDGES_MAX_ROWS) return InducedRefusal::Count;
    if (m < 0 || m > LEGION_INDUCED_MAX_SLOTS) return InducedRefusal::Slots;
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return InducedRefusal::SetSize;
    if (set_bytes < node_set_bytes(k)) return InducedRefusal::SetBytes;
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return InducedRefusal::Capacity;
    if (scratch_bytes < induced_scratch_bytes(m)) return InducedRefusal::Scratch;
    return InducedRefusal::Ok;
}

constexpr InducedRefusal dst_offsets_refusal(int64_t cap, int32_t n)
{
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return InducedRefusal::Capacity;
    if (n < 0 || n > LEGION_IN_EDGES_MAX_ROWS) return InducedRefusal::Count;
    return InducedRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20) && LEGION_INDUCED_MAX_SLOTS == (1 << 30) && LEGION_NODE_SET_MAX_IDS == (1 << 20),
              "induced_refusal_text spells the limits out");
constexpr const char* induced_refusal_text(InducedRefusal r)
{
    switch (r) {
    case InducedRefusal::Ok: return "ok";
    case InducedRefusal::Count: return "n lies in [0, 2^20]";
    case InducedRefusal::Slots: return "m lies in [0, 2^30] (a lookup: [0, 2^31 - 1])";
    case InducedRefusal::SetSize: return "k lies in [0, 2^20]";
    case InducedRefusal::SetBytes: return "set_bytes is at least legion_node_set_bytes(k)";
    case InducedRefusal::Capacity: return "cap lies in [0, 2^31 - 1]";
    case InducedRefusal::Scratch: return "scratch_bytes is at least legion_induced_scratch_bytes(m)";
    }
    return "";
}
