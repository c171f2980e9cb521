// induced_rule.h -- the rule of the vertex set and of induced subgraphs (legion_node_set_build, legion_node_set_lookup,
// legion_induced_count, legion_induced_edges, legion_dst_offsets, include/legion_hip.h): how large the set's table is and where a key's
// probe starts, which arguments are legal, and how large the scratch is.  No HIP, all constexpr: node_set.h and kernels_induced.hip
// evaluate this text on the device, operators.hip asks it before it enqueues anything, tests/cpu/induced_rule_test.cpp pins it over a
// literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

// an empty key of the table: all-ones, the bit pattern of a dead column entry, which is why v >= 0 is tested before any probe
constexpr int32_t NODE_SET_EMPTY_KEY = -1;
// the multiplicative hash of unique_ids' table (kernels_link.hip): odd, a bijection mod 2^32
constexpr uint32_t NODE_SET_HASH = 2654435769u;

// the slots S of the table of k nodes: the power of two that is at least 2 k, and at least 256 (k legal); unique_ids' sizing
constexpr int64_t node_set_slots(int32_t k)
{
    int64_t s = 256;
    while (s < 2 * (int64_t)k) s <<= 1;
    return s;
}

// 32 - log2 S: what the hash is shifted by (S a power of two in [2^8, 2^21]: 24 .. 11)
constexpr int32_t node_set_shift(int64_t slots)
{
    int32_t bits = 0;
    while (((int64_t)1 << bits) < slots) bits++;
    return 32 - bits;
}

// the home slot of v >= 0: where its probe starts
constexpr uint32_t node_set_home(int32_t v, int32_t shift) { return ((uint32_t)v * NODE_SET_HASH) >> shift; }

// int32 keys[S] then uint32 first[S]
constexpr int64_t node_set_bytes(int32_t k)
{
    if (k < 0 || k > LEGION_NODE_SET_MAX_IDS) return -1;
    return 8 * node_set_slots(k);
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

// the tiles of 1 024 slots whose kept counts are summed: at most 2^20
constexpr int64_t induced_tiles(int64_t m) { return (m + 1023) / 1024; }
// the sums of 256 tile counts the one-workgroup scan takes: at most 4 096
constexpr int64_t induced_groups(int64_t m) { return (induced_tiles(m) + 255) / 256; }

// one int64 per tile plus one (the total), plus one int64 per 256 tiles: LABOR's formula
constexpr int64_t induced_scratch_bytes(int64_t m)
{
    if (m < 0 || m > LEGION_INDUCED_MAX_SLOTS) return -1;
    return 8 * (induced_tiles(m) + 1 + induced_groups(m));
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
static_assert(induced_groups(LEGION_INDUCED_MAX_SLOTS) == 4096, "2^20 tile counts make 4 096 second-level sums, the one-workgroup scan's reach");
static_assert(node_set_shift(1 << 21) == 11 && node_set_shift(256) == 24, "S lies in [2^8, 2^21], so the shift in [11, 24]: the home slot lies below S");
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
