// exclude_rule.h -- the rule of seed-edge exclusion (legion_reverse_edge_ids, legion_edge_set_build, legion_edge_set_contains,
// legion_edge_filter_count, legion_edge_filter_edges, include/legion_hip.h): how large the set of edge ids is and where a key's probe
// starts (the pattern of id_table_rule.h, with keys and a hash of 64 bits: edge ids pass 2^32), which arguments are legal, and how large
// the filter's scratch is (kept_rule.h's formula behind this op's limit).  No HIP, all constexpr: kernels_exclude.hip evaluates this text
// on the device, operators.hip asks it before it enqueues anything, tests/cpu/exclude_rule_test.cpp pins it over a literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "kept_rule.h"

// an empty key: all-ones, the bit pattern of "no reverse edge" (-1), which is why e >= 0 is tested before any probe
constexpr int64_t EDGE_SET_EMPTY_KEY = -1;
// the multiplicative hash: odd, a bijection mod 2^64
constexpr uint64_t EDGE_SET_HASH = 0x9E3779B97F4A7C15ull;

// the slots S of the set of k ids: the power of two that is at least 2 k, and at least 256 (k in [0, 2^21])
constexpr int64_t edge_set_slots(int32_t k)
{
    int64_t s = 256;
    while (s < 2 * (int64_t)k) s <<= 1;
    return s;
}

// 64 - log2 S: what the hash is shifted by (S a power of two in [2^8, 2^22]: 56 .. 42)
constexpr int32_t edge_set_shift(int64_t slots)
{
    int32_t bits = 0;
    while (((int64_t)1 << bits) < slots) bits++;
    return 64 - bits;
}

// the home slot of e >= 0: where its probe starts.  Every bit of e counts: nothing is cut to 32 bits
constexpr uint64_t edge_set_home(int64_t e, int32_t shift) { return ((uint64_t)e * EDGE_SET_HASH) >> shift; }

// int64 keys[S]: what a build clears to all-ones; -1 for an illegal k
constexpr int64_t edge_set_bytes(int32_t k)
{
    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return -1;
    return 8 * edge_set_slots(k);
}

static_assert(edge_set_shift(1 << 22) == 42 && edge_set_shift(256) == 56, "S lies in [2^8, 2^22], so the shift in [42, 56]: the home slot lies below S");

enum class ExcludeRefusal { Ok, Count, Via, Unsorted, NoReverse, SetSize, SetBytes, Slots, Capacity, Scratch, Alias };

// rows_sorted: what legion_graph_check_rows_sorted has remembered for the graph (1 sorted, 0 not), or -1 before any check;
// have_reverse: legion_graph_build_reverse has built
constexpr ExcludeRefusal reverse_edge_ids_refusal(int64_t n, int32_t via, int32_t rows_sorted, bool have_reverse)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return ExcludeRefusal::Count;
    if (via != 0 && via != 1) return ExcludeRefusal::Via;
    if (via == 0 && rows_sorted != 1) return ExcludeRefusal::Unsorted;
    if (via == 1 && !have_reverse) return ExcludeRefusal::NoReverse;
    return ExcludeRefusal::Ok;
}

constexpr ExcludeRefusal edge_set_build_refusal(int32_t k, int64_t set_bytes)
{
    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return ExcludeRefusal::SetSize;
    if (set_bytes < edge_set_bytes(k)) return ExcludeRefusal::SetBytes;
    return ExcludeRefusal::Ok;
}

// m: the ids to look up
constexpr ExcludeRefusal edge_set_contains_refusal(int32_t k, int64_t set_bytes, int64_t m)
{
    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return ExcludeRefusal::SetSize;
    if (set_bytes < edge_set_bytes(k)) return ExcludeRefusal::SetBytes;
    if (m < 0 || m > (int64_t)0x7FFFFFFF) return ExcludeRefusal::Slots;
    return ExcludeRefusal::Ok;
}

// the compaction's scratch (kept_rule.h) for a legal m
constexpr int64_t edge_filter_scratch_bytes(int64_t m)
{
    if (m < 0 || m > LEGION_EDGE_FILTER_MAX_EDGES) return -1;
    return kept_scratch_bytes(m);
}

constexpr ExcludeRefusal edge_filter_count_refusal(int64_t m, int32_t k, int64_t set_bytes, int64_t scratch_bytes)
{
    if (m < 0 || m > LEGION_EDGE_FILTER_MAX_EDGES) return ExcludeRefusal::Slots;
    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return ExcludeRefusal::SetSize;
    if (set_bytes < edge_set_bytes(k)) return ExcludeRefusal::SetBytes;
    if (scratch_bytes < edge_filter_scratch_bytes(m)) return ExcludeRefusal::Scratch;
    return ExcludeRefusal::Ok;
}

// two byte ranges share a byte; a range without a byte (cap == 0, m == 0) overlaps nothing, wherever it starts
constexpr bool exclude_ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return a_bytes != 0 && b_bytes != 0 && a < b + b_bytes && b < a + a_bytes;
}

// in[3], out[3]: the addresses of dst, src and eid on either side (non-null but out[2], which may be 0: no eid_out)
constexpr ExcludeRefusal edge_filter_edges_refusal(int64_t m, int32_t k, int64_t set_bytes, int64_t scratch_bytes, int64_t cap,
                                                   const uint64_t (&in)[3], const uint64_t (&out)[3])
{
    if (m < 0 || m > LEGION_EDGE_FILTER_MAX_EDGES) return ExcludeRefusal::Slots;
    if (k < 0 || k > LEGION_EDGE_SET_MAX_IDS) return ExcludeRefusal::SetSize;
    if (set_bytes < edge_set_bytes(k)) return ExcludeRefusal::SetBytes;
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return ExcludeRefusal::Capacity;
    if (scratch_bytes < edge_filter_scratch_bytes(m)) return ExcludeRefusal::Scratch;
    const uint64_t width[3] = {4, 4, 8};
    for (int32_t o = 0; o < 3; o++)
        for (int32_t i = 0; i < 3; i++)
            if (out[o] != 0 && exclude_ranges_overlap(out[o], width[o] * (uint64_t)cap, in[i], width[i] * (uint64_t)m)) return ExcludeRefusal::Alias;
    return ExcludeRefusal::Ok;
}

static_assert(LEGION_EDGE_SET_MAX_IDS == (1 << 21) && LEGION_EDGE_FILTER_MAX_EDGES == (1 << 30), "exclude_refusal_text spells the limits out");
constexpr const char* exclude_refusal_text(ExcludeRefusal r)
{
    switch (r) {
    case ExcludeRefusal::Ok: return "ok";
    case ExcludeRefusal::Count: return "n lies in [0, 2^31 - 1]";
    case ExcludeRefusal::Via: return "via is 0 (the graph's sorted rows) or 1 (the reverse CSR)";
    case ExcludeRefusal::Unsorted: return "via 0 needs rows that legion_graph_check_rows_sorted has found sorted";
    case ExcludeRefusal::NoReverse: return "via 1 needs the reverse CSR that legion_graph_build_reverse builds";
    case ExcludeRefusal::SetSize: return "k lies in [0, 2^21]";
    case ExcludeRefusal::SetBytes: return "set_bytes is at least legion_edge_set_bytes(k)";
    case ExcludeRefusal::Slots: return "m lies in [0, 2^30] (a look-up: [0, 2^31 - 1])";
    case ExcludeRefusal::Capacity: return "cap lies in [0, 2^31 - 1]";
    case ExcludeRefusal::Scratch: return "scratch_bytes is at least legion_edge_filter_scratch_bytes(m)";
    case ExcludeRefusal::Alias: return "the outputs do not overlap the inputs";
    }
    return "";
}
