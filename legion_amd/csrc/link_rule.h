// link_rule.h -- the arguments of the link-prediction seed ops (legion_find_edges, legion_negative_sample, legion_unique_ids,
// include/legion_hip.h): the one place that says which are legal, and how large the scratch of legion_unique_ids is.  Host-only, no
// HIP: operators.hip asks here before it enqueues anything, tests/cpu/link_rule_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "id_table_rule.h"

enum class LinkRefusal { Ok, Count, Fanout, DrawIndex, Exclude, Tries, Unsorted, TooMany, Scratch, Alias };

constexpr LinkRefusal find_edges_refusal(int32_t n)
{
    return n < 0 ? LinkRefusal::Count : LinkRefusal::Ok;
}

// rows_sorted: what legion_graph_check_rows_sorted has remembered for the graph (1 sorted, 0 not), or -1 before any check
constexpr LinkRefusal negative_sample_refusal(int32_t n, int32_t k, int64_t base, int32_t exclude, int32_t max_tries, int32_t rows_sorted)
{
    if (n < 0 || base < 0) return LinkRefusal::Count;
    if (k < 1) return LinkRefusal::Fanout;
    if (base > (int64_t)0x7FFFFFFF || base + (int64_t)n * (int64_t)k > (int64_t)0x7FFFFFFF) return LinkRefusal::DrawIndex;      // (n * k < 2^62)
    if (exclude < 0 || exclude > 3) return LinkRefusal::Exclude;
    if (max_tries < 1 || max_tries > LEGION_NEGATIVE_MAX_TRIES) return LinkRefusal::Tries;
    if ((exclude & 2) && rows_sorted != 1) return LinkRefusal::Unsorted;
    return LinkRefusal::Ok;
}

// the slots of the table of m ids (id_table_rule.h)
constexpr int64_t unique_ids_table_slots(int32_t m) { return id_table_slots(m); }

constexpr int64_t unique_ids_tiles(int32_t m) { return ((int64_t)m + 255) / 256; }

// int32 each: the table's keys and first indices [2 x slots] (what the call clears), every id's slot [m], the rank of every first
// touch by its index [m], the tiles' counts [tiles]
constexpr int64_t unique_ids_scratch_bytes(int32_t m)
{
    if (m < 0 || m > LEGION_UNIQUE_MAX_IDS) return -1;
    return id_table_bytes(unique_ids_table_slots(m)) + 4 * (2 * (int64_t)m + unique_ids_tiles(m));
}

constexpr bool link_ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return a < b + b_bytes && b < a + a_bytes;
}

// ids, unique, local, count: the addresses of the four buffers (non-null: the caller has checked)
constexpr LinkRefusal unique_ids_refusal(int32_t m, int64_t scratch_bytes, uint64_t ids, uint64_t unique, uint64_t local, uint64_t count)
{
    if (m < 0) return LinkRefusal::Count;
    if (m > LEGION_UNIQUE_MAX_IDS) return LinkRefusal::TooMany;
    if (scratch_bytes < unique_ids_scratch_bytes(m)) return LinkRefusal::Scratch;
    const uint64_t bytes = 4 * (uint64_t)m;
    if (link_ranges_overlap(ids, bytes, unique, bytes) || link_ranges_overlap(ids, bytes, local, bytes) || link_ranges_overlap(ids, bytes, count, 4))
        return LinkRefusal::Alias;
    return LinkRefusal::Ok;
}

static_assert(LEGION_NEGATIVE_MAX_TRIES == 256 && LEGION_UNIQUE_MAX_IDS == (1 << 20), "link_refusal_text spells both limits out");
constexpr const char* link_refusal_text(LinkRefusal r)
{
    switch (r) {
    case LinkRefusal::Ok: return "ok";
    case LinkRefusal::Count: return "the count and base are >= 0";
    case LinkRefusal::Fanout: return "k >= 1";
    case LinkRefusal::DrawIndex: return "base + n * k is past the last draw index, 2^31 - 1";
    case LinkRefusal::Exclude: return "exclude lies in [0, 3]";
    case LinkRefusal::Tries: return "max_tries lies in [1, 256]";
    case LinkRefusal::Unsorted: return "excluding edges needs rows checked sorted (legion_graph_check_rows_sorted returned 1)";
    case LinkRefusal::TooMany: return "at most 2^20 ids a call";
    case LinkRefusal::Scratch: return "scratch_bytes is at least legion_unique_ids_scratch_bytes(m)";
    case LinkRefusal::Alias: return "the outputs do not overlap ids";
    }
    return "";
}
