// in_edges_rule.h -- the arguments of the full-neighbour ops (legion_row_offsets, legion_in_edges, include/legion_hip.h): the one place
// that says which are legal, and how large the scratch of legion_row_offsets is.  Host-only, no HIP: operators.hip asks here before it
// enqueues anything, tests/cpu/in_edges_rule_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

enum class InEdgesRefusal { Ok, Count, TooMany, Slots, Scratch };

// the tiles of 256 rows whose sums the one-workgroup scan takes: at most 4 096
constexpr int64_t row_offsets_tiles(int32_t n) { return ((int64_t)n + 255) / 256; }

// one int64 per tile of 256 rows
constexpr int64_t row_offsets_scratch_bytes(int32_t n)
{
    if (n < 0 || n > LEGION_IN_EDGES_MAX_ROWS) return -1;
    return 8 * row_offsets_tiles(n);
}

constexpr InEdgesRefusal row_offsets_refusal(int32_t n, int64_t scratch_bytes)
{
    if (n < 0) return InEdgesRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return InEdgesRefusal::TooMany;
    if (scratch_bytes < row_offsets_scratch_bytes(n)) return InEdgesRefusal::Scratch;
    return InEdgesRefusal::Ok;
}

constexpr InEdgesRefusal in_edges_refusal(int32_t n, int64_t m)
{
    if (n < 0) return InEdgesRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return InEdgesRefusal::TooMany;
    if (m < 0 || m > (int64_t)0x7FFFFFFF) return InEdgesRefusal::Slots;
    return InEdgesRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20), "in_edges_refusal_text spells the limit out; 4 096 tiles is the scan's reach");
constexpr const char* in_edges_refusal_text(InEdgesRefusal r)
{
    switch (r) {
    case InEdgesRefusal::Ok: return "ok";
    case InEdgesRefusal::Count: return "n is >= 0";
    case InEdgesRefusal::TooMany: return "at most 2^20 rows a call";
    case InEdgesRefusal::Slots: return "m lies in [0, 2^31 - 1]";
    case InEdgesRefusal::Scratch: return "scratch_bytes is at least legion_row_offsets_scratch_bytes(n)";
    }
    return "";
}
