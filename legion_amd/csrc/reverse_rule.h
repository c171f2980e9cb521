// reverse_rule.h -- the reverse CSR (legion_graph_build_reverse, include/legion_hip.h): the one place that says which graphs are
// refused, which class sorts a reverse row of a given length, how many sorted runs and merge passes a long row takes, where each pass
// reads and writes, and how the scan of the counts is levelled.  Host-only, no HIP, all constexpr: kernels_reverse.hip asks here before
// it enqueues anything, tests/cpu/reverse_rule_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

#define LG_REVERSE_WAVE 64                                    // the longest row one wave sorts in registers
#define LG_REVERSE_TILE 4096                                  // the longest row, and run, one workgroup sorts in LDS (12 bytes an entry)
#define LG_REVERSE_CHUNK 2048                                 // the outputs of a merge one workgroup takes (merge path)
#define LG_REVERSE_SCAN_ONE (1 << 20)                         // the values launch_scan_int64 takes: 4 096 sums of 256

enum class ReverseRefusal { Ok, Null, TooMany };

constexpr ReverseRefusal reverse_refusal(bool have_graph, int32_t node_num)
{
    if (!have_graph) return ReverseRefusal::Null;
    if (node_num > LEGION_REVERSE_MAX_NODES) return ReverseRefusal::TooMany;
    return ReverseRefusal::Ok;
}

static_assert(LEGION_REVERSE_MAX_NODES == (1 << 28), "reverse_refusal_text spells the limit out; 2^20 sums of 256 is the two-level scan's reach");
constexpr const char* reverse_refusal_text(ReverseRefusal r)
{
    switch (r) {
    case ReverseRefusal::Ok: return "ok";
    case ReverseRefusal::Null: return "the graph is not null";
    case ReverseRefusal::TooMany: return "at most 2^28 vertices";
    }
    return "";
}

// who sorts a reverse row of len entries by edge id
enum class ReverseClass { None, Wave, Tile, Long };

constexpr ReverseClass reverse_class(int64_t len)
{
    if (len <= 1) return ReverseClass::None;
    if (len <= LG_REVERSE_WAVE) return ReverseClass::Wave;
    if (len <= LG_REVERSE_TILE) return ReverseClass::Tile;
    return ReverseClass::Long;
}

// a long row: its sorted runs of LG_REVERSE_TILE (the last one may be short) and the merge passes that make one run of them
constexpr int64_t reverse_runs(int64_t len) { return len <= 0 ? 0 : (len + LG_REVERSE_TILE - 1) / LG_REVERSE_TILE; }

constexpr int32_t reverse_passes(int64_t len)
{
    int32_t p = 0;
    for (int64_t runs = reverse_runs(len); runs > 1; runs = (runs + 1) / 2) p++;
    return p;
}

// the width of the runs that pass p (1 .. passes) merges in pairs
constexpr int64_t reverse_run_width(int32_t pass) { return (int64_t)LG_REVERSE_TILE << (pass - 1); }

// Where a long row's entries are after pass p of `passes` (p == 0: after the runs are sorted): 0 the output, 1 the scratch.  Pass p
// reads where pass p - 1 wrote; the last pass lands in the output
constexpr int32_t reverse_buffer_after(int32_t passes, int32_t pass) { return (passes - pass) & 1; }

// the workgroups of one merge of runs of la and lb entries
constexpr int64_t reverse_merge_chunks(int64_t la, int64_t lb) { return (la + lb + LG_REVERSE_CHUNK - 1) / LG_REVERSE_CHUNK; }

// the levels of the scan over node_num counts: 0 nothing to scan, 1 launch_scan_int64 alone, 2 sums per 256 scanned by it
constexpr int32_t reverse_scan_levels(int32_t node_num) { return node_num <= 0 ? 0 : node_num <= LG_REVERSE_SCAN_ONE ? 1 : 2; }

// the int64 scratch of that scan: the sums per 256 counts and, at two levels, the sums per 256 of those
constexpr int64_t reverse_scan_sums(int32_t node_num) { return node_num <= 0 ? 0 : ((int64_t)node_num + 255) / 256; }
constexpr int64_t reverse_scan_scratch(int32_t node_num)
{
    return reverse_scan_sums(node_num) + (reverse_scan_levels(node_num) == 2 ? (reverse_scan_sums(node_num) + 255) / 256 : 0);
}

// the most rows of the Tile class and of the Long class a reverse of `live` entries can hold: the lists' capacities
constexpr int64_t reverse_tile_rows_cap(int64_t live) { return live / (LG_REVERSE_WAVE + 1); }
constexpr int64_t reverse_long_rows_cap(int64_t live) { return live / (LG_REVERSE_TILE + 1); }

static_assert(reverse_scan_sums(LEGION_REVERSE_MAX_NODES) == LG_REVERSE_SCAN_ONE, "the second level is launch_scan_int64's largest call");
