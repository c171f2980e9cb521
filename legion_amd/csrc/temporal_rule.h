// temporal_rule.h -- the rule of temporal neighbour sampling (legion_graph_set_edge_times, legion_temporal_sample_count,
// legion_temporal_sample_edges, include/legion_hip.h): which entries of a row are candidates under a time bound, how many slots a row
// yields, which RANK among the candidates a slot picks under either strategy, which arguments are legal and in which order they are
// refused, and how large the scratch is.  The rule speaks of ranks, never of positions: the sorted class (rank = position) and the scan
// class (rank = the n-th candidate met) of kernels_temporal.hip are one rule.  No HIP and no floating point, all constexpr: the kernels
// evaluate this text on the device, operators.hip and storage.hip ask it before they enqueue anything, tests/cpu/temporal_rule_test.cpp
// pins it over a literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "etype_rule.h"

#define LG_TEMPORAL_THREADS 256        // four waves a workgroup, a wave per row (kernels_temporal.hip)
#define LG_TEMPORAL_GRID 2048          // workgroup cap of the wave-per-row launches: 8 192 rows a trip

// an entry is a candidate of a row observed at `bound`: strictly earlier, signed 64-bit
constexpr bool temporal_candidate(int64_t time, int64_t bound) { return time < bound; }

// the slots of a row with C candidates under the fan-out f (-1: every candidate): etype_slots, one rule for both ops
constexpr int64_t temporal_slots(int64_t C, int32_t f, int32_t replace) { return etype_slots(C, f, replace); }

// a row whose slots are its candidates in CSR order, without a draw
constexpr bool temporal_takes_all(int64_t C, int32_t f, int32_t replace) { return temporal_slots(C, f, replace) == C; }

// LAST: the `slots` most recent candidates of a row sorted by time, in CSR order; a row taken whole under UNIFORM is the same with
// slots == C
constexpr int64_t temporal_last_rank(int64_t C, int64_t slots, int64_t k) { return C - slots + k; }

// UNIFORM, a row not taken whole: the draw of slot k is etype_draw with t = 0, a function of (key, row vertex, k).  With replacement
// it is the rank; without, it is Floyd's candidate c, drawn from [0, j] with j = C - f + k, and the rank is c unless an earlier slot of
// the row holds c, else j (the kernels resolve the chain, tests/temporal_ref.py loops).  A C at or above 2^32 draws below 2^32.
constexpr int64_t temporal_uniform_draw(uint64_t key, int32_t row, int64_t C, int32_t f, int32_t replace, int32_t k)
{
    return (int64_t)etype_draw(key, row, 0, k, (uint64_t)(replace != 0 ? C : etype_floyd_j(C, f, k) + 1));
}

// legion_graph_set_edge_times after its pass: adjacent entries of the whole array that decrease in time, and those of them that lie
// across a row's first entry.  Equal: no pair inside a row decreases
constexpr int32_t temporal_sorted_verdict(uint64_t descents, uint64_t row_start_descents) { return descents == row_start_descents ? 1 : 0; }

enum class TemporalRefusal { Ok, Count, TooMany, Untimed, Fanout, Strategy, Replace, LastReplace, LastUnsorted, Capacity, Pointer, Scratch };

// the scan's sums (launch_scan_int64): one int64 per tile of 256 rows, as legion_row_offsets
constexpr int64_t temporal_scratch_bytes(int32_t n) { return row_offsets_scratch_bytes(n); }

constexpr bool temporal_fanout_legal(int32_t f) { return f == -1 || (f >= 1 && f <= LEGION_TEMPORAL_MAX_FANOUT); }

// what the two calls check, in this order.  sorted: legion_graph_edge_times_sorted's answer, -1 for an untimed or a null graph;
// pointers: every required one is given.  The count pass has no cap
constexpr TemporalRefusal temporal_edges_refusal(int32_t n, int32_t sorted, int32_t fanout, int32_t strategy, int32_t replace, int64_t cap,
                                                 bool pointers)
{
    if (n < 0) return TemporalRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return TemporalRefusal::TooMany;
    if (sorted < 0) return TemporalRefusal::Untimed;
    if (!temporal_fanout_legal(fanout)) return TemporalRefusal::Fanout;
    if (strategy != LEGION_TEMPORAL_UNIFORM && strategy != LEGION_TEMPORAL_LAST) return TemporalRefusal::Strategy;
    if (replace != 0 && replace != 1) return TemporalRefusal::Replace;
    if (strategy == LEGION_TEMPORAL_LAST && replace != 0) return TemporalRefusal::LastReplace;
    if (strategy == LEGION_TEMPORAL_LAST && sorted == 0) return TemporalRefusal::LastUnsorted;
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return TemporalRefusal::Capacity;
    if (!pointers) return TemporalRefusal::Pointer;
    return TemporalRefusal::Ok;
}

constexpr TemporalRefusal temporal_count_refusal(int32_t n, int32_t sorted, int32_t fanout, int32_t strategy, int32_t replace, bool pointers,
                                                 int64_t scratch_bytes)
{
    const TemporalRefusal r = temporal_edges_refusal(n, sorted, fanout, strategy, replace, 0, pointers);
    if (r != TemporalRefusal::Ok) return r;
    if (scratch_bytes < temporal_scratch_bytes(n)) return TemporalRefusal::Scratch;
    return TemporalRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20) && LEGION_TEMPORAL_MAX_FANOUT == 64 && LEGION_TEMPORAL_UNIFORM == 0 && LEGION_TEMPORAL_LAST == 1,
              "temporal_refusal_text spells the limits out; a wave holds a row's 64 picks");
constexpr const char* temporal_refusal_text(TemporalRefusal r)
{
    switch (r) {
    case TemporalRefusal::Ok: return "ok";
    case TemporalRefusal::Count: return "n is >= 0";
    case TemporalRefusal::TooMany: return "at most 2^20 rows a call";
    case TemporalRefusal::Untimed: return "the graph has edge times (legion_graph_set_edge_times)";
    case TemporalRefusal::Fanout: return "the fan-out is -1 or lies in [1, 64]";
    case TemporalRefusal::Strategy: return "strategy is LEGION_TEMPORAL_UNIFORM or LEGION_TEMPORAL_LAST";
    case TemporalRefusal::Replace: return "replace is 0 or 1";
    case TemporalRefusal::LastReplace: return "LAST draws nothing: replace is 0";
    case TemporalRefusal::LastUnsorted: return "LAST needs rows sorted by time (legion_graph_edge_times_sorted)";
    case TemporalRefusal::Capacity: return "cap lies in [0, 2^31 - 1]";
    case TemporalRefusal::Pointer: return "a required pointer is null";
    case TemporalRefusal::Scratch: return "scratch_bytes is at least legion_temporal_sample_scratch_bytes(n)";
    }
    return "";
}
