// etype_rule.h -- the rule of per-edge-type sampling (legion_graph_set_edge_types, legion_etype_degrees, legion_etype_sample_count,
// legion_etype_sample_edges, include/legion_hip.h): the draw of a slot, how many slots a (row, type) pair yields, how the fan-outs travel
// to the kernels, which arguments are legal and in which order they are refused, and how large the scratch is.  No HIP and no floating
// point, all constexpr: kernels_etype.hip evaluates this text on the device, operators.hip and storage.hip ask it before they enqueue
// anything, tests/cpu/etype_rule_test.cpp pins it over a literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "in_edges_rule.h"
#include "labor_rule.h"

#define LG_ETYPE_THREADS 256           // four waves a workgroup, a wave per row (kernels_etype.hip)
#define LG_ETYPE_GRID 2048             // workgroup cap of the wave-per-row launches: 8 192 rows a trip

// slot k of the pair (row, t) draws from [0, R): the upper 32 bits of a hash of (key, row, t, k), scaled.  With h uniform over 2^32
// values a result's probability differs from 1 / R by less than 2^-32, a bias below R / 2^32 relative.  R < 2^32: the product is below
// 2^64 and the result below R; a longer segment still draws below 2^32 <= R, inside it.  row >= 0, t < 64, k < 64.
constexpr uint64_t etype_draw(uint64_t key, int32_t row, int32_t t, int32_t k, uint64_t R)
{
    const uint64_t x = ((uint64_t)(uint32_t)row << 32) | ((uint64_t)(uint32_t)t << 16) | (uint64_t)(uint32_t)k;
    return ((splitmix64(key ^ x) >> 32) * R) >> 32;
}

// the slots of a pair whose segment holds D entries under the fan-out f (-1: every entry)
constexpr int64_t etype_slots(int64_t D, int32_t f, int32_t replace)
{
    if (f == 0 || D <= 0) return 0;
    if (f < 0) return D;
    if (replace == 0 && D <= (int64_t)f) return D;
    return (int64_t)f;
}

// a pair whose slots are its entries in CSR order, without a draw
constexpr bool etype_takes_all(int64_t D, int32_t f, int32_t replace) { return etype_slots(D, f, replace) == D; }

// Floyd's j of slot k without replacement: the draw of the slot is from [0, j], and j itself is the pick when the draw is taken
constexpr int64_t etype_floyd_j(int64_t D, int32_t f, int32_t k) { return D - (int64_t)f + (int64_t)k; }

// The fan-outs as kernel arguments: f + 1 lies in [0, 65], seven bits, and bit b of it for type t is bit t of plane[b].  A lane reads
// its type's fan-out with seven shifts of scalar registers: no memory, no indexed argument array.
struct EtypeFanouts {
    uint64_t plane[7];
};
constexpr EtypeFanouts etype_pack_fanouts(const int32_t* fanouts, int32_t num_types)
{
    EtypeFanouts p{};
    for (int32_t t = 0; t < num_types && t < LEGION_ETYPE_MAX_TYPES; t++)
        for (int32_t b = 0; b < 7; b++) p.plane[b] |= (uint64_t)(((uint32_t)(fanouts[t] + 1) >> b) & 1u) << t;
    return p;
}
constexpr int32_t etype_fanout(const EtypeFanouts& p, int32_t t)
{
    uint32_t v = 0;
    for (int32_t b = 0; b < 7; b++) v |= (uint32_t)((p.plane[b] >> t) & 1ull) << b;
    return (int32_t)v - 1;
}

// legion_graph_set_edge_types before its pass over the graph: 0 or the code of the first refusal
constexpr int32_t etype_set_refusal(bool graph, bool pointer, int32_t num_types)
{
    if (!graph) return LEGION_ETYPE_NO_GRAPH;
    if (!pointer) return LEGION_ETYPE_NO_POINTER;
    if (num_types < 1 || num_types > LEGION_ETYPE_MAX_TYPES) return LEGION_ETYPE_BAD_COUNT;
    return 0;
}
// ... and after it, from the pass's three counts: entries whose type is >= T, adjacent entries of col that decrease in type, and those
// of them that lie across a row's first entry
constexpr int32_t etype_set_verdict(uint64_t out_of_range, uint64_t descents, uint64_t row_start_descents)
{
    if (out_of_range != 0) return LEGION_ETYPE_TYPE_RANGE;
    if (descents != row_start_descents) return LEGION_ETYPE_UNSORTED;
    return 0;
}

enum class EtypeRefusal { Ok, Count, TooMany, Untyped, Fanout, Replace, Capacity, Pointer, Scratch };

// the scan's sums (launch_scan_int64): one int64 per tile of 256 rows, as legion_row_offsets
constexpr int64_t etype_scratch_bytes(int32_t n) { return row_offsets_scratch_bytes(n); }

constexpr bool etype_fanouts_legal(const int32_t* fanouts, int32_t num_types)
{
    if (fanouts == nullptr) return true;                             // (a null pointer is refused in its own place)
    for (int32_t t = 0; t < num_types; t++)
        if (fanouts[t] < -1 || fanouts[t] > LEGION_ETYPE_MAX_FANOUT) return false;
    return true;
}

// what the three calls check, in this order.  num_types: the graph's, 0 for an untyped or a null graph; pointers: every required one is
// given.  legion_etype_degrees stops after Untyped and Pointer; the count pass has no cap
constexpr EtypeRefusal etype_degrees_refusal(int32_t n, int32_t num_types, bool pointers)
{
    if (n < 0) return EtypeRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return EtypeRefusal::TooMany;
    if (num_types < 1) return EtypeRefusal::Untyped;
    if (!pointers) return EtypeRefusal::Pointer;
    return EtypeRefusal::Ok;
}

constexpr EtypeRefusal etype_edges_refusal(int32_t n, int32_t num_types, const int32_t* fanouts, int32_t replace, int64_t cap, bool pointers)
{
    if (n < 0) return EtypeRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return EtypeRefusal::TooMany;
    if (num_types < 1) return EtypeRefusal::Untyped;
    if (!etype_fanouts_legal(fanouts, num_types)) return EtypeRefusal::Fanout;
    if (replace != 0 && replace != 1) return EtypeRefusal::Replace;
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return EtypeRefusal::Capacity;
    if (!pointers) return EtypeRefusal::Pointer;
    return EtypeRefusal::Ok;
}

constexpr EtypeRefusal etype_count_refusal(int32_t n, int32_t num_types, const int32_t* fanouts, int32_t replace, bool pointers,
                                           int64_t scratch_bytes)
{
    const EtypeRefusal r = etype_edges_refusal(n, num_types, fanouts, replace, 0, pointers);
    if (r != EtypeRefusal::Ok) return r;
    if (scratch_bytes < etype_scratch_bytes(n)) return EtypeRefusal::Scratch;
    return EtypeRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20) && LEGION_ETYPE_MAX_TYPES == 64 && LEGION_ETYPE_MAX_FANOUT == 64,
              "etype_refusal_text spells the limits out; a lane stands for a type, and a wave holds a pair's 64 picks");
constexpr const char* etype_refusal_text(EtypeRefusal r)
{
    switch (r) {
    case EtypeRefusal::Ok: return "ok";
    case EtypeRefusal::Count: return "n is >= 0";
    case EtypeRefusal::TooMany: return "at most 2^20 rows a call";
    case EtypeRefusal::Untyped: return "the graph has edge types (legion_graph_set_edge_types)";
    case EtypeRefusal::Fanout: return "every fan-out lies in [-1, 64]";
    case EtypeRefusal::Replace: return "replace is 0 or 1";
    case EtypeRefusal::Capacity: return "cap lies in [0, 2^31 - 1]";
    case EtypeRefusal::Pointer: return "a required pointer is null";
    case EtypeRefusal::Scratch: return "scratch_bytes is at least legion_etype_sample_scratch_bytes(n)";
    }
    return "";
}
