// labor_rule.h -- the rule of layer-neighbour sampling (legion_labor_count, legion_labor_edges, include/legion_hip.h): the hash that
// gives a source vertex its one random number, the integer predicate that keeps an entry, which arguments are legal, and how large the
// scratch is.  No HIP and no floating point, all constexpr: kernels_labor.hip evaluates this text on the device, operators.hip asks it
// before it enqueues anything, tests/cpu/labor_rule_test.cpp pins it over a literal table with g++.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "kept_rule.h"

// the function of kernels_synth.hip and legion_amd/synth.py::splitmix64_np
constexpr uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the salt is hashed first: two salts do not merely permute the same numbers among neighbouring ids
constexpr uint64_t labor_key(int64_t salt) { return splitmix64((uint64_t)salt); }

// the random number of source vertex v under a key (v >= 0 wherever the rule asks)
constexpr uint32_t labor_hash_keyed(uint64_t key, int32_t v) { return (uint32_t)(splitmix64(key ^ (uint64_t)(uint32_t)v) >> 32); }
constexpr uint32_t labor_hash(int32_t v, int64_t salt) { return labor_hash_keyed(labor_key(salt), v); }

// h * d < fanout * 2^32, exactly: with d = dh 2^32 + dl the product is (h dh + (h dl >> 32)) 2^32 + (h dl mod 2^32), and a number
// t 2^32 + rem with rem < 2^32 lies below fanout 2^32 iff t < fanout.  d >= 0 is a degree, so dh < 2^31 and h dh < 2^63; h dl < 2^64.
// Hence d <= fanout keeps every entry and h == 0 always keeps.
constexpr bool labor_keep(uint32_t h, int64_t d, int32_t fanout)
{
    const uint64_t dh = (uint64_t)d >> 32, dl = (uint64_t)d & 0xFFFFFFFFull;
    return (uint64_t)h * dh + (((uint64_t)h * dl) >> 32) < (uint64_t)(uint32_t)fanout;
}

enum class LaborRefusal { Ok, Count, TooMany, Slots, Fanout, Capacity, Scratch };

// the compaction's scratch (kept_rule.h) for a legal m
constexpr int64_t labor_scratch_bytes(int64_t m)
{
    if (m < 0 || m > LEGION_LABOR_MAX_SLOTS) return -1;
    return kept_scratch_bytes(m);
}

// what both calls check, in this order
constexpr LaborRefusal labor_count_refusal(int32_t n, int64_t m, int32_t fanout, int64_t scratch_bytes)
{
    if (n < 0) return LaborRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return LaborRefusal::TooMany;
    if (m < 0 || m > LEGION_LABOR_MAX_SLOTS) return LaborRefusal::Slots;
    if (fanout < 1) return LaborRefusal::Fanout;
    if (scratch_bytes < labor_scratch_bytes(m)) return LaborRefusal::Scratch;
    return LaborRefusal::Ok;
}

constexpr LaborRefusal labor_edges_refusal(int32_t n, int64_t m, int32_t fanout, int64_t scratch_bytes, int64_t cap)
{
    if (n < 0) return LaborRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return LaborRefusal::TooMany;
    if (m < 0 || m > LEGION_LABOR_MAX_SLOTS) return LaborRefusal::Slots;
    if (fanout < 1) return LaborRefusal::Fanout;
    if (cap < 0 || cap > (int64_t)0x7FFFFFFF) return LaborRefusal::Capacity;
    if (scratch_bytes < labor_scratch_bytes(m)) return LaborRefusal::Scratch;
    return LaborRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20) && LEGION_LABOR_MAX_SLOTS == (1 << 30), "labor_refusal_text spells the limits out");
constexpr const char* labor_refusal_text(LaborRefusal r)
{
    switch (r) {
    case LaborRefusal::Ok: return "ok";
    case LaborRefusal::Count: return "n is >= 0";
    case LaborRefusal::TooMany: return "at most 2^20 rows a call";
    case LaborRefusal::Slots: return "m lies in [0, 2^30]";
    case LaborRefusal::Fanout: return "fanout is at least 1";
    case LaborRefusal::Capacity: return "cap lies in [0, 2^31 - 1]";
    case LaborRefusal::Scratch: return "scratch_bytes is at least legion_labor_scratch_bytes(m)";
    }
    return "";
}
