// id_table_rule.h -- the rule of the open-addressing table of ids that legion_unique_ids keeps in its scratch and legion_node_set_build
// in the caller's set (include/legion_hip.h): its empty key, its hash, how many slots it has, where a key's probe starts and how large
// it is.  No HIP, all constexpr: node_set.h evaluates this text on the device, link_rule.h and induced_rule.h size their buffers by it,
// tests/cpu/link_rule_test.cpp and tests/cpu/induced_rule_test.cpp pin it over literal tables with g++.  (A classic guard: a table that
// includes a changed copy of this file first shadows this one where the rule headers include it.)
#ifndef LEGION_ID_TABLE_RULE_H
#define LEGION_ID_TABLE_RULE_H

#include <cstdint>

// an empty key: all-ones, the bit pattern of a dead column entry, which is why id >= 0 is tested before any probe
constexpr int32_t ID_TABLE_EMPTY_KEY = -1;
// the multiplicative hash: odd, a bijection mod 2^32
constexpr uint32_t ID_TABLE_HASH = 2654435769u;

// the slots S of the table of k ids: the power of two that is at least 2 k, and at least 256 (k in [0, 2^20])
constexpr int64_t id_table_slots(int32_t k)
{
    int64_t s = 256;
    while (s < 2 * (int64_t)k) s <<= 1;
    return s;
}

// 32 - log2 S: what the hash is shifted by (S a power of two in [2^8, 2^21]: 24 .. 11)
constexpr int32_t id_table_shift(int64_t slots)
{
    int32_t bits = 0;
    while (((int64_t)1 << bits) < slots) bits++;
    return 32 - bits;
}

// the home slot of v >= 0: where its probe starts
constexpr uint32_t id_table_home(int32_t v, int32_t shift) { return ((uint32_t)v * ID_TABLE_HASH) >> shift; }

// int32 keys[S] then uint32 first[S]: what a call clears to all-ones
constexpr int64_t id_table_bytes(int64_t slots) { return 8 * slots; }

static_assert(id_table_shift(1 << 21) == 11 && id_table_shift(256) == 24, "S lies in [2^8, 2^21], so the shift in [11, 24]: the home slot lies below S");

#endif
