// claim_rule.h -- the bit formats through which the kernels of a sampled hop talk (kernels_sample.hip: sample_kernel / place_kernel ->
// dedup_lists_kernel -> compact_kernel -> list_known_kernel), each once: the hash and its bucket and sub-bucket bits, the claim pair, the
// place of a claim in the lane's interleaved lists, the words of the de-duplication's LDS table and what a surviving word says, the code a
// loser leaves in slot_pos, the mark it leaves in slot_dst, and the compaction's look-back word.  No HIP, all constexpr: the kernels
// evaluate this text on the device, pool_plan.h sizes what lg_claim_at indexes, tests/cpu/claim_rule_test.cpp pins it over a literal
// table with g++.
#pragma once

#include <cstdint>

#include "sample_plan.h"      // LG_CLAIM_CHUNK_BITS

// ---- the hash: one 32-bit mix of the vertex id, its low BB bits the bucket, the bits above them a pass's sub-bucket ----
constexpr uint32_t lg_tab_hash(int32_t id)
{
    uint32_t x = (uint32_t)id;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// the bucket of a hash / of a vertex in a class of nb = 2^bb buckets
constexpr int32_t lg_hash_bucket(uint32_t h, int32_t nb) { return (int32_t)(h & (uint32_t)(nb - 1)); }
constexpr int32_t lg_bucket(int32_t v, int32_t nb) { return lg_hash_bucket(lg_tab_hash(v), nb); }
// the sub-bucket of a hash when its bucket is de-duplicated in `passes` passes (a power of two, at most 2^14: bits bb .. bb + 13, disjoint
// from the bucket's)
constexpr uint32_t lg_sub_bucket(uint32_t h, int32_t bb, uint32_t passes) { return (h >> bb) & (passes - 1u); }

// ---- the claim pair [ vertex : 32 | value : 32 ]: value is the slot that sampled the vertex (claim lists) or the vertex's position in
// sampled_ids (known lists).  Empty = all ones, which no pair of a vertex >= 0 equals ----
constexpr uint64_t LG_PAIR_EMPTY = ~0ull;
constexpr uint64_t lg_pair(int32_t v, uint32_t value) { return ((uint64_t)(uint32_t)v << 32) | value; }
constexpr int32_t lg_pair_vertex(uint64_t w) { return (int32_t)(w >> 32); }
constexpr uint32_t lg_pair_value(uint64_t w) { return (uint32_t)w; }

// ---- entry k of bucket b's claim list, of nb lists interleaved in chunks of LG_CLAIM_CHUNK entries (LanePtrs::claim_pairs; pool_plan.h
// allocates nb * chunks * LG_CLAIM_CHUNK pairs: PA_CLAIM_PAIRS) ----
constexpr int64_t lg_claim_at(int32_t b, int32_t k, int32_t nb)
{
    return ((((int64_t)(k >> LG_CLAIM_CHUNK_BITS) * nb) + b) << LG_CLAIM_CHUNK_BITS) + (k & (LG_CLAIM_CHUNK - 1));
}

// ---- the de-duplication's LDS table: word = [ vertex : 32 | pending : 1 | value : 31 ], empty = LG_PAIR_EMPTY, and per vertex the LOWEST
// word survives (atomicMin): a known position (pending clear) beats any slot, a lower slot beats a higher one ----
constexpr uint32_t LG_TAB_PENDING = 0x80000000u;
constexpr uint64_t lg_tab_known(int32_t v, uint32_t pos) { return lg_pair(v, pos); }                      // a vertex the batch already holds at pos
constexpr uint64_t lg_tab_claim(int32_t v, uint32_t slot) { return lg_pair(v, LG_TAB_PENDING | slot); }   // a claim of this hop
// where the probe of a hash starts in a table of 2^tb words
constexpr uint32_t lg_tab_home(uint32_t h, int32_t tb) { return (h * 0x9E3779B1u) >> (32 - tb); }

// ---- slot_pos[slot] of a hop: -1 no position yet (sample_kernel), >= 0 the vertex's final position, below LG_POS_NONE "lost to slot s", s a
// LOWER slot of the hop and itself a first touch; the code is its own inverse ----
constexpr int32_t LG_POS_NONE = -1;
constexpr int32_t lg_pos_lost_to(int32_t s) { return -2 - s; }
constexpr int32_t lg_pos_winner(int32_t code) { return -2 - code; }
// slot_dst[slot] of a hop: -1 no edge; v >= 0 the sampled neighbour; v < -1 the neighbour -2 - v, marked by the de-duplication as
// NOT the first touch of a new vertex (an involution: the same expression marks and unmarks).  Both codes hold for v, s <= 2^31 - 2:
// -2 - (2^31 - 1) is not an int32
#define LG_SLOT_LOSER(v) (-2 - (v))

// what the surviving word of a claim's vertex (its low half, `value`) says about the claim of `slot`: that it IS the word -- a first touch --
constexpr bool lg_tab_first_touch(uint32_t value, uint32_t slot) { return value == (LG_TAB_PENDING | slot); }
// -- or what the loser's slot_pos gets: the known position, or lost-to the slot that survived
constexpr int32_t lg_tab_loser_pos(uint32_t value)
{
    return (value & LG_TAB_PENDING) ? lg_pos_lost_to((int32_t)(value & ~LG_TAB_PENDING)) : (int32_t)value;
}

// ---- the compaction's look-back word per super tile: [ status : 2 | edges : 31 | nodes : 31 ], status 0 = not written (the words are zero
// between hops), 1 = the tile's own counts, 2 = the inclusive prefix up to and with the tile ----
#define LG_ST_AGG (1ull << 62)
#define LG_ST_PREF (2ull << 62)
constexpr uint64_t st_word(uint64_t status, int32_t e, int32_t n) { return status | ((uint64_t)(uint32_t)e << 31) | (uint64_t)(uint32_t)n; }
constexpr int32_t st_edges(uint64_t w) { return (int32_t)((w >> 31) & 0x7FFFFFFFull); }
constexpr int32_t st_nodes(uint64_t w) { return (int32_t)(w & 0x7FFFFFFFull); }
constexpr uint32_t st_status(uint64_t w) { return (uint32_t)(w >> 62); }      // 0, LG_ST_AGG >> 62 or LG_ST_PREF >> 62

static_assert(LG_LDS_BITS_LARGE + 14 <= 32, "bucket bits and the sub-bucket bits of 2^14 passes are disjoint bits of the hash");
