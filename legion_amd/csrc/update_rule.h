// update_rule.h -- the sparse row update (legion_row_update, include/legion_hip.h): the one place that says which arguments are
// refused, how many radix passes sort the ids of a table of N rows, how the ids are cut into sort tiles and how the scratch is laid
// out.  Host-only, no HIP, all constexpr: operators.hip asks here before it enqueues anything, kernels_update.hip reads the same
// constants.  The chunk rule, the lane split of a row and the slots of the partial rows are the aggregation's (aggregate_rule.h).
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "aggregate_rule.h"

#define LG_UPD_THREADS 256                                    // four waves
#define LG_UPD_ILP 4                                          // pairs a lane holds of a sort tile
#define LG_UPD_TILE (LG_UPD_THREADS * LG_UPD_ILP)             // 1 024 consecutive pairs
#define LG_UPD_RADIX_BITS 8
#define LG_UPD_RADIX (1 << LG_UPD_RADIX_BITS)                 // one digit per lane of a workgroup

enum class UpdateRefusal { Ok, Null, CachePair, Combine, Optimizer, State, Count, TooMany, Scratch };

// The keys are 0 .. N (N: a dead entry, sorted last): `bits` is the bit width of N, and a pass sorts 8 of them
constexpr int32_t update_bits(int32_t N)
{
    int32_t b = 0;
    for (uint32_t v = N > 0 ? (uint32_t)N : 0u; v != 0; v >>= 1) b++;
    return b;
}
constexpr int32_t update_passes(int32_t N) { return (update_bits(N) + LG_UPD_RADIX_BITS - 1) / LG_UPD_RADIX_BITS; }

// the sort tiles of m pairs, and the values of a pass's digit counts: int64[256][tiles], digit-major, scanned by launch_scan_int64
constexpr int64_t update_tiles(int32_t m) { return m <= 0 ? 0 : ((int64_t)m + LG_UPD_TILE - 1) / LG_UPD_TILE; }
constexpr int64_t update_count_values(int32_t m) { return LG_UPD_RADIX * update_tiles(m); }

// The scratch in 8-byte words, in this order: two pair buffers {key, position} [m] each; the digit counts [256 x tiles], their sums
// per 256 [tiles] and the scan's total [1]; the group arrays: the heads of every tile int32[tiles], U int32[1] (two words together,
// rounded up), group_id int32[m], group_off int32[m + 1]; first_chunk int64[m + 1] and its scan's sums; (16-byte aligned) the
// partial rows float[rows x D].  A partial row's count is the length group_off gives: none is stored
struct UpdateScratch {
    int64_t pairs0, pairs1, counts, count_sums, count_total, tile_heads, groups, group_id, group_off, first_chunk, chunk_sums, partial;
    int64_t words;                  // all of it but the partial rows
};

constexpr int64_t update_even(int64_t words) { return (words + 1) & ~(int64_t)1; }

constexpr UpdateScratch update_scratch(int32_t m)
{
    UpdateScratch s{};
    const int64_t tiles = update_tiles(m);
    s.pairs0 = 0;
    s.pairs1 = s.pairs0 + m;
    s.counts = s.pairs1 + m;
    s.count_sums = s.counts + update_count_values(m);
    s.count_total = s.count_sums + tiles;
    s.tile_heads = s.count_total + 1;
    s.groups = s.tile_heads + (tiles + 1) / 2;
    s.group_id = s.groups + 1;
    s.group_off = s.group_id + ((int64_t)m + 1) / 2;
    s.first_chunk = s.group_off + ((int64_t)m + 2) / 2;
    s.chunk_sums = s.first_chunk + m + 1;
    s.partial = update_even(s.chunk_sums + aggregate_scan_words(m));
    s.words = s.partial;
    return s;
}

// -1: no such call.  N does not size it: the sort's passes reuse the same buffers
constexpr int64_t update_scratch_bytes(int32_t m, int32_t N, int32_t D)
{
    if (m < 0 || m > LEGION_ROW_UPDATE_MAX_IDS || N <= 0 || D <= 0) return -1;
    return 8 * update_scratch(m).words + aggregate_partial_rows(m) * 4 * (int64_t)D;
}

struct UpdateArgs {
    int32_t m, N, D, combine, optimizer;
    int64_t scratch_bytes;
    bool full_table, cache_table, node_map, ids, grads, state1, state2, state_pow, scratch;
};

constexpr UpdateRefusal update_refusal(const UpdateArgs& a)
{
    if (a.combine != LEGION_REDUCE_SUM && a.combine != LEGION_REDUCE_MEAN) return UpdateRefusal::Combine;
    if (a.optimizer != LEGION_UPDATE_SGD && a.optimizer != LEGION_UPDATE_ADAGRAD && a.optimizer != LEGION_UPDATE_ADAM)
        return UpdateRefusal::Optimizer;
    if (a.cache_table != a.node_map) return UpdateRefusal::CachePair;
    if (a.m < 0 || a.N <= 0 || a.D <= 0) return UpdateRefusal::Count;
    if (a.m > LEGION_ROW_UPDATE_MAX_IDS) return UpdateRefusal::TooMany;
    if (!a.full_table || !a.ids || !a.grads || !a.scratch) return UpdateRefusal::Null;
    if (a.optimizer != LEGION_UPDATE_SGD && !a.state1) return UpdateRefusal::State;
    if (a.optimizer == LEGION_UPDATE_ADAM && (!a.state2 || !a.state_pow)) return UpdateRefusal::State;
    if (a.scratch_bytes < update_scratch_bytes(a.m, a.N, a.D)) return UpdateRefusal::Scratch;
    return UpdateRefusal::Ok;
}

static_assert(LEGION_ROW_UPDATE_MAX_IDS == (1 << 22), "4 096 tiles of 1 024 pairs");
static_assert(update_count_values(LEGION_ROW_UPDATE_MAX_IDS) == LG_AGG_SCAN_ONE, "a pass's counts are launch_scan_int64's largest call");
static_assert(update_tiles(LEGION_ROW_UPDATE_MAX_IDS) == 4096, "ONE workgroup scans the tiles' heads (tile_scan_in_place)");
static_assert(LG_UPD_RADIX == LG_UPD_THREADS, "a lane per digit combines the waves' counts");
static_assert(LG_UPD_TILE == LG_UPD_ILP * LG_AGG_K, "a wave ranks a chunk's worth of a tile");
static_assert(update_bits(255) == 8 && update_bits(256) == 9 && update_bits(65536) == 17 && update_bits(1 << 24) == 25, "the width of N");
static_assert(update_passes(255) == 1 && update_passes(256) == 2 && update_passes(65536) == 3 && update_passes(1 << 24) == 4 &&
              update_passes(0x7FFFFFFF) == 4, "8 bits a pass");
static_assert(update_scratch(1).partial % 2 == 0 && update_scratch(1025).partial % 2 == 0, "the partial rows are 16-byte aligned");
