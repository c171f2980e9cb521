// aggregate_rule.h -- the fused neighbour aggregation (legion_aggregate_rows, include/legion_hip.h): the one place that says which
// arguments are refused, how a segment is cut into wave-chunks, how a row is spread over the lanes of a wave, where a multi-chunk
// segment's partial rows lie and how large the scratch is.  Host-only, no HIP, all constexpr: operators.hip asks here before it
// enqueues anything, kernels_aggregate.hip reads the same constants.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

#define LG_AGG_K 256                                          // the entries of a wave-chunk: four per lane
#define LG_AGG_WAVES 4                                        // waves per workgroup, each on its own chunk
#define LG_AGG_THREADS (LG_AGG_WAVES * 64)
#define LG_AGG_MAX_WG 2048                                    // the walks' cap (LG_WALK_MAX_WG): 8 192 waves stride over the chunks
#define LG_AGG_UNROLL 4                                       // rows a group keeps in flight
#define LG_AGG_SCAN_ONE (1 << 20)                             // the values launch_scan_int64 takes: 4 096 sums of 256

enum class AggregateRefusal { Ok, Null, Reduce, Dtype, Weights, CachePair, Pitch, Count, TooMany, Scratch };

// how a stored row is read: 16 bytes of float32 a lane (D % 4 == 0), one float32 a lane (any other D: the gather's tail and scalar
// cases), 16 bytes of bf16 a lane (the pitch is a multiple of 8: the pad is read and never stored)
enum class AggregateRow { F32x4, F32x1, Bf16x8 };

constexpr AggregateRow aggregate_row(int32_t dtype, int32_t D)
{
    return dtype == LEGION_FEATURE_BF16 ? AggregateRow::Bf16x8 : (D % 4 == 0 ? AggregateRow::F32x4 : AggregateRow::F32x1);
}

// the columns one lane holds, and the lane-units of a row
constexpr int32_t aggregate_unit_width(AggregateRow r) { return r == AggregateRow::F32x4 ? 4 : r == AggregateRow::F32x1 ? 1 : 8; }
constexpr int32_t aggregate_units(int32_t dtype, int32_t D)
{
    return (int32_t)(((int64_t)D + aggregate_unit_width(aggregate_row(dtype, D)) - 1) / aggregate_unit_width(aggregate_row(dtype, D)));
}

// C: the lanes that cover a row (a column block of it, past 64 units), a power of two; G = 64 / C rows are in flight in a wave
constexpr int32_t aggregate_lanes(int32_t units)
{
    int32_t c = 1;
    while (c < 64 && c < units) c <<= 1;
    return c;
}
constexpr int32_t aggregate_groups(int32_t units) { return 64 / aggregate_lanes(units); }

// the wave-chunks of a segment of len entries: an empty segment keeps one, which writes its row of zeros
constexpr int64_t aggregate_chunks(int64_t len) { return len <= LG_AGG_K ? 1 : (len + LG_AGG_K - 1) / LG_AGG_K; }

// A multi-chunk segment d with k chunks has k - 1 >= 1 chunks more than a segment needs; x = first_chunk[d] - d counts those of the
// segments before it.  Its chunk j writes the partial row 2 x + j: k <= 2 (k - 1), so the segments' ranges never meet, and the
// partial rows of a call are fewer than 2 (M / K): k - 1 < len / K
constexpr int64_t aggregate_partial_row(int64_t first_chunk, int64_t d, int64_t j) { return 2 * (first_chunk - d) + j; }
constexpr int64_t aggregate_partial_rows(int64_t M) { return M <= 0 ? 0 : 2 * (M / LG_AGG_K); }

// the scan over the n chunk counts, levelled as reverse_rule.h levels its own: 1 launch_scan_int64 alone, 2 sums per 256 scanned by it
constexpr int32_t aggregate_scan_levels(int32_t n) { return n <= 0 ? 0 : n <= LG_AGG_SCAN_ONE ? 1 : 2; }
constexpr int64_t aggregate_scan_sums(int32_t n) { return n <= 0 ? 0 : ((int64_t)n + 255) / 256; }
constexpr int64_t aggregate_scan_words(int32_t n)
{
    return aggregate_scan_sums(n) + (aggregate_scan_levels(n) == 2 ? (aggregate_scan_sums(n) + 255) / 256 : 0);
}

// The scratch, in this order: first_chunk int64[n + 1], the scan's sums, (16-byte aligned) the partial rows float[rows x D], their
// live counts int32[rows].  -1: no such call
constexpr int64_t aggregate_first_words(int32_t n) { return ((int64_t)n + 1 + aggregate_scan_words(n) + 1) & ~(int64_t)1; }
constexpr int64_t aggregate_scratch_bytes(int32_t n, int64_t M, int32_t D)
{
    if (n < 0 || n > LEGION_AGGREGATE_MAX_SEGMENTS || M < 0 || D <= 0) return -1;
    return 8 * aggregate_first_words(n) + aggregate_partial_rows(M) * (4 * (int64_t)D + 4);
}

struct AggregateArgs {
    int32_t dtype, out_dtype, reduce, n, D;
    int64_t M, scratch_bytes;
    bool full_table, cache_table, node_map, offsets, ids, weights, out, scratch;
};

constexpr AggregateRefusal aggregate_refusal(const AggregateArgs& a)
{
    if (a.reduce != LEGION_REDUCE_SUM && a.reduce != LEGION_REDUCE_MEAN && a.reduce != LEGION_REDUCE_MAX) return AggregateRefusal::Reduce;
    if (a.dtype != LEGION_FEATURE_F32 && a.dtype != LEGION_FEATURE_BF16) return AggregateRefusal::Dtype;
    if (a.out_dtype != LEGION_FEATURE_F32 && a.out_dtype != LEGION_FEATURE_BF16) return AggregateRefusal::Dtype;
    if (a.weights && a.reduce != LEGION_REDUCE_SUM) return AggregateRefusal::Weights;
    if (a.cache_table != a.node_map) return AggregateRefusal::CachePair;
    if (a.n < 0 || a.M < 0 || a.D <= 0) return AggregateRefusal::Count;
    if (a.n > LEGION_AGGREGATE_MAX_SEGMENTS) return AggregateRefusal::TooMany;
    if (a.dtype == LEGION_FEATURE_BF16 && a.D > 0x7FFFFFF8) return AggregateRefusal::Pitch;      // round_up(D, 8) is no int32
    if (!a.full_table || !a.offsets || !a.ids || !a.out || !a.scratch) return AggregateRefusal::Null;
    if (a.scratch_bytes < aggregate_scratch_bytes(a.n, a.M, a.D)) return AggregateRefusal::Scratch;
    return AggregateRefusal::Ok;
}

static_assert(LEGION_AGGREGATE_MAX_SEGMENTS == (1 << 28), "2^20 sums of 256 is the two-level scan's reach");
static_assert(aggregate_scan_sums(LEGION_AGGREGATE_MAX_SEGMENTS) == LG_AGG_SCAN_ONE, "the second level is launch_scan_int64's largest call");
static_assert(LG_AGG_K == 4 * 64, "a lane resolves four entries of its wave's chunk");
static_assert(aggregate_lanes(32) == 32 && aggregate_groups(32) == 2, "128-d float32: two rows in flight");
static_assert(aggregate_lanes(16) == 16 && aggregate_groups(16) == 4, "128-d bf16: four rows in flight");
static_assert(aggregate_lanes(65) == 64 && aggregate_lanes(1) == 1, "wider rows are walked in column blocks of 64 units");
static_assert(aggregate_chunks(0) == 1 && aggregate_chunks(LG_AGG_K) == 1 && aggregate_chunks(LG_AGG_K + 1) == 2, "the chunk rule");
static_assert(aggregate_partial_row(0, 0, 1) == 1 && aggregate_partial_row(3, 1, 0) == 4, "two slots per chunk a segment has too many");
