// attention_rule.h -- the fused attention aggregation (legion_attention_rows, include/legion_hip.h): the one place that says which
// arguments are refused, how a row and the heads' state are spread over the lanes and registers of a wave, what a multi-chunk
// segment's partial record holds and how large the scratch is.  Host-only, no HIP, all constexpr: operators.hip asks here before it
// enqueues anything, kernels_attention.hip reads the same constants.  The chunk rule, the row formats and the partial rows' numbering
// are aggregate_rule.h's.
#pragma once

#include <cstdint>

#include "aggregate_rule.h"

#define LG_ATT_MAX_LANE_UNITS 4                               // the units (16 bytes of a row) one lane may hold
#define LG_ATT_MAX_LANE_FLOATS 64                             // a lane's accumulators (and as many query columns): heads' x units x width

enum class AttentionRefusal { Ok, Null, Dtype, Heads, CachePair, NoLogit, Count, TooMany, Pitch, Width, Scratch };

// HP: the heads a kernel is built for, heads rounded up to a power of two (the pad heads have zero queries and are never stored)
constexpr int32_t attention_heads_padded(int32_t heads)
{
    int32_t h = 1;
    while (h < heads) h <<= 1;
    return h;
}

// U: the units a lane holds, ceil(units / 64) rounded up to a power of two: lane cl of the C covering a row holds units cl, cl + C, ...
// There is no column-block walk: the dot product needs the whole row before any exponential
constexpr int32_t attention_lane_units(int32_t units)
{
    int32_t u = 1;
    while ((int64_t)u * 64 < units) u <<= 1;
    return u;
}

// the float32 accumulators a lane keeps for a row format, D and heads: the register plan's size
constexpr int64_t attention_lane_floats(int32_t dtype, int32_t D, int32_t heads)
{
    return (int64_t)attention_heads_padded(heads) * attention_lane_units(aggregate_units(dtype, D)) * aggregate_unit_width(aggregate_row(dtype, D));
}

// the widths the register plan holds.  float32, D % 4 == 0: heads' x D <= 4096 up to D 1024 (8 heads: D <= 512); other float32 D: D <= 256;
// bf16: heads' x round_up(D, 8) <= 4096 up to D 2048 (8 heads: D <= 512)
constexpr bool attention_width_ok(int32_t dtype, int32_t D, int32_t heads)
{
    return attention_lane_units(aggregate_units(dtype, D)) <= LG_ATT_MAX_LANE_UNITS && attention_lane_floats(dtype, D, heads) <= LG_ATT_MAX_LANE_FLOATS;
}

// rows a group keeps in flight: a block of the online softmax (one new maximum and one rescale of the accumulators per block)
constexpr int32_t attention_unroll(int32_t units_x_width) { return units_x_width >= 16 ? 2 : 4; }

// a chunk's partial record in float32: (m, l) per head, then heads x D unnormalised sums
constexpr int64_t attention_record_floats(int32_t D, int32_t heads) { return (int64_t)heads * (2 + (int64_t)D); }

// The scratch, in this order: first_chunk int64[n + 1], the scan's sums (both as the aggregation lays them out), (16-byte aligned) the
// partial records float[rows x record].  -1: no such call
constexpr int64_t attention_scratch_bytes(int32_t n, int64_t M, int32_t D, int32_t heads)
{
    if (n < 0 || n > LEGION_AGGREGATE_MAX_SEGMENTS || M < 0 || D <= 0 || heads < 1 || heads > LEGION_ATTENTION_MAX_HEADS) return -1;
    return 8 * aggregate_first_words(n) + aggregate_partial_rows(M) * 4 * attention_record_floats(D, heads);
}

struct AttentionArgs {
    int32_t dtype, out_dtype, n, D, heads;
    int64_t M, scratch_bytes;
    bool full_table, cache_table, node_map, offsets, ids, queries, bias, out, scratch;
};

constexpr AttentionRefusal attention_refusal(const AttentionArgs& a)
{
    if (a.dtype != LEGION_FEATURE_F32 && a.dtype != LEGION_FEATURE_BF16) return AttentionRefusal::Dtype;
    if (a.out_dtype != LEGION_FEATURE_F32 && a.out_dtype != LEGION_FEATURE_BF16) return AttentionRefusal::Dtype;
    if (a.heads < 1 || a.heads > LEGION_ATTENTION_MAX_HEADS) return AttentionRefusal::Heads;
    if (a.cache_table != a.node_map) return AttentionRefusal::CachePair;
    if (!a.queries && !a.bias) return AttentionRefusal::NoLogit;
    if (a.n < 0 || a.M < 0 || a.D <= 0) return AttentionRefusal::Count;
    if (a.n > LEGION_AGGREGATE_MAX_SEGMENTS) return AttentionRefusal::TooMany;
    if (a.dtype == LEGION_FEATURE_BF16 && a.D > 0x7FFFFFF8) return AttentionRefusal::Pitch;      // round_up(D, 8) is no int32
    if (!attention_width_ok(a.dtype, a.D, a.heads)) return AttentionRefusal::Width;
    if (!a.full_table || !a.offsets || !a.ids || !a.out || !a.scratch) return AttentionRefusal::Null;
    if (a.scratch_bytes < attention_scratch_bytes(a.n, a.M, a.D, a.heads)) return AttentionRefusal::Scratch;
    return AttentionRefusal::Ok;
}

static_assert(LEGION_ATTENTION_MAX_HEADS == 8 && attention_heads_padded(3) == 4 && attention_heads_padded(8) == 8, "kernels for 1, 2, 4, 8 heads");
static_assert(attention_lane_units(64) == 1 && attention_lane_units(65) == 2 && attention_lane_units(130) == 4, "units a lane holds");
static_assert(attention_lane_floats(LEGION_FEATURE_F32, 128, 8) == 32 && attention_lane_floats(LEGION_FEATURE_BF16, 128, 8) == 64,
              "128-d rows, 8 heads: 32 and 64 accumulators a lane");
static_assert(attention_width_ok(LEGION_FEATURE_F32, 512, 8) && !attention_width_ok(LEGION_FEATURE_F32, 516, 8), "8 heads: D <= 512");
static_assert(attention_width_ok(LEGION_FEATURE_F32, 1024, 4) && !attention_width_ok(LEGION_FEATURE_F32, 1028, 1), "float32: D <= 1024");
static_assert(attention_width_ok(LEGION_FEATURE_F32, 255, 8) && !attention_width_ok(LEGION_FEATURE_F32, 257, 1), "a float32 a lane: D <= 256");
static_assert(attention_width_ok(LEGION_FEATURE_BF16, 2048, 2) && !attention_width_ok(LEGION_FEATURE_BF16, 2048, 3) &&
              !attention_width_ok(LEGION_FEATURE_BF16, 2049, 1) && !attention_width_ok(LEGION_FEATURE_BF16, 520, 8), "bf16 widths");
static_assert(attention_unroll(4) == 4 && attention_unroll(32) == 2, "wide lanes keep two rows in flight");
static_assert(attention_record_floats(128, 4) == 4 * 130, "(m, l) and D sums per head");
static_assert(attention_scratch_bytes(5, 0, 128, 1) == aggregate_scratch_bytes(5, 0, 128) && attention_scratch_bytes(0, 0, 4, 9) == -1 &&
              attention_scratch_bytes(0, 512, 4, 2) == 16 + 4 * 4 * 12, "the aggregation's first words, then the records");
