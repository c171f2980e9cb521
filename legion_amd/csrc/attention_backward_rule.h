// attention_backward_rule.h -- the backward pass of the fused attention aggregation (legion_attention_rows_backward,
// include/legion_hip.h): the one place that says which arguments are refused, how many registers a lane may spend on a row set, what
// a multi-chunk segment's partial record holds and how large the scratch is.  Host-only, no HIP, all constexpr: operators.hip asks
// here before it enqueues anything, kernels_attention_backward.hip reads the same constants.  The forward's refusals, the padded
// heads and the units a lane holds are attention_rule.h's; the chunk rule, the row formats and the partial rows' numbering
// aggregate_rule.h's.
#pragma once

#include <cstdint>

#include "attention_rule.h"

// A lane keeps three row sets for a whole chunk -- its columns of q, of dO and of the grad_queries sums, for every head -- where the
// forward keeps two, beside the block of rows in flight and the grad_rows row being formed: half the forward's floats a row set
#define LG_ATTB_MAX_LANE_FLOATS 32

enum class AttentionBackwardRefusal { Ok, Forward, Null, NoOutput, QueriesGrad, Width, Scratch };

// the widths the backward's register plan holds: the forward's, and heads' x U x W <= 32.  float32, D % 4 == 0: 8 heads up to D 256,
// heads' x D <= 2048 up to D 1024; other float32 D: D <= 256; bf16: at most 4 heads (up to D 512), heads' x round_up(D, 8) <= 2048 up to
// D 2048
constexpr bool attention_backward_width_ok(int32_t dtype, int32_t D, int32_t heads)
{
    return attention_width_ok(dtype, D, heads) && attention_lane_floats(dtype, D, heads) <= LG_ATTB_MAX_LANE_FLOATS;
}

// rows a group keeps in flight: the forward's block (there is no rescale here; the block is what is loaded before it is used)
constexpr int32_t attention_backward_unroll(int32_t units_x_width) { return attention_unroll(units_x_width); }

// a chunk's partial record in float32: heads x D unscaled grad_queries sums
constexpr int64_t attention_backward_record_floats(int32_t D, int32_t heads) { return (int64_t)heads * (int64_t)D; }

// The scratch, in this order: first_chunk int64[n + 1], the scan's sums (both as the aggregation lays them out), (16-byte aligned) the
// partial records float[rows x record].  The same with and without grad_queries: a call without it parks nothing.  -1: no such call
constexpr int64_t attention_backward_scratch_bytes(int32_t n, int64_t M, int32_t D, int32_t heads)
{
    if (n < 0 || n > LEGION_AGGREGATE_MAX_SEGMENTS || M < 0 || D <= 0 || heads < 1 || heads > LEGION_ATTENTION_MAX_HEADS) return -1;
    return 8 * aggregate_first_words(n) + aggregate_partial_rows(M) * 4 * attention_backward_record_floats(D, heads);
}

struct AttentionBackwardArgs {
    int32_t dtype, n, D, heads;
    int64_t M, scratch_bytes;
    bool full_table, cache_table, node_map, offsets, ids, queries, bias, grad_out, out, lse, grad_queries, grad_bias, grad_rows, scratch;
};

constexpr AttentionBackwardRefusal attention_backward_refusal(const AttentionBackwardArgs& a)
{
    // the forward's refusals but its scratch size: out is the forward's float32 result
    const AttentionArgs f{.dtype = a.dtype, .out_dtype = LEGION_FEATURE_F32, .n = a.n, .D = a.D, .heads = a.heads, .M = a.M,
                          .scratch_bytes = INT64_MAX, .full_table = a.full_table, .cache_table = a.cache_table, .node_map = a.node_map,
                          .offsets = a.offsets, .ids = a.ids, .queries = a.queries, .bias = a.bias, .out = a.out, .scratch = a.scratch};
    if (attention_refusal(f) != AttentionRefusal::Ok) return AttentionBackwardRefusal::Forward;
    if (!a.grad_out || !a.out || !a.lse) return AttentionBackwardRefusal::Null;
    if (!a.grad_queries && !a.grad_bias && !a.grad_rows) return AttentionBackwardRefusal::NoOutput;
    if (a.grad_queries && !a.queries) return AttentionBackwardRefusal::QueriesGrad;
    if (!attention_backward_width_ok(a.dtype, a.D, a.heads)) return AttentionBackwardRefusal::Width;
    if (a.scratch_bytes < attention_backward_scratch_bytes(a.n, a.M, a.D, a.heads)) return AttentionBackwardRefusal::Scratch;
    return AttentionBackwardRefusal::Ok;
}

static_assert(2 * LG_ATTB_MAX_LANE_FLOATS == LG_ATT_MAX_LANE_FLOATS, "three row sets of half the forward's two");
static_assert(attention_backward_width_ok(LEGION_FEATURE_F32, 128, 8) && attention_backward_width_ok(LEGION_FEATURE_F32, 256, 8) &&
              attention_backward_width_ok(LEGION_FEATURE_F32, 256, 4), "float32: 128-d and 256-d rows at 8 and 4 heads");
static_assert(!attention_backward_width_ok(LEGION_FEATURE_F32, 260, 8) && attention_backward_width_ok(LEGION_FEATURE_F32, 260, 3) &&
              attention_backward_width_ok(LEGION_FEATURE_F32, 512, 4) && !attention_backward_width_ok(LEGION_FEATURE_F32, 512, 8) &&
              attention_backward_width_ok(LEGION_FEATURE_F32, 1024, 2) && !attention_backward_width_ok(LEGION_FEATURE_F32, 1024, 3),
              "float32: heads' x D <= 2048 past 64 units");
static_assert(attention_backward_width_ok(LEGION_FEATURE_F32, 255, 8) && !attention_backward_width_ok(LEGION_FEATURE_F32, 257, 1), "a float32 a lane: D <= 256");
static_assert(attention_backward_width_ok(LEGION_FEATURE_BF16, 128, 4) && !attention_backward_width_ok(LEGION_FEATURE_BF16, 8, 8) &&
              attention_backward_width_ok(LEGION_FEATURE_BF16, 1024, 2) && !attention_backward_width_ok(LEGION_FEATURE_BF16, 1032, 2) &&
              attention_backward_width_ok(LEGION_FEATURE_BF16, 2048, 1), "bf16: eight columns a unit, so at most 4 heads; heads' x D <= 2048 past 64 units");
static_assert(attention_backward_record_floats(128, 4) == 512, "D sums per head");
static_assert(attention_backward_scratch_bytes(5, 0, 128, 1) == aggregate_scratch_bytes(5, 0, 128) && attention_backward_scratch_bytes(0, 0, 4, 9) == -1 &&
              attention_backward_scratch_bytes(0, 512, 4, 2) == 16 + 4 * 4 * 8, "the aggregation's first words, then the records");
