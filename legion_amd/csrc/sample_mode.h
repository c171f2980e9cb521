// sample_mode.h -- the sampler's opt-in modes as one value, and the one place that says which of them are legal: what a pool may be
// set to (sample_mode_refusal) and what a launch needs on top (sample_launch_refusal).  Host-only, no HIP: the pool and pipeline
// setters (storage.hip, pipeline.hip) and the enqueue paths (operators.hip) ask here, launch_hop (kernels_sample.hip) picks its
// kernel instance by draw(), tests/cpu/sample_mode_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

#define LG_DISTINCT_MAX_FANOUT LEGION_DISTINCT_MAX_FANOUT   // largest fan-out of sampling without replacement (the sampler's LDS span of an entry's picks)

// how a slot picks its adjacency position: draw_from_x / floyd_draw + floyd_resolve / the search of the prefix table (draw_rule.h)
enum class SampleDraw { Uniform, Distinct, Weighted };

struct SampleMode {                 // MemoryPool's, and by value in HopParams: every lane of a launch samples with one mode
    int32_t replace = 1;            // 1: draws with replacement (the reference's); 0: distinct positions per entry (DGL's replace=False)
    int32_t edge_ids = 0;           // 1: every sampled edge also gets its position in the full CSR's column array (DGL's dgl.EID)
    int32_t weighted = 0;           // 1: picks by the graph's prefix-sum table instead of the uniform draw (DGL's prob=)
    constexpr SampleDraw draw() const { return weighted ? SampleDraw::Weighted : replace ? SampleDraw::Uniform : SampleDraw::Distinct; }
    constexpr bool operator==(const SampleMode& o) const { return replace == o.replace && edge_ids == o.edge_ids && weighted == o.weighted; }
    constexpr bool operator!=(const SampleMode& o) const { return !(*this == o); }
};

enum class SampleRefusal { Ok, BadValue, WeightedNeedsReplace, Fanout, NoTable, LanesDiffer };

// may a pool sized for fan-outs up to max_fanout take this mode?
constexpr SampleRefusal sample_mode_refusal(const SampleMode& m, int32_t max_fanout)
{
    if (((m.replace | m.edge_ids | m.weighted) & ~1) != 0) return SampleRefusal::BadValue;
    if (m.weighted && !m.replace) return SampleRefusal::WeightedNeedsReplace;
    if (!m.replace && max_fanout > LG_DISTINCT_MAX_FANOUT) return SampleRefusal::Fanout;
    return SampleRefusal::Ok;
}

// may a hop of this fan-out be launched in this mode, against a graph with / without a prefix table (legion_graph_set_edge_weights)?
constexpr SampleRefusal sample_launch_refusal(const SampleMode& m, int32_t fanout, bool graph_has_table)
{
    const SampleRefusal r = sample_mode_refusal(m, fanout);
    if (r != SampleRefusal::Ok) return r;
    return m.weighted && !graph_has_table ? SampleRefusal::NoTable : SampleRefusal::Ok;
}

static_assert(LEGION_DISTINCT_MAX_FANOUT == 256, "sample_refusal_text spells the largest fan-out out");
constexpr const char* sample_refusal_text(SampleRefusal r)
{
    switch (r) {
    case SampleRefusal::Ok: return "ok";
    case SampleRefusal::BadValue: return "a sampling mode is 0 or 1";
    case SampleRefusal::WeightedNeedsReplace: return "weighted sampling is with replacement only";
    case SampleRefusal::Fanout: return "sampling without replacement takes fan-outs up to 256";
    case SampleRefusal::NoTable: return "a weighted hop needs the graph's edge weights (legion_graph_set_edge_weights)";
    case SampleRefusal::LanesDiffer: return "lanes of one group with different sampling modes";
    }
    return "";
}
