// node2vec_rule.h -- the arguments of a node2vec walk (legion_node2vec_walk, include/legion_hip.h): the one place that says which are
// legal (node2vec_refusal) and what the bias (p, q) becomes for the kernel (node2vec_bias: a = 1 / p, b = 1 / q, Mx = max(a, 1, b), in
// IEEE double, once, on the host).  Host-only, no HIP: operators.hip asks here before it enqueues anything,
// tests/cpu/node2vec_rule_test.cpp pins the rules over a literal table.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
// The checks every walk op shares, beside this file.  The second path exists for one caller only: tests/test_node2vec_rule_cpu.py
// compiles a COPY of this header alone from a temporary directory with -I <repository>/include, where the first is not found.
#if __has_include("walk_rule.h")
#include "walk_rule.h"
#else
#include "../legion_amd/csrc/walk_rule.h"
#endif

struct Node2vecBias {
    double a, b, mx;                // the acceptance weights of "return" (u == t) and "other" (u no neighbour of t), and the envelope
    double lo, hi;                  // min(1, b), max(1, b): a candidate u != t is decided without the search outside [lo, hi)
};

// p, q legal (node2vec_refusal): finite and > 0, so a and b are finite and > 0
constexpr Node2vecBias node2vec_bias(float p, float q)
{
    const double a = 1.0 / (double)p, b = 1.0 / (double)q;
    const double lo = b < 1.0 ? b : 1.0, hi = b > 1.0 ? b : 1.0;
    return Node2vecBias{a, b, a > hi ? a : hi, lo, hi};
}

enum class Node2vecRefusal { Ok, Count, DrawIndex, Weighted, NoTable, Tries, Bias, BiasRatio, Unsorted };

// rows_sorted: what legion_graph_check_rows_sorted has remembered for the graph (1 sorted, 0 not), or -1 before any check
constexpr Node2vecRefusal node2vec_refusal(int32_t num_walks, int32_t length, int64_t base, int32_t weighted, bool graph_has_table,
                                           int32_t max_tries, float p, float q, int32_t rows_sorted)
{
    if (num_walks < 0 || length < 1 || base < 0) return Node2vecRefusal::Count;
    if (walk_draw_index_past(base, num_walks, length)) return Node2vecRefusal::DrawIndex;
    if (!walk_flag(weighted)) return Node2vecRefusal::Weighted;
    if (walk_lacks_table(weighted, graph_has_table)) return Node2vecRefusal::NoTable;
    if (max_tries < 1 || max_tries > LEGION_NODE2VEC_MAX_TRIES) return Node2vecRefusal::Tries;
    if (!(p > 0.0f) || !(q > 0.0f) || p > 3.402823466e+38f || q > 3.402823466e+38f) return Node2vecRefusal::Bias;      // (NaN fails p > 0)
    const Node2vecBias w = node2vec_bias(p, q);
    const double least = w.a < w.lo ? w.a : w.lo;
    if (least * (double)LEGION_NODE2VEC_MAX_BIAS < w.mx) return Node2vecRefusal::BiasRatio;
    if (rows_sorted != 1) return Node2vecRefusal::Unsorted;
    return Node2vecRefusal::Ok;
}

static_assert(LEGION_NODE2VEC_MAX_TRIES == 256 && LEGION_NODE2VEC_MAX_BIAS == 16, "node2vec_refusal_text spells both limits out");
constexpr const char* node2vec_refusal_text(Node2vecRefusal r)
{
    switch (r) {
    case Node2vecRefusal::Ok: return "ok";
    case Node2vecRefusal::Count: return "num_walks >= 0, length >= 1 and base >= 0";
    case Node2vecRefusal::DrawIndex: return "base + num_walks * length is past the last draw index, 2^31 - 1";
    case Node2vecRefusal::Weighted: return "weighted is 0 or 1";
    case Node2vecRefusal::NoTable: return "a weighted walk needs the graph's edge weights (legion_graph_set_edge_weights)";
    case Node2vecRefusal::Tries: return "max_tries lies in [1, 256]";
    case Node2vecRefusal::Bias: return "p and q are finite and > 0";
    case Node2vecRefusal::BiasRatio: return "the largest of 1/p, 1, 1/q is at most 16 times the smallest";
    case Node2vecRefusal::Unsorted: return "node2vec needs rows checked sorted (legion_graph_check_rows_sorted returned 1)";
    }
    return "";
}
