// operators.hip -- the five extern "C" operator entry points and the Operator plug-in classes.
//
// Reference: SS/engine/operator_impl.cuh:11-63 (declarations), SS/engine/operator_impl.cu:92-172
// (BatchGenerate), :401-499 (RandomSample), :502-519 (FeatureCacheLookup), :522-539 (IOSubmit),
// :551-580 (IOComplete); SS/engine/operator.cu:15-122 (the five Operator::run bodies).
//
// Same names, argument order, null-pointer behaviour (message + return) and error convention.
// Differences a maintainer should know about:
//   * nothing here blocks on the device: the reference's 64-byte counter read-backs
//     (operator_impl.cu:439-445, cache.cu:187-188) are gone because every kernel reads the
//     frontier / node range from the counters in device memory;
//   * FindTopo runs inside the sampling kernel and FindFeat inside the gather kernel; their
//     outputs (tmp_part_ind/tmp_part_off, cache_search_buffer) are still written;
//   * counter_update is folded into the kernels that produce the counts;
//   * there is no accessed bitmap and no position map: first touches keep no per-vertex state (see
//     legion_core.h), so BatchGenerate has nothing to memset and IOComplete nothing to restore.
#include "legion_core.h"
#include "walk_rule.h"
#include "node2vec_rule.h"
#include "link_rule.h"
#include "in_edges_rule.h"
#include "labor_rule.h"
#include "topk_rule.h"
#include "induced_rule.h"
#include "exclude_rule.h"
#include "node_set.h"

#include <iostream>


// The C handles are the C++ objects themselves, except the cache, whose handle boxes the
// UnifiedCache as its first member (cache.hip: LegionCacheBox).
static inline UnifiedCache* cache_of(LegionUnifiedCache* c) { return reinterpret_cast<UnifiedCache*>(c); }

// ---- lane-group bodies: every operator works on n lanes (n = 1 for the reference-shaped calls) ----
struct LegionLaneGroup {
    std::vector<MemoryPool*> pools;
    std::vector<int32_t> epochs;      // each pool's lanes_epoch when d_lanes was written
    LanePtrs* d_lanes = nullptr;      // contiguous device copy of every pool's current lane
    bool lanes_carved = false;        // ... taken from a pipeline's private block: goes with the block
    int32_t* iter_state = nullptr;    // device {next iteration of lane 0, stride} for graph replay, or null
};

static bool seed_set(FeatureStorage* feature, int32_t dev_id, int32_t mode, int32_t*& all_ids, int32_t*& all_labels,
                     int32_t& total_cap)
{
    all_ids = nullptr;
    all_labels = nullptr;
    total_cap = 0;
    if (mode == TRAINMODE) {
        all_ids = feature->GetTrainingSetIds(dev_id);
        all_labels = feature->GetTrainingLabels(dev_id);
        total_cap = feature->TrainingSetSize(dev_id);
    } else if (mode == VALIDMODE) {
        all_ids = feature->GetValidationSetIds(dev_id);
        all_labels = feature->GetValidationLabels(dev_id);
        total_cap = feature->ValidationSetSize(dev_id);
    } else if (mode == TESTMODE) {
        all_ids = feature->GetTestingSetIds(dev_id);
        all_labels = feature->GetTestingLabels(dev_id);
        total_cap = feature->TestingSetSize(dev_id);
    } else {
        std::cout << "invalid mode: " << mode << "\n";
    }
    if (all_ids == nullptr) {
        std::cout << "invalid src id ptr\n";
        return false;
    }
    if (all_labels == nullptr) {
        std::cout << "invalid label ptr\n";
        return false;
    }
    return true;
}

static void do_batch_generate(hipStream_t s, FeatureStorage* feature, const LanePtrs* d_lanes, int32_t n_lanes,
                              MemoryPool* pool0, int32_t batch_size, int32_t counter, int32_t dev_id, int32_t mode,
                              int32_t hop_num, const int32_t* iter_state)
{
    lg::Range mark("op0 batch_generate lanes=%d B=%d", n_lanes, batch_size);
    lg::SeedParams p;
    int32_t* all_ids = nullptr;
    int32_t* all_labels = nullptr;
    if (!seed_set(feature, dev_id, mode, all_ids, all_labels, p.total_cap)) return;
    p.all_ids = all_ids;
    p.all_labels = all_labels;
    if (batch_size > pool0->batch_size) {
        std::cout << "batch size " << batch_size << " exceeds the pool's " << pool0->batch_size << "\n";
        return;
    }
    p.batch_size = batch_size;
    p.counter0 = counter;
    p.hop_num = hop_num;
    p.iter_state = iter_state;
    lg::launch_batch_generate(s, p, d_lanes, n_lanes);
    // cache->FindFeat(op 0) (operator_impl.cu:167-170) happens inside FeatureCacheLookup(op 1)
}

// May these lanes sample against this graph -- fanout > 0: a hop of that fan-out; 0: a batch as a whole, before its first hop (every
// hop asks again with its own fan-out)?  The lanes of a launch share one HopParams, so they must agree; the rest is sample_mode.h's.
// If not: says why, raises LG_ERR_SAMPLE_MODE on every one of the lanes and returns false -- the caller enqueues nothing
static bool sample_allowed(const char* who, const char* outcome, MemoryPool* const* pools, int32_t n, GraphStorage* graph, int32_t fanout)
{
    SampleRefusal r = sample_launch_refusal(pools[0]->mode, fanout, graph->EdgeCdf() != nullptr);
    for (int32_t i = 1; i < n; i++)
        if (pools[i]->mode != pools[0]->mode) r = SampleRefusal::LanesDiffer;
    if (r == SampleRefusal::Ok) return true;
    if (r == SampleRefusal::Fanout) printf("%s: fan-out %d without replacement (at most %d)%s\n", who, fanout, LG_DISTINCT_MAX_FANOUT, outcome);   // (names the hop's fan-out)
    else printf("%s: %s%s\n", who, sample_refusal_text(r), outcome);
    for (int32_t i = 0; i < n; i++) pools[i]->RaiseError(LG_ERR_SAMPLE_MODE);
    return false;
}

static void do_random_sample(hipStream_t s, GraphStorage* graph, UnifiedCache* cache, const LanePtrs* d_lanes,
                             int32_t n_lanes, MemoryPool* pool0, int32_t count, int32_t dev_id, int32_t op_id,
                             bool is_presc)
{
    if (op_id < INTRABATCH_CON || op_id % INTRABATCH_CON != 0 || count < 1) {
        printf("Sampling Parameters Error\n");   // counter_update's complaint, operator_impl.cu:86-88
        return;
    }
    if (!sample_allowed("Sampling Parameters Error", "", &pool0, 1, graph, count)) return;      // (the fan-out; enqueue_lanes' callers have asked the rest)
    lg::Range mark("op%d sample%s fanout=%d lanes=%d", op_id, is_presc ? " (presc)" : "", count, n_lanes);
    pool0->sample_used = true;              // the mode is fixed from here on (lg_pool_try_set_mode)
    if (pool0->mode.weighted) graph->MarkWeightedUsed();      // ... and so is the graph's table (legion_graph_set_edge_weights)
    lg::HopParams p;
    p.op_id = op_id;
    p.count = count;
    p.partition_count = graph->GetPartitionCount();
    p.csr_dst_node_ids = graph->GetCSRNodeMatrix(dev_id);
    // column slots only from the fill of THIS cache that built them (legion_core.h GraphStorage::BuildColumnSlots)
    const bool pairs_ok = !is_presc && pool0->slot_fs != nullptr && cache != nullptr && graph->ColumnSlotsStamp(dev_id) != 0 &&
                          graph->ColumnSlotsStamp(dev_id) == cache->FillStamp();
    p.csr_dst_x = pairs_ok ? graph->GetCSRXMatrix(dev_id) : nullptr;
    p.col_full = graph->GetCSRNodeMatrixCPU();
    p.colx_full = p.csr_dst_x != nullptr ? graph->GetColumnSlotsFull(dev_id) : nullptr;
    p.row_hdr = graph->GetRowHeaders(dev_id);
    p.last_hop = (size_t)(op_id / INTRABATCH_CON) + 1 >= pool0->max_new.size();
    p.is_presc = is_presc;
    const size_t hop = (size_t)(op_id / INTRABATCH_CON);          // slots of this hop <= B f1..fh
    p.max_slots = (int32_t)(hop < pool0->max_new.size() ? pool0->max_new[hop] : pool0->max_slots);
    p.edge_access_time = (is_presc && cache) ? cache->GetEdgeAccessedMap(dev_id) : nullptr;   // :473
    p.topo_transactions = (is_presc && cache) ? cache->Controller(dev_id)->GetTopoTransactions() : nullptr;
    p.lds_k = 1;                             // (launch_random_sample sets the hop's partition tile)
    p.mode = pool0->mode;
    p.indptr_full = graph->GetCSRNodeIndexCPU();
    p.edge_cdf = graph->EdgeCdf();
    lg::launch_random_sample(s, p, pool0->lds_bucket_bits, pool0->last_hop_claims_hint, d_lanes, n_lanes);
}

static void do_feature_lookup(hipStream_t s, UnifiedCache* cache, const LanePtrs* d_lanes, int32_t n_lanes,
                              MemoryPool* pool0, int32_t op_id, int32_t dev_id, bool use_snapshot, int32_t first_op_id = -1)
{
    if (pool0->GetFloatFeatures() == nullptr) {
        std::cout << "feature buffer not initialized\n";
        return;
    }
    if (cache->FeatureTable() == nullptr) {   // bound by FillUp (cache.cu:581-582) or legion_enqueue_batch
        std::cout << "invalid feature table ptr\n";
        return;
    }
    lg::Range mark("op%d gather lanes=%d first_op=%d", op_id, n_lanes, first_op_id);
    const int64_t max_rows = gather_row_bound(pool0->max_new.data(), (int32_t)pool0->max_new.size(), op_id, first_op_id, use_snapshot,
                                              pool0->feature_rows, pool0->num_ids);
    MemoryPool* pp = pool0;
    const bool prof = pp->prof_on && (size_t)(2 * pp->prof_used + 1) < pp->prof_events.size();
    if (prof) HIP_CALL(hipEventRecord(pp->prof_events[2 * pp->prof_used], s));
    UnifiedCache::GatherCall call;
    call.op_id = op_id;
    call.first_op_id = first_op_id;
    call.use_snapshot = use_snapshot;
    call.last_op = (size_t)(op_id / INTRABATCH_CON) + 1 >= pool0->max_new.size();
    call.max_rows = (int32_t)max_rows;
    call.grid_rows = (int32_t)std::min<int64_t>(pool0->grid_rows_hint, max_rows);
    call.out_dtype = pool0->feature_out_dtype;
    cache->FeatCacheLookup(d_lanes, n_lanes, dev_id, s, call);
    if (prof) {
        HIP_CALL(hipEventRecord(pp->prof_events[2 * pp->prof_used + 1], s));
        pp->prof_op[pp->prof_used] = op_id;
        pp->prof_used++;
    }
}

extern "C" void BatchGenerate(legion_stream_t strm_hdl, LegionFeatureStorage* feature_,
                              LegionUnifiedCache* cache_, LegionMemoryPool* memorypool_,
                              int32_t batch_size, int32_t counter, int32_t part_id, int32_t dev_id,
                              int32_t mode, bool is_presc, int32_t hop_num)
{
    (void)part_id; (void)cache_; (void)is_presc;
    FeatureStorage* feature = reinterpret_cast<FeatureStorage*>(feature_);
    MemoryPool* memorypool = reinterpret_cast<MemoryPool*>(memorypool_);
    if (feature == nullptr || memorypool == nullptr) {
        std::cout << "invalid storage ptr\n";
        return;
    }
    do_batch_generate(static_cast<hipStream_t>(strm_hdl), feature, memorypool->DeviceLane(), 1, memorypool,
                      batch_size, counter, dev_id, mode, hop_num, memorypool->iter_state);
}

extern "C" void RandomSample(legion_stream_t strm_hdl, LegionGraphStorage* graph_, LegionUnifiedCache* cache_,
                             LegionMemoryPool* memorypool_, int32_t count, int32_t dev_id, int32_t op_id,
                             bool is_presc)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    MemoryPool* memorypool = reinterpret_cast<MemoryPool*>(memorypool_);
    if (graph == nullptr || memorypool == nullptr) {
        std::cout << "invalid storage ptr\n";
        return;
    }
    do_random_sample(static_cast<hipStream_t>(strm_hdl), graph, cache_of(cache_), memorypool->DeviceLane(), 1,
                     memorypool, count, dev_id, op_id, is_presc);
}

extern "C" void FeatureCacheLookup(legion_stream_t strm_hdl, LegionUnifiedCache* cache_,
                                   LegionMemoryPool* memorypool_, int32_t op_id, int32_t dev_id)
{
    MemoryPool* memorypool = reinterpret_cast<MemoryPool*>(memorypool_);
    UnifiedCache* cache = cache_of(cache_);
    if (cache == nullptr || memorypool == nullptr) {
        std::cout << "invalid storage ptr\n";
        return;
    }
    // reference semantics: gather the CURRENT new-node range (node_counter[0..1], counter_update(op%3==1))
    do_feature_lookup(static_cast<hipStream_t>(strm_hdl), cache, memorypool->DeviceLane(), 1, memorypool, op_id,
                      dev_id, false);
}

extern "C" void IOSubmit(legion_stream_t, LegionFeatureStorage*, LegionMemoryPool*, int32_t, int32_t)
{
    // SSD tier: the reference body is commented out (operator_impl.cu:522-539); nothing to do
}

extern "C" void IOComplete(legion_stream_t strm_hdl, LegionUnifiedCache* cache_, LegionMemoryPool* memorypool_,
                           int32_t dev_id, int32_t mode)
{
    MemoryPool* memorypool = reinterpret_cast<MemoryPool*>(memorypool_);
    UnifiedCache* cache = cache_of(cache_);
    if (memorypool == nullptr) {
        std::cout << "invalid storage ptr\n";
        return;
    }
    hipStream_t s = static_cast<hipStream_t>(strm_hdl);
    if (mode == TRAINMODE && cache != nullptr)   // CacheProfiling only in train mode (:558,:578)
        cache->CacheProfiling(memorypool->GetSampledIds(), memorypool->GetAggSrcId(), memorypool->GetAggDstId(),
                              memorypool->GetAggSrcOf(), memorypool->GetAggDstOf(), memorypool->GetNodeCounter(),
                              memorypool->GetEdgeCounter(), s, dev_id);
    lg::launch_end_of_batch(s, memorypool->DeviceLane(), 1, memorypool->iter_state);
}

// =============================================================================================
// SS/engine/operator.cu:15-122
class BatchGenerateOP : public Operator {
public:
    explicit BatchGenerateOP(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        MemoryPool* memorypool = (MemoryPool*)(params->memorypool);
        IPCEnv* env = (IPCEnv*)(params->env);
        const int32_t device_id = params->device_id;
        const int32_t mode = memorypool->GetCurrentMode();
        const int32_t iter = memorypool->GetIter();
        const int32_t batch_size = env->GetCurrentBatchsize(device_id, mode);
        BatchGenerate(params->stream, (LegionFeatureStorage*)params->feature, (LegionUnifiedCache*)params->cache,
                      (LegionMemoryPool*)memorypool, batch_size, iter, device_id, device_id, mode,
                      params->is_presc, params->hop_num);
        HIP_CALL(hipEventRecord(params->event, params->stream));
    }
private:
    int op_id_;
};
Operator* NewBatchGenerateOP(int op_id) { return new BatchGenerateOP(op_id); }

class RandomSampleOP : public Operator {
public:
    explicit RandomSampleOP(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        RandomSample(params->stream, (LegionGraphStorage*)params->graph, (LegionUnifiedCache*)params->cache,
                     (LegionMemoryPool*)params->memorypool, params->neighbor_count, params->device_id, op_id_,
                     params->is_presc);
        HIP_CALL(hipEventRecord(params->event, params->stream));
    }
private:
    int op_id_;
};
Operator* NewRandomSampleOP(int op_id) { return new RandomSampleOP(op_id); }

class CacheLookupOP : public Operator {
public:
    explicit CacheLookupOP(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        FeatureCacheLookup(params->stream, (LegionUnifiedCache*)params->cache,
                           (LegionMemoryPool*)params->memorypool, op_id_, params->device_id);
        HIP_CALL(hipEventRecord(params->event, params->stream));
    }
private:
    int op_id_;
};
Operator* NewCacheLookupOP(int op_id) { return new CacheLookupOP(op_id); }

class SSDIOSubmitOP : public Operator {
public:
    explicit SSDIOSubmitOP(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        IOSubmit(params->stream, (LegionFeatureStorage*)params->feature, (LegionMemoryPool*)params->memorypool,
                 op_id_, params->device_id);
        HIP_CALL(hipEventRecord(params->event, params->stream));
    }
private:
    int op_id_;
};
Operator* NewSSDIOSubmitOP(int op_id) { return new SSDIOSubmitOP(op_id); }

class SSDIOCompleteOP : public Operator {
public:
    explicit SSDIOCompleteOP(int op_id) : op_id_(op_id) {}
    void run(OpParams* params) override
    {
        MemoryPool* memorypool = (MemoryPool*)(params->memorypool);
        IOComplete(params->stream, (LegionUnifiedCache*)params->cache, (LegionMemoryPool*)memorypool,
                   params->device_id, memorypool->GetCurrentMode());
        HIP_CALL(hipEventRecord(params->event, params->stream));
    }
private:
    int op_id_;
};
Operator* NewSSDIOCompleteOP(int op_id) { return new SSDIOCompleteOP(op_id); }

// ---- kernel-level C entry points ----------------------------------------------------------
extern "C" int32_t legion_gather_rows_fmt(legion_stream_t stream, int32_t dtype, int32_t out_dtype, const void* full_table,
                                          const void* const* cache_tables, const int32_t* node_map, int32_t node_capacity,
                                          int32_t float_feature_len, int32_t total_num_nodes, const int32_t* sampled_ids,
                                          const int32_t* node_slot, int32_t* cache_index_out, const int32_t* range_devptr, void* dst,
                                          int32_t max_rows, int32_t dst_rows, int32_t grid_rows, int32_t last_op, int32_t* plan_out)
{
    lg::GatherParams g;
    g.replica = nullptr;
    g.replica_rows = 0;
    g.Kg = 1;
    g.member = 0;
    g.striped = true;               // the caller's node_map may address several tables: always decode (owner, row)
    g.stats = nullptr;
    g.full_table = static_cast<const float*>(full_table);
    g.cache_tables = reinterpret_cast<const float* const*>(cache_tables);
    g.local_table = nullptr;
    g.node_map = node_map;
    g.node_capacity = node_capacity;
    g.D = float_feature_len;
    g.skip_remote = false;
    g.grid_rows = grid_rows;
    g.last_op = last_op != 0;
    g.hybrid = false;
    g.hybrid_cpu_cap = g.hybrid_gpu_cap = 0;
    g.hybrid_cpu_cache = nullptr;
    g.total_num_nodes = total_num_nodes;
    g.max_rows = max_rows;
    g.dtype = dtype;
    g.pitch = lg_feature_pitch(dtype, float_feature_len);
    g.out_dtype = out_dtype;
    return lg::launch_gather_explicit(static_cast<hipStream_t>(stream), g, sampled_ids, node_slot, cache_index_out, range_devptr, dst,
                                      dst_rows, plan_out);
}

extern "C" void legion_gather_rows(legion_stream_t stream, const float* full_table,
                                   const float* const* cache_tables, const int32_t* node_map,
                                   int32_t node_capacity, int32_t float_feature_len, int32_t total_num_nodes,
                                   const int32_t* sampled_ids, int32_t* cache_index_out,
                                   const int32_t* range_devptr, float* dst, int32_t max_rows)
{
    legion_gather_rows_fmt(stream, LEGION_FEATURE_F32, LEGION_FEATURE_F32, full_table, reinterpret_cast<const void* const*>(cache_tables),
                           node_map, node_capacity, float_feature_len, total_num_nodes, sampled_ids, nullptr, cache_index_out,
                           range_devptr, dst, max_rows, 0x7FFFFFFF, 0, 1, nullptr);
}

extern "C" void legion_draw_batch(legion_stream_t stream, const int32_t* idx, const int32_t* deg, int32_t* out,
                                  int32_t n)
{
    lg::launch_draw_batch(static_cast<hipStream_t>(stream), idx, deg, out, n);
}

extern "C" void legion_draw_weighted_batch(legion_stream_t stream, const int32_t* idx, const int64_t* row_start, const int32_t* deg,
                                           const float* cdf, int32_t* out, int32_t n)
{
    lg::launch_draw_weighted_batch(static_cast<hipStream_t>(stream), idx, row_start, deg, cdf, out, n);
}

extern "C" int32_t legion_draw_distinct_batch(legion_stream_t stream, const int32_t* base, const int32_t* deg, int32_t f,
                                              int32_t* out, int32_t n)
{
    if (f < 1 || f > LG_DISTINCT_MAX_FANOUT || n < 0) return -1;
    lg::launch_draw_distinct_batch(static_cast<hipStream_t>(stream), base, deg, f, out, n);
    return 0;
}

// Random walks over the full CSR (the rule: legion_hip.h; the refusals: walk_rule.h).  Every check comes before the launch: a refused
// call enqueues nothing and touches no buffer.
static lg::WalkParams walk_params(GraphStorage* graph, const int32_t* seeds, int32_t num_walks, int32_t length, int32_t weighted,
                                  float restart_prob, int64_t base, int32_t* traces, int64_t* edge_ids)
{
    return lg::WalkParams{.indptr = graph->GetCSRNodeIndexCPU(), .col = graph->GetCSRNodeMatrixCPU(),
                          .edge_cdf = weighted == 1 ? graph->EdgeCdf() : nullptr, .seeds = seeds, .traces = traces, .edge_ids = edge_ids,
                          .node_num = graph->NodeNum(), .num_walks = num_walks, .length = length, .restart_prob = restart_prob, .base = base};
}

extern "C" int32_t legion_random_walk(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* seeds_devptr, int32_t num_walks,
                                      int32_t length, int32_t weighted, float restart_prob, int64_t base, int32_t* traces_out,
                                      int64_t* edge_ids_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !seeds_devptr || !traces_out) return -1;
    if (walk_refusal(num_walks, length, base, weighted, graph->EdgeCdf() != nullptr, restart_prob) != WalkRefusal::Ok) return -1;
    if (num_walks == 0) return 0;
    if (weighted == 1) graph->MarkWeightedUsed();       // the table stays as it is from here on, as after a weighted hop
    lg::launch_random_walk(static_cast<hipStream_t>(stream),
                           walk_params(graph, seeds_devptr, num_walks, length, weighted, restart_prob, base, traces_out, edge_ids_out));
    return 0;
}

// node2vec walks (the rule: legion_hip.h; the refusals and the bias in double: node2vec_rule.h).  As above: every check comes before
// the launch.  p == q == 1 runs the node2vec kernel too: it is that kernel's pin against random_walk_kernel.
extern "C" int32_t legion_node2vec_walk(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* seeds_devptr, int32_t num_walks,
                                        int32_t length, float p, float q, int32_t weighted, int32_t max_tries, int64_t base,
                                        int32_t* traces_out, int64_t* edge_ids_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !seeds_devptr || !traces_out) return -1;
    if (node2vec_refusal(num_walks, length, base, weighted, graph->EdgeCdf() != nullptr, max_tries, p, q, graph->RowsSorted()) !=
        Node2vecRefusal::Ok)
        return -1;
    if (num_walks == 0) return 0;
    if (weighted == 1) graph->MarkWeightedUsed();
    const Node2vecBias bias = node2vec_bias(p, q);
    const lg::Node2vecParams k{.walk = walk_params(graph, seeds_devptr, num_walks, length, weighted, 0.0f, base, traces_out, edge_ids_out),
                               .a = bias.a, .b = bias.b, .mx = bias.mx, .lo = bias.lo, .hi = bias.hi, .max_tries = max_tries};
    lg::launch_node2vec_walk(static_cast<hipStream_t>(stream), k);
    return 0;
}

// PinSAGE's neighbour sampler (the rule: legion_hip.h; the refusals: walk_rule.h).  As above: every check comes before the launch.
extern "C" int32_t legion_pinsage_neighbors(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* seeds_devptr, int32_t num_seeds,
                                            int32_t num_walks_per_seed, int32_t walk_length, int32_t num_neighbors, int32_t weighted,
                                            float termination_prob, int64_t base, int32_t* neighbors_out, int32_t* counts_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !seeds_devptr || !neighbors_out || !counts_out) return -1;
    if (pinsage_refusal(num_seeds, num_walks_per_seed, walk_length, num_neighbors, base, weighted, graph->EdgeCdf() != nullptr,
                        termination_prob) != WalkRefusal::Ok)
        return -1;
    if (num_seeds == 0) return 0;
    if (weighted == 1) graph->MarkWeightedUsed();
    const lg::PinsageParams p{.walk = walk_params(graph, seeds_devptr, num_seeds, walk_length, weighted, termination_prob, base, nullptr, nullptr),
                              .walks_per_seed = num_walks_per_seed, .num_neighbors = num_neighbors, .neighbors = neighbors_out,
                              .counts = counts_out};
    lg::launch_pinsage_neighbors(static_cast<hipStream_t>(stream), p);
    return 0;
}

// The seeds of a link-prediction batch (the rules: legion_hip.h; the refusals and the scratch size: link_rule.h).  As above: every check
// comes before the launch.
extern "C" int32_t legion_find_edges(legion_stream_t stream, LegionGraphStorage* graph_, const int64_t* eids_devptr, int32_t n,
                                     int32_t* row_out, int32_t* col_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !eids_devptr || !row_out || !col_out) return -1;
    if (find_edges_refusal(n) != LinkRefusal::Ok) return -1;
    if (n == 0) return 0;
    lg::launch_find_edges(static_cast<hipStream_t>(stream), graph->GetCSRNodeIndexCPU(), graph->GetCSRNodeMatrixCPU(), graph->NodeNum(),
                          graph->EdgeNum(), eids_devptr, n, row_out, col_out);
    return 0;
}

extern "C" int32_t legion_negative_sample(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n, int32_t k,
                                          int32_t exclude, int32_t max_tries, int64_t base, int32_t* neg_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !neg_out) return -1;
    if (negative_sample_refusal(n, k, base, exclude, max_tries, graph->RowsSorted()) != LinkRefusal::Ok) return -1;
    if (n == 0) return 0;
    lg::NegativeParams p;
    p.indptr = graph->GetCSRNodeIndexCPU();
    p.col = graph->GetCSRNodeMatrixCPU();
    p.rows = rows_devptr;
    p.neg = neg_out;
    p.node_num = graph->NodeNum();
    p.n = n;
    p.k = k;
    p.exclude = exclude;
    p.max_tries = max_tries;
    p.base = base;
    lg::launch_negative_sample(static_cast<hipStream_t>(stream), p);
    return 0;
}

extern "C" int64_t legion_unique_ids_scratch_bytes(int32_t m)
{
    return unique_ids_scratch_bytes(m);
}

extern "C" int32_t legion_unique_ids(legion_stream_t stream, const int32_t* ids_devptr, int32_t m, int32_t* unique_out, int32_t* local_out,
                                     int32_t* count_out, void* scratch, int64_t scratch_bytes)
{
    if (!ids_devptr || !unique_out || !local_out || !count_out || !scratch) return -1;
    if (unique_ids_refusal(m, scratch_bytes, (uint64_t)(uintptr_t)ids_devptr, (uint64_t)(uintptr_t)unique_out, (uint64_t)(uintptr_t)local_out,
                           (uint64_t)(uintptr_t)count_out) != LinkRefusal::Ok)
        return -1;
    lg::launch_unique_ids(static_cast<hipStream_t>(stream), ids_devptr, m, unique_out, local_out, count_out, scratch,
                          unique_ids_table_slots(m), unique_ids_tiles(m));
    return 0;
}

// A neighbourhood taken whole (the rules: legion_hip.h; the refusals and the scratch size: in_edges_rule.h).  As above: every check
// comes before the launch.
extern "C" int64_t legion_row_offsets_scratch_bytes(int32_t n)
{
    return row_offsets_scratch_bytes(n);
}

extern "C" int32_t legion_row_offsets(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                      int64_t* offsets_out, void* scratch, int64_t scratch_bytes)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_out || !scratch) return -1;
    if (row_offsets_refusal(n, scratch_bytes) != InEdgesRefusal::Ok) return -1;
    lg::launch_row_offsets(static_cast<hipStream_t>(stream), graph->GetCSRNodeIndexCPU(), graph->NodeNum(), rows_devptr, n, offsets_out,
                           scratch, row_offsets_tiles(n));
    return 0;
}

// what legion_in_edges, legion_labor_count and legion_labor_edges hand the row expansion (row_slots.h)
static lg::RowSlots row_slots(GraphStorage* graph, const int32_t* rows, int32_t n, const int64_t* offsets, int64_t m)
{
    return lg::RowSlots{.indptr = graph->GetCSRNodeIndexCPU(), .col = graph->GetCSRNodeMatrixCPU(), .rows = rows, .offsets = offsets,
                        .node_num = graph->NodeNum(), .n = n, .m = m};
}

extern "C" int32_t legion_in_edges(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                   const int64_t* offsets_devptr, int64_t m, int32_t* dst_out, int32_t* src_out, int64_t* eid_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_devptr || !dst_out || !src_out) return -1;
    if (in_edges_refusal(n, m) != InEdgesRefusal::Ok) return -1;
    if (m == 0) return 0;
    const lg::InEdgesParams p{.slots = row_slots(graph, rows_devptr, n, offsets_devptr, m), .dst = dst_out, .src = src_out, .eid = eid_out};
    lg::launch_in_edges(static_cast<hipStream_t>(stream), p);
    return 0;
}

// what a pass of a kept-slot compaction takes beside the row slots (kept_slots.h).  The count pass: count, and cap 0 without outputs;
// the write pass: no count
static lg::KeptParams kept_params(int64_t m, const void* scratch, int64_t* count, int64_t cap, int32_t* dst, int32_t* src, int64_t* eid)
{
    return lg::KeptParams{.tiles = static_cast<int64_t*>(const_cast<void*>(scratch)), .count = count, .dst = dst, .src = src, .eid = eid,
                          .n_tiles = kept_tiles(m), .n_groups = kept_groups(m), .cap = cap};
}

// Layer-neighbour sampling (the rules: legion_hip.h; the hash, the predicate, the refusals and the scratch size: labor_rule.h).  As
// above: every check comes before the launch.
extern "C" int64_t legion_labor_scratch_bytes(int64_t m)
{
    return labor_scratch_bytes(m);
}

static lg::LaborParams labor_params(const lg::RowSlots& slots, const lg::KeptParams& kept, int32_t fanout, int64_t salt)
{
    return lg::LaborParams{.slots = slots, .kept = kept, .fanout = fanout, .key = labor_key(salt)};
}

extern "C" int32_t legion_labor_count(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                      const int64_t* offsets_devptr, int64_t m, int32_t fanout, int64_t salt, int64_t* count_out,
                                      void* scratch, int64_t scratch_bytes)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_devptr || !count_out || !scratch) return -1;
    if (labor_count_refusal(n, m, fanout, scratch_bytes) != LaborRefusal::Ok) return -1;
    const lg::KeptParams kept = kept_params(m, scratch, count_out, 0, nullptr, nullptr, nullptr);
    lg::launch_labor_count(static_cast<hipStream_t>(stream), labor_params(row_slots(graph, rows_devptr, n, offsets_devptr, m), kept, fanout, salt));
    return 0;
}

extern "C" int32_t legion_labor_edges(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                      const int64_t* offsets_devptr, int64_t m, int32_t fanout, int64_t salt, const void* scratch,
                                      int64_t scratch_bytes, int64_t cap, int32_t* dst_out, int32_t* src_out, int64_t* eid_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_devptr || !scratch || !dst_out || !src_out) return -1;
    if (labor_edges_refusal(n, m, fanout, scratch_bytes, cap) != LaborRefusal::Ok) return -1;
    if (cap == 0) return 0;
    const lg::KeptParams kept = kept_params(m, scratch, nullptr, cap, dst_out, src_out, eid_out);
    lg::launch_labor_edges(static_cast<hipStream_t>(stream), labor_params(row_slots(graph, rows_devptr, n, offsets_devptr, m), kept, fanout, salt));
    return 0;
}

// The k best entries of each row (the rules: legion_hip.h; the keys, the refusals and the scratch size: topk_rule.h).  As above: every
// check comes before the launch.
extern "C" int64_t legion_row_topk_scratch_bytes(int32_t n)
{
    return topk_scratch_bytes(n);
}

extern "C" int32_t legion_row_topk(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n, int32_t k,
                                   int32_t mode, const float* w_devptr, int64_t salt, int32_t* src_out, int64_t* eid_out, int32_t* count_out,
                                   void* scratch, int64_t scratch_bytes)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (topk_refusal(n, k, mode, w_devptr != nullptr, graph && rows_devptr && src_out && scratch, scratch_bytes) != TopkRefusal::Ok) return -1;
    if (n == 0) return 0;
    lg::TopkParams p{};
    p.indptr = graph->GetCSRNodeIndexCPU();
    p.col = graph->GetCSRNodeMatrixCPU();
    p.w = w_devptr;
    p.rows = rows_devptr;
    p.src = src_out;
    p.eid = eid_out;
    p.count = count_out;
    p.long_rows = static_cast<int32_t*>(scratch);
    p.node_num = graph->NodeNum();
    p.n = n;
    p.k = k;
    p.mode = mode;
    p.key = labor_key(salt);
    lg::launch_row_topk(static_cast<hipStream_t>(stream), p);
    return 0;
}

extern "C" int32_t legion_topk_keys(legion_stream_t stream, LegionGraphStorage* graph_, const int64_t* eids_devptr, int64_t n, int32_t mode,
                                    const float* w_devptr, int64_t salt, uint64_t* key_out, uint8_t* eligible_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (topk_keys_refusal(n, mode, w_devptr != nullptr, graph && eids_devptr && key_out && eligible_out) != TopkRefusal::Ok) return -1;
    if (n == 0) return 0;
    lg::launch_topk_keys(static_cast<hipStream_t>(stream), graph->GetCSRNodeMatrixCPU(), graph->EdgeNum(), w_devptr, eids_devptr, n, mode,
                         labor_key(salt), key_out, eligible_out);
    return 0;
}

// A vertex set and the subgraph it induces (the rules: legion_hip.h; the table's size, the refusals and the scratch size:
// induced_rule.h).  As above: every check comes before the launch.
extern "C" int64_t legion_node_set_bytes(int32_t k)
{
    return node_set_bytes(k);
}

// the table in the caller's memory (k, set_bytes legal).  NodeSetView repeats IdTable's fields, const, and is not built around one:
// the order of a kernel's arguments moved registers in these files, so the kernels' view stays as it was
static lg::NodeSetView node_set_view(const void* set, int32_t k)
{
    const lg::IdTable t = lg::id_table_carve(const_cast<void*>(set), node_set_slots(k));
    return lg::NodeSetView{.keys = t.keys, .first = t.first, .mask = t.mask, .shift = t.shift, .k = k, .wide = ((uintptr_t)set & 15u) == 0 ? 1 : 0};
}

extern "C" int32_t legion_node_set_build(legion_stream_t stream, const int32_t* nodes_devptr, int32_t k, void* set, int64_t set_bytes,
                                         int32_t* distinct_out)
{
    if (!nodes_devptr || !set || !distinct_out) return -1;
    if (node_set_build_refusal(k, set_bytes) != InducedRefusal::Ok) return -1;
    lg::launch_node_set_build(static_cast<hipStream_t>(stream), nodes_devptr, k, set, distinct_out);
    return 0;
}

extern "C" int32_t legion_node_set_lookup(legion_stream_t stream, const void* set, int64_t set_bytes, int32_t k, const int32_t* ids_devptr,
                                          int64_t m, int32_t* local_out)
{
    if (!set || !ids_devptr || !local_out) return -1;
    if (node_set_lookup_refusal(k, set_bytes, m) != InducedRefusal::Ok) return -1;
    if (m == 0) return 0;
    lg::launch_node_set_lookup(static_cast<hipStream_t>(stream), node_set_view(set, k), ids_devptr, m, local_out);
    return 0;
}

extern "C" int64_t legion_induced_scratch_bytes(int64_t m)
{
    return induced_scratch_bytes(m);
}

static lg::InducedParams induced_params(const lg::RowSlots& slots, const lg::KeptParams& kept, const void* set, int32_t k)
{
    return lg::InducedParams{.slots = slots, .set = node_set_view(set, k), .kept = kept};
}

extern "C" int32_t legion_induced_count(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                        const int64_t* offsets_devptr, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                                        int64_t* count_out, void* scratch, int64_t scratch_bytes)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_devptr || !set || !count_out || !scratch) return -1;
    if (induced_count_refusal(n, m, k, set_bytes, scratch_bytes) != InducedRefusal::Ok) return -1;
    const lg::KeptParams kept = kept_params(m, scratch, count_out, 0, nullptr, nullptr, nullptr);
    lg::launch_induced_count(static_cast<hipStream_t>(stream), induced_params(row_slots(graph, rows_devptr, n, offsets_devptr, m), kept, set, k));
    return 0;
}

extern "C" int32_t legion_induced_edges(legion_stream_t stream, LegionGraphStorage* graph_, const int32_t* rows_devptr, int32_t n,
                                        const int64_t* offsets_devptr, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                                        const void* scratch, int64_t scratch_bytes, int64_t cap, int32_t* dst_out, int32_t* src_local_out,
                                        int64_t* eid_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !rows_devptr || !offsets_devptr || !set || !scratch || !dst_out || !src_local_out) return -1;
    if (induced_edges_refusal(n, m, k, set_bytes, scratch_bytes, cap) != InducedRefusal::Ok) return -1;
    if (cap == 0) return 0;
    const lg::KeptParams kept = kept_params(m, scratch, nullptr, cap, dst_out, src_local_out, eid_out);
    lg::launch_induced_edges(static_cast<hipStream_t>(stream), induced_params(row_slots(graph, rows_devptr, n, offsets_devptr, m), kept, set, k));
    return 0;
}

extern "C" int32_t legion_dst_offsets(legion_stream_t stream, const int32_t* dst_devptr, int64_t cap, const int64_t* count_devptr, int32_t n,
                                      int64_t* indptr_out)
{
    if (!dst_devptr || !count_devptr || !indptr_out) return -1;
    if (dst_offsets_refusal(cap, n) != InducedRefusal::Ok) return -1;
    lg::launch_dst_offsets(static_cast<hipStream_t>(stream), dst_devptr, cap, count_devptr, n, indptr_out);
    return 0;
}

// Seed-edge exclusion (the rules: legion_hip.h; the set's size, the refusals and the scratch size: exclude_rule.h).  As above: every
// check comes before the launch.
extern "C" int32_t legion_reverse_edge_ids(legion_stream_t stream, LegionGraphStorage* graph_, const int64_t* eids_devptr, int64_t n,
                                           int32_t via, int64_t* reverse_out)
{
    GraphStorage* graph = reinterpret_cast<GraphStorage*>(graph_);
    if (!graph || !eids_devptr || !reverse_out) return -1;
    const int64_t* rindptr = nullptr;
    const int32_t* rcol = nullptr;
    const int64_t* reid = nullptr;
    const bool have_reverse = graph->ReverseCSR(&rindptr, &rcol, &reid) >= 0;
    if (reverse_edge_ids_refusal(n, via, graph->RowsSorted(), have_reverse) != ExcludeRefusal::Ok) return -1;
    if (n == 0) return 0;
    lg::ReverseIdsParams p;
    p.indptr = graph->GetCSRNodeIndexCPU();
    p.col = graph->GetCSRNodeMatrixCPU();
    p.t_indptr = via == 0 ? p.indptr : rindptr;
    p.t_col = via == 0 ? p.col : rcol;
    p.t_eid = via == 0 ? nullptr : reid;
    p.eids = eids_devptr;
    p.out = reverse_out;
    p.num_edges = graph->EdgeNum();
    p.n = n;
    p.node_num = graph->NodeNum();
    p.via = via;
    lg::launch_reverse_edge_ids(static_cast<hipStream_t>(stream), p);
    return 0;
}

extern "C" int64_t legion_edge_set_bytes(int32_t k)
{
    return edge_set_bytes(k);
}

// the set in the caller's memory (k, set_bytes legal)
static lg::EdgeSetView edge_set_view(const void* set, int32_t k)
{
    const int64_t slots = edge_set_slots(k);
    return lg::EdgeSetView{.keys = static_cast<const int64_t*>(set), .mask = (uint64_t)(slots - 1), .shift = edge_set_shift(slots)};
}

extern "C" int32_t legion_edge_set_build(legion_stream_t stream, const int64_t* eids_devptr, int32_t k, void* set, int64_t set_bytes)
{
    if (!eids_devptr || !set) return -1;
    if (edge_set_build_refusal(k, set_bytes) != ExcludeRefusal::Ok) return -1;
    lg::launch_edge_set_build(static_cast<hipStream_t>(stream), eids_devptr, k, set);
    return 0;
}

extern "C" int32_t legion_edge_set_contains(legion_stream_t stream, const void* set, int64_t set_bytes, int32_t k, const int64_t* eids_devptr,
                                            int64_t m, int32_t* member_out)
{
    if (!set || !eids_devptr || !member_out) return -1;
    if (edge_set_contains_refusal(k, set_bytes, m) != ExcludeRefusal::Ok) return -1;
    if (m == 0) return 0;
    lg::launch_edge_set_contains(static_cast<hipStream_t>(stream), edge_set_view(set, k), eids_devptr, m, member_out);
    return 0;
}

extern "C" int64_t legion_edge_filter_scratch_bytes(int64_t m)
{
    return edge_filter_scratch_bytes(m);
}

static lg::EdgeFilterParams edge_filter_params(const int32_t* dst, const int32_t* src, const int64_t* eid, int64_t m, const void* set, int32_t k,
                                               const lg::KeptParams& kept)
{
    return lg::EdgeFilterParams{.dst = dst, .src = src, .eid = eid, .m = m, .set = edge_set_view(set, k), .kept = kept};
}

extern "C" int32_t legion_edge_filter_count(legion_stream_t stream, const int32_t* dst_devptr, const int32_t* src_devptr, const int64_t* eid_devptr,
                                            int64_t m, const void* set, int64_t set_bytes, int32_t k, int64_t* count_out, void* scratch,
                                            int64_t scratch_bytes)
{
    if (!dst_devptr || !src_devptr || !eid_devptr || !set || !count_out || !scratch) return -1;
    if (edge_filter_count_refusal(m, k, set_bytes, scratch_bytes) != ExcludeRefusal::Ok) return -1;
    const lg::KeptParams kept = kept_params(m, scratch, count_out, 0, nullptr, nullptr, nullptr);
    lg::launch_edge_filter_count(static_cast<hipStream_t>(stream), edge_filter_params(dst_devptr, src_devptr, eid_devptr, m, set, k, kept));
    return 0;
}

extern "C" int32_t legion_edge_filter_edges(legion_stream_t stream, const int32_t* dst_devptr, const int32_t* src_devptr, const int64_t* eid_devptr,
                                            int64_t m, const void* set, int64_t set_bytes, int32_t k, const void* scratch, int64_t scratch_bytes,
                                            int64_t cap, int32_t* dst_out, int32_t* src_out, int64_t* eid_out)
{
    if (!dst_devptr || !src_devptr || !eid_devptr || !set || !scratch || !dst_out || !src_out) return -1;
    const uint64_t in[3] = {(uint64_t)(uintptr_t)dst_devptr, (uint64_t)(uintptr_t)src_devptr, (uint64_t)(uintptr_t)eid_devptr};
    const uint64_t out[3] = {(uint64_t)(uintptr_t)dst_out, (uint64_t)(uintptr_t)src_out, (uint64_t)(uintptr_t)eid_out};
    if (edge_filter_edges_refusal(m, k, set_bytes, scratch_bytes, cap, in, out) != ExcludeRefusal::Ok) return -1;
    if (cap == 0) return 0;
    const lg::KeptParams kept = kept_params(m, scratch, nullptr, cap, dst_out, src_out, eid_out);
    lg::launch_edge_filter_edges(static_cast<hipStream_t>(stream), edge_filter_params(dst_devptr, src_devptr, eid_devptr, m, set, k, kept));
    return 0;
}

// One whole mini-batch in the op order of GPURunner::RunOnce / RunPreSc (SS/engine/server.cu:285-332)
// without the IPC hand-off: what a Runner enqueues per batch, exposed for callers that own the
// buffers themselves (tests, bench.py, an in-process trainer).
static void enqueue_lanes(hipStream_t s, GraphStorage* graph, FeatureStorage* feature, UnifiedCache* cache,
                          const LanePtrs* d_lanes, int32_t n_lanes, MemoryPool* pool0, int32_t* iter_state,
                          int32_t batch_size, int32_t counter, int32_t dev_id, int32_t mode, bool is_presc,
                          const int32_t* fanout, int32_t hop_num, int32_t phase = LG_PHASE_ALL)
{
    if (cache == nullptr && !is_presc) {
        std::cout << "invalid cache ptr\n";     // serving needs the cache object (it owns the feature tiers)
        return;
    }
    if (cache && feature && cache->FeatureTable() == nullptr)
        cache->BindFeatureTable(feature);
    const bool profile = is_presc && mode == TRAINMODE && cache != nullptr;
    const BatchOpList ops = batch_op_list(hop_num, phase, is_presc, profile);     // batch_ops.h: the order, the op ids, which gathers share a launch
    const bool weave = phase >= LG_PHASE_HEAD;                                     // (serve mode only)
    for (int32_t i = 0; i < ops.n; i++) {
        const BatchOp& op = ops.op[i];
        switch (op.kind) {
        case BatchOpKind::Seeds:
            do_batch_generate(s, feature, d_lanes, n_lanes, pool0, batch_size, counter, dev_id, mode, hop_num, iter_state);
            break;
        case BatchOpKind::Sample:
            do_random_sample(s, graph, cache, d_lanes, n_lanes, pool0, fanout[op.hop], dev_id, op.op_id, !weave && is_presc);
            break;
        case BatchOpKind::Gather:
            do_feature_lookup(s, cache, d_lanes, n_lanes, pool0, op.op_id, dev_id, true, op.first_op_id);
            break;
        case BatchOpKind::Profile:      // CacheProfiling (one lane only in PreSC)
            cache->CacheProfiling(pool0->GetSampledIds(), pool0->GetAggSrcId(), pool0->GetAggDstId(), pool0->GetAggSrcOf(),
                                  pool0->GetAggDstOf(), pool0->GetNodeCounter(), pool0->GetEdgeCounter(), s, dev_id);
            break;
        case BatchOpKind::EndOfBatch:
            lg::launch_end_of_batch(s, d_lanes, n_lanes, iter_state);
            break;
        }
    }
}

extern "C" void legion_enqueue_batch(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                     LegionUnifiedCache* cache, LegionMemoryPool* memorypool, int32_t batch_size,
                                     int32_t counter, int32_t dev_id, int32_t mode, bool is_presc,
                                     const int32_t* fanout, int32_t hop_num)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(memorypool);
    if (!graph || !feature || !mp) { std::cout << "invalid storage ptr\n"; return; }
    if (!sample_allowed("legion_hip", "; nothing enqueued", &mp, 1, reinterpret_cast<GraphStorage*>(graph), 0)) return;
    enqueue_lanes(static_cast<hipStream_t>(strm_hdl), reinterpret_cast<GraphStorage*>(graph),
                  reinterpret_cast<FeatureStorage*>(feature), cache_of(cache), mp->DeviceLane(), 1, mp, mp->iter_state,
                  batch_size, counter, dev_id, mode, is_presc, fanout, hop_num);
}

// ---- lane groups: G independent mini-batches served by every launch ---------------------------
// `priv`: the block the group's copy of its lanes is carved from (an arena pipeline's, behind its lanes' private arrays), or null
LegionLaneGroup* lg_group_create(LegionMemoryPool** pools, int32_t n, PrivateBlock* priv)
{
    LegionLaneGroup* g = new LegionLaneGroup();
    std::vector<LanePtrs> h;
    for (int32_t i = 0; i < n; i++) {
        MemoryPool* mp = reinterpret_cast<MemoryPool*>(pools[i]);
        g->pools.push_back(mp);
        g->epochs.push_back(mp->lanes_epoch);
        h.push_back(mp->HostLane(mp->GetCurrentPipe()));
    }
    SetGPUDevice(g->pools[0]->dev_id);
    g->d_lanes = (LanePtrs*)lg_private_take(priv, (int64_t)n * sizeof(LanePtrs));
    g->lanes_carved = priv != nullptr;
    HIP_CALL(hipMemcpy(g->d_lanes, h.data(), h.size() * sizeof(LanePtrs), hipMemcpyHostToDevice));
    return g;
}
extern "C" LegionLaneGroup* legion_group_create(LegionMemoryPool** pools, int32_t n) { return lg_group_create(pools, n, nullptr); }

// a pool whose lane descriptor changed after the group was made (legion_pool_set_edge_ids: possible only before the pool has
// sampled, so never between the replays of a captured graph): its entry of d_lanes is written again
extern "C" void legion_group_refresh(LegionLaneGroup* g)
{
    if (!g) return;
    for (size_t i = 0; i < g->pools.size(); i++) {
        MemoryPool* mp = g->pools[i];
        if (g->epochs[i] == mp->lanes_epoch) continue;
        SetGPUDevice(mp->dev_id);
        const LanePtrs h = mp->HostLane(mp->GetCurrentPipe());
        HIP_CALL(hipMemcpy(g->d_lanes + i, &h, sizeof(LanePtrs), hipMemcpyHostToDevice));
        g->epochs[i] = mp->lanes_epoch;
    }
}

extern "C" void legion_group_set_iter_state(LegionLaneGroup* g, int32_t* iter_state_devptr) { if (g) g->iter_state = iter_state_devptr; }
// device address of lane `lane`'s descriptor (GPURunner: the source of a hand-over copy)
extern "C" const void* legion_group_lane_desc(LegionLaneGroup* g, int32_t lane)
{
    return (g && lane >= 0 && lane < (int32_t)g->pools.size()) ? (const void*)(g->d_lanes + lane) : nullptr;
}

extern "C" void legion_group_destroy(LegionLaneGroup* g)
{
    if (!g) return;
    if (!g->lanes_carved) d_free_space(g->d_lanes);
    delete g;
}

// Lane i of the group produces batch `counter0 + i` (serve mode).  One launch of every kernel covers
// all lanes (grid.y = lanes).
extern "C" void legion_enqueue_group_phase(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                           LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t n_active,
                                           int32_t batch_size, int32_t counter0, int32_t dev_id, int32_t mode,
                                           const int32_t* fanout, int32_t hop_num, int32_t phase)
{
    if (!graph || !feature || !group || group->pools.empty()) { std::cout << "invalid storage ptr\n"; return; }
    if (n_active < 1 || n_active > (int32_t)group->pools.size()) n_active = (int32_t)group->pools.size();
    // every lane samples with lane 0's modes (HopParams is shared by the launch): lanes that disagree are refused, and every lane's
    // modes are fixed from here on (lg_pool_try_set_mode)
    {
        bool stale = false;
        for (size_t i = 0; i < group->pools.size(); i++) stale |= group->epochs[i] != group->pools[i]->lanes_epoch;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (stale) HIP_CALL(hipStreamIsCapturing(static_cast<hipStream_t>(strm_hdl), &cap));
        if (stale && cap != hipStreamCaptureStatusNone) {      // (a copy cannot run inside a capture: legion_pipeline_set_edge_ids refreshes its groups itself)
            printf("legion_hip: a lane's mode changed after its group was made; nothing captured\n");
            for (int32_t j = 0; j < n_active; j++) group->pools[j]->RaiseError(LG_ERR_SAMPLE_MODE);
            return;
        }
        if (stale) legion_group_refresh(group);
    }
    if (!sample_allowed("legion_hip", "; nothing enqueued", group->pools.data(), n_active, reinterpret_cast<GraphStorage*>(graph), 0)) return;
    for (int32_t i = 0; i < n_active; i++) group->pools[i]->sample_used = true;
    if (group->pools[0]->mode.weighted) reinterpret_cast<GraphStorage*>(graph)->MarkWeightedUsed();
    enqueue_lanes(static_cast<hipStream_t>(strm_hdl), reinterpret_cast<GraphStorage*>(graph),
                  reinterpret_cast<FeatureStorage*>(feature), cache_of(cache), group->d_lanes, n_active, group->pools[0],
                  group->iter_state, batch_size, counter0, dev_id, mode, false, fanout, hop_num, phase);
}

extern "C" void legion_enqueue_group_n(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                       LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t n_active,
                                       int32_t batch_size, int32_t counter0, int32_t dev_id, int32_t mode,
                                       const int32_t* fanout, int32_t hop_num)
{
    legion_enqueue_group_phase(strm_hdl, graph, feature, cache, group, n_active, batch_size, counter0, dev_id, mode,
                               fanout, hop_num, LG_PHASE_ALL);
}

extern "C" void legion_enqueue_group(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                     LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t batch_size,
                                     int32_t counter0, int32_t dev_id, int32_t mode, const int32_t* fanout,
                                     int32_t hop_num)
{
    legion_enqueue_group_n(strm_hdl, graph, feature, cache, group, 0, batch_size, counter0, dev_id, mode, fanout, hop_num);
}

// Diagnostics (bench.py's roofline.cold / roofline.warm_again, tools/): the gather of the group's LAST op once more, over the lanes as
// they stand -- same kernel instance, same grid, same ranges (the hop snapshot in hop_scratch) as inside a group's op list.
extern "C" void legion_enqueue_group_last_gather(legion_stream_t strm_hdl, LegionUnifiedCache* cache, LegionLaneGroup* group,
                                                 int32_t n_active, int32_t dev_id, int32_t hop_num)
{
    if (!cache || !group || group->pools.empty() || hop_num < 1) { std::cout << "invalid cache/group ptr\n"; return; }
    if (n_active < 1 || n_active > (int32_t)group->pools.size()) n_active = (int32_t)group->pools.size();
    do_feature_lookup(static_cast<hipStream_t>(strm_hdl), cache_of(cache), group->d_lanes, n_active, group->pools[0],
                      batch_whole_gather(hop_num).op_id, dev_id, true, -1);
}

// ---- gather-op timing (HIP events recorded on the op's stream around the gather launch) -------
extern "C" void legion_pool_profile_begin(LegionMemoryPool* p_, int32_t max_ops)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) return;
    SetGPUDevice(mp->dev_id);
    while ((int32_t)mp->prof_events.size() < 2 * max_ops) {
        hipEvent_t e;
        HIP_CALL(hipEventCreate(&e));
        mp->prof_events.push_back(e);
    }
    mp->prof_op.assign(max_ops, -1);
    mp->prof_used = 0;
    mp->prof_on = true;
}

// Stops recording; out_ms[i] / out_op[i] = elapsed time and op id of the i-th timed gather.
// The caller must have synchronised the stream.  Returns the number of timed ops.
extern "C" int32_t legion_pool_profile_end(LegionMemoryPool* p_, float* out_ms, int32_t* out_op, int32_t cap)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) return 0;
    mp->prof_on = false;
    int32_t n = mp->prof_used < cap ? mp->prof_used : cap;
    for (int32_t i = 0; i < n; i++) {
        HIP_CALL(hipEventElapsedTime(&out_ms[i], mp->prof_events[2 * i], mp->prof_events[2 * i + 1]));
        out_op[i] = mp->prof_op[i];
    }
    return n;
}
