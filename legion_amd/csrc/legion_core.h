// legion_core.h -- host-side object model of the MI355X sampling server.
//
// The class and method names mirror the reference's plugin/operator interface for the hot path
// (paths relative to the reference repo, SS = sampling_server/src):
//   Operator / OpParams            SS/engine/operator.h:4-28
//   Server / Runner / RunnerParams SS/engine/server.h:5-33
//   MemoryPool                     SS/engine/memorypool.cuh:20-221
//   GraphStorage                   SS/storage/graph_storage.cuh:7-24
//   FeatureStorage                 SS/storage/feature_storage.cuh:6-34
//   CacheController / UnifiedCache SS/cache/cache.cuh:10-177
//   IPCEnv                         SS/engine/ipc_service.h:6-35
// The implementations are new: device-resident counters (no host read-backs), first touches
// resolved bucket by bucket in LDS instead of bitmap + position map (no per-vertex state at all),
// direct-mapped id->slot tables instead of the vendored cuckoo hash, deterministic slot-ordered compaction.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/legion_hip.h"
#include "sample_mode.h"
#include "sample_plan.h"
#include "pool_plan.h"
#include "claim_rule.h"      // lg_tab_hash, the claim pair, lg_claim_at, LG_SLOT_LOSER: the formats the sampler's kernels talk through

#define INTERBATCH_CON LEGION_INTERBATCH_CON
#define INTRABATCH_CON LEGION_INTRABATCH_CON
#define MAX_DEVICE LEGION_MAX_DEVICE
#define MEMORY_USAGE LEGION_MEMORY_USAGE
#define TRAINMODE LEGION_TRAINMODE
#define VALIDMODE LEGION_VALIDMODE
#define TESTMODE LEGION_TESTMODE
#define CACHEMISS_FLAG LEGION_CACHEMISS_FLAG

// Error convention of the reference (cudaCheckError, SS/engine/operator_impl.cu:16-24): print and exit.
#define hipCheckError()                                                                       \
    {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess) {                                                               \
            printf("HIP failure %s:%d: '%s'\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            exit(EXIT_FAILURE);                                                               \
        }                                                                                     \
    }
#define HIP_CALL(expr)                                                                        \
    {                                                                                         \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            printf("HIP failure %s:%d: '%s'\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            exit(EXIT_FAILURE);                                                               \
        }                                                                                     \
    }

// ---- first touches without per-vertex state (replaces accessed_map + position_map) ----------
// The reference marks first touches with atomicOr on an N-bit map it memsets per batch and keeps positions in an N-entry map it
// clears node by node (operator_impl.cu:151,244-272,542-548).  Here a hop issues no memory-side atomic per claim and keeps
// nothing per vertex: a hop's claims (vertex, slot) are written, grouped by hash bucket, into one list per bucket of the lane
// (ranks by LDS atomics, one reservation per bucket and tile); a second kernel gives every (lane, bucket) a workgroup that builds
// an open-addressing table of the bucket's vertices IN LDS -- the batch's known vertices of that bucket (the seeds from
// sampled_ids, the nodes earlier hops added from the bucket's known list, which list_known_kernel keeps) with their positions,
// then the claims with atomicMin on (vertex, pending | slot) -- and marks every claim that is not the lowest slot of a new
// vertex.  Nothing survives the hop, nothing to clear, nothing that scales with N.  A bucket whose vertices do not fit the
// table is handled in several passes over sub-buckets, so the result never depends on the hash.
// Buckets per lane (8, 16, 64 or 256) follow the pool's largest hop; the classes, their constants and every launch decision that
// rests on them are in sample_plan.h.
// (Rounds 1-4 also had a uint32[N] array per lane and a per-lane open-addressing table in memory, claimed with one atomicMin per
// pick: slower by 5-14 % wherever the LDS form applied, removed in round 5 when it applied everywhere -- DESIGN_HISTORY.md.)
// feature row format (legion_hip.h LEGION_FEATURE_*): elements per stored row and its bytes
static inline int32_t lg_feature_pitch(int32_t dtype, int32_t D) { return dtype == LEGION_FEATURE_BF16 ? (D + 7) & ~7 : D; }
static inline int64_t lg_feature_row_bytes(int32_t dtype, int32_t D)
{
    return dtype == LEGION_FEATURE_BF16 ? (int64_t)lg_feature_pitch(dtype, D) * 2 : (int64_t)D * 4;
}

// per-hop scratch written by the scan kernel, read by scatter / localise (device int32[16])
enum HopScratch {
    HS_FRONTIER_IS_SEEDS = 0,
    HS_FRONTIER_OFF = 1,   // offset of the frontier inside agg_src_ids / agg_src_off
    HS_FRONTIER_LEN = 2,
    HS_NODE_BASE = 3,
    HS_EDGE_BASE = 4,
    HS_N_NEW = 5,
    HS_N_EDGE = 6,
    HS_SLOTS = 7,
    HS_CTICKET = 24,       // compact_kernel: next super tile to hand out / workgroups that finished (both zero between hops)
    HS_CDONE = 25,
    HS_ERROR = 29,         // sticky error bits of the lane (LG_ERR_*), also mirrored to the pool's host-visible flag
    HS_RANGE = 10,         // [HS_RANGE + 2h], [+1]: {offset, count} of the new nodes of op 3h, kept for its gather
    HS_WORDS = 32
};
static_assert(HS_WORDS == POOL_HOP_SCRATCH_WORDS, "pool_plan.h sizes hop_scratch");

// error bits a kernel can raise for its lane (MemoryPool::ErrorBits / legion_pool_error)
#define LG_ERR_TABLE_FULL 1       // a de-duplication bucket did not fit its LDS table even in 2^14 sub-bucket passes (not a hash problem: cannot happen)
#define LG_ERR_FEATURE_ROWS 2     // the batch has more rows than the feature buffer: the gather stopped at its end
#define LG_ERR_CHAIN 4            // compact_kernel gave up waiting for an earlier tile's status word / a winner's position (cannot happen)
#define LG_ERR_SAMPLE_MODE 8      // a hop was not sampled: a fan-out above LG_DISTINCT_MAX_FANOUT without replacement, or lanes of one
                                  // group with different sampling, edge-id or weighted modes (set on the host; the setters refuse
                                  // these), or a weighted hop against a graph without a prefix table (legion_graph_set_edge_weights)

// Device code: a pointer that was loaded from memory (LanePtrs, pointer tables, LDS) is "generic" to
// the compiler, which then emits flat_* instructions; those count on lgkmcnt as well as vmcnt, so every
// LDS wait also waits for the memory operations in flight.  Kernels cast such pointers to the global
// address space once (every buffer of this library is HBM, peer HBM or mapped host memory).
#define LG_G __attribute__((address_space(1)))
#define LG_GPTR(T, p) ((LG_G T*)(p))

// phases of a whole-batch enqueue (legion_enqueue_group_phase): LG_PHASE_* and the ops each of them issues, in order, are
// batch_ops.h's (batch_op_list)
#include "batch_ops.h"
static_assert(BATCH_OP_STRIDE == INTRABATCH_CON, "batch_ops.h numbers the ops of a batch as the counters do");

// Feature-cache slot of a sampled neighbour, carried from the sampler to the gather (see "column slots", GraphStorage):
// a value >= 0 or CACHEMISS_FLAG is what node_map[id] holds; LG_FS_UNKNOWN means "not carried: look it up"
#define LG_FS_UNKNOWN (-3)
// (slot_dst[slot] of a hop and its loser mark LG_SLOT_LOSER: claim_rule.h)

// Per-vertex row header: where the adjacency of v lives (slot of the CSR pointer tables: P = the
// full CSR, d < P = GPU d's cached CSR), its first edge and its degree.  One 16-byte read resolves
// what the reference does with two hash finds + two indptr reads (cache.cu:217-225,
// operator_impl.cu:224-230).
struct alignas(16) RowHdr {
    int64_t start;
    int32_t deg;
    int32_t slot;
};
static_assert(sizeof(RowHdr) == POOL_ROW_HDR_BYTES, "pool_plan.h sizes fh_edge");

struct BuildInfo {  // SS/include/buildinfo.h (only the fields of the in-memory path)
    int32_t partition_count = 0;
    std::vector<int32_t> training_set_num, validation_set_num, testing_set_num;
    std::vector<std::vector<int32_t>> training_set_ids, training_labels;
    std::vector<std::vector<int32_t>> validation_set_ids, validation_labels;
    std::vector<std::vector<int32_t>> testing_set_ids, testing_labels;
    int32_t total_num_nodes = 0;
    int32_t float_feature_len = 0;
    float* host_float_feature = nullptr;   // device-dereferenceable (HBM or mapped pinned)
    int32_t feature_dtype = LEGION_FEATURE_F32;   // row format of host_float_feature (LEGION_FEATURE_*)
    int64_t* csr_node_index = nullptr;     // device-dereferenceable
    int32_t* csr_dst_node_ids = nullptr;
    int64_t total_edge_num = 0;
    int32_t epoch = 0;
    int32_t raw_batch_size = 0;
};

// Everything a kernel needs to know about ONE in-flight mini-batch (a lane): the buffers of its
// MemoryPool.  Arrays of these live in device memory; kernels are launched with grid.y = number of
// lanes and each workgroup works on lanes[blockIdx.y], so one launch serves a whole group of
// independent mini-batches (the per-kernel latency floor is paid once per group, not per batch).
struct LanePtrs {
    int32_t* sampled_ids;
    int32_t* labels;
    int32_t* agg_src_ids;
    int32_t* agg_dst_ids;
    int32_t* agg_src_off;
    int32_t* agg_dst_off;
    char* tmp_part_ind;
    // first touches (no per-vertex state, see above): the hop's claims, one list per hash bucket
    unsigned long long* claim_pairs;   // (vertex << 32 | slot): [buckets][claim_cap], interleaved by chunk (below)
    int32_t* run_off;                  // 256-bucket class: [partition tiles][buckets] x {first place in the bucket's claim list, count} (sample_kernel -> place_kernel)
    int32_t lds_buckets;               // 8, 16, 64 or 256
    // one list of claims per bucket: the sampling kernel reserves places for a super tile's (8/16 buckets) or a partition tile's
    // (64/256 buckets) claims of a bucket with one atomic on claim_cnt[bucket]; a count beyond claim_cap says the list is incomplete
    // and the bucket's workgroup reads the hop's slots instead (kernels_sample.hip)
    // The lists are interleaved in chunks of LG_CLAIM_CHUNK entries -- entry k of bucket b sits at lg_claim_at(b, k, buckets) --
    // so that what a hop really uses (a fraction of the capacity) is one dense prefix of the array, as few pages as the segment form
    // touches (measured: with one contiguous region per bucket, 16 x oversized, both kernels lost ~15 us per group to translation misses)
    int32_t* claim_cnt;                // [buckets], zero between hops
    int32_t claim_cap;
    int32_t ids_cap;                   // capacity of sampled_ids (what may be read before the live counters are known)
    // ... and the batch's vertices that later hops must recognise (every node but the seeds and the last hop's), one list
    // per bucket: scatter appends (vertex << 32 | position), the next hop's workgroup of that bucket reads only its list
    unsigned long long* known_pairs;   // [buckets][known_cap]
    int32_t* known_cnt;                // [buckets] entries appended (may exceed known_cap: then the list is not used)
    int32_t known_cap;
    int32_t* err_flag;                 // mapped pinned host word: kernels OR LG_ERR_* bits into it
    int32_t* counter_mirror;           // mapped pinned host int32[32] or null: the end-of-batch kernel leaves the batch's
                                       // node_counter / edge_counter there (GPURunner's lanes: no device read-back per hand-over)
    const void* deliver;               // lg::DeliverParams* (device) or null: the gather of this lane also hands its batch
                                       // over to that trainer-visible pipe slot (GPURunner's hand-over descriptors)
    int32_t* node_counter;
    int32_t* edge_counter;
    int32_t* slot_dst;
    int32_t* slot_pos;                 // [max_slots] -1, or for a loser: the vertex's position / -2 - (the winning slot); winners publish their position here
    int32_t* slot_fs;                  // [max_slots] feature-cache slot of the slot's sampled neighbour, or LG_FS_UNKNOWN (column slots)
    int32_t* node_slot;                // [num_ids] the same per node of the batch, by position in sampled_ids: what the gather reads
                                       // instead of node_map[id] (one 128-byte line per row for 4 bytes)
    unsigned long long* tile_state;    // [super tiles] look-back status words of compact_kernel (zero between hops)
    int32_t* hop_scratch;
    RowHdr* fh_edge;
    int32_t* cache_search_buffer;
    float* float_features;
    int32_t feature_rows;
    int32_t max_slots;
    // edge-id mode (MemoryPool::mode.edge_ids), else both null: the adjacency position each slot drew (sample_kernel -> compact_kernel)
    // and, per edge of the batch, its position in the FULL CSR's column array -- indexed like agg_src_ids
    int32_t* slot_pick;                // [max_slots]
    int64_t* agg_edge_ids;             // [num_ids]
};

// Where a pool's memory comes from.  Default (all null): one allocation per array.  `arena`: the trainer-visible arrays (sampled_ids,
// features, labels, agg_src_off, agg_dst_off, the two counter blocks) of a pool of depth 1 are carved from it -- GPURunner's and an
// arena pipeline's ONE exportable allocation for every lane, so that a trainer end opens it once and takes a batch as views of its
// lane -- and the counters are mirrored to its host-visible block.  `priv`: the lane-private arrays (pool_plan.h) are carved from one
// block of shuffled chunks as well (measured: +0.9 % on the whole job, +4 % on the sampler chain, against both separate allocations
// and one plain block); never freed one by one: the block goes when its pipeline goes.  claims_hint: what PreSC saw of the LAST hop,
// the largest one -- its edges (= the claims its de-duplication takes) and the batch's nodes before it, maxima over the PreSC
// batches; 0, 0 = unknown -- picks the small class's bucket count (sample_plan.h).
struct PoolArena {
    char* base = nullptr;
    int64_t bytes = 0, used = 0;
    int32_t* mirror_host = nullptr;    // [mirror_lanes][32] mapped pinned host memory ...
    int32_t* mirror_dev = nullptr;     // ... and its device address
    int32_t mirror_lanes = 0, mirror_used = 0;
};
struct PrivateBlock { char* base = nullptr; int64_t bytes = 0, used = 0; };
struct PoolSource {
    PoolArena* arena = nullptr;
    PrivateBlock* priv = nullptr;
    int64_t claims_hint[2] = {0, 0};
};
PrivateBlock* lg_private_block_create(int64_t bytes, int32_t scatter_mb);
void lg_private_block_destroy(PrivateBlock* b);
// `bytes` (rounded up to 256) from the block, or from d_alloc_space where there is none; a block too small is fatal
void* lg_private_take(PrivateBlock* b, int64_t bytes);

// ---------------------------------------------------------------------------------------------
class MemoryPool {
public:
    explicit MemoryPool(int32_t pipeline_depth)
        : pipeline_depth_(pipeline_depth), float_features_(pipeline_depth, nullptr),
          labels_(pipeline_depth, nullptr), node_counter_(pipeline_depth, nullptr),
          edge_counter_(pipeline_depth, nullptr), sampled_ids_(pipeline_depth, nullptr),
          agg_src_off_(pipeline_depth, nullptr), agg_dst_off_(pipeline_depth, nullptr) {}

    int32_t GetIter() const { return iter_; }
    int32_t GetCurrentMode() const { return mode_; }
    int32_t GetCurrentPipe() const { return current_pipe_; }
    int32_t PipelineDepth() const { return pipeline_depth_; }
    float* GetFloatFeatures() const { return float_features_[current_pipe_]; }
    int32_t* GetCacheSearchBuffer() const { return cache_search_buffer_; }
    int32_t* GetLabels() const { return labels_[current_pipe_]; }
    int32_t* GetPositionMap() const { return nullptr; }      // (the reference's accessor, memorypool.cuh:120-135: no such array here)
    int32_t* GetNodeCounter() const { return node_counter_[current_pipe_]; }
    int32_t* GetEdgeCounter() const { return edge_counter_[current_pipe_]; }
    int32_t* GetSampledIds() const { return sampled_ids_[current_pipe_]; }
    int32_t* GetAggSrcId() const { return agg_src_ids_; }
    int32_t* GetAggDstId() const { return agg_dst_ids_; }
    int32_t* GetAggSrcOf() const { return agg_src_off_[current_pipe_]; }
    int32_t* GetAggDstOf() const { return agg_dst_off_[current_pipe_]; }
    char* GetTmpPartIdx() const { return tmp_part_ind_; }
    int32_t* GetTmpPartOff() const { return tmp_part_off_; }

    void SetFloatFeatures(float* p, int32_t pipe) { float_features_[pipe] = p; lanes_dirty_ = true; }
    void SetCacheSearchBuffer(int32_t* p) { cache_search_buffer_ = p; lanes_dirty_ = true; }
    void SetLabels(int32_t* p, int32_t pipe) { labels_[pipe] = p; lanes_dirty_ = true; }
    void SetNodeCounter(int32_t* p, int32_t pipe) { node_counter_[pipe] = p; lanes_dirty_ = true; }
    void SetEdgeCounter(int32_t* p, int32_t pipe) { edge_counter_[pipe] = p; lanes_dirty_ = true; }
    void SetSampledIds(int32_t* p, int32_t pipe) { sampled_ids_[pipe] = p; lanes_dirty_ = true; }
    void SetAggSrcId(int32_t* p) { agg_src_ids_ = p; lanes_dirty_ = true; }
    void SetAggDstId(int32_t* p) { agg_dst_ids_ = p; lanes_dirty_ = true; }
    void SetAggSrcOf(int32_t* p, int32_t pipe) { agg_src_off_[pipe] = p; lanes_dirty_ = true; }
    void SetAggDstOf(int32_t* p, int32_t pipe) { agg_dst_off_[pipe] = p; lanes_dirty_ = true; }
    void SetTmpPartIdx(char* p) { tmp_part_ind_ = p; lanes_dirty_ = true; }
    void SetTmpPartOff(int32_t* p) { tmp_part_off_ = p; }
    void SetCurrentPipe(int32_t pipe) { current_pipe_ = pipe; }
    LanePtrs HostLane(int32_t pipe) const;          // the pool's buffers of one pipe slot
    const LanePtrs* DeviceLane();                    // device copy of HostLane(current pipe)
    void InvalidateDeviceLanes() { lanes_dirty_ = true; }
    void SetCurrentMode(int32_t mode) { mode_ = mode; }
    void SetIter(int32_t iter) { iter_ = iter; }

    // new in this build: sampler scratch (all device memory, private to the server)
    int32_t* slot_dst = nullptr;       // [max_slots] sampled neighbour per slot
    int32_t* slot_pos = nullptr;       // [max_slots] see LanePtrs
    int32_t* slot_fs = nullptr;        // [max_slots] / [num_ids]: feature-cache slots carried from the sampler to the gather
    int32_t* node_slot = nullptr;
    unsigned long long* tile_state = nullptr;   // [max_tiles / 4 + 1] (LanePtrs)
    RowHdr* fh_edge = nullptr;         // [num_ids] frontier row headers written by scatter
    int32_t* hop_scratch = nullptr;    // [HS_WORDS]
    unsigned long long* claim_pairs = nullptr; // see LanePtrs
    int32_t* run_off = nullptr;
    int32_t* claim_cnt = nullptr;
    int32_t claim_cap = 0;
    int32_t lds_bucket_bits = 0;
    int64_t last_hop_claims_hint = 0;  // PreSC's maximum of the last hop's edges (0: unknown), see lg_pool_alloc_private
    unsigned long long* known_pairs = nullptr;
    int32_t* known_cnt = nullptr;
    int32_t known_cap = 0;
    int32_t* err_host = nullptr;       // host-visible error word (mapped pinned), err_dev = its device address
    int32_t* err_dev = nullptr;
    int32_t ErrorBits() const { return err_host ? *(volatile int32_t*)err_host : 0; }
    void RaiseError(int32_t bits) { if (err_host) __atomic_fetch_or(err_host, bits, __ATOMIC_SEQ_CST); }
    // lanes of a GPURunner group or an arena pipeline (source.arena): the trainer-visible arrays live in the arena (not freed
    // here) and the counters are mirrored to host-visible memory by the end-of-batch kernel
    bool arena_backed = false;
    PoolSource source;                 // kept for the pool's later feature allocation
    PoolPrivatePlan private_plan;      // the private arrays' list (pool_plan.h) and, entry by entry, what lg_pool_alloc_private's walk of it took
    std::vector<void*> private_arrays;
    bool private_carved = false;       // ... from source.priv: Finalize frees none of them
    int32_t* counter_mirror_dev = nullptr;
    int32_t* counter_mirror_host = nullptr;
    int32_t num_ids = 0;
    int32_t max_slots = 0;             // largest hop = B * f1 * ... * fH
    std::vector<int64_t> max_new;      // [h] upper bound of new nodes of op 3h (h = 0: the seeds)
    int32_t total_num_nodes = 0;
    int32_t batch_size = 0;
    int32_t float_feature_len = 0;
    int64_t feature_rows = 0;
    // dtype of the rows gathered into the feature buffer (LEGION_FEATURE_*): bf16 = rows of D bf16 elements.  Fixed by the first
    // legion_pool_alloc_features (features_allocated); the buffer's element size follows it, its capacity in rows does not
    int32_t feature_out_dtype = LEGION_FEATURE_F32;
    bool features_allocated = false;
    // the sampler's modes (sample_mode.h), each fixed once the pool has sampled a hop, eagerly or into a captured graph (sample_used):
    // replace 0 takes distinct adjacency positions per frontier entry; edge_ids 1 also gives every sampled edge e agg_edge_ids[e] = its
    // position in the full CSR's column array, next to agg_src_ids[e] -- the two arrays below exist only then (lg_pool_alloc_edge_ids:
    // plain allocations of the pool, never part of a lane arena: the trainer-visible arrays and the wire do not change); weighted 1
    // picks position i of a row with probability w'[i] / row total, by an upper-bound search of the graph's per-row prefix-sum table
    // (GraphStorage::EdgeCdf, legion_graph_set_edge_weights) -- nothing is allocated in the pool: the table lives with the graph
    SampleMode mode;
    bool sample_used = false;
    int32_t max_fanout = 0;            // largest fan-out the pool was sized for
    int32_t* slot_pick = nullptr;      // [max_slots] see LanePtrs
    int64_t* agg_edge_ids = nullptr;   // [num_ids]
    int32_t lanes_epoch = 0;           // bumped when the pool's lane descriptor changes after creation (a lane group re-uploads its copy)
    int64_t grid_rows_hint = 0;        // > 0: rows a batch typically has (the Runner's pipe-slot pool holds the worst case: launches are sized for the usual one)
    int32_t dev_id = 0;
    bool owns_buffers = false;

    // graph replay: {next iteration, stride} on the device; when set, BatchGenerate reads the
    // iteration there and IOComplete advances it (no per-replay kernel-argument update)
    int32_t* iter_state = nullptr;

    // optional per-op timing with HIP events on the op's own stream (bench.py roofline leg)
    std::vector<hipEvent_t> prof_events;   // pairs: [2*i] before, [2*i+1] after
    std::vector<int32_t> prof_op;          // op id of each pair
    int32_t prof_used = 0;
    bool prof_on = false;

    void Finalize();

private:
    int32_t iter_ = 0;
    int32_t mode_ = 0;
    int32_t* cache_search_buffer_ = nullptr;
    int32_t* agg_src_ids_ = nullptr;
    int32_t* agg_dst_ids_ = nullptr;
    char* tmp_part_ind_ = nullptr;
    int32_t* tmp_part_off_ = nullptr;
    int32_t pipeline_depth_;
    int32_t current_pipe_ = 0;
    LanePtrs* d_lanes_ = nullptr;      // [pipeline_depth] device copies
    bool lanes_dirty_ = true;
    int64_t uploaded_rows_ = -1;
    std::vector<float*> float_features_;
    std::vector<int32_t*> labels_;
    std::vector<int32_t*> node_counter_;
    std::vector<int32_t*> edge_counter_;
    std::vector<int32_t*> sampled_ids_;
    std::vector<int32_t*> agg_src_off_;
    std::vector<int32_t*> agg_dst_off_;
};

// ---------------------------------------------------------------------------------------------
class GraphStorage {
public:
    virtual ~GraphStorage() = default;
    virtual void Build(BuildInfo* info) = 0;
    virtual void GraphCache(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) = 0;
    virtual void Finalize() = 0;
    virtual int32_t GetPartitionCount() const = 0;
    virtual int64_t** GetCSRNodeIndex(int32_t part_id) const = 0;
    virtual int32_t** GetCSRNodeMatrix(int32_t part_id) const = 0;
    virtual int64_t* GetCSRNodeIndexCPU() const = 0;
    virtual int32_t* GetCSRNodeMatrixCPU() const = 0;
    virtual int32_t NodeNum() const = 0;
    virtual int64_t EdgeNum() const = 0;
    virtual const RowHdr* GetRowHeaders(int32_t part_id) const = 0;   // new: [N] per GPU
    // Weighted sampling (new): edge_cdf, float32[E] indexed like the full column array -- per row the inclusive prefix sums of the
    // sanitised weights (finite and > 0, else 0), accumulated in double and rounded once (kernels_weights.hip).  One plain
    // allocation on the device current at the call, built on `s`; a second call replaces the contents.  -1 (nothing changes) for null
    // weights or once a weighted hop has been enqueued against this graph (MarkWeightedUsed: captured graphs hold the pointer and
    // batches in flight read it).
    virtual int32_t SetEdgeWeights(hipStream_t s, const float* w) = 0;
    virtual const float* EdgeCdf() const = 0;                         // null before SetEdgeWeights
    virtual void MarkWeightedUsed() = 0;
    // Sorted rows (new): are the column entries of every row of the full CSR non-decreasing as int32?  CheckRowsSorted counts on the
    // device current at the call (kernels_node2vec.hip), reads the answer back through `s` (set-up: it synchronises s) and remembers
    // it; RowsSorted: 1 / 0, or -1 before any check.  node2vec's membership test is a binary search of a row (legion_node2vec_walk).
    virtual int32_t CheckRowsSorted(hipStream_t s) = 0;
    virtual int32_t RowsSorted() const = 0;
    // The reverse CSR (new): the transpose of the full CSR (the rule: legion_graph_build_reverse in legion_hip.h), three plain
    // allocations on the device current at the first BuildReverse, which builds on `s` (set-up: it synchronises s) and returns 0; a
    // second call returns 0 without work.  ReverseCSR: the live entries E' and the arrays, or -1 and nulls before a build.
    virtual int32_t BuildReverse(hipStream_t s) = 0;
    virtual int64_t ReverseCSR(const int64_t** rindptr, const int32_t** rcol, const int64_t** reid) const = 0;
    // "Column slots" (new): a copy of the full column array in which every entry is the pair {neighbour id, feature-cache
    // slot of that neighbour = node_map[id]} (8 bytes).  The sampler's scattered 4-byte pick costs a whole 64-byte sector
    // either way; read as 8 bytes it brings the neighbour's cache slot along for free, and the gather no longer fetches a
    // 128-byte line of node_map per row (measured: 10 % of the hop-2 gather's traffic at D = 128, 19 % at D = 64).  Built per
    // GPU after FillUp from that GPU's node_map (which is what makes it clique-specific), only when the column array is
    // device memory and 8 bytes per edge are affordable (LegionTuning.col_slots); slots of cached-topology CSRs are not
    // paired: their picks carry LG_FS_UNKNOWN and the gather looks those rows up as before.
    virtual int32_t** GetCSRXMatrix(int32_t part_id) const = 0;       // device table [P+1] of pair arrays (null entries), or null
    virtual const int32_t* GetColumnSlotsFull(int32_t part_id) const = 0;   // that GPU's pair copy of the full column array, or null
    // The pairs are only as good as the node_map they were built from: they carry the stamp (cache uid, fill generation) of
    // that fill, and the sampler is given them only by a cache whose CURRENT fill has the same stamp (ColumnSlotsStamp) -- a
    // re-fill with other capacities, or another cache object over the same graph, samples from the plain column array and
    // the gather looks the slots up (a stale carried slot would address a wrong or out-of-range cache row).  Launch groups
    // captured into hipGraphs hold these pointers: destroy pipelines before re-filling a cache.
    virtual void BuildColumnSlots(int32_t dev, const int32_t* node_map, uint64_t stamp = 0) = 0;
    virtual void DropColumnSlots(int32_t dev) = 0;
    virtual uint64_t ColumnSlotsStamp(int32_t dev) const = 0;     // stamp of the fill the pairs belong to; 0: none built
    // GraphCache in two steps, so that a clique spread over processes can exchange the stripes in
    // between: build the cached CSR of every LOCAL member, then link every known member's CSR into the
    // local members' pointer tables and row headers.  SetPeerCSR registers a member owned by another
    // process (pointers opened from its IPC handles).
    virtual void GraphCacheBuildLocal(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) = 0;
    virtual void GraphCacheLink(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) = 0;
    virtual void SetPeerCSR(int32_t dev, int64_t* csr_node_index, int32_t* csr_dst_node_ids) = 0;
    virtual int64_t* CachedCSRIndex(int32_t dev) const = 0;
    virtual int32_t* CachedCSRDst(int32_t dev) const = 0;
};
extern "C" GraphStorage* NewCompleteGraphStorage();

class FeatureStorage {
public:
    virtual ~FeatureStorage() = default;
    virtual void Build(BuildInfo* info, int in_memory_mode) = 0;
    virtual void Finalize() = 0;
    virtual int32_t* GetTrainingSetIds(int32_t part_id) const = 0;
    virtual int32_t* GetValidationSetIds(int32_t part_id) const = 0;
    virtual int32_t* GetTestingSetIds(int32_t part_id) const = 0;
    virtual int32_t* GetTrainingLabels(int32_t part_id) const = 0;
    virtual int32_t* GetValidationLabels(int32_t part_id) const = 0;
    virtual int32_t* GetTestingLabels(int32_t part_id) const = 0;
    virtual int32_t TrainingSetSize(int32_t part_id) const = 0;
    virtual int32_t ValidationSetSize(int32_t part_id) const = 0;
    virtual int32_t TestingSetSize(int32_t part_id) const = 0;
    virtual int32_t TotalNodeNum() const = 0;
    virtual float* GetAllFloatFeature() const = 0;
    virtual int32_t GetFloatFeatureLen() const = 0;
    // row format of the table (LEGION_FEATURE_F32 | LEGION_FEATURE_BF16, legion_hip.h): with bf16 GetAllFloatFeature() is the
    // address of N rows of lg_feature_pitch() bf16 elements, not floats.  Every tier built from the storage keeps its format.
    virtual int32_t FeatureDtype() const { return LEGION_FEATURE_F32; }
    // SSD tier: unreleased in the reference (feature_storage.cu:146-154 are TODO stubs); kept as no-ops
    virtual void IOSubmit(int32_t*, int32_t*, int32_t*, float*, int32_t, int32_t, hipStream_t) {}
    virtual void IOComplete() {}
    // plain-buffer set-up used by the C API
    virtual void SetIds(int32_t dev_id, int32_t mode, const int32_t* host_ids,
                        const int32_t* host_labels, int32_t count) = 0;
};
extern "C" FeatureStorage* NewCompleteFeatureStorage();

// ---------------------------------------------------------------------------------------------
class CacheController {  // SS/cache/cache.cuh:10-62, the cache-policy plug-in point
public:
    virtual ~CacheController() = default;
    virtual void Initialize(int32_t dev_id, int32_t total_num_nodes) = 0;
    virtual void Finalize() = 0;
    virtual void FindFeat(int32_t* sampled_ids, int32_t* cache_offset, int32_t* node_counter,
                          int32_t op_id, void* stream) = 0;
    virtual void FindTopo(int32_t* input_ids, char* partition_index, int32_t* partition_offset,
                          int32_t batch_size, int32_t op_id, void* strm_hdl, int32_t device_id) = 0;
    virtual void CacheProfiling(int32_t* sampled_ids, int32_t* agg_src_id, int32_t* agg_dst_id,
                                int32_t* agg_src_off, int32_t* agg_dst_off, int32_t* node_counter,
                                int32_t* edge_counter, bool is_presc, void* stream) = 0;
    virtual void InitializeMap(int node_capacity, int edge_capacity) = 0;
    virtual void Insert(int32_t* QT, int32_t* QF, int32_t cache_expand, int32_t Kg) = 0;
    virtual void HybridInsert(int32_t* QF, int32_t cpu_cache_capacity, int32_t gpu_cache_capacity) = 0;
    virtual void AccessCount(int32_t* d_key, int32_t num_keys, void* stream) = 0;
    virtual unsigned long long int* GetNodeAccessedMap() = 0;
    virtual unsigned long long int* GetEdgeAccessedMap() = 0;
    virtual unsigned long long int* GetTopoTransactions() = 0;   // device counter, see sample_kernel
    virtual int32_t MaxIdNum() = 0;
    // direct-mapped id->value tables (the bcht::find contract), device pointers, may be null
    virtual const int32_t* NodeMap() const = 0;
    virtual const char* EdgeIndexMap() const = 0;
    virtual const int32_t* EdgeOffsetMap() const = 0;
};
CacheController* NewPreSCCacheController(int32_t train_step, int32_t device_count);

namespace lg { struct BulkLists; struct GatherParams; }

class UnifiedCache {
public:
    void Initialize(int64_t cache_memory, int32_t float_feature_len, int32_t train_step,
                    int32_t device_count, int32_t cpu_cache_capacity, int32_t gpu_cache_capacity);
    void InitializeCacheController(int32_t dev_id, int32_t total_num_nodes);
    void Finalize(int32_t dev_id);
    void FindFeat(int32_t* sampled_ids, int32_t* cache_offset, int32_t* node_counter, int32_t op_id,
                  void* stream, int32_t dev_id);
    void FindTopo(int32_t* input_ids, char* partition_index, int32_t* partition_offset,
                  int32_t batch_size, int32_t op_id, void* strm_hdl, int32_t dev_id);
    void CacheProfiling(int32_t* sampled_ids, int32_t* agg_src_id, int32_t* agg_dst_id,
                        int32_t* agg_src_off, int32_t* agg_dst_off, int32_t* node_counter,
                        int32_t* edge_counter, void* stream, int32_t dev_id);
    void CandidateSelection(int cache_agg_mode, FeatureStorage* feature, GraphStorage* graph);
    void CostModel(int cache_agg_mode, FeatureStorage* feature, GraphStorage* graph,
                   std::vector<uint64_t>& counters, int32_t train_step);
    void FillUp(int cache_agg_mode, FeatureStorage* feature, GraphStorage* graph);
    void FillUpLocal(FeatureStorage* feature, GraphStorage* graph);   // maps + the local members' stripes
    void FillUpLink(FeatureStorage* feature, GraphStorage* graph);    // pointer tables over every known member
    // The hybrid CPU-cache / GPU-cache tier (SS/cache/cache.cu:614-670; the reference's server.cu:112 keeps the call commented
    // out): per GPU, its OWN hotness order; the gpu_cache_capacity hottest rows in an HBM cache, the next cpu_cache_capacity
    // in a mapped pinned host cache, the rest misses.  Replaces CandidateSelection + CostModel + FillUp.  miss_from_table:
    // a miss row is read from the FeatureStorage table (this build's stand-in for the unreleased SSD reader); false = the
    // reference's kernel to the letter: the gather leaves a miss row unwritten.
    void HybridInit(FeatureStorage* feature, GraphStorage* graph, bool miss_from_table = true);
    void SetHybridCapacity(int32_t cpu_cache_capacity, int32_t gpu_cache_capacity)
    {
        cpu_cache_capacity_ = cpu_cache_capacity;
        gpu_cache_capacity_ = gpu_cache_capacity;
    }
    int32_t CPUCapacity() const { return cpu_cache_capacity_; }     // cache.cu:676-682
    int32_t GPUCapacity() const { return gpu_cache_capacity_; }
    bool IsHybrid() const { return hybrid_; }
    const float* HybridCPUCache(int32_t dev_id) const { return dev_id < (int32_t)cpu_cache_dev_.size() ? cpu_cache_dev_[dev_id] : nullptr; }
    void SetPeerFeatureCache(int32_t dev, float* ptr) { float_feature_cache_[dev] = ptr; }
    float* FeatureCachePtr(int32_t dev) const { return float_feature_cache_[dev]; }
    void SetPeerMaxIds(const int32_t* v, int32_t n) { peer_max_ids_.assign(v, v + n); }
    // Hot-row replica (new; MI355X has 288 GB per GPU): besides its stripe of the clique's cache every member keeps a
    // private copy of the clique's hottest rows, as many as `bytes` hold.  The lookup result (hit mask, global slot) is
    // unchanged -- only where a hit row is READ changes: ranks below the replica size come from local HBM instead of a
    // peer over xGMI.  Set before FillUp.
    void SetReplicaMemory(int64_t bytes) { replica_bytes_ = bytes; }
    int32_t ReplicaRows(int32_t dev_id) const { return replica_rows_.empty() ? 0 : replica_rows_[dev_id]; }
    int32_t FloatFeatureLen() const { return float_feature_len_; }
    // row format of every feature tier (stripes, replica, hybrid caches, the bound table): taken from the FeatureStorage the
    // tiers are built from (CostModel, FillUpLocal, HybridInit, BindFeatureTable).  Lanes and trainer rows stay float32.
    void AdoptFeatureFormat(const FeatureStorage* feature) { if (feature) feature_dtype_ = feature->FeatureDtype(); }
    int32_t FeatureDtype() const { return feature_dtype_; }
    int32_t RowPitch() const { return lg_feature_pitch(feature_dtype_, float_feature_len_); }       // elements per stored row
    int64_t RowBytes() const { return lg_feature_row_bytes(feature_dtype_, float_feature_len_); }
    bool gather_stats_on_ = true;        // GatherStats() arms the counters; SetGatherStats pauses them (a device word: graphs follow)
    void SetGatherStats(bool on);
    unsigned long long* GatherStats(int32_t dev_id);   // device {stripe rows, replica rows, peer-stripe rows}, allocated on first use
    int32_t MaxIdNum(int32_t dev_id);
    void LastHopMax(int32_t dev_id, int32_t out[2]);   // PreSC maxima {edges of the last hop, nodes before it}; {0, 0} before PreSC
    unsigned long long int* GetEdgeAccessedMap(int32_t dev_id);
    // the gather over a group of lanes (the reference's per-array arguments live in LanePtrs)
    struct GatherCall {
        int32_t op_id;
        int32_t first_op_id = -1;       // < op_id: one launch also covers the new-node ranges of the earlier ops first_op_id, +3, ...
        bool use_snapshot = true;       // the rows' range from the snapshot the op's producer left (false: from the live counters)
        bool last_op = true;            // the batch's last gather: what it leaves in cache_search_buffer is what the batch hands over
        bool skip_remote = false;       // peer_gather = bulk: rows of other members' stripes are the owners' to push
        int32_t max_rows = 0;           // rows the lanes' feature buffers hold
        int32_t grid_rows = 0;          // rows a lane typically has (sizes the grid); 0: max_rows
        int32_t out_dtype = LEGION_FEATURE_F32;
    };
    void FeatCacheLookup(const LanePtrs* d_lanes, int32_t n_lanes, int32_t dev_id, hipStream_t strm_hdl, const GatherCall& call);
    // peer_gather = bulk (lg::BulkLists): the requester's bucket pass over every row of its group's batches (whole: batch_whole_gather),
    // and the owner's push
    void BulkBucket(const LanePtrs* d_lanes, int32_t n_lanes, const BatchOp& whole, int32_t dev_id, hipStream_t s, int32_t max_rows,
                    const lg::BulkLists& lists, const char* arena_base);
    lg::GatherParams GatherParamsOf(int32_t dev_id, int32_t op_id, int32_t max_rows, bool use_snapshot, int32_t first_op_id, bool last_op);
    void BulkPush(int32_t owner_dev, hipStream_t s, const int32_t* fidx, const int64_t* dst, const unsigned long long* cnt,
                  int64_t cap, char* peer_arena);

    // new / exposed for the C API and the fused kernels
    void SetCapacity(int32_t node_capacity, int32_t edge_capacity);
    void BindFeatureTable(float* table, int32_t total_num_nodes) { cpu_float_features_ = table; total_num_nodes_ = total_num_nodes; }
    void BindFeatureTable(FeatureStorage* feature)
    {
        AdoptFeatureFormat(feature);
        BindFeatureTable(feature->GetAllFloatFeature(), feature->TotalNodeNum());
    }
    float* FeatureTable() const { return cpu_float_features_; }
    int32_t NodeCapacity(int32_t dev_id) const;
    int32_t EdgeCapacity(int32_t dev_id) const;
    CacheController* Controller(int32_t dev_id) const { return cache_controller_[dev_id]; }
    bool IsPresc() const { return is_presc_; }
    // (uid of this cache object, generation of its latest FillUpLocal): what column slots built from its node_map carry
    uint64_t FillStamp() const { return (uid_ << 24) | (fill_generation_ & 0xFFFFFFu); }
    bool world_reduced = false;   // hotness already all-reduced across processes (RCCL)
    // how the last CandidateSelection summed the counters of each clique: 0 nothing to sum / taken as they are, 1 the leader
    // loop over peer pointers, 2 RCCL all-reduce; and the milliseconds the RCCL calls took
    std::vector<int32_t> hotness_reduce_path_;
    double hotness_reduce_ms_ = 0;
    int32_t total_num_nodes_ = 0;
    int32_t Kc_ = 1, Kg_ = 1;
    int cache_agg_mode_ = 0;
    std::vector<int32_t*> QF_, QT_;
    std::vector<unsigned long long int*> AF_, AT_;
    float** Global_Float_Feature_Cache(int32_t dev_id) const { return d_float_feature_cache_ptr_[dev_id]; }

private:
    int32_t device_count_ = 0;
    std::vector<CacheController*> cache_controller_;
    std::vector<int32_t> node_capacity_, edge_capacity_;
    int32_t cpu_cache_capacity_ = 0, gpu_cache_capacity_ = 0;
    int64_t cache_memory_ = 0;
    std::vector<float*> float_feature_cache_;
    std::vector<float**> d_float_feature_cache_ptr_;
    int32_t float_feature_len_ = 0;
    int32_t feature_dtype_ = LEGION_FEATURE_F32;
    uint64_t uid_ = 0, fill_generation_ = 0;
    float* cpu_float_features_ = nullptr;
    bool is_presc_ = true;
    std::vector<int32_t> peer_max_ids_;   // MaxIdNum of every clique member when they live in other processes
    int64_t replica_bytes_ = 0;
    std::vector<float*> replica_;         // [device] hottest rows of its clique in rank order, or null
    std::vector<int32_t> replica_rows_;
    std::vector<unsigned long long*> gather_stats_;
    // hybrid tier: one CPU cache per GPU (the reference allocates a single one on device 0 although every GPU orders its rows
    // by its own counters, cache.cu:616,630-641 -- "single gpu version", :681)
    bool hybrid_ = false, hybrid_miss_from_table_ = true;
    std::vector<float*> cpu_cache_dev_, cpu_cache_host_;   // device-side / host-side address of each GPU's mapped pinned cache
    float* hybrid_table_ = nullptr;                        // the FeatureStorage table misses are served from
};

// ---------------------------------------------------------------------------------------------
class IPCEnv {  // SS/engine/ipc_service.h:6-33
public:
    virtual ~IPCEnv() = default;
    // dtype of the rows handed to the trainers (LEGION_FEATURE_*): sizes the pipe-slot feature buffers and is published to the
    // trainer end (set before InitializeFeaturesBuffer)
    int32_t feature_out_dtype = LEGION_FEATURE_F32;
    virtual void Coordinate(BuildInfo* info) = 0;
    virtual int32_t GetMaxStep() = 0;
    virtual void InitializeSamplesBuffer(int32_t batch_size, int32_t num_ids, int32_t feature_dim,
                                         int32_t device_id, int32_t pipeline_depth) = 0;
    virtual void InitializeFeaturesBuffer(int32_t batch_size, int32_t num_ids, int32_t feature_dim,
                                          int32_t device_id, int32_t pipeline_depth) = 0;
    virtual int32_t GetRawBatchsize() = 0;
    virtual int32_t GetLocalBatchId(int32_t global_batch_id) = 0;
    virtual int32_t GetCurrentBatchsize(int32_t dev_id, int32_t current_mode) = 0;
    virtual int32_t GetCurrentMode(int32_t global_batch_id) = 0;
    virtual int32_t* GetIds(int32_t dev_id, int32_t current_pipe) = 0;
    virtual float* GetFloatFeatures(int32_t dev_id, int32_t current_pipe) = 0;
    virtual int32_t* GetLabels(int32_t dev_id, int32_t current_pipe) = 0;
    virtual int32_t* GetAggSrc(int32_t dev_id, int32_t current_pipe) = 0;
    virtual int32_t* GetAggDst(int32_t dev_id, int32_t current_pipe) = 0;
    virtual int32_t* GetNodeCounter(int32_t dev_id, int32_t current_pipe) = 0;
    virtual int32_t* GetEdgeCounter(int32_t dev_id, int32_t current_pipe) = 0;
    virtual void IPCPost(int32_t dev_id, int32_t current_pipe) = 0;
    virtual void IPCWait(int32_t dev_id, int32_t current_pipe) = 0;
    // new in this build (see ipc_env.hip): host-visible per-slot counter mirror written by the GPU, non-blocking wait
    virtual int32_t* GetCounterMirror(int32_t dev_id, int32_t current_pipe) = 0;
    virtual void PublishMirror() = 0;
    virtual bool IPCTryWait(int32_t dev_id, int32_t current_pipe) = 0;
    // direct-view hand-over (round 4, ipc_env.hip shmExt): the lane arena's IPC handle, whether the trainer end of dev_id
    // takes views of it, and the per-slot description of the batch being posted
    virtual int32_t* HostCounterMirror(int32_t dev_id, int32_t current_pipe) = 0;
    virtual bool PublishArena(int32_t dev_id, void* base, int64_t bytes) = 0;
    virtual bool TrainerTakesViews(int32_t dev_id) = 0;
    virtual void SetView(int32_t dev_id, int32_t pipe, const int64_t* off5, const int32_t* counters32) = 0;
    virtual void AbortServing() = 0;
    virtual void Finalize() = 0;
    virtual int32_t GetTrainStep() = 0;
};
IPCEnv* NewIPCEnvImpl(int32_t device_count, bool create_shm);

// ---------------------------------------------------------------------------------------------
struct OpParams {  // SS/engine/operator.h:4-17
    int device_id;
    hipStream_t stream;
    hipEvent_t event;
    void* memorypool;
    void* cache;
    void* graph;
    void* feature;
    void* env;
    int neighbor_count;
    bool is_presc;
    bool in_memory;
    int hop_num;
};

class Operator {
public:
    virtual ~Operator() = default;
    virtual void run(OpParams* params) = 0;
};
Operator* NewBatchGenerateOP(int op_id);
Operator* NewRandomSampleOP(int op_id);
Operator* NewCacheLookupOP(int op_id);
Operator* NewSSDIOSubmitOP(int op_id);
Operator* NewSSDIOCompleteOP(int op_id);

struct RunnerParams {  // SS/engine/server.h:5-14
    int device_id;
    std::vector<int> fanout;
    void* cache;
    void* graph;
    void* feature;
    void* env;
    int global_batch_id;
    bool in_memory;
};

class Server {
public:
    virtual ~Server() = default;
    virtual void Initialize(int global_shard_count, std::vector<int> fanout, int in_memory_mode) = 0;
    virtual void PreSc(int cache_agg_mode) = 0;
    virtual void Run() = 0;
    virtual void Finalize() = 0;
};

class Runner {
public:
    virtual ~Runner() = default;
    virtual void Initialize(RunnerParams* params) = 0;
    virtual void InitializeFeaturesBuffer(RunnerParams* params) = 0;
    virtual void RunPreSc(RunnerParams* params) = 0;
    virtual void RunOnce(RunnerParams* params) = 0;
    virtual void Finalize(RunnerParams* params) = 0;
    virtual void PrepareServing(RunnerParams*) {}   // new: allocations / graph capture of the serving phase, before "ready"
};
Runner* NewGPURunner();

// one process per GPU with a clique spread over processes: only device `dev` is owned by this process
extern "C" void legion_set_local_device(int32_t dev);
bool lg_is_local(int32_t dev);

void lg_pool_alloc_private(MemoryPool* mp, int32_t dev_id, int32_t total_num_nodes, int32_t batch_size,
                           const int32_t* fanout, int32_t hop_num, int32_t float_feature_len, const PoolSource& source = PoolSource());
// legion_pool_create with a source (the extern "C" function passes an empty one)
MemoryPool* lg_pool_create(int32_t dev_id, int32_t total_num_nodes, int32_t batch_size, const int32_t* fanout, int32_t hop_num,
                           int32_t float_feature_len, int32_t pipeline_depth, const PoolSource& source);
// the private plan of a pool of this shape under the tuning as it stands (what lg_pool_alloc_private walks)
PoolPrivatePlan lg_pool_private_plan(const PoolShape& shape, const PoolSource& source);
// the two arrays of the edge-id mode (MemoryPool::mode.edge_ids), part of the pool's private allocation: made when the mode is turned on
void lg_pool_alloc_edge_ids(MemoryPool* mp);
// the one way a pool's mode changes (the three legion_pool_set_* of storage.hip, and legion_pipeline_set_* for every lane): refused
// once the pool has sampled and for what sample_mode_refusal names; check_only: answer, change nothing
bool lg_pool_try_set_mode(MemoryPool* mp, const SampleMode& mode, bool check_only = false);
// alloc helpers, SS/engine/server_imp.cuh:2-51
extern "C" void* d_alloc_space(int64_t num_bytes);
extern "C" void d_free_space(void* d_ptr);
extern "C" void* host_alloc_space(int64_t num_bytes);
extern "C" void SetGPUDevice(int32_t shard_id);
extern "C" int32_t GetGPUDevice();
// hipIpcGetMemHandle with a few retries: on this pool's driver (dmabuf IPC) an export now and then fails with
// 'invalid argument' for a fresh, valid allocation and succeeds a moment later; a persistent failure is fatal as before
void lg_ipc_export(void* handle64, void* dev_ptr, const char* file, int line);
void* lg_alloc_exported(int64_t num_bytes, void* handle64, const char* file, int line);   // fresh buffer + its handle; tries other blocks

// ---- extern "C" functions one source file of the library calls in another and include/legion_hip.h does not list (the public ones
//      come from that header): declared once, here, so that the compiler checks every caller against the definition ---------------
// storage.hip: device memory built from shuffled physical chunks, and its hand-over to other GPUs and processes
extern "C" void* d_alloc_scattered(int64_t num_bytes, int32_t chunk_mb);
extern "C" void* d_alloc_scattered_exportable(int64_t num_bytes, int32_t chunk_mb);
extern "C" int64_t lg_scattered_info(void* ptr, int32_t* n_chunks);
extern "C" int32_t lg_scattered_grant(void* ptr, const int32_t* logical_devs, int32_t n);
extern "C" int32_t lg_scattered_serve(void* ptr, const char* name);
extern "C" int32_t lg_scattered_exportable(void* ptr);
extern "C" void* lg_scattered_map_remote(const char* name, int32_t n_chunks, int64_t chunk_bytes);
extern "C" void lg_scattered_unmap_remote(void* base);
extern "C" int lg_scattered_export_fd(void* ptr, int32_t index);
// operators.hip: lane groups
LegionLaneGroup* lg_group_create(LegionMemoryPool** pools, int32_t n, PrivateBlock* priv);      // legion_group_create with its lanes' copy carved from `priv`
extern "C" void legion_enqueue_group_phase(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                           LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t n_active,
                                           int32_t batch_size, int32_t counter0, int32_t dev_id, int32_t mode,
                                           const int32_t* fanout, int32_t hop_num, int32_t phase);
extern "C" const void* legion_group_lane_desc(LegionLaneGroup* g, int32_t lane);
extern "C" void legion_group_refresh(LegionLaneGroup* g);
extern "C" void legion_enqueue_group_last_gather(legion_stream_t strm_hdl, LegionUnifiedCache* cache, LegionLaneGroup* group,
                                                 int32_t n_active, int32_t dev_id, int32_t hop_num);
// pipeline.hip: what GPURunner needs beyond the public pipeline API
LegionPipeline* lg_pipeline_create(LegionGraphStorage* graph, LegionFeatureStorage* feature, LegionUnifiedCache* cache, int32_t dev_id,
                                   int32_t batch_size, const int32_t* fanout, int32_t hop_num, int32_t group_size, int32_t slots,
                                   int64_t feature_rows, int32_t use_graph, int32_t feature_out_dtype, PoolArena* caller_arena);
extern "C" int32_t legion_pipeline_submit_ex(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size);
extern "C" void legion_pipeline_prepare(LegionPipeline* p, int32_t mode, int32_t n_active, int32_t batch_size);
extern "C" legion_stream_t legion_pipeline_stream(LegionPipeline* p);
extern "C" void* legion_pipeline_slot_done_event(LegionPipeline* p, int32_t slot);
extern "C" void legion_pipeline_wait_sleeping(LegionPipeline* p, int32_t slot, int32_t spin_us);
extern "C" void legion_pipeline_set_gathers(LegionPipeline* p, int32_t on);
extern "C" int32_t legion_pipeline_bulk_enable_shared(LegionPipeline* p, const PoolArena* arena);
extern "C" int32_t legion_pipeline_submit_bulk_inproc(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size);

// ---------------------------------------------------------------------------------------------
// kernel launchers (kernels_*.hip)
namespace lg {

// the process-wide LegionTuning (include/legion_hip.h section 6, tuning.hip): launch paths read it here, nothing else
// parses LEGION_* tuning variables.  tuning_refresh() re-reads the environment (unless a host program installed its own
// values with legion_tuning_set); pools, pipelines and servers call it when they are created.
LegionTuning tuning();           // a snapshot by value (tuning.hip)
void tuning_refresh();

struct HopParams {                  // what every lane of a launch shares
    int32_t op_id;
    int32_t count;                  // fan-out of this hop
    int32_t partition_count;        // P: slot of the full CSR in the pointer tables
    int32_t* const* csr_dst_node_ids;   // device table [P+1] of column arrays
    int32_t* const* csr_dst_x;          // device table [P+1] of {id, feature-cache slot} pair arrays (column slots), or null
    const int32_t* col_full;            // the full CSR's column array and its pair copy BY VALUE: a pick from slot P (nearly all of
    const int32_t* colx_full;           // them) then needs no dependent load of a table entry before the column load itself
    const RowHdr* row_hdr;          // [N] per-vertex row headers of this GPU
    bool last_hop;                  // no next hop: scatter skips the header lookup
    bool is_presc;
    int32_t max_slots;              // capacity of slot_dst for this hop
    unsigned long long* edge_access_time;  // presample only (single lane), else null
    unsigned long long* topo_transactions; // presample only: 64-byte transactions the hop's topology reads amount to
    int32_t lds_k;                  // super tiles per partition tile in this hop (set by launch_random_sample)
    const int64_t* indptr_full;     // the full CSR's row pointers (slot P of the pointer tables): read by the edge-id and weighted instances only
    SampleMode mode;                // MemoryPool::mode: picks the sample / compact instances (launch_hop); no kernel reads it.  (It stands
                                    // between the two pointers only so that they are not adjacent, as they never were)
    const float* edge_cdf;          // GraphStorage::EdgeCdf(), indexed like col_full: the weighted instances, which also read indptr_full (cached rows)
};
// bucket_bits, last_hop_claims_hint: the pool's (MemoryPool); the launch follows sample_hop_plan (sample_plan.h)
void launch_random_sample(hipStream_t s, const HopParams& p, int32_t bucket_bits, int64_t last_hop_claims_hint, const LanePtrs* d_lanes,
                          int32_t n_lanes);

// hand-over of a lane's finished batch to a trainer-visible pipe slot (kernels_gather.hip)
struct DeliverParams {
    int32_t* sampled_ids; int32_t* labels; int32_t* agg_src_off; int32_t* agg_dst_off;   // the slot's buffers
    int32_t* node_counter; int32_t* edge_counter;
    int32_t* mirror;          // device address of the slot's host-visible counter mirror [32], or null
    int32_t num_ids;          // capacity of the id / edge arrays
    int32_t batch_cap;        // capacity of labels
};

struct GatherParams {
    const float* full_table;
    const float* replica;           // local copy of the clique's `replica_rows` hottest rows (hotness rank order), or null
    int32_t replica_rows;
    int32_t Kg;                     // GPUs per clique: rank t of a hit = (g % cap) * Kg + g / cap
    int32_t member;                 // this GPU's index inside its clique (dev_id % Kg)
    bool striped;                   // slots encode (owner, row) = (g / capacity, g % capacity); false: one table, row = g (no division)
    unsigned long long* stats;      // optional {rows read through a stripe pointer, rows from the local replica, rows from a PEER's stripe}
    const float* const* cache_tables;
    const float* local_table;       // this member's own stripe by value (cache_tables[member]): no dependent pointer load for local rows
    const int32_t* node_map;
    int32_t node_capacity;
    int32_t D;
    int32_t total_num_nodes;
    int32_t max_rows;               // rows any lane can have for this op: the kernel never gathers more (and the grid covers them, unless ...)
    int32_t grid_rows;              // ... > 0: the rows a lane TYPICALLY has: the grid is sized for these (the workgroups walk a lane's tiles, so a
                                    // lane with more rows -- up to max_rows -- is still gathered whole); 0: size the grid for max_rows
    int32_t hop;                    // >= 0: take the range from hop_scratch[HS_RANGE + 2*hop] (snapshot that later
                                    // hops do not overwrite, so the gather may run beside the next hop); < 0: node_counter[0..1]
    int32_t first_hop;              // with hop >= 0: also gather the ranges of hops first_hop .. hop-1 (they are adjacent in
                                    // sampled_ids); == hop for a plain single-op gather
    bool last_op;                   // the gather of the batch's last op (kernel instance of its own: hand-over, traces)
    bool skip_remote;               // peer_gather = bulk: rows of OTHER members' stripes are not fetched here (their owners push them)
    // hybrid CPU-cache / GPU-cache tier (feat_cache_lookup, SS/cache/cache_impl.cuh:202-235): slots [0, cpu_cap) are rows of
    // hybrid_cpu_cache (mapped pinned host memory), slots >= cpu_cap rows (g - cpu_cap) % gpu_cap of local_table; a miss reads
    // full_table when that is bound and is left unwritten otherwise
    bool hybrid;
    int32_t hybrid_cpu_cap, hybrid_gpu_cap;
    const float* hybrid_cpu_cache;
    // row format of every source above (LEGION_FEATURE_*): bf16 sources are rows of `pitch` bf16 elements (pitch = D rounded up
    // to 8, zero padded), read 16 bytes per lane and widened to the float32 output row (bits << 16, exact)
    int32_t dtype;
    int32_t pitch;
    // row format of the destination (LEGION_FEATURE_*, the pool's feature output dtype): bf16 output rows are D bf16 elements,
    // stride D, no pad -- bf16 sources copied verbatim, float32 ones rounded to nearest even
    int32_t out_dtype;
};

// Owner-bucketed bulk transfer of a striped gather (LegionTuning.peer_gather = bulk; SURVEY section 7 "hard parts", the
// alternative to 512-1024-byte direct loads over xGMI, SS/cache/cache_impl.cuh:268).  The REQUESTER lists, per owner, the rows
// of that owner's stripe its launch group needs and where they go: row index inside the stripe, byte offset of the destination
// row inside the requester's lane arena.  The OWNER then reads its own HBM and pushes whole rows to the requester with
// coalesced posted stores (bulk_push_kernel).  One list set per pipeline slot, in requester memory, exported to the owners.
struct BulkLists {
    int32_t Kg;
    int64_t cap;                     // entries per owner list
    int32_t* fidx;                   // [Kg][cap]
    int64_t* dst;                    // [Kg][cap]
    unsigned long long* cnt;         // [Kg] entries listed (never beyond cap: a group has at most cap rows)
};
void launch_bulk_bucket(hipStream_t s, const GatherParams& g, const LanePtrs* d_lanes, int32_t n_lanes, const BulkLists& lists,
                        const char* arena_base);
void launch_bulk_push(hipStream_t s, const float* stripe, int32_t D, const int32_t* fidx, const int64_t* dst,
                      const unsigned long long* cnt, int64_t cap, char* peer_arena);
void launch_gather(hipStream_t s, const GatherParams& g, const LanePtrs* d_lanes, int32_t n_lanes);
void launch_deliver(hipStream_t s, const LanePtrs* d_lane, const DeliverParams& d);
// the whole finished batch of a lane -- ids, feature rows, labels, both edge arrays, counters -- copied into a pipe slot
// stand-alone form for tests / probes: explicit arrays, one lane (node_slot, plan_out may be null); -1 = refused by the plan, nothing enqueued
int32_t launch_gather_explicit(hipStream_t s, const GatherParams& g, const int32_t* sampled_ids, const int32_t* node_slot,
                               int32_t* cache_index_out, const int32_t* range, void* dst, int32_t dst_rows, int32_t* plan_out);

struct SeedParams {
    int32_t batch_size;
    int32_t counter0;               // lane i takes iteration counter0 + i (or iter_state[0] + i)
    const int32_t* all_ids;
    const int32_t* all_labels;
    int32_t total_cap;
    int32_t hop_num;
    const int32_t* iter_state;      // device {next iteration, stride} or null
};
void launch_batch_generate(hipStream_t s, const SeedParams& p, const LanePtrs* d_lanes, int32_t n_lanes);

void launch_end_of_batch(hipStream_t s, const LanePtrs* d_lanes, int32_t n_lanes, int32_t* iter_state);
void launch_draw_batch(hipStream_t s, const int32_t* idx, const int32_t* deg, int32_t* out, int32_t n);
void launch_draw_distinct_batch(hipStream_t s, const int32_t* base, const int32_t* deg, int32_t f, int32_t* out, int32_t n);
// the weighted pick rule on its own (tests): out[i] = pick of slot idx[i] in the row {row_start[i], deg[i]} of cdf, or -1
void launch_draw_weighted_batch(hipStream_t s, const int32_t* idx, const int64_t* row_start, const int32_t* deg, const float* cdf,
                                int32_t* out, int32_t n);
// the per-row prefix-sum table of weighted sampling (kernels_weights.hip): cdf[E] from w[E] and the full CSR's indptr[n_rows + 1];
// long_rows: scratch of the build, int32[1 + long_cap] with long_cap = lg_weights_long_rows_cap(E) (a count, then the rows a whole
// workgroup scans)
int64_t lg_weights_long_rows_cap(int64_t num_edges);
void build_edge_cdf(hipStream_t s, const int64_t* indptr, int32_t n_rows, const float* w, float* cdf, int32_t* long_rows, int32_t long_cap);

// random walks over the full CSR (kernels_walk.hip; the rule: legion_random_walk in legion_hip.h)
struct WalkParams {
    const int64_t* indptr;          // the FULL CSR (slot P of the pointer tables), int64[node_num + 1]
    const int32_t* col;
    const float* edge_cdf;          // the graph's prefix table: a weighted walk; null: the uniform pick
    const int32_t* seeds;           // int32[num_walks]
    int32_t* traces;                // int32[num_walks x (length + 1)]
    int64_t* edge_ids;              // int64[num_walks x length], or null
    int32_t node_num;
    int32_t num_walks;
    int32_t length;
    float restart_prob;             // > 0: the instances with the restart draw
    int64_t base;                   // draw index of walk 0's first step
};
void launch_random_walk(hipStream_t s, const WalkParams& p);

// node2vec walks over the full CSR (kernels_node2vec.hip; the rule: legion_node2vec_walk in legion_hip.h)
struct Node2vecParams {
    WalkParams walk;                // as for launch_random_walk; restart_prob unused
    double a, b, mx;                // 1 / p, 1 / q and max(1 / p, 1, 1 / q) (node2vec_rule.h)
    double lo, hi;                  // min(1, 1 / q), max(1, 1 / q): the weights of a candidate u != t, whichever class the search finds
    int32_t max_tries;
};
void launch_node2vec_walk(hipStream_t s, const Node2vecParams& p);
// counts[0] += #{ e in [1, E) : col[e - 1] > col[e] }, counts[1] += the same inversions at e = indptr[v] of rows v with entries and
// e > 0: the rows are sorted iff the two agree (every inversion lies across a row boundary)
void launch_row_inversion_counts(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t n_rows, int64_t num_edges,
                                 unsigned long long* counts);

// the seeds of a link-prediction batch (kernels_link.hip; the rules: legion_find_edges, legion_negative_sample and legion_unique_ids in
// legion_hip.h).  The arguments are the caller's to check (link_rule.h).
void launch_find_edges(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t node_num, int64_t num_edges, const int64_t* eids,
                       int32_t n, int32_t* row_out, int32_t* col_out);
struct NegativeParams {
    const int64_t* indptr;          // the FULL CSR; read only with exclude & 2
    const int32_t* col;
    const int32_t* rows;            // int32[n]
    int32_t* neg;                   // int32[n x k]
    int32_t node_num;
    int32_t n, k;
    int32_t exclude;                // bit 0: the row itself, bit 1: the entries of its row
    int32_t max_tries;
    int64_t base;                   // draw index of slot 0
};
void launch_negative_sample(hipStream_t s, const NegativeParams& p);
// slots, n_tiles: unique_ids_table_slots(m), unique_ids_tiles(m); scratch: unique_ids_scratch_bytes(m) bytes, cleared here on s
void launch_unique_ids(hipStream_t s, const int32_t* ids, int32_t m, int32_t* unique, int32_t* local, int32_t* count, void* scratch,
                       int64_t slots, int64_t n_tiles);

// a neighbourhood taken whole (kernels_in_edges.hip; the rules: legion_row_offsets and legion_in_edges in legion_hip.h).  The arguments
// are the caller's to check (in_edges_rule.h).
// n_tiles: row_offsets_tiles(n); scratch: row_offsets_scratch_bytes(n) bytes, 8-byte aligned
void launch_row_offsets(hipStream_t s, const int64_t* indptr, int32_t node_num, const int32_t* rows, int32_t n, int64_t* offsets,
                        void* scratch, int64_t n_tiles);
// values[0 .. n) become their exclusive prefix sums, total[0] and (unless null) total2[0] their sum, in three launches: the sum per 256
// values to sums[0 .. n_sums), n_sums = ceil(n / 256) <= 4 096 (summed: the caller's own launch has written them), ONE workgroup's
// scan of the sums, the in-256 scan plus its base.  n == 0: the second launch alone, the totals 0
void launch_scan_int64(hipStream_t s, int64_t* values, int32_t n, int64_t* sums, int32_t n_sums, bool summed, int64_t* total, int64_t* total2);
// the rows whose entries are spread over slots, and the slots (row_slots.h)
struct RowSlots {
    const int64_t* indptr;          // the FULL CSR
    const int32_t* col;
    const int32_t* rows;            // int32[n]
    const int64_t* offsets;         // int64[n + 1]: whatever they hold, nothing is read outside them, rows, indptr and col
    int32_t node_num;
    int32_t n;
    int64_t m;                      // slots to look at
};
struct InEdgesParams {
    RowSlots slots;                 // m: slots to write, <= 2^31 - 1
    int32_t* dst;                   // int32[m]
    int32_t* src;                   // int32[m]
    int64_t* eid;                   // int64[m], or null
};
void launch_in_edges(hipStream_t s, const InEdgesParams& p);

// the reverse CSR (kernels_reverse.hip; the rule: legion_graph_build_reverse in legion_hip.h, its classes and refusals reverse_rule.h).
// The arguments are the caller's to check.  Builds on s and synchronises it; returns the live entries E' and three allocations of
// d_alloc_space on the current device: rindptr int64[node_num + 1], rcol int32[E'], reid int64[E'].  Its temporaries are freed
int64_t build_reverse_csr(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t node_num, int64_t num_edges, int64_t** rindptr_out,
                          int32_t** rcol_out, int64_t** reid_out);

// the slots of a row expansion that a predicate keeps, compacted in order (kept_slots.h): what the count and the write pass of
// LABOR and of induced subgraphs take beside their RowSlots
struct KeptParams {
    int64_t* tiles;                 // the scratch: int64[n_tiles + 1 + n_groups]: the tiles' kept counts, then their exclusive prefix sums
                                    // with the total K at [n_tiles]; behind it the sums per 256 tiles
    int64_t* count;                 // int64[1] (the count pass)
    int32_t* dst;                   // int32[cap] (the write pass, as src and eid)
    int32_t* src;                   // int32[cap]
    int64_t* eid;                   // int64[cap], or null
    int64_t n_tiles, n_groups;      // kept_tiles(m), kept_groups(m) (kept_rule.h)
    int64_t cap;                    // entries of dst, src and eid, <= 2^31 - 1
};

// layer-neighbour sampling, LABOR-0 (kernels_labor.hip; the rule: legion_labor_count and legion_labor_edges in legion_hip.h, its text
// labor_rule.h).  The arguments are the caller's to check (labor_rule.h).
struct LaborParams {
    RowSlots slots;                 // m <= 2^30
    KeptParams kept;
    int32_t fanout;                 // >= 1
    uint64_t key;                   // labor_key(salt)
};
void launch_labor_count(hipStream_t s, const LaborParams& p);
void launch_labor_edges(hipStream_t s, const LaborParams& p);

// the open-addressing table of ids of unique_ids and of a vertex set (id_table_rule.h; carved and claimed in node_set.h)
struct IdTable {
    int32_t* keys;                  // int32[S]: an empty key is all-ones
    uint32_t* first;                // uint32[S]: the least index whose id claimed the slot, all-ones: none
    uint32_t mask;                  // S - 1
    int32_t shift;                  // 32 - log2 S
};

// a vertex set and induced subgraphs (kernels_induced.hip; the rules: legion_node_set_build .. legion_dst_offsets in legion_hip.h, their
// text induced_rule.h).  The arguments are the caller's to check (induced_rule.h).
struct NodeSetView {
    const int32_t* keys;            // int32[S]: an empty key is all-ones
    const uint32_t* first;          // uint32[S]: the first position of the slot's key in the nodes
    uint32_t mask;                  // S - 1
    int32_t shift;                  // 32 - log2 S
    int32_t k;                      // the nodes the set was built from: a position is accepted inside [0, k)
    int32_t wide;                   // keys starts at a 16-byte boundary: a probe step loads four keys at once (node_set.h)
};
// set: node_set_bytes(k) bytes, cleared here on s; distinct: int32[1]
void launch_node_set_build(hipStream_t s, const int32_t* nodes, int32_t k, void* set, int32_t* distinct);
void launch_node_set_lookup(hipStream_t s, const NodeSetView& set, const int32_t* ids, int64_t m, int32_t* local);
struct InducedParams {
    RowSlots slots;                 // m <= 2^30
    NodeSetView set;                // (between the two, where it stood: induced_count_kernel spills 29 SGPRs so, 34 with set first)
    KeptParams kept;                // src: positions in the set
};
void launch_induced_count(hipStream_t s, const InducedParams& p);
void launch_induced_edges(hipStream_t s, const InducedParams& p);
// indptr[i] = #{ p in [0, L) : dst[p] < i } for i in [0, n], L = count[0] clamped to [0, cap]
void launch_dst_offsets(hipStream_t s, const int32_t* dst, int64_t cap, const int64_t* count, int32_t n, int64_t* indptr);

// seed-edge exclusion (kernels_exclude.hip; the rules: legion_reverse_edge_ids .. legion_edge_filter_edges in legion_hip.h, their text
// exclude_rule.h).  The arguments are the caller's to check (exclude_rule.h).
struct ReverseIdsParams {
    const int64_t* indptr;          // the FULL CSR: row(e) and col[e] come from it
    const int32_t* col;
    const int64_t* t_indptr;        // the CSR whose rows are searched: the graph's own (via 0) or the reverse CSR (via 1)
    const int32_t* t_col;
    const int64_t* t_eid;           // reid of the reverse CSR (via 1); via 0: a position in t_col is the edge id
    const int64_t* eids;            // int64[n]
    int64_t* out;                   // int64[n]
    int64_t num_edges;
    int64_t n;                      // <= 2^31 - 1
    int32_t node_num;
    int32_t via;                    // 0, 1
};
void launch_reverse_edge_ids(hipStream_t s, const ReverseIdsParams& p);
// a set of edge ids in the caller's memory: int64 keys[S], an empty key all-ones
struct EdgeSetView {
    const int64_t* keys;
    uint64_t mask;                  // S - 1
    int32_t shift;                  // 64 - log2 S
};
// set: edge_set_bytes(k) bytes, cleared here on s
void launch_edge_set_build(hipStream_t s, const int64_t* eids, int32_t k, void* set);
void launch_edge_set_contains(hipStream_t s, const EdgeSetView& set, const int64_t* eids, int64_t m, int32_t* out);
struct EdgeFilterParams {
    const int32_t* dst;             // int32[m]: the list to filter
    const int32_t* src;             // int32[m]
    const int64_t* eid;             // int64[m]
    int64_t m;                      // <= 2^30
    EdgeSetView set;
    KeptParams kept;
};
void launch_edge_filter_count(hipStream_t s, const EdgeFilterParams& p);
void launch_edge_filter_edges(hipStream_t s, const EdgeFilterParams& p);

// the k best entries of each row (kernels_topk.hip; the rule: legion_row_topk and legion_topk_keys in legion_hip.h, its text
// topk_rule.h).  The arguments are the caller's to check (topk_rule.h).
struct TopkParams {
    const int64_t* indptr;          // the FULL CSR
    const int32_t* col;
    const float* w;                 // float32[E], or null (SAMPLE: every weight 1)
    const int32_t* rows;            // int32[n]
    int32_t* src;                   // int32[n x k]
    int64_t* eid;                   // int64[n x k], or null
    int32_t* count;                 // int32[n], or null
    int32_t* long_rows;             // the scratch: int32[n + 1]: how many rows were listed, then their positions in rows
    int32_t node_num;
    int32_t n;
    int32_t k;                      // 1 .. 64
    int32_t mode;                   // LEGION_TOPK_*
    uint64_t key;                   // labor_key(salt)
};
void launch_row_topk(hipStream_t s, const TopkParams& p);
void launch_topk_keys(hipStream_t s, const int32_t* col, int64_t num_edges, const float* w, const int64_t* eids, int64_t n, int32_t mode,
                      uint64_t key, uint64_t* key_out, uint8_t* eligible_out);

// PinSAGE's neighbour sampler (kernels_pinsage.hip; the rule: legion_pinsage_neighbors in legion_hip.h)
struct PinsageParams {
    WalkParams walk;                // indptr, col, edge_cdf, node_num, base; seeds = the n seeds; length = T; restart_prob = the
                                    // termination probability; num_walks = n (one row of results per seed); traces, edge_ids unused
    int32_t walks_per_seed;         // R
    int32_t num_neighbors;          // k
    int32_t* neighbors;             // int32[n x k]
    int32_t* counts;                // int32[n x k]
};
void launch_pinsage_neighbors(hipStream_t s, const PinsageParams& p);

// a roctx range for the enclosing scope (markers.hip): visible to rocprofv3 --marker-trace, near-free otherwise
struct Range {
    explicit Range(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
    ~Range();
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
private:
    bool on_;
};

// the hotness all-reduce (collective.hip): RCCL over the members of a clique that live in this process
bool clique_is_physical(const std::vector<int32_t>& devs);
double allreduce_u64_clique(const std::vector<int32_t>& devs, const std::vector<unsigned long long*>& send,
                            const std::vector<unsigned long long*>& recv, int64_t count);

// set-up kernels (kernels_cache.hip)
void launch_hotness_measure(hipStream_t s, const int32_t* sampled_ids, const int32_t* node_counter,
                            unsigned long long* access_map);
void init_row_headers(hipStream_t s, RowHdr* hdr, const int64_t* csr_index, int32_t n, int32_t slot);
void cache_row_headers(hipStream_t s, RowHdr* hdr, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity,
                       int32_t n, const int64_t* d_index, int32_t slot);
void launch_find(hipStream_t s, const int32_t* keys, int32_t n, const int32_t* map32,
                 const char* map8, int32_t* out32, char* out8);
void aggregate_access(hipStream_t s, unsigned long long* agg, const unsigned long long* add, int32_t n);
void sort_hotness_desc(hipStream_t s, unsigned long long* keys_inout, int32_t* order_out, int32_t n);
void inclusive_scan_u64(hipStream_t s, const unsigned long long* in, unsigned long long* out, int32_t n);
void edge_mem_in_order(hipStream_t s, const int32_t* order, unsigned long long* edge_mem, int32_t n,
                       const int64_t* csr_index);
void init_node_map(hipStream_t s, int32_t* node_map, const int32_t* QF, int32_t capacity, int32_t Kg,
                   int32_t n);
void init_node_map_hybrid(hipStream_t s, int32_t* node_map, const int32_t* QF, int32_t cpu_cache_capacity,
                          int32_t gpu_cache_capacity, int32_t n);
void init_edge_maps(hipStream_t s, char* index_map, int32_t* offset_map, const int32_t* QT,
                    int32_t capacity, int32_t Kg, int32_t Ki, int32_t n);
void fill_value_i32(hipStream_t s, int32_t* p, int32_t v, int64_t n);
void build_column_slots(hipStream_t s, const int32_t* col, const int32_t* node_map, int32_t* colx_pairs, int64_t num_edges);
void fill_value_i8(hipStream_t s, char* p, char v, int64_t n);
void feat_fill_up(hipStream_t s, int32_t capacity, int32_t D, float* cache, const float* table,
                  const int32_t* QF, int32_t Kg, int32_t Ki, int32_t n);
// the same fill for bf16 rows of `pitch` elements (pitch % 8 == 0: whole 16-byte chunks, padding included)
void feat_fill_up_bf16(hipStream_t s, int32_t capacity, int32_t pitch, uint16_t* cache, const uint16_t* table,
                       const int32_t* QF, int32_t Kg, int32_t Ki, int32_t n);
// f32[rows x D] -> bf16[rows x pitch], round to nearest even, NaN kept a NaN, pad elements zero.  Both sides device-accessible
// (HBM or mapped pinned host memory).
void convert_f32_to_bf16(hipStream_t s, const float* src, int64_t rows, int32_t D, int32_t pitch, uint16_t* dst);
void topo_neighbor_count(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity,
                         int32_t n, const int64_t* csr_index, int64_t* counts);
void inclusive_scan_i64(hipStream_t s, const int64_t* in, int64_t* out, int32_t n);
void topo_fill_up(hipStream_t s, const int32_t* QT, int32_t Kg, int32_t Ki, int32_t capacity, int32_t n,
                  const int64_t* csr_index, const int32_t* csr_dst, const int64_t* d_index,
                  int32_t* d_dst);
}  // namespace lg
