/*
 * legion_hip.h -- C ABI of liblegion_hip.so, the MI355X-native (gfx950) drop-in for the hot path
 * of RC4ML/Legion's sampling server: seed batch -> multi-hop CSR neighbour sampling -> node
 * de-duplication -> feature-cache lookup + gather, plus the one-time hotness -> cache-partition ->
 * fill set-up that feeds it.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * repository; SS = sampling_server/src).  Signatures carry plain pointers and sizes only: no
 * torch types, no C++ types.  Object arguments are opaque handles to the library's own
 * GraphStorage / FeatureStorage / UnifiedCache / MemoryPool / IPCEnv objects (the reference passes
 * pointers to its C++ classes of the same names through the same positions).
 *
 * Error convention (SS/engine/operator_impl.cu:16-24,141-148): functions return void; a null
 * object prints a message and returns; any HIP error prints "HIP failure file:line: 'msg'" and
 * exits the process.  There is NO CPU fallback anywhere in this library.
 */
#ifndef LEGION_HIP_H
#define LEGION_HIP_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SS/include/system_config.cuh:47-57 -- part of the wire contract */
#define LEGION_INTERBATCH_CON 2
#define LEGION_INTRABATCH_CON 3
#define LEGION_MAX_DEVICE 8
#define LEGION_MEMORY_USAGE 7
#define LEGION_TRAINMODE 0
#define LEGION_VALIDMODE 1
#define LEGION_TESTMODE 2
#define LEGION_CACHEMISS_FLAG (-2)

/* Feature dtype: the row format of a feature table and of every cache tier built from it.  float32 is the default;
 * bfloat16 rows hold round_up(D, 8) elements (16-byte aligned rows, zero padded), 2 bytes each, rounded to nearest
 * even from float32.  Whatever the storage, rows reach the lanes and the trainer as float32 (bf16 -> f32 is exact).
 * Values other than these are refused (room is left for further formats). */
#define LEGION_FEATURE_F32 0
#define LEGION_FEATURE_BF16 1

typedef void* legion_stream_t;            /* hipStream_t in the position of cudaStream_t */
typedef struct LegionGraphStorage   LegionGraphStorage;    /* SS/storage/graph_storage.cuh:7-24  */
typedef struct LegionFeatureStorage LegionFeatureStorage;  /* SS/storage/feature_storage.cuh:6-34 */
typedef struct LegionUnifiedCache   LegionUnifiedCache;    /* SS/cache/cache.cuh:66-177 */
typedef struct LegionMemoryPool     LegionMemoryPool;      /* SS/engine/memorypool.cuh:20-221 */
typedef struct LegionIPCEnv         LegionIPCEnv;          /* SS/engine/ipc_service.h:6-33 */
typedef struct LegionServer         LegionServer;          /* SS/engine/server.h:16-23 */

/* =====================================================================================
 * 1. The five operator entry points -- SS/engine/operator_impl.cuh:11-63, same names, same
 *    argument order and meaning.  All work is enqueued on `strm_hdl`; nothing synchronises
 *    with the host (the reference's blocking 64-byte counter read-backs are gone: frontier and
 *    node counts stay on the device and every kernel reads them there).
 * ===================================================================================== */
void BatchGenerate(legion_stream_t strm_hdl, LegionFeatureStorage* feature, LegionUnifiedCache* cache,
                   LegionMemoryPool* memorypool, int32_t batch_size, int32_t counter, int32_t part_id,
                   int32_t dev_id, int32_t mode, bool is_presc, int32_t hop_num);
void RandomSample(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionUnifiedCache* cache,
                  LegionMemoryPool* memorypool, int32_t count, int32_t dev_id, int32_t op_id,
                  bool is_presc);
void FeatureCacheLookup(legion_stream_t strm_hdl, LegionUnifiedCache* cache, LegionMemoryPool* memorypool,
                        int32_t op_id, int32_t dev_id);
void IOSubmit(legion_stream_t strm_hdl, LegionFeatureStorage* feature, LegionMemoryPool* memorypool,
              int32_t op_id, int32_t dev_id);
void IOComplete(legion_stream_t strm_hdl, LegionUnifiedCache* cache, LegionMemoryPool* memorypool,
                int32_t dev_id, int32_t mode);

/* One whole mini-batch in the op order of GPURunner::RunOnce / RunPreSc (SS/engine/server.cu:285-332)
 * without the IPC hand-off.  In PreSC mode only ops 0,3,6,...,last run (server.cu:290). */
void legion_enqueue_batch(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                          LegionUnifiedCache* cache, LegionMemoryPool* memorypool, int32_t batch_size,
                          int32_t counter, int32_t dev_id, int32_t mode, bool is_presc,
                          const int32_t* fanout, int32_t hop_num);

/* =====================================================================================
 * 2. Object construction from plain buffers (replaces StorageManagement::Initialze's wiring,
 *    SS/storage/storage_management.cu:234-269, for callers that already hold the arrays).
 *    "devptr" = a pointer the GPU can dereference: HBM (hipMalloc / a torch CUDA tensor) or
 *    mapped pinned host memory.  On MI355X the full CSR and, when it fits, the full feature
 *    table live in HBM; the pinned-host tier is the spill-over.
 * ===================================================================================== */

/* GraphStorage: SS/storage/graph_storage.cu:12-73.  Slot `partition_count` of the pointer
 * tables is the full CSR (int64 indptr[N+1], int32 col[E]). */
LegionGraphStorage* legion_graph_create(int32_t partition_count, int32_t node_num, int64_t edge_num,
                                        const int64_t* csr_node_index_devptr,
                                        const int32_t* csr_dst_node_ids_devptr);
void legion_graph_destroy(LegionGraphStorage* g);
/* New in this build ("column slots", LegionTuning.col_slots): after FillUp every GPU may hold a copy of the full column array
 * whose entries are {neighbour id, feature-cache slot of that neighbour} pairs.  The sampler's scattered pick reads the pair in
 * the one sector it fetches anyway, and the gather no longer looks the row's cache slot up (a 128-byte line per row for four
 * bytes: SS/cache/cache.cu:180-215 does it with a hash find per row).  Results are unchanged.  Returns 1 when GPU dev has it. */
int32_t legion_graph_column_slots(const LegionGraphStorage* g, int32_t dev);
/* The cached CSR logical GPU dev holds after a fill (GraphStorage::GraphCache, SS/storage/graph_storage.cu:76-111; kernels
 * SS/storage/graph_storage_impl.cuh:33-53): device pointers to int64 index[capacity + 1] and int32 dst[index[capacity]]; nulls before a
 * fill.  Introspection: tests/test_gpu_ref_graph_cache.py compares them with what the reference's own kernels produce (oracle/_ref). */
void legion_graph_cached_csr(const LegionGraphStorage* g, int32_t dev, const int64_t** index_out, const int32_t** dst_out);
/* Weighted neighbour sampling (DGL's NeighborSampler prob=), new in this build; with replacement only.
 * Weights: the caller's float32 w[E] on the device, aligned with the full CSR's column array.  The sanitised weight is
 *   w'[i] = w[i] if w[i] is finite and > 0, else 0        (negative values, NaN, +-inf and -0 count as 0).
 * Prefix table: edge_cdf, float32[E], indexed like the column array, a plain allocation of the library.  For row v with
 * s = indptr[v] and degree D:  edge_cdf[s + i] = (float)(sum_{j <= i} (double)w'[s + j]) -- accumulated in double, rounded once.  How
 * the sum is associated is not fixed; what holds is: non-decreasing inside a row; w'[s + i] == 0  =>  edge_cdf[s + i] ==
 * edge_cdf[s + i - 1] (== 0 at i = 0); |edge_cdf - exact| <= 2^-23 * exact (D < 2^29).  Where every partial sum is exactly
 * representable in float32 the table is unique.  Row totals must stay below FLT_MAX.
 * Pick of slot idx = q * f + k, k < min(f, D), on a pool in weighted mode (legion_pool_set_sample_weighted):
 *   T = edge_cdf[s + D - 1];  D == 0 or T == 0: the slot has no edge, exactly like k >= deg (slot_dst = -1: no claim, no hotness, no id);
 *   else r = (double)(x - 1) / 2147483646.0 with x = minstd(idx + 1) (the r of the uniform draw), t = r * (double)T and
 *   pick = #{ i in [0, D) : (double)edge_cdf[s + i] <= t }   -- an upper-bound binary search, ceil(log2(D + 1)) dependent 4-byte loads.
 * t < T, so pick <= D - 1, and edge_cdf[s + pick] > t >= edge_cdf[s + pick - 1]: an entry of weight zero is never drawn.  s is always the
 * FULL CSR's indptr[v], also for a row whose columns are read from a cached topology (the fill copies rows in CSR order): only the
 * table lives with the full CSR.  With all weights 1.0f and D < 2^24 the pick is floor(r * D), the uniform draw: the batch is bit for
 * bit the unweighted one.  Every frontier entry still owns slots q*f .. q*f + f - 1 and yields min(f, D) edges, or 0 when T == 0: no
 * buffer size changes.  Not offered: weighted sampling without replacement; the server, the launcher and the wire (in-process and
 * pipeline only, like edge ids); a table per rank of a multi-process clique is untested.
 * legion_graph_set_edge_weights builds the table on the device current at the call, enqueued on `stream`; the caller's array may go
 * once the stream has completed, and a weighted hop on ANOTHER stream (a pipeline's) must not start before.  Calling it again
 * replaces the table.  Returns 0, or -1 for a null graph or null weights, or once a
 * weighted hop has been enqueued against this graph.  legion_graph_edge_cdf: the table, or null before that call (introspection). */
int32_t legion_graph_set_edge_weights(LegionGraphStorage* g, legion_stream_t stream, const float* w_devptr);
const float* legion_graph_edge_cdf(const LegionGraphStorage* g);
/* Are the rows of the full CSR sorted: col[e - 1] <= col[e], as int32, for every two adjacent entries of one row?  (Dead entries, -1,
 * then come first in their row; parallel edges are fine.)  One pass over the full CSR on the device current at the call, enqueued on
 * `stream`; the result is read back -- set-up: the call synchronises that stream -- and remembered in the graph, so a repeat call
 * returns it without work.  1: sorted, 0: not, -1: a null graph.  legion_node2vec_walk asks for a remembered 1. */
int32_t legion_graph_check_rows_sorted(LegionGraphStorage* g, legion_stream_t stream);
/* The reverse CSR (DGL's dgl.reverse; through it g.out_edges, g.out_degrees and g.successors), new in this build; no reference
 * counterpart.  A row of the library's CSR is the destination side of an edge and a column entry its source side, so every op reads a
 * vertex's in-edges; the reverse is a CSR of the same shape whose rows hold the out-edges, and every op works on it as it stands.
 * (Where an op below lists out-edges under "Not offered", with or without "there is no reverse CSR", it speaks of that call on the
 * graph it is given: the call on the reverse of the graph is the op over out-edges.)
 * The rule.  N = node_num, E the column entries.  A LIVE entry is an e with 0 <= col[e] < N; dead entries (-1) and entries outside the
 * graph are dropped, as everywhere else.  row(e) is the one v with indptr[v] <= e < indptr[v + 1] (-1 where an indptr that does not
 * run from 0 to E leaves none).
 *   rindptr int64[N + 1]:  rindptr[u] = #{ live e : col[e] < u };  rindptr[N] = E', the number of live entries;
 *   reid    int64[E']:     the live e with col[e] == u, ASCENDING, at rindptr[u] <= p < rindptr[u + 1];
 *   rcol    int32[E']:     rcol[p] = row(reid[p]).
 * "Ascending" makes the result a function of the graph alone -- bit-identical from run to run, whatever order the atomics of the
 * build arrived in -- and every reverse row sorted by vertex id, parallel edges in the order of their edge ids: the rows of the reverse
 * are sorted in legion_graph_check_rows_sorted's sense.  If the graph has sorted rows and no dead entries, the reverse of the reverse
 * is the graph itself and reid(reverse)[reid(reverse of reverse)[p]] == p.
 * legion_graph_build_reverse reads the FULL CSR on the device current at the call and enqueues on `stream`.  It is set-up, like
 * legion_graph_set_edge_weights and legion_graph_check_rows_sorted: it synchronises that stream (E', and the list of the rows too long
 * for one workgroup's sort, are read back) and must not be captured.  The three arrays are plain allocations of the library, owned by
 * the graph and freed by legion_graph_destroy; every temporary (N-sized cursors, the lists, a scratch as long as the long rows
 * together -- nothing E-sized) is freed before the call returns.  Returns 0; a second call returns 0 without work.  Returns -1, with
 * nothing enqueued and nothing allocated, for a null graph or N > LEGION_REVERSE_MAX_NODES (the reach of the two-level scan: 2^20 sums
 * of 256 counts).  N == 0 or E == 0 gives rindptr all zero and E' = 0.
 * legion_graph_reverse_csr returns E' and the three device pointers; before a build, and for a null graph, -1 and nulls.  Any
 * out-pointer may be null.
 * Not offered: N above 2^28; the reverse of a cached topology or of a partition; to_bidirected; pairing an edge with its reverse edge
 * id (seed-edge exclusion); heterogeneous graphs; the server, the launcher and the wire.
 * (The pairing exists since: legion_reverse_edge_ids, below, searches a row of this reverse CSR -- or of a graph with sorted rows -- for
 * an edge's reverse edge id; "not offered" speaks of this call, which pairs nothing.) */
#define LEGION_REVERSE_MAX_NODES (1 << 28)
int32_t legion_graph_build_reverse(LegionGraphStorage* g, legion_stream_t stream);
int64_t legion_graph_reverse_csr(const LegionGraphStorage* g, const int64_t** rindptr, const int32_t** rcol, const int64_t** reid);

/* FeatureStorage: SS/storage/feature_storage.cu:18-90.  ids/labels are HOST arrays copied to
 * device `dev_id`; mode selects the training / validation / testing set. */
LegionFeatureStorage* legion_feature_create(int32_t partition_count, int32_t total_num_nodes,
                                            int32_t float_feature_len,
                                            const float* all_float_feature_devptr);
void legion_feature_set_ids(LegionFeatureStorage* f, int32_t dev_id, int32_t mode,
                            const int32_t* host_ids, const int32_t* host_labels, int32_t count);
void legion_feature_destroy(LegionFeatureStorage* f);
/* legion_feature_create with a feature dtype (LEGION_FEATURE_*).  LEGION_FEATURE_F32 is legion_feature_create (the caller's
 * table is used in place).  LEGION_FEATURE_BF16: the library converts the caller's float32 table (device-accessible,
 * N x float_feature_len) into a bf16 table of its own -- in HBM, or in mapped pinned host memory under
 * LEGION_TABLE_PLACEMENT=pinned -- and frees it in legion_feature_destroy; the caller's table may go once this returns.
 * NULL for an unknown dtype. */
LegionFeatureStorage* legion_feature_create_ex(int32_t partition_count, int32_t total_num_nodes, int32_t float_feature_len,
                                               int32_t feature_dtype, const float* all_float_feature_devptr);
int32_t legion_feature_dtype(const LegionFeatureStorage* f);
int64_t legion_feature_row_bytes(const LegionFeatureStorage* f);     /* bytes of one stored row: 4 D (f32), 2 round_up(D, 8) (bf16) */
const void* legion_feature_table(const LegionFeatureStorage* f);     /* device address of the stored table */
/* The conversion on its own: src float32[rows x D] -> dst bf16[rows x round_up(D, 8)] (both device-accessible), round to nearest
 * even, NaN kept a NaN, pad elements zero; enqueued on `stream`. */
void legion_convert_f32_to_bf16(legion_stream_t stream, const float* src, int64_t rows, int32_t D, uint16_t* dst);

/* MemoryPool + its buffers: SS/engine/server.cu:172-273 (GPURunner::Initialize buffer
 * allocation) and SS/engine/ipc_service.cu:134-211 (the 7 IPC-shared outputs per pipe slot).
 * fanout/hop_num size num_ids = B(1 + f1 + f1 f2 + ...) (SS/engine/server.cu:187-199). */
LegionMemoryPool* legion_pool_create(int32_t dev_id, int32_t total_num_nodes, int32_t batch_size,
                                     const int32_t* fanout, int32_t hop_num, int32_t float_feature_len,
                                     int32_t pipeline_depth);
/* SS/engine/server.cu:275-283: rows = int(1.2 * MaxIdNum) in the reference; caller passes rows. */
void legion_pool_alloc_features(LegionMemoryPool* p, int64_t rows);
/* Feature output dtype (LEGION_FEATURE_*): the dtype of the rows the pool's gathers write, independent of the storage dtype.
 * LEGION_FEATURE_BF16: float_features is a contiguous bf16[rows x D] (stride D, no pad); each row is the bf16 of the float32 row
 * (round to nearest even, NaN kept a quiet NaN), or a bf16 storage's stored bits verbatim.  Call before
 * legion_pool_alloc_features: returns 0, or -1 after it (nothing changes), for an unknown dtype or a null pool. */
int32_t legion_pool_set_feature_out_dtype(LegionMemoryPool* p, int32_t dtype);
int32_t legion_pool_feature_out_dtype(const LegionMemoryPool* p);
/* Sampling mode of the pool's hops.  1 (default): every frontier entry of degree D at fan-out f gets min(f, D) independent draws
 * with replacement (SS/engine/operator_impl.cu:228-242).  0: without replacement (DGL's replace=False): min(f, D) distinct
 * adjacency positions -- D <= f: all of them in CSR order; D > f: Floyd's algorithm over the same per-slot draw
 * (legion_draw_distinct_batch).  Sizes, buffers and every later step are the same in both modes.  Returns 0, or -1 (nothing
 * changes) once the pool has sampled a hop (eagerly or into a captured graph), for a value other than 0 / 1, for 0 when a fan-out
 * of the pool exceeds LEGION_DISTINCT_MAX_FANOUT, or for a null pool. */
#define LEGION_DISTINCT_MAX_FANOUT 256
int32_t legion_pool_set_sample_replace(LegionMemoryPool* p, int32_t replace);
int32_t legion_pool_sample_replace(const LegionMemoryPool* p);
/* Edge-id mode of the pool (DGL's block.edata[dgl.EID]); 0 is the default.  1: every sampled edge e of a batch also gets
 * agg_edge_ids[e] (int64, legion_pool_buffer 14), indexed like agg_src_ids[e] / agg_dst_ids[e] -- the same cumulative per-hop
 * ranges (edge_counter), capacity num_ids:  agg_edge_ids[e] = indptr[agg_dst_ids[e]] + the adjacency position the slot drew, with
 * the FULL CSR's indptr -- also for a row that was read from a cached topology (the fill copies a row in CSR order).  So
 * indptr[s] <= id < indptr[s + 1] and col[id] == agg_src_ids[e]; parallel edges get their own ids.  A slot without an edge
 * (k >= min(f, D), a negative column entry, a frontier entry < 0) has no id.  Everything else a batch holds is bit for bit what it
 * is with the mode off, in both sampling modes.  Two arrays (int32 per slot, int64 per edge) are allocated when the mode is turned
 * on, outside any lane arena; with the mode off nothing is allocated and no kernel differs.  In-process only for now: the server,
 * the shared segment and the trainer end do not carry edge ids.  Returns 0, or -1 (nothing changes) once
 * the pool has sampled a hop (eagerly or into a captured graph), for a value other than 0 / 1, or for a null pool.  Lanes of a
 * pipeline take the mode through legion_pipeline_set_edge_ids. */
int32_t legion_pool_set_edge_ids(LegionMemoryPool* p, int32_t on);
int32_t legion_pool_edge_ids(const LegionMemoryPool* p);
/* Weighted mode of the pool (see legion_graph_set_edge_weights for the pick rule); 0 is the default.  1: every slot picks its
 * adjacency position by the graph's prefix table instead of the uniform draw; everything after the pick (de-duplication, compaction,
 * counters, gathers, hotness, edge ids) is unchanged.  Nothing is allocated in the pool.  Returns 0, or -1 (nothing changes) once the
 * pool has sampled a hop, for a value other than 0 / 1, for a null pool, or for 1 while the pool samples without replacement;
 * legion_pool_set_sample_replace(p, 0) returns -1 on a weighted pool.  A weighted hop against a graph without a table is not
 * sampled (error bit 8).  Lanes of a pipeline take the mode through legion_pipeline_set_sample_weighted. */
int32_t legion_pool_set_sample_weighted(LegionMemoryPool* p, int32_t on);
int32_t legion_pool_sample_weighted(const LegionMemoryPool* p);
void legion_pool_set_current_pipe(LegionMemoryPool* p, int32_t pipe);
void legion_pool_set_mode_iter(LegionMemoryPool* p, int32_t mode, int32_t iter);
int32_t legion_pool_num_ids(const LegionMemoryPool* p);
/* which: 0 sampled_ids 1 float_features 2 labels 3 agg_src_off 4 agg_dst_off 5 node_counter
 *        6 edge_counter (the IPC slot order, SS/engine/ipc_service.cu:163-169,203);
 *        7 agg_src_ids 8 agg_dst_ids 9 cache_search_buffer 10 tmp_part_ind 11 tmp_part_off
 *        12 position_map (always null here); 13 node_slot (new: int32[num_ids], the feature-cache slot the sampler carried for
 *        each node of the batch, -3 = not carried: the gather looks node_map up); 14 agg_edge_ids (int64[num_ids], null unless the
 *        pool's edge-id mode is on: legion_pool_set_edge_ids).  Returns the device pointer of the CURRENT pipe slot. */
void* legion_pool_buffer(LegionMemoryPool* p, int32_t which);
/* New in this build.  The reference keeps first touches in accessed_map (N bits, memset per batch) + position_map (N entries,
 * SS/engine/memorypool.cuh:120-135); a pool here keeps NOTHING per vertex: a hop's claims are de-duplicated bucket by bucket in
 * LDS (legion_core.h).  hash buckets per lane: 8, 16, 64 or 256 by the pool's largest hop; state_bytes: one hop's claim lists +
 * the known lists (scale with the batch, not with the graph).  which = 12 of legion_pool_buffer (position_map) returns NULL. */
int32_t legion_pool_lds_buckets(const LegionMemoryPool* p);
int64_t legion_pool_state_bytes(const LegionMemoryPool* p);
/* Sticky error bits raised on the device for this pool (0 = none): 1 a de-duplication bucket that fits no LDS table, 2 batch larger than the
 * feature buffer (gather stopped at its end; the reference overruns, SS/engine/server.cu:277), 4 internal, 8 a hop not sampled
 * (a fan-out above LEGION_DISTINCT_MAX_FANOUT without replacement, lanes of one group with different sampling, edge-id or
 * weighted modes, or a weighted hop against a graph without a prefix table: legion_graph_set_edge_weights).  The
 * word lives in host-visible memory: reading it after the batch completed needs no copy. */
int32_t legion_pool_error(const LegionMemoryPool* p);
void legion_pool_destroy(LegionMemoryPool* p);

/* UnifiedCache: SS/cache/cache.cu:295-321 (Initialize), :323-328 (InitializeCacheController). */
LegionUnifiedCache* legion_cache_create(int64_t cache_memory, int32_t float_feature_len,
                                        int32_t train_step, int32_t device_count,
                                        int32_t total_num_nodes);
void legion_cache_init_controller(LegionUnifiedCache* c, int32_t dev_id);
/* New in this build (no counterpart in the reference, whose GPUs had 16-80 GB): with caches striped over a clique of Kg
 * GPUs (cache_impl.cuh:89-109) every member may ALSO keep a private copy of the clique's hottest rows, as many as
 * `bytes` hold.  Lookup results (hit mask, global slot in cache_search_buffer) are unchanged; a hit whose hotness rank is
 * below the replica size is read from local HBM instead of a peer over xGMI.  Call before legion_cache_fill_up*. */
void legion_cache_set_replica_memory(LegionUnifiedCache* c, int64_t bytes);
int32_t legion_cache_replica_rows(const LegionUnifiedCache* c, int32_t dev_id);
/* Enables row-source statistics of the gathers on dev_id (Kg > 1) and returns the totals so far:
 * out2[0] rows read through a stripe pointer (own or peer), out2[1] rows read from the local replica. */
void legion_cache_gather_stats(LegionUnifiedCache* c, int32_t dev_id, uint64_t* out2);
/* same with out3[2] = the part of out3[0] that came from ANOTHER member's stripe (over xGMI between physical GPUs) */
void legion_cache_gather_stats3(LegionUnifiedCache* c, int32_t dev_id, uint64_t* out3);
/* pauses (0) / resumes (1) the counting: it costs the gather an atomic per hit row, so measurements count in an untimed pass */
void legion_cache_gather_stats_enable(LegionUnifiedCache* c, int32_t on);
/* SS/cache/cache.cu:360-443.  Hotness is summed over the clique on the clique leader through
 * peer pointers (one process, several GPUs); when `world_reduced` is non-zero the caller has
 * already all-reduced the counters across processes with RCCL and they are used as they are. */
void legion_cache_candidate_selection(LegionUnifiedCache* c, int32_t cache_agg_mode,
                                      LegionGraphStorage* graph, int32_t world_reduced);
/* The hotness all-reduce as the product's own RCCL call (collective.hip; reference: the leader's aggregate_access loop over peer
 * pointers, SS/cache/cache.cu:408-411,428-431).  Inside ONE server process (a thread per GPU) CandidateSelection issues it itself
 * over the clique's distinct physical GPUs (LegionTuning.hotness_reduce).  With one process per GPU the host program carries a
 * 128-byte unique id from rank 0 to every rank (any channel), each rank joins with the logical GPU it owns, and
 * legion_cache_allreduce_hotness sums GPU dev_id's two uint64[N] counter arrays in place over all ranks; then
 * candidate_selection(world_reduced = 1).  Returns: 1 / the world size on success, 0 on failure. */
int32_t legion_collective_unique_id(void* out128);
int32_t legion_collective_init_rank(const void* id128, int32_t world, int32_t rank, int32_t dev_id);
int32_t legion_collective_allreduce_u64(void* devptr, int64_t count, double* ms_out);
void legion_collective_destroy(void);
int32_t legion_cache_allreduce_hotness(LegionUnifiedCache* c, int32_t dev_id, double* ms_out);
/* how the last candidate selection summed the counters of dev_id's clique: 0 nothing to sum / taken as given, 1 the leader loop
 * over peer pointers, 2 an RCCL all-reduce issued by the library */
int32_t legion_cache_hotness_reduce_path(const LegionUnifiedCache* c, int32_t dev_id);
/* SS/cache/cache.cu:445-551; counters[2] = PCIe/xGMI transaction counts (zeros reproduce v2). */
void legion_cache_cost_model(LegionUnifiedCache* c, LegionFeatureStorage* feature,
                             LegionGraphStorage* graph, const uint64_t* counters, int32_t train_step);
/* Bypass for the all-resident configuration: fix the capacities instead of solving for them. */
void legion_cache_set_capacity(LegionUnifiedCache* c, int32_t node_capacity, int32_t edge_capacity);
/* SS/cache/cache.cu:553-611 */
void legion_cache_fill_up(LegionUnifiedCache* c, LegionFeatureStorage* feature, LegionGraphStorage* graph);
/* The hybrid CPU-cache / GPU-cache tier: UnifiedCache::HybridInit (SS/cache/cache.cu:614-670) with
 * PreSCCacheController::HybridInsert (:138-153, HybridInitPair SS/cache/cache_impl.cuh:113-123) INSTEAD OF candidate_selection +
 * cost_model + fill_up -- the call the reference keeps commented out at SS/engine/server.cu:112.  Every GPU orders the vertices by
 * its OWN PreSC counters (no clique sum); the gpu_cache_capacity hottest rows live in an HBM cache (slots cpu_cap + rank), the next
 * cpu_cache_capacity in a mapped pinned host cache (slots rank - gpu_cap), everything else is a miss; the topology maps stay empty.
 * The gather then resolves a slot as feat_cache_lookup does (cache_impl.cuh:202-235).  The capacities are the disk-mode
 * meta_config fields 14 and 15 (SS/storage/storage_management.cu:91-94).  The reference fills neither cache (cache.cu:616,656);
 * here both are filled from the feature table.  miss_from_table != 0: a miss row is read from the FeatureStorage table (the stand-in
 * for the unreleased SSD reader, IOSubmit SS/engine/operator_impl.cu:522-539); 0: as that kernel, a miss row is left unwritten. */
void legion_cache_hybrid_init(LegionUnifiedCache* c, LegionFeatureStorage* feature, LegionGraphStorage* graph,
                              int32_t cpu_cache_capacity, int32_t gpu_cache_capacity, int32_t miss_from_table);
/* device address of GPU dev_id's CPU cache (mapped pinned host memory, float[cpu_cache_capacity x D]) / of its HBM cache
 * (float[capacity x D]: this member's stripe after fill_up, the GPU cache after hybrid_init); null before either */
const float* legion_cache_hybrid_cpu_cache(const LegionUnifiedCache* c, int32_t dev_id);
const float* legion_cache_feature_cache(const LegionUnifiedCache* c, int32_t dev_id);
void legion_cache_destroy(LegionUnifiedCache* c);
/* A clique spread over PROCESSES (one process per GPU, Kg = world size): every rank owns member
 * `dev` = its rank (legion_set_local_device), builds its own stripe, publishes three IPC handles
 * (feature cache, cached CSR indptr, cached CSR columns; 192 bytes), opens the other members' handles
 * and links them into its pointer tables: remote cache rows and adjacency are then read with direct
 * peer loads over xGMI, as the reference does over NVLink inside one process (cache_impl.cuh:268,
 * operator_impl.cu:228-242).  Order on every rank: PreSC -> all-reduce hotness (RCCL) ->
 * set_peer_max_ids -> candidate_selection(world_reduced = 1) -> cost_model -> fill_up_local -> export ->
 * all-gather handles -> import_peer for every other rank -> fill_up_link. */
void legion_set_local_device(int32_t dev);
void legion_cache_set_peer_max_ids(LegionUnifiedCache* c, const int32_t* max_ids, int32_t n);
void legion_cache_fill_up_local(LegionUnifiedCache* c, LegionFeatureStorage* feature, LegionGraphStorage* graph);
void legion_cache_export(LegionUnifiedCache* c, LegionGraphStorage* graph, int32_t dev_id, void* handles192);
void legion_cache_import_peer(LegionUnifiedCache* c, LegionGraphStorage* graph, int32_t local_dev, int32_t peer_dev,
                              const void* handles192);
void legion_cache_fill_up_link(LegionUnifiedCache* c, LegionFeatureStorage* feature, LegionGraphStorage* graph);

/* introspection for the parity tests; arrays are device pointers on the clique leader */
int32_t legion_cache_node_capacity(const LegionUnifiedCache* c, int32_t dev_id);
int32_t legion_cache_edge_capacity(const LegionUnifiedCache* c, int32_t dev_id);
int32_t legion_cache_max_id_num(const LegionUnifiedCache* c, int32_t dev_id);
/* 64-byte transactions GPU dev_id's PreSC epoch spent on topology reads, counted by the sampler itself
 * (per sampled row: 1 for the row-pointer pair + min(fan-out, ceil(4*deg/64)) for the picks).  This is the
 * quantity the paper took from Intel PCM and v2 hard-wires to 0 (SS/engine/server.cu:105-110,
 * SS/engine/monitor.cuh); sum it over the GPUs and pass it as counters[0] to legion_cache_cost_model to
 * restore the topology-vs-feature trade-off, or pass {0,0} to reproduce v2. */
uint64_t legion_cache_topo_transactions(LegionUnifiedCache* c, int32_t dev_id);
/* which: 0 QF 1 QT (int32[N]) 2 AF 3 AT (uint64[N]) 4 node_access_time 5 edge_access_time
 *        (uint64[N], per device) 6 node_map 8 edge_offset_map (int32[N]) 7 edge_index_map (int8[N]) */
void* legion_cache_array(LegionUnifiedCache* c, int32_t dev_id, int32_t which);
/* UnifiedCache::FindTopo / FindFeat (SS/cache/cache.cu:335-357) on device arrays.  The sampler and
 * the gather resolve rows themselves (row headers, fused lookup); these remain for callers that
 * want the reference's explicit outputs: owner device / row offset or -2, cache slot or -2. */
void legion_cache_find_topo(LegionUnifiedCache* c, int32_t dev_id, legion_stream_t stream,
                            const int32_t* input_ids, int32_t batch_size, char* partition_index,
                            int32_t* partition_offset);
void legion_cache_find_feat(LegionUnifiedCache* c, int32_t dev_id, legion_stream_t stream,
                            const int32_t* sampled_ids, int32_t* cache_offset, const int32_t* node_counter,
                            int32_t op_id);

/* =====================================================================================
 * 3. Runner / Server / IPC -- SS/engine/server.h:5-33, SS/engine/ipc_service.h:6-35,
 *    sampling_server/sampling_server.cpp:7 (Run(fanout, gpu_number, in_memory_mode, cache_mode)).
 * ===================================================================================== */
LegionServer* NewGPUServer(void);
void legion_server_initialize(LegionServer* s, int32_t global_shard_count, const int32_t* fanout,
                              int32_t hop_num, int32_t in_memory_mode);
void legion_server_presc(LegionServer* s, int32_t cache_agg_mode);
void legion_server_run(LegionServer* s);
void legion_server_finalize(LegionServer* s);
/* pybind `sampling_server.Run` equivalent; reads ./meta_config from the cwd */
int32_t legion_run(const int32_t* fanout, int32_t hop_num, int32_t gpu_number, int32_t in_memory_mode,
                   int32_t cache_mode);
/* Feature dtype (LEGION_FEATURE_*) of the tables the NEXT legion_server_initialize / legion_run loads: the float32 `features`
 * file is converted while it is placed.  Returns 0, or -1 for an unknown dtype (nothing changes). */
int32_t legion_server_set_feature_dtype(int32_t feature_dtype);
/* Feature output dtype (LEGION_FEATURE_*) of the rows the NEXT legion_server_initialize / legion_run hands to its trainers
 * (published in the shared segment's extension, version 4).  Returns 0, or -1 for an unknown dtype (nothing changes). */
int32_t legion_server_set_feature_out_dtype(int32_t feature_out_dtype);
/* Sampling mode (legion_pool_set_sample_replace) of every pool the NEXT legion_server_initialize / legion_run creates, PreSC's
 * included.  Returns 0, or -1 for a value other than 0 / 1 (nothing changes).  The trainer side needs no change. */
int32_t legion_server_set_sample_replace(int32_t replace);

LegionIPCEnv* NewIPCEnv(int32_t device_count);
/* step arithmetic, SS/engine/ipc_service.cu:60-132,213-253 (host only, no GPU needed) */
void legion_ipc_coordinate(LegionIPCEnv* e, int32_t partition_count, const int32_t* train_num,
                           const int32_t* valid_num, const int32_t* test_num, int32_t raw_batch_size,
                           int32_t epoch);
int32_t legion_ipc_train_step(LegionIPCEnv* e);
int32_t legion_ipc_max_step(LegionIPCEnv* e);
int32_t legion_ipc_current_mode(LegionIPCEnv* e, int32_t global_batch_id);
int32_t legion_ipc_local_batch_id(LegionIPCEnv* e, int32_t global_batch_id);
int32_t legion_ipc_current_batchsize(LegionIPCEnv* e, int32_t dev_id, int32_t mode);
void legion_ipc_finalize(LegionIPCEnv* e);

/* Lane groups: every kernel of the path takes an array of per-mini-batch buffer descriptors and is
 * launched with grid.y = lanes, so ONE launch of each kernel serves `n` independent mini-batches
 * (lane i produces batch counter0 + i into pool i).  The reference-shaped operators above are the
 * n = 1 case.  No reference counterpart: this is how the path keeps 256 CUs busy at B = 1024. */
typedef struct LegionLaneGroup LegionLaneGroup;
LegionLaneGroup* legion_group_create(LegionMemoryPool** pools, int32_t n);
void legion_group_set_iter_state(LegionLaneGroup* g, int32_t* iter_state_devptr);
void legion_group_destroy(LegionLaneGroup* g);
void legion_enqueue_group(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                          LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t batch_size,
                          int32_t counter0, int32_t dev_id, int32_t mode, const int32_t* fanout, int32_t hop_num);
/* same with only the first n_active lanes working */
void legion_enqueue_group_n(legion_stream_t strm_hdl, LegionGraphStorage* graph, LegionFeatureStorage* feature,
                            LegionUnifiedCache* cache, LegionLaneGroup* group, int32_t n_active, int32_t batch_size,
                            int32_t counter0, int32_t dev_id, int32_t mode, const int32_t* fanout, int32_t hop_num);

/* Pipeline: `slots` groups of `group_size` mini-batches in flight on one GPU; each group is replayed
 * as one hipGraph on its own stream (sizes and the batch index live on the device, so a replay
 * needs no argument update).  The MI355X-native form of the Runner's inter-batch pipe
 * (SS/engine/server.cu:302-332 with INTERBATCH_CON output slots): submit() never blocks on the
 * group it enqueues, only on the slot's previous one.  feature_rows sizes each lane's feature buffer
 * (SS/engine/server.cu:275-283).  use_graph: bit 0 = replay hipGraphs (else eager launches), bit 1 =
 * let kernels of different slots overlap on the GPU (default: slots are chained by an event, so a
 * group's launch latency hides behind the previous group but their kernels never share the GPU). */
typedef struct LegionPipeline LegionPipeline;
LegionPipeline* legion_pipeline_create(LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                       LegionUnifiedCache* cache, int32_t dev_id, int32_t batch_size,
                                       const int32_t* fanout, int32_t hop_num, int32_t group_size,
                                       int32_t slots, int64_t feature_rows, int32_t use_graph);
/* the same with the lanes' feature output dtype (legion_pool_set_feature_out_dtype); legion_pipeline_create is
 * feature_out_dtype = LEGION_FEATURE_F32.  Returns NULL for an unknown dtype.  bf16 output refuses peer_gather = bulk
 * (legion_pipeline_bulk_enable returns 0). */
LegionPipeline* legion_pipeline_create_ex(LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                          LegionUnifiedCache* cache, int32_t dev_id, int32_t batch_size,
                                          const int32_t* fanout, int32_t hop_num, int32_t group_size,
                                          int32_t slots, int64_t feature_rows, int32_t use_graph, int32_t feature_out_dtype);
/* The three setters below: where one succeeds, the pipeline's GPU is the calling thread's current device afterwards.
 * sampling mode of every lane (legion_pool_set_sample_replace).  Returns 0, or -1 (nothing changes) once the pipeline has
 * submitted a group, for a value other than 0 / 1 or for 0 with a fan-out above LEGION_DISTINCT_MAX_FANOUT. */
int32_t legion_pipeline_set_sample_replace(LegionPipeline* p, int32_t replace);
/* edge-id mode of every lane (legion_pool_set_edge_ids; a lane's ids: legion_pool_buffer(legion_pipeline_pool(..), 14)).  Returns
 * 0, or -1 (nothing changes) once the pipeline has submitted a group or for a value other than 0 / 1. */
int32_t legion_pipeline_set_edge_ids(LegionPipeline* p, int32_t on);
/* weighted mode of every lane (legion_pool_set_sample_weighted).  Returns 0, or -1 (nothing changes) once the pipeline has submitted
 * a group, for a value other than 0 / 1, or for 1 on a pipeline that samples without replacement. */
int32_t legion_pipeline_set_sample_weighted(LegionPipeline* p, int32_t on);
/* enqueues batches counter0 .. counter0 + group_size - 1; returns the slot */
int32_t legion_pipeline_submit(LegionPipeline* p, int32_t counter0, int32_t mode);
/* only the first n_active lanes work (tail of a run that is not a multiple of group_size) */
int32_t legion_pipeline_submit_n(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active);
void legion_pipeline_wait(LegionPipeline* p, int32_t slot);                          /* slot < 0: all slots */
LegionMemoryPool* legion_pipeline_pool(LegionPipeline* p, int32_t slot, int32_t lane);
void legion_pipeline_destroy(LegionPipeline* p);
/* Owner-bucketed bulk transfer for a striped feature cache (LegionTuning.peer_gather = bulk; SURVEY section 7 "hard parts"; the
 * alternative to the 512-1024-byte direct peer loads of SS/cache/cache_impl.cuh:268).  A pipeline created with use_graph bits 5 + 6 keeps
 * its lanes' trainer-visible arrays in ONE arena other GPUs and processes can reach (shuffled physical chunks created exportable; a
 * plain allocation with LegionTuning.arena_scatter_mb = 0).  Per group, phase A on every member of the clique
 * (sampler, bucket pass that lists per owner {row inside its stripe, destination inside the requester's arena}, gather of everything
 * that is not another member's stripe) -> the caller's barrier -> phase B on every member as an OWNER (its rows, read from its own
 * HBM, pushed to the requesters with coalesced posted stores) -> barrier.  Lookup results and rows are those of the direct
 * arrangement, bit for bit.  _export / _import carry what a member in another process needs (<= 512 bytes: IPC handles of the lists and
 * of a plain arena, or the name of the abstract unix socket that serves a chunked arena's file descriptors to a same-user peer), _link
 * takes a member that lives in the same process (and grants its GPU access to a chunked arena). */
int32_t legion_pipeline_bulk_enable(LegionPipeline* p);
int32_t legion_pipeline_bulk_export(LegionPipeline* p, void* out_handles, int32_t out_bytes);
int32_t legion_pipeline_bulk_import(LegionPipeline* p, const void* handles);
int32_t legion_pipeline_bulk_link(LegionPipeline* p, LegionPipeline* other);
int32_t legion_pipeline_bulk_phase_a(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size);
void legion_pipeline_bulk_phase_b(LegionPipeline* p, int32_t slot);
int64_t legion_pipeline_bulk_listed(LegionPipeline* p, int32_t slot);
/* Measurement aid: HIP events on each slot's stream around every gather launch.  While it is on,
 * groups are launched eagerly (HIP cannot time events recorded by graph nodes).  read() fills, per
 * gather op id, the summed elapsed ms and the launch count of every batch waited for since begin();
 * returns the op count. */
void legion_pipeline_profile_begin(LegionPipeline* p);
void legion_pipeline_profile_end(LegionPipeline* p);
int32_t legion_pipeline_profile_read(LegionPipeline* p, int32_t* op_ids, double* ms_sums, int64_t* counts,
                                     int32_t cap);
/* Measurement aid: the gather of the LAST op of the group sitting in `slot`, launched `repeats` more times over the lanes as they
 * stand -- the kernel instance, grid and ranges of the group's own op list (multiGPU_feat_cache_lookup for op 3H+1,
 * SS/cache/cache_impl.cuh:239-272) -- each launch between two HIP events on the slot's stream; ms_each[i] = its duration.  A caller
 * may rewrite the lanes' ids (legion_pool_buffer 0 / 13) in between: bench.py's roofline.cold gathers rows of which none repeats
 * inside the launch.  Returns the launches timed. */
int32_t legion_pipeline_regather_last(LegionPipeline* p, int32_t slot, int32_t n_active, int32_t repeats, double* ms_each);

/* =====================================================================================
 * 4. Kernel-level launchers (what the operators call), exported so the hot kernels can be
 *    measured and tested alone.
 * ===================================================================================== */
/* The gather of SS/cache/cache_impl.cuh:239-272 with the id->slot lookup of
 * SS/cache/cache.cu:180-215 fused in.  range[0..1] = {row offset, row count} is read on the
 * device (node_counter layout).  node_map may be NULL (every row is a miss). */
void legion_gather_rows(legion_stream_t stream, const float* full_table, const float* const* cache_tables,
                        const int32_t* node_map, int32_t node_capacity, int32_t float_feature_len,
                        int32_t total_num_nodes, const int32_t* sampled_ids, int32_t* cache_index_out,
                        const int32_t* range_devptr, float* dst, int32_t max_rows);
/* legion_gather_rows with every argument of a gather launch, so that each instance of the gather kernel can be run alone.
 *   dtype, out_dtype  LEGION_FEATURE_*: the row format of full_table and of every cache table, and that of dst.  bf16 source rows are
 *                     round_up(float_feature_len, 8) elements apart (legion_feature_row_bytes), their pad elements are never stored;
 *                     dst rows are float_feature_len elements of out_dtype, no pad.
 *   node_slot         NULL, or int32 indexed like sampled_ids: the feature-cache slot carried for each row (what node_map[id] would
 *                     give: a slot >= 0 or -2 for a miss), or -3 for "look it up".  Read only with a node_map.
 *   dst_rows          rows dst holds: rows range[0] + r >= dst_rows are not written (a lane's feature buffer; legion_gather_rows
 *                     passes INT32_MAX)
 *   grid_rows         the rows the grid is sized for, 0 = max_rows (a lane with more rows is still gathered whole: workgroups walk tiles)
 *   last_op           0 / 1: the kernel instance of a batch's early gathers / of its last one (legion_gather_rows runs the last one's)
 *   plan_out          NULL, or host int32[3] filled before the call returns with what was launched: {row format 0 .. 5 = F32, F32Tail,
 *                     F32Scalar, Bf16x8, Bf16Copy, F32Narrow; rows per tile; grid x}, {-1, 0, 0} where there was nothing to launch
 *                     (float_feature_len <= 0 or max_rows <= 0).  LEGION_GATHER_ROWS (LegionTuning.gather_rows_per_wg) applies as in a batch.
 * Returns 0, or -1 with nothing enqueued and plan_out untouched for a dtype or out_dtype that is no LEGION_FEATURE_*. */
int32_t legion_gather_rows_fmt(legion_stream_t stream, int32_t dtype, int32_t out_dtype, const void* full_table,
                               const void* const* cache_tables, const int32_t* node_map, int32_t node_capacity,
                               int32_t float_feature_len, int32_t total_num_nodes, const int32_t* sampled_ids,
                               const int32_t* node_slot, int32_t* cache_index_out, const int32_t* range_devptr, void* dst,
                               int32_t max_rows, int32_t dst_rows, int32_t grid_rows, int32_t last_op, int32_t* plan_out);
/* the draw of SS/engine/operator_impl.cu:235-238 evaluated on the GPU for n (idx, deg) pairs */
void legion_draw_batch(legion_stream_t stream, const int32_t* idx, const int32_t* deg, int32_t* out,
                       int32_t n);
/* the picks of sampling without replacement for n frontier entries: entry i has its first slot at base[i] (q * f) and degree
 * deg[i]; out[i * f + k] = its pick k (an adjacency position) or -1 for k >= min(f, deg[i]).  Returns 0, or -1 for f outside
 * [1, LEGION_DISTINCT_MAX_FANOUT] (nothing is launched). */
int32_t legion_draw_distinct_batch(legion_stream_t stream, const int32_t* base, const int32_t* deg, int32_t f, int32_t* out,
                                   int32_t n);
/* the weighted pick rule on its own (legion_graph_set_edge_weights), for n slots: slot idx[i] in the row that starts at row_start[i]
 * of cdf and has deg[i] entries; out[i] = pick, or -1 for deg[i] <= 0 or a row total of 0 */
void legion_draw_weighted_batch(legion_stream_t stream, const int32_t* idx, const int64_t* row_start, const int32_t* deg,
                                const float* cdf, int32_t* out, int32_t n);
/* Random walks over the graph (DGL's dgl.sampling.random_walk), new in this build; no reference counterpart.
 * num_walks walks of `length` steps: traces_out is int32[num_walks x (length + 1)], row-major, and edge_ids_out, if not NULL,
 * int64[num_walks x length] (both device memory).  Everything is enqueued on `stream`, on the device current at the call; nothing
 * synchronises with the host, and the call may be captured into a graph.  The walk reads the FULL CSR only (slot partition_count of
 * the pointer tables: the arrays given to legion_graph_create), and edge_cdf when weighted; a GPU's cached topology and its column-slot
 * copy are not read.
 * Walk w:  traces[w][0] = seeds[w], copied as given.  For step j = 1 .. length let v = traces[w][j - 1], n = base + w * length + (j - 1)
 * and minstd(k) = 48271^k mod (2^31 - 1), the power of the sampler's draw.  Then, in this order:
 *   1. ended walk: v < 0 or v >= node_num (a bad seed too): traces[w][j] = -1, and so is every later entry -- no memory is read for v;
 *   2. restart, only if restart_prob > 0: y = minstd((uint32)(n + 1) + 2^31), r2 = (double)(y - 1) / 2147483646.0; r2 < (double)restart_prob:
 *      the walk ends before this transition (DGL's restart_prob).  With restart_prob == 0 nothing is drawn;
 *   3. row: s = indptr[v], D = indptr[v + 1] - s; D == 0: the walk ends;
 *   4. pick: x = minstd(n + 1), r = (double)(x - 1) / 2147483646.0.  Unweighted: pick = (int)(r * D), the sampler's uniform draw.
 *      Weighted: the pick of legion_graph_set_edge_weights -- T = edge_cdf[s + D - 1]; T == 0: the walk ends; else t = r * (double)T and
 *      pick = min(#{ i in [0, D) : (double)edge_cdf[s + i] <= t }, D - 1), by the same upper-bound search;
 *   5. next vertex: u = col[s + pick]; u < 0 (a dead column entry): the walk ends; else traces[w][j] = u and edge_ids[w][j - 1] = s + pick;
 *   6. wherever traces[w][j] == -1, edge_ids[w][j - 1] == -1.
 * With all weights 1.0f (D < 2^24) the weighted walk is the unweighted one bit for bit.  Since 48271 generates the whole group,
 * minstd(k + 2^31) == minstd(k + 2): the restart draw of index n is the number the pick of index n + 2 uses, so a
 * walk that survives step j's restart draw picks at step j + 2 with r >= restart_prob: with restart_prob > 0 the picks from the third
 * step on favour the later entries of a row.  The rule is kept as specified; DESIGN.md 4.11 says what would remove the dependence.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, seeds_devptr or traces_out; num_walks < 0; length < 1;
 * base < 0; base + num_walks * length > 2^31 - 1 (the draw index, the restart offset included, stays where the power tables reach);
 * weighted outside {0, 1}; weighted == 1 on a graph without a table; restart_prob NaN or outside [0, 1].  num_walks == 0 returns 0
 * and enqueues nothing.  A weighted walk counts as a weighted hop for legion_graph_set_edge_weights: the table cannot be replaced
 * afterwards.  node2vec's p / q bias is legion_node2vec_walk, below.  Not offered: metapaths; the server, the launcher and the wire. */
int32_t legion_random_walk(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* seeds_devptr, int32_t num_walks,
                           int32_t length, int32_t weighted, float restart_prob, int64_t base, int32_t* traces_out,
                           int64_t* edge_ids_out /* may be NULL */);
/* node2vec walks over the graph (DGL's dgl.sampling.node2vec_random_walk), new in this build; no reference counterpart.  A second-order
 * walk: the step from v depends on the vertex t the walk came from, by rejection sampling -- candidates are drawn as legion_random_walk
 * draws its step and accepted with probability wt / Mx, wt = 1/p for a return to t, 1 for a neighbour of t, 1/q for any other vertex.
 * Buffers, stream, capture and what is read (the FULL CSR, edge_cdf when weighted) as in legion_random_walk.  "u is a neighbour of t" is
 * a binary search of t's row, so the graph's rows must have been checked sorted (legion_graph_check_rows_sorted == 1).
 * Walk w:  traces[w][0] = seeds[w], copied as given.  Step j = 1 .. length has v = traces[w][j - 1], t = traces[w][j - 2] (none at j = 1),
 * draw index n = base + w * length + (j - 1), minstd(k) = 48271^k mod (2^31 - 1), and a = 1.0 / (double)p, b = 1.0 / (double)q,
 * Mx = max(a, 1.0, b) (IEEE double, computed once on the host).  Then, in this order:
 *   1. ended walk: v < 0 or v >= node_num (a bad seed too): traces[w][j] = -1, and so is every later entry -- no memory is read for v;
 *   2. row: s = indptr[v], D = indptr[v + 1] - s; D == 0: the walk ends.  Weighted: T = edge_cdf[s + D - 1]; T == 0: the walk ends;
 *   3. tries i = 0, 1, .. max_tries - 1:
 *        candidate draw: x = minstd((uint32)(n + 1) + i * 2^23), r = (double)(x - 1) / 2147483646.0;
 *        pick: unweighted pick = (int)(r * D); weighted t' = r * (double)T and pick = min(#{ e in [0, D) : (double)edge_cdf[s + e] <= t' }, D - 1),
 *          the upper-bound search of legion_random_walk;
 *        candidate: u = col[s + pick]; u < 0 (a dead column entry): the walk ends at once;
 *        unconditional accept: at j == 1, or at i == max_tries - 1 (the last try), u is accepted without an accept draw;
 *        class: else wt = a if u == t; else 1.0 if u occurs in col[indptr[t] .. indptr[t + 1]); else b -- the paper's d(t, u) = 0 / 1 / 2; on
 *          the symmetric graphs node2vec is used on it equals DGL's test;
 *        accept draw: y = minstd((uint32)(n + 1) + i * 2^23 + 2^22), ry = (double)(y - 1) / 2147483646.0;
 *        accept test: u is accepted iff ry * Mx < wt, in double (wt == Mx always accepts: ry < 1);
 *   4. on acceptance traces[w][j] = u and edge_ids[w][j - 1] = s + pick; wherever traces[w][j] == -1, edge_ids[w][j - 1] == -1.
 * With p == q == 1 (every wt == Mx), or with max_tries == 1 (the first try is the last), the walk is legion_random_walk's with
 * restart_prob = 0, bit for bit.  Within a step the 2 * 256 draw indices are distinct (255 * 2^23 + 2^22 < 2^31 - 2, the order of 48271);
 * they coincide only with draws of steps whose index differs by a multiple of 2^22, walks four million steps away: accepted.  The forced
 * acceptance at the last try has probability at most (15/16)^255, about 7e-8, per step at the default max_tries and the worst legal bias.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, seeds_devptr or traces_out; num_walks < 0; length < 1;
 * base < 0; base + num_walks * length > 2^31 - 1; weighted outside {0, 1}; weighted == 1 on a graph without a table; max_tries outside
 * [1, LEGION_NODE2VEC_MAX_TRIES]; p or q NaN, infinite or <= 0; min(a, 1, b) * LEGION_NODE2VEC_MAX_BIAS < max(a, 1, b); a graph whose rows
 * legion_graph_check_rows_sorted has not checked, or has found unsorted.  num_walks == 0 returns 0 and enqueues nothing.  A weighted call
 * counts as a weighted hop for legion_graph_set_edge_weights.  Not offered: the server, the launcher and the wire. */
#define LEGION_NODE2VEC_MAX_TRIES 256
#define LEGION_NODE2VEC_MAX_BIAS  16
int32_t legion_node2vec_walk(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* seeds_devptr, int32_t num_walks,
                             int32_t length, float p, float q, int32_t weighted, int32_t max_tries, int64_t base,
                             int32_t* traces_out /* int32[n x (length + 1)] */, int64_t* edge_ids_out /* int64[n x length], or NULL */);
/* PinSAGE's neighbour sampler (DGL's dgl.sampling.RandomWalkNeighborSampler / PinSAGESampler on a homogeneous graph), new in this build;
 * no reference counterpart.  For each of num_seeds seeds: num_walks_per_seed (R) walks of walk_length (T) steps, the visited vertices
 * counted, and the num_neighbors (k) most visited returned with their counts.  neighbors_out and counts_out are int32[num_seeds x k],
 * row-major, device memory.  Everything is enqueued on `stream`, on the device current at the call; nothing synchronises with the host,
 * and the call may be captured into a graph.  It reads the FULL CSR only, and edge_cdf when weighted, as legion_random_walk does.  No
 * traces are written anywhere.
 * Walks.  Walk r of seed i is global walk w = i * R + r and starts at seeds[i].  Step j = 1 .. T has draw index
 * n = base + w * T + (j - 1) and is exactly steps 1-5 of legion_random_walk's rule (ended-walk test before any load, restart, row, uniform
 * or weighted pick, dead column entry) with restart_prob = termination_prob -- except that step j = 1 takes NO restart draw, whatever
 * termination_prob is: DGL passes restart_prob = 0 for the first traversal.  Steps j >= 2 take the restart draw of their index
 * (y = minstd((uint32)(n + 1) + 2^31), r2 < (double)termination_prob ends the walk) when termination_prob > 0.  With termination_prob == 0
 * the walks are, bit for bit, those of legion_random_walk over seeds with each entry repeated R times, length T, the same base.
 * Visits.  The visits of seed i are the multiset of the vertices its R walks reach at steps j = 1 .. T (trace entries >= 0).  The seed
 * position j = 0 is not a visit; the seed's own id is one whenever a walk returns to it, as in DGL.
 * Result.  The distinct visited vertices of a seed are ordered by visit count descending, ties by vertex id ascending (a total order;
 * DGL leaves ties open).  neighbors[i][m], counts[i][m] for m < k are the m-th of them; slots past the number of distinct vertices hold
 * -1 / 0.  A seed outside [0, node_num), a seed without out-edges and a seed whose walks all end at step 1 give a row of -1 / 0.
 * The rule of the walk is shared, and so is its weakness: the restart draw of index n is the number the pick of index n + 2 uses (see
 * legion_random_walk), so with termination_prob > 0 a walk that survives step j's restart draw picks at step j + 2 with r >= termination_prob.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, seeds_devptr, neighbors_out or counts_out; num_seeds < 0;
 * R < 1, T < 1 or k < 1; R * T > LEGION_PINSAGE_MAX_VISITS or k > LEGION_PINSAGE_MAX_VISITS; base < 0;
 * base + num_seeds * R * T > 2^31 - 1 (in 64 bits); weighted outside {0, 1}; weighted == 1 on a graph without a table; termination_prob
 * NaN or outside [0, 1].  num_seeds == 0 returns 0 and enqueues nothing.  A weighted call counts as a weighted hop for
 * legion_graph_set_edge_weights, like a weighted walk.  Not offered: metapaths (heterogeneous graphs); the server, the launcher, the wire. */
#define LEGION_PINSAGE_MAX_VISITS 1024
int32_t legion_pinsage_neighbors(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* seeds_devptr, int32_t num_seeds,
                                 int32_t num_walks_per_seed, int32_t walk_length, int32_t num_neighbors, int32_t weighted,
                                 float termination_prob, int64_t base, int32_t* neighbors_out /* int32[n x k] */,
                                 int32_t* counts_out /* int32[n x k] */);
/* The seeds of a link-prediction batch (DGL's as_edge_prediction_sampler with a negative sampler: find_edges, negatives,
 * compact_graphs), new in this build; no reference counterpart.  Three ops: the endpoints of B seed edges, k negative endpoints per edge
 * that are no neighbours, and the list of the distinct ids among the B (2 + k) with local indices into it -- the distinct list is what
 * legion_feature_set_ids / BatchGenerate need, whose de-duplication assumes no duplicate among a batch's seeds.  All buffers are device
 * memory.  Each op is enqueued on `stream`, on the device current at the call; nothing synchronises with the host, and each call may be
 * captured into a graph.  The two graph ops read the FULL CSR only (the arrays given to legion_graph_create).  A CSR row is the sampler's
 * dst side and a column entry its src side (col[agg_edge_ids[e]] == agg_src_ids[e]): hence `row` and `col`, not src and dst.
 *
 * legion_find_edges (DGL's g.find_edges).  With N = node_num, E = the number of column entries, for i in [0, n), e = eids[i]:
 *   1. e < 0 or e >= E: row_out[i] = col_out[i] = -1 -- no memory is read for e;
 *   2. c = col[e]; c < 0 (a dead column entry): row_out[i] = col_out[i] = -1, as everywhere else in the library;
 *   3. row_out[i] = #{ v in [0, N] : indptr[v] <= e } - 1, an upper-bound search over the N + 1 row pointers in int64: the one row v with
 *      indptr[v] <= e < indptr[v + 1], rows without entries skipped; col_out[i] = c.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for a null graph, eids_devptr, row_out or col_out, or n < 0.  n == 0
 * returns 0 and enqueues nothing. */
int32_t legion_find_edges(legion_stream_t stream, LegionGraphStorage* graph, const int64_t* eids_devptr /* int64[n] */, int32_t n,
                          int32_t* row_out /* int32[n] */, int32_t* col_out /* int32[n] */);
/* legion_negative_sample (exclude == 0: DGL's negative_sampler.Uniform(k); with bit 1: PyG's structured_negative_sampling).  neg_out is
 * int32[n x k], row-major.  Slot m = i * k + j (i in [0, n), j in [0, k)) belongs to row r = rows[i] and has draw index nn = base + m;
 * minstd(e) = 48271^e mod (2^31 - 1), the power of the sampler's draw.  Then, in this order:
 *   1. r < 0 or r >= N: neg_out[m] = -1 -- no memory is read for r;
 *   2. tries t = 0, 1, .. max_tries - 1:
 *        draw: x = minstd((uint32)(nn + 1) + t * 2^23), r01 = (double)(x - 1) / 2147483646.0, u = (int)(r01 * N): the sampler's uniform
 *          draw over N (legion_node2vec_walk's try stepping: x of try t + 1 = x of try t * 48271^(2^23));
 *        u is rejected if exclude & 1 and u == r;
 *        u is rejected if exclude & 2 and u occurs in col[indptr[r] .. indptr[r + 1]) (a binary search of the sorted row; the pair
 *          {indptr[r], indptr[r + 1]} is loaded once per slot);
 *        the first u not rejected is neg_out[m];
 *   3. every try rejected: neg_out[m] = -1.
 * With exclude == 0 the first draw is taken and nothing but rows is read.  The index of try t coincides with try 0 of the slot t * 2^23
 * further on (as node2vec's tries coincide with steps four million steps away): accepted.  A row whose every vertex is excluded gives -1
 * at any max_tries.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, rows_devptr or neg_out; n < 0; k < 1; base < 0;
 * base + n * k > 2^31 - 1 (in 64 bits); exclude outside [0, 3]; max_tries outside [1, LEGION_NEGATIVE_MAX_TRIES] (255 * 2^23 + 2^31 < 2^32,
 * the reach of the power tables); exclude & 2 on a graph whose rows legion_graph_check_rows_sorted has not checked, or has found
 * unsorted.  n == 0 returns 0 and enqueues nothing.  Not offered: degree-biased negatives. */
#define LEGION_NEGATIVE_MAX_TRIES 256
int32_t legion_negative_sample(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                               int32_t k, int32_t exclude, int32_t max_tries, int64_t base, int32_t* neg_out /* int32[n x k] */);
/* legion_unique_ids (compact_graphs' relabelling, in order of first appearance).  No graph is involved.  For i in [0, m):
 *   1. ids[i] < 0: local_out[i] = -1; the entry is no seed;
 *   2. else first(i) = min{ j : ids[j] == ids[i] }.  The entries with first(i) == i are numbered rank = 0 .. U - 1 in index order;
 *      unique_out[rank(i)] = ids[i] for each of them, local_out[i] = rank(first(i)) for every i of 2., count_out[0] = U;
 *   3. unique_out[U .. m) = -1: the whole buffer is defined.
 * unique_out and local_out are int32[m], count_out int32[1].  scratch: device memory, 4-byte aligned, of at least
 * legion_unique_ids_scratch_bytes(m) bytes (-1 for m < 0 or m > LEGION_UNIQUE_MAX_IDS); the call clears what it needs of it on `stream`
 * itself, and two calls in flight on different streams need scratch of their own.  The result does not depend on the order in which the
 * device takes the ids.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null ids_devptr, unique_out, local_out, count_out or scratch; m < 0;
 * m > LEGION_UNIQUE_MAX_IDS; scratch_bytes below legion_unique_ids_scratch_bytes(m); unique_out, local_out or count_out overlapping
 * ids.  m == 0 returns 0 and writes count_out[0] = 0 only.
 * Not offered by these three: excluding the seed edges from the sampled neighbourhood (a consumer masks by agg_edge_ids); device-resident
 * seed sets for BatchGenerate (legion_feature_set_ids still takes host arrays); the server, the launcher and the wire.
 * (The exclusion exists since, as calls of its own: legion_reverse_edge_ids, legion_edge_set_build and legion_edge_filter_count /
 * legion_edge_filter_edges, below, drop the seed edges and their reverses from an edge list -- a pool's consumer hands them the batch's
 * agg_dst_ids, agg_src_ids and agg_edge_ids; these three ops still exclude nothing.) */
#define LEGION_UNIQUE_MAX_IDS 1048576
int64_t legion_unique_ids_scratch_bytes(int32_t m);
int32_t legion_unique_ids(legion_stream_t stream, const int32_t* ids_devptr /* int32[m] */, int32_t m, int32_t* unique_out /* int32[m] */,
                          int32_t* local_out /* int32[m] */, int32_t* count_out /* int32[1] */, void* scratch, int64_t scratch_bytes);
/* A neighbourhood taken whole (DGL's g.in_edges(v, form='all'), the edges of MultiLayerFullNeighborSampler(1) and of dgl.in_subgraph
 * followed by to_block), new in this build; no reference counterpart.  Two ops: the prefix sums of the degrees of a list of rows, and
 * every entry of those rows as a (dst, src, eid) triple.  All buffers are device memory.  Each op is enqueued on `stream`, on the device
 * current at the call; nothing synchronises with the host, and each call may be captured into a graph.  Both read the FULL CSR only (the
 * arrays given to legion_graph_create).  A CSR row is the sampler's dst side and a column entry its src side, as above.  N = node_num;
 * rows is int32[n], and its entries may repeat.
 *
 * legion_row_offsets (also DGL's g.in_degrees(v), by differences).  For i in [0, n), r = rows[i]:
 *   1. deg(i) = indptr[r + 1] - indptr[r] for r in [0, N) (the pair is one 16-byte load); for r outside the graph deg(i) = 0 and no
 *      memory is read for r.  Dead (negative) column entries count: a slot is a position in the row;
 *   2. offsets_out[i] = the sum of deg(i') over i' < i, for i in [0, n], in int64: offsets_out[n] is the total M.
 * offsets_out is int64[n + 1].  scratch: device memory, 8-byte aligned, of at least legion_row_offsets_scratch_bytes(n) bytes (one int64
 * per tile of 256 rows; -1 for n < 0 or n > LEGION_IN_EDGES_MAX_ROWS, the reach of the one-workgroup scan over at most 4 096 tile sums);
 * two calls in flight on different streams need scratch of their own.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, rows_devptr, offsets_out or scratch; n < 0;
 * n > LEGION_IN_EDGES_MAX_ROWS; scratch_bytes below legion_row_offsets_scratch_bytes(n).  n == 0 returns 0 and writes offsets_out[0] = 0
 * only.
 *
 * legion_in_edges takes rows, n, the offsets of the call above and m, the slots to write.  For slot p in [0, m):
 *   1. i = #{ v in [0, n] : offsets[v] <= p } - 1, an upper-bound binary search over the n + 1 offsets: rows without entries are skipped
 *      (a lower bound would name the first of a run of empty rows);
 *   2. i >= n (that is, p >= offsets[n]): dst_out[p] = src_out[p] = -1 and eid_out[p] = -1;
 *   3. else j = p - offsets[i], r = rows[i], e = indptr[r] + j in 64 bits: dst_out[p] = i (the position in rows: the block's dst index),
 *      src_out[p] = col[e] (a dead entry stays -1, as everywhere else in the library), eid_out[p] = e;
 *   4. memory safety does not rest on the caller's offsets: whatever they hold, nothing is read outside offsets[0 .. n], rows, indptr
 *      and col.  A slot is -1 / -1 / -1 unless i lies in [0, n), r lies in [0, N) and 0 <= j < indptr[r + 1] - indptr[r] (the pair
 *      loaded once).  For offsets that are not non-decreasing the search of 1. finds some i in [-1, n], which one is not specified;
 *      the slot is then either -1 / -1 / -1 or the entry j = p - offsets[i] of row rows[i].
 * m is a capacity: the whole of dst_out, src_out (int32[m]) and eid_out (int64[m], may be NULL) is defined.  m below M writes a prefix,
 * m above M writes -1 from M on, so that a capturing caller picks a bound without a host read.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, rows_devptr, offsets_devptr, dst_out or src_out; n < 0;
 * n > LEGION_IN_EDGES_MAX_ROWS; m < 0; m > 2^31 - 1.  m == 0 returns 0 and enqueues nothing.
 * Not offered: out-edges (there is no reverse CSR); dropping dead entries; heterogeneous graphs; more than 2^20 rows a call (a caller
 * batches); the server, the launcher and the wire. */
#define LEGION_IN_EDGES_MAX_ROWS 1048576
int64_t legion_row_offsets_scratch_bytes(int32_t n);
int32_t legion_row_offsets(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                           int64_t* offsets_out /* int64[n + 1] */, void* scratch, int64_t scratch_bytes);
int32_t legion_in_edges(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                        const int64_t* offsets_devptr /* int64[n + 1] */, int64_t m, int32_t* dst_out /* int32[m] */,
                        int32_t* src_out /* int32[m] */, int64_t* eid_out /* int64[m], or NULL */);
/* Layer-neighbour sampling (LABOR-0 of Balin and Catalyurek, NeurIPS 2023; DGL's dgl.sampling.sample_labors and
 * dgl.dataloading.LaborSampler), new in this build; no reference counterpart.  Every SOURCE vertex t has one random number r_t for the
 * whole call, and the entry t -> s is kept iff r_t < fanout / deg(s): a seed keeps fanout neighbours in expectation, and seeds with
 * common neighbours keep the same ones, so a layer has fewer input nodes than per-seed sampling gives.  The ops are legion_in_edges with
 * a predicate and a stable compaction.  Orientation, N, rows, the buffers, the stream and the FULL CSR are as for legion_in_edges: a
 * CSR row is the dst side and a column entry the src side.  The result is a pure function of the arguments.
 *
 * The hash.  splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
 * x ^ x >> 31, in uint64 (the function of the synthetic generators).  key = splitmix64((uint64)salt);
 * labor_hash(v, salt) = (uint32)(splitmix64(key ^ (uint64)(uint32)v) >> 32).  The salt is hashed first so that two salts do not merely
 * permute the same numbers among neighbouring ids.
 * The predicate.  labor_keep(h, d, fanout) is true iff h * d < fanout * 2^32, evaluated exactly in integers (d is an int64 degree and
 * may exceed 2^32: the product has up to 95 bits); there is no floating point anywhere in the rule.  Hence d <= fanout keeps every
 * entry and h == 0 always keeps.
 *
 * For slot p in [0, m):
 *   1. i, j, r, e and src = col[e] are found exactly as rules 1 - 4 of legion_in_edges find them, with the same guarantee: memory
 *      safety does not rest on the caller's offsets;
 *   2. d = indptr[r + 1] - indptr[r] from the pair loaded once, not from offsets: dead entries count in d, as they do in
 *      legion_row_offsets, and so do the slots of the row at or past m;
 *   3. the slot is kept iff it resolved to an entry (e >= 0), src >= 0, and labor_keep(labor_hash(src, salt), d, fanout);
 *   4. kept slots are written in slot order: the kept slot p goes to position #{ kept p' < p }, its triple is (dst = i, src, eid = e).
 *      dst is non-decreasing, so a caller gets CSR offsets by a search.
 * legion_labor_count leaves in scratch the exclusive prefix sums of the kept counts per tile of 1 024 slots and their total K, and
 * writes K to count_out[0] (int64[1]).  legion_labor_edges, given the same rows, n, offsets, m, fanout and salt and the scratch as
 * _count left it, writes the kept triples to positions [0, min(K, cap)) and -1 / -1 / -1 to [K, cap).  cap is a capacity, as m is for
 * legion_in_edges: dst_out, src_out (int32[cap]) and eid_out (int64[cap], may be NULL) are defined whole, and both calls may be captured
 * into one graph with no host read between them.  Memory safety does not rest on the content of scratch: a triple whose position falls
 * outside [0, cap) is dropped and the fill is clamped to [0, cap]; with a scratch that _count did not write the output values are
 * unspecified, but nothing outside [0, cap) is written.
 * scratch: device memory, 8-byte aligned, of at least legion_labor_scratch_bytes(m) bytes: one int64 per tile plus one, plus one int64
 * per 256 tiles; -1 for m < 0 or m > LEGION_LABOR_MAX_SLOTS (2^20 tile counts make at most 4 096 second-level sums, the reach of the
 * one-workgroup scan; a caller batches beyond it).  Two calls in flight on different streams need scratch of their own.
 * Both return 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, rows_devptr, offsets_devptr, scratch, count_out,
 * dst_out or src_out; n < 0; n > LEGION_IN_EDGES_MAX_ROWS; m < 0; m > LEGION_LABOR_MAX_SLOTS; fanout < 1; cap < 0; cap > 2^31 - 1;
 * scratch_bytes below legion_labor_scratch_bytes(m).  m == 0: _count writes count_out[0] = 0 and a zero total only.  cap == 0 returns 0
 * and enqueues nothing.
 * Not offered: the importance-sampled variants (LABOR-1, LABOR-*); per-edge importance weights (with LABOR-0 the mean over the kept
 * in-edges is the Hajek estimator); prob=; out-edges (there is no reverse CSR); heterogeneous graphs; the server, the launcher and the
 * wire. */
#define LEGION_LABOR_MAX_SLOTS 1073741824
int64_t legion_labor_scratch_bytes(int64_t m);
int32_t legion_labor_count(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                           const int64_t* offsets_devptr /* int64[n + 1] */, int64_t m, int32_t fanout, int64_t salt,
                           int64_t* count_out /* int64[1] */, void* scratch, int64_t scratch_bytes);
int32_t legion_labor_edges(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                           const int64_t* offsets_devptr /* int64[n + 1] */, int64_t m, int32_t fanout, int64_t salt,
                           const void* scratch /* as legion_labor_count left it */, int64_t scratch_bytes, int64_t cap,
                           int32_t* dst_out /* int32[cap] */, int32_t* src_out /* int32[cap] */, int64_t* eid_out /* int64[cap], or NULL */);
/* Induced subgraphs (DGL's g.subgraph / dgl.node_subgraph: the op behind ClusterGCN's partitions, GraphSAINT's walk-visited vertices and
 * ShaDow-GNN's k-hop neighbourhoods), new in this build; no reference counterpart.  Three pieces: a vertex set as an object of its own,
 * the in-edges of a list of rows whose SOURCE is a member of the set, written with the member's position in the set, and the row
 * pointers of that result.  Orientation, N, rows, the buffers, the stream, capture and the FULL CSR are as for legion_in_edges: a CSR row
 * is the dst side and a column entry the src side.  All buffers are device memory; nothing synchronises with the host.
 *
 * The vertex set.  nodes is int32[k], 0 <= k <= LEGION_NODE_SET_MAX_IDS.  pos(v) = min{ j : nodes[j] == v } for v >= 0; pos(v) = -1 for
 * v < 0 and for a v that does not occur.  Negative entries of nodes are members of nothing.  Ids at or above N are legal: no graph is
 * involved in building the set, and such ids simply never match a column entry.  The set lives in caller-held device memory, 4-byte
 * aligned (at a 16-byte boundary the probes load four keys at once; the results are the same), of at least legion_node_set_bytes(k) bytes: int32 keys[S] then uint32 first[S], 8 S bytes, S the smallest power of two that is
 * at least 256 and at least 2 k (legion_unique_ids' sizing); -1 for k outside [0, LEGION_NODE_SET_MAX_IDS].  It is an open-addressing
 * table: the home slot of v is ((uint32)v * 2654435769u) >> (32 - log2 S), probing is linear and wraps, at most S probes, an empty key is
 * all-ones.
 * legion_node_set_build clears the table on `stream` itself, inserts every non-negative entry (atomicCAS on the key, then atomicMin of the
 * entry's index on first) and writes the number of distinct non-negative values to distinct_out[0] (int32[1]).  Which slot a key lands in
 * depends on the order in which the device takes the entries; pos and the count do not, and nothing else of the table is specified.
 * k == 0 clears, writes 0 and nothing else.  Two sets in flight on different streams need memory of their own.
 * legion_node_set_lookup: local_out[i] = pos(ids[i]) for i in [0, m), ids and local_out int32[m].  v >= 0 is tested before any probe: a
 * dead column entry is -1, the bit pattern of the empty key, and never matches it.  A probe stops at the key, at an empty key, or after
 * S probes; the value read from first is accepted only if it lies in [0, k).  Memory safety does not rest on what the set holds: with a
 * set that _build did not write the values are unspecified but lie in {-1} u [0, k), and nothing outside keys[0 .. S) and first[0 .. S)
 * is read.  k and set_bytes are those of the build.
 * _build returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null nodes_devptr, set or distinct_out; k outside
 * [0, LEGION_NODE_SET_MAX_IDS]; set_bytes below legion_node_set_bytes(k).  _lookup likewise for: a null set, ids_devptr or local_out; k
 * and set_bytes as above; m outside [0, 2^31 - 1].  m == 0 returns 0 and enqueues nothing.
 *
 * The edges.  legion_induced_count / legion_induced_edges take what legion_labor_count / legion_labor_edges take, with set, set_bytes
 * and k in place of fanout and salt.  For slot p in [0, m), rules 1, 2 and 4 of the LABOR contract stand unchanged (the resolution of p
 * to i, j, r, e and src = col[e]; memory safety independent of offsets; kept slots written in slot order, so dst is non-decreasing), and
 *   3. the slot is kept iff it resolved to an entry (e >= 0), src >= 0 and pos(src) lies in [0, k);
 * a kept slot writes (dst = i, src_local = pos(src), eid = e).  rows and the set are independent arguments: the row side need not equal
 * the set (edges from a set into a frontier: ShaDow's and a bipartite block's case).  Parallel entries and self-loops are kept like any
 * other entry; dead entries never are.  _count leaves in scratch the exclusive prefix sums of the kept counts per tile of 1 024 slots
 * and their total K, and writes K to count_out[0] (int64[1]); _edges, given the same rows, n, offsets, m and set and the scratch as
 * _count left it, writes the kept triples to [0, min(K, cap)) and -1 / -1 / -1 to [K, cap).  cap is a capacity as in
 * legion_labor_edges: a triple whose position falls outside [0, cap) is dropped whatever the scratch holds, and the fill is clamped to
 * [0, cap].  scratch: device memory, 8-byte aligned, of at least legion_induced_scratch_bytes(m) bytes, LABOR's formula: one int64 per
 * tile plus one, plus one per 256 tiles; -1 for m outside [0, LEGION_INDUCED_MAX_SLOTS].
 * Both return 0, or -1 -- nothing enqueued, no buffer touched -- for, in this order: a null graph, rows_devptr, offsets_devptr, set,
 * scratch, count_out, dst_out or src_local_out (eid_out may be null); n outside [0, LEGION_IN_EDGES_MAX_ROWS]; m outside
 * [0, LEGION_INDUCED_MAX_SLOTS]; k outside [0, LEGION_NODE_SET_MAX_IDS]; set_bytes below legion_node_set_bytes(k); cap outside
 * [0, 2^31 - 1]; scratch_bytes below legion_induced_scratch_bytes(m).  m == 0: _count writes count_out[0] = 0 and a zero total only.
 * cap == 0 returns 0 and enqueues nothing.
 *
 * The row pointers.  legion_dst_offsets: L = count[0] clamped to [0, cap], read on the device (count: int64[1], device memory);
 * indptr_out[i] = #{ p in [0, L) : dst[p] < i } for i in [0, n], int64[n + 1].  It is a lower-bound search over dst[0 .. L) and nothing
 * else: exact for a non-decreasing dst, which _edges guarantees, and some value in [0, L] otherwise.  No host read: count, edges and
 * offsets can be captured in one graph.  Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null dst_devptr, count_devptr
 * or indptr_out; cap outside [0, 2^31 - 1]; n outside [0, LEGION_IN_EDGES_MAX_ROWS].
 * Not offered: edge_subgraph; out-edges (there is no reverse CSR); khop_in_subgraph as one call; heterogeneous graphs; more than 2^20
 * set members or rows a call (a caller batches); keeping the original ids (nodes[src_local], one gather); the server, the launcher and
 * the wire. */
#define LEGION_NODE_SET_MAX_IDS 1048576
#define LEGION_INDUCED_MAX_SLOTS 1073741824
int64_t legion_node_set_bytes(int32_t k);
int32_t legion_node_set_build(legion_stream_t stream, const int32_t* nodes_devptr /* int32[k] */, int32_t k, void* set, int64_t set_bytes,
                              int32_t* distinct_out /* int32[1] */);
int32_t legion_node_set_lookup(legion_stream_t stream, const void* set /* as legion_node_set_build left it */, int64_t set_bytes, int32_t k,
                               const int32_t* ids_devptr /* int32[m] */, int64_t m, int32_t* local_out /* int32[m] */);
int64_t legion_induced_scratch_bytes(int64_t m);
int32_t legion_induced_count(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                             const int64_t* offsets_devptr /* int64[n + 1] */, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                             int64_t* count_out /* int64[1] */, void* scratch, int64_t scratch_bytes);
int32_t legion_induced_edges(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n,
                             const int64_t* offsets_devptr /* int64[n + 1] */, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                             const void* scratch /* as legion_induced_count left it */, int64_t scratch_bytes, int64_t cap,
                             int32_t* dst_out /* int32[cap] */, int32_t* src_local_out /* int32[cap] */,
                             int64_t* eid_out /* int64[cap], or NULL */);
int32_t legion_dst_offsets(legion_stream_t stream, const int32_t* dst_devptr /* int32[cap] */, int64_t cap,
                           const int64_t* count_devptr /* int64[1] */, int32_t n, int64_t* indptr_out /* int64[n + 1] */);
/* Seed-edge exclusion (DGL's as_edge_prediction_sampler(exclude="self" | "reverse_id"), which runs ExcludeCertainEdges after
 * sample_neighbors), new in this build; no reference counterpart.  Without it a link-prediction model sees the edge it is asked to
 * predict.  Three pieces: the reverse edge id of an edge, a set of edge ids as an object of its own, and the filter that drops the set's
 * members from an edge list.  All buffers are device memory.  Each op is enqueued on `stream`, on the device current at the call; nothing
 * synchronises with the host, and each call may be captured into a graph.  An edge id is a position in col of the FULL CSR, int64: ids
 * pass 2^32, and neither a key nor a hash is ever cut to 32 bits.  A CSR row is the dst side and a column entry the src side, as above.
 *
 * legion_reverse_edge_ids.  N = node_num, E the column entries.  For i in [0, n), e = eids[i]:
 *   1. e < 0 or e >= E: reverse_out[i] = -1 -- no memory is read for e;
 *   2. u = col[e]; u < 0 (a dead entry) or u >= N: reverse_out[i] = -1;
 *   3. v = row(e), the one v with indptr[v] <= e < indptr[v + 1] (legion_find_edges' upper bound); none in [0, N): -1;
 *   4. reverse_out[i] = the LEAST e' in row u (indptr[u] <= e' < indptr[u + 1]) with col[e'] == v; -1 if there is none.
 * So edge e is v <- u and e' is u <- v.  A self-loop maps to the least parallel self-loop of its row, usually itself.  PARALLEL EDGES ALL
 * MAP TO THE FIRST REVERSE EDGE: the k-th of several u -> v is not paired with the k-th of several v -> u, so rev(rev(e)) == e holds only
 * where e is the least of its parallel edges.  For exclusion that is what is wanted of one id per edge; a caller that must exclude every
 * parallel reverse edge excludes by vertex pair, which is not offered.  The result is a function of the graph alone: bit-identical from
 * run to run.  reverse_out is int64[n].
 * via chooses where rule 4 searches; both give the same reverse_out on a graph with sorted rows:
 *   via == 0: a lower-bound search for v of row u of the graph itself.  Needs sorted rows: refused unless
 *             legion_graph_check_rows_sorted has returned 1 for the graph, as legion_negative_sample's exclude & 2 is;
 *   via == 1: a lower-bound search for u of row v of the reverse CSR, returning reid[position].  Reverse rows are sorted by vertex and,
 *             within a vertex, by ascending edge id, so the first match is the least e'.  Needs legion_graph_build_reverse to have
 *             built; works on unsorted rows.  The reverse CSR lives on the device that was current at its build: a via == 1 call is
 *             made with that device current (it is not checked).
 * One kernel: the upper bound over indptr, then the lower bound of the row, four ids per lane with their chains of dependent loads
 * interleaved; rows of up to 2^31 - 1 entries.  Whatever eids holds, nothing outside eids, indptr, col and the reverse CSR is read.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null graph, eids_devptr or reverse_out; n < 0; n > 2^31 - 1; via
 * outside {0, 1}; via == 0 on a graph whose rows have not been checked or are unsorted; via == 1 before the reverse is built.  n == 0
 * returns 0 and enqueues nothing.
 *
 * The set.  eids is int64[k], 0 <= k <= LEGION_EDGE_SET_MAX_IDS (a million seed edges and their reverses).  An id is a member iff it is
 * >= 0 and occurs in eids: negative entries are never inserted and never members, which covers the -1 of "no reverse edge".  Duplicates
 * are fine.  The set lives in caller-held device memory, 8-byte aligned, of at least legion_edge_set_bytes(k) bytes: int64 keys[S], S the
 * smallest power of two that is at least 256 and at least 2 k; -1 for k outside [0, LEGION_EDGE_SET_MAX_IDS].  It is an open-addressing
 * table: the home slot of e is ((uint64)e * 0x9E3779B97F4A7C15) >> (64 - log2 S), probing is linear and wraps, at most S probes, an
 * empty key is all-ones.
 * legion_edge_set_build clears the table on `stream` itself and inserts every non-negative entry by a 64-bit compare-and-swap on the
 * key.  Which slot a key lands in depends on the order in which the device takes the entries; membership does not, and nothing else of
 * the table is specified.  k == 0 clears and nothing else.  Two sets in flight on different streams need memory of their own.
 * legion_edge_set_contains: member_out[i] = 1 if ids[i] is a member, else 0, for i in [0, m); member_out is int32[m].  e >= 0 is tested
 * before any probe; a probe stops at the key, at an empty key, or after S probes.  Whatever the set holds, nothing outside keys[0 .. S)
 * is read.  k and set_bytes are those of the build.
 * _build returns 0, or -1 -- nothing enqueued, no buffer touched -- for: a null eids_devptr or set; k outside
 * [0, LEGION_EDGE_SET_MAX_IDS]; set_bytes below legion_edge_set_bytes(k).  _contains likewise for: a null set, eids_devptr or member_out;
 * k and set_bytes as above; m outside [0, 2^31 - 1].  m == 0 returns 0 and enqueues nothing.
 *
 * The filter.  The input is an edge list dst int32[m], src int32[m], eid int64[m]: the triples of legion_in_edges, legion_labor_edges,
 * legion_induced_edges and the block ops.  Entry p is KEPT iff dst[p] >= 0 and eid[p] is not a member of the set.  So the -1 tail of a
 * capacity call drops out, and a dead entry (src == -1) is kept unless its id is excluded.  The kept entries are written in the order of
 * the list (stable) to dst_out / src_out / eid_out.  legion_edge_filter_count leaves in scratch the exclusive prefix sums of the kept
 * counts per tile of 1 024 entries and their total K, and writes K to count_out[0] (int64[1]); legion_edge_filter_edges, given the same
 * list and set and the scratch as _count left it, writes the kept triples to [0, min(K, cap)) and -1 / -1 / -1 to [K, cap): a capacity as
 * in legion_labor_edges -- a triple whose position falls outside [0, cap) is dropped whatever the scratch holds, and the fill is clamped
 * to [0, cap].  scratch: device memory, 8-byte aligned, of at least legion_edge_filter_scratch_bytes(m) bytes, LABOR's formula; -1 for m
 * outside [0, LEGION_EDGE_FILTER_MAX_EDGES].
 * Both return 0, or -1 -- nothing enqueued, no buffer touched -- for, in this order: a null dst_devptr, src_devptr, eid_devptr, set,
 * scratch, count_out, dst_out or src_out (eid_out may be null); m outside [0, LEGION_EDGE_FILTER_MAX_EDGES]; k outside
 * [0, LEGION_EDGE_SET_MAX_IDS]; set_bytes below legion_edge_set_bytes(k); cap outside [0, 2^31 - 1]; scratch_bytes below
 * legion_edge_filter_scratch_bytes(m); an output that overlaps an input (cap entries against m entries; with cap == 0 or
 * m == 0 there is no byte to share, and nothing overlaps).  m == 0: _count writes
 * count_out[0] = 0 and a zero total only.  cap == 0 returns 0 and enqueues nothing.
 * Not offered: rank-matched pairing of parallel edges (the k-th u -> v with the k-th v -> u); exclusion by vertex pair;
 * exclude="reverse_types" and heterogeneous graphs; the filter inside the pool's hops or the launch group (a consumer of a pool with edge
 * ids calls legion_edge_filter_count / _edges on the batch's arrays); a whole-graph reverse-id map; the server, the launcher and the
 * wire. */
#define LEGION_EDGE_SET_MAX_IDS 2097152
#define LEGION_EDGE_FILTER_MAX_EDGES 1073741824
int32_t legion_reverse_edge_ids(legion_stream_t stream, LegionGraphStorage* graph, const int64_t* eids_devptr /* int64[n] */, int64_t n,
                                int32_t via, int64_t* reverse_out /* int64[n] */);
int64_t legion_edge_set_bytes(int32_t k);
int32_t legion_edge_set_build(legion_stream_t stream, const int64_t* eids_devptr /* int64[k] */, int32_t k, void* set, int64_t set_bytes);
int32_t legion_edge_set_contains(legion_stream_t stream, const void* set /* as legion_edge_set_build left it */, int64_t set_bytes, int32_t k,
                                 const int64_t* eids_devptr /* int64[m] */, int64_t m, int32_t* member_out /* int32[m] */);
int64_t legion_edge_filter_scratch_bytes(int64_t m);
int32_t legion_edge_filter_count(legion_stream_t stream, const int32_t* dst_devptr /* int32[m] */, const int32_t* src_devptr /* int32[m] */,
                                 const int64_t* eid_devptr /* int64[m] */, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                                 int64_t* count_out /* int64[1] */, void* scratch, int64_t scratch_bytes);
int32_t legion_edge_filter_edges(legion_stream_t stream, const int32_t* dst_devptr /* int32[m] */, const int32_t* src_devptr /* int32[m] */,
                                 const int64_t* eid_devptr /* int64[m] */, int64_t m, const void* set, int64_t set_bytes, int32_t k,
                                 const void* scratch /* as legion_edge_filter_count left it */, int64_t scratch_bytes, int64_t cap,
                                 int32_t* dst_out /* int32[cap] */, int32_t* src_out /* int32[cap] */,
                                 int64_t* eid_out /* int64[cap], or NULL */);
/* The k best entries of each row (DGL's dgl.sampling.select_topk, and sample_neighbors(prob=w, replace=False): weighted sampling
 * WITHOUT replacement), new in this build; no reference counterpart.  One selection kernel, the k smallest keys of a row; only the key
 * differs between the modes.  Orientation, N, rows, the buffers, the stream, capture and the FULL CSR are as for legion_in_edges: a CSR
 * row is the dst side and a column entry the src side.  w is float32[E], device memory, aligned with col (the caller's array: the
 * graph's prefix-sum table is not involved); in LEGION_TOPK_SAMPLE it may be NULL, which means every weight is 1.
 *
 * Eligibility and key of an entry e (a position in col, in row v).  A smaller key is better.
 *   LARGEST   eligible iff col[e] >= 0 and w[e] is not NaN;                     K(e) = 0xFFFFFFFF - o
 *   SMALLEST  eligible iff col[e] >= 0 and w[e] is not NaN;                     K(e) = o
 *   SAMPLE    eligible iff col[e] >= 0 and w[e] is finite and > 0 (the rule of  K(e) = the uint64 bit pattern of
 *             legion_graph_set_edge_weights; every live entry when w == NULL);         E(e, salt) / (double) w[e]
 * o is a monotone uint32 of the weight: b = the bits of w[e], -0 taken as +0; o = (b & 0x80000000) ? ~b : (b | 0x80000000).  +-inf are
 * eligible and order as IEEE does.  In SAMPLE the key is a positive finite double, so its bits order as its value.
 * E(e, salt) is an Exp(1) variate (the Efraimidis-Spirakis / exponential-clock key: the k smallest E / w are a weighted sample without
 * replacement), the same to the last bit on the device, in numpy and under g++.  x = splitmix64(key ^ (uint64) e), key =
 * splitmix64((uint64) salt) as LABOR's, then
 *   j = x >> 12;  u = (double)(2 j + 1) * 2^-53                         exact, in (0, 1)
 *   (m, ex) = frexp(u), m in [0.5, 1);  if (m < SQ) { m = 2 m; ex -= 1; }      SQ = 0.7071067811865476
 *   s = (m - 1) / (m + 1);  z = s * s
 *   p = C[10];  for t = 9 .. 0:  p = p * z + C[t]                       C[t] = 1.0 / (2 t + 1), a rounded division of literals
 *   E = -((double) ex * LN2 + (2 s) * p)                                LN2 = 0.6931471805599453
 * with every *, +, / one IEEE double operation rounded on its own (p * z + C[t] is never fused).  0 < E < 37, and E / w is finite for
 * every positive float32, denormals included.
 *
 * legion_row_topk.  For i in [0, n), r = rows[i]: the eligible entries of row r ordered by (K(e), e) ascending -- a tie goes to the
 * smaller position -- are e_0, e_1, ...; c_i = min(k, their number); src_out[i k + j] = col[e_j] and eid_out[i k + j] = e_j for
 * j < c_i, both -1 for j in [c_i, k); count_out[i] = c_i.  src_out is int32[n x k]; eid_out (int64[n x k]) and count_out (int32[n]) may
 * be NULL.  A row id outside [0, N) has no entries, and no memory is read for it.  A row's result depends only on (graph, w, row, k,
 * mode, salt): the same row listed twice gets the same picks, and a fresh salt per batch is the caller's to choose.  Whatever rows holds,
 * nothing outside rows, indptr, col and w is read.
 * scratch: device memory, 4-byte aligned, of at least legion_row_topk_scratch_bytes(n) = 4 (n + 1) bytes (a counter and the list of
 * rows of more than 4 096 entries; -1 for n outside [0, LEGION_IN_EDGES_MAX_ROWS]); the call clears the counter on `stream` itself, and
 * two calls in flight on different streams need scratch of their own.
 * Returns 0, or -1 -- nothing enqueued, no buffer touched -- for, in this order: n < 0; n > LEGION_IN_EDGES_MAX_ROWS; k < 1;
 * k > LEGION_TOPK_MAX_K; a mode outside 0 .. 2; w == NULL outside SAMPLE; a null graph, rows_devptr, src_out or scratch; scratch_bytes
 * below legion_row_topk_scratch_bytes(n).  n == 0 returns 0 and enqueues nothing.
 *
 * legion_topk_keys, the key rule alone: for i in [0, n), e = eids[i]: eligible_out[i] = 1 and key_out[i] = K(e) for an eligible entry;
 * 0 and all-ones for one that is not, and for e outside [0, E), for which nothing is read.  Returns 0, or -1 for: n < 0; n > 2^31 - 1; a
 * mode outside 0 .. 2; w == NULL outside SAMPLE; a null graph, eids_devptr, key_out or eligible_out.  n == 0 enqueues nothing.
 * Not offered: k above 64 (a wave holds the picks, one per lane); the pool's sampling modes (weighted sampling inside BatchGenerate
 * stays with replacement); out-edges; heterogeneous graphs; the server, the launcher and the wire. */
#define LEGION_TOPK_MAX_K 64
#define LEGION_TOPK_LARGEST  0      /* select_topk, ascending=False */
#define LEGION_TOPK_SMALLEST 1      /* select_topk, ascending=True  */
#define LEGION_TOPK_SAMPLE   2      /* sample_neighbors(prob=w, replace=False) */
int64_t legion_row_topk_scratch_bytes(int32_t n);
int32_t legion_row_topk(legion_stream_t stream, LegionGraphStorage* graph, const int32_t* rows_devptr /* int32[n] */, int32_t n, int32_t k,
                        int32_t mode, const float* w_devptr /* float32[E], or NULL in SAMPLE */, int64_t salt,
                        int32_t* src_out /* int32[n x k] */, int64_t* eid_out /* int64[n x k], or NULL */,
                        int32_t* count_out /* int32[n], or NULL */, void* scratch, int64_t scratch_bytes);
int32_t legion_topk_keys(legion_stream_t stream, LegionGraphStorage* graph, const int64_t* eids_devptr /* int64[n] */, int64_t n,
                         int32_t mode, const float* w_devptr /* float32[E], or NULL in SAMPLE */, int64_t salt,
                         uint64_t* key_out /* uint64[n] */, uint8_t* eligible_out /* uint8[n] */);
/* Measurement aid (no reference counterpart): while enabled, FeatureCacheLookup records a HIP event
 * on its own stream before and after the gather launch.  _end returns how many gathers were timed
 * and fills their elapsed ms and op ids; call it after synchronising the stream. */
void legion_pool_profile_begin(LegionMemoryPool* p, int32_t max_ops);
int32_t legion_pool_profile_end(LegionMemoryPool* p, float* out_ms, int32_t* out_op, int32_t cap);

/* Cumulative PCIe / xGMI byte counters of logical GPU dev_id from the driver's gpu_metrics table (the MI355X counterpart
 * of the Intel-PCM PCIe counters that feed CostModel in the paper: SS/engine/server.cu:105-110, SS/engine/monitor.cuh).
 * Returns 1 and fills the two totals, or 0 when the table is missing / has an unknown revision.  Host-only. */
int32_t legion_link_counters(int32_t dev_id, uint64_t* pcie_bytes, uint64_t* xgmi_bytes);
/* The same table in full: PCIe total, xGMI bytes READ and WRITTEN by this GPU in total and per link (8 links; 7 populated
 * on an 8-GPU MI355X node), the table revision that was found (known: 1.8) and the GPU's PCI bus id.  CostModel's second
 * counter (counters[1]) is fed with the xGMI bytes the clique's members READ during the PreSC epoch / 64
 * (SS/engine/server.cu:105-106: the two PCM counters are summed into "transactions of topology", cache.cu:459). */
typedef struct LegionLinkCounters {
    uint64_t pcie_bytes;
    uint64_t xgmi_read_bytes, xgmi_write_bytes;
    uint64_t xgmi_read_bytes_link[8], xgmi_write_bytes_link[8];
    int32_t format_revision, content_revision;
    char pci_bus_id[32];
    int32_t source;              /* 1 rocm_smi_lib's versioned decoder (rsmi_dev_gpu_metrics_info_get), 2 the table parsed by byte offset */
    int32_t reserved;
} LegionLinkCounters;
int32_t legion_link_counters_ex(int32_t dev_id, LegionLinkCounters* out);
/* the same from ONE source (1 / 2 as above; 0 = the library's decoder first, the byte-offset parser second, as _ex does) */
int32_t legion_link_counters_from(int32_t dev_id, int32_t source, LegionLinkCounters* out);
/* 64-byte transactions the gathers of dev_id have so far read from OTHER members' stripes of a striped feature cache
 * (rows read through a peer's pointer x row bytes / 64; enables the row-source statistics like
 * legion_cache_gather_stats).  The computed stand-in for the xGMI counter where the driver's table is unavailable or
 * cannot move (one physical GPU). */
uint64_t legion_cache_peer_transactions(LegionUnifiedCache* c, int32_t dev_id);

/* =====================================================================================
 * 5. Synthetic workload generators (RMAT + counter-hash features); device side.
 * ===================================================================================== */
void legion_synth_rmat_edges(legion_stream_t stream, int32_t scale, int64_t num_edges, uint64_t seed,
                             int32_t* src_out, int32_t* dst_out);
/* same edges with Graph500-style label scrambling (a keyed bijection of [0, 2^scale)); key 0 = none */
void legion_synth_rmat_edges_scrambled(legion_stream_t stream, int32_t scale, int64_t num_edges, uint64_t seed,
                                       int32_t* src_out, int32_t* dst_out, uint64_t scramble_key);
void legion_synth_features(legion_stream_t stream, float* out, int64_t first_row, int64_t num_rows,
                           int32_t dim, uint64_t seed);
void legion_synth_feature_check(legion_stream_t stream, const float* rows, const int32_t* ids,
                                int64_t num_rows, int32_t dim, uint64_t seed,
                                unsigned long long* mismatch_count_devptr);

/* Measurement aid (no reference counterpart): one launch that loads every float of a batch's feature rows and every entry of its
 * two COO arrays and folds them into *acc_devptr -- a trainer-side consumer that really reads its batches
 * (tools/server_throughput.py --consume, bench.py's boundary.consuming_trainer). */
void legion_consume_batch(legion_stream_t stream, const float* feats, int64_t n_floats, const int32_t* src, const int32_t* dst,
                          int64_t n_edges, double* acc_devptr);

/* Spill-over tier: mapped pinned host memory (what the reference uses for the full CSR / feature table,
 * SS/storage/storage_management.cu:106-107,161).  Returns the pointer the GPU dereferences; *host_ptr_out
 * is the host-side address to fill and to pass to legion_host_free. */
void* legion_host_alloc(int64_t num_bytes, void** host_ptr_out);
void legion_host_free(void* host_ptr);

/* One process per GPU: logical GPU d of this process is physical GPU (base + d) % device_count.
 * Call once before creating any object (bench.py passes LOCAL_RANK). */
void legion_set_device_base(int32_t base);
int32_t legion_get_device_base(void);

/* =====================================================================================
 * 6. Tuning.  Every switch that changes how the path runs (never what it computes) lives in ONE
 *    struct.  The library keeps one process-wide copy; it is (re)filled from the LEGION_* environment
 *    variables named below by legion_tuning_from_env(), which the library itself calls whenever a
 *    MemoryPool, a Pipeline or a Server is created -- never inside a launch path.  A host program may
 *    instead fill the struct and call legion_tuning_set(): values set that way are kept (the
 *    environment is then only read again after legion_tuning_from_env() is called explicitly).
 *    No reference counterpart (the reference has compile-time constants only, system_config.cuh).
 *    Not tuning and therefore still plain environment: LEGION_IPC_NAMESPACE, LEGION_IPC_LOCAL,
 *    LEGION_IPC_DEVICE (deployment: which shm names / which GPU a trainer attaches to), and the trainer module's own
 *    LEGION_NO_DIRECT_VIEWS / LEGION_NO_SHM_MIRROR (ipc_service is a separate extension: it reads them once, in initialize()).
 * ===================================================================================== */
typedef struct LegionTuning {
    /* -- sampler ------------------------------------------------------------------------------------------------------------ */
    int32_t lds_small_buckets;   /* LEGION_LDS_SMALL_BUCKETS (0 auto | 8 | 16): hash buckets per lane of pools whose hops have <= 2^19 slots;
                                    auto = 16 where PreSC saw more last-hop edges + earlier nodes than 8 buckets take in one pass */
    int32_t lds_part_wg;         /* LEGION_LDS_PART_WG     (8192): workgroups a sampling launch of the 64/256-bucket classes aims for (picks the
                                    partition tile: 1..8 super tiles) */
    int32_t sample_max_wg;       /* LEGION_SAMPLE_MAX_WG   (4096): workgroup cap of the strided sampler grids */
    int32_t lds_known_cap;       /* LEGION_LDS_KNOWN_CAP   (0 = 2 x an even share): entries per known-node list (tests force the fallback) */
    int32_t lds_claim_cap;       /* LEGION_LDS_CLAIM_CAP   (0 = 2 x an even share): entries per claim list (tests force the fallback) */
    int32_t col_slots;           /* LEGION_COL_SLOTS       (-1 auto): the {neighbour id, feature-cache slot} copy of the column array that
                                    lets the gather skip its node_map lookup (8 B per edge of HBM per GPU): 1 always, 0 never,
                                    -1 when the column array is device memory and the copy fits half of the HBM that is free after the fills, leaving 24 GB */
    /* -- gather ------------------------------------------------------------------------------------------------------------- */
    int32_t gather_rows_per_wg;  /* LEGION_GATHER_ROWS     (0 = by row width): rows per gather workgroup, 16|32|64|128|256 */
    int32_t peer_gather;         /* LEGION_PEER_GATHER=direct|bulk -> 0|1: rows of OTHER members' stripes of a striped feature cache are
                                    read by direct peer loads, or pushed by their owners in bulk (pipeline.hip) */
    /* -- launch groups ------------------------------------------------------------------------------------------------------- */
    int32_t arena_scatter_mb;    /* LEGION_ARENA_SCATTER_MB (2; 0 = plain allocations): lane arenas are built from physical chunks of this many MB
                                    mapped in shuffled order (HIP virtual memory management): the gathers write a group's rows all over the
                                    HBM instead of into one contiguous range (0.87 instead of 0.80 of the peak) */
    int32_t weave_priority;      /* LEGION_WEAVE_PRIORITY  (-1): priority of the light stream (heads of the next group): -1 low, 0 equal, 1 high */
    int32_t markers;             /* LEGION_MARKERS         (1): roctx ranges around ops and launch groups (visible to rocprofv3 --marker-trace) */
    /* -- Runner (server side of the boundary) -------------------------------------------------------------------------------- */
    int32_t runner_graph;        /* LEGION_RUNNER_GRAPH    (1): Runner serves from lane groups + hipGraph; 0 = operator by operator */
    int32_t runner_lanes;        /* LEGION_RUNNER_LANES    (0 = min(512, 524288 / batch)): lanes of a Runner group */
    int32_t runner_slots;        /* LEGION_RUNNER_SLOTS    (3): launch groups the Runner keeps in flight (2..4): one being handed over, one
                                    running, one queued behind it */
    int32_t runner_handover;     /* LEGION_RUNNER_HANDOVER=auto|gather -> 0|1: how the Runner's batches reach a trainer.  auto: a trainer end that
                                    opened the lane arena gets a batch as VIEWS of its lane (no per-batch GPU work), any other gets its rows
                                    gathered straight into the pipe slot by one launch per batch.  gather: that for every trainer end */
    int32_t runner_ho_stream;    /* LEGION_RUNNER_HO_STREAM (2): hand-over streams of the gather hand-over: 0 the sampler's, 1 one shared, 2 one per pipe slot */
    int32_t runner_spin_us;      /* LEGION_RUNNER_SPIN_US  (-1 auto): how long the Runner polls (a trainer's semaphore, a group's completion) before it
                                    blocks.  auto: 20 us when batches are handed over as views (a group completes every few ms: the host
                                    sleeps in between), polling only with the gather hand-over (per-batch latency is the rate there) */
    int32_t runner_overflow;     /* LEGION_RUNNER_OVERFLOW (1): a batch with more rows than 1.2 x the PreSC maximum (the lanes' feature buffers) still goes
                                    out whole: views from one of two num_ids-row overflow buffers inside the arena, the other hand-overs into pipe-slot
                                    buffers of num_ids rows; 0 = the rule everywhere: a views server stops there, the slab path truncates with a warning */
    int32_t runner_stats;        /* LEGION_RUNNER_STATS    (0): print where a hand-over's time went at Finalize */
    int32_t shm_mirror;          /* LEGION_NO_SHM_MIRROR unset -> 1: counters also go to a host-visible mirror (no D2H copy per batch) */
    /* -- set-up -------------------------------------------------------------------------------------------------------------- */
    int32_t table_placement;     /* LEGION_TABLE_PLACEMENT=hbm|pinned -> 0|1: where the server puts the full CSR / feature table */
    int32_t hotness_reduce;      /* LEGION_HOTNESS_REDUCE=auto|p2p|rccl -> -1|0|1: the clique sum of the access counters: rccl = all-reduce
                                    over the server's distinct physical GPUs, p2p = the reference's leader loop over peer pointers
                                    (SS/cache/cache.cu:408-411); auto = rccl when the members sit on distinct physical GPUs, p2p if that fails */
    int32_t link_counters;       /* LEGION_LINK_COUNTERS=v2|measured|smi|"a,b" -> 0|1|2|3: what feeds CostModel's counters */
    uint64_t link_counter_values[2];   /* the injected pair of LEGION_LINK_COUNTERS="a,b" */
} LegionTuning;
void legion_tuning_from_env(void);
void legion_tuning_get(LegionTuning* out);
void legion_tuning_set(const LegionTuning* in);

/* library / device info */
const char* legion_version(void);
int32_t legion_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* LEGION_HIP_H */
