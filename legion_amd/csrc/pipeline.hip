// pipeline.hip -- groups of mini-batches in flight on one GPU, each group replayed as one hipGraph.
//
// The reference's GPURunner (SS/engine/server.cu:302-332) issues ~16 launches per batch from the
// host, blocks on three 64-byte read-backs per hop, and keeps INTERBATCH_CON = 2 output slots so
// the trainer can consume batch i while batch i+1 is produced.  On MI355X one mini-batch is a chain
// of short, latency-bound kernels (3-8 us each at B = 1024) that cannot fill 256 CUs, ~16 eager
// launches cost more host time than the kernels take, and kernels of different HIP streams overlap
// only two at a time on this part (measured).  So:
//   * a GROUP of G independent mini-batches (lanes) is served by every launch: each kernel runs with
//     grid.y = G and lane g works on the buffers of pool g (LanePtrs).  The per-kernel latency floor
//     and launch cost are paid once per group, and the HBM-bound gather sees G times the rows;
//   * the whole op list of a group is captured once per (slot, mode) into a hipGraph; nothing in it
//     depends on host-side values: sizes (including the clamped last batch) are computed on the
//     device and the batch index lives in iter_state on the device, advanced by the last kernel;
//   * `slots` groups are in flight (default 2): while the consumer reads slot s, slot s+1 runs;
//   * weave (use_graph bit 4, what bench.py and the Runner use): a group is cut where its character changes -- the
//     HEAD (seeds + every hop but the last) of group k+1 runs on a low-priority stream under the heavy kernels of group k
//     (see phases_of).  The plain two-stream split (every sampler on one stream, every gather on another, with CU masks and
//     priorities) was measured against it in rounds 2-4 and removed in round 5: DESIGN_HISTORY.md 4.5.
#include "ipc_wire.h"
#include "legion_core.h"

#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cstring>
#include <map>
#include <tuple>


struct Slot {
    std::vector<MemoryPool*> pools;           // G lanes
    LegionLaneGroup* group = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t sampled = nullptr;             // weave: the group's head has finished
    bool busy = false;
    std::map<std::tuple<int32_t, int32_t, int32_t, int32_t>, hipGraphExec_t> exec;   // key: (phase, mode, active lanes, batch_size)
    int32_t* d_iter = nullptr;                // device {next counter0, stride}
    int32_t* h_iter = nullptr;                // pinned staging
    int32_t next_iter = -1;                   // what d_iter[0] will hold once the slot is idle
    int32_t prof_pairs = 0;                   // timed gathers of the group in flight
};

// peer_gather = bulk (lg::BulkLists, kernels_gather.hip): per pipeline slot this GPU's request lists, and what it knows of
// the other members of its clique -- their lane arenas and their lists, as pointers this process can dereference
struct BulkPeer {
    char* arena = nullptr;
    bool mapped_chunks = false;                  // arena mapped from another process's file descriptors (unmapped at destroy)
    std::vector<lg::BulkLists> lists;            // [slot], pointers into the peer's memory
};
struct BulkState {
    int32_t Kg = 1, member = 0;
    int64_t cap = 0;
    std::vector<void*> alloc;                    // [slot] one exportable allocation: cnt | fidx | dst
    std::vector<lg::BulkLists> mine;             // [slot]
    std::vector<BulkPeer> peers;                 // [Kg]
    std::vector<hipStream_t> owner_streams;      // [Kg] in-process pull: a stream on each owner's device for THIS requester's pushes
    int32_t served_tag = -1;                     // >= 0: this arena's chunks are served on wire_bulk_socket_name(pid, tag)
};

struct LegionPipeline {
    GraphStorage* graph;
    FeatureStorage* feature;
    LegionUnifiedCache* cache_handle;
    int32_t dev_id, batch_size, hop_num, group_size, slots_n;
    std::vector<int32_t> fanout;
    std::vector<Slot> slots;
    bool use_graph;
    bool overlap = false;   // let kernels of different slots run concurrently (default: chained)
    bool weave = false;     // head of group k+1 on a second stream under the heavy kernels of group k (see phases_of)
    bool gathers = true;        // weave: false = the REST phase stops before the gathers (legion_pipeline_set_gathers)
    bool sample_only = false;   // only the sampler phase runs here; the owner gathers each lane itself (GPURunner: straight
                                // into a trainer-visible pipe slot)
    hipStream_t sample_stream = nullptr;      // weave: the light stream
    int32_t rr = 0;
    int32_t last_slot = -1;
    bool profiling = false;
    std::map<int32_t, double> prof_ms;        // op id -> summed elapsed ms of its gather launches
    std::map<int32_t, int64_t> prof_cnt;
    PoolArena arena;                          // use_graph bit 5: the lanes' trainer-visible arrays live in ONE exportable allocation
    BulkState* bulk = nullptr;
    PrivateBlock* priv = nullptr;             // the block of shuffled chunks the lanes' private arrays were carved from (arena pipelines)
    bool arena_borrowed = false;              // the arena belongs to the caller (legion_pipeline_bulk_enable_shared)
    int64_t feature_rows = 0;
    int32_t feature_out_dtype = LEGION_FEATURE_F32;      // of every lane (legion_pool_set_feature_out_dtype)
};

// caller_arena: the lanes' trainer-visible arrays are carved from an arena the CALLER owns (GPURunner's lane arena), or null
LegionPipeline* lg_pipeline_create(LegionGraphStorage* graph, LegionFeatureStorage* feature, LegionUnifiedCache* cache, int32_t dev_id,
                                   int32_t batch_size, const int32_t* fanout, int32_t hop_num, int32_t group_size, int32_t slots,
                                   int64_t feature_rows, int32_t use_graph, int32_t feature_out_dtype, PoolArena* caller_arena)
{
    if (!graph || !feature || !cache) { printf("invalid storage ptr\n"); return nullptr; }
    if (feature_out_dtype != LEGION_FEATURE_F32 && feature_out_dtype != LEGION_FEATURE_BF16) {
        printf("legion_hip: unknown feature output dtype %d\n", feature_out_dtype);
        return nullptr;
    }
    LegionPipeline* p = new LegionPipeline();
    p->feature_out_dtype = feature_out_dtype;
    p->graph = reinterpret_cast<GraphStorage*>(graph);
    p->feature = reinterpret_cast<FeatureStorage*>(feature);
    p->cache_handle = cache;
    p->dev_id = dev_id;
    p->batch_size = batch_size;
    p->hop_num = hop_num;
    p->fanout.assign(fanout, fanout + hop_num);
    p->group_size = group_size < 1 ? 1 : group_size;
    p->slots_n = slots < 1 ? 1 : slots;
    p->use_graph = (use_graph & 1) != 0;
    p->overlap = (use_graph & 2) != 0;
    p->sample_only = (use_graph & 8) != 0;
    p->weave = (use_graph & 16) != 0;
    if (p->sample_only) p->weave = false;
    SetGPUDevice(dev_id);
    lg::tuning_refresh();
    if (p->weave) {
        // the light stream (heads of the next group) runs at LOW priority: its dozen small kernels have the whole rest of the
        // current group (1.6 ms for 0.2 ms of work) to finish, and at equal priority their workgroups take slots from the
        // dominant gather whenever both have some ready (measured: 5.11-5.12 -> 5.21-5.23 G edges/s at the headline)
        const int wp = lg::tuning().weave_priority;
        int lo = 0, hi = 0;                                  // hi is the numerically lowest = highest priority
        HIP_CALL(hipDeviceGetStreamPriorityRange(&lo, &hi));
        if (wp == 0) HIP_CALL(hipStreamCreateWithFlags(&p->sample_stream, hipStreamNonBlocking))
        else HIP_CALL(hipStreamCreateWithPriority(&p->sample_stream, hipStreamNonBlocking, wp > 0 ? hi : lo));
    }
    p->slots.resize(p->slots_n);
    p->feature_rows = feature_rows;
    const int32_t D = p->feature->GetFloatFeatureLen();
    const PoolShape shape = pool_shape(batch_size, fanout, hop_num);
    PoolSource source;
    source.arena = caller_arena;
    if ((use_graph & 32) != 0) {       // one arena for every lane (peer_gather = bulk: the owners push rows into it)
        p->arena.bytes = pool_visible_bytes(batch_size, shape.num_ids, feature_rows, D, feature_out_dtype) * p->group_size * p->slots_n;
        // The arena is built from shuffled physical chunks (storage.hip d_alloc_scattered; LegionTuning.arena_scatter_mb = 0: one plain
        // allocation).  use_graph bit 6: it must be reachable from another process or GPU (peer_gather = bulk: owners push rows into
        // it) -- then its chunks are created exportable, other GPUs of this process are granted access when they are linked
        // (legion_pipeline_bulk_link) and other processes map them from file descriptors (legion_pipeline_bulk_export / _import).
        // (Round 4 kept such arenas plain: hipIpcGetMemHandle cannot export chunked memory.)
        const int32_t chunk_mb = lg::tuning().arena_scatter_mb;
        p->arena.base = (char*)(chunk_mb <= 0 ? d_alloc_space(p->arena.bytes)
                                              : ((use_graph & 64) != 0 ? d_alloc_scattered_exportable(p->arena.bytes, std::max(chunk_mb, 16))
                                                                       : d_alloc_scattered(p->arena.bytes, chunk_mb)));
        source.arena = &p->arena;
    }
    // what PreSC saw of the largest hop decides the small class's bucket count (8 or 16, sample_plan.h)
    if (p->cache_handle != nullptr) {       // (the handle boxes the UnifiedCache as its first member, cache.hip)
        int32_t last_hop[2] = {0, 0};
        reinterpret_cast<UnifiedCache*>(p->cache_handle)->LastHopMax(dev_id, last_hop);
        source.claims_hint[0] = last_hop[0];
        source.claims_hint[1] = last_hop[1];
    }
    // Arena pipelines (own arena or the caller's -- the server's) also carve their lanes' PRIVATE arrays from one block of shuffled
    // chunks (storage.hip): per lane what its plan adds up to (pool_plan.h) plus 64 KiB, and 8 MiB on top.  Behind each slot's lanes
    // the block also holds the slot's copy of their descriptors and its iteration state.
    const int64_t lane_private = shape.over_limit ? 0 : lg_pool_private_plan(shape, source).sum;      // (over the limit: the first pool says so and exits)
    if (source.arena != nullptr && lg::tuning().arena_scatter_mb > 0) {
        p->priv = lg_private_block_create((lane_private + (64 << 10)) * p->group_size * p->slots_n + ((int64_t)8 << 20), lg::tuning().arena_scatter_mb);
        source.priv = p->priv;
    }
    for (Slot& sl : p->slots) {
        std::vector<LegionMemoryPool*> handles;
        for (int32_t g = 0; g < p->group_size; g++) {
            const int64_t before = p->priv ? p->priv->used : 0;
            MemoryPool* mp = lg_pool_create(dev_id, p->feature->TotalNodeNum(), batch_size, fanout, hop_num, D, 1, source);
            if (p->priv && p->priv->used - before != lane_private) {      // the plan and the allocations are one list, or nothing runs
                printf("legion_hip: a lane took %lld bytes of the private block, its plan says %lld\n", (long long)(p->priv->used - before),
                       (long long)lane_private);
                exit(EXIT_FAILURE);
            }
            LegionMemoryPool* h = reinterpret_cast<LegionMemoryPool*>(mp);
            legion_pool_set_feature_out_dtype(h, feature_out_dtype);
            if (feature_rows > 0) legion_pool_alloc_features(h, feature_rows);
            handles.push_back(h);
            sl.pools.push_back(mp);
        }
        sl.group = lg_group_create(handles.data(), p->group_size, p->priv);
        sl.d_iter = (int32_t*)lg_private_take(p->priv, 2 * sizeof(int32_t));
        HIP_CALL(hipMemset(sl.d_iter, 0, 2 * sizeof(int32_t)));
        HIP_CALL(hipHostMalloc((void**)&sl.h_iter, 2 * sizeof(int32_t), hipHostMallocDefault));
        // chained slots share one in-order stream (back-to-back graph launches, no event round trip);
        // overlapping slots get a stream each
        if (p->overlap || &sl == &p->slots[0])
            HIP_CALL(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking))
        else
            sl.stream = p->slots[0].stream;
        HIP_CALL(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        HIP_CALL(hipEventCreateWithFlags(&sl.sampled, hipEventDisableTiming));
    }
    return p;
}

extern "C" LegionPipeline* legion_pipeline_create_ex(LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                                     LegionUnifiedCache* cache, int32_t dev_id, int32_t batch_size,
                                                     const int32_t* fanout, int32_t hop_num, int32_t group_size,
                                                     int32_t slots, int64_t feature_rows, int32_t use_graph, int32_t feature_out_dtype)
{
    return lg_pipeline_create(graph, feature, cache, dev_id, batch_size, fanout, hop_num, group_size, slots, feature_rows, use_graph,
                              feature_out_dtype, nullptr);
}

extern "C" LegionPipeline* legion_pipeline_create(LegionGraphStorage* graph, LegionFeatureStorage* feature,
                                                  LegionUnifiedCache* cache, int32_t dev_id, int32_t batch_size,
                                                  const int32_t* fanout, int32_t hop_num, int32_t group_size,
                                                  int32_t slots, int64_t feature_rows, int32_t use_graph)
{
    return legion_pipeline_create_ex(graph, feature, cache, dev_id, batch_size, fanout, hop_num, group_size, slots, feature_rows,
                                     use_graph, LEGION_FEATURE_F32);
}

// Every lane of every slot takes the mode with one field changed (legion_pool_set_*), all or none: refused once any lane has sampled
// (a captured graph never mixes modes) or where any lane's pool refuses.  Each slot's copy of its lanes' descriptors is written again
// before anything is captured (only edge_ids changes a descriptor: a refresh with unchanged epochs copies nothing).  All three leave
// the pipeline's GPU as the calling thread's current device (before, legion_pipeline_set_sample_replace did not)
static int32_t pipeline_set_mode_field(LegionPipeline* p, int32_t SampleMode::*field, int32_t value)
{
    if (!p) return -1;
    auto each_pool = [&](bool check_only) {
        for (Slot& sl : p->slots)
            for (MemoryPool* mp : sl.pools) {
                SampleMode mode = mp->mode;
                mode.*field = value;
                if (!lg_pool_try_set_mode(mp, mode, check_only)) return false;
            }
        return true;
    };
    if (!each_pool(true)) return -1;
    SetGPUDevice(p->dev_id);
    if (!each_pool(false)) return -1;
    for (Slot& sl : p->slots) legion_group_refresh(sl.group);
    return 0;
}

extern "C" int32_t legion_pipeline_set_sample_replace(LegionPipeline* p, int32_t replace) { return pipeline_set_mode_field(p, &SampleMode::replace, replace); }
extern "C" int32_t legion_pipeline_set_edge_ids(LegionPipeline* p, int32_t on) { return pipeline_set_mode_field(p, &SampleMode::edge_ids, on); }
extern "C" int32_t legion_pipeline_set_sample_weighted(LegionPipeline* p, int32_t on) { return pipeline_set_mode_field(p, &SampleMode::weighted, on); }

static void slot_wait(LegionPipeline* p, Slot& sl)
{
    if (!sl.busy) return;
    HIP_CALL(hipEventSynchronize(sl.done));
    sl.busy = false;
    if (p->profiling) {                         // collect the HIP-event times of the finished group
        MemoryPool* mp = sl.pools[0];
        for (int32_t i = 0; i < sl.prof_pairs; i++) {
            float ms = 0.f;
            HIP_CALL(hipEventElapsedTime(&ms, mp->prof_events[2 * i], mp->prof_events[2 * i + 1]));
            p->prof_ms[mp->prof_op[i]] += ms;
            p->prof_cnt[mp->prof_op[i]] += 1;
        }
    }
    sl.prof_pairs = 0;
}

// The hipGraph of one phase of a group on a slot, captured on first use.  Nothing in it depends on host-side values: the
// iteration lives in sl.d_iter on the device (the group's iter_state must be set), sizes are computed by the kernels.
static hipGraphExec_t graph_of(LegionPipeline* p, Slot& sl, hipStream_t strm, int32_t phase, int32_t mode, int32_t n_active,
                               int32_t batch_size)
{
    // (a tuple, not packed bit fields: groups have up to 512 lanes, and (mode m, 256 + k lanes) must not meet (mode m + 1, k lanes))
    const auto key = std::make_tuple(phase, mode, n_active, batch_size);
    auto it = sl.exec.find(key);
    if (it == sl.exec.end()) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_CALL(hipStreamSynchronize(strm));
        HIP_CALL(hipStreamBeginCapture(strm, hipStreamCaptureModeThreadLocal));
        legion_enqueue_group_phase(strm, reinterpret_cast<LegionGraphStorage*>(p->graph), reinterpret_cast<LegionFeatureStorage*>(p->feature),
                                   p->cache_handle, sl.group, n_active, batch_size, 0, p->dev_id, mode, p->fanout.data(),
                                   p->hop_num, phase);
        HIP_CALL(hipStreamEndCapture(strm, &graph));
        HIP_CALL(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        HIP_CALL(hipGraphDestroy(graph));
        it = sl.exec.emplace(key, exec).first;
    }
    return it->second;
}

// A batch larger than the lanes were created for cannot be served: shrinking it silently would drop part of a validation
// or test set (their batches are sized from a raw 512, SS/engine/ipc_service.cu:91-115, whatever the training batch is)
// while the schedule's step counts stay the same.  The owner must size the pipeline for the largest batch of any mode
// (GPURunner::Initialize does); anything else is a bug and ends the process like every other error here.
static int32_t checked_batch_size(const LegionPipeline* p, int32_t batch_size)
{
    if (batch_size < 1) return p->batch_size;            // "the pipeline's own"
    if (batch_size > p->batch_size) {
        printf("legion_hip: batch size %d exceeds the %d the pipeline's lanes were created for\n", batch_size, p->batch_size);
        fflush(stdout);
        exit(EXIT_FAILURE);
    }
    return batch_size;
}

// Which phases (batch_ops.h) a group runs on a slot, in order, and on which stream.
// Weave: the group is cut where its character changes.  HEAD (seeds + every hop but the last: a dozen small,
// latency-bound kernels that cannot fill the chip) runs on the light stream Y; REST (the last hop -- scattered
// atomics at ~2 TB/s of sector traffic -- and every gather) runs on the heavy stream X:
//     X:  rest(k)                | rest(k+1)                 | ...
//     Y:      head(k+1)          |      head(k+2)            |
// The head of the next group hides under the current group's heavy kernels, which lose nothing measurable to it
// (the dominant gather keeps 0.78 of the HBM peak); the two heavy kinds of traffic never share the machine, which
// is what costs the plain two-stream split (sampler || gathers) a quarter of the gather's bandwidth.
// Measured (RMAT-26, B = 1024, 256 lanes): 4.25-4.31 G edges/s against 4.06-4.15 G on one stream.  Running the
// last hop's compaction kernels on Y beside the early gathers as well was measured too: no gain, gather at 0.75.
struct SlotPhases {
    int32_t n;
    struct { hipStream_t stream; int32_t phase; } at[2];
};
static SlotPhases phases_of(const LegionPipeline* p, const Slot& sl)
{
    if (p->weave) return {2, {{p->sample_stream, LG_PHASE_HEAD}, {sl.stream, p->gathers ? LG_PHASE_REST : LG_PHASE_REST_SAMPLE}}};
    return {1, {{sl.stream, p->sample_only ? LG_PHASE_SAMPLE : LG_PHASE_ALL}}};
}

// The next slot (round robin), idle -- this waits for its previous group, which must have been consumed -- with lane g set to
// batch counter0 + g of `mode`
static int32_t acquire_slot(LegionPipeline* p, int32_t counter0, int32_t mode)
{
    const int32_t si = p->rr;
    p->rr = (p->rr + 1) % p->slots_n;
    Slot& sl = p->slots[si];
    slot_wait(p, sl);
    for (int32_t g = 0; g < p->group_size; g++) {
        sl.pools[g]->SetCurrentMode(mode);
        sl.pools[g]->SetIter(counter0 + g);
    }
    return si;
}

// Captures and instantiates, on EVERY slot, the graph(s) a later submit of (mode, n_active, batch_size) will replay, without
// launching anything.  A server calls this for every group shape of its schedule before it starts serving: stream capture
// and graph instantiation then never run beside another thread's HIP calls (GPURunner's poster polls events; a capture
// concurrent with hipEventQuery on the same stream crashed inside the runtime about once in thirty starts, ROCm 7.2).
extern "C" void legion_pipeline_prepare(LegionPipeline* p, int32_t mode, int32_t n_active, int32_t batch_size)
{
    if (!p || !p->use_graph) return;
    if (n_active < 1 || n_active > p->group_size) n_active = p->group_size;
    batch_size = checked_batch_size(p, batch_size);
    SetGPUDevice(p->dev_id);
    for (Slot& sl : p->slots) {
        slot_wait(p, sl);
        legion_group_set_iter_state(sl.group, sl.d_iter);
        const SlotPhases ph = phases_of(p, sl);
        for (int32_t i = 0; i < ph.n; i++) (void)graph_of(p, sl, ph.at[i].stream, ph.at[i].phase, mode, n_active, batch_size);
    }
}

// Enqueues the group of batches counter0 .. counter0 + G - 1 of `mode` on the next slot (round robin)
// and returns the slot index.  The slot's previous group must have been consumed: this call waits
// for its completion first.
extern "C" int32_t legion_pipeline_submit(LegionPipeline* p, int32_t counter0, int32_t mode)
{
    return legion_pipeline_submit_n(p, counter0, mode, p ? p->group_size : 0);
}
extern "C" int32_t legion_pipeline_submit_n(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active)
{
    return legion_pipeline_submit_ex(p, counter0, mode, n_active, p ? p->batch_size : 0);
}
extern "C" legion_stream_t legion_pipeline_stream(LegionPipeline* p) { return p ? (legion_stream_t)p->slots[0].stream : nullptr; }
// (GPURunner) the event recorded behind the last submitted group of a slot: another stream may wait for it
extern "C" void* legion_pipeline_slot_done_event(LegionPipeline* p, int32_t slot)
{
    return (p && slot >= 0 && slot < p->slots_n) ? (void*)p->slots[slot].done : nullptr;
}

// Same with only the first n_active lanes of the group working (the tail of a run whose length is
// not a multiple of the group size) and an explicit batch size (validation / test batches differ from
// training batches, SS/engine/ipc_service.cu:91-115; never larger than the pools were created for).
extern "C" int32_t legion_pipeline_submit_ex(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size)
{
    if (!p) { printf("invalid pipeline ptr\n"); return -1; }
    if (n_active < 1 || n_active > p->group_size) n_active = p->group_size;
    batch_size = checked_batch_size(p, batch_size);
    SetGPUDevice(p->dev_id);
    lg::Range mark("group slot=%d first=%d lanes=%d mode=%d B=%d", p->rr, counter0, n_active, mode, batch_size);
    const int32_t si = acquire_slot(p, counter0, mode);
    Slot& sl = p->slots[si];
    sl.pools[0]->prof_used = 0;
    // Chain the slots: this group starts on the GPU when the previously submitted one has finished.
    // The launch (and its host latency) still happens while that group runs, but kernels of different
    // groups never share the machine -- on this part two streams' kernels mostly take turns anyway,
    // and a gather that runs alone streams at ~73% of HBM peak instead of ~52%.
    // (chained slots share one stream, so the order is the stream's own)
    p->last_slot = si;
    const SlotPhases ph = phases_of(p, sl);
    const bool eager = !p->use_graph || p->profiling;            // HIP cannot time events recorded by graph nodes
    legion_group_set_iter_state(sl.group, eager ? nullptr : sl.d_iter);      // eager: iteration by value
    if (!eager && sl.next_iter != counter0) {                    // (re)position the device-resident iteration
        sl.h_iter[0] = counter0;
        sl.h_iter[1] = p->group_size * p->slots_n;
        HIP_CALL(hipMemcpyAsync(sl.d_iter, sl.h_iter, 2 * sizeof(int32_t), hipMemcpyHostToDevice, ph.at[0].stream));
    }
    for (int32_t i = 0; i < ph.n; i++) {
        const hipStream_t strm = ph.at[i].stream;
        if (i > 0 && strm != ph.at[i - 1].stream) {              // another stream: it starts behind the phase before
            HIP_CALL(hipEventRecord(sl.sampled, ph.at[i - 1].stream));
            HIP_CALL(hipStreamWaitEvent(strm, sl.sampled, 0));
        }
        if (eager)
            legion_enqueue_group_phase(strm, reinterpret_cast<LegionGraphStorage*>(p->graph), reinterpret_cast<LegionFeatureStorage*>(p->feature),
                                       p->cache_handle, sl.group, n_active, batch_size, counter0, p->dev_id, mode, p->fanout.data(),
                                       p->hop_num, ph.at[i].phase);
        else
            HIP_CALL(hipGraphLaunch(graph_of(p, sl, strm, ph.at[i].phase, mode, n_active, batch_size), strm));
    }
    // what the last kernel of a replay leaves in d_iter[0] (a partial group breaks the regular stride; eager launches leave it alone)
    sl.next_iter = (!eager && n_active == p->group_size) ? counter0 + p->group_size * p->slots_n : -1;
    if (eager) sl.prof_pairs = sl.pools[0]->prof_used;
    HIP_CALL(hipEventRecord(sl.done, sl.stream));
    sl.busy = true;
    return si;
}

// Diagnostics: the last op's gather of the group sitting in `slot`, launched `repeats` more times over the lanes as they stand
// (a caller may have rewritten the lanes' ids in between: bench.py's cold-row figure), each launch between two HIP events on the
// slot's stream; ms_each[i] = its duration.  Returns the launches timed.
extern "C" int32_t legion_pipeline_regather_last(LegionPipeline* p, int32_t slot, int32_t n_active, int32_t repeats, double* ms_each)
{
    if (!p || slot < 0 || slot >= p->slots_n || repeats < 1 || !ms_each) return 0;
    SetGPUDevice(p->dev_id);
    Slot& sl = p->slots[slot];
    slot_wait(p, sl);
    HIP_CALL(hipDeviceSynchronize());
    const bool was_on = sl.pools[0]->prof_on;
    sl.pools[0]->prof_on = false;                 // (this launch is timed here, not by the pool's op profile)
    hipEvent_t a, b;
    HIP_CALL(hipEventCreate(&a));
    HIP_CALL(hipEventCreate(&b));
    for (int32_t i = 0; i < repeats; i++) {
        HIP_CALL(hipEventRecord(a, sl.stream));
        legion_enqueue_group_last_gather(sl.stream, p->cache_handle, sl.group, n_active, p->dev_id, p->hop_num);
        HIP_CALL(hipEventRecord(b, sl.stream));
        HIP_CALL(hipEventSynchronize(b));
        float ms = 0.f;
        HIP_CALL(hipEventElapsedTime(&ms, a, b));
        ms_each[i] = ms;
    }
    HIP_CALL(hipEventDestroy(a));
    HIP_CALL(hipEventDestroy(b));
    sl.pools[0]->prof_on = was_on;
    return repeats;
}

extern "C" void legion_pipeline_wait(LegionPipeline* p, int32_t slot)
{
    if (!p) return;
    SetGPUDevice(p->dev_id);
    if (slot >= 0) { slot_wait(p, p->slots[slot % p->slots_n]); return; }
    for (Slot& sl : p->slots) slot_wait(p, sl);
}

// The same for a host thread that has nothing else to do until the group is complete (GPURunner handing batches over as views: a
// group completes every few ms): poll for at most spin_us microseconds, then SLEEP between polls (200 us naps: a completion is
// noticed at most that late, which delays a hand-over that has two more groups queued behind it, not the GPU).
// (hipEventSynchronize on an event created with hipEventBlockingSync was tried first: on this runtime the waiting thread and
// one of the runtime's own threads then burn 0.6 of a core each -- 1.25 cores per GPU at B = 8000 against 0.27 at B = 1024, where
// the thread mostly sleeps on the trainer's semaphore instead.)
extern "C" void legion_pipeline_wait_sleeping(LegionPipeline* p, int32_t slot, int32_t spin_us)
{
    if (!p) return;
    SetGPUDevice(p->dev_id);
    Slot& sl = p->slots[slot % p->slots_n];
    if (sl.busy) {
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t q = hipEventQuery(sl.done);
        while (q == hipErrorNotReady && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < spin_us) q = hipEventQuery(sl.done);
        while (q == hipErrorNotReady) {
            std::this_thread::sleep_for(std::chrono::microseconds(200));
            q = hipEventQuery(sl.done);
        }
        (void)hipGetLastError();
        if (q != hipSuccess) HIP_CALL(q);
    }
    slot_wait(p, sl);       // (complete by now: returns at once, collects the profile)
}

extern "C" LegionMemoryPool* legion_pipeline_pool(LegionPipeline* p, int32_t slot, int32_t lane)
{
    if (!p) return nullptr;
    return reinterpret_cast<LegionMemoryPool*>(p->slots[slot % p->slots_n].pools[lane % p->group_size]);
}

// weave arrangement: whether the groups submitted (and the graphs prepared) from now on include their gathers.  GPURunner
// switches them off when the trainer end it serves gets its rows gathered batch by batch straight into a pipe slot.
extern "C" void legion_pipeline_set_gathers(LegionPipeline* p, int32_t on) { if (p) p->gathers = on != 0; }

extern "C" void legion_pipeline_destroy(LegionPipeline* p)
{
    if (!p) return;
    SetGPUDevice(p->dev_id);
    if (p->sample_stream) HIP_CALL(hipStreamSynchronize(p->sample_stream));
    for (Slot& sl : p->slots) {
        slot_wait(p, sl);
        HIP_CALL(hipStreamSynchronize(sl.stream));
        for (auto& kv : sl.exec) HIP_CALL(hipGraphExecDestroy(kv.second));
        legion_group_destroy(sl.group);
        if (p->priv == nullptr) d_free_space(sl.d_iter);
        HIP_CALL(hipHostFree(sl.h_iter));
        for (MemoryPool* mp : sl.pools) legion_pool_destroy(reinterpret_cast<LegionMemoryPool*>(mp));
        HIP_CALL(hipEventDestroy(sl.done));
        HIP_CALL(hipEventDestroy(sl.sampled));
        if (p->overlap || &sl == &p->slots[0]) HIP_CALL(hipStreamDestroy(sl.stream));
    }
    if (p->sample_stream) HIP_CALL(hipStreamDestroy(p->sample_stream));
    if (p->bulk) {
        for (size_t o = 0; o < p->bulk->owner_streams.size(); o++)
            if (p->bulk->owner_streams[o] != nullptr) {
                SetGPUDevice(p->dev_id / p->bulk->Kg * p->bulk->Kg + (int32_t)o);
                HIP_CALL(hipStreamDestroy(p->bulk->owner_streams[o]));
            }
        SetGPUDevice(p->dev_id);
        for (BulkPeer& peer : p->bulk->peers)
            if (peer.mapped_chunks && peer.arena != nullptr) lg_scattered_unmap_remote(peer.arena);
        for (void* a : p->bulk->alloc) d_free_space(a);
        delete p->bulk;
    }
    if (p->arena.base && !p->arena_borrowed) d_free_space(p->arena.base);
    lg_private_block_destroy(p->priv);
    delete p;
}

// ---- peer_gather = bulk: owner-bucketed transfer of the rows a striped gather needs from other members ----------------------
// (kernels_gather.hip bulk_bucket_kernel / bulk_push_kernel; LegionTuning.peer_gather.)  A group is produced in two host-visible
// phases, because the owners of the rows are other GPUs -- possibly other processes -- that must know the group's lists are final:
//   phase A (every member, its own group):  sampler -> bucket pass (per-owner lists) -> gather of everything that is NOT another
//            member's stripe (own stripe, replica, misses); stream synchronised on return
//   --- the caller's barrier over the clique (threads: any barrier; processes: e.g. torch.distributed) ---
//   phase B (every member, as an owner):    for every other member, push the rows it listed for this GPU into its lane arena;
//            stream synchronised on return
//   --- barrier --- : every lane of the slot holds its complete batch.
// Lookup results (cache_search_buffer, hit mask) and rows are those of the direct arrangement, bit for bit.
struct LegionBulkHandles {
    hipIpcMemHandle_t arena;          // arena_kind 0: a plain allocation
    hipIpcMemHandle_t lists[4];
    int64_t cap;
    int32_t slots, member;
    // arena_kind 1: the arena consists of arena_chunks chunks of arena_chunk_bytes, served as file descriptors on the abstract unix
    // socket wire_bulk_socket_name(arena_pid, arena_tag)
    int32_t arena_kind, arena_chunks, arena_pid, arena_tag;
    int64_t arena_chunk_bytes;
};
static_assert(sizeof(LegionBulkHandles) <= 512, "bulk handles travel in a 512-byte buffer");

extern "C" int32_t legion_pipeline_bulk_enable(LegionPipeline* p)
{
    if (!p || p->arena.base == nullptr) { printf("legion_hip: bulk transfers need a pipeline created with arena-backed lanes (use_graph bit 5)\n"); return 0; }
    if (p->slots_n > 4) { printf("legion_hip: at most 4 pipeline slots with bulk transfers\n"); return 0; }
    UnifiedCache* cache = reinterpret_cast<UnifiedCache*>(p->cache_handle);
    if (cache->FeatureDtype() != LEGION_FEATURE_F32 || p->feature->FeatureDtype() != LEGION_FEATURE_F32) {
        printf("legion_hip: peer_gather = bulk pushes float32 stripe rows only; a bf16 feature storage needs peer_gather = direct\n");
        return 0;
    }
    if (p->feature_out_dtype != LEGION_FEATURE_F32) {
        printf("legion_hip: peer_gather = bulk pushes float32 rows only; bf16 feature output needs peer_gather = direct\n");
        return 0;
    }
    SetGPUDevice(p->dev_id);
    BulkState* b = new BulkState();
    b->Kg = cache->Kg_ > 0 ? cache->Kg_ : 1;
    b->member = p->dev_id % b->Kg;
    b->cap = (int64_t)p->group_size * std::max<int64_t>(p->feature_rows, 1);
    b->peers.resize(b->Kg);
    for (int32_t s = 0; s < p->slots_n; s++) {
        const int64_t bytes = 256 + b->Kg * b->cap * 12;
        char* a = (char*)d_alloc_space(bytes);
        HIP_CALL(hipMemset(a, 0, 256));
        lg::BulkLists l;
        l.Kg = b->Kg;
        l.cap = b->cap;
        l.cnt = (unsigned long long*)a;
        l.dst = (int64_t*)(a + 256);
        l.fidx = (int32_t*)(a + 256 + b->Kg * b->cap * 8);
        b->alloc.push_back(a);
        b->mine.push_back(l);
    }
    // the other members of the clique, as owners, write rows into THIS arena: a chunked arena must grant their devices access
    // (members that live in other processes map the chunks themselves: legion_pipeline_bulk_import)
    if (lg_scattered_info(p->arena.base, nullptr) > 0) {
        std::vector<int32_t> devs;
        const int32_t base = p->dev_id / b->Kg * b->Kg;
        for (int32_t o = 0; o < b->Kg; o++)
            if (lg_is_local(base + o)) devs.push_back(base + o);
        if (!lg_scattered_grant(p->arena.base, devs.data(), (int32_t)devs.size())) {
            for (void* a : b->alloc) d_free_space(a);
            delete b;
            return 0;
        }
    }
    p->bulk = b;
    return 1;
}

// the lanes were carved from an arena the CALLER owns (GPURunner's lane arena, handed to lg_pipeline_create):
// bulk transfers address it, the pipeline does not free it
extern "C" int32_t legion_pipeline_bulk_enable_shared(LegionPipeline* p, const PoolArena* arena)
{
    if (!p || !arena || arena->base == nullptr || p->arena.base != nullptr) return 0;
    p->arena = *arena;
    p->arena_borrowed = true;
    return legion_pipeline_bulk_enable(p);
}

static lg::BulkLists lists_at(char* a, int32_t Kg, int64_t cap)
{
    lg::BulkLists l;
    l.Kg = Kg;
    l.cap = cap;
    l.cnt = (unsigned long long*)a;
    l.dst = (int64_t*)(a + 256);
    l.fidx = (int32_t*)(a + 256 + Kg * cap * 8);
    return l;
}

// what the other members need of this GPU: IPC handles of its lane arena and of its lists (400 bytes)
extern "C" int32_t legion_pipeline_bulk_export(LegionPipeline* p, void* out_handles, int32_t out_bytes)
{
    if (!p || !p->bulk || !out_handles || out_bytes < (int32_t)sizeof(LegionBulkHandles)) return 0;
    SetGPUDevice(p->dev_id);
    LegionBulkHandles h;
    memset(&h, 0, sizeof(h));
    int32_t n_chunks = 0;
    const int64_t chunk_bytes = lg_scattered_info(p->arena.base, &n_chunks);
    if (chunk_bytes > 0) {              // an arena of shuffled chunks: other processes map it from file descriptors
        if (!lg_scattered_exportable(p->arena.base)) {      // (a pipeline created with arena = True, bit 5 without bit 6)
            printf("legion_hip: legion_pipeline_bulk_export: this pipeline's lane arena was not created exportable (use_graph bit 6 / arena = \"shared\"); "
                   "another process cannot map it\n");
            return 0;
        }
        static std::atomic<int32_t> next_tag{0};
        if (p->bulk->served_tag < 0) {
            p->bulk->served_tag = next_tag.fetch_add(1);
            char name[WIRE_NAME_MAX];
            wire_bulk_socket_name(name, sizeof(name), (int)getpid(), p->bulk->served_tag);
            if (!lg_scattered_serve(p->arena.base, name)) { printf("legion_hip: could not serve the lane arena's chunks on %s\n", name); return 0; }
        }
        h.arena_kind = 1;
        h.arena_chunks = n_chunks;
        h.arena_chunk_bytes = chunk_bytes;
        h.arena_pid = (int32_t)getpid();
        h.arena_tag = p->bulk->served_tag;
    } else {
        lg_ipc_export(&h.arena, p->arena.base, __FILE__, __LINE__);
    }
    for (int32_t s = 0; s < p->slots_n; s++) lg_ipc_export(&h.lists[s], p->bulk->alloc[s], __FILE__, __LINE__);
    h.cap = p->bulk->cap;
    h.slots = p->slots_n;
    h.member = p->bulk->member;
    memcpy(out_handles, &h, sizeof(h));
    return (int32_t)sizeof(h);
}

// a member that lives in ANOTHER process: open its handles
extern "C" int32_t legion_pipeline_bulk_import(LegionPipeline* p, const void* handles)
{
    if (!p || !p->bulk || !handles) return 0;
    LegionBulkHandles h;
    memcpy(&h, handles, sizeof(h));
    // (a member's lists have ITS capacity -- lanes x its own feature rows, which follow its own PreSC maximum)
    if (h.member < 0 || h.member >= p->bulk->Kg || h.member == p->bulk->member || h.slots != p->slots_n || h.cap <= 0) {
        printf("legion_hip: bulk handles of member %d do not fit this pipeline (slots %d/%d, cap %lld)\n", h.member, h.slots, p->slots_n,
               (long long)h.cap);
        return 0;
    }
    SetGPUDevice(p->dev_id);
    BulkPeer& peer = p->bulk->peers[h.member];
    void* a = nullptr;
    if (h.arena_kind == 1) {
        char name[WIRE_NAME_MAX];
        wire_bulk_socket_name(name, sizeof(name), h.arena_pid, h.arena_tag);
        a = lg_scattered_map_remote(name, h.arena_chunks, h.arena_chunk_bytes);
        if (a == nullptr) return 0;
        peer.mapped_chunks = true;
    } else {
        HIP_CALL(hipIpcOpenMemHandle(&a, h.arena, hipIpcMemLazyEnablePeerAccess));
    }
    peer.arena = (char*)a;
    peer.lists.clear();
    for (int32_t s = 0; s < h.slots; s++) {
        void* l = nullptr;
        HIP_CALL(hipIpcOpenMemHandle(&l, h.lists[s], hipIpcMemLazyEnablePeerAccess));
        peer.lists.push_back(lists_at((char*)l, p->bulk->Kg, h.cap));
    }
    return 1;
}

// a member that lives in THIS process (a thread per GPU, or logical GPUs of a test): take its pointers
extern "C" int32_t legion_pipeline_bulk_link(LegionPipeline* p, LegionPipeline* other)
{
    if (!p || !p->bulk || !other || !other->bulk || other->bulk->member == p->bulk->member || other->slots_n != p->slots_n) return 0;
    BulkPeer& peer = p->bulk->peers[other->bulk->member];
    peer.arena = other->arena.base;
    peer.lists = other->bulk->mine;
    // this GPU, as an owner, writes rows into the other member's arena: a chunked arena must say so (a plain one is reached through
    // the peer access SetGPUDevice enabled)
    const int32_t me = p->dev_id;
    if (lg_scattered_info(other->arena.base, nullptr) > 0 && !lg_scattered_grant(other->arena.base, &me, 1)) return 0;
    return 1;
}

// phase A; returns the slot
extern "C" int32_t legion_pipeline_bulk_phase_a(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size)
{
    if (!p || !p->bulk) { printf("invalid pipeline ptr\n"); return -1; }
    if (n_active < 1 || n_active > p->group_size) n_active = p->group_size;
    batch_size = checked_batch_size(p, batch_size);
    SetGPUDevice(p->dev_id);
    lg::Range mark("bulk group A slot=%d first=%d lanes=%d", p->rr, counter0, n_active);
    const int32_t si = acquire_slot(p, counter0, mode);      // (the gathers' timing is submit_ex's: prof_used stays)
    Slot& sl = p->slots[si];
    hipStream_t X = sl.stream;
    LegionGraphStorage* gr = reinterpret_cast<LegionGraphStorage*>(p->graph);
    LegionFeatureStorage* f = reinterpret_cast<LegionFeatureStorage*>(p->feature);
    UnifiedCache* cache = reinterpret_cast<UnifiedCache*>(p->cache_handle);
    legion_group_set_iter_state(sl.group, nullptr);            // eager launches: the iteration by value
    legion_enqueue_group_phase(X, gr, f, p->cache_handle, sl.group, n_active, batch_size, counter0, p->dev_id, mode, p->fanout.data(),
                               p->hop_num, LG_PHASE_SAMPLE);
    const lg::BulkLists& mine = p->bulk->mine[si];
    HIP_CALL(hipMemsetAsync(mine.cnt, 0, 256, X));
    const LanePtrs* d_lanes = static_cast<const LanePtrs*>(legion_group_lane_desc(sl.group, 0));
    const int32_t max_rows = (int32_t)std::min<int64_t>(p->feature_rows, sl.pools[0]->num_ids);
    cache->BulkBucket(d_lanes, n_active, batch_whole_gather(p->hop_num), p->dev_id, X, max_rows, mine, p->arena.base);
    // the gathers of a whole-batch enqueue, in its order (batch_ops.h), each skipping the rows of other members' stripes
    const BatchOpList ops = batch_op_list(p->hop_num, LG_PHASE_GATHER, false, false);
    for (int32_t i = 0; i < ops.n; i++) {
        UnifiedCache::GatherCall call;
        call.op_id = ops.op[i].op_id;
        call.first_op_id = ops.op[i].first_op_id;
        call.last_op = ops.op[i].hop + 1 == p->hop_num;
        call.skip_remote = true;
        call.max_rows = max_rows;
        call.out_dtype = p->feature_out_dtype;
        cache->FeatCacheLookup(d_lanes, n_active, p->dev_id, X, call);
    }
    HIP_CALL(hipStreamSynchronize(X));
    sl.next_iter = -1;
    p->last_slot = si;
    return si;
}

// phase B: this GPU as an owner, for the group every member has in `slot`
extern "C" void legion_pipeline_bulk_phase_b(LegionPipeline* p, int32_t slot)
{
    if (!p || !p->bulk || slot < 0 || slot >= p->slots_n) { printf("invalid pipeline ptr\n"); return; }
    SetGPUDevice(p->dev_id);
    lg::Range mark("bulk group B slot=%d", slot);
    Slot& sl = p->slots[slot];
    UnifiedCache* cache = reinterpret_cast<UnifiedCache*>(p->cache_handle);
    const int32_t me = p->bulk->member;
    for (int32_t r = 0; r < p->bulk->Kg; r++) {
        if (r == me) continue;
        const BulkPeer& peer = p->bulk->peers[r];
        if (peer.arena == nullptr || (int32_t)peer.lists.size() <= slot) {
            printf("legion_hip: member %d of the clique was never imported / linked\n", r);
            exit(EXIT_FAILURE);
        }
        const lg::BulkLists& l = peer.lists[slot];
        cache->BulkPush(p->dev_id, sl.stream, l.fidx + (int64_t)me * l.cap, l.dst + (int64_t)me * l.cap, l.cnt + me, l.cap, peer.arena);
    }
    HIP_CALL(hipStreamSynchronize(sl.stream));
    HIP_CALL(hipEventRecord(sl.done, sl.stream));
    sl.busy = true;
}

// One server process, a thread per GPU (the reference's deployment): the whole group in one call, no barrier.  Every member's
// stripe lives in this process, so the REQUESTER's thread itself launches the push kernels on the owners' devices (any thread
// may launch on any device; peer access is on: StorageManagement::EnableP2PAccess) as soon as its own lists are final, and waits
// for them.  Eager launches, synchronous: returns the slot with the group complete.
extern "C" int32_t legion_pipeline_submit_bulk_inproc(LegionPipeline* p, int32_t counter0, int32_t mode, int32_t n_active, int32_t batch_size)
{
    if (!p || !p->bulk) { printf("invalid pipeline ptr\n"); return -1; }
    const int32_t si = legion_pipeline_bulk_phase_a(p, counter0, mode, n_active, batch_size);
    if (si < 0) return si;
    BulkState* b = p->bulk;
    UnifiedCache* cache = reinterpret_cast<UnifiedCache*>(p->cache_handle);
    const int32_t base = p->dev_id / b->Kg * b->Kg, me = b->member;
    const lg::BulkLists& l = b->mine[si];
    if (b->owner_streams.empty()) b->owner_streams.assign(b->Kg, nullptr);
    for (int32_t o = 0; o < b->Kg; o++) {
        if (o == me) continue;
        SetGPUDevice(base + o);
        if (b->owner_streams[o] == nullptr) HIP_CALL(hipStreamCreateWithFlags(&b->owner_streams[o], hipStreamNonBlocking));
        cache->BulkPush(base + o, b->owner_streams[o], l.fidx + (int64_t)o * l.cap, l.dst + (int64_t)o * l.cap, l.cnt + o, l.cap, p->arena.base);
    }
    for (int32_t o = 0; o < b->Kg; o++) {
        if (o == me) continue;
        SetGPUDevice(base + o);
        HIP_CALL(hipStreamSynchronize(b->owner_streams[o]));
    }
    SetGPUDevice(p->dev_id);
    Slot& sl = p->slots[si];
    HIP_CALL(hipEventRecord(sl.done, sl.stream));
    sl.busy = true;
    return si;
}

// rows this GPU listed for the other members in `slot` (diagnostics: what crosses xGMI towards this GPU in phase B)
extern "C" int64_t legion_pipeline_bulk_listed(LegionPipeline* p, int32_t slot)
{
    if (!p || !p->bulk || slot < 0 || slot >= p->slots_n) return 0;
    SetGPUDevice(p->dev_id);
    unsigned long long c[8] = {0};
    HIP_CALL(hipMemcpy(c, p->bulk->mine[slot].cnt, sizeof(unsigned long long) * std::min(p->bulk->Kg, 8), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int32_t i = 0; i < std::min(p->bulk->Kg, 8); i++) n += (int64_t)c[i];
    return n;
}

// Gather timing over the live pipeline: HIP events recorded on each slot's stream right before and
// after every gather launch.  hipEventElapsedTime rejects events recorded by graph nodes
// ('invalid resource handle' on ROCm 7.2), so groups submitted while profiling is on are launched
// eagerly (same kernels, same grouping).  read() returns, per gather op id, the summed elapsed ms and
// launch count of all groups that have been waited for since begin().
extern "C" void legion_pipeline_profile_begin(LegionPipeline* p)
{
    if (!p) return;
    SetGPUDevice(p->dev_id);
    for (Slot& sl : p->slots) {
        slot_wait(p, sl);
        HIP_CALL(hipStreamSynchronize(sl.stream));
        legion_pool_profile_begin(reinterpret_cast<LegionMemoryPool*>(sl.pools[0]), p->hop_num + 1);
    }
    p->prof_ms.clear();
    p->prof_cnt.clear();
    p->profiling = true;
}

extern "C" void legion_pipeline_profile_end(LegionPipeline* p)
{
    if (!p) return;
    for (Slot& sl : p->slots) {
        slot_wait(p, sl);
        sl.pools[0]->prof_on = false;
    }
    p->profiling = false;
}

extern "C" int32_t legion_pipeline_profile_read(LegionPipeline* p, int32_t* op_ids, double* ms_sums, int64_t* counts,
                                                int32_t cap)
{
    if (!p) return 0;
    int32_t n = 0;
    for (auto& kv : p->prof_ms) {
        if (n >= cap) break;
        op_ids[n] = kv.first;
        ms_sums[n] = kv.second;
        counts[n] = p->prof_cnt[kv.first];
        n++;
    }
    return n;
}
