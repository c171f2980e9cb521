// batch_ops.h -- the op order of a mini-batch, stated once: which ops a phase of a whole-batch enqueue issues, in which order, with
// which op ids, and which gathers share a launch.  Host-only, no HIP: enqueue_lanes (operators.hip) executes the list,
// legion_pipeline_bulk_phase_a (pipeline.hip) walks its gathers, the Runner's hand-over and BulkBucket take batch_whole_gather;
// tests/cpu/batch_ops_test.cpp pins every list over a literal table.
#pragma once

#include <cstdint>

// phases of a whole-batch enqueue (legion_enqueue_group_phase)
#define LG_PHASE_ALL 0      // reference op order: gather right after the op that produced its rows
#define LG_PHASE_SAMPLE 1   // BatchGenerate + every RandomSample + IOComplete
#define LG_PHASE_GATHER 2   // every FeatureCacheLookup, from the per-op range snapshots (bulk phase A, behind its own sampler phase)
// "weave" arrangement (pipeline.hip): the group cut where its character changes
#define LG_PHASE_HEAD 3     // BatchGenerate + every hop but the last, complete: small, latency-bound kernels
#define LG_PHASE_REST 4     // the last hop (sample .. localise) + IOComplete + every gather, in that order
#define LG_PHASE_REST_SAMPLE 5   // LG_PHASE_REST without the gathers (GPURunner serving a trainer end that gets its rows gathered
                                 // batch by batch straight into a pipe slot)

// op ids (SS/engine/server.cu:201-211): 0 the seeds, 3h hop h's sampler, 3h + 1 the gather of the rows op 3h added (op 1: the seeds')
constexpr int32_t BATCH_OP_STRIDE = 3;      // INTRABATCH_CON
constexpr int32_t BATCH_MAX_HOPS = 6;       // the counter block holds no more

enum class BatchOpKind { Seeds, Sample, Profile, EndOfBatch, Gather };
// hop: index into fanout[] (Sample), or of the hop whose rows are gathered (Gather; -1: the seeds'); first_op_id >= 0: the launch also
// covers the new-node ranges of the earlier ops first_op_id, +3, ...; -1 = alone
struct BatchOp { BatchOpKind kind; int32_t op_id; int32_t hop; int32_t first_op_id; };
struct BatchOpList { int32_t n; BatchOp op[16]; };

// Every row of the batch in one launch: the last op's gather with every earlier gather riding along
static inline BatchOp batch_whole_gather(int32_t hop_num) { return {BatchOpKind::Gather, BATCH_OP_STRIDE * hop_num + 1, hop_num - 1, 1}; }

// profile: CacheProfiling runs behind a PreSC batch's sampler (is_presc && TRAINMODE && a cache: the caller's to say).  The weave
// phases serve only: is_presc and profile do not reach them.
static inline BatchOpList batch_op_list(int32_t hop_num, int32_t phase, bool is_presc, bool profile)
{
    BatchOpList l{};
    if (hop_num > BATCH_MAX_HOPS) hop_num = BATCH_MAX_HOPS;      // (no pool exists for more: the longest list, ALL at six hops, has 14 ops)
    auto put = [&](BatchOpKind kind, int32_t op_id, int32_t hop, int32_t first_op_id) { l.op[l.n++] = {kind, op_id, hop, first_op_id}; };
    auto sample = [&](int32_t h) { put(BatchOpKind::Sample, BATCH_OP_STRIDE * (h + 1), h, -1); };
    // Inside a whole-batch enqueue every gather reads the {offset, count} snapshot its producer left in hop_scratch[HS_RANGE + 2h]
    // (not overwritten by later hops), so a gather may run any time after its producer.  The seeds' rows (op 1) are few and directly
    // in front of hop 1's: when a later gather follows (so that what FindFeat leaves in cache_search_buffer is the last op's either
    // way), one launch fetches both.
    const bool seeds_ride = hop_num >= 2;
    auto gather = [&](int32_t h) {      // of hop h's rows; -1: the seeds'
        if (h < 0 && seeds_ride) return;
        put(BatchOpKind::Gather, BATCH_OP_STRIDE * (h + 1) + 1, h, (h == 0 && seeds_ride) ? 1 : -1);
    };
    const bool weave = phase >= LG_PHASE_HEAD;
    const bool gathers = phase == LG_PHASE_REST || ((phase == LG_PHASE_ALL || phase == LG_PHASE_GATHER) && !is_presc);
    if (phase == LG_PHASE_HEAD) {
        put(BatchOpKind::Seeds, 0, -1, -1);
        for (int32_t h = 0; h + 1 < hop_num; h++) sample(h);
    } else if (weave) {
        // (every gather stays on the heavy stream, behind the last hop: the seeds' and earlier hops' gathers on the light stream
        // under the previous group's last gather were measured in round 4 -- no gain -- and removed)
        if (hop_num >= 1) sample(hop_num - 1);
        put(BatchOpKind::EndOfBatch, -1, -1, -1);
        if (gathers)
            for (int32_t h = -1; h < hop_num; h++) gather(h);
    } else {
        const bool sampler = phase != LG_PHASE_GATHER;
        if (sampler) put(BatchOpKind::Seeds, 0, -1, -1);
        if (gathers) gather(-1);
        for (int32_t h = 0; h < hop_num; h++) {      // (LG_PHASE_ALL: each gather right behind the op that produced its rows)
            if (sampler) sample(h);
            if (gathers) gather(h);
        }
        if (sampler && is_presc && profile) put(BatchOpKind::Profile, -1, -1, -1);
        if (sampler) put(BatchOpKind::EndOfBatch, -1, -1, -1);
    }
    return l;
}

// The rows a gather launch may write, and the bound its grid is sized by: the lane's feature buffer (feature_rows, never more than
// num_ids), and no more than the new nodes of op 3h can be (max_new[h] <= B f1..fh) plus those of the earlier ops that ride along
static inline int64_t gather_row_bound(const int64_t* max_new, int32_t n_max_new, int32_t op_id, int32_t first_op_id, bool use_snapshot,
                                       int64_t feature_rows, int64_t num_ids)
{
    int64_t max_rows = feature_rows;
    if (max_rows > num_ids) max_rows = num_ids;
    const uint64_t hop = (uint64_t)(op_id / BATCH_OP_STRIDE), n = (uint64_t)(n_max_new < 0 ? 0 : n_max_new);      // (a negative op: no hop's bound)
    int64_t bound = 0;
    for (uint64_t h = (use_snapshot && first_op_id >= 0 && first_op_id < op_id) ? (uint64_t)(first_op_id / BATCH_OP_STRIDE) : hop; h <= hop && h < n; h++)
        bound += max_new[h];
    if (hop < n && bound < max_rows) max_rows = bound;
    return max_rows;
}
