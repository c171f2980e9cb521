// pool_plan.h -- how much memory a lane (a MemoryPool of depth 1) needs: the shape of a batch (pool_shape), the bytes of its
// trainer-visible arrays (pool_visible_bytes) and the list of its private arrays with their sizes (pool_private_plan).  Host-only, no
// HIP: lg_pool_alloc_private (storage.hip) allocates by walking the list, MemoryPool::Finalize frees what that walk recorded, the
// pipeline sizes its private block from the list's sum, and tests/cpu/pool_plan_test.cpp pins the sums over a table of shapes.
#pragma once

#include <cstdint>
#include <vector>

#include "sample_plan.h"

#define POOL_IDS_LIMIT (((int64_t)1 << 31) - 16384)      // positions and slot indices are int32, as in the reference (operator_impl.cu:208)
#define POOL_ROW_HDR_BYTES 16                            // sizeof(RowHdr), legion_core.h asserts it
#define POOL_HOP_SCRATCH_WORDS 32                        // HS_WORDS, likewise
#ifndef LG_CLAIM_CNT_STRIDE
#define LG_CLAIM_CNT_STRIDE 32        // ints between the claim-list counts of two buckets: a line each (the 8 / 16 reservations of a super tile go to different lines)
#endif

// bytes of one element of a row handed to the caller (a pool's feature output dtype, LEGION_FEATURE_*)
static inline int64_t lg_feature_out_bytes(int32_t out_dtype) { return out_dtype == LEGION_FEATURE_BF16 ? 2 : 4; }
// what one allocation takes from an arena or a block, and what d_alloc_space hands out at least
static inline int64_t pool_round(int64_t bytes) { return ((bytes > 0 ? bytes : 16) + 255) & ~(int64_t)255; }

// The one place the fan-out product is formed (server.cu:187-199).  num_ids and max_slots are int64 here: a shape over the limit
// is refused by the caller (message and exit are its own) before it narrows them.
struct PoolShape {
    int64_t num_ids = 0;               // B + B f1 + ... + B f1..fH
    int64_t max_slots = 0;             // the largest hop, B f1..fH
    std::vector<int64_t> max_new;      // [h] upper bound of the new nodes of op 3h (h = 0: the seeds)
    int32_t max_fanout = 0;
    int64_t listed_nodes = 0;          // what hops 1 .. H-1 can add (the known lists hold them)
    bool over_limit = false;           // num_ids >= 2^31 - 16384
};
static inline PoolShape pool_shape(int32_t batch_size, const int32_t* fanout, int32_t hop_num)
{
    PoolShape s;
    int64_t per = batch_size;
    s.num_ids = batch_size;
    s.max_new.assign(1, batch_size);
    for (int32_t h = 0; h < hop_num; h++) {
        per *= fanout[h];
        s.num_ids += per;
        s.max_new.push_back(per);
        if (fanout[h] > s.max_fanout) s.max_fanout = fanout[h];
        if (h + 1 < hop_num) s.listed_nodes += per;
    }
    s.max_slots = per;
    s.over_limit = s.num_ids >= POOL_IDS_LIMIT;
    return s;
}

// the trainer-visible arrays of one lane as an arena holds them: sampled_ids, agg_src_off, agg_dst_off, labels, the two counter
// blocks and the feature rows, each rounded up to 256 bytes
static inline int64_t pool_visible_bytes(int64_t batch_size, int64_t num_ids, int64_t feature_rows, int64_t float_feature_len, int32_t feature_out_dtype)
{
    auto r = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    return 3 * r(num_ids * 4) + r(batch_size * 4) + 2 * r(64) + r(feature_rows * float_feature_len * lg_feature_out_bytes(feature_out_dtype));
}

// the lane-private arrays, named as MemoryPool's members are, in the order they are allocated
enum PoolArray {
    PA_CACHE_SEARCH, PA_CLAIM_PAIRS, PA_CLAIM_CNT, PA_RUN_OFF, PA_KNOWN_PAIRS, PA_KNOWN_CNT, PA_AGG_SRC_IDS, PA_AGG_DST_IDS,
    PA_TMP_PART_IND, PA_TMP_PART_OFF, PA_SLOT_DST, PA_SLOT_POS, PA_SLOT_FS, PA_NODE_SLOT, PA_TILE_STATE, PA_FH_EDGE, PA_HOP_SCRATCH,
    PA_COUNT
};
struct PoolPrivatePlan {
    struct Entry { PoolArray what; int64_t bytes; };
    Entry entries[PA_COUNT];
    int32_t n = 0;
    int64_t sum = 0;                   // every entry rounded up to 256, as d_alloc_space counts it and a private block is carved
    SamplePoolPlan sample;
    int64_t bytes_of(PoolArray what) const
    {
        for (int32_t i = 0; i < n; i++) if (entries[i].what == what) return entries[i].bytes;
        return 0;
    }
};
// col_slots: LegionTuning's (!= 0: the carried feature-cache slots exist).  The edge-id arrays are not here: plain allocations of the
// pool, made when the mode is turned on (lg_pool_alloc_edge_ids)
static inline PoolPrivatePlan pool_private_plan(const PoolShape& s, const SamplePoolPlan& sp, int32_t col_slots)
{
    PoolPrivatePlan p;
    p.sample = sp;
    auto add = [&](PoolArray what, int64_t bytes) {
        p.entries[p.n++] = {what, bytes};
        p.sum += pool_round(bytes);
    };
    const int64_t n_buckets = (int64_t)1 << sp.bucket_bits;
    add(PA_CACHE_SEARCH, s.num_ids * 4);
    // first touches (legion_core.h): no per-vertex state; one claim list (interleaved by chunk: LanePtrs) and one known list per hash bucket
    add(PA_CLAIM_PAIRS, n_buckets * sp.claim_chunks * LG_CLAIM_CHUNK * 8);
    add(PA_CLAIM_CNT, n_buckets * LG_CLAIM_CNT_STRIDE * 4);
    if (sp.run_off_parts > 0)          // 256 buckets: {first place, count} per partition tile and bucket (sample_kernel -> place_kernel)
        add(PA_RUN_OFF, sp.run_off_parts * n_buckets * 2 * 4);
    if (sp.known_cap > 0) {            // per-bucket lists of the nodes hops 1 .. H-1 add
        add(PA_KNOWN_PAIRS, n_buckets * sp.known_cap * 8);
        add(PA_KNOWN_CNT, n_buckets * 4);
    }
    add(PA_AGG_SRC_IDS, s.num_ids * 4);
    add(PA_AGG_DST_IDS, s.num_ids * 4);
    add(PA_TMP_PART_IND, s.num_ids);
    add(PA_TMP_PART_OFF, s.num_ids * 4);
    add(PA_SLOT_DST, s.max_slots * 4);
    add(PA_SLOT_POS, s.max_slots * 4);
    if (col_slots != 0) {              // carried feature-cache slots (column slots): per slot of a hop, per node of the batch
        add(PA_SLOT_FS, s.max_slots * 4);
        add(PA_NODE_SLOT, s.num_ids * 4);
    }
    const int64_t max_tiles = (s.max_slots + LG_TILE - 1) / LG_TILE + 1;
    add(PA_TILE_STATE, (max_tiles / LG_SLOTS_PER_LANE + 2) * 8);
    add(PA_FH_EDGE, s.num_ids * POOL_ROW_HDR_BYTES);
    add(PA_HOP_SCRATCH, POOL_HOP_SCRATCH_WORDS * 4);
    return p;
}
// the pool plan of a shape with a source's hints and the tuning's three fields, as lg_pool_alloc_private and the pipeline both ask
static inline PoolPrivatePlan pool_private_plan(const PoolShape& s, const int64_t claims_hint[2], int32_t lds_small_buckets, int32_t lds_claim_cap,
                                                int32_t lds_known_cap, int32_t col_slots)
{
    return pool_private_plan(s, sample_pool_plan(s.max_slots, s.listed_nodes, claims_hint[0], claims_hint[1], lds_small_buckets, lds_claim_cap, lds_known_cap),
                             col_slots);
}
