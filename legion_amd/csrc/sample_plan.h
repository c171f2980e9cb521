// sample_plan.h -- the sampler's launch decisions: the hash-bucket class of a pool and the sizes of its claim / known lists
// (sample_pool_plan), and the grids, partition tile and de-duplication instance of one hop (sample_hop_plan).  Host-only, no HIP:
// lg_pool_alloc_private (storage.hip) allocates the pool plan, launch_random_sample (kernels_sample.hip) launches the hop plan,
// tests/cpu/sample_plan_test.cpp pins both over a table of shapes -- the sampled batch never depends on any of this, only its speed.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

// Buckets per lane follow the pool's largest hop, so that a bucket sees a few thousand claims: 8 (or 16, dense graphs) up to 2^19
// slots per lane (B = 1024-class batches), 64 up to 2^22 (B = 8000 with [25,10]), 256 beyond (B = 8000 with [15,10,5] has 6 M,
// with [25,10,10] 20 M; larger hops run more passes per bucket).  The kernels are instantiated for the four classes.
#define LG_LDS_BITS_SMALL 3
#define LG_LDS_BITS_SMALL16 4                    // the same class with 16 buckets: dense graphs, see PoolSource::claims_hint
#ifndef LG_LDS_BITS_MEDIUM
#define LG_LDS_BITS_MEDIUM 6
#endif
#ifndef LG_LDS_BITS_LARGE
#define LG_LDS_BITS_LARGE 8
#endif
#ifndef LG_DEDUP_CLAIMS
#define LG_DEDUP_CLAIMS 5                       // claims a thread of a de-duplication workgroup keeps in registers (a bucket of at most LG_DEDUP_CLAIMS x 1024 is "resident")
#endif
#ifndef LG_DEDUP_CLAIMS_MID
#define LG_DEDUP_CLAIMS_MID 10                  // ... 10 where PreSC saw buckets of 5-10 k claims (B = 8000 on the less repetitive graphs: uk-union size, RMAT-28): 64 KB
#endif                                          // table, two workgroups per CU as with 5
#ifndef LG_DEDUP_CLAIMS_BIG
#define LG_DEDUP_CLAIMS_BIG 20                  // ... 20 beyond (B = 8000 [15,10,5] on RMAT-26: 15 k per bucket)
#endif
#ifndef LG_DEDUP_BIG_TABLE_BITS
#define LG_DEDUP_BIG_TABLE_BITS 14               // ... and the log2 words of its LDS table (14: 128 KB)
#endif
#define LG_LDS_SLOTS_SMALL (1 << 19)
#define LG_LDS_SLOTS_MEDIUM (1 << 22)
#ifndef LG_LDS_TABLE_BITS
#define LG_LDS_TABLE_BITS 13
#endif
#define LG_LDS_TABLE (1 << LG_LDS_TABLE_BITS)   // 64-bit words of LDS per (lane, bucket) workgroup
#ifndef LG_LDS_FILL_16THS
#define LG_LDS_FILL_16THS 14                    // a pass may fill its table up to this many sixteenths (bound: known + claims of the pass)
#endif
#define LG_CLAIM_CHUNK_BITS 9
#define LG_CLAIM_CHUNK (1 << LG_CLAIM_CHUNK_BITS)   // claim lists are interleaved in chunks of this many entries (LanePtrs)

#define LG_TILE 256            // compaction tile == threads per workgroup in the sampler kernels
#define LG_SLOTS_PER_LANE 4    // independent slots each lane keeps in flight
#define LG_SUPER (LG_TILE * LG_SLOTS_PER_LANE)   // slots one workgroup owns per iteration
#ifndef LG_COMPACT_THREADS
#define LG_COMPACT_THREADS 256 // threads of a compact_kernel workgroup
#endif
#define LG_LIST_CHUNK 8192     // new nodes a list_known_kernel workgroup takes per iteration
#define LG_PLACE_MAX_K 8       // most super tiles a partition tile of the 256-bucket class may have (place_kernel stages them in LDS)
// fewest super tiles a partition tile may have: the hop plan never goes below it, and the pool plan sizes run_off by it
static inline int32_t lg_lds_k_min(int32_t bucket_bits) { return bucket_bits == LG_LDS_BITS_LARGE ? 4 : 1; }

// What a bucket class fixes for its kernel instances: sample_kernel's SINGLE (partition tile = super tile; else place_kernel writes
// the claim lists) and STAGED (claims staged per super tile in LDS), and the most claims per thread its de-duplication is built for
struct SampleClassInfo { int32_t bits; bool single, staged; int32_t max_claims; };
constexpr SampleClassInfo SAMPLE_CLASSES[] = {
    {LG_LDS_BITS_SMALL, true, false, LG_DEDUP_CLAIMS},
    {LG_LDS_BITS_SMALL16, true, false, LG_DEDUP_CLAIMS},
    {LG_LDS_BITS_MEDIUM, true, true, LG_DEDUP_CLAIMS_BIG},
    {LG_LDS_BITS_LARGE, false, false, LG_DEDUP_CLAIMS_MID},
};
constexpr SampleClassInfo sample_class(int32_t bucket_bits)      // (bits of no class: the 256-bucket one, as the pool plan's fall-through)
{
    for (const SampleClassInfo& c : SAMPLE_CLASSES)
        if (c.bits == bucket_bits) return c;
    return SAMPLE_CLASSES[3];
}
// log2 words of the LDS table of the de-duplication that keeps `claims` per thread
constexpr int32_t lg_dedup_table_bits(int32_t claims) { return claims == LG_DEDUP_CLAIMS_BIG ? LG_DEDUP_BIG_TABLE_BITS : LG_LDS_TABLE_BITS; }

// what PreSC counted, as the plans take it: +10 %, because buckets are not even (a bucket that still outgrows what was planned
// for it is served all the same, by more passes or by re-reading its list)
static inline int64_t lg_hint_with_margin(int64_t counted) { return counted * 11 / 10; }

struct SamplePoolPlan {
    int32_t bucket_bits;     // LG_LDS_BITS_SMALL / SMALL16 / MEDIUM / LARGE
    int32_t claim_cap;       // entries per claim list
    int64_t claim_chunks;    // LG_CLAIM_CHUNK-entry chunks per claim list
    int32_t known_cap;       // entries per known-node list, 0: nothing is listed (a single hop)
    int64_t run_off_parts;   // partition tiles run_off has room for, 0: the class has no run_off
};

// slots: the pool's largest hop (B f1..fH); listed_nodes: the nodes hops 1 .. H-1 can add; hint_*: PreSC's maxima of the last hop's
// edges and of the nodes before it (PoolSource::claims_hint; 0: unknown); the rest: LegionTuning's fields of these names
static inline SamplePoolPlan sample_pool_plan(int64_t slots, int64_t listed_nodes, int64_t hint_last_hop_edges, int64_t hint_nodes_before,
                                              int32_t lds_small_buckets, int32_t lds_claim_cap, int32_t lds_known_cap)
{
    SamplePoolPlan p{};
    // Slots say how large a hop CAN get; PreSC says how many claims the largest hop really has.  64 buckets serve a hop as long as
    // a bucket's claims fit the registers of its workgroup (LG_DEDUP_CLAIMS_BIG x 1024; it then runs its passes over sub-buckets
    // from the registers) -- e.g. B = 8000 with [15,10,5]: 6 M slots but ~0.9 M claims in hop 3 -- and the sampling kernel writes 64
    // lists itself; beyond that 256 buckets, whose lists a second kernel writes (place_kernel).  Without PreSC's numbers: by slots.
    const int64_t hint_claims = lg_hint_with_margin(hint_last_hop_edges);
    const bool medium = hint_claims > 0 ? hint_claims <= (int64_t)64 * LG_DEDUP_CLAIMS_BIG * 1024 && slots <= ((int64_t)1 << 24)
                                        : slots <= LG_LDS_SLOTS_MEDIUM;
    p.bucket_bits = slots <= LG_LDS_SLOTS_SMALL ? LG_LDS_BITS_SMALL : (medium ? LG_LDS_BITS_MEDIUM : LG_LDS_BITS_LARGE);
    if (p.bucket_bits == LG_LDS_BITS_SMALL) {
        // The small class has 8 or 16 buckets per lane.  Slots do not say how many of them hold an edge: on a dense graph
        // (ogbn-products: 60 k edges per batch of 1024 where RMAT-26 has 35 k) a bucket of 8 holds more vertices than one LDS
        // table takes and every workgroup runs two passes (217 us instead of ~110 per 256-lane group).  PreSC has seen the real
        // numbers: 16 buckets where 8 would overflow one pass, else 8 (which is 8 us faster per group where both fit).
        const int64_t one_pass = LG_LDS_TABLE / 16 * LG_LDS_FILL_16THS;
        const int64_t need = lg_hint_with_margin(hint_last_hop_edges + hint_nodes_before);
        if (lds_small_buckets == 16 || (lds_small_buckets != 8 && need / 8 > one_pass)) p.bucket_bits = LG_LDS_BITS_SMALL16;
    }
    const int64_t n_buckets = (int64_t)1 << p.bucket_bits;
    // one claim list per bucket, twice an even share each (a bucket that outgrows its list is served from the hop's slots
    // instead, kernels_sample.hip)
    p.claim_cap = (int32_t)(2 * ((slots + n_buckets - 1) / n_buckets) + 256);
    if (lds_claim_cap > 0) p.claim_cap = lds_claim_cap;      // tests: force the fallback
    p.claim_chunks = ((int64_t)p.claim_cap + LG_CLAIM_CHUNK - 1) / LG_CLAIM_CHUNK;
    if (n_buckets > 64) {        // 256 buckets: sample_kernel -> place_kernel by partition tiles, the smallest the hop plan may pick
        const int64_t n_super = (slots + LG_SUPER - 1) / LG_SUPER + 1, k_min = lg_lds_k_min(p.bucket_bits);
        p.run_off_parts = (n_super + k_min - 1) / k_min + 1;
    }
    // per-bucket lists of the nodes hops 1 .. H-1 add (later hops must recognise them): twice an even share each; a bucket that
    // outgrows its list is served by scanning sampled_ids instead (kernels_sample.hip)
    if (listed_nodes > 0) {
        p.known_cap = (int32_t)(2 * ((listed_nodes + n_buckets - 1) / n_buckets) + 256);
        if (lds_known_cap > 0) p.known_cap = lds_known_cap;   // tests: force the scan
    }
    return p;
}

struct SampleHopPlan {
    int32_t sample_gx;       // grid x of sample_kernel: strided over super tiles, or (256 buckets) the place grid
    int32_t k;               // super tiles per partition tile (HopParams.lds_k)
    int32_t place_gx;        // 256 buckets: grid x of place_kernel and its dynamic LDS; else 0
    int64_t stage_bytes;
    int32_t dedup_claims;    // claims per thread of the dedup_lists_kernel instance, and the log2 words of its LDS table
    int32_t dedup_table_bits;
    int32_t compact_gx;      // grid x of compact_kernel
    int32_t known_chunks;    // grid x of list_known_kernel, 0 on the last hop
};

// bucket_bits: the pool plan's; max_slots: this hop's capacity (B f1..fh); n_lanes: grid y of every launch; last_hop_claims_hint:
// PreSC's maximum of the last hop's edges (0: unknown); sample_max_wg, lds_part_wg: LegionTuning's
static inline SampleHopPlan sample_hop_plan(int32_t bucket_bits, int32_t max_slots, int32_t n_lanes, bool last_hop, int64_t last_hop_claims_hint,
                                            int32_t sample_max_wg, int32_t lds_part_wg)
{
    SampleHopPlan p{};
    // Fixed grids that stride over super tiles; grid.y = lanes (independent mini-batches of a group).
    int32_t max_super = (max_slots + LG_SUPER - 1) / LG_SUPER;
    if (max_super < 1) max_super = 1;
    int32_t gx = max_super < 1024 ? max_super : 1024;
    while (gx > 64 && (int64_t)gx * n_lanes > sample_max_wg) gx /= 2;  // keep the whole launch near 2 x resident capacity
    while (gx > 1 && (int64_t)gx * n_lanes > sample_max_wg && sample_max_wg < 4096) gx /= 2;   // (experiments with fewer workgroups)
    {
        // Equal workgroups that fill the machine about twice leave its second round half empty: between one and six rounds' worth
        // (8 workgroups of this kernel per CU x 256 CUs), take ONE round of longer-lived workgroups instead.  Measured (one_round_ab.txt):
        // 64 lanes at B = 8000 (3 904 -> 2 048 workgroups) +1 %, 128 lanes at B = 4096 +1.4 %, 256 lanes and D = 256 the same within
        // the noise; 512 lanes at B = 1024 (15 rounds) are not touched.
        const int64_t resident = 8 * 256, total = (int64_t)gx * n_lanes;
        if (total > resident && total < 6 * resident) gx = (int32_t)(resident / n_lanes > 1 ? resident / n_lanes : 1);
    }
    // 8 / 16 / 64 buckets: the sampling kernel writes the claim lists itself (64: staged per super tile in LDS).  256 buckets: it
    // samples partition tiles of K super tiles and place_kernel writes the lists; K follows THIS hop: as large as the staging allows
    // (LG_PLACE_MAX_K) unless that leaves the launch with fewer than ~8 k workgroups by the hop's capacity (a hop typically fills a
    // quarter of it: ~2 k active ones; measured at B = 8000: 2 k -> 8 k +1...2 %, beyond: the same), and never below the class's minimum
    const bool single = sample_class(bucket_bits).single;
    p.k = single ? 1 : LG_PLACE_MAX_K;
    while (p.k > lg_lds_k_min(bucket_bits) && (int64_t)(max_super / p.k) * n_lanes < lds_part_wg) p.k /= 2;
    p.sample_gx = gx;
    if (!single) {
        int32_t gp = (max_super + p.k - 1) / p.k;              // one workgroup per partition tile ...
        while (gp > 16 && (int64_t)gp * n_lanes > 16384) gp = (gp + 1) / 2;  // ... within reason
        p.sample_gx = p.place_gx = gp;
        p.stage_bytes = (int64_t)p.k * LG_SUPER * 8;           // (a 64-bit pair per slot of the tile)
    }
    // 64- and 256-bucket classes, last hop: how many claims a de-duplication thread keeps in registers follows what PreSC saw in
    // that hop (a bucket of up to claims x 1024 is worked on from registers, whatever the number of passes over its sub-buckets)
    p.dedup_claims = LG_DEDUP_CLAIMS;
    if (last_hop && (bucket_bits == LG_LDS_BITS_MEDIUM || bucket_bits == LG_LDS_BITS_LARGE)) {
        const int64_t per_bucket = lg_hint_with_margin(last_hop_claims_hint) >> bucket_bits;
        if (per_bucket > (int64_t)LG_DEDUP_CLAIMS_MID * 1024 && bucket_bits == LG_LDS_BITS_MEDIUM) p.dedup_claims = LG_DEDUP_CLAIMS_BIG;
        else if (per_bucket > (int64_t)LG_DEDUP_CLAIMS * 1024) p.dedup_claims = LG_DEDUP_CLAIMS_MID;
    }
    p.dedup_table_bits = lg_dedup_table_bits(p.dedup_claims);
    // compaction: LG_COMPACT_THREADS per workgroup (a workgroup iteration takes 4 x that many consecutive slots), as many workgroups
    // per lane as the strided sampling grid has per 1024 slots' worth
    p.compact_gx = gx * LG_TILE / LG_COMPACT_THREADS > 1 ? gx * LG_TILE / LG_COMPACT_THREADS : 1;
    if (!last_hop) {             // later hops must recognise the nodes this one added: their buckets' lists
        p.known_chunks = (max_slots + LG_LIST_CHUNK - 1) / LG_LIST_CHUNK;
        if (p.known_chunks > 256) p.known_chunks = 256;
    }
    return p;
}
