// Pins the sampler's launch plans (legion_amd/csrc/sample_plan.h: sample_pool_plan, the bucket class and list sizes of a pool;
// sample_hop_plan, the grids, partition tile and de-duplication instance of a hop) over a table of shapes.  The expected values were
// worked out from the three code sites the plans replaced (lg_pool_alloc_private, do_random_sample, launch_random_sample), not from
// the header.
//   g++ -O1 -std=c++17 sample_plan_test.cpp -o t && ./t
#include <cstdio>
#include <initializer_list>

#include "../../legion_amd/csrc/sample_plan.h"

struct PoolCase {
    long long slots, listed, hint_edges, hint_before;
    int small_buckets, force_claim_cap, force_known_cap;
    int bits, claim_cap;
    long long claim_chunks;
    int known_cap;
    long long run_off_parts;
};

static const PoolCase pool_cases[] = {
    // slots, listed, PreSC's last-hop edges and nodes before, lds_small_buckets, forced claim / known cap -> bits, claim_cap, chunks, known_cap, run_off
    // B = 1024 with [25,10], with [25] (nothing listed), and a pool without hops
    {256000, 25600, 0, 0, 0, 0, 0,  3, 64256, 126, 6656, 0},
    {25600, 0, 0, 0, 0, 0, 0,  3, 6656, 13, 0, 0},
    {1024, 0, 0, 0, 0, 0, 0,  3, 512, 1, 0, 0},
    // the class boundaries by slots (no PreSC hint): 2^19 and 2^22
    {524288, 52429, 0, 0, 0, 0, 0,  3, 131328, 257, 13364, 0},
    {524289, 52429, 0, 0, 0, 0, 0,  6, 16642, 33, 1896, 0},
    {4194304, 419431, 0, 0, 0, 0, 0,  6, 131328, 257, 13364, 0},
    {4194305, 419431, 0, 0, 0, 0, 0,  8, 33026, 65, 3534, 1026},
    // B = 8000: [25,10]; [15,10,5] without and with PreSC's numbers; [25,10,10] is 256 buckets whatever the hint
    {2000000, 200000, 0, 0, 0, 0, 0,  6, 62756, 123, 6506, 0},
    {6000000, 1320000, 0, 0, 0, 0, 0,  8, 47132, 93, 10570, 1467},
    {6000000, 1320000, 900000, 700000, 0, 0, 0,  6, 187756, 367, 41506, 0},
    {20000000, 2200000, 0, 0, 0, 0, 0,  8, 156506, 306, 17444, 4885},
    {20000000, 2200000, 900000, 700000, 0, 0, 0,  8, 156506, 306, 17444, 4885},
    {20000000, 2200000, 1, 1, 0, 0, 0,  8, 156506, 306, 17444, 4885},
    // the hint's edge, 64 x 20 x 1024 claims after its +10 % (1191564 * 11 / 10 = 1310720), and the 2^24 slots beyond which a hint does not help
    {6000000, 1320000, 1191564, 0, 0, 0, 0,  6, 187756, 367, 41506, 0},
    {6000000, 1320000, 1191565, 0, 0, 0, 0,  8, 47132, 93, 10570, 1467},
    {16777216, 1320000, 900000, 0, 0, 0, 0,  6, 524544, 1025, 41506, 0},
    {16777217, 1320000, 900000, 0, 0, 0, 0,  8, 131330, 257, 10570, 4098},
    // a hint too large for 64 buckets decides below 2^22 slots too; the small class goes by slots alone
    {3000000, 300000, 2000000, 0, 0, 0, 0,  8, 23694, 47, 2600, 734},
    {256000, 25600, 2000000, 0, 8, 0, 0,  3, 64256, 126, 6656, 0},
    // 8 or 16 buckets: (edges + nodes before) + 10 % over 7168 per bucket of 8 (52138 * 11 / 10 / 8 = 7168); LEGION_LDS_SMALL_BUCKETS 8 and 16
    // overrule it (any other value does not), and only in the small class
    {256000, 25600, 50000, 2138, 0, 0, 0,  3, 64256, 126, 6656, 0},
    {256000, 25600, 50000, 2139, 0, 0, 0,  4, 32256, 63, 3456, 0},
    {256000, 25600, 52139, 0, 0, 0, 0,  4, 32256, 63, 3456, 0},
    {256000, 25600, 0, 52139, 0, 0, 0,  4, 32256, 63, 3456, 0},
    {256000, 25600, 50000, 2139, 8, 0, 0,  3, 64256, 126, 6656, 0},
    {256000, 25600, 0, 0, 16, 0, 0,  4, 32256, 63, 3456, 0},
    {256000, 25600, 50000, 2139, 16, 0, 0,  4, 32256, 63, 3456, 0},
    {256000, 25600, 50000, 2139, 4, 0, 0,  4, 32256, 63, 3456, 0},
    {2000000, 200000, 0, 0, 16, 0, 0,  6, 62756, 123, 6506, 0},
    {2000000, 200000, 900000, 900000, 8, 0, 0,  6, 62756, 123, 6506, 0},
    // forced capacities (chunks of 512 claims; a forced known cap lists nothing where nothing is listed)
    {256000, 25600, 0, 0, 0, 100, 0,  3, 100, 1, 6656, 0},
    {256000, 25600, 0, 0, 0, 512, 0,  3, 512, 1, 6656, 0},
    {256000, 25600, 0, 0, 0, 513, 64,  3, 513, 2, 64, 0},
    {256000, 0, 0, 0, 0, 0, 64,  3, 64256, 126, 0, 0},
    {6000000, 1320000, 0, 0, 0, 1000, 1000,  8, 1000, 2, 1000, 1467},
    {128000, 12800, 0, 0, 16, 0, 0,  4, 16256, 32, 1856, 0},
};

struct HopCase {
    int bits, max_slots, n_lanes, last_hop;
    long long hint;
    int sample_max_wg, lds_part_wg;
    int sample_gx, k, place_gx;
    long long stage_bytes;
    int claims, table_bits, compact_gx, known_chunks;
};

static const HopCase hop_cases[] = {
    // bits, max_slots, lanes, last hop, PreSC's last-hop edges, sample_max_wg, lds_part_wg -> sample grid, k, place grid, stage bytes, claims, table bits,
    // compaction grid, known-list chunks
    // B = 1024 [25,10], 512 lanes: 250 -> 125 -> 62 by the cap of 4096 (31 744 workgroups: outside the one-round window); 16 buckets the same
    // one lane; no slots at all; more lanes than one round has workgroups
    {3, 256000, 512, 1, 0, 4096, 8192,  62, 1, 0, 0, 5, 13, 62, 0},
    {3, 25600, 512, 0, 0, 4096, 8192,  25, 1, 0, 0, 5, 13, 25, 4},
    {4, 256000, 512, 1, 60000, 4096, 8192,  62, 1, 0, 0, 5, 13, 62, 0},
    {4, 25600, 256, 0, 60000, 4096, 8192,  8, 1, 0, 0, 5, 13, 8, 4},
    {3, 256000, 1, 1, 0, 4096, 8192,  250, 1, 0, 0, 5, 13, 250, 0},
    {3, 25600, 1, 0, 0, 4096, 8192,  25, 1, 0, 0, 5, 13, 25, 4},
    {3, 0, 1, 0, 0, 4096, 8192,  1, 1, 0, 0, 5, 13, 1, 0},
    {3, 0, 512, 1, 0, 4096, 8192,  1, 1, 0, 0, 5, 13, 1, 0},
    {3, 1024, 4096, 1, 0, 4096, 8192,  1, 1, 0, 0, 5, 13, 1, 0},
    {3, 1025, 16, 0, 0, 4096, 8192,  2, 1, 0, 0, 5, 13, 2, 1},
    // B = 8000 [25,10], 64 lanes: 1954 super tiles -> 1024 -> 64 by the cap -> 32 by the one-round rule (2048 workgroups)
    {6, 2000000, 64, 1, 0, 4096, 8192,  32, 1, 0, 0, 5, 13, 32, 0},
    {6, 200000, 64, 0, 0, 4096, 8192,  32, 1, 0, 0, 5, 13, 32, 25},
    {6, 2000000, 16, 1, 0, 4096, 8192,  128, 1, 0, 0, 5, 13, 128, 0},
    {6, 2000000, 1, 1, 0, 4096, 8192,  1024, 1, 0, 0, 5, 13, 1024, 0},
    // the one-round rule's edges: 2048 workgroups are one round, 12288 are six -- both untouched, 3072 and 11264 are not
    {6, 2000000, 2, 1, 0, 4096, 8192,  1024, 1, 0, 0, 5, 13, 1024, 0},
    {6, 2000000, 3, 1, 0, 4096, 8192,  682, 1, 0, 0, 5, 13, 682, 0},
    {6, 2000000, 12, 1, 0, 16384, 8192,  1024, 1, 0, 0, 5, 13, 1024, 0},
    {6, 2000000, 11, 1, 0, 16384, 8192,  186, 1, 0, 0, 5, 13, 186, 0},
    {6, 2000000, 4, 1, 0, 2048, 8192,  512, 1, 0, 0, 5, 13, 512, 0},
    {6, 2000000, 4, 1, 0, 4096, 8192,  512, 1, 0, 0, 5, 13, 512, 0},
    // both sample_max_wg loops: the second one (below 64 per lane) only for caps under 4096
    {6, 2000000, 64, 1, 0, 1024, 8192,  16, 1, 0, 0, 5, 13, 16, 0},
    {6, 2000000, 64, 1, 0, 64, 8192,  1, 1, 0, 0, 5, 13, 1, 0},
    {6, 2000000, 64, 1, 0, 8192, 8192,  32, 1, 0, 0, 5, 13, 32, 0},
    {3, 256000, 512, 1, 0, 100000, 8192,  125, 1, 0, 0, 5, 13, 125, 0},
    {3, 256000, 512, 1, 0, 512, 8192,  1, 1, 0, 0, 5, 13, 1, 0},
    // claims per thread, 64 buckets, last hop only: 5 / 10 / 20 on both sides of 5120 and 10240 per bucket after the +10 %
    {6, 6000000, 16, 1, 900000, 4096, 8192,  128, 1, 0, 0, 20, 14, 128, 0},
    {6, 1200000, 16, 0, 900000, 4096, 8192,  128, 1, 0, 0, 5, 13, 128, 147},
    {6, 6000000, 16, 1, 297949, 4096, 8192,  128, 1, 0, 0, 5, 13, 128, 0},
    {6, 6000000, 16, 1, 297950, 4096, 8192,  128, 1, 0, 0, 10, 13, 128, 0},
    {6, 6000000, 16, 1, 595839, 4096, 8192,  128, 1, 0, 0, 10, 13, 128, 0},
    {6, 6000000, 16, 1, 595840, 4096, 8192,  128, 1, 0, 0, 20, 14, 128, 0},
    // 256 buckets: 5 or 10 (1191797 * 11 / 10 >> 8 = 5121), never 20
    {8, 6000000, 16, 1, 0, 4096, 8192,  733, 8, 733, 65536, 5, 13, 128, 0},
    {8, 6000000, 16, 1, 1191796, 4096, 8192,  733, 8, 733, 65536, 5, 13, 128, 0},
    {8, 6000000, 16, 1, 1191797, 4096, 8192,  733, 8, 733, 65536, 10, 13, 128, 0},
    {8, 20000000, 16, 1, 10000000, 4096, 8192,  611, 8, 611, 65536, 10, 13, 128, 0},
    {8, 2000000, 16, 0, 10000000, 4096, 8192,  489, 4, 489, 32768, 5, 13, 128, 245},
    // k: 8 unless that leaves fewer than lds_part_wg workgroups by capacity, then 4, never below (5860 super tiles: 732 x 12 = 8784, x 11 = 8052)
    {8, 6000000, 8, 1, 0, 4096, 8192,  1465, 4, 1465, 32768, 5, 13, 256, 0},
    {8, 6000000, 1, 1, 0, 4096, 8192,  1465, 4, 1465, 32768, 5, 13, 1024, 0},
    {8, 20000000, 4, 1, 0, 4096, 8192,  2442, 8, 2442, 65536, 5, 13, 512, 0},
    {8, 20000000, 2, 1, 0, 4096, 8192,  4883, 4, 4883, 32768, 5, 13, 1024, 0},
    {8, 6000000, 8, 1, 0, 4096, 2048,  733, 8, 733, 65536, 5, 13, 256, 0},
    {8, 80000, 16, 0, 0, 4096, 8192,  20, 4, 20, 32768, 5, 13, 79, 10},
    {8, 0, 1, 0, 0, 4096, 8192,  1, 4, 1, 32768, 5, 13, 1, 0},
    {8, 6000000, 12, 1, 0, 4096, 8192,  733, 8, 733, 65536, 5, 13, 170, 0},
    {8, 6000000, 11, 1, 0, 4096, 8192,  1465, 4, 1465, 32768, 5, 13, 186, 0},
    // the place grid's cap of 16384 workgroups (halved while above it, not below 16 per lane)
    {8, 20000000, 16, 1, 0, 4096, 8192,  611, 8, 611, 65536, 5, 13, 128, 0},
    {8, 20000000, 8, 1, 0, 4096, 8192,  1221, 8, 1221, 65536, 5, 13, 256, 0},
    {8, 8388608, 16, 1, 0, 4096, 8192,  1024, 8, 1024, 65536, 5, 13, 128, 0},
    {8, 8388609, 16, 1, 0, 4096, 8192,  513, 8, 513, 65536, 5, 13, 128, 0},
    {8, 20000000, 2048, 1, 0, 4096, 8192,  10, 8, 10, 65536, 5, 13, 64, 0},
};

// the dedup_lists_kernel instances the library has: {bucket bits, claims per thread, log2 words of the LDS table}
static const int dedup_instances[7][3] = {{3, 5, 13}, {4, 5, 13}, {6, 5, 13}, {6, 10, 13}, {6, 20, 14}, {8, 5, 13}, {8, 10, 13}};
static bool is_instance(int bits, int claims, int table_bits)
{
    for (const auto& d : dedup_instances)
        if (d[0] == bits && d[1] == claims && d[2] == table_bits) return true;
    return false;
}

int main()
{
    int bad = 0, n = 0;
    for (const PoolCase& c : pool_cases) {
        n++;
        const SamplePoolPlan p = sample_pool_plan(c.slots, c.listed, c.hint_edges, c.hint_before, c.small_buckets, c.force_claim_cap, c.force_known_cap);
        if (p.bucket_bits != c.bits || p.claim_cap != c.claim_cap || p.claim_chunks != c.claim_chunks || p.known_cap != c.known_cap ||
            p.run_off_parts != c.run_off_parts) {
            printf("MISMATCH pool: slots %lld listed %lld hint %lld + %lld small_buckets %d caps %d %d: got bits %d claim_cap %d chunks %lld known_cap %d "
                   "run_off %lld, want bits %d claim_cap %d chunks %lld known_cap %d run_off %lld\n",
                   c.slots, c.listed, c.hint_edges, c.hint_before, c.small_buckets, c.force_claim_cap, c.force_known_cap, p.bucket_bits, p.claim_cap,
                   (long long)p.claim_chunks, p.known_cap, (long long)p.run_off_parts, c.bits, c.claim_cap, c.claim_chunks, c.known_cap, c.run_off_parts);
            bad++;
        }
        // the pool's last hop, planned with the pool's own class and hint, takes a de-duplication instance that exists; and run_off
        // has room for every partition tile that hop can have
        for (int lanes : {1, 16, 512}) {
            const SampleHopPlan h = sample_hop_plan(p.bucket_bits, (int)c.slots, lanes, true, c.hint_edges, 4096, 8192);
            const long long parts = (c.slots + (long long)h.k * LG_SUPER - 1) / ((long long)h.k * LG_SUPER);
            if (!is_instance(p.bucket_bits, h.dedup_claims, h.dedup_table_bits) || (p.bucket_bits == LG_LDS_BITS_LARGE && parts > p.run_off_parts)) {
                printf("MISMATCH pool -> hop: slots %lld hint %lld lanes %d: bits %d claims %d table bits %d k %d, run_off %lld\n", c.slots, c.hint_edges,
                       lanes, p.bucket_bits, h.dedup_claims, h.dedup_table_bits, h.k, (long long)p.run_off_parts);
                bad++;
            }
        }
    }
    for (const HopCase& c : hop_cases) {
        n++;
        const SampleHopPlan p = sample_hop_plan(c.bits, c.max_slots, c.n_lanes, c.last_hop != 0, c.hint, c.sample_max_wg, c.lds_part_wg);
        if (p.sample_gx != c.sample_gx || p.k != c.k || p.place_gx != c.place_gx || p.stage_bytes != c.stage_bytes || p.dedup_claims != c.claims ||
            p.dedup_table_bits != c.table_bits || p.compact_gx != c.compact_gx || p.known_chunks != c.known_chunks ||
            !is_instance(c.bits, p.dedup_claims, p.dedup_table_bits)) {
            printf("MISMATCH hop: bits %d max_slots %d lanes %d last %d hint %lld max_wg %d part_wg %d: got sample %d k %d place %d stage %lld claims %d "
                   "table bits %d compact %d known %d, want sample %d k %d place %d stage %lld claims %d table bits %d compact %d known %d\n",
                   c.bits, c.max_slots, c.n_lanes, c.last_hop, c.hint, c.sample_max_wg, c.lds_part_wg, p.sample_gx, p.k, p.place_gx,
                   (long long)p.stage_bytes, p.dedup_claims, p.dedup_table_bits, p.compact_gx, p.known_chunks, c.sample_gx, c.k, c.place_gx, c.stage_bytes,
                   c.claims, c.table_bits, c.compact_gx, c.known_chunks);
            bad++;
        }
    }
    printf("%d shapes, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
