// Pins a lane's memory plan (legion_amd/csrc/pool_plan.h: pool_shape, pool_visible_bytes, pool_private_plan) over a table of shapes.
// The private sums were PRINTED by the library before the plan existed -- what a probe lane asked d_alloc_space for, minus its
// trainer-visible arrays -- on an MI355X, one arena pipeline per row (DESIGN.md 4.16 lists the rows); they are not the header's output.
//   g++ -O1 -std=c++17 pool_plan_test.cpp -o t && ./t
#include <cstdio>
#include <vector>

#include "../../legion_amd/csrc/pool_plan.h"

static int failed = 0;
#define CHECK(what, got, want)                                                                                   \
    if ((long long)(got) != (long long)(want)) {                                                                  \
        printf("MISMATCH %s row %d: %s = %lld, expected %lld\n", table, row, what, (long long)(got), (long long)(want)); \
        failed++;                                                                                                 \
    }

struct PrivateCase {
    int batch;
    std::vector<int> fanout;
    int small_buckets, claim_cap, known_cap, col_slots;      // LegionTuning's fields (col_slots -1: the default, on)
    long long sum;
    int n_entries;
};
static const PrivateCase private_cases[] = {
    // 1, 2, 3 and 6 hops
    {64, {5}, 0, 0, 0, -1, 52480, 14},
    {64, {6, 3}, 0, 0, 0, -1, 163072, 16},
    {64, {4, 3, 2}, 0, 0, 0, -1, 215808, 16},
    {16, {3, 2, 2, 2, 2, 2}, 0, 0, 0, -1, 239104, 16},
    // LG_LDS_SLOTS_SMALL slots (8 buckets), just past it (64), just past LG_LDS_SLOTS_MEDIUM (256: the only class with run_off)
    {1024, {32, 16}, 0, 0, 0, -1, 35908352, 16},
    {1025, {32, 16}, 0, 0, 0, -1, 36288000, 16},
    {1025, {64, 64}, 0, 0, 0, -1, 280093184, 17},
    // LEGION_LDS_SMALL_BUCKETS 8 and 16
    {64, {6, 3}, 8, 0, 0, -1, 163072, 16},
    {64, {6, 3}, 16, 0, 0, -1, 180480, 16},
    // column slots off, with and without known lists
    {64, {6, 3}, 0, 0, 0, 0, 152064, 14},
    {64, {5}, 0, 0, 0, 0, 49664, 12},
    // forced claim and known capacities
    {64, {6, 3}, 0, 300, 0, -1, 130304, 16},
    {64, {6, 3}, 0, 0, 100, -1, 146944, 16},
    // one seed with one neighbour; a batch that is no multiple of 64; B = 1000 with [25,10]
    {1, {1}, 0, 0, 0, -1, 36864, 14},
    {100, {6, 3}, 0, 0, 0, -1, 209664, 16},
    {1000, {25, 10}, 0, 0, 0, -1, 17664000, 16},
};

struct ShapeCase {
    int batch;
    std::vector<int> fanout;
    long long num_ids, max_slots, listed;
    int max_fanout;
    bool over;
};
static const ShapeCase shape_cases[] = {
    {1024, {25, 10}, 282624, 256000, 25600, 25, false},
    {64, {}, 64, 64, 0, 0, false},
    {16, {3, 2, 2}, 16 + 48 + 96 + 192, 192, 48 + 96, 3, false},
    // the limit 2^31 - 16384 = 2147467264: B (1 + 1) with one hop of fan-out 1 on both sides of it
    {1073733631, {1}, 2147467262, 1073733631, 0, 1, false},
    {1073733632, {1}, 2147467264, 1073733632, 0, 1, true},
    // B (1 + f) = 2147467263 = 3 x 715822421, the last shape below the limit
    {715822421, {2}, 2147467263, 1431644842, 0, 2, false},
    // a product beyond 2^32 is formed in int64
    {65536, {256, 256, 2}, 65536LL + 16777216LL + 4294967296LL + 8589934592LL, 8589934592LL, 16777216LL + 4294967296LL, 256, true},
};

struct VisibleCase { long long batch, num_ids, rows, len; int dtype; long long bytes; };
static const VisibleCase visible_cases[] = {
    // 3 x ids + labels + 2 x 256 + rows, each rounded up to 256
    {64, 1600, 1600, 32, LEGION_FEATURE_F32, 3 * 6400 + 256 + 512 + 204800},
    {64, 1600, 1600, 32, LEGION_FEATURE_BF16, 3 * 6400 + 256 + 512 + 102400},
    {64, 1600, 0, 32, LEGION_FEATURE_F32, 3 * 6400 + 256 + 512},
    {100, 1301, 7, 3, LEGION_FEATURE_F32, 3 * 5376 + 512 + 512 + 256},
    {100, 1301, 7, 3, LEGION_FEATURE_BF16, 3 * 5376 + 512 + 512 + 256},
    {1, 2, 100, 8, LEGION_FEATURE_F32, 3 * 256 + 256 + 512 + 3328},
};

int main()
{
    int row = 0;
    const char* table = "private";
    for (const PrivateCase& c : private_cases) {
        const PoolShape s = pool_shape(c.batch, c.fanout.data(), (int)c.fanout.size());
        const int64_t no_hint[2] = {0, 0};
        const PoolPrivatePlan p = pool_private_plan(s, no_hint, c.small_buckets, c.claim_cap, c.known_cap, c.col_slots);
        CHECK("sum", p.sum, c.sum);
        CHECK("entries", p.n, c.n_entries);
        long long again = 0;
        for (int i = 0; i < p.n; i++) {
            again += pool_round(p.entries[i].bytes);
            if (i > 0) CHECK("order", p.entries[i].what > p.entries[i - 1].what, 1);
        }
        CHECK("sum of the entries", again, c.sum);
        CHECK("claim entry", p.bytes_of(PA_CLAIM_PAIRS), (p.sample.claim_chunks * LG_CLAIM_CHUNK << p.sample.bucket_bits) * 8);
        CHECK("known entry", p.bytes_of(PA_KNOWN_PAIRS), ((long long)p.sample.known_cap << p.sample.bucket_bits) * 8);
        CHECK("run_off only with 256 buckets", p.bytes_of(PA_RUN_OFF) > 0, p.sample.bucket_bits == LG_LDS_BITS_LARGE);
        CHECK("column slots", p.bytes_of(PA_NODE_SLOT) > 0, c.col_slots != 0);
        row++;
    }
    row = 0;
    table = "shape";
    for (const ShapeCase& c : shape_cases) {
        const PoolShape s = pool_shape(c.batch, c.fanout.data(), (int)c.fanout.size());
        CHECK("num_ids", s.num_ids, c.num_ids);
        CHECK("max_slots", s.max_slots, c.max_slots);
        CHECK("listed_nodes", s.listed_nodes, c.listed);
        CHECK("max_fanout", s.max_fanout, c.max_fanout);
        CHECK("over_limit", s.over_limit, c.over);
        CHECK("max_new entries", s.max_new.size(), c.fanout.size() + 1);
        CHECK("max_new[last]", s.max_new.back(), c.max_slots);
        row++;
    }
    row = 0;
    table = "visible";
    for (const VisibleCase& c : visible_cases) {
        CHECK("bytes", pool_visible_bytes(c.batch, c.num_ids, c.rows, c.len, c.dtype), c.bytes);
        row++;
    }
    printf("pool_plan_test: %d failed\n", failed);
    return failed ? 1 : 0;
}
