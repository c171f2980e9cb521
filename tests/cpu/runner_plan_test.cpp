// Pins GPURunner's sizing (legion_amd/csrc/runner_plan.h: runner_rows, runner_group_plan) and the schedule's group rule
// (runner_schedule.h: runner_group_at, runner_largest_group) over literal tables.  The expected values were computed from the lines
// the plan replaced in GPURunner::InitializeFeaturesBuffer and ::CreateGroups, kept verbatim in a scratch program, not from the header.
//   g++ -O1 -std=c++17 runner_plan_test.cpp -o t && ./t
#include <cstdio>
#include <vector>

#include "../../legion_amd/csrc/runner_plan.h"
#include "../../legion_amd/csrc/runner_schedule.h"

static int failed = 0;
#define CHECK(what, got, want)                                                                                   \
    if ((long long)(got) != (long long)(want)) {                                                                  \
        printf("MISMATCH %s row %d: %s = %lld, expected %lld\n", table, row, what, (long long)(got), (long long)(want)); \
        failed++;                                                                                                 \
    }

struct GroupCase {
    int batch, num_ids, max_slots, len, dtype, lane_rule_rows;
    long long free_bytes;
    int handover, runner_slots, runner_lanes, runner_overflow, largest_group, pipe_slots;
    int slots, lanes, lane_features, lane_feature_rows;
    long long arena_lane, overflow_bytes, arena_bytes;
};
// B = 1024 with [25,10] unless said: 282624 ids, 256000 slots; 128 float32 features: a worst-case batch is 144703488 bytes of rows, a lane
// of 60000 rows is reckoned at 52589056 bytes, 512 lanes x 3 groups at 80776790016 = 0.6 x 134627983360
static const GroupCase group_cases[] = {
    // lanes caps: 512 and 524288 / B
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 60000, 34116096LL, 144703488LL, 52691730432LL},
    {512, 141312, 128000, 128, 0, 30000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 30000, 17058304LL, 72351744LL, 26346258432LL},
    {2048, 565248, 512000, 128, 0, 120000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 256, 1, 120000, 68231680LL, 289406976LL, 52980744192LL},
    {8000, 2208000, 2000000, 128, 0, 400000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 64, 1, 400000, 231328512LL, 1130496000LL, 46676066304LL},
    {1, 276, 250, 128, 0, 100, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 100, 55808LL, 143360LL, 86007808LL},
    // runner_lanes forced; the largest group below the cap, and below forced lanes
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 3, 48, 1, 1048576, 2,  3, 48, 1, 60000, 34116096LL, 144703488LL, 5202124800LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 3, 0, 1, 100, 2,  3, 100, 1, 60000, 34116096LL, 144703488LL, 10524235776LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 3, 48, 1, 7, 2,  3, 7, 1, 60000, 34116096LL, 144703488LL, 1005844992LL},
    // halvings against free HBM: none (at the edge), one (just below it), one, two, three
    {1024, 282624, 256000, 128, 0, 60000, 134627983360LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 60000, 34116096LL, 144703488LL, 52691730432LL},
    {1024, 282624, 256000, 128, 0, 60000, 134627983350LL, 0, 3, 0, 1, 1048576, 2,  3, 256, 1, 60000, 34116096LL, 144703488LL, 26490568704LL},
    {1024, 282624, 256000, 128, 0, 60000, 100000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 256, 1, 60000, 34116096LL, 144703488LL, 26490568704LL},
    {1024, 282624, 256000, 128, 0, 60000, 50000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 128, 1, 60000, 34116096LL, 144703488LL, 13389987840LL},
    {1024, 282624, 256000, 128, 0, 60000, 25000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 64, 1, 60000, 34116096LL, 144703488LL, 6839697408LL},
    // slots: 2, 3, 5 -> 4, 1 and 0 -> 3
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 2, 0, 1, 1048576, 2,  2, 512, 1, 60000, 34116096LL, 144703488LL, 35224289280LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 5, 0, 1, 1048576, 2,  4, 512, 1, 60000, 34116096LL, 144703488LL, 70159171584LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 4, 0, 1, 1048576, 2,  4, 512, 1, 60000, 34116096LL, 144703488LL, 70159171584LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 1, 0, 1, 1048576, 2,  3, 512, 1, 60000, 34116096LL, 144703488LL, 52691730432LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 0, 0, 1, 1048576, 2,  3, 512, 1, 60000, 34116096LL, 144703488LL, 52691730432LL},
    // overflow refused by the tenth-of-free rule (and at its edge: 2 x 144703488 = free / 10), by the seven-tenths rule, by runner_overflow = 0,
    // by handover = 1, not needed; bf16; no features
    {1024, 282624, 256000, 128, 0, 60000, 2000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 4, 1, 60000, 34116096LL, 0LL, 409393152LL},
    {1024, 282624, 256000, 128, 0, 60000, 2894069760LL, 0, 3, 0, 1, 1048576, 2,  3, 8, 1, 60000, 34116096LL, 144703488LL, 1108193280LL},
    {1024, 282624, 256000, 128, 0, 60000, 2894069759LL, 0, 3, 0, 1, 1048576, 2,  3, 8, 1, 60000, 34116096LL, 0LL, 818786304LL},
    {1024, 282624, 256000, 1, 0, 60000, 50000000LL, 0, 3, 0, 1, 1048576, 2,  3, 1, 1, 60000, 3636224LL, 0LL, 10908672LL},
    {1024, 282624, 256000, 1, 0, 60000, 200000000LL, 0, 3, 0, 1, 1048576, 2,  3, 1, 1, 60000, 3636224LL, 1130496LL, 13169664LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 0, 3, 0, 0, 1048576, 2,  3, 512, 1, 60000, 34116096LL, 0LL, 52402323456LL},
    {1024, 282624, 256000, 128, 0, 60000, 200000000000LL, 1, 3, 0, 1, 1048576, 2,  3, 512, 0, 0, 3396096LL, 0LL, 5216403456LL},
    {1024, 282624, 256000, 128, 0, 282624, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 128, 1, 282624, 148099584LL, 0LL, 56870240256LL},
    {1024, 282624, 256000, 128, 0, 282629, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 128, 1, 282624, 148099584LL, 0LL, 56870240256LL},
    {1024, 282624, 256000, 128, 1, 60000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 60000, 18756096LL, 72351744LL, 28954066944LL},
    {1024, 282624, 256000, 0, 0, 60000, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 0, 0, 3396096LL, 0LL, 5216403456LL},
    {1024, 282624, 256000, 128, 0, 0, 200000000000LL, 0, 3, 0, 1, 1048576, 2,  3, 512, 1, 1, 3396608LL, 144703488LL, 5506596864LL},
};

struct RowsCase {
    int presc_max_ids, batch, raw_batch, num_ids, len, dtype;
    long long free_bytes;
    int pipe_slots, runner_overflow;
    int lane_rule_rows;
    long long slot_rows;
};
static const RowsCase rows_cases[] = {
    // a validation batch 1, 2 and 3 times the raw batch, and one past the raw batch
    {50000, 1024, 1024, 282624, 128, 0, 200000000000LL, 2, 1,  60000, 282624LL},
    {50000, 2048, 1024, 565248, 128, 0, 200000000000LL, 2, 1,  120000, 565248LL},
    {50000, 3072, 1024, 847872, 128, 0, 200000000000LL, 2, 1,  180000, 847872LL},
    {50000, 1025, 1024, 282900, 128, 0, 200000000000LL, 2, 1,  120000, 282900LL},
    {33333, 1024, 1024, 282624, 128, 0, 200000000000LL, 2, 1,  39999, 282624LL},
    // clamped at num_ids, floored at 1
    {250000, 1024, 1024, 282624, 128, 0, 200000000000LL, 2, 1,  282624, 282624LL},
    {150000, 2048, 1024, 300000, 128, 0, 200000000000LL, 2, 1,  300000, 300000LL},
    {0, 1024, 1024, 282624, 128, 0, 200000000000LL, 2, 1,  1, 282624LL},
    // the pipe slots: worst case at the edge of a tenth of free HBM, the rule below it, the rule with runner_overflow = 0; bf16 halves the pair
    {50000, 1024, 1024, 282624, 128, 0, 2894069760LL, 2, 1,  60000, 282624LL},
    {50000, 1024, 1024, 282624, 128, 0, 2894069759LL, 2, 1,  60000, 60000LL},
    {50000, 1024, 1024, 282624, 128, 0, 200000000000LL, 2, 0,  60000, 60000LL},
    {50000, 1024, 1024, 282624, 128, 1, 1447034880LL, 2, 1,  60000, 282624LL},
    {50000, 1024, 1024, 282624, 128, 1, 1447034879LL, 2, 1,  60000, 60000LL},
};

// a schedule: five training batches, three validation batches, then training batches with local ids 5 and 7 (a gap)
static const int sched_mode[] = {0, 0, 0, 0, 0, 1, 1, 1, 0, 0};
static const int sched_local[] = {0, 1, 2, 3, 4, 0, 1, 2, 5, 7};
struct GroupAt { int first, cap, max_step, n, mode, local0; };
static const GroupAt group_at_cases[] = {
    {0, 4, 10, 4, 0, 0},      // the cap
    {4, 4, 10, 1, 0, 4},      // the mode changes at 5
    {0, 8, 10, 5, 0, 0},
    {5, 4, 10, 3, 1, 0},      // ... and back at 8
    {5, 4, 7, 2, 1, 0},       // never past max_step
    {8, 4, 10, 1, 0, 5},      // a gap in the local ids
    {9, 4, 10, 1, 0, 7},
    {3, 1, 10, 1, 0, 3},
};
struct Largest { int cap, max_step, best; };
static const Largest largest_cases[] = {{1, 10, 1}, {2, 10, 2}, {4, 10, 4}, {5, 10, 5}, {8, 10, 5}, {512, 10, 5}, {512, 3, 3}, {512, 0, 1}, {3, 8, 3}};

int main()
{
    int row = 0;
    const char* table = "groups";
    for (const GroupCase& c : group_cases) {
        int asked_cap = -1;
        const RunnerGroupPlan p = runner_group_plan(c.batch, c.num_ids, c.max_slots, c.len, c.dtype, c.lane_rule_rows, c.free_bytes, c.handover, c.runner_slots,
                                                    c.runner_lanes, c.runner_overflow, [&](int32_t cap) { asked_cap = cap; return c.largest_group; }, c.pipe_slots);
        CHECK("slots", p.slots, c.slots);
        CHECK("lanes", p.lanes, c.lanes);
        CHECK("lane_features", p.lane_features, c.lane_features);
        CHECK("lane_feature_rows", p.lane_feature_rows, c.lane_feature_rows);
        CHECK("arena_lane", p.arena_lane, c.arena_lane);
        CHECK("overflow_bytes", p.overflow_bytes, c.overflow_bytes);
        CHECK("arena_bytes", p.arena_bytes, c.arena_bytes);
        CHECK("arena_bytes is lanes and overflow buffers", p.arena_bytes, p.arena_lane * p.lanes * p.slots + c.pipe_slots * p.overflow_bytes);
        CHECK("the schedule is asked with the cap before the halvings", asked_cap >= p.lanes, 1);
        row++;
    }
    row = 0;
    table = "rows";
    for (const RowsCase& c : rows_cases) {
        const RunnerRows r = runner_rows(c.presc_max_ids, c.batch, c.raw_batch, c.num_ids, c.len, c.dtype, c.free_bytes, c.pipe_slots, c.runner_overflow);
        CHECK("lane_rule_rows", r.lane_rule_rows, c.lane_rule_rows);
        CHECK("slot_rows", r.slot_rows, c.slot_rows);
        row++;
    }
    auto mode_of = [](int32_t k) { return sched_mode[k]; };
    auto local_of = [](int32_t k) { return sched_local[k]; };
    row = 0;
    table = "group_at";
    for (const GroupAt& c : group_at_cases) {
        int32_t mode = -1, local0 = -1;
        CHECK("n", runner_group_at(c.first, c.cap, c.max_step, mode_of, local_of, mode, local0), c.n);
        CHECK("mode", mode, c.mode);
        CHECK("local0", local0, c.local0);
        row++;
    }
    row = 0;
    table = "largest";
    for (const Largest& c : largest_cases) {
        CHECK("best", runner_largest_group(c.cap, c.max_step, mode_of, local_of), c.best);
        row++;
    }
    // the estimate the halvings use is NOT the exact plan's sum
    table = "estimate";
    CHECK("lane estimate", runner_lane_private_estimate(282624, 256000), 282624LL * 40 + 256000LL * 28);
    printf("runner_plan_test: %d failed\n", failed);
    return failed ? 1 : 0;
}
