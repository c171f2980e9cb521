// Pins the op order of a mini-batch (legion_amd/csrc/batch_ops.h: batch_op_list, what a phase of a whole-batch enqueue issues, in
// which order, with which op ids and which gathers sharing a launch; batch_whole_gather; gather_row_bound) over a literal table:
// every phase x 0 ... 6 hops x serving / PreSC x CacheProfiling on / off.  An op on the wrong side of the weave cut, or a gather
// launched alone that should carry the seeds' rows, gives the same batch, only slower: no GPU test sees it.  Host-only:
//   g++ -O1 -std=c++17 batch_ops_test.cpp -o t && ./t
#include <cstdio>
#include <cstring>
#include <string>

#include "../../legion_amd/csrc/batch_ops.h"

// One op as text.  S: the seeds (op 0); H<op>f<i>: the sampler op with fan-out fanout[i]; G<op>h<i>: the gather of the rows hop i
// added (h-1: the seeds'), "+<first>" when the earlier ops first, first + 3, ... ride along; P: CacheProfiling; E: end of batch
static std::string text(const BatchOpList& l)
{
    std::string s;
    for (int32_t i = 0; i < l.n; i++) {
        const BatchOp& o = l.op[i];
        char b[64];
        switch (o.kind) {
        case BatchOpKind::Seeds: snprintf(b, sizeof(b), o.op_id == 0 ? "S" : "S?%d", o.op_id); break;
        case BatchOpKind::Sample: snprintf(b, sizeof(b), "H%df%d", o.op_id, o.hop); break;
        case BatchOpKind::Gather:
            if (o.first_op_id >= 0) snprintf(b, sizeof(b), "G%dh%d+%d", o.op_id, o.hop, o.first_op_id);
            else snprintf(b, sizeof(b), "G%dh%d", o.op_id, o.hop);
            break;
        case BatchOpKind::Profile: snprintf(b, sizeof(b), "P"); break;
        case BatchOpKind::EndOfBatch: snprintf(b, sizeof(b), "E"); break;
        default: snprintf(b, sizeof(b), "?"); break;
        }
        if (i) s += ' ';
        s += b;
    }
    return s;
}

// [hop_num]
typedef const char* Lists[7];
static const Lists ALL_SERVING = {
    "S G1h-1 E",
    "S G1h-1 H3f0 G4h0 E",
    "S H3f0 G4h0+1 H6f1 G7h1 E",
    "S H3f0 G4h0+1 H6f1 G7h1 H9f2 G10h2 E",
    "S H3f0 G4h0+1 H6f1 G7h1 H9f2 G10h2 H12f3 G13h3 E",
    "S H3f0 G4h0+1 H6f1 G7h1 H9f2 G10h2 H12f3 G13h3 H15f4 G16h4 E",
    "S H3f0 G4h0+1 H6f1 G7h1 H9f2 G10h2 H12f3 G13h3 H15f4 G16h4 H18f5 G19h5 E",
};
static const Lists SAMPLER = {          // SAMPLE serving; ALL and SAMPLE in PreSC without CacheProfiling
    "S E",
    "S H3f0 E",
    "S H3f0 H6f1 E",
    "S H3f0 H6f1 H9f2 E",
    "S H3f0 H6f1 H9f2 H12f3 E",
    "S H3f0 H6f1 H9f2 H12f3 H15f4 E",
    "S H3f0 H6f1 H9f2 H12f3 H15f4 H18f5 E",
};
static const Lists SAMPLER_PROFILED = {      // ALL and SAMPLE in PreSC with CacheProfiling
    "S P E",
    "S H3f0 P E",
    "S H3f0 H6f1 P E",
    "S H3f0 H6f1 H9f2 P E",
    "S H3f0 H6f1 H9f2 H12f3 P E",
    "S H3f0 H6f1 H9f2 H12f3 H15f4 P E",
    "S H3f0 H6f1 H9f2 H12f3 H15f4 H18f5 P E",
};
static const Lists GATHERS = {
    "G1h-1",
    "G1h-1 G4h0",
    "G4h0+1 G7h1",
    "G4h0+1 G7h1 G10h2",
    "G4h0+1 G7h1 G10h2 G13h3",
    "G4h0+1 G7h1 G10h2 G13h3 G16h4",
    "G4h0+1 G7h1 G10h2 G13h3 G16h4 G19h5",
};
static const Lists NOTHING = {"", "", "", "", "", "", ""};
static const Lists HEAD = {
    "S",
    "S",
    "S H3f0",
    "S H3f0 H6f1",
    "S H3f0 H6f1 H9f2",
    "S H3f0 H6f1 H9f2 H12f3",
    "S H3f0 H6f1 H9f2 H12f3 H15f4",
};
static const Lists REST = {
    "E G1h-1",
    "H3f0 E G1h-1 G4h0",
    "H6f1 E G4h0+1 G7h1",
    "H9f2 E G4h0+1 G7h1 G10h2",
    "H12f3 E G4h0+1 G7h1 G10h2 G13h3",
    "H15f4 E G4h0+1 G7h1 G10h2 G13h3 G16h4",
    "H18f5 E G4h0+1 G7h1 G10h2 G13h3 G16h4 G19h5",
};
static const Lists REST_SAMPLE = {"E", "H3f0 E", "H6f1 E", "H9f2 E", "H12f3 E", "H15f4 E", "H18f5 E"};

// [phase][is_presc][profile]
static const Lists* const WANT[6][2][2] = {
    {{&ALL_SERVING, &ALL_SERVING}, {&SAMPLER, &SAMPLER_PROFILED}},      // LG_PHASE_ALL
    {{&SAMPLER, &SAMPLER}, {&SAMPLER, &SAMPLER_PROFILED}},              // LG_PHASE_SAMPLE
    {{&GATHERS, &GATHERS}, {&NOTHING, &NOTHING}},                       // LG_PHASE_GATHER
    {{&HEAD, &HEAD}, {&HEAD, &HEAD}},                                   // LG_PHASE_HEAD: the weave serves only, the flags are ignored
    {{&REST, &REST}, {&REST, &REST}},                                   // LG_PHASE_REST
    {{&REST_SAMPLE, &REST_SAMPLE}, {&REST_SAMPLE, &REST_SAMPLE}},       // LG_PHASE_REST_SAMPLE
};
static_assert(LG_PHASE_ALL == 0 && LG_PHASE_SAMPLE == 1 && LG_PHASE_GATHER == 2 && LG_PHASE_HEAD == 3 && LG_PHASE_REST == 4 &&
              LG_PHASE_REST_SAMPLE == 5, "the phases index WANT (and are part of legion_enqueue_group_phase's interface)");

struct BoundCase {
    const char* what;
    int32_t n_max_new, op_id, first_op_id;
    bool use_snapshot;
    int64_t feature_rows, num_ids, want;
};
// a pool of B = 8, fan-outs [3, 2]: max_new = {8, 24, 48}, num_ids = 80
static const int64_t MAX_NEW[3] = {8, 24, 48};
static const BoundCase BOUNDS[] = {
    {"no snapshot, op 4", 3, 4, -1, false, 80, 80, 24},
    {"no snapshot ignores first_op_id", 3, 4, 1, false, 80, 80, 24},
    {"snapshot alone, op 1", 3, 1, -1, true, 80, 80, 8},
    {"snapshot alone, op 4", 3, 4, -1, true, 80, 80, 24},
    {"snapshot alone, op 7", 3, 7, -1, true, 80, 80, 48},
    {"the seeds ride with op 4", 3, 4, 1, true, 80, 80, 32},
    {"the whole batch in op 7", 3, 7, 1, true, 80, 80, 80},
    {"ops 4 and 7", 3, 7, 4, true, 80, 80, 72},
    {"first_op_id == op_id", 3, 4, 4, true, 80, 80, 24},
    {"first_op_id > op_id", 3, 4, 7, true, 80, 80, 24},
    {"an op beyond max_new keeps the buffer's rows", 3, 10, -1, true, 60, 80, 60},
    {"an op beyond max_new, riders from op 1", 3, 10, 1, true, 60, 80, 60},
    {"an op beyond a shorter max_new", 2, 7, 1, true, 70, 80, 70},
    {"feature_rows below the bound", 3, 7, -1, true, 40, 80, 40},
    {"feature_rows above the bound", 3, 4, 1, true, 33, 80, 32},
    {"feature_rows equal to the bound", 3, 4, 1, true, 32, 80, 32},
    {"feature_rows above num_ids", 3, 10, -1, true, 500, 80, 80},
    {"feature_rows above num_ids, bound below both", 3, 7, 1, true, 500, 90, 80},
    {"no feature rows", 3, 7, 1, true, 0, 80, 0},
    {"no max_new at all", 0, 4, 1, true, 50, 80, 50},
};

int main()
{
    int n = 0, bad = 0;
    for (int32_t phase = 0; phase < 6; phase++)
        for (int32_t presc = 0; presc < 2; presc++)
            for (int32_t profile = 0; profile < 2; profile++)
                for (int32_t hops = 0; hops <= 6; hops++) {
                    n++;
                    const std::string got = text(batch_op_list(hops, phase, presc != 0, profile != 0));
                    const char* want = (*WANT[phase][presc][profile])[hops];
                    if (got != want) {
                        printf("MISMATCH phase %d hops %d presc %d profile %d: got \"%s\", want \"%s\"\n", phase, hops, presc, profile, got.c_str(), want);
                        bad++;
                    }
                }
    static const int32_t WHOLE_OP[7] = {1, 4, 7, 10, 13, 16, 19};
    for (int32_t hops = 0; hops <= 6; hops++) {
        n++;
        const BatchOp w = batch_whole_gather(hops);
        if (w.kind != BatchOpKind::Gather || w.op_id != WHOLE_OP[hops] || w.first_op_id != 1 || w.hop != hops - 1) {
            printf("MISMATCH whole gather of %d hops: got op %d first %d hop %d, want op %d first 1 hop %d\n", hops, w.op_id, w.first_op_id, w.hop,
                   WHOLE_OP[hops], hops - 1);
            bad++;
        }
    }
    for (const BoundCase& c : BOUNDS) {
        n++;
        const int64_t got = gather_row_bound(MAX_NEW, c.n_max_new, c.op_id, c.first_op_id, c.use_snapshot, c.feature_rows, c.num_ids);
        if (got != c.want) {
            printf("MISMATCH row bound, %s: got %lld, want %lld\n", c.what, (long long)got, (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
