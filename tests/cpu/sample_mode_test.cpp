// Pins the sampler's mode rules (legion_amd/csrc/sample_mode.h: sample_mode_refusal, what a pool may be set to; sample_launch_refusal,
// what a launch needs on top; SampleMode::draw, the kernel instance a mode picks) over a literal table: all eight (replace, edge_ids,
// weighted) combinations at fan-outs 1, LG_DISTINCT_MAX_FANOUT and one above, against a graph with and without a prefix table, and
// values outside {0, 1}.  The expected codes were written down from the rules as include/legion_hip.h documents them, not from the header.
//   g++ -O1 -std=c++17 sample_mode_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/sample_mode.h"

static_assert(LG_DISTINCT_MAX_FANOUT == 256, "the table below spells the fan-outs out");
enum { OK, BAD, WNR, FAN, TAB };      // ok, bad value, weighted needs replacement, fan-out above 256 without replacement, no prefix table
enum { U, D, W };                     // draw(): uniform, distinct, weighted

struct Case { int replace, edge_ids, weighted, fanout, table; int mode_code, launch_code, draw; };
static const Case cases[] = {
    // replace, edge_ids, weighted, fan-out, graph has a table -> pool setter, launch, draw
    // with replacement, uniform: anything goes, at any fan-out, table or not
    {1, 0, 0, 1, 0,  OK, OK, U}, {1, 0, 0, 256, 0,  OK, OK, U}, {1, 0, 0, 257, 0,  OK, OK, U},
    {1, 0, 0, 1, 1,  OK, OK, U}, {1, 0, 0, 256, 1,  OK, OK, U}, {1, 0, 0, 257, 1,  OK, OK, U},
    {1, 1, 0, 1, 0,  OK, OK, U}, {1, 1, 0, 256, 0,  OK, OK, U}, {1, 1, 0, 257, 0,  OK, OK, U},
    {1, 1, 0, 1, 1,  OK, OK, U}, {1, 1, 0, 256, 1,  OK, OK, U}, {1, 1, 0, 257, 1,  OK, OK, U},
    // without replacement: fan-outs up to 256, edge ids or not, table or not
    {0, 0, 0, 1, 0,  OK, OK, D}, {0, 0, 0, 256, 0,  OK, OK, D}, {0, 0, 0, 257, 0,  FAN, FAN, D},
    {0, 0, 0, 1, 1,  OK, OK, D}, {0, 0, 0, 256, 1,  OK, OK, D}, {0, 0, 0, 257, 1,  FAN, FAN, D},
    {0, 1, 0, 1, 0,  OK, OK, D}, {0, 1, 0, 256, 0,  OK, OK, D}, {0, 1, 0, 257, 0,  FAN, FAN, D},
    {0, 1, 0, 1, 1,  OK, OK, D}, {0, 1, 0, 256, 1,  OK, OK, D}, {0, 1, 0, 257, 1,  FAN, FAN, D},
    // weighted with replacement: a pool may be set to it at any fan-out; a launch needs the graph's table
    {1, 0, 1, 1, 0,  OK, TAB, W}, {1, 0, 1, 256, 0,  OK, TAB, W}, {1, 0, 1, 257, 0,  OK, TAB, W},
    {1, 0, 1, 1, 1,  OK, OK, W}, {1, 0, 1, 256, 1,  OK, OK, W}, {1, 0, 1, 257, 1,  OK, OK, W},
    {1, 1, 1, 1, 0,  OK, TAB, W}, {1, 1, 1, 256, 0,  OK, TAB, W}, {1, 1, 1, 257, 0,  OK, TAB, W},
    {1, 1, 1, 1, 1,  OK, OK, W}, {1, 1, 1, 256, 1,  OK, OK, W}, {1, 1, 1, 257, 1,  OK, OK, W},
    // weighted without replacement: never, whatever the fan-out and the table (draw() of a refused mode is not asked)
    {0, 0, 1, 1, 0,  WNR, WNR, -1}, {0, 0, 1, 256, 0,  WNR, WNR, -1}, {0, 0, 1, 257, 0,  WNR, WNR, -1},
    {0, 0, 1, 1, 1,  WNR, WNR, -1}, {0, 0, 1, 256, 1,  WNR, WNR, -1}, {0, 0, 1, 257, 1,  WNR, WNR, -1},
    {0, 1, 1, 1, 0,  WNR, WNR, -1}, {0, 1, 1, 256, 0,  WNR, WNR, -1}, {0, 1, 1, 257, 0,  WNR, WNR, -1},
    {0, 1, 1, 1, 1,  WNR, WNR, -1}, {0, 1, 1, 256, 1,  WNR, WNR, -1}, {0, 1, 1, 257, 1,  WNR, WNR, -1},
    // a value outside {0, 1} in any field, before any other rule
    {2, 0, 0, 1, 1,  BAD, BAD, -1}, {-1, 0, 0, 1, 1,  BAD, BAD, -1}, {1, 2, 0, 1, 1,  BAD, BAD, -1}, {1, -1, 0, 1, 1,  BAD, BAD, -1},
    {1, 0, 2, 1, 1,  BAD, BAD, -1}, {1, 0, -1, 1, 1,  BAD, BAD, -1}, {2, 0, 1, 257, 0,  BAD, BAD, -1}, {0, 0, 2, 257, 0,  BAD, BAD, -1},
};

static int code(SampleRefusal r)
{
    switch (r) {
    case SampleRefusal::Ok: return OK;
    case SampleRefusal::BadValue: return BAD;
    case SampleRefusal::WeightedNeedsReplace: return WNR;
    case SampleRefusal::Fanout: return FAN;
    case SampleRefusal::NoTable: return TAB;
    default: return -1;
    }
}
static int code(SampleDraw d) { return d == SampleDraw::Uniform ? U : d == SampleDraw::Distinct ? D : W; }

int main()
{
    int bad = 0, n = 0;
    for (const Case& c : cases) {
        n++;
        SampleMode m;
        m.replace = c.replace; m.edge_ids = c.edge_ids; m.weighted = c.weighted;
        const int mc = code(sample_mode_refusal(m, c.fanout)), lc = code(sample_launch_refusal(m, c.fanout, c.table != 0));
        const int dr = c.draw < 0 ? -1 : code(m.draw());
        if (mc != c.mode_code || lc != c.launch_code || dr != c.draw) {
            printf("MISMATCH replace %d edge_ids %d weighted %d fan-out %d table %d: got mode %d launch %d draw %d, want mode %d launch %d draw %d\n",
                   c.replace, c.edge_ids, c.weighted, c.fanout, c.table, mc, lc, dr, c.mode_code, c.launch_code, c.draw);
            bad++;
        }
        SampleMode other = m;
        other.edge_ids = !m.edge_ids;
        if (!(m == m) || m == other || !(m != other)) { printf("MISMATCH ==: replace %d edge_ids %d weighted %d\n", c.replace, c.edge_ids, c.weighted); bad++; }
        if (sample_refusal_text(sample_launch_refusal(m, c.fanout, c.table != 0))[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    // the default mode is the reference's: with replacement, nothing else
    if (!(SampleMode{} == SampleMode{1, 0, 0})) { printf("MISMATCH default mode\n"); bad++; }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
