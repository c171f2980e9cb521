// Pins the argument rules of random walks and of PinSAGE's neighbour sampler (legion_amd/csrc/walk_rule.h: walk_refusal and
// pinsage_refusal, which calls legion_random_walk and legion_pinsage_neighbors refuse) over a literal table.  The expected codes were
// written down from the checks the two entry points made inline before the header existed, in their order, not from the header -- but
// for the entries with a base of 2^63 - 1: there the inline sum base + count * per left int64 (undefined), and the code expected is the
// rule's as include/legion_hip.h words it, a draw index past 2^31 - 1.  The header asks base > 2^31 - 1 before it forms the sum.
//   g++ -O1 -std=c++17 walk_rule_test.cpp -o t && ./t
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../legion_amd/csrc/walk_rule.h"

static_assert(LEGION_PINSAGE_MAX_VISITS == 1024, "the table below spells the limit out");
enum { OK, CNT, VIS, IDX, WGT, TAB, PRB };

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();
static const float Above1 = std::nextafter(1.0f, 2.0f), BelowZero = -std::numeric_limits<float>::denorm_min();
static const int32_t I31 = 2147483647;
static const int64_t M31 = 2147483647, P62 = (int64_t)1 << 62, I63 = std::numeric_limits<int64_t>::max();

struct WalkCase { int32_t n, length; int64_t base; int32_t weighted, table; float prob; int want; };
static const WalkCase walks[] = {
    // walks, length, base, weighted, graph has a table, restart_prob -> code
    {8, 4, 0, 0, 0, 0.0f, OK}, {8, 4, 0, 1, 1, 0.5f, OK}, {8, 4, 0, 0, 1, 0.25f, OK},
    // counts at -1, 0 and 1, length at 0 and 1, base at -1
    {-1, 4, 0, 0, 0, 0.0f, CNT}, {0, 4, 0, 0, 0, 0.0f, OK}, {1, 4, 0, 0, 0, 0.0f, OK}, {8, 0, 0, 0, 0, 0.0f, CNT}, {8, 1, 0, 0, 0, 0.0f, OK},
    {8, -2, 0, 0, 0, 0.0f, CNT}, {8, 4, -1, 0, 0, 0.0f, CNT}, {0, 0, 0, 0, 0, 0.0f, CNT},
    // the draw index: its last legal value, one past it, far past it (num_walks * length near 2^62)
    {8, 4, M31 - 32, 0, 0, 0.0f, OK}, {8, 4, M31 - 31, 0, 0, 0.0f, IDX}, {0, 4, M31, 0, 0, 0.0f, OK}, {0, 4, M31 + 1, 0, 0, 0.0f, IDX},
    {I31, 1, 0, 0, 0, 0.0f, OK}, {I31, 1, 1, 0, 0, 0.0f, IDX}, {I31, 2, 0, 0, 0, 0.0f, IDX}, {1, I31, 0, 0, 0, 0.0f, OK}, {1, I31, 1, 0, 0, 0.0f, IDX},
    {I31, I31, 0, 0, 0, 0.0f, IDX}, {I31, I31, M31, 0, 0, 0.0f, IDX}, {I31, I31, P62 - 1, 0, 0, 0.0f, IDX}, {8, 4, P62, 0, 0, 0.0f, IDX},
    {1, 1, I63, 0, 0, 0.0f, IDX}, {I31, I31, I63, 0, 0, 0.0f, IDX},      // (as the rule reads: the sum itself is past int64)
    // weighted at -1, 2, and 1 without a table
    {8, 4, 0, -1, 1, 0.0f, WGT}, {8, 4, 0, 2, 1, 0.0f, WGT}, {8, 4, 0, 1, 0, 0.0f, TAB}, {0, 4, 0, 1, 0, 0.0f, TAB},
    // restart_prob: [0, 1] as a float
    {8, 4, 0, 0, 0, -0.0f, OK}, {8, 4, 0, 0, 0, 1.0f, OK}, {8, 4, 0, 0, 0, Above1, PRB}, {8, 4, 0, 0, 0, BelowZero, PRB},
    {8, 4, 0, 0, 0, NaN, PRB}, {8, 4, 0, 0, 0, Inf, PRB}, {8, 4, 0, 0, 0, -Inf, PRB}, {0, 4, 0, 0, 0, NaN, PRB},
    // the order of the checks: the first rule that fails names the refusal
    {-1, 4, M31, 2, 0, NaN, CNT}, {8, 4, M31, 2, 0, NaN, IDX}, {8, 4, 0, 2, 0, NaN, WGT}, {8, 4, 0, 1, 0, NaN, TAB}, {8, 4, 0, 0, 0, NaN, PRB},
};

struct PinsageCase { int32_t n, R, T, K; int64_t base; int32_t weighted, table; float prob; int want; };
static const PinsageCase pinsages[] = {
    // seeds, walks per seed, walk length, num_neighbors, base, weighted, graph has a table, termination_prob -> code
    {8, 4, 3, 10, 0, 0, 0, 0.5f, OK}, {8, 4, 3, 10, 0, 1, 1, 0.0f, OK}, {0, 4, 3, 10, 0, 0, 0, 1.0f, OK}, {1, 1, 1, 1, 0, 0, 0, -0.0f, OK},
    // counts
    {-1, 4, 3, 10, 0, 0, 0, 0.5f, CNT}, {8, 0, 3, 10, 0, 0, 0, 0.5f, CNT}, {8, 4, 0, 10, 0, 0, 0, 0.5f, CNT}, {8, 4, 3, 0, 0, 0, 0, 0.5f, CNT},
    {8, 4, 3, 10, -1, 0, 0, 0.5f, CNT}, {8, -4, -3, 10, 0, 0, 0, 0.5f, CNT},
    // visits at 1024 and 1025, num_neighbors at 1024 and 1025
    {8, 32, 32, 10, 0, 0, 0, 0.5f, OK}, {8, 1024, 1, 10, 0, 0, 0, 0.5f, OK}, {8, 1025, 1, 10, 0, 0, 0, 0.5f, VIS}, {8, 1, 1025, 10, 0, 0, 0, 0.5f, VIS},
    {8, 33, 32, 10, 0, 0, 0, 0.5f, VIS}, {8, I31, I31, 10, 0, 0, 0, 0.5f, VIS}, {8, 4, 3, 1024, 0, 0, 0, 0.5f, OK}, {8, 4, 3, 1025, 0, 0, 0, 0.5f, VIS},
    // base above 2^31 - 1 alone; num_seeds * visits at its edge
    {0, 1, 1, 1, M31, 0, 0, 0.5f, OK}, {0, 1, 1, 1, M31 + 1, 0, 0, 0.5f, IDX}, {8, 4, 3, 10, I63, 0, 0, 0.5f, IDX},
    {2097151, 32, 32, 10, 1023, 0, 0, 0.5f, OK}, {2097151, 32, 32, 10, 1024, 0, 0, 0.5f, IDX}, {2097152, 32, 32, 10, 0, 0, 0, 0.5f, IDX},
    {I31, 1, 1, 1, 0, 0, 0, 0.5f, OK}, {I31, 1, 1, 1, 1, 0, 0, 0.5f, IDX}, {I31, 32, 32, 1, 0, 0, 0, 0.5f, IDX}, {I31, 32, 32, 1, I63, 0, 0, 0.5f, IDX},
    // weighted and the probability
    {8, 4, 3, 10, 0, -1, 1, 0.5f, WGT}, {8, 4, 3, 10, 0, 2, 1, 0.5f, WGT}, {8, 4, 3, 10, 0, 1, 0, 0.5f, TAB},
    {8, 4, 3, 10, 0, 0, 0, Above1, PRB}, {8, 4, 3, 10, 0, 0, 0, BelowZero, PRB}, {8, 4, 3, 10, 0, 0, 0, NaN, PRB}, {8, 4, 3, 10, 0, 0, 0, -Inf, PRB},
    // the order of the checks
    {-1, 1025, 1, 10, M31 + 1, 2, 0, NaN, CNT}, {8, 1025, 1, 10, M31 + 1, 2, 0, NaN, VIS}, {8, 4, 3, 10, M31 + 1, 2, 0, NaN, IDX},
    {8, 4, 3, 10, 0, 2, 0, NaN, WGT}, {8, 4, 3, 10, 0, 1, 0, NaN, TAB}, {8, 4, 3, 10, 0, 0, 0, NaN, PRB},
};

static int code(WalkRefusal r)
{
    switch (r) {
    case WalkRefusal::Ok: return OK;
    case WalkRefusal::Count: return CNT;
    case WalkRefusal::Visits: return VIS;
    case WalkRefusal::DrawIndex: return IDX;
    case WalkRefusal::Weighted: return WGT;
    case WalkRefusal::NoTable: return TAB;
    case WalkRefusal::Prob: return PRB;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const WalkCase& c : walks) {
        n++;
        const WalkRefusal r = walk_refusal(c.n, c.length, c.base, c.weighted, c.table != 0, c.prob);
        if (code(r) != c.want) {
            printf("MISMATCH walk: walks %d length %d base %lld weighted %d table %d prob %g: got %d, want %d\n", c.n, c.length, (long long)c.base,
                   c.weighted, c.table, (double)c.prob, code(r), c.want);
            bad++;
        }
        if (walk_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const PinsageCase& c : pinsages) {
        n++;
        const WalkRefusal r = pinsage_refusal(c.n, c.R, c.T, c.K, c.base, c.weighted, c.table != 0, c.prob);
        if (code(r) != c.want) {
            printf("MISMATCH pinsage: seeds %d walks %d length %d neighbors %d base %lld weighted %d table %d prob %g: got %d, want %d\n", c.n, c.R,
                   c.T, c.K, (long long)c.base, c.weighted, c.table, (double)c.prob, code(r), c.want);
            bad++;
        }
        if (walk_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
