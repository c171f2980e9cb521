// Pins the rule of metapath walks and of PinSAGE over a metapath (legion_amd/csrc/metapath_rule.h) over literal tables: every refusal at
// and beside its edge and their order, as include/legion_hip.h lists them (counts, period, visits, draw index, untyped graph, metapath
// entry, probability, null pointers); the period index and how the metapath travels at L in {1, 2, 3, 64}; where PinSAGE's termination
// draw and its visit fall at L in {1, 3}; the pick inside a segment.
//   g++ -O1 -std=c++17 -I include metapath_rule_test.cpp -o t && ./t
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../../legion_amd/csrc/metapath_rule.h"

static_assert(LEGION_METAPATH_MAX_PERIOD == 64 && LEGION_PINSAGE_MAX_VISITS == 1024, "the tables below spell the limits out");
enum { OK, CNT, PER, VIS, IDX, UNT, TYP, PRB, PTR };

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Above1 = std::nextafter(1.0f, 2.0f);
static const int32_t I31 = 2147483647;
static const int64_t M31 = 2147483647, I63 = std::numeric_limits<int64_t>::max();
static const uint8_t P01[64] = {0, 1}, P3[64] = {0, 3, 0}, P63[64] = {63, 0, 63};      // (the rest zeros)

struct WalkCase { int32_t n; const uint8_t* path; int32_t L, length; int64_t base; int32_t T; float prob; int ptrs, want; };
static const WalkCase walks[] = {
    // walks, metapath, period, length, base, the graph's types, restart_prob, pointers given -> code
    {8, P01, 2, 4, 0, 2, 0.0f, 1, OK}, {8, P01, 2, 100, 0, 64, 0.5f, 1, OK}, {0, P01, 2, 4, 0, 2, 0.0f, 1, OK}, {8, P01, 1, 1, 0, 1, 1.0f, 1, OK},
    // counts
    {-1, P01, 2, 4, 0, 2, 0.0f, 1, CNT}, {8, P01, 2, 0, 0, 2, 0.0f, 1, CNT}, {8, P01, 2, 4, -1, 2, 0.0f, 1, CNT},
    // the period at 0, 1, 64 and 65 (longer than the walk is legal: the tail goes unused)
    {8, P01, 0, 4, 0, 2, 0.0f, 1, PER}, {8, P01, -1, 4, 0, 2, 0.0f, 1, PER}, {8, P01, 64, 4, 0, 2, 0.0f, 1, OK}, {8, P01, 65, 4, 0, 2, 0.0f, 1, PER},
    // the draw index
    {8, P01, 2, 4, M31 - 32, 2, 0.0f, 1, OK}, {8, P01, 2, 4, M31 - 31, 2, 0.0f, 1, IDX}, {I31, P01, 1, 1, 0, 2, 0.0f, 1, OK},
    {I31, P01, 1, 1, 1, 2, 0.0f, 1, IDX}, {I31, P01, 2, I31, I63, 2, 0.0f, 1, IDX}, {0, P01, 2, 4, M31 + 1, 2, 0.0f, 1, IDX},
    // an untyped (or null) graph; a metapath entry at T - 1 and T
    {8, P01, 2, 4, 0, 0, 0.0f, 1, UNT}, {8, P01, 2, 4, 0, 1, 0.0f, 1, TYP}, {8, P01, 1, 4, 0, 1, 0.0f, 1, OK}, {8, P3, 3, 4, 0, 3, 0.0f, 1, TYP},
    {8, P3, 3, 4, 0, 4, 0.0f, 1, OK}, {8, P3, 1, 4, 0, 1, 0.0f, 1, OK}, {8, P63, 3, 4, 0, 64, 0.0f, 1, OK}, {8, P63, 3, 4, 0, 63, 0.0f, 1, TYP},
    // the probability; null pointers (the metapath among them)
    {8, P01, 2, 4, 0, 2, Above1, 1, PRB}, {8, P01, 2, 4, 0, 2, NaN, 1, PRB}, {8, P01, 2, 4, 0, 2, -1.0f, 1, PRB}, {8, P01, 2, 4, 0, 2, -0.0f, 1, OK},
    {8, P01, 2, 4, 0, 2, 0.0f, 0, PTR}, {8, nullptr, 2, 4, 0, 2, 0.0f, 1, PTR}, {0, nullptr, 2, 4, 0, 2, 0.0f, 1, PTR},
    // the order: the first rule that fails names the refusal
    {-1, nullptr, 65, 4, M31 + 1, 0, NaN, 0, CNT}, {8, nullptr, 65, 4, M31 + 1, 0, NaN, 0, PER}, {8, nullptr, 2, 4, M31 + 1, 0, NaN, 0, IDX},
    {8, P3, 2, 4, 0, 0, NaN, 0, UNT}, {8, P3, 2, 4, 0, 2, NaN, 0, TYP}, {8, P01, 2, 4, 0, 2, NaN, 0, PRB}, {8, nullptr, 2, 4, 0, 2, NaN, 1, PRB},
};

struct PinsageCase { int32_t n; const uint8_t* path; int32_t L, R, Q, K; int64_t base; int32_t T; float prob; int ptrs, want; };
static const PinsageCase pinsages[] = {
    // seeds, metapath, period, walks per seed, traversals, num_neighbors, base, types, termination_prob, pointers -> code
    {8, P01, 2, 4, 3, 10, 0, 2, 0.5f, 1, OK}, {0, P01, 2, 4, 3, 10, 0, 2, 0.0f, 1, OK}, {1, P01, 1, 1, 1, 1, 0, 1, 1.0f, 1, OK},
    {-1, P01, 2, 4, 3, 10, 0, 2, 0.5f, 1, CNT}, {8, P01, 2, 0, 3, 10, 0, 2, 0.5f, 1, CNT}, {8, P01, 2, 4, 0, 10, 0, 2, 0.5f, 1, CNT},
    {8, P01, 2, 4, 3, 0, 0, 2, 0.5f, 1, CNT}, {8, P01, 2, 4, 3, 10, -1, 2, 0.5f, 1, CNT},
    {8, P01, 0, 4, 3, 10, 0, 2, 0.5f, 1, PER}, {8, P01, 64, 4, 3, 10, 0, 2, 0.5f, 1, OK}, {8, P01, 65, 4, 3, 10, 0, 2, 0.5f, 1, PER},
    // visits are R * Q, whatever the period: 1024 and 1025; num_neighbors at 1024 and 1025
    {8, P01, 64, 32, 32, 10, 0, 2, 0.5f, 1, OK}, {8, P01, 1, 33, 32, 10, 0, 2, 0.5f, 1, VIS}, {8, P01, 2, 1, 1025, 10, 0, 2, 0.5f, 1, VIS},
    {8, P01, 2, I31, I31, 10, 0, 2, 0.5f, 1, VIS}, {8, P01, 2, 4, 3, 1024, 0, 2, 0.5f, 1, OK}, {8, P01, 2, 4, 3, 1025, 0, 2, 0.5f, 1, VIS},
    // the draw index counts every step: n * R * Q * L
    {32767, P01, 64, 32, 32, 10, 65535, 2, 0.5f, 1, OK}, {32767, P01, 64, 32, 32, 10, 65536, 2, 0.5f, 1, IDX}, {32768, P01, 64, 32, 32, 10, 0, 2, 0.5f, 1, IDX},
    {I31, P01, 1, 1, 1, 1, 0, 2, 0.5f, 1, OK}, {I31, P01, 2, 1, 1, 1, 0, 2, 0.5f, 1, IDX}, {I31, P01, 64, 32, 32, 1, I63, 2, 0.5f, 1, IDX},
    {8, P01, 2, 4, 3, 10, 0, 0, 0.5f, 1, UNT}, {8, P01, 2, 4, 3, 10, 0, 1, 0.5f, 1, TYP}, {8, P01, 2, 4, 3, 10, 0, 2, NaN, 1, PRB},
    {8, P01, 2, 4, 3, 10, 0, 2, Above1, 1, PRB}, {8, P01, 2, 4, 3, 10, 0, 2, 0.5f, 0, PTR}, {8, nullptr, 2, 4, 3, 10, 0, 2, 0.5f, 1, PTR},
    // the order
    {-1, nullptr, 65, 1025, 1, 10, M31 + 1, 0, NaN, 0, CNT}, {8, nullptr, 65, 1025, 1, 10, M31 + 1, 0, NaN, 0, PER},
    {8, nullptr, 2, 1025, 1, 10, M31 + 1, 0, NaN, 0, VIS}, {8, nullptr, 2, 4, 3, 10, M31 + 1, 0, NaN, 0, IDX}, {8, P3, 2, 4, 3, 10, 0, 0, NaN, 0, UNT},
    {8, P3, 2, 4, 3, 10, 0, 2, NaN, 0, TYP}, {8, P01, 2, 4, 3, 10, 0, 2, NaN, 0, PRB}, {8, P01, 2, 4, 3, 10, 0, 2, 0.5f, 0, PTR},
};

static int bad = 0, cases = 0;
static void expect(bool ok, const char* what, long long a, long long b)
{
    cases++;
    if (!ok) { printf("MISMATCH %s: %lld %lld\n", what, a, b); bad++; }
}

int main()
{
    for (const WalkCase& c : walks) {
        const MetapathRefusal r = metapath_walk_refusal(c.n, c.path, c.L, c.length, c.base, c.T, c.prob, c.ptrs != 0);
        expect((int)r == c.want, "walk refusal: case, got", (long long)(&c - walks), (int)r);
        expect(metapath_refusal_text(r)[0] != 0, "a reason without a text", (int)r, 0);
    }
    for (const PinsageCase& c : pinsages) {
        const MetapathRefusal r = pinsage_metapath_refusal(c.n, c.path, c.L, c.R, c.Q, c.K, c.base, c.T, c.prob, c.ptrs != 0);
        expect((int)r == c.want, "pinsage refusal: case, got", (long long)(&c - pinsages), (int)r);
    }
    // the period index: the running index is the modulo, and the packed words give back every entry
    for (int32_t L : {1, 2, 3, 64}) {
        uint8_t path[64];
        for (int32_t i = 0; i < L; i++) path[i] = (uint8_t)((i * 37 + 5) % 64);
        const MetapathWords w = metapath_pack(path, L);
        int32_t run = 0;
        for (int64_t j = 1; j <= 200; j++, run = metapath_next(run, L)) {
            expect(metapath_index(j, L) == run && run == (int32_t)((j - 1) % L), "period index at L, j", L, j);
            expect(metapath_type(w, run) == path[(j - 1) % L], "type at L, j", L, j);
        }
        for (int32_t i = L; i < 64; i++) expect(metapath_type(w, i) == 0, "an unused entry", L, i);
    }
    // PinSAGE: at L = 1 the draw comes before every step but the first and every step is a visit (legion_pinsage_neighbors); at L = 3
    // the draw before steps 4, 7, ... and the visit at steps 3, 6, ...
    for (int32_t j = 1; j <= 12; j++) {
        expect(metapath_terminates_before(j, 1) == (j > 1) && metapath_visit_at(j, 1), "L = 1 at step", j, 0);
        expect(metapath_terminates_before(j, 3) == (j == 4 || j == 7 || j == 10), "the termination draw, L = 3, at step", j, 0);
        expect(metapath_visit_at(j, 3) == (j == 3 || j == 6 || j == 9 || j == 12), "the visit, L = 3, at step", j, 0);
    }
    // the pick: the segment's first entry at r = 0, its last just below 1, never hi
    expect(metapath_pick(5, 9, 0.0) == 5 && metapath_pick(5, 9, 0.25) == 6 && metapath_pick(5, 9, std::nextafter(1.0, 0.0)) == 8, "pick in [5, 9)", 0, 0);
    expect(metapath_pick(70000, 70001, 0.999) == 70000 && metapath_pick(0, 70001, 0.5) == 35000, "pick in a hub", 0, 0);
    printf("%d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
