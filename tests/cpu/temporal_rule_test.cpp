// Pins the rule of temporal neighbour sampling (legion_amd/csrc/temporal_rule.h: the candidate test, the slot count of a row, the ranks
// of LAST, the draw of UNIFORM, which calls are refused and in which order, and the scratch size) over a literal table.  The draws were
// computed with tests/etype_ref.py at t = 0, the codes written down from the rules as include/legion_hip.h documents them; none comes
// from the header.
//   g++ -O1 -std=c++17 temporal_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/temporal_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576 && LEGION_TEMPORAL_MAX_FANOUT == 64 && LEGION_TEMPORAL_UNIFORM == 0 && LEGION_TEMPORAL_LAST == 1,
              "the tables spell the limits out");
static_assert(temporal_slots(7, 3, 0) == 3 && temporal_last_rank(7, 3, 0) == 4 && temporal_uniform_draw(labor_key(0), 0, 7, 3, 0, 0) == 3,
              "the rule is constexpr: the device runs this text");
enum { OK, CNT, MANY, UNTIMED, FAN, STRAT, REP, LASTREP, LASTUNS, CAP, PTR, SCR };
enum { U = 0, L = 1 };
static const int64_t BIG = (int64_t)1 << 40, MIN64 = -9223372036854775807LL - 1, MAX64 = 9223372036854775807LL;

// strict and signed: the low words alone order the third and fourth pair the other way
struct CandCase { int64_t time, bound; bool want; };
static const CandCase cands[] = {
    {5, 5, false}, {4, 5, true}, {(int64_t)1 << 32, 5, false}, {-1, 0, true}, {MIN64, MIN64, false}, {MIN64, MIN64 + 1, true},
    {MAX64 - 1, MAX64, true}, {MAX64, MAX64, false}, {-5, -5, false}, {-6, -5, true},
};

struct SlotCase { int64_t C; int32_t f, replace; int64_t want; };
static const SlotCase slotcases[] = {
    // C in {0, f - 1, f, f + 1} for both replace values, then f = -1
    {0, 5, 0, 0}, {4, 5, 0, 4}, {5, 5, 0, 5}, {6, 5, 0, 5}, {0, 5, 1, 0}, {4, 5, 1, 5}, {5, 5, 1, 5}, {6, 5, 1, 5}, {0, 1, 0, 0}, {1, 1, 0, 1},
    {2, 1, 0, 1}, {63, 64, 0, 63}, {64, 64, 0, 64}, {65, 64, 0, 64}, {63, 64, 1, 64}, {65, 64, 1, 64}, {BIG, 5, 0, 5}, {0, -1, 0, 0},
    {1, -1, 0, 1}, {70001, -1, 1, 70001}, {BIG, -1, 0, BIG},
};

// LAST: slot k of `slots` picks rank C - slots + k
struct LastCase { int64_t C, slots, k, want; };
static const LastCase lasts[] = {{7, 3, 0, 4}, {7, 3, 2, 6}, {5, 5, 0, 0}, {5, 5, 4, 4}, {70001, 64, 0, 69937}, {70001, 64, 63, 70000}, {1, 1, 0, 0}, {BIG, 1, 0, BIG - 1}};

struct DrawCase { int64_t salt; int32_t row; int64_t C; int32_t f, replace, k; int64_t want; };
static const DrawCase draws[] = {
    {0, 0, 7, 3, 0, 0, 3}, {0, 0, 7, 3, 0, 2, 5}, {5, 9, 100, 64, 1, 63, 95}, {-1, 70000, 70001, 5, 0, 4, 19318},
    {3, 2147483647, 4294967301LL, 1, 1, 0, 1304519152LL}, {7, 12, BIG, 64, 0, 63, 3629718016LL},
};

// scratch < 0: the write pass with cap; otherwise the count pass with that many scratch bytes.  sorted: -1 no times, 0, 1
struct CallCase { int32_t n, sorted, f, strategy, replace; int64_t cap; bool ptrs; int64_t scratch; int want; };
static const CallCase calls[] = {
    {100, 1, 5, U, 0, 10, true, -1, OK}, {100, 0, 5, U, 1, 10, true, -1, OK}, {100, 1, 64, L, 0, 10, true, -1, OK}, {0, 1, -1, L, 0, 0, true, -1, OK},
    {1048576, 0, 1, U, 0, 2147483647LL, true, -1, OK}, {-1, 1, 5, U, 0, 10, true, -1, CNT}, {1048577, 1, 5, U, 0, 10, true, -1, MANY},
    {100, -1, 5, U, 0, 10, true, -1, UNTIMED}, {100, 1, 0, U, 0, 10, true, -1, FAN}, {100, 1, 65, U, 0, 10, true, -1, FAN},
    {100, 1, -2, U, 0, 10, true, -1, FAN}, {100, 1, 5, 2, 0, 10, true, -1, STRAT}, {100, 1, 5, -1, 0, 10, true, -1, STRAT},
    {100, 1, 5, U, 2, 10, true, -1, REP}, {100, 1, 5, U, -1, 10, true, -1, REP}, {100, 1, 5, L, 1, 10, true, -1, LASTREP},
    {100, 0, 5, L, 0, 10, true, -1, LASTUNS}, {100, 1, 5, U, 0, -1, true, -1, CAP}, {100, 1, 5, U, 0, 2147483648LL, true, -1, CAP},
    {100, 1, 5, U, 0, 10, false, -1, PTR},
    // the order of the checks: n, n, untimed, fan-out, strategy, replace, LAST with replace, LAST unsorted, cap, pointers, scratch
    {-1, -1, 0, 2, 2, -1, false, -1, CNT}, {1048577, -1, 0, 2, 2, -1, false, -1, MANY}, {100, -1, 0, 2, 2, -1, false, -1, UNTIMED},
    {100, 0, 0, 2, 2, -1, false, -1, FAN}, {100, 0, 5, 2, 2, -1, false, -1, STRAT}, {100, 0, 5, L, 2, -1, false, -1, REP},
    {100, 0, 5, L, 1, -1, false, -1, LASTREP}, {100, 0, 5, L, 0, -1, false, -1, LASTUNS}, {100, 1, 5, L, 0, -1, false, -1, CAP},
    {100, 1, 5, L, 0, 5, false, -1, PTR}, {100, 1, 5, L, 0, 0, false, 0, PTR}, {100, 1, 5, L, 0, 0, true, 7, SCR},
    {100, 1, 5, U, 0, 0, true, 8, OK}, {257, 0, 5, U, 0, 0, true, 15, SCR}, {257, 0, 5, U, 0, 0, true, 16, OK}, {0, 1, 5, U, 0, 0, true, 0, OK},
};

struct BytesCase { int32_t n; int64_t want; };
static const BytesCase sizes[] = {{0, 0}, {1, 8}, {256, 8}, {257, 16}, {1048576, 32768}, {1048577, -1}, {-1, -1}};

int main()
{
    int bad = 0, n = 0;
    for (const CandCase& c : cands) {
        n++;
        if (temporal_candidate(c.time, c.bound) != c.want) {
            printf("MISMATCH temporal_candidate(time %lld, bound %lld): want %d\n", (long long)c.time, (long long)c.bound, (int)c.want);
            bad++;
        }
    }
    for (const SlotCase& c : slotcases) {
        n++;
        if (temporal_slots(c.C, c.f, c.replace) != c.want || temporal_takes_all(c.C, c.f, c.replace) != (c.want == c.C)) {
            printf("MISMATCH temporal_slots(C %lld, f %d, replace %d): got %lld, want %lld\n", (long long)c.C, c.f, c.replace,
                   (long long)temporal_slots(c.C, c.f, c.replace), (long long)c.want);
            bad++;
        }
    }
    for (const LastCase& c : lasts) {
        n++;
        if (temporal_last_rank(c.C, c.slots, c.k) != c.want) {
            printf("MISMATCH temporal_last_rank(C %lld, slots %lld, k %lld): got %lld, want %lld\n", (long long)c.C, (long long)c.slots, (long long)c.k,
                   (long long)temporal_last_rank(c.C, c.slots, c.k), (long long)c.want);
            bad++;
        }
    }
    for (const DrawCase& c : draws) {
        n++;
        const int64_t got = temporal_uniform_draw(labor_key(c.salt), c.row, c.C, c.f, c.replace, c.k);
        if (got != c.want) {
            printf("MISMATCH temporal_uniform_draw(salt %lld, row %d, C %lld, f %d, replace %d, k %d): got %lld, want %lld\n", (long long)c.salt, c.row,
                   (long long)c.C, c.f, c.replace, c.k, (long long)got, (long long)c.want);
            bad++;
        }
    }
    for (const CallCase& c : calls) {
        n++;
        const TemporalRefusal r = c.scratch < 0 ? temporal_edges_refusal(c.n, c.sorted, c.f, c.strategy, c.replace, c.cap, c.ptrs)
                                                : temporal_count_refusal(c.n, c.sorted, c.f, c.strategy, c.replace, c.ptrs, c.scratch);
        if ((int)r != c.want || temporal_refusal_text(r)[0] == 0) {
            printf("MISMATCH call n %d sorted %d f %d strategy %d replace %d cap %lld pointers %d scratch %lld: got %d, want %d\n", c.n, c.sorted, c.f,
                   c.strategy, c.replace, (long long)c.cap, c.ptrs, (long long)c.scratch, (int)r, c.want);
            bad++;
        }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (temporal_scratch_bytes(c.n) != c.want) {
            printf("MISMATCH scratch bytes of %d: got %lld, want %lld\n", c.n, (long long)temporal_scratch_bytes(c.n), (long long)c.want);
            bad++;
        }
    }
    n += 2;
    if (temporal_sorted_verdict(3, 3) != 1 || temporal_sorted_verdict(0, 0) != 1) { printf("MISMATCH sorted verdict of equal counts\n"); bad++; }
    if (temporal_sorted_verdict(4, 3) != 0) { printf("MISMATCH sorted verdict of a descent inside a row\n"); bad++; }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
