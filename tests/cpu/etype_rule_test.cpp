// Pins the rule of per-edge-type sampling (legion_amd/csrc/etype_rule.h: the draw, the slot count of a pair, which calls are refused and
// in which order, and the scratch size) over a literal table.  The draws were computed with tests/etype_ref.py, the codes written down
// from the rules as include/legion_hip.h documents them; none comes from the header.
//   g++ -O1 -std=c++17 etype_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/etype_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576 && LEGION_ETYPE_MAX_TYPES == 64 && LEGION_ETYPE_MAX_FANOUT == 64, "the tables spell the limits out");
static_assert(etype_draw(labor_key(0), 0, 0, 0, 5) == 3 && etype_slots(7, 3, 0) == 3, "the rule is constexpr: the device runs this text");
enum { OK, CNT, MANY, UNTYPED, FAN, REP, CAP, PTR, SCR };
static const int64_t BIG = (int64_t)1 << 40;

struct DrawCase { int64_t salt; int32_t row, t, k; uint64_t R, want; };
static const DrawCase draws[] = {
    {0LL, 0, 0, 0, 5ull, 3ull}, {1LL, 7, 3, 2, 100ull, 58ull}, {-1LL, 12345, 63, 63, 4097ull, 2252ull},
    {-9223372036854775807LL - 1, 5, 1, 0, 2ull, 1ull}, {99LL, 2147483647, 0, 1, 1000ull, 709ull}, {3LL, 9, 2, 4, 1ull, 0ull},
    {3LL, 9, 2, 4, 2147483647ull, 1331445703ull}, {12345LL, 70000, 17, 33, 70001ull, 18729ull},
    {9223372036854775807LL, 1, 63, 0, 4294967295ull, 665727107ull},
};

struct SlotCase { int64_t D; int32_t f, replace; int64_t want; };
static const SlotCase slotcases[] = {
    // D in {0, f - 1, f, f + 1} for both replace values, then f in {-1, 0}
    {0, 5, 0, 0}, {4, 5, 0, 4}, {5, 5, 0, 5}, {6, 5, 0, 5}, {0, 5, 1, 0}, {4, 5, 1, 5}, {5, 5, 1, 5}, {6, 5, 1, 5},
    {63, 64, 0, 63}, {64, 64, 0, 64}, {65, 64, 0, 64}, {63, 64, 1, 64}, {65, 64, 1, 64}, {BIG, 5, 0, 5},
    {0, -1, 0, 0}, {1, -1, 0, 1}, {70001, -1, 1, 70001}, {BIG, -1, 0, BIG}, {0, 0, 0, 0}, {9, 0, 0, 0}, {9, 0, 1, 0},
};

// scratch < 0: the write pass with cap; otherwise the count pass with that many scratch bytes
static const int32_t F_OK[4] = {-1, 0, 5, 64}, F_LOW[4] = {-1, 0, -2, 64}, F_HIGH[4] = {-1, 0, 5, 65};
struct CallCase { int32_t n, T; const int32_t* f; int32_t replace; int64_t cap; bool ptrs; int64_t scratch; int want; };
static const CallCase calls[] = {
    {100, 4, F_OK, 0, 10, true, -1, OK}, {0, 4, F_OK, 1, 0, true, -1, OK}, {1048576, 4, F_OK, 0, 2147483647LL, true, -1, OK},
    {-1, 4, F_OK, 0, 10, true, -1, CNT}, {1048577, 4, F_OK, 0, 10, true, -1, MANY}, {100, 0, F_OK, 0, 10, true, -1, UNTYPED},
    {100, 4, F_LOW, 0, 10, true, -1, FAN}, {100, 4, F_HIGH, 0, 10, true, -1, FAN}, {100, 3, F_HIGH, 0, 10, true, -1, OK},
    {100, 4, F_OK, 2, 10, true, -1, REP}, {100, 4, F_OK, -1, 10, true, -1, REP}, {100, 4, F_OK, 0, -1, true, -1, CAP},
    {100, 4, F_OK, 0, 2147483648LL, true, -1, CAP}, {100, 4, F_OK, 0, 10, false, -1, PTR}, {100, 4, nullptr, 0, 10, false, -1, PTR},
    // the order of the checks: n, n, untyped, fan-out, replace, cap, pointers, scratch
    {-1, 0, F_HIGH, 2, -1, false, -1, CNT}, {1048577, 0, F_HIGH, 2, -1, false, -1, MANY}, {100, 0, F_HIGH, 2, -1, false, -1, UNTYPED},
    {100, 4, F_HIGH, 2, -1, false, -1, FAN}, {100, 3, F_HIGH, 2, -1, false, -1, REP}, {100, 3, F_HIGH, 1, -1, false, -1, CAP},
    {100, 3, F_HIGH, 1, 5, false, -1, PTR}, {100, 3, F_HIGH, 1, 0, false, 0, PTR}, {100, 3, F_HIGH, 1, 0, true, 7, SCR},
    {100, 4, F_OK, 0, 0, true, 8, OK}, {257, 4, F_OK, 0, 0, true, 15, SCR}, {257, 4, F_OK, 0, 0, true, 16, OK}, {0, 4, F_OK, 0, 0, true, 0, OK},
};

struct BytesCase { int32_t n; int64_t want; };
static const BytesCase sizes[] = {{0, 0}, {1, 8}, {256, 8}, {257, 16}, {1048576, 32768}, {1048577, -1}, {-1, -1}};

int main()
{
    int bad = 0, n = 0;
    for (const DrawCase& c : draws) {
        n++;
        const uint64_t got = etype_draw(labor_key(c.salt), c.row, c.t, c.k, c.R);
        if (got != c.want) {
            printf("MISMATCH etype_draw(salt %lld, row %d, t %d, k %d, R %llu): got %llu, want %llu\n", (long long)c.salt, c.row, c.t, c.k,
                   (unsigned long long)c.R, (unsigned long long)got, (unsigned long long)c.want);
            bad++;
        }
    }
    for (const SlotCase& c : slotcases) {
        n++;
        if (etype_slots(c.D, c.f, c.replace) != c.want) {
            printf("MISMATCH etype_slots(D %lld, f %d, replace %d): got %lld, want %lld\n", (long long)c.D, c.f, c.replace,
                   (long long)etype_slots(c.D, c.f, c.replace), (long long)c.want);
            bad++;
        }
    }
    for (const CallCase& c : calls) {
        n++;
        const EtypeRefusal r = c.scratch < 0 ? etype_edges_refusal(c.n, c.T, c.f, c.replace, c.cap, c.ptrs)
                                             : etype_count_refusal(c.n, c.T, c.f, c.replace, c.ptrs, c.scratch);
        if ((int)r != c.want || etype_refusal_text(r)[0] == 0) {
            printf("MISMATCH call n %d T %d replace %d cap %lld pointers %d scratch %lld: got %d, want %d\n", c.n, c.T, c.replace, (long long)c.cap,
                   c.ptrs, (long long)c.scratch, (int)r, c.want);
            bad++;
        }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (etype_scratch_bytes(c.n) != c.want) {
            printf("MISMATCH scratch bytes of %d: got %lld, want %lld\n", c.n, (long long)etype_scratch_bytes(c.n), (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
