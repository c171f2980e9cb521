// Pins the rule of layer-neighbour sampling (legion_amd/csrc/labor_rule.h: the hash, the integer predicate, which calls
// legion_labor_count and legion_labor_edges refuse, and the scratch size, whose formula is kept_rule.h's) over a literal table.  The
// hash values were computed with legion_amd/synth.py::splitmix64_np, the predicate's with Python integers, the codes written down from the rules as
// include/legion_hip.h documents them; none comes from the header.
//   g++ -O1 -std=c++17 labor_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/kept_rule.h"      // first: a changed copy of it shadows the one labor_rule.h includes
#include "../../legion_amd/csrc/labor_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576 && LEGION_LABOR_MAX_SLOTS == 1073741824, "the tables below spell the limits out");
static_assert(labor_hash(0, 0) <= 0xffffffffu && labor_keep(0u, (int64_t)1 << 62, 1), "the rule is constexpr: the device runs this text");
enum { OK, CNT, MANY, SLOTS, FAN, CAP, SCR };
static const int64_t BIG = (int64_t)1 << 40;
static const int64_t P32 = (int64_t)1 << 32;

struct HashCase { int32_t v; int64_t salt; uint32_t want; };
static const HashCase hashes[] = {
    {0, 0, 0xa706dd2fu}, {7, 3, 0xe880a903u}, {5, -1, 0x3562133au}, {2147483647, 0, 0x78bae605u},
    {2147483647, -9223372036854775807LL - 1, 0xff259974u}, {1, 9223372036854775807LL, 0xd1448f4du}, {123456, 12345, 0xc36e88f4u},
};

struct KeepCase { uint32_t h; int64_t d; int32_t fanout; bool want; };
static const KeepCase keeps[] = {
    // h * d < fanout * 2^32
    {0xffffffffu, 5, 5, true},                                     // d == fanout keeps whatever the number
    {0xffffffffu, 1, 1, true},
    {0xffffffffu, 6, 5, false},                                    // d == fanout + 1 with the largest number
    {0xffffffffu, 2, 1, false},
    {0u, 6, 5, true}, {0u, 9223372036854775807LL, 1, true},        // h == 0 always keeps
    {0x80000000u, 2, 1, false}, {0x7fffffffu, 2, 1, true},         // probability one half: the threshold is 2^31
    {0xd5555555u, 6, 5, true}, {0xd5555556u, 6, 5, false},         // 5 / 6: floor(5 * 2^32 / 6) = 0xd5555555 keeps (0xd5555555 * 6 = 5 * 2^32 - 2)
    // d = 2^32: h * 2^32 < fanout * 2^32 iff h < fanout
    {4u, P32, 5, true}, {5u, P32, 5, false}, {0u, P32, 1, true}, {1u, P32, 1, false},
    // d = 2^32 + 1: h (2^32 + 1) < fanout 2^32 iff h < fanout (h >= 1 adds h to the low word)
    {4u, P32 + 1, 5, true}, {5u, P32 + 1, 5, false}, {1u, P32 + 1, 1, false},
    // where 64 bits wrap: 2^32 * 2^32 = 2^64 truncates to 0 < anything
    {0x80000000u, (int64_t)1 << 33, 1, false}, {0xffffffffu, P32, 2147483647, false}, {0xffffffffu, P32 + 1, 1, false},
    {3u, ((int64_t)1 << 62) + 1, 1, false}, {1u, (int64_t)1 << 62, 2147483647, true}, {2u, (int64_t)1 << 62, 2147483647, false},
    // fanout = 2^31 - 1
    {0xffffffffu, 2147483647, 2147483647, true}, {0xffffffffu, 2147483648LL, 2147483647, false},
    {0xfffffffdu, 2147483648LL, 2147483647, true}, {0xfffffffeu, 2147483648LL, 2147483647, false},
};

struct CountCase { int32_t n; int64_t m; int32_t fanout; int64_t scratch; int want; };
static const CountCase counts[] = {
    // n, m, fanout, scratch_bytes -> code
    {100, 1000, 10, 24, OK}, {100, 1000, 10, 23, SCR}, {100, 1000, 10, 0, SCR}, {100, 1000, 10, -1, SCR}, {100, 1000, 10, BIG, OK},
    {0, 0, 1, 8, OK}, {0, 0, 1, 7, SCR}, {100, 0, 1, 8, OK}, {100, 1024, 1, 24, OK}, {100, 1025, 1, 24, SCR}, {100, 1025, 1, 32, OK},
    {1048576, 1073741824LL, 2147483647, 8421384, OK}, {1048576, 1073741824LL, 1, 8421383, SCR},
    {-1, 1000, 10, BIG, CNT}, {1048577, 1000, 10, BIG, MANY}, {2147483647, 1000, 10, BIG, MANY},
    {100, -1, 10, BIG, SLOTS}, {100, 1073741825LL, 10, BIG, SLOTS}, {100, BIG, 10, BIG, SLOTS}, {100, -9223372036854775807LL, 10, BIG, SLOTS},
    {100, 1000, 0, BIG, FAN}, {100, 1000, -1, BIG, FAN}, {100, 1000, -2147483647 - 1, BIG, FAN}, {100, 1000, 1, BIG, OK},
    // the order of the checks: n, m, fanout, scratch
    {-1, -1, 0, -1, CNT}, {1048577, -1, 0, -1, MANY}, {100, -1, 0, -1, SLOTS}, {100, 1073741825LL, 0, -1, SLOTS}, {100, 1000, 0, -1, FAN},
};

struct EdgesCase { int32_t n; int64_t m; int32_t fanout; int64_t scratch; int64_t cap; int want; };
static const EdgesCase edges[] = {
    // n, m, fanout, scratch_bytes, cap -> code
    {100, 1000, 10, 24, 500, OK}, {100, 1000, 10, 24, 0, OK}, {100, 1000, 10, 24, 2147483647LL, OK}, {100, 1000, 10, 24, 2147483648LL, CAP},
    {100, 1000, 10, 24, -1, CAP}, {100, 1000, 10, 24, BIG, CAP}, {100, 1000, 10, 23, 500, SCR}, {0, 0, 1, 8, 5, OK}, {0, 0, 1, 0, 5, SCR},
    {-1, 1000, 10, BIG, 500, CNT}, {1048577, 1000, 10, BIG, 500, MANY}, {100, -1, 10, BIG, 500, SLOTS}, {100, 1073741825LL, 10, BIG, 500, SLOTS},
    {100, 1073741824LL, 10, BIG, 500, OK}, {100, 1000, 0, BIG, 500, FAN},
    // the order of the checks: n, m, fanout, cap, scratch
    {-1, -1, 0, -1, -1, CNT}, {1048577, -1, 0, -1, -1, MANY}, {100, -1, 0, -1, -1, SLOTS}, {100, 1000, 0, -1, -1, FAN},
    {100, 1000, 1, -1, -1, CAP}, {100, 1000, 1, -1, 2147483648LL, CAP}, {100, 1000, 1, -1, 5, SCR},
};

struct BytesCase { int64_t m; int64_t want; };
static const BytesCase sizes[] = {
    // 8 x (tiles of 1 024 slots + 1 + groups of 256 tiles)
    {0, 8}, {1, 24}, {1024, 24}, {1025, 32}, {262144, 2064}, {262145, 2080}, {1073741824LL, 8421384}, {1073741825LL, -1}, {-1, -1},
};

static int code(LaborRefusal r)
{
    switch (r) {
    case LaborRefusal::Ok: return OK;
    case LaborRefusal::Count: return CNT;
    case LaborRefusal::TooMany: return MANY;
    case LaborRefusal::Slots: return SLOTS;
    case LaborRefusal::Fanout: return FAN;
    case LaborRefusal::Capacity: return CAP;
    case LaborRefusal::Scratch: return SCR;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const HashCase& c : hashes) {
        n++;
        if (labor_hash(c.v, c.salt) != c.want || labor_hash_keyed(labor_key(c.salt), c.v) != c.want) {
            printf("MISMATCH labor_hash(%d, %lld): got %08x, want %08x\n", c.v, (long long)c.salt, labor_hash(c.v, c.salt), c.want);
            bad++;
        }
    }
    if (splitmix64(0) != 0xe220a8397b1dcdafull || labor_key(-1) != 0xe4d971771b652c20ull) { printf("MISMATCH splitmix64 / labor_key\n"); bad++; }
    for (const KeepCase& c : keeps) {
        n++;
        if (labor_keep(c.h, c.d, c.fanout) != c.want) {
            printf("MISMATCH labor_keep(%08x, %lld, %d): got %d, want %d\n", c.h, (long long)c.d, c.fanout, !c.want, c.want);
            bad++;
        }
#ifdef __SIZEOF_INT128__
        if (((unsigned __int128)c.h * (unsigned __int128)c.d < ((unsigned __int128)c.fanout << 32)) != c.want) {
            printf("MISMATCH: the table itself at (%08x, %lld, %d)\n", c.h, (long long)c.d, c.fanout);
            bad++;
        }
#endif
    }
    for (const CountCase& c : counts) {
        n++;
        const LaborRefusal r = labor_count_refusal(c.n, c.m, c.fanout, c.scratch);
        if (code(r) != c.want) {
            printf("MISMATCH count n %d m %lld fanout %d scratch %lld: got %d, want %d\n", c.n, (long long)c.m, c.fanout, (long long)c.scratch,
                   code(r), c.want);
            bad++;
        }
        if (labor_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const EdgesCase& c : edges) {
        n++;
        const LaborRefusal r = labor_edges_refusal(c.n, c.m, c.fanout, c.scratch, c.cap);
        if (code(r) != c.want) {
            printf("MISMATCH edges n %d m %lld fanout %d scratch %lld cap %lld: got %d, want %d\n", c.n, (long long)c.m, c.fanout,
                   (long long)c.scratch, (long long)c.cap, code(r), c.want);
            bad++;
        }
        if (labor_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (labor_scratch_bytes(c.m) != c.want) {
            printf("MISMATCH scratch bytes of %lld: got %lld, want %lld\n", (long long)c.m, (long long)labor_scratch_bytes(c.m), (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
