// Pins the rule of the vertex set and of induced subgraphs (legion_amd/csrc/induced_rule.h and, under it, id_table_rule.h and
// kept_rule.h: the table's slots, shift, home slot and size,
// which calls legion_node_set_build, legion_node_set_lookup, legion_induced_count, legion_induced_edges and legion_dst_offsets refuse, and
// the scratch size) over a literal table.  The home slots were computed with Python integers ((v * 2654435769 mod 2^32) >> shift), the
// codes written down from the rules as include/legion_hip.h documents them; none comes from the header.
//   g++ -O1 -std=c++17 induced_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/id_table_rule.h"      // these two first: a changed copy of one shadows the one induced_rule.h includes
#include "../../legion_amd/csrc/kept_rule.h"
#include "../../legion_amd/csrc/induced_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576 && LEGION_INDUCED_MAX_SLOTS == 1073741824 && LEGION_NODE_SET_MAX_IDS == 1048576,
              "the tables below spell the limits out");
static_assert(node_set_home(1, 24) <= 255u && node_set_bytes(-1) == -1, "the rule is constexpr: the device runs this text");
static_assert(NODE_SET_EMPTY_KEY == -1 && (uint32_t)NODE_SET_EMPTY_KEY == 0xFFFFFFFFu, "an empty key is all-ones");
enum { OK, CNT, SLOTS, SIZE, BYTES, CAP, SCR };
static const int64_t BIG = (int64_t)1 << 40;

struct SlotsCase { int32_t k; int64_t slots; int32_t shift; int64_t bytes; };
static const SlotsCase tables[] = {
    // k -> S (the power of two >= max(256, 2 k)), 32 - log2 S, 8 S
    {0, 256, 24, 2048}, {1, 256, 24, 2048}, {100, 256, 24, 2048}, {127, 256, 24, 2048}, {128, 256, 24, 2048}, {129, 512, 23, 4096},
    {256, 512, 23, 4096}, {257, 1024, 22, 8192}, {3000, 8192, 19, 65536}, {4096, 8192, 19, 65536}, {4097, 16384, 18, 131072},
    {524288, 1048576, 12, 8388608}, {524289, 2097152, 11, 16777216}, {1048576, 2097152, 11, 16777216},
};

struct HomeCase { int32_t v; int32_t shift; uint32_t want; };
static const HomeCase homes[] = {
    // ((uint32)v * 2654435769) >> shift
    {0, 24, 0}, {1, 24, 158}, {2, 24, 60}, {144, 24, 255}, {288, 24, 254}, {377, 24, 255}, {521, 24, 254}, {5999, 24, 149},
    {2147483647, 24, 225}, {1, 11, 1296111}, {2147483647, 11, 1849616}, {6, 23, 362}, {123456, 19, 33},
};

struct BytesCase { int32_t k; int64_t want; };
static const BytesCase set_sizes[] = {{-1, -1}, {1048577, -1}, {2147483647, -1}, {-2147483647 - 1, -1}};

struct BuildCase { int32_t k; int64_t set_bytes; int want; };
static const BuildCase builds[] = {
    {0, 2048, OK}, {0, 2047, BYTES}, {128, 2048, OK}, {129, 2048, BYTES}, {129, 4096, OK}, {1048576, 16777216, OK}, {1048576, 16777215, BYTES},
    {1048577, BIG, SIZE}, {-1, BIG, SIZE}, {5, 0, BYTES}, {5, -1, BYTES}, {5, BIG, OK},
    // the order of the checks: k, set_bytes
    {-1, -1, SIZE},
};

struct LookupCase { int32_t k; int64_t set_bytes; int64_t m; int want; };
static const LookupCase lookups[] = {
    {5, 2048, 0, OK}, {5, 2048, 2147483647LL, OK}, {5, 2048, 2147483648LL, SLOTS}, {5, 2048, -1, SLOTS}, {5, 2047, 10, BYTES},
    {1048577, BIG, 10, SIZE}, {-1, BIG, 10, SIZE}, {0, 2048, 10, OK},
    // the order of the checks: k, set_bytes, m
    {-1, -1, -1, SIZE}, {5, -1, -1, BYTES},
};

struct CountCase { int32_t n; int64_t m; int32_t k; int64_t set_bytes; int64_t scratch; int want; };
static const CountCase counts[] = {
    // n, m, k, set_bytes, scratch_bytes -> code
    {100, 1000, 8, 2048, 24, OK}, {100, 1000, 8, 2048, 23, SCR}, {100, 1000, 8, 2048, 0, SCR}, {100, 1000, 8, 2048, -1, SCR},
    {100, 1000, 8, BIG, BIG, OK}, {0, 0, 0, 2048, 8, OK}, {0, 0, 0, 2048, 7, SCR}, {100, 1024, 8, 2048, 24, OK}, {100, 1025, 8, 2048, 24, SCR},
    {100, 1025, 8, 2048, 32, OK}, {1048576, 1073741824LL, 1048576, 16777216, 8421384, OK}, {1048576, 1073741824LL, 1048576, 16777216, 8421383, SCR},
    {-1, 1000, 8, BIG, BIG, CNT}, {1048577, 1000, 8, BIG, BIG, CNT}, {2147483647, 1000, 8, BIG, BIG, CNT},
    {100, -1, 8, BIG, BIG, SLOTS}, {100, 1073741825LL, 8, BIG, BIG, SLOTS}, {100, BIG, 8, BIG, BIG, SLOTS},
    {100, 1000, -1, BIG, BIG, SIZE}, {100, 1000, 1048577, BIG, BIG, SIZE}, {100, 1000, 129, 2048, BIG, BYTES}, {100, 1000, 8, 2047, BIG, BYTES},
    {100, 1000, 8, -1, BIG, BYTES},
    // the order of the checks: n, m, k, set_bytes, scratch
    {-1, -1, -1, -1, -1, CNT}, {100, -1, -1, -1, -1, SLOTS}, {100, 1000, -1, -1, -1, SIZE}, {100, 1000, 8, -1, -1, BYTES},
    {100, 1000, 8, 2048, -1, SCR},
};

struct EdgesCase { int32_t n; int64_t m; int32_t k; int64_t set_bytes; int64_t scratch; int64_t cap; int want; };
static const EdgesCase edges[] = {
    // n, m, k, set_bytes, scratch_bytes, cap -> code
    {100, 1000, 8, 2048, 24, 500, OK}, {100, 1000, 8, 2048, 24, 0, OK}, {100, 1000, 8, 2048, 24, 2147483647LL, OK},
    {100, 1000, 8, 2048, 24, 2147483648LL, CAP}, {100, 1000, 8, 2048, 24, -1, CAP}, {100, 1000, 8, 2048, 24, BIG, CAP},
    {100, 1000, 8, 2048, 23, 500, SCR}, {0, 0, 0, 2048, 8, 5, OK}, {0, 0, 0, 2048, 0, 5, SCR}, {-1, 1000, 8, BIG, BIG, 500, CNT},
    {1048577, 1000, 8, BIG, BIG, 500, CNT}, {100, -1, 8, BIG, BIG, 500, SLOTS}, {100, 1073741825LL, 8, BIG, BIG, 500, SLOTS},
    {100, 1073741824LL, 8, BIG, BIG, 500, OK}, {100, 1000, 1048577, BIG, BIG, 500, SIZE}, {100, 1000, 8, 2047, BIG, 500, BYTES},
    // the order of the checks: n, m, k, set_bytes, cap, scratch
    {-1, -1, -1, -1, -1, -1, CNT}, {100, -1, -1, -1, -1, -1, SLOTS}, {100, 1000, -1, -1, -1, -1, SIZE}, {100, 1000, 8, -1, -1, -1, BYTES},
    {100, 1000, 8, 2048, -1, -1, CAP}, {100, 1000, 8, 2048, -1, 2147483648LL, CAP}, {100, 1000, 8, 2048, -1, 5, SCR},
};

struct OffsetsCase { int64_t cap; int32_t n; int want; };
static const OffsetsCase offsets[] = {
    {0, 0, OK}, {2147483647LL, 1048576, OK}, {2147483648LL, 5, CAP}, {-1, 5, CAP}, {BIG, 5, CAP}, {5, -1, CNT}, {5, 1048577, CNT},
    // the order of the checks: cap, n
    {-1, -1, CAP},
};

struct ScratchCase { int64_t m; int64_t want; };
static const ScratchCase sizes[] = {
    // 8 x (tiles of 1 024 slots + 1 + groups of 256 tiles)
    {0, 8}, {1, 24}, {1024, 24}, {1025, 32}, {262144, 2064}, {262145, 2080}, {1073741824LL, 8421384}, {1073741825LL, -1}, {-1, -1},
};

static int code(InducedRefusal r)
{
    switch (r) {
    case InducedRefusal::Ok: return OK;
    case InducedRefusal::Count: return CNT;
    case InducedRefusal::Slots: return SLOTS;
    case InducedRefusal::SetSize: return SIZE;
    case InducedRefusal::SetBytes: return BYTES;
    case InducedRefusal::Capacity: return CAP;
    case InducedRefusal::Scratch: return SCR;
    }
    return -1;
}

static int bad = 0, n = 0;

static void check(const char* what, long long a, long long b, long long c, InducedRefusal r, int want)
{
    n++;
    if (code(r) != want) {
        printf("MISMATCH %s (%lld, %lld, %lld, ..): got %d, want %d\n", what, a, b, c, code(r), want);
        bad++;
    }
    if (induced_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
}

int main()
{
    for (const SlotsCase& c : tables) {
        n++;
        if (node_set_slots(c.k) != c.slots || node_set_shift(c.slots) != c.shift || node_set_bytes(c.k) != c.bytes) {
            printf("MISMATCH table of %d: got %lld slots, shift %d, %lld bytes\n", c.k, (long long)node_set_slots(c.k), node_set_shift(node_set_slots(c.k)),
                   (long long)node_set_bytes(c.k));
            bad++;
        }
    }
    for (const HomeCase& c : homes) {
        n++;
        if (node_set_home(c.v, c.shift) != c.want) {
            printf("MISMATCH home of %d at shift %d: got %u, want %u\n", c.v, c.shift, node_set_home(c.v, c.shift), c.want);
            bad++;
        }
    }
    for (const BytesCase& c : set_sizes) {
        n++;
        if (node_set_bytes(c.k) != c.want) { printf("MISMATCH set bytes of %d\n", c.k); bad++; }
    }
    for (const BuildCase& c : builds) check("build", c.k, c.set_bytes, 0, node_set_build_refusal(c.k, c.set_bytes), c.want);
    for (const LookupCase& c : lookups) check("lookup", c.k, c.set_bytes, c.m, node_set_lookup_refusal(c.k, c.set_bytes, c.m), c.want);
    for (const CountCase& c : counts) check("count", c.n, c.m, c.k, induced_count_refusal(c.n, c.m, c.k, c.set_bytes, c.scratch), c.want);
    for (const EdgesCase& c : edges) check("edges", c.n, c.m, c.k, induced_edges_refusal(c.n, c.m, c.k, c.set_bytes, c.scratch, c.cap), c.want);
    for (const OffsetsCase& c : offsets) check("dst_offsets", c.cap, c.n, 0, dst_offsets_refusal(c.cap, c.n), c.want);
    for (const ScratchCase& c : sizes) {
        n++;
        if (induced_scratch_bytes(c.m) != c.want) {
            printf("MISMATCH scratch bytes of %lld: got %lld, want %lld\n", (long long)c.m, (long long)induced_scratch_bytes(c.m), (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
