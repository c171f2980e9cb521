// Pins the rules of seed-edge exclusion (legion_amd/csrc/exclude_rule.h: the slots, the shift, the home slot and the bytes of the set of
// edge ids, the limits, which calls legion_reverse_edge_ids, legion_edge_set_build, legion_edge_set_contains, legion_edge_filter_count and
// legion_edge_filter_edges refuse and in which order, the filter's scratch) over a literal table.  The expected values were written down
// from the rules as include/legion_hip.h states them -- the home slots with Python's integers, ((e * 0x9E3779B97F4A7C15) mod 2^64) >>
// (64 - log2 S) -- not from the header.
//   g++ -O1 -std=c++17 exclude_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/exclude_rule.h"

static_assert(LEGION_EDGE_SET_MAX_IDS == 2097152 && LEGION_EDGE_FILTER_MAX_EDGES == 1073741824, "the tables below spell the limits out");
enum { OK, COUNT, VIA, UNSORTED, NOREV, SETSIZE, SETBYTES, SLOTS, CAP, SCRATCH, ALIAS };

struct SizeCase { int32_t k; int64_t slots; int32_t shift; int64_t bytes; };
static const SizeCase sizes[] = {
    // k -> slots (a power of two, at least 256 and at least 2 k), 64 - log2 slots, 8 bytes a slot; -1 bytes for an illegal k
    {0, 256, 56, 2048}, {1, 256, 56, 2048}, {127, 256, 56, 2048}, {128, 256, 56, 2048}, {129, 512, 55, 4096}, {256, 512, 55, 4096},
    {257, 1024, 54, 8192}, {1000, 2048, 53, 16384}, {1048576, 2097152, 43, 16777216}, {1048577, 4194304, 42, 33554432},
    {2097152, 4194304, 42, 33554432}, {2097153, 0, 0, -1}, {-1, 0, 0, -1}, {2147483647, 0, 0, -1},
};

struct HomeCase { int64_t e; int64_t slots; uint64_t home; };
static const HomeCase homes[] = {
    // e, slots -> the home slot: every bit of e and of the product counts
    {0, 256, 0}, {1, 256, 158}, {2, 256, 60}, {1, 512, 316}, {1, 4194304, 2592222}, {3, 4194304, 3582363},
    {4294967296, 256, 127}, {4294967297, 256, 29}, {4294967297, 4194304, 483453}, {2147483648, 256, 191}, {7, 4096, 1336},
    {2147483655, 4096, 306}, {4294967303, 4096, 3372}, {123, 1048576, 19063}, {1099511627899, 1048576, 324153},
    {4611686018427387904, 256, 64}, {9223372036854775807, 256, 225}, {9223372036854775807, 4194304, 3699233},
};

struct ReverseCase { int64_t n; int32_t via, sorted; bool built; int want; };
static const ReverseCase reverses[] = {
    // n, via, rows_sorted (1, 0, -1: never checked), the reverse is built -> code
    {0, 0, 1, false, OK}, {1, 0, 1, false, OK}, {2147483647, 0, 1, true, OK}, {2147483648, 0, 1, true, COUNT}, {-1, 0, 1, true, COUNT},
    {5, 0, 0, true, UNSORTED}, {5, 0, -1, true, UNSORTED}, {5, 1, 0, true, OK}, {5, 1, -1, true, OK}, {5, 1, 1, false, NOREV},
    {5, 1, 0, false, NOREV}, {5, 2, 1, true, VIA}, {5, -1, 1, true, VIA}, {0, 1, 1, false, NOREV}, {0, 0, 0, true, UNSORTED},
    // the order of the checks
    {-1, 2, 0, false, COUNT}, {5, 2, 0, false, VIA},
};

struct BuildCase { int32_t k; int64_t bytes; int want; };
static const BuildCase builds[] = {
    {0, 2048, OK}, {0, 2047, SETBYTES}, {128, 2048, OK}, {129, 2048, SETBYTES}, {129, 4096, OK}, {2097152, 33554432, OK},
    {2097152, 33554431, SETBYTES}, {2097153, 1 << 30, SETSIZE}, {-1, 1 << 30, SETSIZE}, {-1, 0, SETSIZE},
};

struct ContainsCase { int32_t k; int64_t bytes, m; int want; };
static const ContainsCase contains[] = {
    {1, 2048, 0, OK}, {1, 2048, 2147483647, OK}, {1, 2048, 2147483648, SLOTS}, {1, 2048, -1, SLOTS}, {1, 2047, 5, SETBYTES},
    {2097153, 1 << 30, 5, SETSIZE}, {2097153, 0, -1, SETSIZE}, {1, 2047, -1, SETBYTES},
};

struct ScratchCase { int64_t m, bytes; };
static const ScratchCase scratches[] = {
    // m -> 8 (tiles of 1 024 + 1 + sums per 256 tiles); -1 for an illegal m
    {0, 8}, {1, 24}, {1024, 24}, {1025, 32}, {262144, 8 * 258}, {262145, 8 * 260}, {1073741824, 8 * (1048576 + 1 + 4096)},
    {1073741825, -1}, {-1, -1},
};

struct CountCase { int64_t m; int32_t k; int64_t set_bytes, scratch; int want; };
static const CountCase counts[] = {
    {0, 0, 2048, 8, OK}, {0, 0, 2048, 7, SCRATCH}, {1025, 1, 2048, 32, OK}, {1025, 1, 2048, 31, SCRATCH}, {1025, 1, 2047, 32, SETBYTES},
    {1073741824, 1, 2048, 1 << 24, OK}, {1073741825, 1, 2048, 1 << 24, SLOTS}, {-1, 1, 2048, 1 << 24, SLOTS}, {5, 2097153, 1 << 30, 24, SETSIZE},
    // the order of the checks
    {-1, -1, 0, 0, SLOTS}, {5, -1, 0, 0, SETSIZE}, {5, 1, 0, 0, SETBYTES},
};

struct EdgesCase { int64_t m; int32_t k; int64_t set_bytes, scratch, cap; uint64_t in[3], out[3]; int want; };
static const EdgesCase edges[] = {
    // m, k, set_bytes, scratch_bytes, cap, the addresses of dst / src / eid in and out -> code.  m = 1 000: inputs of 4 000, 4 000, 8 000 bytes
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 600000}, OK},
    {1000, 1, 2048, 24, 0, {100000, 200000, 300000}, {100000, 200000, 300000}, OK},                 // cap 0: no byte of an output
    {1000, 1, 2048, 24, 0, {100000, 200000, 300000}, {100004, 203996, 300008}, OK},                 // ... nor with a pointer inside an input
    {0, 1, 2048, 8, 1000, {400004, 500100, 607992}, {400000, 500000, 600000}, OK},                  // m 0: no byte of an input, inside an output
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {100000, 500000, 600000}, ALIAS},           // dst_out == dst
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 203999, 600000}, ALIAS},           // src_out starts at src's last byte
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 204000, 600000}, OK},              // ... and right behind it
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 196000, 600000}, OK},              // src_out ends where src starts
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 196001, 600000}, ALIAS},
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 307999}, ALIAS},           // eid_out inside eid: 8 bytes an entry
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 308000}, OK},
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 103999}, ALIAS},           // eid_out over dst
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {303000, 500000, 600000}, ALIAS},           // dst_out over eid
    {1000, 1, 2048, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 0}, OK},                   // no eid_out
    {1000, 1, 2048, 24, 2000, {100000, 200000, 300000}, {92001, 500000, 600000}, ALIAS},            // cap entries on the output side
    {1000, 1, 2048, 24, 2000, {100000, 200000, 300000}, {92000, 500000, 600000}, OK},
    {1000, 1, 2048, 24, 2147483647, {1ull << 40, 2ull << 40, 3ull << 40}, {4ull << 40, 5ull << 40, 6ull << 40}, OK},
    {1000, 1, 2048, 24, 2147483648, {1ull << 40, 2ull << 40, 3ull << 40}, {4ull << 40, 5ull << 40, 6ull << 40}, CAP},
    {1000, 1, 2048, 24, -1, {100000, 200000, 300000}, {400000, 500000, 600000}, CAP},
    {1000, 1, 2048, 23, 1000, {100000, 200000, 300000}, {400000, 500000, 600000}, SCRATCH},
    {1000, 1, 2047, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 600000}, SETBYTES},
    {1000, 2097153, 1 << 30, 24, 1000, {100000, 200000, 300000}, {400000, 500000, 600000}, SETSIZE},
    {1073741825, 1, 2048, 1 << 24, 1000, {1ull << 40, 2ull << 40, 3ull << 40}, {4ull << 40, 5ull << 40, 6ull << 40}, SLOTS},
    // the order of the checks
    {-1, -1, 0, 0, -1, {100000, 200000, 300000}, {100000, 200000, 300000}, SLOTS},
    {1000, 1, 2048, 0, -1, {100000, 200000, 300000}, {100000, 200000, 300000}, CAP},
    {1000, 1, 2048, 0, 1000, {100000, 200000, 300000}, {100000, 200000, 300000}, SCRATCH},
};

static int code(ExcludeRefusal r)
{
    switch (r) {
    case ExcludeRefusal::Ok: return OK;
    case ExcludeRefusal::Count: return COUNT;
    case ExcludeRefusal::Via: return VIA;
    case ExcludeRefusal::Unsorted: return UNSORTED;
    case ExcludeRefusal::NoReverse: return NOREV;
    case ExcludeRefusal::SetSize: return SETSIZE;
    case ExcludeRefusal::SetBytes: return SETBYTES;
    case ExcludeRefusal::Slots: return SLOTS;
    case ExcludeRefusal::Capacity: return CAP;
    case ExcludeRefusal::Scratch: return SCRATCH;
    case ExcludeRefusal::Alias: return ALIAS;
    }
    return -1;
}

static int check(const char* what, long long a, long long b, ExcludeRefusal r, int want)
{
    int bad = 0;
    if (code(r) != want) { printf("MISMATCH %s %lld %lld: got %d, want %d\n", what, a, b, code(r), want); bad++; }
    if (exclude_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    return bad;
}

int main()
{
    int bad = 0, n = 0;
    if (EDGE_SET_EMPTY_KEY != -1 || (uint64_t)EDGE_SET_EMPTY_KEY != 0xFFFFFFFFFFFFFFFFull) { printf("MISMATCH: the empty key is all-ones\n"); bad++; }
    for (const SizeCase& c : sizes) {
        n++;
        const bool legal = c.bytes >= 0;
        if (edge_set_bytes(c.k) != c.bytes || (legal && (edge_set_slots(c.k) != c.slots || edge_set_shift(c.slots) != c.shift))) {
            printf("MISMATCH set of %d ids: slots %lld shift %d bytes %lld, want %lld %d %lld\n", c.k, (long long)edge_set_slots(legal ? c.k : 0),
                   legal ? edge_set_shift(c.slots) : 0, (long long)edge_set_bytes(c.k), (long long)c.slots, c.shift, (long long)c.bytes);
            bad++;
        }
    }
    for (const HomeCase& c : homes) {
        n++;
        const uint64_t got = edge_set_home(c.e, edge_set_shift(c.slots));
        if (got != c.home || got >= (uint64_t)c.slots) {
            printf("MISMATCH home of %lld in %lld slots: got %llu, want %llu\n", (long long)c.e, (long long)c.slots, (unsigned long long)got,
                   (unsigned long long)c.home);
            bad++;
        }
    }
    for (const ReverseCase& c : reverses) { n++; bad += check("reverse ids n, via", c.n, c.via, reverse_edge_ids_refusal(c.n, c.via, c.sorted, c.built), c.want); }
    for (const BuildCase& c : builds) { n++; bad += check("set build k, bytes", c.k, c.bytes, edge_set_build_refusal(c.k, c.bytes), c.want); }
    for (const ContainsCase& c : contains) { n++; bad += check("set contains k, m", c.k, c.m, edge_set_contains_refusal(c.k, c.bytes, c.m), c.want); }
    for (const ScratchCase& c : scratches) {
        n++;
        if (edge_filter_scratch_bytes(c.m) != c.bytes) {
            printf("MISMATCH scratch of %lld edges: got %lld, want %lld\n", (long long)c.m, (long long)edge_filter_scratch_bytes(c.m), (long long)c.bytes);
            bad++;
        }
    }
    for (const CountCase& c : counts) { n++; bad += check("filter count m, k", c.m, c.k, edge_filter_count_refusal(c.m, c.k, c.set_bytes, c.scratch), c.want); }
    for (const EdgesCase& c : edges) {
        n++;
        bad += check("filter edges m, cap", c.m, c.cap, edge_filter_edges_refusal(c.m, c.k, c.set_bytes, c.scratch, c.cap, c.in, c.out), c.want);
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
