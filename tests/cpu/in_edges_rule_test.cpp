// Pins the argument rules of the full-neighbour ops (legion_amd/csrc/in_edges_rule.h: which calls legion_row_offsets and legion_in_edges
// refuse, and the scratch size of the first) over a literal table.  The expected codes were written down from the rules as
// include/legion_hip.h documents them, not from the header.
//   g++ -O1 -std=c++17 in_edges_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/in_edges_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576, "the tables below spell the limit out");
enum { OK, CNT, MANY, SLOTS, SCR };

struct OffCase { int32_t n; int64_t scratch; int want; };
static const OffCase offs[] = {
    // n, scratch_bytes -> code
    {100, 8, OK}, {100, 7, SCR}, {100, 0, SCR}, {100, -1, SCR}, {100, (int64_t)1 << 40, OK},
    {0, 0, OK}, {0, -1, SCR}, {1, 8, OK}, {1, 7, SCR}, {256, 8, OK}, {257, 8, SCR}, {257, 16, OK}, {257, 15, SCR},
    {1048576, 32768, OK}, {1048576, 32767, SCR}, {-1, (int64_t)1 << 40, CNT}, {1048577, (int64_t)1 << 40, MANY},
    {2147483647, (int64_t)1 << 40, MANY},
    // the order of the checks
    {-1, -1, CNT}, {1048577, -1, MANY},
};

struct EdgeCase { int32_t n; int64_t m; int want; };
static const EdgeCase edges[] = {
    // n, m -> code
    {100, 1000, OK}, {0, 0, OK}, {0, 5, OK}, {100, 0, OK}, {1048576, 2147483647LL, OK}, {100, 2147483647LL, OK},
    {100, 2147483648LL, SLOTS}, {100, -1, SLOTS}, {100, (int64_t)1 << 40, SLOTS}, {100, -9223372036854775807LL, SLOTS},
    {-1, 1000, CNT}, {1048577, 1000, MANY},
    // the order of the checks
    {-1, -1, CNT}, {1048577, 2147483648LL, MANY},
};

struct BytesCase { int32_t n; int64_t want; };
static const BytesCase sizes[] = {
    // 8 x the tiles of 256 rows
    {0, 0}, {1, 8}, {255, 8}, {256, 8}, {257, 16}, {524288, 16384}, {524289, 16392}, {1048576, 32768}, {-1, -1}, {1048577, -1},
};

static int code(InEdgesRefusal r)
{
    switch (r) {
    case InEdgesRefusal::Ok: return OK;
    case InEdgesRefusal::Count: return CNT;
    case InEdgesRefusal::TooMany: return MANY;
    case InEdgesRefusal::Slots: return SLOTS;
    case InEdgesRefusal::Scratch: return SCR;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const OffCase& c : offs) {
        n++;
        const InEdgesRefusal r = row_offsets_refusal(c.n, c.scratch);
        if (code(r) != c.want) {
            printf("MISMATCH row_offsets n %d scratch %lld: got %d, want %d\n", c.n, (long long)c.scratch, code(r), c.want);
            bad++;
        }
        if (in_edges_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const EdgeCase& c : edges) {
        n++;
        const InEdgesRefusal r = in_edges_refusal(c.n, c.m);
        if (code(r) != c.want) {
            printf("MISMATCH in_edges n %d m %lld: got %d, want %d\n", c.n, (long long)c.m, code(r), c.want);
            bad++;
        }
        if (in_edges_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (row_offsets_scratch_bytes(c.n) != c.want) {
            printf("MISMATCH scratch bytes of %d: got %lld, want %lld\n", c.n, (long long)row_offsets_scratch_bytes(c.n), (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
