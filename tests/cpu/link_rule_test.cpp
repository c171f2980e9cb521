// Pins the argument rules of the link-prediction seed ops (legion_amd/csrc/link_rule.h: which calls legion_find_edges,
// legion_negative_sample and legion_unique_ids refuse, and the scratch size of the last) over a literal table.  The expected codes were
// written down from the rules as include/legion_hip.h documents them, not from the header.
//   g++ -O1 -std=c++17 link_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/id_table_rule.h"      // first: a changed copy of it shadows the one link_rule.h includes
#include "../../legion_amd/csrc/link_rule.h"

static_assert(LEGION_NEGATIVE_MAX_TRIES == 256 && LEGION_UNIQUE_MAX_IDS == 1048576, "the tables below spell both limits out");
enum { OK, CNT, FAN, IDX, EXC, TRY, SORT, MANY, SCR, ALIAS };

static const int64_t M31 = 2147483647;

struct NegCase { int32_t n, k; int64_t base; int32_t exclude, tries, sorted; int want; };
static const NegCase negs[] = {
    // rows, k, base, exclude, max_tries, rows checked sorted -> code
    {8, 5, 0, 0, 256, -1, OK}, {8, 5, 0, 1, 256, 0, OK}, {8, 5, 0, 2, 256, 1, OK}, {8, 5, 0, 3, 1, 1, OK}, {0, 1, 0, 3, 256, 1, OK},
    {0, 1, M31, 0, 1, -1, OK},
    // counts
    {-1, 5, 0, 0, 256, 1, CNT}, {8, 5, -1, 0, 256, 1, CNT}, {8, 0, 0, 0, 256, 1, FAN}, {8, -3, 0, 0, 256, 1, FAN},
    // the draw index
    {8, 5, M31 - 40, 0, 256, 1, OK}, {8, 5, M31 - 39, 0, 256, 1, IDX}, {2147483647, 1, 0, 0, 256, 1, OK}, {2147483647, 1, 1, 0, 256, 1, IDX},
    {2147483647, 2, 0, 0, 256, 1, IDX}, {2147483647, 2147483647, 0, 0, 256, 1, IDX}, {1, 1, M31, 0, 256, 1, IDX}, {0, 1, M31 + 1, 0, 256, 1, IDX},
    {8, 5, (int64_t)1 << 62, 0, 256, 1, IDX}, {8, 5, 9223372036854775807LL, 0, 256, 1, IDX},
    // exclude
    {8, 5, 0, -1, 256, 1, EXC}, {8, 5, 0, 4, 256, 1, EXC}, {8, 5, 0, 7, 256, 1, EXC},
    // tries
    {8, 5, 0, 0, 0, 1, TRY}, {8, 5, 0, 0, -1, 1, TRY}, {8, 5, 0, 0, 257, 1, TRY}, {8, 5, 0, 3, 256, 1, OK}, {8, 5, 0, 3, 255, 1, OK},
    // the graph's rows: only the edge exclusion asks
    {8, 5, 0, 2, 256, 0, SORT}, {8, 5, 0, 2, 256, -1, SORT}, {8, 5, 0, 3, 256, 0, SORT}, {8, 5, 0, 3, 256, -1, SORT}, {0, 5, 0, 2, 256, -1, SORT},
    {8, 5, 0, 0, 256, 0, OK}, {8, 5, 0, 1, 256, -1, OK},
    // the order of the checks: the first rule that fails names the refusal
    {-1, 0, M31, 4, 0, 0, CNT}, {8, 0, M31, 4, 0, 0, FAN}, {8, 5, M31, 4, 0, 0, IDX}, {8, 5, 0, 4, 0, 0, EXC}, {8, 5, 0, 2, 0, 0, TRY},
};

struct UniCase { int32_t m; int64_t scratch; uint64_t ids, unique, local, count; int want; };
static const uint64_t A = 0x100000;     // addresses far apart unless a case says otherwise
static const UniCase unis[] = {
    // m, scratch_bytes, the addresses of ids, unique_out, local_out, count_out -> code
    {100, 2852, A, 2 * A, 3 * A, 4 * A, OK}, {100, 2851, A, 2 * A, 3 * A, 4 * A, SCR}, {100, 1 << 30, A, 2 * A, 3 * A, 4 * A, OK},
    {0, 2048, A, 2 * A, 3 * A, 4 * A, OK}, {0, 2047, A, 2 * A, 3 * A, 4 * A, SCR}, {0, 0, A, 2 * A, 3 * A, 4 * A, SCR},
    {-1, 1 << 30, A, 2 * A, 3 * A, 4 * A, CNT}, {1048577, (int64_t)1 << 40, 64 * A, 128 * A, 192 * A, 4 * A, MANY},
    {1048576, 25182208, 64 * A, 128 * A, 192 * A, 4 * A, OK}, {1048576, 25182207, 64 * A, 128 * A, 192 * A, 4 * A, SCR},
    {100, -1, A, 2 * A, 3 * A, 4 * A, SCR},
    // outputs that overlap ids: wholly, by the last id, by the first; the count inside ids
    {100, 2852, A, A, 3 * A, 4 * A, ALIAS}, {100, 2852, A, 2 * A, A, 4 * A, ALIAS}, {100, 2852, A, A + 396, 3 * A, 4 * A, ALIAS},
    {100, 2852, A, A + 400, 3 * A, 4 * A, OK}, {100, 2852, A, 2 * A, A - 396, 4 * A, ALIAS}, {100, 2852, A, 2 * A, A - 400, 4 * A, OK},
    {100, 2852, A, 2 * A, 3 * A, A, ALIAS}, {100, 2852, A, 2 * A, 3 * A, A + 396, ALIAS}, {100, 2852, A, 2 * A, 3 * A, A + 400, OK},
    {100, 2852, A, 2 * A, 3 * A, A - 4, OK},
    // the order of the checks
    {-1, 0, A, A, A, A, CNT}, {1048577, 0, A, A, A, A, MANY}, {100, 0, A, A, A, A, SCR},
};

struct BytesCase { int32_t m; int64_t want; };
static const BytesCase sizes[] = {
    // 4 x (2 x slots + 2 m + tiles): slots the power of two >= max(2 m, 256), tiles of 256 ids
    {0, 2048}, {1, 2060}, {100, 2852}, {128, 3076}, {129, 5132}, {256, 6148}, {257, 10256}, {70001, 2658256},
    {1048576, 25182208}, {-1, -1}, {1048577, -1},
};

struct HomeCase { int32_t v; int32_t shift; uint32_t want; };
static const HomeCase homes[] = {
    // where the probe of an id starts in unique_ids' table: ((uint32)v * 2654435769) >> shift, computed with Python integers
    {1, 24, 158}, {144, 24, 255}, {123456, 19, 33}, {70001, 14, 261420}, {1000003, 11, 1767345}, {2147483647, 11, 1849616},
};

static int code(LinkRefusal r)
{
    switch (r) {
    case LinkRefusal::Ok: return OK;
    case LinkRefusal::Count: return CNT;
    case LinkRefusal::Fanout: return FAN;
    case LinkRefusal::DrawIndex: return IDX;
    case LinkRefusal::Exclude: return EXC;
    case LinkRefusal::Tries: return TRY;
    case LinkRefusal::Unsorted: return SORT;
    case LinkRefusal::TooMany: return MANY;
    case LinkRefusal::Scratch: return SCR;
    case LinkRefusal::Alias: return ALIAS;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const NegCase& c : negs) {
        n++;
        const LinkRefusal r = negative_sample_refusal(c.n, c.k, c.base, c.exclude, c.tries, c.sorted);
        if (code(r) != c.want) {
            printf("MISMATCH negative rows %d k %d base %lld exclude %d tries %d sorted %d: got %d, want %d\n", c.n, c.k, (long long)c.base,
                   c.exclude, c.tries, c.sorted, code(r), c.want);
            bad++;
        }
        if (link_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const UniCase& c : unis) {
        n++;
        const LinkRefusal r = unique_ids_refusal(c.m, c.scratch, c.ids, c.unique, c.local, c.count);
        if (code(r) != c.want) {
            printf("MISMATCH unique m %d scratch %lld ids %llx unique %llx local %llx count %llx: got %d, want %d\n", c.m, (long long)c.scratch,
                   (unsigned long long)c.ids, (unsigned long long)c.unique, (unsigned long long)c.local, (unsigned long long)c.count, code(r), c.want);
            bad++;
        }
        if (link_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (unique_ids_scratch_bytes(c.m) != c.want) {
            printf("MISMATCH scratch bytes of %d: got %lld, want %lld\n", c.m, (long long)unique_ids_scratch_bytes(c.m), (long long)c.want);
            bad++;
        }
    }
    for (const HomeCase& c : homes) {
        n++;
        if (id_table_home(c.v, c.shift) != c.want) {
            printf("MISMATCH home of %d at shift %d: got %u, want %u\n", c.v, c.shift, id_table_home(c.v, c.shift), c.want);
            bad++;
        }
    }
    n += 3;
    if (code(find_edges_refusal(-1)) != CNT || code(find_edges_refusal(0)) != OK || code(find_edges_refusal(2147483647)) != OK) {
        printf("MISMATCH find_edges\n");
        bad++;
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
