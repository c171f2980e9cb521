// Pins the rules of the reverse CSR (legion_amd/csrc/reverse_rule.h: which graphs legion_graph_build_reverse refuses, which class sorts
// a reverse row of a given length, the runs and merge passes of a long row, where each pass leaves the row, and the levels and scratch of
// the scan) over a literal table.  The expected values were written down from the rules as include/legion_hip.h and the issue's text
// state them, not from the header.
//   g++ -O1 -std=c++17 reverse_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/reverse_rule.h"

static_assert(LEGION_REVERSE_MAX_NODES == 268435456, "the tables below spell the limit out");
static_assert(LG_REVERSE_WAVE == 64 && LG_REVERSE_TILE == 4096 && LG_REVERSE_CHUNK == 2048, "the tables below spell the classes out");
enum { OK, NUL, MANY };
enum { NONE, WAVE, TILE, LONG };

struct RefusalCase { bool graph; int32_t n; int want; };
static const RefusalCase refusals[] = {
    // graph, node_num -> code
    {true, 0, OK}, {true, 1, OK}, {true, 6000, OK}, {true, 268435455, OK}, {true, 268435456, OK}, {true, 268435457, MANY},
    {true, 2147483647, MANY}, {false, 0, NUL}, {false, 6000, NUL},
    // the order of the checks
    {false, 268435457, NUL},
};

struct ClassCase { int64_t len; int cls; int64_t runs; int32_t passes; };
static const ClassCase classes[] = {
    // length -> class, runs of 4 096, merge passes
    {0, NONE, 0, 0}, {1, NONE, 1, 0}, {2, WAVE, 1, 0}, {63, WAVE, 1, 0}, {64, WAVE, 1, 0}, {65, TILE, 1, 0}, {4095, TILE, 1, 0},
    {4096, TILE, 1, 0}, {4097, LONG, 2, 1}, {8192, LONG, 2, 1}, {8193, LONG, 3, 2}, {12293, LONG, 4, 2}, {16384, LONG, 4, 2},
    {16385, LONG, 5, 3}, {20479, LONG, 5, 3}, {32768, LONG, 8, 3}, {32769, LONG, 9, 4}, {1000000, LONG, 245, 8},
    {(int64_t)1 << 32, LONG, 1048576, 20}, {((int64_t)1 << 32) + 1, LONG, 1048577, 21}, {-1, NONE, 0, 0},
};

struct BufferCase { int32_t passes, pass; int32_t want; int64_t width; };
static const BufferCase buffers[] = {
    // passes, pass -> where the row is after it (0 the output, 1 the scratch), and the width of the runs the pass merges
    {1, 0, 1, 0}, {1, 1, 0, 4096}, {2, 0, 0, 0}, {2, 1, 1, 4096}, {2, 2, 0, 8192}, {3, 0, 1, 0}, {3, 1, 0, 4096}, {3, 2, 1, 8192},
    {3, 3, 0, 16384}, {8, 0, 0, 0}, {8, 8, 0, 524288}, {21, 0, 1, 0}, {21, 21, 0, (int64_t)1 << 32},
};

struct ChunkCase { int64_t la, lb, want; };
static const ChunkCase chunks[] = {
    {4096, 4096, 4}, {4096, 1, 3}, {4096, 0, 2}, {1, 0, 1}, {2048, 0, 1}, {2049, 0, 2}, {8192, 4101, 7}, {(int64_t)1 << 31, (int64_t)1 << 31, 2097152},
};

struct ScanCase { int32_t n; int32_t levels; int64_t sums, scratch; };
static const ScanCase scans[] = {
    // node_num -> levels, sums per 256 counts, int64 words of scratch
    {0, 0, 0, 0}, {-1, 0, 0, 0}, {1, 1, 1, 1}, {256, 1, 1, 1}, {257, 1, 2, 2}, {1048575, 1, 4096, 4096}, {1048576, 1, 4096, 4096},
    {1048577, 2, 4097, 4097 + 17}, {1048833, 2, 4098, 4098 + 17}, {268435456, 2, 1048576, 1048576 + 4096},
};

struct CapCase { int64_t live, tile_rows, long_rows; };
static const CapCase caps[] = {
    {0, 0, 0}, {64, 0, 0}, {65, 1, 0}, {129, 1, 0}, {130, 2, 0}, {4096, 63, 0}, {4097, 63, 1}, {8193, 126, 1}, {8194, 126, 2},
};

static int code(ReverseRefusal r)
{
    switch (r) {
    case ReverseRefusal::Ok: return OK;
    case ReverseRefusal::Null: return NUL;
    case ReverseRefusal::TooMany: return MANY;
    }
    return -1;
}

static int code(ReverseClass c)
{
    switch (c) {
    case ReverseClass::None: return NONE;
    case ReverseClass::Wave: return WAVE;
    case ReverseClass::Tile: return TILE;
    case ReverseClass::Long: return LONG;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const RefusalCase& c : refusals) {
        n++;
        const ReverseRefusal r = reverse_refusal(c.graph, c.n);
        if (code(r) != c.want) {
            printf("MISMATCH refusal graph %d node_num %d: got %d, want %d\n", (int)c.graph, c.n, code(r), c.want);
            bad++;
        }
        if (reverse_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const ClassCase& c : classes) {
        n++;
        if (code(reverse_class(c.len)) != c.cls || reverse_runs(c.len) != c.runs || reverse_passes(c.len) != c.passes) {
            printf("MISMATCH length %lld: class %d runs %lld passes %d, want %d %lld %d\n", (long long)c.len, code(reverse_class(c.len)),
                   (long long)reverse_runs(c.len), reverse_passes(c.len), c.cls, (long long)c.runs, c.passes);
            bad++;
        }
    }
    for (const BufferCase& c : buffers) {
        n++;
        if (reverse_buffer_after(c.passes, c.pass) != c.want || (c.pass > 0 && reverse_run_width(c.pass) != c.width)) {
            printf("MISMATCH pass %d of %d: buffer %d width %lld, want %d %lld\n", c.pass, c.passes, reverse_buffer_after(c.passes, c.pass),
                   (long long)(c.pass > 0 ? reverse_run_width(c.pass) : 0), c.want, (long long)c.width);
            bad++;
        }
    }
    for (const ChunkCase& c : chunks) {
        n++;
        if (reverse_merge_chunks(c.la, c.lb) != c.want) {
            printf("MISMATCH chunks of %lld + %lld: got %lld, want %lld\n", (long long)c.la, (long long)c.lb,
                   (long long)reverse_merge_chunks(c.la, c.lb), (long long)c.want);
            bad++;
        }
    }
    for (const ScanCase& c : scans) {
        n++;
        if (reverse_scan_levels(c.n) != c.levels || reverse_scan_sums(c.n) != c.sums || reverse_scan_scratch(c.n) != c.scratch) {
            printf("MISMATCH scan of %d: levels %d sums %lld scratch %lld, want %d %lld %lld\n", c.n, reverse_scan_levels(c.n),
                   (long long)reverse_scan_sums(c.n), (long long)reverse_scan_scratch(c.n), c.levels, (long long)c.sums, (long long)c.scratch);
            bad++;
        }
    }
    for (const CapCase& c : caps) {
        n++;
        if (reverse_tile_rows_cap(c.live) != c.tile_rows || reverse_long_rows_cap(c.live) != c.long_rows) {
            printf("MISMATCH lists of %lld live entries: %lld and %lld rows, want %lld and %lld\n", (long long)c.live,
                   (long long)reverse_tile_rows_cap(c.live), (long long)reverse_long_rows_cap(c.live), (long long)c.tile_rows, (long long)c.long_rows);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
