// Pins gather_plan (legion_amd/csrc/gather_plan.h: which gather_kernel instance a gather launches) over a table of shapes.  The
// expected values were worked out from the launch code the plan replaced, not from the plan itself.
//   g++ -O1 -std=c++17 gather_plan_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/gather_plan.h"

static const char* name(GatherFormat f)
{
    switch (f) {
        case GatherFormat::F32: return "F32";
        case GatherFormat::F32Tail: return "F32Tail";
        case GatherFormat::F32Scalar: return "F32Scalar";
        case GatherFormat::Bf16x8: return "Bf16x8";
        case GatherFormat::Bf16Copy: return "Bf16Copy";
        case GatherFormat::F32Narrow: return "F32Narrow";
    }
    return "?";
}

enum { F32 = LEGION_FEATURE_F32, BF16 = LEGION_FEATURE_BF16 };
enum { FULL = 4096, LANES = 512 };      // a full launch group: 512 lanes of 4096 rows (never few tiles)
struct Case {
    int dtype, out_dtype, D, pitch, grid_rows, n_lanes, rows_override;
    GatherPlan::Error error;
    GatherFormat format;
    int rows, unroll;
    bool tail;
};
using GF = GatherFormat;
static const GatherPlan::Error OK = GatherPlan::OK, BAD_DTYPE = GatherPlan::BAD_DTYPE, BAD_PITCH = GatherPlan::BAD_PITCH;

static const Case cases[] = {
    // float32 -> float32, 16-byte rows: 16 KB of source payload per tile for rows of 512 bytes and more, 32 KB below (+ 1/4 margin)
    {F32, F32, 128, 0, FULL, LANES, 0, OK, GF::F32, 32, 4, false},
    {F32, F32, 100, 0, FULL, LANES, 0, OK, GF::F32, 64, 4, false},
    {F32, F32, 64, 0, FULL, LANES, 0, OK, GF::F32, 128, 4, false},
    {F32, F32, 256, 0, FULL, LANES, 0, OK, GF::F32, 16, 4, false},
    {F32, F32, 1024, 0, FULL, LANES, 0, OK, GF::F32, 16, 4, false},
    {F32, F32, 4, 0, FULL, LANES, 0, OK, GF::F32, 256, 4, false},
    {F32, F32, 8, 0, FULL, LANES, 0, OK, GF::F32, 256, 4, false},
    {F32, F32, 124, 0, FULL, LANES, 0, OK, GF::F32, 64, 4, false},      // 496-byte rows: the 32 KB payload
    {F32, F32, 72, 0, FULL, LANES, 0, OK, GF::F32, 128, 4, false},      // 128 x 288 B = 36 KB: inside the margin
    {F32, F32, 80, 0, FULL, LANES, 0, OK, GF::F32, 128, 4, false},      // 40 KB: the margin's edge
    {F32, F32, 84, 0, FULL, LANES, 0, OK, GF::F32, 64, 4, false},       // 42 KB: past it
    {F32, F32, 160, 0, FULL, LANES, 0, OK, GF::F32, 32, 4, false},      // 32 x 640 B = 20 KB: the margin's edge of the 16 KB payload
    {F32, F32, 164, 0, FULL, LANES, 0, OK, GF::F32, 16, 4, false},
    // a launch of few tiles (fewer than 4096 over all lanes) takes 16-row tiles
    {F32, F32, 128, 0, 1024, 1, 0, OK, GF::F32, 16, 4, false},
    {F32, F32, 128, 0, 1024, 128, 0, OK, GF::F32, 32, 4, false},         // 32 tiles x 128 lanes = 4096
    {F32, F32, 128, 0, 1024, 127, 0, OK, GF::F32, 16, 4, false},
    {F32, F32, 4, 0, 1024, LANES, 0, OK, GF::F32, 16, 4, false},          // 4 tiles of 256 rows x 512 lanes
    // LEGION_GATHER_ROWS replaces the whole rule; what is not a tile size gives 64
    {F32, F32, 128, 0, FULL, LANES, 48, OK, GF::F32, 64, 4, false},
    {F32, F32, 128, 0, FULL, LANES, 256, OK, GF::F32, 256, 4, false},
    {F32, F32, 128, 0, FULL, LANES, 16, OK, GF::F32, 16, 4, false},
    {F32, F32, 128, 0, FULL, LANES, 128, OK, GF::F32, 128, 4, false},
    {F32, F32, 128, 0, 1024, 1, 256, OK, GF::F32, 256, 4, false},
    {F32, F32, 1024, 0, FULL, LANES, 1, OK, GF::F32, 64, 4, false},
    {F32, F32, 128, 0, FULL, LANES, -5, OK, GF::F32, 32, 4, false},
    // float32 -> float32, D % 4 != 0 and D > 4: 64 rows, 16 with few 64-row tiles or rows of more than 1 KB; no LEGION_GATHER_ROWS
    {F32, F32, 602, 0, FULL, LANES, 0, OK, GF::F32Tail, 16, 4, true},
    {F32, F32, 7, 0, FULL, LANES, 0, OK, GF::F32Tail, 64, 4, true},
    {F32, F32, 5, 0, FULL, LANES, 0, OK, GF::F32Tail, 64, 4, true},
    {F32, F32, 7, 0, 1024, 1, 0, OK, GF::F32Tail, 16, 4, true},
    {F32, F32, 7, 0, 1024, 256, 0, OK, GF::F32Tail, 64, 4, true},          // 16 tiles x 256 lanes = 4096
    {F32, F32, 7, 0, 1024, 255, 0, OK, GF::F32Tail, 16, 4, true},
    {F32, F32, 255, 0, FULL, LANES, 0, OK, GF::F32Tail, 64, 4, true},      // 64 x 1020 B <= 64 KB
    {F32, F32, 257, 0, FULL, LANES, 0, OK, GF::F32Tail, 16, 4, true},
    {F32, F32, 602, 0, FULL, LANES, 256, OK, GF::F32Tail, 16, 4, true},
    {F32, F32, 7, 0, FULL, LANES, 48, OK, GF::F32Tail, 64, 4, true},
    {F32, F32, 7, 0, FULL, LANES, 16, OK, GF::F32Tail, 64, 4, true},
    {F32, F32, 7, 0, 1024, 1, 256, OK, GF::F32Tail, 16, 4, true},
    // float32 -> float32, D < 4: always 64 rows
    {F32, F32, 3, 0, FULL, LANES, 0, OK, GF::F32Scalar, 64, 4, false},
    {F32, F32, 1, 0, FULL, LANES, 0, OK, GF::F32Scalar, 64, 4, false},
    {F32, F32, 2, 0, 1024, 1, 0, OK, GF::F32Scalar, 64, 4, false},
    {F32, F32, 3, 0, FULL, LANES, 256, OK, GF::F32Scalar, 64, 4, false},
    // bf16 storage -> float32: the rule over 2 P bytes per source row, P = D rounded up to 8
    {BF16, F32, 128, 128, FULL, LANES, 0, OK, GF::Bf16x8, 128, 4, false},
    {BF16, F32, 100, 104, FULL, LANES, 0, OK, GF::Bf16x8, 128, 4, false},
    {BF16, F32, 256, 256, FULL, LANES, 0, OK, GF::Bf16x8, 32, 4, false},
    {BF16, F32, 1024, 1024, FULL, LANES, 0, OK, GF::Bf16x8, 16, 4, false},
    {BF16, F32, 3, 8, FULL, LANES, 0, OK, GF::Bf16x8, 256, 4, false},
    {BF16, F32, 602, 608, FULL, LANES, 0, OK, GF::Bf16x8, 16, 4, false},
    {BF16, F32, 100, 112, FULL, LANES, 0, OK, GF::Bf16x8, 128, 4, false},   // a wider pitch than needed sizes the tile
    {BF16, F32, 128, 128, 1024, 1, 0, OK, GF::Bf16x8, 16, 4, false},
    {BF16, F32, 128, 128, FULL, LANES, 48, OK, GF::Bf16x8, 64, 4, false},
    {BF16, F32, 128, 128, FULL, LANES, 32, OK, GF::Bf16x8, 32, 4, false},
    // bf16 storage -> bf16 rows
    {BF16, BF16, 128, 128, FULL, LANES, 0, OK, GF::Bf16Copy, 128, 4, false},
    {BF16, BF16, 100, 104, FULL, LANES, 0, OK, GF::Bf16Copy, 128, 4, false},
    {BF16, BF16, 7, 8, FULL, LANES, 0, OK, GF::Bf16Copy, 256, 4, false},
    {BF16, BF16, 128, 128, 1024, 1, 0, OK, GF::Bf16Copy, 16, 4, false},
    {BF16, BF16, 128, 128, FULL, LANES, 256, OK, GF::Bf16Copy, 256, 4, false},
    // float32 storage -> bf16 rows: the rule over 4 D bytes per source row, half the unroll
    {F32, BF16, 128, 0, FULL, LANES, 0, OK, GF::F32Narrow, 32, 2, false},
    {F32, BF16, 100, 0, FULL, LANES, 0, OK, GF::F32Narrow, 64, 2, false},
    {F32, BF16, 3, 0, FULL, LANES, 0, OK, GF::F32Narrow, 256, 2, false},
    {F32, BF16, 7, 0, FULL, LANES, 0, OK, GF::F32Narrow, 256, 2, false},
    {F32, BF16, 602, 0, FULL, LANES, 0, OK, GF::F32Narrow, 16, 2, false},
    {F32, BF16, 128, 0, 1024, 1, 0, OK, GF::F32Narrow, 16, 2, false},
    {F32, BF16, 128, 0, FULL, LANES, 128, OK, GF::F32Narrow, 128, 2, false},
    {F32, BF16, 100, 7, FULL, LANES, 0, OK, GF::F32Narrow, 64, 2, false},    // the pitch of a float32 source is not looked at
    // refused: an unknown dtype or output dtype; bf16 source rows with a pitch below D or not a multiple of 8
    {2, F32, 128, 0, FULL, LANES, 0, BAD_DTYPE, GF::F32, 0, 0, false},
    {-1, F32, 128, 0, FULL, LANES, 0, BAD_DTYPE, GF::F32, 0, 0, false},
    {F32, 2, 128, 0, FULL, LANES, 0, BAD_DTYPE, GF::F32, 0, 0, false},
    {BF16, -1, 128, 128, FULL, LANES, 0, BAD_DTYPE, GF::F32, 0, 0, false},
    {2, F32, 100, 100, FULL, LANES, 0, BAD_DTYPE, GF::F32, 0, 0, false},     // the dtype is checked first
    {BF16, F32, 100, 100, FULL, LANES, 0, BAD_PITCH, GF::F32, 0, 0, false},
    {BF16, F32, 100, 96, FULL, LANES, 0, BAD_PITCH, GF::F32, 0, 0, false},
    {BF16, BF16, 100, 100, FULL, LANES, 0, BAD_PITCH, GF::F32, 0, 0, false},
    {BF16, BF16, 128, 0, FULL, LANES, 0, BAD_PITCH, GF::F32, 0, 0, false},
};

int main()
{
    int bad = 0, n = 0;
    for (const Case& c : cases) {
        n++;
        const GatherPlan p = gather_plan(c.dtype, c.out_dtype, c.D, c.pitch, c.grid_rows, c.n_lanes, c.rows_override);
        const GatherFormatInfo fi = gather_info(p.format);
        // (and the plan's tile size is one the format has instances for)
        const bool ok = p.error == c.error && (c.error != GatherPlan::OK || (p.format == c.format && p.rows == c.rows && fi.unroll == c.unroll &&
                                                                           fi.tail == c.tail && (fi.tiles & p.rows) != 0));
        if (!ok) {
            printf("MISMATCH dtype %d out %d D %d pitch %d grid_rows %d lanes %d override %d: got error %d %s rows %d unroll %d tail %d, "
                   "want error %d %s rows %d unroll %d tail %d\n",
                   c.dtype, c.out_dtype, c.D, c.pitch, c.grid_rows, c.n_lanes, c.rows_override, (int)p.error, name(p.format), p.rows,
                   fi.unroll, (int)fi.tail, (int)c.error, name(c.format), c.rows, c.unroll, (int)c.tail);
            bad++;
        }
    }
    printf("%d shapes, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
