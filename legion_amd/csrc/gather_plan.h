// gather_plan.h -- which gather_kernel instance a gather launches: its row format, tile size (ROWS), UNROLL and TAIL.  Host-only,
// no HIP: launch_gather_impl (kernels_gather.hip) launches the plan, tests/cpu/gather_plan_test.cpp pins it over a table of shapes.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"

enum class GatherFormat { F32, F32Tail, F32Scalar, Bf16x8, Bf16Copy, F32Narrow };

// What a format fixes for its instances: UNROLL (chunks in flight per lane), TAIL (the scalar pass over a row's last D % 4 floats),
// bf16 source rows (2 P bytes per row for the tile rule, else 4 D) and its tile sizes (ROWS, a mask of 16 ... 256).
struct GatherFormatInfo { int32_t unroll; bool tail, src_bf16; int32_t tiles; };
constexpr GatherFormatInfo GATHER_FORMATS[] = {      // in GatherFormat order
    {4, false, false, 16 | 32 | 64 | 128 | 256},     // F32: float32 -> float32, D % 4 == 0
    {4, true, false, 16 | 64},                       // F32Tail: float32 -> float32, D % 4 != 0 and D > 4
    {4, false, false, 64},                           // F32Scalar: float32 -> float32, D < 4
    {4, false, true, 16 | 32 | 64 | 128 | 256},      // Bf16x8: bf16 -> float32
    {4, false, true, 16 | 32 | 64 | 128 | 256},      // Bf16Copy: bf16 -> bf16
    {2, false, false, 16 | 32 | 64 | 128 | 256},     // F32Narrow: float32 -> bf16; 32 bytes per chunk, so half the chunks in flight
};                                                   // per lane keep the others' bytes in flight, and its registers the 8-wave budget
constexpr GatherFormatInfo gather_info(GatherFormat f) { return GATHER_FORMATS[(int)f]; }

// BAD_DTYPE: dtype or out_dtype is no LEGION_FEATURE_*; BAD_PITCH: bf16 source rows with a pitch below D or not a multiple of 8
struct GatherPlan {
    enum Error { OK, BAD_DTYPE, BAD_PITCH } error;
    GatherFormat format;   // UNROLL and TAIL are gather_info(format)'s
    int32_t rows;          // ROWS: rows per tile
};

// dtype, out_dtype, D, pitch: those of GatherParams; grid_rows: the rows a lane typically has (they size the grid); rows_override:
// LegionTuning.gather_rows_per_wg (LEGION_GATHER_ROWS), 0 = the rule below
static inline GatherPlan gather_plan(int32_t dtype, int32_t out_dtype, int32_t D, int32_t pitch, int32_t grid_rows, int32_t n_lanes,
                                     int32_t rows_override)
{
    const bool src16 = dtype == LEGION_FEATURE_BF16, out16 = out_dtype == LEGION_FEATURE_BF16;
    if ((!src16 && dtype != LEGION_FEATURE_F32) || (!out16 && out_dtype != LEGION_FEATURE_F32)) return {GatherPlan::BAD_DTYPE};
    if (src16 && (pitch < D || pitch % 8 != 0)) return {GatherPlan::BAD_PITCH};
    GatherPlan p{GatherPlan::OK};
    p.format = out16 ? (src16 ? GatherFormat::Bf16Copy : GatherFormat::F32Narrow)
                     : src16 ? GatherFormat::Bf16x8 : D % 4 == 0 ? GatherFormat::F32 : D > 4 ? GatherFormat::F32Tail : GatherFormat::F32Scalar;
    // a launch of one or a few lanes (the Runner's per-batch hand-over) has too few 64-row tiles to keep 256 CUs busy: 16-row
    // tiles give it 4 x the workgroups
    auto few_tiles = [&](int32_t rows) { return (int64_t)((grid_rows + rows - 1) / rows) * n_lanes < 4096; };
    if (p.format == GatherFormat::F32Scalar) {          // (LEGION_GATHER_ROWS does not apply to these two)
        p.rows = 64;
    } else if (p.format == GatherFormat::F32Tail) {
        p.rows = few_tiles(64) || (int64_t)D * 4 * 64 > 65536 ? 16 : 64;
    } else if (rows_override > 0) {
        p.rows = rows_override == 16 || rows_override == 32 || rows_override == 128 || rows_override == 256 ? rows_override : 64;
    } else {
        // The tile whose SOURCE payload is 16 KB for rows of 512 bytes and more, 32 KB below: measured for float32 rows in round 3
        // (DESIGN.md 4.1); the bf16 formats take the same rule over their source rows, measured only against float32 at the headline
        // shapes, not against other tile sizes (tools/feature_dtype_ab.py --rows R is the timing sweep still to run; every format is
        // CHECKED at every tile size, tests/test_gpu_gather_formats.py).
        const int64_t row_bytes = gather_info(p.format).src_bf16 ? (int64_t)pitch * 2 : (int64_t)D * 4;
        const int64_t payload = row_bytes >= 512 ? 16384 : 32768;
        p.rows = 16;
        while (p.rows < 256 && (int64_t)p.rows * 2 * row_bytes <= payload + payload / 4) p.rows *= 2;
        if (few_tiles(p.rows)) p.rows = 16;
    }
    return p;
}
