// aggregate_device.h -- what the segmented row reductions share on the device (kernels_aggregate.hip, kernels_attention.hip): a segment's
// clamped bounds, the wave's LDS hand-over, the bf16 rounding, the scan over the chunk counts, a unit of a stored row as float32 and
// the stores of a lane's columns.  Moved here from kernels_aggregate.hip as they stood; the constants are aggregate_rule.h's.
#pragma once

#include "legion_core.h"
#include "aggregate_rule.h"
#include "row_slots.h"
#include "tile_scan.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_AGG_MAX_WG == LG_WALK_MAX_WG, "the grid is the walks' cap");

// the int64 scan's outer launches (kernels_in_edges.hip)
__global__ void scan_sum_kernel(const int64_t* values, int32_t n, int32_t n_sums, int64_t* sums);
__global__ void scan_apply_kernel(int64_t* values, int32_t n, int32_t n_sums, const int64_t* sums);

// the entries [s, e) of segment d inside ids, whatever offsets hold
__device__ __forceinline__ void aggregate_segment(const AggregateParams& a, int64_t d, int64_t& s, int64_t& e)
{
    s = min(max(a.offsets[d], (int64_t)0), a.M);
    e = min(max(a.offsets[d + 1], s), a.M);
}

// LDS written by some lanes of a wave is read by others of it
__device__ __forceinline__ void aggregate_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// torch's float32 -> bfloat16 rounding (the gather's: round to nearest even, NaNs kept quiet NaNs)
__device__ __forceinline__ uint32_t aggregate_bf16_rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// first_chunk[0 .. n) holds the counts: they become their exclusive prefix sums and first_chunk[n] their total
static void aggregate_scan(hipStream_t s, int64_t* first_chunk, int32_t n, int64_t* sums)
{
    const int32_t n_sums = (int32_t)aggregate_scan_sums(n);
    if (aggregate_scan_levels(n) < 2) {
        launch_scan_int64(s, first_chunk, n, sums, n_sums, false, first_chunk + n, nullptr);
        return;
    }
    int64_t* sums2 = sums + n_sums;
    scan_sum_kernel<<<walk_grid(n), LG_SCAN_THREADS, 0, s>>>(first_chunk, n, n_sums, sums);
    launch_scan_int64(s, sums, n_sums, sums2, (n_sums + 255) / 256, false, first_chunk + n, nullptr);
    scan_apply_kernel<<<walk_grid(n), LG_SCAN_THREADS, 0, s>>>(first_chunk, n, n_sums, sums);
    hipCheckError();
}

// one unit of a stored row as W float32
template <AggregateRow ROW> struct AggregateUnit;
template <> struct AggregateUnit<AggregateRow::F32x4> {
    typedef float f4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void load(uint64_t row, int32_t u, float (&x)[4])
    {
        const f4 v = ((const LG_G f4*)row)[u];                        // D % 4 == 0: rows are 16-byte aligned
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
};
template <> struct AggregateUnit<AggregateRow::F32x1> {
    static __device__ __forceinline__ void load(uint64_t row, int32_t u, float (&x)[1]) { x[0] = ((const LG_G float*)row)[u]; }
};
template <> struct AggregateUnit<AggregateRow::Bf16x8> {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void load(uint64_t row, int32_t u, float (&x)[8])
    {
        const u4 v = ((const LG_G u4*)row)[u];                        // the pitch is a multiple of 8: the pad is inside the row
        const u4 lo = v << 16, hi = v & 0xFFFF0000u;                  // elements 2k, 2k + 1 (bits << 16, exact)
        x[0] = __uint_as_float(lo.x); x[1] = __uint_as_float(hi.x); x[2] = __uint_as_float(lo.y); x[3] = __uint_as_float(hi.y);
        x[4] = __uint_as_float(lo.z); x[5] = __uint_as_float(hi.z); x[6] = __uint_as_float(lo.w); x[7] = __uint_as_float(hi.w);
    }
};

// columns [col0, col0 + W) of a float32 row of D: 16-byte stores (dword aligned) where the unit is whole, else its columns below D
template <int32_t W>
__device__ __forceinline__ void aggregate_store_f32(float* row, int32_t D, int32_t col0, const float (&v)[W])
{
    typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
    if constexpr (W >= 4) {
        if (col0 + W <= D) {
#pragma unroll
            for (int32_t k = 0; k < W; k += 4) *(LG_G v4u*)(row + col0 + k) = v4u{v[k], v[k + 1], v[k + 2], v[k + 3]};
            return;
        }
    }
#pragma unroll
    for (int32_t k = 0; k < W; k++)
        if (col0 + k < D) row[col0 + k] = v[k];
}

// the same of a bf16 row (stride D, no pad): dwords where the rows are dword aligned and the unit is whole
template <int32_t W>
__device__ __forceinline__ void aggregate_store_bf16(uint16_t* row, int32_t D, int32_t col0, const float (&v)[W])
{
    if constexpr (W >= 2) {
        if ((D & 1) == 0 && col0 + W <= D) {
#pragma unroll
            for (int32_t k = 0; k < W; k += 2)
                *(uint32_t*)(row + col0 + k) = aggregate_bf16_rne(v[k]) | (aggregate_bf16_rne(v[k + 1]) << 16);
            return;
        }
    }
#pragma unroll
    for (int32_t k = 0; k < W; k++)
        if (col0 + k < D) row[col0 + k] = (uint16_t)aggregate_bf16_rne(v[k]);
}

}  // namespace lg
