// tile_scan.h -- the scan pieces of a workgroup of 256 lanes (four waves of 64) over int32_t or int64_t sums, each once: the sum and the
// exclusive prefix of one value per lane, and ONE workgroup's exclusive scan of at most 4 096 values in place.  Their users: row_offsets
// and LABOR's second level (the int64 launches of kernels_in_edges.hip) and unique_ids (kernels_link.hip).  The sampler's scans have
// other shapes (one wave over its bucket counts) and share the wave step only, wave_inclusive; the weight table's stays where it is.
// Device code; include inside namespace lg's files after legion_core.h.
#pragma once

#include <cstdint>

namespace lg {

#define LG_SCAN_THREADS 256
#define LG_SCAN_WAVES (LG_SCAN_THREADS / 64)                  // the entries of s_wave

// the sum of v over the workgroup, in every lane (both barriers inside: every lane of the workgroup calls it)
template <typename T>
__device__ __forceinline__ T tile_sum(T v, T* s_wave)
{
    for (int32_t off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    const T sum = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return sum;
}

// the sum of v over this lane of the wave and the lanes below it (lane = threadIdx.x & 63), exact in the first `width` lanes (a power of
// two): every active lane of the wave calls it.  The sampler's three scans (kernels_sample.hip) use it too
template <typename T>
__device__ __forceinline__ T wave_inclusive(T v, int32_t lane, int32_t width = 64)
{
    for (int32_t off = 1; off < width; off <<= 1) {
        const T y = __shfl_up(v, off, 64);
        if (lane >= off) v += y;
    }
    return v;
}

// the sum of v over the lanes of the workgroup below this one (both barriers inside: every lane of the workgroup calls it)
template <typename T>
__device__ __forceinline__ T tile_exclusive(T v, T* s_wave)
{
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive(v, lane);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T before = inc - v;
    for (int32_t w = 0; w < wave; w++) before += s_wave[w];
    __syncthreads();
    return before;
}

// ONE workgroup: a[0 .. n), n <= 4 096 (16 a thread), becomes its exclusive prefix sums; the total goes to total[0] and, unless null,
// to total2[0].  n == 0: the totals only, both 0
template <typename T>
__device__ __forceinline__ void tile_scan_in_place(T* a, int32_t n, T* total, T* total2, T* s_wave)
{
    const int32_t per = (n + LG_SCAN_THREADS - 1) / LG_SCAN_THREADS;  // a thread's run of consecutive values
    const int32_t t0 = min((int32_t)threadIdx.x * per, n), t1 = min(t0 + per, n);
    T sum = 0;
    for (int32_t t = t0; t < t1; t++) sum += a[t];
    T before = tile_exclusive(sum, s_wave);
    for (int32_t t = t0; t < t1; t++) {
        const T c = a[t];
        a[t] = before;
        before += c;
    }
    if (threadIdx.x == LG_SCAN_THREADS - 1) {                         // (the last thread's run ends the array, or is empty behind it)
        total[0] = before;
        if (total2) total2[0] = before;
    }
}

}  // namespace lg
