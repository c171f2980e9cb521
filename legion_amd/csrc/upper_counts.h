// upper_counts.h -- the interleaved upper-bound searches by which the kernels that expand CSR rows over slots (kernels_in_edges.hip,
// kernels_labor.hip) find a slot's row in a list of offsets.  Device code; include inside namespace lg's files after legion_core.h.
#pragma once

#include <cstdint>

namespace lg {

// K upper bounds at once, their chains of dependent loads interleaved: c[j] = #{ v in [0, len) : a[v] <= q[j] } for a non-decreasing a
// (for any other a: some value in [0, len]); len <= 0 or !live[j]: 0.  Reads a[0 .. len) only.
template <int32_t K>
__device__ __forceinline__ void upper_counts(const int64_t* a, int32_t len, const int64_t (&q)[K], const bool (&live)[K], int32_t (&c)[K])
{
    int32_t m[K];
#pragma unroll
    for (int32_t j = 0; j < K; j++) {
        c[j] = 0;
        m[j] = live[j] ? max(len, 0) : 0;
    }
    bool more = true;
    while (more) {                                                    // each trip halves every m[j] > 0: at most 21 trips
        more = false;
        int64_t v[K];
#pragma unroll
        for (int32_t j = 0; j < K; j++) v[j] = m[j] > 0 ? a[c[j] + (m[j] >> 1)] : 0;      // (c + m / 2 < c + m <= len)
#pragma unroll
        for (int32_t j = 0; j < K; j++) {
            if (m[j] > 0) {
                const int32_t half = m[j] >> 1;
                if (v[j] <= q[j]) { c[j] += half + 1; m[j] -= half + 1; }
                else m[j] = half;
                more |= m[j] > 0;
            }
        }
    }
}

}  // namespace lg
