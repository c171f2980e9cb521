// walk_step.h -- one transition of a random walk over the full CSR, shared by the walk (kernels_walk.hip) and PinSAGE's neighbour
// sampler (kernels_pinsage.hip): rule steps 1-5 of legion_random_walk (include/legion_hip.h).  Device code only.
#pragma once

#include "legion_core.h"
#include "draw_rule.h"

namespace lg {

// {indptr[v], indptr[v + 1]}: adjacent int64s, 8-byte aligned
struct __attribute__((packed, aligned(8))) WalkRowPair { int64_t s, e; };

// one transition of walk rule steps 1-5: the next vertex, or -1 when the walk has ended or ends here; eid = its position in col
template <bool WEIGHTED, bool RESTART>
__device__ __forceinline__ int32_t walk_step(const WalkParams& p, int32_t v, uint32_t n1, int64_t& eid)      // n1 = n + 1
{
    eid = -1;
    if ((uint32_t)v >= (uint32_t)p.node_num) return -1;                     // 1. ended (or a bad seed): before any load
    if (RESTART) {                                                          // 2.
        const uint32_t y = minstd_pow(n1 + 0x80000000u);
        double r2 = (double)(uint32_t)(y - 1u);
        r2 /= 2147483646.0;
        if (r2 < (double)p.restart_prob) return -1;
    }
    const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + v);      // 3. (v + 1 <= node_num: inside indptr)
    const int64_t s = row.s;
    const int32_t D = (int32_t)(row.e - s);
    if (D <= 0) return -1;
    const uint32_t x = minstd_pow(n1);                                      // 4.
    int32_t pick;
    if (WEIGHTED) {
        const float* c = p.edge_cdf + s;
        const float T = c[D - 1];
        if (!(T > 0.0f)) return -1;
        const double t = weighted_target(x, T);
        int32_t lo = 0, m = D;
        while (m > 0) weighted_step(c[lo + (m >> 1)], t, lo, m);            // probes lo + m / 2 < lo + m <= D
        pick = min(lo, D - 1);
    } else {
        pick = draw_from_x(x, D);                                           // r < 1: pick <= D - 1
    }
    const int32_t u = p.col[s + pick];                                      // 5.
    if (u < 0) return -1;
    eid = s + pick;
    return u;
}

}  // namespace lg
