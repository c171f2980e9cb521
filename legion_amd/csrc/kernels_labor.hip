// kernels_labor.hip -- layer-neighbour sampling (LABOR-0 of Balin and Catalyurek; DGL's dgl.sampling.sample_labors) for gfx950 (CDNA4,
// wave64): in_edges' expansion of rows over slots (row_slots.h) with a predicate and a stable compaction.  Every source vertex has ONE
// random number, a hash of (src, salt); the entry src -> dst is kept iff that number lies below fanout / deg(dst), in integers
// (labor_rule.h, whose text runs here on the device).  The rules are the contracts in include/legion_hip.h.
// The layout is in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles of 1 024 consecutive
// slots, four per lane, 256 apart; every offset 64 bits wide, no workgroup waits for another and every loop carries its bound.  The
// count, scan and write passes are the kept-slot compaction's (kept_slots.h); this file brings the predicate.
// Bound: the col reads and, for rows of a degree near the fan-out, the stores; no MFMA.
#include "legion_core.h"
#include "labor_rule.h"
#include "kept_slots.h"

namespace lg {

// a lane's four slots and rule 3 for them
struct LaborSlots : LaneSlots {
    bool keep[LG_ROW_ILP];

    // Rules 1 -- 3 for the slots of a tile: the resolution, then the predicate: the degree is the row's whole one, a dead entry is
    // never kept.  One barrier inside, resolve_row_slots'
    __device__ __forceinline__ void resolve(const LaborParams& p, int64_t tile, int64_t* s_off)
    {
        resolve_row_slots(p.slots, tile, s_off, *this);
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++)
            keep[j] = e[j] >= 0 && src[j] >= 0 && labor_keep(labor_hash_keyed(p.key, src[j]), d[j], p.fanout);
    }
    __device__ __forceinline__ bool kept(int32_t j) const { return keep[j]; }
    __device__ __forceinline__ int32_t source(int32_t j) const { return src[j]; }
};

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void labor_count_kernel(LaborParams p)
{
    kept_count_tiles<LaborSlots>(p);
}

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void labor_edges_kernel(LaborParams p)
{
    kept_write_tiles<LaborSlots>(p);
}

// the arguments are the caller's to check (legion_labor_count, legion_labor_edges)
void launch_labor_count(hipStream_t s, const LaborParams& p) { launch_kept_count(s, labor_count_kernel, p); }
void launch_labor_edges(hipStream_t s, const LaborParams& p) { launch_kept_write(s, labor_edges_kernel, p); }

}  // namespace lg
