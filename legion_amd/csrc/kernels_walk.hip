// kernels_walk.hip -- random walks over the full CSR for gfx950 (CDNA4, wave64): DGL's dgl.sampling.random_walk.
//
// The rule is the contract in include/legion_hip.h (legion_random_walk): walk w starts at seeds[w]; step j draws with the sampler's own
// minstd power at index n = base + w * length + (j - 1) (draw_rule.h), uniformly over the row or by the graph's prefix table, after an
// optional restart draw; an ended walk is -1 from there on.  One transition is walk_step (walk_step.h, shared with kernels_pinsage.hip).
//
// A walk is a chain of dependent random loads -- per step the row-pointer pair, ceil(log2(D + 1)) probes of the table when weighted,
// one column entry -- so nothing inside a walk can overlap and the rate comes from walks in flight: one lane per walk, 256 lanes per
// workgroup, eight workgroups per CU (at most 64 VGPRs, at most 20 KiB of LDS), a grid that strides over tiles of 256 walks.  The tile,
// its LDS staging and the flush are WalkTile (walk_step.h, which says why the pitch is odd and why a chunk is 8 with edge ids).
// RESTART, WEIGHTED and EIDS are template flags: the plain instance has no restart draw, no table pointer and no edge-id staging.
// Bound: the part's rate of random requests at the occupancy above; no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"

namespace lg {

template <bool WEIGHTED, bool RESTART, bool EIDS>
__global__ __launch_bounds__(LG_WALK_THREADS, 8) void random_walk_kernel(WalkParams p)
{
    using Tile = WalkTile<EIDS>;
    __shared__ int32_t s_trace[Tile::TRACE];
    __shared__ int64_t s_eid[Tile::EID];
    Tile tile{s_trace, s_eid};
    for (int64_t t = blockIdx.x; t < walk_tiles(p.num_walks); t += gridDim.x) {
        int32_t v;                                        // the lane's walk: where it is, and n + 1 of its next draw index n
        uint32_t n1;
        tile.begin(p, t, v, n1);
        for (int32_t p0 = 0; p0 < Tile::row_len(p); p0 += Tile::CHUNK) {
            const int32_t cw = Tile::width(p, p0);
            for (int32_t k = 0; k < cw; k++) {
                int64_t eid = -1;
                if (p0 + k > 0) v = walk_step<WEIGHTED, RESTART>(p, v, n1++, eid);      // position 0 is the seed, copied as given
                tile.stage(k, v, eid);
            }
            tile.flush(p, p0, cw);
        }
    }
}

template <bool WEIGHTED, bool RESTART>
static void launch_walk(hipStream_t s, const WalkParams& p)
{
    if (p.edge_ids != nullptr) random_walk_kernel<WEIGHTED, RESTART, true><<<walk_grid(p.num_walks), LG_WALK_THREADS, 0, s>>>(p);
    else random_walk_kernel<WEIGHTED, RESTART, false><<<walk_grid(p.num_walks), LG_WALK_THREADS, 0, s>>>(p);
}

// the arguments are the caller's to check (legion_random_walk): this only picks the instance
void launch_random_walk(hipStream_t s, const WalkParams& p)
{
    if (p.num_walks <= 0) return;
    const bool weighted = p.edge_cdf != nullptr, restart = p.restart_prob > 0.0f;
    if (weighted) { if (restart) launch_walk<true, true>(s, p); else launch_walk<true, false>(s, p); }
    else          { if (restart) launch_walk<false, true>(s, p); else launch_walk<false, false>(s, p); }
    hipCheckError();
}

}  // namespace lg
