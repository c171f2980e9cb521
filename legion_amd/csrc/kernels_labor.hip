// kernels_labor.hip -- layer-neighbour sampling (LABOR-0 of Balin and Catalyurek; DGL's dgl.sampling.sample_labors) for gfx950 (CDNA4,
// wave64): in_edges' expansion of rows over slots (row_slots.h) with a predicate and a stable compaction.  Every source vertex has ONE
// random number, a hash of (src, salt); the entry src -> dst is kept iff that number lies below fanout / deg(dst), in integers
// (labor_rule.h, whose text runs here on the device).  The rules are the contracts in include/legion_hip.h.
// The layout is in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles of 1 024 consecutive
// slots, four per lane, 256 apart; every offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * count    a tile resolves its slots (row_slots.h), evaluates the predicate and sums the kept slots by ballot / popcount and four
//              wave totals through LDS: one int64 per tile;
//   * scan     the three int64 launches of kernels_in_edges.hip (launch_scan_int64) over the tiles' counts: the sum per 256 tiles, ONE
//              workgroup's exclusive prefix sums of the at most 4 096 sums (the total K goes to the scratch and to count_out), and the
//              in-group exclusive scan plus its base;
//   * write    resolves the tile and evaluates the predicate again (reading col twice is cheaper than writing and re-reading 12 -- 20
//              bytes a slot).  The rank of a kept slot inside its tile is stable: strip j (256 consecutive slots) before strip j + 1,
//              lane order inside a strip: a ballot and mbcnt per strip, sixteen wave counts in LDS, one barrier.  A triple goes to
//              base + rank when that lies in [0, cap), whatever the scratch holds.  Then the same grid strides over [K, cap) with -1,
//              K clamped to [0, cap].  A tile whose prefix sum equals the next one's keeps nothing and is not resolved at all.
// Bound: the col reads and, for rows of a degree near the fan-out, the stores; no MFMA.
#include "legion_core.h"
#include "labor_rule.h"
#include "row_slots.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_ROW_TILE == 1024 && labor_tiles(LG_ROW_TILE + 1) == 2, "labor_rule.h counts the scratch in tiles of 1 024 slots");
static_assert(labor_groups(256 * LG_ROW_TILE + 1) == 2, "launch_scan_int64 sums per 256 tiles, as labor_rule.h counts the scratch");

// a lane's four slots and rule 3 for them
struct LaborSlots : LaneSlots {
    bool keep[LG_ROW_ILP];
};

// Rules 1 -- 3 for the slots of a tile: the resolution, then the predicate: the degree is the row's whole one, a dead entry is never
// kept.  One barrier inside, resolve_row_slots'
__device__ __forceinline__ void labor_resolve(const LaborParams& p, int64_t tile, int64_t* s_off, LaborSlots& o)
{
    resolve_row_slots(p.slots, tile, s_off, o);
#pragma unroll
    for (int32_t j = 0; j < LG_ROW_ILP; j++)
        o.keep[j] = o.e[j] >= 0 && o.src[j] >= 0 && labor_keep(labor_hash_keyed(p.key, o.src[j]), o.d[j], p.fanout);
}

// ------------------------------------------------------------------------------------------
// count
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS, 8) void labor_count_kernel(LaborParams p)
{
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_wave[LG_ROW_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        LaborSlots o;
        labor_resolve(p, tile, s_off, o);
        int32_t kept = 0;
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) kept += __popcll(__ballot(o.keep[j]));
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
        __syncthreads();                                              // (and: the next tile stages over s_off)
        if (threadIdx.x == 0) p.tiles[tile] = (int64_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        // the next write of s_wave lies behind the next tile's staging barrier
    }
}

// the arguments are the caller's to check (legion_labor_count)
void launch_labor_count(hipStream_t s, const LaborParams& p)
{
    if (p.n_tiles > 0) labor_count_kernel<<<walk_grid(p.n_tiles * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);
    // tiles[0 .. n_tiles) becomes its exclusive prefix sums, tiles[n_tiles] and count[0] the total (m == 0: both totals 0, only)
    launch_scan_int64(s, p.tiles, (int32_t)p.n_tiles, p.tiles + p.n_tiles + 1, (int32_t)p.n_groups, false, p.tiles + p.n_tiles, p.count);
}

// ------------------------------------------------------------------------------------------
// write
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS, 8) void labor_edges_kernel(LaborParams p)
{
    constexpr int32_t ILP = LG_ROW_ILP, WAVES = LG_ROW_THREADS / 64;
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_cnt[ILP * WAVES];                            // [strip][wave]: the order of the ranks
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)p.tiles[tile];                // (whatever it holds: the stores below are guarded)
        if ((uint64_t)p.tiles[tile + 1] == base) continue;            // the tile keeps nothing ([n_tiles] is the total): the whole workgroup
                                                                      // skips it.  Resolving every tile was 2 -- 3 x slower on hub rows
        LaborSlots o;
        labor_resolve(p, tile, s_off, o);
        int32_t below[ILP];                                           // kept slots of the strip in lower lanes of this wave
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const unsigned long long b = __ballot(o.keep[j]);
            below[j] = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (lane == 0) s_cnt[j * WAVES + wave] = __popcll(b);
        }
        __syncthreads();                                              // (and: the next tile stages over s_off)
        int32_t run = 0, before[ILP];
#pragma unroll
        for (int32_t k = 0; k < ILP * WAVES; k++) {
            if ((k & (WAVES - 1)) == wave) before[k / WAVES] = run;
            run += s_cnt[k];
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const uint64_t at = base + (uint64_t)(before[j] + below[j]);
            if (o.keep[j] && at < (uint64_t)p.cap) {
                p.dst[at] = o.i[j];
                p.src[at] = o.src[j];
                if (p.eid) p.eid[at] = o.e[j];
            }
        }
        // the next write of s_cnt lies behind the next tile's staging barrier
    }
    // [K, cap): -1 / -1 / -1
    const int64_t total = p.tiles[p.n_tiles];
    const int64_t first = total < 0 ? 0 : total > p.cap ? p.cap : total;
    for (int64_t at = first + (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; at < p.cap; at += (int64_t)gridDim.x * LG_ROW_THREADS) {
        p.dst[at] = -1;
        p.src[at] = -1;
        if (p.eid) p.eid[at] = -1;
    }
}

// the arguments are the caller's to check (legion_labor_edges)
void launch_labor_edges(hipStream_t s, const LaborParams& p)
{
    if (p.cap <= 0) return;
    const int64_t tiles = p.n_tiles > (p.cap + LG_ROW_TILE - 1) / LG_ROW_TILE ? p.n_tiles : (p.cap + LG_ROW_TILE - 1) / LG_ROW_TILE;
    labor_edges_kernel<<<walk_grid(tiles * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);      // a workgroup per tile, of slots or of the fill
    hipCheckError();
}

}  // namespace lg
