// kept_slots.h -- the stable compaction of the slots of a row expansion (row_slots.h) that a predicate keeps, once: what
// kernels_labor.hip and kernels_induced.hip share.  An op brings a struct derived from LaneSlots that holds the predicate's results as
// members (apart from the slots they cost labor_count_kernel 1.1 -- 1.3 % on hub rows: DESIGN.md 4.19) and says
//     void resolve(const Params& p, int64_t tile, int64_t* s_off)      the tile's slots (resolve_row_slots: one barrier) and the predicate
//     bool kept(int32_t j) const                                       is the lane's slot of strip j kept?
//     int32_t source(int32_t j) const                                  what goes to src for it
// and a Params whose member `kept` is the KeptParams (legion_core.h) and whose member `slots` the RowSlots.  The passes:
//   * count    a tile of 1 024 slots resolves and sums its kept slots by ballot / popcount and four wave totals through LDS: one int64
//              per tile; then launch_scan_int64 (kernels_in_edges.hip) turns the counts into exclusive prefix sums, the total K going
//              to the scratch and to count;
//   * write    resolves and evaluates again (cheaper than storing and re-reading 12 -- 20 bytes a slot).  The rank of a kept slot inside
//              its tile is stable: strip j (256 consecutive slots) before strip j + 1, lane order inside a strip: a ballot and mbcnt per
//              strip, sixteen wave counts in LDS, one barrier.  A triple goes to base + rank when that lies in [0, cap), whatever the
//              scratch holds.  A tile whose prefix sum equals the next one's keeps nothing and is not resolved at all (resolving every
//              tile was 2 -- 3 x slower on hub rows: DESIGN.md 4.18).  Then the same grid strides over [K, cap) with -1, K clamped to
//              [0, cap].
// Device code and its launches; include inside namespace lg's files after legion_core.h.
#pragma once

#include "legion_core.h"
#include "kept_rule.h"
#include "row_slots.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_ROW_TILE == 1024 && kept_tiles(LG_ROW_TILE + 1) == 2, "kept_rule.h counts the scratch in tiles of 1 024 slots");
static_assert(kept_groups(256 * LG_ROW_TILE + 1) == 2, "launch_scan_int64 sums per 256 tiles, as kept_rule.h counts the scratch");

// the body of a count kernel: tiles[tile] = the tile's kept slots
template <class Slots, class Params>
__device__ __forceinline__ void kept_count_tiles(const Params& p)
{
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_wave[LG_ROW_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < p.kept.n_tiles; tile += gridDim.x) {
        Slots o;
        o.resolve(p, tile, s_off);
        int32_t kept = 0;
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) kept += __popcll(__ballot(o.kept(j)));
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
        __syncthreads();                                              // (and: the next tile stages over s_off)
        if (threadIdx.x == 0) p.kept.tiles[tile] = (int64_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        // the next write of s_wave lies behind the next tile's staging barrier
    }
}

// the body of a write kernel: the kept slots' triples at their ranks, then [K, cap): -1 / -1 / -1
template <class Slots, class Params>
__device__ __forceinline__ void kept_write_tiles(const Params& p)
{
    constexpr int32_t ILP = LG_ROW_ILP, WAVES = LG_ROW_THREADS / 64;
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_cnt[ILP * WAVES];                            // [strip][wave]: the order of the ranks
    const KeptParams& k = p.kept;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < k.n_tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)k.tiles[tile];                // (whatever it holds: the stores below are guarded)
        if ((uint64_t)k.tiles[tile + 1] == base) continue;            // the tile keeps nothing ([n_tiles] is the total): the whole workgroup skips it
        Slots o;
        o.resolve(p, tile, s_off);
        int32_t below[ILP];                                           // kept slots of the strip in lower lanes of this wave
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const unsigned long long b = __ballot(o.kept(j));
            below[j] = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (lane == 0) s_cnt[j * WAVES + wave] = __popcll(b);
        }
        __syncthreads();                                              // (and: the next tile stages over s_off)
        int32_t run = 0, before[ILP];
#pragma unroll
        for (int32_t c = 0; c < ILP * WAVES; c++) {
            if ((c & (WAVES - 1)) == wave) before[c / WAVES] = run;
            run += s_cnt[c];
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const uint64_t at = base + (uint64_t)(before[j] + below[j]);
            if (o.kept(j) && at < (uint64_t)k.cap) {
                k.dst[at] = o.i[j];
                k.src[at] = o.source(j);
                if (k.eid) k.eid[at] = o.e[j];
            }
        }
        // the next write of s_cnt lies behind the next tile's staging barrier
    }
    const int64_t total = k.tiles[k.n_tiles];
    const int64_t first = total < 0 ? 0 : total > k.cap ? k.cap : total;
    for (int64_t at = first + (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; at < k.cap; at += (int64_t)gridDim.x * LG_ROW_THREADS) {
        k.dst[at] = -1;
        k.src[at] = -1;
        if (k.eid) k.eid[at] = -1;
    }
}

// the count pass; the arguments are the caller's to check
template <class Params>
void launch_kept_count(hipStream_t s, void (*kernel)(Params), const Params& p)
{
    const KeptParams& k = p.kept;
    if (k.n_tiles > 0) kernel<<<walk_grid(k.n_tiles * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);
    // tiles[0 .. n_tiles) becomes its exclusive prefix sums, tiles[n_tiles] and count[0] the total (m == 0: both totals 0, only)
    launch_scan_int64(s, k.tiles, (int32_t)k.n_tiles, k.tiles + k.n_tiles + 1, (int32_t)k.n_groups, false, k.tiles + k.n_tiles, k.count);
}

// the write pass: a workgroup per tile, of slots or of the fill; the arguments are the caller's to check
template <class Params>
void launch_kept_write(hipStream_t s, void (*kernel)(Params), const Params& p)
{
    const KeptParams& k = p.kept;
    if (k.cap <= 0) return;
    const int64_t fill = (k.cap + LG_ROW_TILE - 1) / LG_ROW_TILE;
    kernel<<<walk_grid((k.n_tiles > fill ? k.n_tiles : fill) * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);
    hipCheckError();
}

}  // namespace lg
