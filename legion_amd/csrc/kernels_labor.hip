// kernels_labor.hip -- layer-neighbour sampling (LABOR-0 of Balin and Catalyurek; DGL's dgl.sampling.sample_labors) for gfx950 (CDNA4,
// wave64): the expansion of kernels_in_edges.hip with a predicate and a stable compaction.  Every source vertex has ONE random number,
// a hash of (src, salt); the entry src -> dst is kept iff that number lies below fanout / deg(dst), in integers (labor_rule.h, whose
// text runs here on the device).  The rules are the contracts in include/legion_hip.h.
// The layout is in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles of 1 024 consecutive
// slots, four per lane, 256 apart; every offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * count    a tile resolves its slots as in_edges_kernel does (the tile's range of offsets from two interleaved upper-bound searches,
//              staged in LDS when it has at most 1 025 entries, else searched in global memory), loads col[e], evaluates the predicate
//              and sums the kept slots by ballot / popcount and four wave totals through LDS: one int64 per tile;
//   * scan     three launches over int64, row_offsets' way: the sum per 256 tiles, ONE workgroup's exclusive prefix sums of the at most
//              4 096 sums (the total K goes to the scratch and to count_out), and the in-group exclusive scan plus its base;
//   * write    resolves the tile and evaluates the predicate again (reading col twice is cheaper than writing and re-reading 12 -- 20
//              bytes a slot).  The rank of a kept slot inside its tile is stable: strip j (256 consecutive slots) before strip j + 1,
//              lane order inside a strip: a ballot and mbcnt per strip, sixteen wave counts in LDS, one barrier.  A triple goes to
//              base + rank when that lies in [0, cap), whatever the scratch holds.  Then the same grid strides over [K, cap) with -1,
//              K clamped to [0, cap].  A tile whose prefix sum equals the next one's keeps nothing and is not resolved at all.
// Bound: the col reads and, for rows of a degree near the fan-out, the stores; no MFMA.
#include "legion_core.h"
#include "labor_rule.h"
#include "upper_counts.h"
#include "walk_step.h"

namespace lg {

#define LG_LABOR_THREADS 256
#define LG_LABOR_ILP 4                                        // slots per lane, 256 apart
#define LG_LABOR_TILE (LG_LABOR_THREADS * LG_LABOR_ILP)
#define LG_LABOR_STAGE (LG_LABOR_TILE + 1)                    // a tile's non-empty rows and the closing offset
#define LG_LABOR_GROUP 256                                    // tiles per second-level sum

static_assert(LG_LABOR_THREADS == LG_WALK_THREADS, "the grids below are walk_grid's: a tile of 256 outputs, the walks' cap");
static_assert(LG_LABOR_TILE == 1024 && labor_tiles(LG_LABOR_TILE + 1) == 2, "labor_rule.h counts the scratch in tiles of 1 024 slots");

// what a lane knows of its four slots of a tile
struct LaborSlots {
    int64_t q[LG_LABOR_ILP];        // the slot
    int64_t e[LG_LABOR_ILP];        // its entry of col, -1: none
    int32_t i[LG_LABOR_ILP];        // its index into rows
    int32_t src[LG_LABOR_ILP];      // col[e]
    bool keep[LG_LABOR_ILP];        // rule 3
};

// Rules 1 -- 3 for the slots of a tile: in_edges_kernel's resolution, the degree from the pair loaded once, the predicate.  One barrier
// inside (every lane of the workgroup calls it); the caller puts another between its last read of what follows and the next call.
__device__ __forceinline__ void labor_resolve(const LaborParams& p, int64_t tile, int64_t* s_off, LaborSlots& o)
{
    constexpr int32_t ILP = LG_LABOR_ILP;
    const int32_t n1 = p.n + 1;                                       // offsets' entries
    const int64_t p0 = tile * LG_LABOR_TILE;
    // the row indices the tile touches: a = the first (its upper bound - 1, at least 0), b = the last's closing offset (at most n)
    const int64_t ends[2] = {p0, min(p0 + LG_LABOR_TILE - 1, p.m - 1)};
    const bool both[2] = {true, true};
    int32_t ub[2];
    upper_counts<2>(p.offsets, n1, ends, both, ub);
    const int32_t a = max(ub[0] - 1, 0), b = min(ub[1], p.n);
    const int32_t cnt = max(b - a + 1, 0);                            // offsets[a .. b]: inside offsets[0 .. n]
    const bool staged = cnt <= LG_LABOR_STAGE;
    if (staged)
        for (int32_t k = threadIdx.x; k < cnt; k += LG_LABOR_THREADS) s_off[k] = p.offsets[a + k];
    __syncthreads();
    bool live[ILP];
    int32_t c[ILP];
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) {
        o.q[j] = p0 + threadIdx.x + (int64_t)j * LG_LABOR_THREADS;
        live[j] = o.q[j] < p.m;
    }
    if (staged) upper_counts<ILP>(s_off, cnt, o.q, live, c);
    else upper_counts<ILP>(p.offsets + a, cnt, o.q, live, c);
    // slot q[j] lies in the row of index i = a + c - 1 (c == 0: before the range, no row), at position jj of it
    int32_t r[ILP];
    int64_t jj[ILP], d[ILP];
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) {
        o.i[j] = c[j] > 0 ? a + c[j] - 1 : -1;
        if (o.i[j] >= p.n) o.i[j] = -1;                               // past offsets[n]: no row
        const int64_t opens = o.i[j] < 0 ? 0 : staged ? s_off[c[j] - 1] : p.offsets[o.i[j]];      // offsets[i]
        jj[j] = o.i[j] >= 0 ? (int64_t)((uint64_t)o.q[j] - (uint64_t)opens) : -1;
    }
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) r[j] = o.i[j] >= 0 ? p.rows[o.i[j]] : -1;
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) {
        o.e[j] = -1;
        d[j] = 0;
        if ((uint32_t)r[j] < (uint32_t)p.node_num) {                  // else: no memory is read for r
            const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + r[j]);      // (r + 1 <= node_num: inside indptr)
            d[j] = row.e - row.s;                                     // the row's whole degree, dead entries and slots past m included
            if (jj[j] >= 0 && jj[j] < d[j]) o.e[j] = row.s + jj[j];   // s <= e < indptr[r + 1] <= E
        }
    }
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) o.src[j] = o.e[j] >= 0 ? p.col[o.e[j]] : -1;      // a dead entry stays -1
#pragma unroll
    for (int32_t j = 0; j < ILP; j++)
        o.keep[j] = o.e[j] >= 0 && o.src[j] >= 0 && labor_keep(labor_hash_keyed(p.key, o.src[j]), d[j], p.fanout);
}

// ------------------------------------------------------------------------------------------
// count
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_LABOR_THREADS, 8) void labor_count_kernel(LaborParams p)
{
    __shared__ int64_t s_off[LG_LABOR_STAGE];
    __shared__ int32_t s_wave[LG_LABOR_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        LaborSlots o;
        labor_resolve(p, tile, s_off, o);
        int32_t kept = 0;
#pragma unroll
        for (int32_t j = 0; j < LG_LABOR_ILP; j++) kept += __popcll(__ballot(o.keep[j]));
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
        __syncthreads();                                              // (and: the next tile stages over s_off)
        if (threadIdx.x == 0) p.tiles[tile] = (int64_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        // the next write of s_wave lies behind the next tile's staging barrier
    }
}

// ------------------------------------------------------------------------------------------
// scan: tiles[0 .. n_tiles) becomes its exclusive prefix sums, tiles[n_tiles] and count[0] the total (kernels_in_edges.hip's three
// launches over int64, the first of them over counts it reads instead of degrees)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_LABOR_THREADS) void labor_group_kernel(const int64_t* tiles, int32_t n_tiles, int32_t n_groups, int64_t* groups)
{
    __shared__ int64_t s_wave[LG_LABOR_THREADS / 64];
    for (int32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int32_t t = g * LG_LABOR_GROUP + (int32_t)threadIdx.x;
        int64_t v = t < n_tiles ? tiles[t] : 0;
        for (int32_t off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) groups[g] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
}

// one workgroup: groups[] becomes its exclusive prefix sums; the total to total[0] and count[0]
__global__ __launch_bounds__(LG_LABOR_THREADS) void labor_scan_kernel(int64_t* groups, int32_t n_groups, int64_t* total, int64_t* count)
{
    __shared__ int64_t s_wave[LG_LABOR_THREADS / 64];
    const int32_t per = (n_groups + LG_LABOR_THREADS - 1) / LG_LABOR_THREADS;      // a thread's run of consecutive sums
    const int32_t t0 = min((int32_t)threadIdx.x * per, n_groups), t1 = min(t0 + per, n_groups);
    int64_t sum = 0;
    for (int32_t t = t0; t < t1; t++) sum += groups[t];
    int64_t inc = sum;                                                // inclusive over the wave
    const int32_t lane = threadIdx.x & 63;
    for (int32_t off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    int64_t before = inc - sum;
    for (int32_t w = 0; w < (int32_t)(threadIdx.x >> 6); w++) before += s_wave[w];
    for (int32_t t = t0; t < t1; t++) {
        const int64_t c = groups[t];
        groups[t] = before;
        before += c;
    }
    if (threadIdx.x == LG_LABOR_THREADS - 1) {                        // (the last thread's run ends the array, or is empty behind it)
        total[0] = before;
        count[0] = before;
    }
}

__global__ __launch_bounds__(LG_LABOR_THREADS) void labor_apply_kernel(int32_t n_tiles, int32_t n_groups, int64_t* tiles, const int64_t* groups)
{
    __shared__ int64_t s_wave[LG_LABOR_THREADS / 64];
    for (int32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int32_t t = g * LG_LABOR_GROUP + (int32_t)threadIdx.x;
        const int64_t c = t < n_tiles ? tiles[t] : 0;
        int64_t inc = c;                                              // inclusive over the wave
        const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int32_t off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(inc, off, 64);
            if (lane >= off) inc += y;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int64_t before = groups[g] + inc - c;
        for (int32_t w = 0; w < wave; w++) before += s_wave[w];
        if (t < n_tiles) tiles[t] = before;
        __syncthreads();
    }
}

// the arguments are the caller's to check (legion_labor_count)
void launch_labor_count(hipStream_t s, const LaborParams& p)
{
    int64_t* groups = p.tiles + p.n_tiles + 1;
    const int32_t n_tiles = (int32_t)p.n_tiles, n_groups = (int32_t)p.n_groups;
    if (n_tiles > 0) {
        labor_count_kernel<<<walk_grid(p.n_tiles * LG_LABOR_THREADS), LG_LABOR_THREADS, 0, s>>>(p);
        labor_group_kernel<<<walk_grid(p.n_tiles), LG_LABOR_THREADS, 0, s>>>(p.tiles, n_tiles, n_groups, groups);
    }
    labor_scan_kernel<<<1, LG_LABOR_THREADS, 0, s>>>(groups, n_groups, p.tiles + p.n_tiles, p.count);      // (m == 0: both totals 0, only)
    if (n_tiles > 0) labor_apply_kernel<<<walk_grid(p.n_tiles), LG_LABOR_THREADS, 0, s>>>(n_tiles, n_groups, p.tiles, groups);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// write
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_LABOR_THREADS, 8) void labor_edges_kernel(LaborParams p)
{
    constexpr int32_t ILP = LG_LABOR_ILP, WAVES = LG_LABOR_THREADS / 64;
    __shared__ int64_t s_off[LG_LABOR_STAGE];
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
    for (int64_t at = first + (int64_t)blockIdx.x * LG_LABOR_THREADS + threadIdx.x; at < p.cap; at += (int64_t)gridDim.x * LG_LABOR_THREADS) {
        p.dst[at] = -1;
        p.src[at] = -1;
        if (p.eid) p.eid[at] = -1;
    }
}

// the arguments are the caller's to check (legion_labor_edges)
void launch_labor_edges(hipStream_t s, const LaborParams& p)
{
    if (p.cap <= 0) return;
    const int64_t tiles = p.n_tiles > (p.cap + LG_LABOR_TILE - 1) / LG_LABOR_TILE ? p.n_tiles : (p.cap + LG_LABOR_TILE - 1) / LG_LABOR_TILE;
    labor_edges_kernel<<<walk_grid(tiles * LG_LABOR_THREADS), LG_LABOR_THREADS, 0, s>>>(p);      // a workgroup per tile, of slots or of the fill
    hipCheckError();
}

}  // namespace lg
