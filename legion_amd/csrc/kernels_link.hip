// kernels_link.hip -- the seeds of a link-prediction batch for gfx950 (CDNA4, wave64): the endpoints of seed edges (DGL's
// g.find_edges), uniform negatives that are no neighbours (negative_sampler.Uniform / PyG's structured_negative_sampling) and the list
// of distinct ids with local indices, in order of first appearance (compact_graphs' relabelling).
//
// The rules are the contracts in include/legion_hip.h (legion_find_edges, legion_negative_sample, legion_unique_ids).  The layout:
//   * find_edges, negative_sample: one lane per output (find_edges: per four), 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over
//     tiles (the walks' cap, walk_step.h); consecutive lanes write consecutive outputs.  Every offset into indptr and col is 64
//     bits wide.  negative_sample is a flat loop over tries with the two exclusions as template flags: the instance without either
//     loads nothing but rows, the row pair {s, e} of the edge exclusion is loaded once per slot, and try t + 1 is try t times the
//     constant 48271^(2^23) -- node2vec's stepping and row search (kPow23, row_has: walk_step.h): one table look-up per slot;
//   * find_edges: a lane searches for four edge ids at once, 256 apart, their chains of dependent loads interleaved -- the op is bound
//     by latency times loads in flight.  Measured against one and two ids per lane and against the top eight levels of the search
//     staged in LDS, which gained nothing beside it and is not built;
//   * unique_ids: six launches (the first clears the table) over the id table of node_set.h in the caller's scratch, none of which waits for another workgroup:
//       insert   a lane claims its id's slot by a 32-bit compare-and-swap on the key (linear probing from the home slot, at most `slots`
//                probes: the table has at least 2 m slots, so a free one exists) and takes atomicMin of its index on the slot's first
//                index -- whichever lane claims, the minimum is the first appearance.  The slot is remembered per id;
//       count    first touches (first[slot[i]] == i) per tile of 256 ids;
//       scan     ONE workgroup: the exclusive prefix sums of the tile counts in place, and the total to count_out (tile_scan.h);
//       apply    a tile ranks its first touches (ballot prefix inside a wave, four wave totals through LDS), writes unique[rank]
//                and remembers the rank at the first index;
//       scatter  local[i] = the rank remembered at first[slot[i]]; unique[U .. m) = -1.
//     Which slot a key lands in depends on arrival order; no output does.
// Bound: find_edges and the edge exclusion by the part's rate of dependent random requests; unique_ids by its atomics; no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "node_set.h"
#include "tile_scan.h"
#include "walk_step.h"

namespace lg {

#define LG_LINK_THREADS 256
#define LG_FIND_EDGES_ILP 4      // edge ids per lane, searched for at once (1, 2 and 4 measured: DESIGN.md 4.14)

static_assert(LG_LINK_THREADS == LG_WALK_THREADS, "the grids below are walk_grid's: a tile of 256 outputs, the walks' cap");
static_assert(LG_LINK_THREADS == LG_SCAN_THREADS, "unique_scan_kernel is tile_scan.h's workgroup");

// a tile is 256 x ILP edge ids; a lane's ILP ids lie 256 apart, so consecutive lanes read and write consecutive entries
__global__ __launch_bounds__(LG_LINK_THREADS, 8) void find_edges_kernel(const int64_t* indptr, const int32_t* col, int32_t node_num,
                                                                        int64_t num_edges, const int64_t* eids, int32_t n, int32_t* row_out,
                                                                        int32_t* col_out)
{
    constexpr int32_t ILP = LG_FIND_EDGES_ILP;
    const int64_t rows1 = (int64_t)node_num + 1;                      // indptr's entries
    constexpr int64_t TILE = (int64_t)LG_LINK_THREADS * ILP;
    for (int64_t i0 = (int64_t)blockIdx.x * TILE + threadIdx.x; i0 < n; i0 += (int64_t)gridDim.x * TILE) {
        int64_t e[ILP], lo[ILP], len[ILP];
        int32_t c[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const int64_t i = i0 + (int64_t)j * LG_LINK_THREADS;
            e[j] = i < n ? eids[i] : -1;
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) c[j] = e[j] >= 0 && e[j] < num_edges ? col[e[j]] : -1;      // else: no memory is read for e
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {                           // the range of indptr to count in: [lo, lo + len); none for a dead entry
            lo[j] = 0;
            len[j] = c[j] >= 0 ? rows1 : 0;
        }
        bool more = true;
        while (more) {                                                // upper bound: lo ends at #{ v in [0, N] : indptr[v] <= e }
            more = false;
            int64_t v[ILP];
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) v[j] = indptr[len[j] > 0 ? lo[j] + (len[j] >> 1) : 0];      // (lo + len / 2 < lo + len <= rows1)
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) {
                if (len[j] > 0) {
                    const int64_t half = len[j] >> 1;
                    if (v[j] <= e[j]) { lo[j] += half + 1; len[j] -= half + 1; }
                    else len[j] = half;
                    more |= len[j] > 0;
                }
            }
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const int64_t i = i0 + (int64_t)j * LG_LINK_THREADS;
            if (i < n) {                                              // indptr[0] = 0 <= e < E = indptr[N]: the count lies in [1, N]
                row_out[i] = c[j] >= 0 ? (int32_t)(lo[j] - 1) : -1;
                col_out[i] = c[j] >= 0 ? c[j] : -1;                   // a dead entry: both -1
            }
        }
    }
}

void launch_find_edges(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t node_num, int64_t num_edges, const int64_t* eids,
                       int32_t n, int32_t* row_out, int32_t* col_out)
{
    if (n <= 0) return;
    const dim3 grid = walk_grid(((int64_t)n + LG_FIND_EDGES_ILP - 1) / LG_FIND_EDGES_ILP);
    find_edges_kernel<<<grid, LG_LINK_THREADS, 0, s>>>(indptr, col, node_num, num_edges, eids, n, row_out, col_out);
    hipCheckError();
}

template <bool SELF, bool EDGES>
__global__ __launch_bounds__(LG_LINK_THREADS, 8) void negative_sample_kernel(NegativeParams p)
{
    const int64_t total = (int64_t)p.n * p.k;                         // <= 2^31 - 1 (negative_sample_refusal)
    for (int64_t m = (int64_t)blockIdx.x * LG_LINK_THREADS + threadIdx.x; m < total; m += (int64_t)gridDim.x * LG_LINK_THREADS) {
        const int32_t r = p.rows[m / p.k];
        int32_t out = -1;
        if ((uint32_t)r < (uint32_t)p.node_num) {                     // else: no memory is read for r
            int64_t s = 0;
            int32_t D = 0;
            if (EDGES) {                                              // the row, once per slot
                const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + r);      // (r + 1 <= node_num: inside indptr)
                s = row.s;
                D = (int32_t)(row.e - s);
            }
            uint32_t x = minstd_pow((uint32_t)(p.base + m) + 1u);
            for (int32_t t = 0; t < p.max_tries; t++) {
                const int32_t u = draw_from_x(x, p.node_num);         // r01 < 1: u <= node_num - 1
                const bool reject = (SELF && u == r) || (EDGES && row_has(p.col + s, D, u));      // (s + D <= E: probes inside col)
                if (!reject) { out = u; break; }
                x = mulmod31(x, kPow23);
            }
        }
        p.neg[m] = out;
    }
}

// the arguments are the caller's to check (legion_negative_sample): this only picks the instance
void launch_negative_sample(hipStream_t s, const NegativeParams& p)
{
    const int64_t total = (int64_t)p.n * p.k;
    if (total <= 0) return;
    const dim3 grid = walk_grid(total);
    switch (p.exclude & 3) {
    case 0: negative_sample_kernel<false, false><<<grid, LG_LINK_THREADS, 0, s>>>(p); break;
    case 1: negative_sample_kernel<true, false><<<grid, LG_LINK_THREADS, 0, s>>>(p); break;
    case 2: negative_sample_kernel<false, true><<<grid, LG_LINK_THREADS, 0, s>>>(p); break;
    default: negative_sample_kernel<true, true><<<grid, LG_LINK_THREADS, 0, s>>>(p); break;
    }
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// unique_ids.  Scratch (link_rule.h: unique_ids_scratch_bytes), int32 each: the id table [2 x slots] (node_set.h), slot[m], rank_at[m],
// tiles[T].  The call clears the table.
// ------------------------------------------------------------------------------------------
struct UniquePlan {
    const int32_t* ids;
    int32_t* unique;
    int32_t* local;
    int32_t* count;
    int32_t* keys;
    uint32_t* first;
    int32_t* slot;
    int32_t* rank_at;
    int32_t* tiles;
    int32_t m;
    int32_t n_tiles;
    uint32_t mask;               // slots - 1
    int32_t shift;               // 32 - log2(slots)
};

__global__ __launch_bounds__(LG_LINK_THREADS) void unique_clear_kernel(uint32_t* table, int64_t words)
{
    id_table_clear(table, words, nullptr);
}

__global__ __launch_bounds__(LG_LINK_THREADS) void unique_insert_kernel(UniquePlan p)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_LINK_THREADS + threadIdx.x; i < p.m; i += (int64_t)gridDim.x * LG_LINK_THREADS) {
        const int32_t id = p.ids[i];
        int32_t at = -1;
        if (id >= 0) {
            uint32_t h = id_table_home(id, p.shift);
            for (uint32_t probe = 0; probe <= p.mask; probe++) {      // at most `slots` probes; a free slot exists (slots >= 2 m)
                const int32_t old = atomicCAS(p.keys + h, ID_TABLE_EMPTY_KEY, id);
                if (old == ID_TABLE_EMPTY_KEY || old == id) { at = (int32_t)h; break; }
                h = (h + 1u) & p.mask;
            }
            if (at >= 0) atomicMin(p.first + at, (uint32_t)i);
        }
        p.slot[i] = at;
    }
}

// is entry i the first appearance of its id?
__device__ __forceinline__ bool unique_first_touch(const UniquePlan& p, int64_t i)
{
    if (i >= p.m) return false;
    const int32_t at = p.slot[i];
    return at >= 0 && p.first[at] == (uint32_t)i;
}

__global__ __launch_bounds__(LG_LINK_THREADS) void unique_count_kernel(UniquePlan p)
{
    __shared__ int32_t s_wave[LG_LINK_THREADS / 64];
    for (int32_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const bool flag = unique_first_touch(p, (int64_t)tile * LG_LINK_THREADS + threadIdx.x);
        const unsigned long long b = __ballot(flag);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) p.tiles[tile] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
}

// one workgroup: tiles[] becomes its exclusive prefix sums, count[0] the total
__global__ __launch_bounds__(LG_LINK_THREADS) void unique_scan_kernel(UniquePlan p)
{
    __shared__ int32_t s_wave[LG_SCAN_WAVES];
    tile_scan_in_place<int32_t>(p.tiles, p.n_tiles, p.count, nullptr, s_wave);
}

__global__ __launch_bounds__(LG_LINK_THREADS) void unique_apply_kernel(UniquePlan p)
{
    __shared__ int32_t s_wave[LG_LINK_THREADS / 64];
    for (int32_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t i = (int64_t)tile * LG_LINK_THREADS + threadIdx.x;
        const bool flag = unique_first_touch(p, i);
        const unsigned long long b = __ballot(flag);
        const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        if (flag) {
            int32_t rank = p.tiles[tile] + __popcll(b & ((1ull << lane) - 1ull));
            for (int32_t w = 0; w < wave; w++) rank += s_wave[w];
            p.unique[rank] = p.ids[i];                                // rank < U <= m
            p.rank_at[i] = rank;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LG_LINK_THREADS) void unique_scatter_kernel(UniquePlan p)
{
    const int32_t U = p.count[0];
    for (int64_t i = (int64_t)blockIdx.x * LG_LINK_THREADS + threadIdx.x; i < p.m; i += (int64_t)gridDim.x * LG_LINK_THREADS) {
        const int32_t at = p.slot[i];
        p.local[i] = at >= 0 ? p.rank_at[p.first[at]] : -1;         // first[at] <= i < m: a first touch, whose rank apply has written
        if (i >= U) p.unique[i] = -1;
    }
}

// the arguments are the caller's to check (legion_unique_ids); scratch holds unique_ids_scratch_bytes(m) bytes
void launch_unique_ids(hipStream_t s, const int32_t* ids, int32_t m, int32_t* unique, int32_t* local, int32_t* count, void* scratch,
                       int64_t slots, int64_t n_tiles)
{
    UniquePlan p;
    p.ids = ids;
    p.unique = unique;
    p.local = local;
    p.count = count;
    const IdTable t = id_table_carve(scratch, slots);
    p.keys = t.keys;
    p.first = t.first;
    p.mask = t.mask;
    p.shift = t.shift;
    p.slot = p.keys + 2 * slots;
    p.rank_at = p.slot + m;
    p.tiles = p.rank_at + m;
    p.m = m;
    p.n_tiles = (int32_t)n_tiles;
    if (m > 0) {
        const dim3 grid = walk_grid(m);
        unique_clear_kernel<<<walk_grid(2 * slots), LG_LINK_THREADS, 0, s>>>(reinterpret_cast<uint32_t*>(p.keys), 2 * slots);
        unique_insert_kernel<<<grid, LG_LINK_THREADS, 0, s>>>(p);
        unique_count_kernel<<<grid, LG_LINK_THREADS, 0, s>>>(p);
    }
    unique_scan_kernel<<<1, LG_LINK_THREADS, 0, s>>>(p);              // (m == 0: no tiles, count = 0)
    if (m > 0) {
        const dim3 grid = walk_grid(m);
        unique_apply_kernel<<<grid, LG_LINK_THREADS, 0, s>>>(p);
        unique_scatter_kernel<<<grid, LG_LINK_THREADS, 0, s>>>(p);
    }
    hipCheckError();
}

}  // namespace lg
