// kernels_induced.hip -- a vertex set and the subgraph it induces (DGL's node_subgraph; the ops behind ClusterGCN, GraphSAINT and
// ShaDow-GNN) for gfx950 (CDNA4, wave64).  The set is the open-addressing table of unique_ids (kernels_link.hip) as an object of its
// own: keys / first, the multiplicative hash, atomicCAS on the key then atomicMin on first, probed through node_set.h.  The edges are
// LABOR's count / scan / write (kernels_labor.hip) with two changes: the predicate is "the source is a member of the set", and the
// written source is the member's position in the set.  The rules are the contracts in include/legion_hip.h, their text induced_rule.h.
// The layout is in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides, every offset 64 bits wide, no
// workgroup waits for another and every loop carries its bound.
//   * clear    the table's 2 S words all-ones and the distinct count 0, one launch (captured and ordered with the rest);
//   * insert   a lane per node: at most S probes of atomicCAS, then atomicMin on first.  The one inserter that saw the empty key counts
//              the key: a ballot per wave, one atomicAdd per wave that claimed any;
//   * lookup   a grid-stride lane per id, node_set_positions<1>;
//   * count    a tile of 1 024 slots resolves (row_slots.h), then a lane's four probe chains run interleaved (node_set_positions<4>:
//              each probe step is a dependent load -- of four keys at once where the table starts at a 16-byte boundary -- and four are
//              in flight per lane); the kept slots are summed by ballot / popcount and four wave totals through LDS: one int64 per tile;
//   * scan     launch_scan_int64 (kernels_in_edges.hip) over the tiles' counts; the total K goes to the scratch and to count_out;
//   * write    resolves and probes again (cheaper than storing and re-reading 12 -- 20 bytes a slot, as LABOR measured), ranks the kept
//              slots strip-major by ballot + mbcnt and sixteen wave counts in LDS, stores guarded by [0, cap), then fills [K, cap) with
//              -1.  A tile whose prefix sum equals the next one's keeps nothing and is not resolved at all: for a small set on a large
//              graph that is most tiles.  66 VGPRs: seven waves per SIMD (at eight the four key groups spilled);
//   * offsets  a lane per i in [0, n]: a lower-bound search over dst[0 .. L) of at most 31 trips, one 8-byte store.
// Bound: the col reads and the probes' dependent loads (a table of at most 16 MB: the Infinity Cache holds it); no MFMA.
#include "legion_core.h"
#include "induced_rule.h"
#include "node_set.h"
#include "row_slots.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_ROW_TILE == 1024 && induced_tiles(LG_ROW_TILE + 1) == 2, "induced_rule.h counts the scratch in tiles of 1 024 slots");
static_assert(induced_groups(256 * LG_ROW_TILE + 1) == 2, "launch_scan_int64 sums per 256 tiles, as induced_rule.h counts the scratch");

// ------------------------------------------------------------------------------------------
// the set
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_clear_kernel(uint32_t* table, int64_t words, int32_t* distinct)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; i < words; i += (int64_t)gridDim.x * LG_ROW_THREADS) table[i] = 0xFFFFFFFFu;
    if (blockIdx.x == 0 && threadIdx.x == 0) distinct[0] = 0;
}

__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_insert_kernel(const int32_t* nodes, int32_t k, int32_t* keys, uint32_t* first,
                                                                         uint32_t mask, int32_t shift, int32_t* distinct)
{
    // the trip count is the wave's, not the lane's: every lane of a wave reaches the ballot
    for (int64_t base = (int64_t)blockIdx.x * LG_ROW_THREADS; base < k; base += (int64_t)gridDim.x * LG_ROW_THREADS) {
        const int64_t i = base + threadIdx.x;
        const int32_t id = i < k ? nodes[i] : -1;
        bool claimed = false;
        if (id >= 0) {                                                // a negative entry is a member of nothing
            uint32_t h = node_set_home(id, shift) & mask;
            for (uint32_t probe = 0; probe <= mask; probe++) {        // at most S probes; a free slot exists (S >= 2 k)
                const int32_t old = atomicCAS(keys + h, NODE_SET_EMPTY_KEY, id);
                if (old == NODE_SET_EMPTY_KEY || old == id) {
                    claimed = old == NODE_SET_EMPTY_KEY;              // exactly one inserter of a key sees the empty key
                    atomicMin(first + h, (uint32_t)i);
                    break;
                }
                h = (h + 1u) & mask;
            }
        }
        const unsigned long long b = __ballot(claimed);
        if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(distinct, __popcll(b));
    }
}

__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_lookup_kernel(NodeSetView s, const int32_t* ids, int64_t m, int32_t* local)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * LG_ROW_THREADS) {
        const int32_t v[1] = {ids[i]};
        int32_t pos[1];
        node_set_positions<1>(s, v, pos);
        local[i] = pos[0];
    }
}

// the arguments are the caller's to check (legion_node_set_build); set holds node_set_bytes(k) bytes
void launch_node_set_build(hipStream_t s, const int32_t* nodes, int32_t k, void* set, int32_t* distinct)
{
    const int64_t slots = node_set_slots(k);
    int32_t* keys = static_cast<int32_t*>(set);
    uint32_t* first = reinterpret_cast<uint32_t*>(keys + slots);
    node_set_clear_kernel<<<walk_grid(2 * slots), LG_ROW_THREADS, 0, s>>>(reinterpret_cast<uint32_t*>(keys), 2 * slots, distinct);
    if (k > 0)
        node_set_insert_kernel<<<walk_grid(k), LG_ROW_THREADS, 0, s>>>(nodes, k, keys, first, (uint32_t)(slots - 1), node_set_shift(slots), distinct);
    hipCheckError();
}

// the arguments are the caller's to check (legion_node_set_lookup)
void launch_node_set_lookup(hipStream_t s, const NodeSetView& set, const int32_t* ids, int64_t m, int32_t* local)
{
    if (m <= 0) return;
    node_set_lookup_kernel<<<walk_grid(m), LG_ROW_THREADS, 0, s>>>(set, ids, m, local);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the edges
// ------------------------------------------------------------------------------------------
// a lane's four slots and rule 3 for them
struct InducedSlots : LaneSlots {
    int32_t pos[LG_ROW_ILP];        // pos(src), -1: not kept
};

// Rules 1 -- 3 for the slots of a tile: the resolution, then the membership of src (a dead entry and a slot without an entry have
// src == -1 and are never probed for).  One barrier inside, resolve_row_slots'
__device__ __forceinline__ void induced_resolve(const InducedParams& p, int64_t tile, int64_t* s_off, InducedSlots& o)
{
    resolve_row_slots(p.slots, tile, s_off, o);
    node_set_positions<LG_ROW_ILP>(p.set, o.src, o.pos);              // (src is -1 wherever e is: no entry, no probe)
}

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void induced_count_kernel(InducedParams p)
{
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_wave[LG_ROW_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        InducedSlots o;
        induced_resolve(p, tile, s_off, o);
        int32_t kept = 0;
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) kept += __popcll(__ballot(o.pos[j] >= 0));
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
        __syncthreads();                                              // (and: the next tile stages over s_off)
        if (threadIdx.x == 0) p.tiles[tile] = (int64_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        // the next write of s_wave lies behind the next tile's staging barrier
    }
}

// the arguments are the caller's to check (legion_induced_count)
void launch_induced_count(hipStream_t s, const InducedParams& p)
{
    if (p.n_tiles > 0) induced_count_kernel<<<walk_grid(p.n_tiles * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);
    // tiles[0 .. n_tiles) becomes its exclusive prefix sums, tiles[n_tiles] and count[0] the total (m == 0: both totals 0, only)
    launch_scan_int64(s, p.tiles, (int32_t)p.n_tiles, p.tiles + p.n_tiles + 1, (int32_t)p.n_groups, false, p.tiles + p.n_tiles, p.count);
}

__global__ __launch_bounds__(LG_ROW_THREADS, 7) void induced_edges_kernel(InducedParams p)
{
    constexpr int32_t ILP = LG_ROW_ILP, WAVES = LG_ROW_THREADS / 64;
    __shared__ int64_t s_off[LG_ROW_STAGE];
    __shared__ int32_t s_cnt[ILP * WAVES];                            // [strip][wave]: the order of the ranks
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)p.tiles[tile];                // (whatever it holds: the stores below are guarded)
        if ((uint64_t)p.tiles[tile + 1] == base) continue;            // the tile keeps nothing ([n_tiles] is the total): the whole workgroup skips it
        InducedSlots o;
        induced_resolve(p, tile, s_off, o);
        int32_t below[ILP];                                           // kept slots of the strip in lower lanes of this wave
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const unsigned long long b = __ballot(o.pos[j] >= 0);
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
            if (o.pos[j] >= 0 && at < (uint64_t)p.cap) {
                p.dst[at] = o.i[j];
                p.src[at] = o.pos[j];
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

// the arguments are the caller's to check (legion_induced_edges)
void launch_induced_edges(hipStream_t s, const InducedParams& p)
{
    if (p.cap <= 0) return;
    const int64_t tiles = p.n_tiles > (p.cap + LG_ROW_TILE - 1) / LG_ROW_TILE ? p.n_tiles : (p.cap + LG_ROW_TILE - 1) / LG_ROW_TILE;
    induced_edges_kernel<<<walk_grid(tiles * LG_ROW_THREADS), LG_ROW_THREADS, 0, s>>>(p);      // a workgroup per tile, of slots or of the fill
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the row pointers
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS) void dst_offsets_kernel(const int32_t* dst, int64_t cap, const int64_t* count, int32_t n, int64_t* indptr)
{
    const int64_t total = count[0];
    const int64_t L = total < 0 ? 0 : total > cap ? cap : total;      // <= 2^31 - 1
    for (int64_t i = (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * LG_ROW_THREADS) {
        int64_t lo = 0, len = L;                                      // #{ p in [0, L) : dst[p] < i }: the answer lies in [lo, lo + len]
        for (int32_t trip = 0; trip < 32 && len > 0; trip++) {        // len halves: at most 31 trips
            const int64_t half = len >> 1;
            if ((int64_t)dst[lo + half] < i) { lo += half + 1; len -= half + 1; }      // (lo + half < lo + len <= L <= cap)
            else len = half;
        }
        indptr[i] = lo;
    }
}

// the arguments are the caller's to check (legion_dst_offsets)
void launch_dst_offsets(hipStream_t s, const int32_t* dst, int64_t cap, const int64_t* count, int32_t n, int64_t* indptr)
{
    dst_offsets_kernel<<<walk_grid((int64_t)n + 1), LG_ROW_THREADS, 0, s>>>(dst, cap, count, n, indptr);
    hipCheckError();
}

}  // namespace lg
