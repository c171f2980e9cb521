// kernels_metapath.hip -- metapath random walks and PinSAGE over a metapath on typed edges for gfx950 (CDNA4, wave64): DGL's
// dgl.sampling.random_walk(g, nodes, metapath=[...]) and PinSAGESampler(g, ntype, other_type, ...) on a graph whose rows are sorted by
// edge type (legion_graph_set_edge_types).
//
// The rule is the contract in include/legion_hip.h (legion_metapath_walk, legion_pinsage_metapath_neighbors), its text metapath_rule.h:
// step j of a walk draws uniformly inside the segment of type metapath[(j - 1) mod L] of the current row, with the walk ops' own draw.
//
// Both kernels keep the outer shape of the kernels they extend, because the reason for that shape is unchanged: a walk is a chain of
// dependent random loads, so its rate comes from walks in flight -- a lane per walk, 256 lanes a workgroup, eight workgroups a CU (at
// most 64 VGPRs), WalkTile's LDS staging and run-wise flush (walk_step.h) for the traces, kernels_pinsage.hip's visit segments, sorts
// and output (pinsage_tile.h) for PinSAGE.  What is new is the step: the row pair, the row's TYPE SEGMENT, one column entry.
//   * the metapath: 64 bytes of kernel arguments (MetapathWords), copied once with constant indices into 64 bytes of LDS.  Every lane
//     of a workgroup is at the same step, so reading the step's type is one LDS address for the wave, a broadcast; a running period
//     index replaces the modulo;
//   * short rows, D <= LG_METAPATH_SHORT (16): the row's type bytes lie in three aligned 8-byte words.  All three loads are in flight
//     together, the row's 16 bytes are shifted out of them into two registers, and the segment's ends are two masked byte counts
//     (a compare of eight bytes at once, then a population count): one round trip, no search.  Where a word would leave etype[0, E)
//     -- a row in the array's first 7 or last 23 bytes -- the row is read byte by byte instead, clipped to the row;
//   * long rows: the lower bounds of t and of t + 1 are two searches run as ONE loop: a round issues both brackets' probes before it
//     uses any, and while the two brackets coincide the probes are shared.  t == 0 and t + 1 == T need no load: their bounds are 0 and
//     D.  The walk kernel searches with one probe a bracket a round (ceil(log2(D + 1)) dependent rounds, not twice that), PinSAGE with
//     three (ceil(log4(D + 1)) rounds): each has what was faster for it on the hub list.  Every probe lies inside its bracket,
//     lo + m <= D, whatever the bytes hold.
// Bound: the part's rate of random requests at the occupancy above, as kernels_walk.hip (DESIGN.md 4.28 has the measured cost of the
// segment step); no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"
#include "pinsage_tile.h"
#include "metapath_rule.h"

namespace lg {

#define LG_METAPATH_SHORT 16      // rows up to here are counted in registers, longer ones searched
// the long rows' search, per kernel: 2 = one probe a bracket a round, 4 = three.  Each kernel has the one that was faster for it on
// the hub list (DESIGN.md 4.28 has both measured for both)
#ifndef LG_METAPATH_WALK_ARITY
#define LG_METAPATH_WALK_ARITY 2
#endif
#ifndef LG_METAPATH_PINSAGE_ARITY
#define LG_METAPATH_PINSAGE_ARITY 4
#endif

static_assert(LEGION_ETYPE_MAX_TYPES <= 64, "count_at_least compares in seven bits: a type and t + 1 are at most 64");
static_assert(sizeof(MetapathWords) == sizeof(MetapathParams::path), "the metapath's words are the kernel's arguments");

// how many of the bytes of x that `valid` marks (0x80 per byte) are >= t, t in [0, 64]: bytes are below 128, so b + (128 - t) sets bit 7
// of its byte iff b >= t, and no byte carries into the next
__device__ __forceinline__ int32_t count_at_least(uint64_t x, uint64_t valid, int32_t t)
{
    const uint64_t sum = (x & 0x7F7F7F7F7F7F7F7Full) + (uint64_t)(128 - t) * 0x0101010101010101ull;
    return __popcll(sum & valid);
}

// 0x80 in each of the first n bytes: none for n <= 0, all eight for n >= 8
__device__ __forceinline__ uint64_t first_bytes(int32_t n)
{
    return n >= 8 ? 0x8080808080808080ull : (0x8080808080808080ull & ((1ull << (8 * max(n, 0))) - 1ull));
}

// the segment [lo, hi) of type t in the row {s, D}, D in [1, LG_METAPATH_SHORT]
__device__ __forceinline__ void short_segment(const MetapathParams& p, int64_t s, int32_t D, int32_t t, int32_t& lo, int32_t& hi)
{
    const uintptr_t first = reinterpret_cast<uintptr_t>(p.etype), at = first + (uintptr_t)s, a0 = at & ~(uintptr_t)7;
    uint64_t r0, r1;                                                         // the row's bytes 0 .. 7 and 8 .. 15
    if (a0 >= first && a0 + 24 <= first + (uintptr_t)p.num_edges) {
        const uint64_t* w = reinterpret_cast<const uint64_t*>(a0);          // bytes [a0, a0 + 24) hold [at, at + 16)
        const uint64_t w0 = w[0], w1 = w[1], w2 = w[2];
        const uint32_t sh = (uint32_t)(at & 7) * 8;
        r0 = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
        r1 = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
    } else {
        const uint8_t* row = p.etype + s;
        r0 = r1 = 0;
#pragma unroll
        for (int32_t i = 0; i < 8; i++) {                                    // s + i < s + D <= E
            if (i < D) r0 |= (uint64_t)row[i] << (8 * i);
            if (i + 8 < D) r1 |= (uint64_t)row[i + 8] << (8 * i);
        }
    }
    const uint64_t v0 = first_bytes(D), v1 = first_bytes(D - 8);
    lo = D - count_at_least(r0, v0, t) - count_at_least(r1, v1, t);
    hi = D - count_at_least(r0, v0, t + 1) - count_at_least(r1, v1, t + 1);
}

// one round of the 4-ary search on the bracket {lo, m}, m > 0: the probes lie at q1 <= q2 <= q3 < lo + m, and c says of each whether
// its entry lies before the bound.  Taken from the last probe down, so a branch's two probes differ and m stays >= 0 whatever the
// bytes hold; lo + m never grows
__device__ __forceinline__ void narrow4(int32_t& lo, int32_t& m, int32_t q1, int32_t q2, int32_t q3, bool c1, bool c2, bool c3)
{
    const int32_t end = lo + m;
    if (c3) { lo = q3 + 1; m = end - lo; }
    else if (c2) { lo = q2 + 1; m = q3 - lo; }
    else if (c1) { lo = q1 + 1; m = q2 - lo; }
    else m = q1 - lo;
}

// the same of a longer row, three probes a bracket a round: ceil(log4(D + 1)) dependent rounds of up to six loads, all issued before
// any is used; while the brackets coincide the three probes are shared.  {lo, m} brackets the lower bound of t, {hi, n} that of t + 1
__device__ __forceinline__ void long_segment4(const MetapathParams& p, int64_t s, int32_t D, int32_t t, int32_t& lo, int32_t& hi)
{
    const uint8_t* row = p.etype + s;
    int32_t m = t > 0 ? D : 0, n = t + 1 < p.num_types ? D : 0;
    lo = 0;
    hi = D - n;
    while ((m | n) > 0) {
        const int32_t i1 = lo + (m >> 2), i2 = lo + (m >> 1), i3 = i2 + (m >> 2);      // m / 2 + m / 4 < m
        const int32_t k1 = hi + (n >> 2), k2 = hi + (n >> 1), k3 = k2 + (n >> 2);
        const bool same = lo == hi && m == n;
        int32_t a1 = 0, a2 = 0, a3 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (m > 0) { a1 = row[i1]; a2 = row[i2]; a3 = row[i3]; }            // i3 < lo + m <= D
        if (n > 0 && !same) { b1 = row[k1]; b2 = row[k2]; b3 = row[k3]; }   // k3 < hi + n <= D
        if (same) { b1 = a1; b2 = a2; b3 = a3; }
        if (m > 0) narrow4(lo, m, i1, i2, i3, a1 < t, a2 < t, a3 < t);
        if (n > 0) narrow4(hi, n, k1, k2, k3, b1 <= t, b2 <= t, b3 <= t);
    }
}

// the same with one probe a bracket a round: ceil(log2(D + 1)) rounds; lo + m <= D and hi + n <= D throughout
__device__ __forceinline__ void long_segment2(const MetapathParams& p, int64_t s, int32_t D, int32_t t, int32_t& lo, int32_t& hi)
{
    const uint8_t* row = p.etype + s;
    int32_t m = t > 0 ? D : 0, n = t + 1 < p.num_types ? D : 0;
    lo = 0;
    hi = D - n;
    while ((m | n) > 0) {
        const int32_t i = lo + (m >> 1), k = hi + (n >> 1);
        int32_t a = 0, b = 0;
        if (m > 0) a = row[i];                                               // i < lo + m <= D
        if (n > 0 && (m <= 0 || k != i)) b = row[k];                         // k < hi + n <= D
        if (n > 0 && m > 0 && k == i) b = a;
        if (m > 0) {
            if (a < t) { lo = i + 1; m -= (m >> 1) + 1; } else m >>= 1;
        }
        if (n > 0) {
            if (b <= t) { hi = k + 1; n -= (n >> 1) + 1; } else n >>= 1;
        }
    }
}

// one transition of the metapath rule for type t: the next vertex, or -1 when the walk has ended or ends here; eid = its position in
// col.  restart_now: the step takes the restart draw (every step of a walk, the first of a later traversal in PinSAGE)
template <bool RESTART, int ARITY>
__device__ __forceinline__ int32_t metapath_step(const MetapathParams& p, int32_t v, uint32_t n1, int32_t t, bool restart_now, int64_t& eid)
{
    eid = -1;
    if ((uint32_t)v >= (uint32_t)p.walk.node_num) return -1;                 // 1. ended (or a bad seed): before any load
    if (RESTART && restart_now && unit_draw(minstd_pow(n1 + 0x80000000u)) < (double)p.walk.restart_prob) return -1;      // 2.
    int64_t s;
    int32_t D;
    float total;
    if (!walk_row<false>(p.walk, v, s, D, total)) return -1;                 // 3.
    int32_t lo, hi;                                                          // 4.
    if (D <= LG_METAPATH_SHORT) short_segment(p, s, D, t, lo, hi);
    else if (ARITY == 4) long_segment4(p, s, D, t, lo, hi);
    else long_segment2(p, s, D, t, lo, hi);
    if (hi <= lo) return -1;
    const int32_t pick = lo + draw_from_x(minstd_pow(n1), hi - lo);          // r < 1: pick < hi <= D
    const int32_t u = p.walk.col[s + pick];                                  // 5.
    if (u < 0) return -1;
    eid = s + pick;
    return u;
}

// the metapath from the kernel's arguments into LDS; the caller holds the barrier
__device__ __forceinline__ void stage_metapath(const MetapathParams& p, uint64_t* s_path)
{
    if (threadIdx.x == 0) {
#pragma unroll
        for (int32_t w = 0; w < 8; w++) s_path[w] = p.path[w];
    }
}

template <bool RESTART, bool EIDS>
__global__ __launch_bounds__(LG_WALK_THREADS, 8) void metapath_walk_kernel(MetapathParams p)
{
    using Tile = WalkTile<EIDS>;
    __shared__ int32_t s_trace[Tile::TRACE];
    __shared__ int64_t s_eid[Tile::EID];
    __shared__ uint64_t s_path[8];
    const uint8_t* path = reinterpret_cast<const uint8_t*>(s_path);
    stage_metapath(p, s_path);
    __syncthreads();
    Tile tile{s_trace, s_eid};
    for (int64_t t = blockIdx.x; t < walk_tiles(p.walk.num_walks); t += gridDim.x) {
        int32_t v;
        uint32_t n1;
        tile.begin(p.walk, t, v, n1);
        int32_t pi = 0;                                                      // (j - 1) mod L of the next step j: the same in every lane
        for (int32_t p0 = 0; p0 < Tile::row_len(p.walk); p0 += Tile::CHUNK) {
            const int32_t cw = Tile::width(p.walk, p0);
            for (int32_t k = 0; k < cw; k++) {
                int64_t eid = -1;
                if (p0 + k > 0) {                                            // position 0 is the seed, copied as given
                    v = metapath_step<RESTART, LG_METAPATH_WALK_ARITY>(p, v, n1++, path[pi], true, eid);
                    pi = metapath_next(pi, p.period);
                }
                tile.stage(k, v, eid);
            }
            tile.flush(p.walk, p0, cw);
        }
    }
}

// kernels_pinsage.hip's kernel with the metapath step in phase 1: walk r of a seed makes Q traversals of the L-step metapath and its
// visit q lands in s_vis[seed][r * Q + q]; the termination draw comes before the first step of traversals 2 .. Q only
template <int VPAD, bool RESTART>
__global__ __launch_bounds__(LG_PINSAGE_THREADS, 8) void pinsage_metapath_kernel(PinsageMetapathParams p)
{
    constexpr int32_t S = LG_PINSAGE_SLOTS / VPAD;       // seeds of a tile
    __shared__ __attribute__((aligned(16))) int32_t s_vis[LG_PINSAGE_LDS_ENTRIES];
    __shared__ __attribute__((aligned(16))) int32_t s_key[LG_PINSAGE_LDS_ENTRIES];
    __shared__ uint64_t s_path[8];
    const uint8_t* path = reinterpret_cast<const uint8_t*>(s_path);
    const int32_t tid = threadIdx.x;
    const int32_t R = p.walks_per_seed, Q = p.num_traversals, L = p.m.period, K = p.num_neighbors;
    const int64_t n = p.m.walk.num_walks;
    const int64_t n_tiles = (n + S - 1) / S;
    stage_metapath(p.m, s_path);                         // (the first tile's barrier below orders it before any read)
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t seed0 = tile * S;
        const int32_t live = (int32_t)min((int64_t)S, n - seed0);
#pragma unroll
        for (int32_t q = 0; q < 8; q++) s_vis[lds_at(tid + q * LG_PINSAGE_THREADS)] = LG_PINSAGE_EMPTY;
        __syncthreads();
        // 1. the walks of the tile's live seeds: live * R <= S * VPAD
        for (int32_t wl = tid; wl < live * R; wl += LG_PINSAGE_THREADS) {
            const int32_t sl = wl / R, r = wl - sl * R;
            const int64_t w = (seed0 + sl) * R + r;
            int32_t v = p.m.walk.seeds[seed0 + sl];
            uint32_t n1 = (uint32_t)(p.m.walk.base + w * Q * L) + 1u;
            int32_t out = sl * VPAD + r * Q;                                 // r * Q + Q <= R * Q <= VPAD
            for (int32_t q = 0; q < Q && v >= 0; q++) {
                for (int32_t pi = 0; pi < L && v >= 0; pi++) {
                    int64_t eid;
                    v = metapath_step<RESTART, LG_METAPATH_PINSAGE_ARITY>(p.m, v, n1++, path[pi], pi == 0 && q > 0, eid);
                }
                if (v >= 0) s_vis[lds_at(out++)] = v;                        // a walk that ends inside a traversal records nothing more
            }
        }
        __syncthreads();
        // 2.-5. (pinsage_tile.h)
        pinsage_rank_and_emit<VPAD>(s_vis, s_key, tid, seed0, live, K, p.neighbors, p.counts);
        __syncthreads();                                                     // (the next tile's fill overwrites what these lanes read)
    }
}

// the arguments are the caller's to check (legion_metapath_walk): this only picks the instance
void launch_metapath_walk(hipStream_t s, const MetapathParams& p)
{
    if (p.walk.num_walks <= 0) return;
    const dim3 grid = walk_grid(p.walk.num_walks);
    const bool restart = p.walk.restart_prob > 0.0f, eids = p.walk.edge_ids != nullptr;
    if (restart) {
        if (eids) metapath_walk_kernel<true, true><<<grid, LG_WALK_THREADS, 0, s>>>(p);
        else metapath_walk_kernel<true, false><<<grid, LG_WALK_THREADS, 0, s>>>(p);
    } else {
        if (eids) metapath_walk_kernel<false, true><<<grid, LG_WALK_THREADS, 0, s>>>(p);
        else metapath_walk_kernel<false, false><<<grid, LG_WALK_THREADS, 0, s>>>(p);
    }
    hipCheckError();
}

template <int VPAD>
static void launch_pinsage_metapath_class(hipStream_t s, const PinsageMetapathParams& p)
{
    constexpr int64_t S = LG_PINSAGE_SLOTS / VPAD;
    const int64_t n_tiles = ((int64_t)p.m.walk.num_walks + S - 1) / S;
    const dim3 grid((uint32_t)(n_tiles < LG_WALK_MAX_WG ? n_tiles : LG_WALK_MAX_WG));
    if (p.m.walk.restart_prob > 0.0f) pinsage_metapath_kernel<VPAD, true><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
    else pinsage_metapath_kernel<VPAD, false><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
}

// ... (legion_pinsage_metapath_neighbors): the instance by R * Q
void launch_pinsage_metapath_neighbors(hipStream_t s, const PinsageMetapathParams& p)
{
    if (p.m.walk.num_walks <= 0) return;
    const int32_t visits = p.walks_per_seed * p.num_traversals;              // <= LEGION_PINSAGE_MAX_VISITS
    if (visits <= 32) launch_pinsage_metapath_class<32>(s, p);
    else if (visits <= 64) launch_pinsage_metapath_class<64>(s, p);
    else if (visits <= 256) launch_pinsage_metapath_class<256>(s, p);
    else launch_pinsage_metapath_class<1024>(s, p);
    hipCheckError();
}

}  // namespace lg
