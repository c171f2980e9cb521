// walk_step.h -- what the walk ops over the full CSR share (kernels_walk.hip, kernels_node2vec.hip, kernels_pinsage.hip, kernels_link.hip),
// each piece once: a step's row and candidate (rule steps 1-5 of legion_random_walk, include/legion_hip.h), the unit draw, the search
// of a sorted row, and the tile of 256 walks whose trace rows are staged in LDS and flushed as runs.  Device code only.
#pragma once

#include "legion_core.h"
#include "draw_rule.h"

namespace lg {

#define LG_WALK_THREADS 256
#define LG_WALK_MAX_WG 2048      // 256 CUs x 8 resident workgroups: every further tile is a stride of the grid

static constexpr uint32_t kPow22 = make_pow_tables().t2[1];      // 48271^(2^22): from a try's candidate draw to its accept draw
static constexpr uint32_t kPow23 = make_pow_tables().t2[2];      // 48271^(2^23): from a try's candidate draw to the next try's

// {indptr[v], indptr[v + 1]}: adjacent int64s, 8-byte aligned
struct __attribute__((packed, aligned(8))) WalkRowPair { int64_t s, e; };

// a draw y in [1, 2^31 - 2] as a double in [0, 1]
__device__ __forceinline__ double unit_draw(uint32_t y)
{
    return (double)(uint32_t)(y - 1u) / 2147483646.0;
}

// is u in the sorted row[0 .. D)?  At most ceil(log2(D + 1)) dependent 4-byte loads, ended early by a hit
__device__ __forceinline__ bool row_has(const int32_t* row, int32_t D, int32_t u)
{
    int32_t lo = 0, m = D;
    while (m > 0) {
        const int32_t half = m >> 1, cv = row[lo + half];
        if (cv == u) return true;
        if (cv < u) { lo += half + 1; m -= half + 1; }
        else m = half;
    }
    return false;
}

// the row {s, D} of v, v < node_num, as ONE 16-byte load (8-byte aligned: the hardware asks for 4), and its total T when weighted;
// false: no step leaves v (no entries, or no weight)
template <bool WEIGHTED>
__device__ __forceinline__ bool walk_row(const WalkParams& p, int32_t v, int64_t& s, int32_t& D, float& T)
{
    const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + v);      // (v + 1 <= node_num: inside indptr)
    s = row.s;
    D = (int32_t)(row.e - s);
    if (D <= 0) return false;
    if (WEIGHTED) {
        T = p.edge_cdf[s + D - 1];
        if (!(T > 0.0f)) return false;
    }
    return true;
}

// the entry of the row {s, D} (total T) that the draw x picks: in [0, D)
template <bool WEIGHTED>
__device__ __forceinline__ int32_t walk_candidate(const WalkParams& p, int64_t s, int32_t D, float T, uint32_t x)
{
    if (!WEIGHTED) return draw_from_x(x, D);                                // r < 1: pick <= D - 1
    const float* c = p.edge_cdf + s;
    const double t = weighted_target(x, T);
    int32_t lo = 0, m = D;
    while (m > 0) weighted_step(c[lo + (m >> 1)], t, lo, m);                // probes lo + m / 2 < lo + m <= D
    return min(lo, D - 1);
}

// one transition of walk rule steps 1-5: the next vertex, or -1 when the walk has ended or ends here; eid = its position in col
template <bool WEIGHTED, bool RESTART>
__device__ __forceinline__ int32_t walk_step(const WalkParams& p, int32_t v, uint32_t n1, int64_t& eid)      // n1 = n + 1
{
    eid = -1;
    if ((uint32_t)v >= (uint32_t)p.node_num) return -1;                     // 1. ended (or a bad seed): before any load
    if (RESTART && unit_draw(minstd_pow(n1 + 0x80000000u)) < (double)p.restart_prob) return -1;      // 2.
    int64_t s;
    int32_t D;
    float T = 0.0f;                                                         // (read only when weighted, which sets it)
    if (!walk_row<WEIGHTED>(p, v, s, D, T)) return -1;                      // 3.
    const int32_t pick = walk_candidate<WEIGHTED>(p, s, D, T, minstd_pow(n1));      // 4.
    const int32_t u = p.col[s + pick];                                      // 5.
    if (u < 0) return -1;
    eid = s + pick;
    return u;
}

// ------------------------------------------------------------------------------------------
// The tile: 256 walks, one lane each, whose trace rows (and edge ids) are staged in LDS a chunk of positions at a time and leave as
// runs of chunk * 4 bytes per row; written step by step they would be 4-byte stores at a stride of (length + 1) * 4 bytes.  The
// staging rows are one entry longer than a chunk, so that the lanes' writes (stride chunk + 1, odd) and the flush's reads fall in
// distinct banks.  With edge ids the chunk is 8 positions, not 16: the int64 ids triple the staged bytes per position, and a chunk of
// 16 would leave three workgroups per CU where latency asks for all it can get; at 8 it is five (17 408 B and 27 648 B of LDS).
// The kernel declares the two arrays (TRACE and EID entries) and hands them over; per tile it calls begin, then per chunk stage for
// each of its width(p0) positions, then flush.  flush reads the w0 and live_rows that begin set, and it holds both barriers: every
// lane of the workgroup reaches every flush, a lane past the last walk and an ended walk included.
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int64_t walk_tiles(int64_t num_walks) { return (num_walks + LG_WALK_THREADS - 1) / LG_WALK_THREADS; }

template <bool EIDS>
struct WalkTile {
    static constexpr int32_t CHUNK = EIDS ? 8 : 16;      // trace positions staged per flush
    static constexpr int32_t PITCH = CHUNK + 1;
    static constexpr int32_t TRACE = LG_WALK_THREADS * PITCH, EID = EIDS ? TRACE : 1;
    int32_t* s_trace;
    int64_t* s_eid;
    int64_t w0;                  // the tile's first walk
    int32_t live_rows;           // its walks: 256 but for the last tile

    // the lane's walk of tile `tile`: its seed v (a lane past the last walk is an ended walk: no load, no store) and n1 = n + 1 of its
    // first step's draw index n
    __device__ __forceinline__ void begin(const WalkParams& p, int64_t tile, int32_t& v, uint32_t& n1)
    {
        w0 = tile * LG_WALK_THREADS;
        const int64_t w = w0 + threadIdx.x;
        live_rows = (int32_t)min((int64_t)LG_WALK_THREADS, (int64_t)p.num_walks - w0);
        v = (int32_t)threadIdx.x < live_rows ? p.seeds[w] : -1;
        n1 = (uint32_t)(p.base + w * p.length) + 1u;
    }

    // a trace row: positions 0 .. length; the positions of its chunk at p0
    static __device__ __forceinline__ int32_t row_len(const WalkParams& p) { return p.length + 1; }
    static __device__ __forceinline__ int32_t width(const WalkParams& p, int32_t p0) { return min(CHUNK, row_len(p) - p0); }

    // the lane's position k of the chunk
    __device__ __forceinline__ void stage(int32_t k, int32_t v, int64_t eid)
    {
        s_trace[threadIdx.x * PITCH + k] = v;
        if (EIDS) s_eid[threadIdx.x * PITCH + k] = eid;
    }

    // the tile's rows x the chunk's cw positions from p0 on, consecutive lanes on consecutive positions of a row
    __device__ __forceinline__ void flush(const WalkParams& p, int32_t p0, int32_t cw)
    {
        __syncthreads();
        for (int32_t i = threadIdx.x; i < LG_WALK_THREADS * CHUNK; i += LG_WALK_THREADS) {
            const int32_t r = i / CHUNK, k = i % CHUNK;
            if (r < live_rows && k < cw) {
                p.traces[(w0 + r) * row_len(p) + p0 + k] = s_trace[r * PITCH + k];
                if (EIDS && p0 + k > 0) p.edge_ids[(w0 + r) * p.length + p0 + k - 1] = s_eid[r * PITCH + k];
            }
        }
        __syncthreads();
    }
};

// the launchers' grid: a workgroup per tile, at most LG_WALK_MAX_WG
static inline dim3 walk_grid(int64_t num_walks)
{
    return dim3((uint32_t)(walk_tiles(num_walks) < LG_WALK_MAX_WG ? walk_tiles(num_walks) : LG_WALK_MAX_WG));
}

}  // namespace lg
