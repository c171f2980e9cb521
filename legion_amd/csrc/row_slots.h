// row_slots.h -- the tile of a row expansion: what the kernels that spread the entries of a list of CSR rows over consecutive slots
// (kernels_in_edges.hip, kernels_labor.hip) share, each piece once: the tile's constants, the interleaved upper-bound searches and the
// resolution of a tile's slots to {row index, entry, source}.  Device code; include inside namespace lg's files after legion_core.h.
#pragma once

#include "legion_core.h"
#include "walk_step.h"

namespace lg {

#define LG_ROW_THREADS 256
#define LG_ROW_ILP 4                                          // slots per lane, 256 apart
#define LG_ROW_TILE (LG_ROW_THREADS * LG_ROW_ILP)
#define LG_ROW_STAGE (LG_ROW_TILE + 1)                        // a tile's non-empty rows and the closing offset

static_assert(LG_ROW_THREADS == LG_WALK_THREADS, "the grids of these kernels are walk_grid's: a tile of 256 outputs, the walks' cap");

// K upper bounds at once, their chains of dependent loads interleaved: c[j] = #{ v in [0, len) : a[v] <= q[j] } for a non-decreasing a
// (for any other a: some value in [0, len]); len <= 0 or !live[j]: 0.  Reads a[0 .. len) only.
template <int32_t K>
__device__ __forceinline__ void upper_counts(const int64_t* a, int32_t len, const int64_t (&q)[K], const bool (&live)[K], int32_t (&c)[K])
{
    int32_t m[K];
#pragma unroll
    for (int32_t j = 0; j < K; j++) {
        c[j] = 0;
        m[j] = live[j] ? max(len, 0) : 0;
    }
    bool more = true;
    while (more) {                                                    // each trip halves every m[j] > 0: at most 21 trips
        more = false;
        int64_t v[K];
#pragma unroll
        for (int32_t j = 0; j < K; j++) v[j] = m[j] > 0 ? a[c[j] + (m[j] >> 1)] : 0;      // (c + m / 2 < c + m <= len)
#pragma unroll
        for (int32_t j = 0; j < K; j++) {
            if (m[j] > 0) {
                const int32_t half = m[j] >> 1;
                if (v[j] <= q[j]) { c[j] += half + 1; m[j] -= half + 1; }
                else m[j] = half;
                more |= m[j] > 0;
            }
        }
    }
}

// what a lane knows of its four slots of a tile
struct LaneSlots {
    int64_t q[LG_ROW_ILP];          // the slot
    int64_t e[LG_ROW_ILP];          // its entry of col, -1: none
    int64_t d[LG_ROW_ILP];          // its row's whole degree, dead entries and slots past m included; 0: no row
    int32_t i[LG_ROW_ILP];          // its index into rows, -1: none
    int32_t src[LG_ROW_ILP];        // col[e], -1: no entry or a dead one
    bool live[LG_ROW_ILP];          // q < m
};

// The slots of a tile of 1 024 consecutive ones, four per lane, 256 apart.  The first and the last row index the tile touches come from
// two interleaved upper-bound searches over offsets in global memory; if that range with its closing offset has at most 1 025 entries
// it is staged in s_off (LG_ROW_STAGE entries) and each slot searches there, else (any number of empty rows may lie between a tile's
// at most 1 024 non-empty ones) each slot searches the range in global memory.  A lane's four searches, and the loads of rows, the row
// pair and col behind them, are interleaved.  Whatever the offsets hold, nothing is read outside them, rows, indptr and col.  One
// barrier inside (every lane of the workgroup calls it); the caller puts another between this call and the next, which stages over s_off.
__device__ __forceinline__ void resolve_row_slots(const RowSlots& p, int64_t tile, int64_t* s_off, LaneSlots& o)
{
    constexpr int32_t ILP = LG_ROW_ILP;
    const int32_t n1 = p.n + 1;                                       // offsets' entries
    const int64_t p0 = tile * LG_ROW_TILE;
    // the row indices the tile touches: a = the first (its upper bound - 1, at least 0), b = the last's closing offset (at most n)
    const int64_t ends[2] = {p0, min(p0 + LG_ROW_TILE - 1, p.m - 1)};
    const bool both[2] = {true, true};
    int32_t ub[2];
    upper_counts<2>(p.offsets, n1, ends, both, ub);
    const int32_t a = max(ub[0] - 1, 0), b = min(ub[1], p.n);
    const int32_t cnt = max(b - a + 1, 0);                            // offsets[a .. b]: inside offsets[0 .. n]
    const bool staged = cnt <= LG_ROW_STAGE;
    if (staged)
        for (int32_t k = threadIdx.x; k < cnt; k += LG_ROW_THREADS) s_off[k] = p.offsets[a + k];
    __syncthreads();
    int32_t c[ILP];
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) {
        o.q[j] = p0 + threadIdx.x + (int64_t)j * LG_ROW_THREADS;
        o.live[j] = o.q[j] < p.m;
    }
    if (staged) upper_counts<ILP>(s_off, cnt, o.q, o.live, c);
    else upper_counts<ILP>(p.offsets + a, cnt, o.q, o.live, c);
    // slot q[j] lies in the row of index i = a + c - 1 (c == 0: before the range, no row), at position jj of it
    int32_t r[ILP];
    int64_t jj[ILP];
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
        o.d[j] = 0;
        if ((uint32_t)r[j] < (uint32_t)p.node_num) {                  // else: no memory is read for r
            const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + r[j]);      // (r + 1 <= node_num: inside indptr)
            o.d[j] = row.e - row.s;
            if (jj[j] >= 0 && jj[j] < o.d[j]) o.e[j] = row.s + jj[j];  // s <= e < indptr[r + 1] <= E
        }
    }
#pragma unroll
    for (int32_t j = 0; j < ILP; j++) o.src[j] = o.e[j] >= 0 ? p.col[o.e[j]] : -1;      // a dead entry stays -1
}

}  // namespace lg
