// kernels_in_edges.hip -- a neighbourhood taken whole for gfx950 (CDNA4, wave64): the prefix sums of the degrees of a list of rows
// (legion_row_offsets; DGL's g.in_degrees by differences) and every entry of those rows as (dst, src, eid) triples (legion_in_edges; DGL's
// g.in_edges(v, form='all'), the edges of MultiLayerFullNeighborSampler(1)).  The rules are the contracts in include/legion_hip.h.
// The layout: 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles (the walks' cap, walk_step.h), every
// offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * row_offsets: three launches, the count / one-workgroup scan / apply of unique_ids (kernels_link.hip) over int64 sums:
//       degree   a lane per row: the pair {indptr[r], indptr[r + 1]} as one 16-byte load, the degree to offsets_out[i]; the tile's sum
//                (a shuffle reduction inside a wave, four wave totals through LDS) to scratch;
//       scan     ONE workgroup: the exclusive prefix sums of the at most 4 096 tile sums in place, and the total to offsets_out[n];
//       apply    a tile's in-tile exclusive scan of the degrees it reads back, plus its base, over offsets_out[i];
//   * in_edges: a workgroup takes tiles of 1 024 consecutive slots, four per lane, 256 apart (find_edges' tile): consecutive lanes write
//     consecutive slots and inside a row read consecutive column entries, so a hub row is spread over lanes and workgroups and short
//     rows idle no lane.  Per tile the first and the last row index it touches come from two upper-bound searches over offsets in global
//     memory, run interleaved; if that range with its closing offset has at most 1 025 entries it is staged in LDS and each slot searches
//     there, else (any number of empty rows may lie between a tile's at most 1 024 non-empty ones) each slot searches the range in global
//     memory.  A lane's four searches, and the loads of rows, the row pair and col behind them, are interleaved.  Measured against
//     every slot searching all of offsets in global memory (a fifth slower) and against staging each row's pair {indptr[r], indptr[r + 1]}
//     beside the offsets (12 KiB more LDS, seven workgroups a CU: 4 -- 20 % slower); neither is built.
// Bound: in_edges by its stores and the col reads (12 -- 20 bytes a slot); no MFMA.
#include "legion_core.h"
#include "upper_counts.h"
#include "walk_step.h"

namespace lg {

#define LG_IN_EDGES_THREADS 256
#define LG_IN_EDGES_ILP 4                                     // slots per lane, 256 apart
#define LG_IN_EDGES_TILE (LG_IN_EDGES_THREADS * LG_IN_EDGES_ILP)
#define LG_IN_EDGES_STAGE (LG_IN_EDGES_TILE + 1)              // a tile's non-empty rows and the closing offset

static_assert(LG_IN_EDGES_THREADS == LG_WALK_THREADS, "the grids below are walk_grid's: a tile of 256 outputs, the walks' cap");

// ------------------------------------------------------------------------------------------
// row_offsets
// ------------------------------------------------------------------------------------------
// the sum of v over the workgroup, in every lane (both barriers inside: every lane of the workgroup calls it)
__device__ __forceinline__ int64_t tile_sum(int64_t v, int64_t* s_wave)
{
    for (int32_t off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    const int64_t sum = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return sum;
}

__global__ __launch_bounds__(LG_IN_EDGES_THREADS) void row_degree_kernel(const int64_t* indptr, int32_t node_num, const int32_t* rows,
                                                                         int32_t n, int32_t n_tiles, int64_t* offsets, int64_t* tiles)
{
    __shared__ int64_t s_wave[LG_IN_EDGES_THREADS / 64];
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = (int64_t)tile * LG_IN_EDGES_THREADS + threadIdx.x;
        int64_t deg = 0;
        if (i < n) {
            const int32_t r = rows[i];
            if ((uint32_t)r < (uint32_t)node_num) {                   // else: no memory is read for r
                const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(indptr + r);      // (r + 1 <= node_num: inside indptr)
                deg = row.e - row.s;
            }
            offsets[i] = deg;
        }
        const int64_t sum = tile_sum(deg, s_wave);
        if (threadIdx.x == 0) tiles[tile] = sum;
    }
}

// one workgroup: tiles[] becomes its exclusive prefix sums, total[0] the total
__global__ __launch_bounds__(LG_IN_EDGES_THREADS) void row_scan_kernel(int64_t* tiles, int32_t n_tiles, int64_t* total)
{
    __shared__ int64_t s_wave[LG_IN_EDGES_THREADS / 64];
    const int32_t per = (n_tiles + LG_IN_EDGES_THREADS - 1) / LG_IN_EDGES_THREADS;      // a thread's run of consecutive tiles
    const int32_t t0 = min((int32_t)threadIdx.x * per, n_tiles), t1 = min(t0 + per, n_tiles);
    int64_t sum = 0;
    for (int32_t t = t0; t < t1; t++) sum += tiles[t];
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
        const int64_t c = tiles[t];
        tiles[t] = before;
        before += c;
    }
    if (threadIdx.x == LG_IN_EDGES_THREADS - 1) total[0] = before;    // (the last thread's run ends the array, or is empty behind it)
}

__global__ __launch_bounds__(LG_IN_EDGES_THREADS) void row_apply_kernel(int32_t n, int32_t n_tiles, int64_t* offsets, const int64_t* tiles)
{
    __shared__ int64_t s_wave[LG_IN_EDGES_THREADS / 64];
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = (int64_t)tile * LG_IN_EDGES_THREADS + threadIdx.x;
        const int64_t deg = i < n ? offsets[i] : 0;
        int64_t inc = deg;                                            // inclusive over the wave
        const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int32_t off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(inc, off, 64);
            if (lane >= off) inc += y;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int64_t before = tiles[tile] + inc - deg;
        for (int32_t w = 0; w < wave; w++) before += s_wave[w];
        if (i < n) offsets[i] = before;
        __syncthreads();
    }
}

// the arguments are the caller's to check (legion_row_offsets); scratch holds row_offsets_scratch_bytes(n) bytes
void launch_row_offsets(hipStream_t s, const int64_t* indptr, int32_t node_num, const int32_t* rows, int32_t n, int64_t* offsets,
                        void* scratch, int64_t n_tiles)
{
    int64_t* tiles = static_cast<int64_t*>(scratch);
    const dim3 grid = walk_grid(n);
    if (n > 0) row_degree_kernel<<<grid, LG_IN_EDGES_THREADS, 0, s>>>(indptr, node_num, rows, n, (int32_t)n_tiles, offsets, tiles);
    row_scan_kernel<<<1, LG_IN_EDGES_THREADS, 0, s>>>(tiles, (int32_t)n_tiles, offsets + n);      // (n == 0: no tiles, offsets[0] = 0)
    if (n > 0) row_apply_kernel<<<grid, LG_IN_EDGES_THREADS, 0, s>>>(n, (int32_t)n_tiles, offsets, tiles);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// in_edges
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_IN_EDGES_THREADS, 8) void in_edges_kernel(InEdgesParams p)
{
    constexpr int32_t ILP = LG_IN_EDGES_ILP;
    __shared__ int64_t s_off[LG_IN_EDGES_STAGE];
    const int64_t n_tiles = (p.m + LG_IN_EDGES_TILE - 1) / LG_IN_EDGES_TILE;
    const int32_t n1 = p.n + 1;                                       // offsets' entries
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * LG_IN_EDGES_TILE;
        // the row indices the tile touches: a = the first (its upper bound - 1, at least 0), b = the last's closing offset (at most n)
        const int64_t ends[2] = {p0, min(p0 + LG_IN_EDGES_TILE - 1, p.m - 1)};
        const bool both[2] = {true, true};
        int32_t ub[2];
        upper_counts<2>(p.offsets, n1, ends, both, ub);
        const int32_t a = max(ub[0] - 1, 0), b = min(ub[1], p.n);
        const int32_t cnt = max(b - a + 1, 0);                        // offsets[a .. b]: inside offsets[0 .. n]
        const bool staged = cnt <= LG_IN_EDGES_STAGE;
        if (staged)
            for (int32_t k = threadIdx.x; k < cnt; k += LG_IN_EDGES_THREADS) s_off[k] = p.offsets[a + k];
        __syncthreads();
        int64_t q[ILP];
        bool live[ILP];
        int32_t c[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            q[j] = p0 + threadIdx.x + (int64_t)j * LG_IN_EDGES_THREADS;
            live[j] = q[j] < p.m;
        }
        if (staged) upper_counts<ILP>(s_off, cnt, q, live, c);
        else upper_counts<ILP>(p.offsets + a, cnt, q, live, c);
        // slot q[j] lies in the row of index i = a + c - 1 (c == 0: before the range, no row), at position jj of it
        int32_t i[ILP], r[ILP];
        int64_t jj[ILP], e[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            i[j] = c[j] > 0 ? a + c[j] - 1 : -1;
            if (i[j] >= p.n) i[j] = -1;                               // past offsets[n]: no row
            const int64_t opens = i[j] < 0 ? 0 : staged ? s_off[c[j] - 1] : p.offsets[i[j]];      // offsets[i]
            jj[j] = i[j] >= 0 ? (int64_t)((uint64_t)q[j] - (uint64_t)opens) : -1;
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) r[j] = i[j] >= 0 ? p.rows[i[j]] : -1;
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            e[j] = -1;
            if ((uint32_t)r[j] < (uint32_t)p.node_num) {              // else: no memory is read for r
                const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + r[j]);      // (r + 1 <= node_num: inside indptr)
                if (jj[j] >= 0 && jj[j] < row.e - row.s) e[j] = row.s + jj[j];                        // s <= e < indptr[r + 1] <= E
            }
        }
        int32_t src[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) src[j] = e[j] >= 0 ? p.col[e[j]] : -1;      // a dead entry stays -1
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            if (live[j]) {
                p.dst[q[j]] = e[j] >= 0 ? i[j] : -1;
                p.src[q[j]] = src[j];
                if (p.eid) p.eid[q[j]] = e[j];
            }
        }
        __syncthreads();                                              // the next tile stages over s_off
    }
}

// the arguments are the caller's to check (legion_in_edges)
void launch_in_edges(hipStream_t s, const InEdgesParams& p)
{
    if (p.m <= 0) return;
    const dim3 grid = walk_grid((p.m + LG_IN_EDGES_ILP - 1) / LG_IN_EDGES_ILP);
    in_edges_kernel<<<grid, LG_IN_EDGES_THREADS, 0, s>>>(p);
    hipCheckError();
}

}  // namespace lg
