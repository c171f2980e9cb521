// kernels_in_edges.hip -- a neighbourhood taken whole for gfx950 (CDNA4, wave64): the prefix sums of the degrees of a list of rows
// (legion_row_offsets; DGL's g.in_degrees by differences) and every entry of those rows as (dst, src, eid) triples (legion_in_edges; DGL's
// g.in_edges(v, form='all'), the edges of MultiLayerFullNeighborSampler(1)).  The rules are the contracts in include/legion_hip.h.
// The layout: 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles (the walks' cap, walk_step.h), every
// offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * the int64 scan (launch_scan_int64, LABOR's second level too): three launches whose pieces are tile_scan.h's:
//       sum      a lane per value, the sum per 256 values to the scratch (row_offsets runs its own, fused with the degrees);
//       scan     ONE workgroup: the exclusive prefix sums of the at most 4 096 sums in place, and the total to one or two places;
//       apply    the in-256 exclusive scan of the values read back, plus the base, over the values;
//   * row_offsets: the first launch of that scan is row_degree_kernel, a lane per row: the pair {indptr[r], indptr[r + 1]} as one
//     16-byte load, the degree to offsets_out[i], the tile's sum to scratch; the total goes to offsets_out[n];
//   * in_edges: a workgroup takes tiles of 1 024 consecutive slots, four per lane, 256 apart (find_edges' tile): consecutive lanes write
//     consecutive slots and inside a row read consecutive column entries, so a hub row is spread over lanes and workgroups and short
//     rows idle no lane.  The tile is resolved by row_slots.h (the range of offsets staged in LDS, or searched in global memory); the
//     kernel stores.  Measured against every slot searching all of offsets in global memory (a fifth slower) and against staging each
//     row's pair {indptr[r], indptr[r + 1]} beside the offsets (12 KiB more LDS, seven workgroups a CU: 4 -- 20 % slower); neither is
//     built.
// Bound: in_edges by its stores and the col reads (12 -- 20 bytes a slot); no MFMA.
#include "legion_core.h"
#include "row_slots.h"
#include "tile_scan.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_SCAN_THREADS == LG_WALK_THREADS, "the grids below are walk_grid's: a tile of 256 outputs, the walks' cap");

// ------------------------------------------------------------------------------------------
// the int64 scan
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_SCAN_THREADS) void scan_sum_kernel(const int64_t* values, int32_t n, int32_t n_sums, int64_t* sums)
{
    __shared__ int64_t s_wave[LG_SCAN_WAVES];
    for (int32_t g = blockIdx.x; g < n_sums; g += gridDim.x) {
        const int64_t i = (int64_t)g * LG_SCAN_THREADS + threadIdx.x;
        const int64_t sum = tile_sum<int64_t>(i < n ? values[i] : 0, s_wave);
        if (threadIdx.x == 0) sums[g] = sum;
    }
}

__global__ __launch_bounds__(LG_SCAN_THREADS) void scan_sums_kernel(int64_t* sums, int32_t n_sums, int64_t* total, int64_t* total2)
{
    __shared__ int64_t s_wave[LG_SCAN_WAVES];
    tile_scan_in_place(sums, n_sums, total, total2, s_wave);
}

__global__ __launch_bounds__(LG_SCAN_THREADS) void scan_apply_kernel(int64_t* values, int32_t n, int32_t n_sums, const int64_t* sums)
{
    __shared__ int64_t s_wave[LG_SCAN_WAVES];
    for (int32_t g = blockIdx.x; g < n_sums; g += gridDim.x) {
        const int64_t i = (int64_t)g * LG_SCAN_THREADS + threadIdx.x;
        const int64_t before = sums[g] + tile_exclusive<int64_t>(i < n ? values[i] : 0, s_wave);
        if (i < n) values[i] = before;
    }
}

void launch_scan_int64(hipStream_t s, int64_t* values, int32_t n, int64_t* sums, int32_t n_sums, bool summed, int64_t* total, int64_t* total2)
{
    if (n > 0 && !summed) scan_sum_kernel<<<walk_grid(n), LG_SCAN_THREADS, 0, s>>>(values, n, n_sums, sums);
    scan_sums_kernel<<<1, LG_SCAN_THREADS, 0, s>>>(sums, n_sums, total, total2);      // (n == 0: no sums, the totals 0, only)
    if (n > 0) scan_apply_kernel<<<walk_grid(n), LG_SCAN_THREADS, 0, s>>>(values, n, n_sums, sums);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// row_offsets
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_SCAN_THREADS) void row_degree_kernel(const int64_t* indptr, int32_t node_num, const int32_t* rows,
                                                                     int32_t n, int32_t n_tiles, int64_t* offsets, int64_t* tiles)
{
    __shared__ int64_t s_wave[LG_SCAN_WAVES];
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = (int64_t)tile * LG_SCAN_THREADS + threadIdx.x;
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

// the arguments are the caller's to check (legion_row_offsets); scratch holds row_offsets_scratch_bytes(n) bytes
void launch_row_offsets(hipStream_t s, const int64_t* indptr, int32_t node_num, const int32_t* rows, int32_t n, int64_t* offsets,
                        void* scratch, int64_t n_tiles)
{
    int64_t* tiles = static_cast<int64_t*>(scratch);
    if (n > 0) row_degree_kernel<<<walk_grid(n), LG_SCAN_THREADS, 0, s>>>(indptr, node_num, rows, n, (int32_t)n_tiles, offsets, tiles);
    launch_scan_int64(s, offsets, n, tiles, (int32_t)n_tiles, true, offsets + n, nullptr);
}

// ------------------------------------------------------------------------------------------
// in_edges
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS, 8) void in_edges_kernel(InEdgesParams p)
{
    __shared__ int64_t s_off[LG_ROW_STAGE];
    const int64_t n_tiles = (p.slots.m + LG_ROW_TILE - 1) / LG_ROW_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        LaneSlots o;
        resolve_row_slots(p.slots, tile, s_off, o);
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) {
            if (o.live[j]) {
                p.dst[o.q[j]] = o.e[j] >= 0 ? o.i[j] : -1;
                p.src[o.q[j]] = o.src[j];
                if (p.eid) p.eid[o.q[j]] = o.e[j];
            }
        }
        __syncthreads();                                              // the next tile stages over s_off
    }
}

// the arguments are the caller's to check (legion_in_edges)
void launch_in_edges(hipStream_t s, const InEdgesParams& p)
{
    if (p.slots.m <= 0) return;
    const dim3 grid = walk_grid((p.slots.m + LG_ROW_ILP - 1) / LG_ROW_ILP);
    in_edges_kernel<<<grid, LG_ROW_THREADS, 0, s>>>(p);
    hipCheckError();
}

}  // namespace lg
