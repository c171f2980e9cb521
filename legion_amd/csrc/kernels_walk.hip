// kernels_walk.hip -- random walks over the full CSR for gfx950 (CDNA4, wave64): DGL's dgl.sampling.random_walk.
//
// The rule is the contract in include/legion_hip.h (legion_random_walk): walk w starts at seeds[w]; step j draws with the sampler's own
// minstd power at index n = base + w * length + (j - 1) (draw_rule.h), uniformly over the row or by the graph's prefix table, after an
// optional restart draw; an ended walk is -1 from there on.  One transition is walk_step (walk_step.h, shared with kernels_pinsage.hip).
//
// A walk is a chain of dependent random loads -- per step the row-pointer pair, ceil(log2(D + 1)) probes of the table when weighted,
// one column entry -- so nothing inside a walk can overlap and the rate comes from walks in flight: one lane per walk, 256 lanes per
// workgroup, eight workgroups per CU (at most 64 VGPRs, at most 20 KiB of LDS), a grid that strides over tiles of 256 walks.
//   * the row-pointer pair {indptr[v], indptr[v + 1]} is ONE 16-byte load (8-byte aligned: the hardware asks for 4);
//   * a tile's trace rows are staged in LDS a chunk of steps at a time and leave as runs of chunk * 4 bytes per row; written step by
//     step they would be 4-byte stores at a stride of (length + 1) * 4 bytes.  The staging rows are one entry longer than a chunk,
//     so that the lanes' writes (stride chunk + 1, odd) and the flush's reads fall in distinct banks;
//   * RESTART, WEIGHTED and EIDS are template flags: the plain instance has no restart draw, no table pointer and no edge-id staging.
//     With edge ids the chunk is 8 steps, not 16: the int64 ids triple the staged bytes per step, and a chunk of 16 would leave
//     three workgroups per CU where latency asks for all it can get; at 8 it is five.
// Bound: the part's rate of random requests at the occupancy above; no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"

namespace lg {

#define LG_WALK_THREADS 256
#define LG_WALK_MAX_WG 2048      // 256 CUs x 8 resident workgroups: every further tile is a stride of the grid

template <bool WEIGHTED, bool RESTART, bool EIDS>
__global__ __launch_bounds__(LG_WALK_THREADS, 8) void random_walk_kernel(WalkParams p)
{
    constexpr int32_t CHUNK = EIDS ? 8 : 16;             // trace positions staged per flush
    constexpr int32_t PITCH = CHUNK + 1;
    __shared__ int32_t s_trace[LG_WALK_THREADS * PITCH];
    __shared__ int64_t s_eid[EIDS ? LG_WALK_THREADS * PITCH : 1];
    const int32_t tid = threadIdx.x;
    const int32_t row_len = p.length + 1;                // positions 0 .. length of a trace row
    const int64_t n_tiles = ((int64_t)p.num_walks + LG_WALK_THREADS - 1) / LG_WALK_THREADS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t w0 = tile * LG_WALK_THREADS;
        const int64_t w = w0 + tid;
        const int32_t live_rows = (int32_t)min((int64_t)LG_WALK_THREADS, (int64_t)p.num_walks - w0);
        int32_t v = tid < live_rows ? p.seeds[w] : -1;    // (a lane past the last walk is an ended walk: no load, no store)
        uint32_t n1 = (uint32_t)(p.base + w * p.length) + 1u;
        for (int32_t p0 = 0; p0 < row_len; p0 += CHUNK) {
            const int32_t cw = min(CHUNK, row_len - p0);
            for (int32_t k = 0; k < cw; k++) {
                int64_t eid = -1;
                if (p0 + k > 0) v = walk_step<WEIGHTED, RESTART>(p, v, n1++, eid);      // position 0 is the seed, copied as given
                s_trace[tid * PITCH + k] = v;
                if (EIDS) s_eid[tid * PITCH + k] = eid;
            }
            __syncthreads();
            // the tile's rows x this chunk's positions, consecutive lanes on consecutive positions of a row
            for (int32_t i = tid; i < LG_WALK_THREADS * CHUNK; i += LG_WALK_THREADS) {
                const int32_t r = i / CHUNK, k = i % CHUNK;
                if (r < live_rows && k < cw) {
                    p.traces[(w0 + r) * row_len + p0 + k] = s_trace[r * PITCH + k];
                    if (EIDS && p0 + k > 0) p.edge_ids[(w0 + r) * p.length + p0 + k - 1] = s_eid[r * PITCH + k];
                }
            }
            __syncthreads();
        }
    }
}

template <bool WEIGHTED, bool RESTART>
static void launch_walk(hipStream_t s, dim3 grid, const WalkParams& p)
{
    if (p.edge_ids != nullptr) random_walk_kernel<WEIGHTED, RESTART, true><<<grid, LG_WALK_THREADS, 0, s>>>(p);
    else random_walk_kernel<WEIGHTED, RESTART, false><<<grid, LG_WALK_THREADS, 0, s>>>(p);
}

// the arguments are the caller's to check (legion_random_walk): this only picks the instance
void launch_random_walk(hipStream_t s, const WalkParams& p)
{
    if (p.num_walks <= 0) return;
    const int64_t n_tiles = ((int64_t)p.num_walks + LG_WALK_THREADS - 1) / LG_WALK_THREADS;
    const dim3 grid((uint32_t)(n_tiles < LG_WALK_MAX_WG ? n_tiles : LG_WALK_MAX_WG));
    const bool weighted = p.edge_cdf != nullptr, restart = p.restart_prob > 0.0f;
    if (weighted) { if (restart) launch_walk<true, true>(s, grid, p); else launch_walk<true, false>(s, grid, p); }
    else          { if (restart) launch_walk<false, true>(s, grid, p); else launch_walk<false, false>(s, grid, p); }
    hipCheckError();
}

}  // namespace lg
