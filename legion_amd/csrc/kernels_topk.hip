// kernels_topk.hip -- the k best entries of each row (legion_row_topk, legion_topk_keys; DGL's select_topk and
// sample_neighbors(prob=, replace=False)) for gfx950 (CDNA4, wave64): a per-row selection of the k <= 64 smallest composites
// (key, position), the key by topk_rule.h, whose text runs here on the device.  The rules are the contracts in include/legion_hip.h.
// The shape is kernels_weights.hip's, because degrees run from 0 to millions and no lane may walk a row alone:
//   * rows of up to LG_TOPK_LONG entries: a wave per row, grid-strided under a grid of at most LG_TOPK_GRID workgroups of four waves.
//     The wave keeps its best 64 composites, one per lane, sorted ascending, a sentinel where there is none yet; the threshold is lane
//     k - 1's.  A step loads 64 consecutive col / w entries coalesced, forms the keys and ballots "eligible and below the threshold": no
//     vote, the common case a few steps into a long row, and the step is over.  Otherwise the step's 64 are bitonic-sorted DESCENDING
//     by cross-lane exchanges (no LDS) and the lane-wise minimum against the best list is a bitonic sequence of the 64 smallest of
//     both, which six merge stages sort again.  The first step of a row is one ascending sort;
//   * longer rows are only listed there, into the scratch by one atomic per row, and a second launch gives each a workgroup of 16
//     waves: every wave runs the loop above over its interleaved 64-entry steps, then the 16 sorted lists merge pairwise through LDS
//     (16 x 64 composites of 16 bytes: 16 KB), four levels.
// One kernel template over the mode; the selection is written once.  Every loop carries its bound; nothing is read outside rows,
// indptr, col and w, nothing written outside [i k, (i + 1) k) of the outputs and the listed scratch.
// Bound: the col / w reads; in SAMPLE the two double divisions and the series per entry.  No MFMA.
#include "legion_core.h"
#include "topk_rule.h"

namespace lg {

#define LG_TOPK_THREADS 256
#define LG_TOPK_LONG_THREADS 1024
#define LG_TOPK_LONG_WAVES (LG_TOPK_LONG_THREADS / 64)

// a candidate: its key and its position inside the row.  The sentinel is above every real one
struct Comp {
    uint64_t key;
    uint64_t j;
};
__device__ __forceinline__ bool comp_less(const Comp& a, const Comp& b) { return a.key < b.key || (a.key == b.key && a.j < b.j); }
__device__ __forceinline__ Comp comp_none() { return Comp{TOPK_NO_KEY, ~0ull}; }
__device__ __forceinline__ Comp comp_shfl_xor(const Comp& a, int32_t mask) { return Comp{__shfl_xor(a.key, mask), __shfl_xor(a.j, mask)}; }
__device__ __forceinline__ Comp comp_shfl(const Comp& a, int32_t lane) { return Comp{__shfl(a.key, lane), __shfl(a.j, lane)}; }

// one compare-exchange with the lane `stride` away: this lane keeps the smaller of the two iff keep_min
__device__ __forceinline__ void comp_exchange(Comp& v, int32_t stride, bool keep_min)
{
    const Comp o = comp_shfl_xor(v, stride);
    if (comp_less(o, v) == keep_min) v = o;
}

// the wave's 64 composites sorted across the lanes, ascending or descending: 21 exchanges
__device__ __forceinline__ void wave_sort(Comp& v, int32_t lane, bool ascending)
{
#pragma unroll
    for (int32_t size = 2; size <= 64; size <<= 1) {
        const bool up = ((lane & size) == 0) == ascending;            // (size 64: lane & 64 == 0 everywhere: the final direction)
#pragma unroll
        for (int32_t stride = size >> 1; stride > 0; stride >>= 1) comp_exchange(v, stride, ((lane & stride) == 0) == up);
    }
}

// a bitonic sequence over the lanes sorted ascending: 6 exchanges
__device__ __forceinline__ void wave_merge(Comp& v, int32_t lane)
{
#pragma unroll
    for (int32_t stride = 32; stride > 0; stride >>= 1) comp_exchange(v, stride, (lane & stride) == 0);
}

// best (ascending) and other (DESCENDING) -> the 64 smallest of both in best, ascending
__device__ __forceinline__ void wave_take(Comp& best, const Comp& other, int32_t lane)
{
    if (comp_less(other, best)) best = other;
    wave_merge(best, lane);
}

// the entries [first, D) of the row at `start`, `stride` apart in steps of 64, folded into best.  fresh: best is all sentinels
template <int32_t MODE>
__device__ __forceinline__ void scan_steps(const TopkParams& p, int64_t start, int64_t D, int64_t first, int64_t stride, int32_t lane, Comp& best,
                                           bool fresh)
{
    for (int64_t i0 = first; i0 < D; i0 += stride) {
        const int64_t i = i0 + lane;
        Comp c = comp_none();
        if (i < D) {
            const int64_t e = start + i;
            const int32_t src = p.col[e];
            const float w = p.w ? p.w[e] : 1.0f;
            if (topk_eligible(MODE, src, w, p.w != nullptr)) c = Comp{topk_key(MODE, w, p.key, e), (uint64_t)i};
        }
        const Comp thr = comp_shfl(best, p.k - 1);
        if (__ballot(comp_less(c, thr)) == 0ull) continue;            // (an ineligible entry is the sentinel: never below anything)
        if (fresh) {
            wave_sort(c, lane, true);
            best = c;
            fresh = false;
        } else {
            wave_sort(c, lane, false);
            wave_take(best, c, lane);
        }
    }
}

// row i's result from the wave's sorted list
__device__ __forceinline__ void write_row(const TopkParams& p, int32_t i, int64_t start, const Comp& best, int32_t lane)
{
    const bool have = lane < p.k && best.key != TOPK_NO_KEY;
    if (lane < p.k) {
        const int64_t at = (int64_t)i * p.k + lane;
        const int64_t e = start + (int64_t)best.j;
        p.src[at] = have ? p.col[e] : -1;
        if (p.eid) p.eid[at] = have ? e : -1;
    }
    const unsigned long long b = __ballot(have);
    if (p.count && lane == 0) p.count[i] = __popcll(b);
}

// (start, D) of rows[i]: D = 0 for a row outside the graph, for which nothing is read
__device__ __forceinline__ void row_extent(const TopkParams& p, int32_t i, int64_t& start, int64_t& D)
{
    const int32_t r = p.rows[i];
    start = 0;
    D = 0;
    if (r >= 0 && r < p.node_num) {
        start = p.indptr[r];
        D = p.indptr[r + 1] - start;
        if (D < 0) D = 0;
    }
}

template <int32_t MODE>
__global__ __launch_bounds__(LG_TOPK_THREADS) void topk_rows_kernel(TopkParams p)
{
    const int32_t lane = threadIdx.x & 63;
    const int32_t waves = (int32_t)gridDim.x * (LG_TOPK_THREADS / 64);
    for (int32_t i = (int32_t)blockIdx.x * (LG_TOPK_THREADS / 64) + (int32_t)(threadIdx.x >> 6); i < p.n; i += waves) {
        int64_t start, D;
        row_extent(p, i, start, D);
        if (D > LG_TOPK_LONG) {
            if (lane == 0) {
                const int32_t at = atomicAdd(p.long_rows, 1);
                if (at >= 0 && at < p.n) p.long_rows[1 + at] = i;      // (always: every row is listed at most once)
            }
            continue;
        }
        Comp best = comp_none();
        scan_steps<MODE>(p, start, D, 0, 64, lane, best, true);
        write_row(p, i, start, best, lane);
    }
}

template <int32_t MODE>
__global__ __launch_bounds__(LG_TOPK_LONG_THREADS) void topk_long_rows_kernel(TopkParams p)
{
    __shared__ Comp s_list[LG_TOPK_LONG_WAVES][64];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t n_long = p.long_rows[0];
    n_long = n_long < 0 ? 0 : n_long > p.n ? p.n : n_long;
    for (int32_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const int32_t i = p.long_rows[1 + q];
        if (i < 0 || i >= p.n) continue;                               // (whatever the scratch holds; the whole workgroup alike)
        int64_t start, D;
        row_extent(p, i, start, D);
        Comp best = comp_none();
        scan_steps<MODE>(p, start, D, (int64_t)wave * 64, (int64_t)LG_TOPK_LONG_THREADS, lane, best, true);
        // four levels: the upper wave of a pair hands its list over, the lower one takes it reversed, a descending list
#pragma unroll
        for (int32_t d = 1; d < LG_TOPK_LONG_WAVES; d <<= 1) {
            if ((wave & (2 * d - 1)) == d) s_list[wave][lane] = best;
            __syncthreads();
            if ((wave & (2 * d - 1)) == 0) wave_take(best, s_list[wave + d][63 - lane], lane);
        }
        if (wave == 0) write_row(p, i, start, best, lane);
        __syncthreads();                                              // (the next row's lists go over these)
    }
}

template <int32_t MODE>
static void launch_row_topk_mode(hipStream_t s, const TopkParams& p)
{
    int32_t grid = (p.n + LG_TOPK_THREADS / 64 - 1) / (LG_TOPK_THREADS / 64);
    if (grid > LG_TOPK_GRID) grid = LG_TOPK_GRID;
    topk_rows_kernel<MODE><<<grid, LG_TOPK_THREADS, 0, s>>>(p);
    hipCheckError();
    topk_long_rows_kernel<MODE><<<p.n < LG_TOPK_LONG_GRID ? p.n : LG_TOPK_LONG_GRID, LG_TOPK_LONG_THREADS, 0, s>>>(p);
    hipCheckError();
}

// the arguments are the caller's to check (legion_row_topk)
void launch_row_topk(hipStream_t s, const TopkParams& p)
{
    if (p.n <= 0) return;
    HIP_CALL(hipMemsetAsync(p.long_rows, 0, sizeof(int32_t), s));
    switch (p.mode) {
    case LEGION_TOPK_LARGEST: launch_row_topk_mode<LEGION_TOPK_LARGEST>(s, p); break;
    case LEGION_TOPK_SMALLEST: launch_row_topk_mode<LEGION_TOPK_SMALLEST>(s, p); break;
    default: launch_row_topk_mode<LEGION_TOPK_SAMPLE>(s, p); break;
    }
}

// ------------------------------------------------------------------------------------------
// the key rule alone
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_keys_kernel(const int32_t* __restrict__ col, int64_t num_edges, const float* __restrict__ w,
                                                         const int64_t* __restrict__ eids, int64_t n, int32_t mode, uint64_t key,
                                                         uint64_t* __restrict__ key_out, uint8_t* __restrict__ eligible_out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t e = eids[i];
        bool ok = false;
        uint64_t out = TOPK_NO_KEY;
        if (e >= 0 && e < num_edges) {
            const float x = w ? w[e] : 1.0f;
            ok = topk_eligible(mode, col[e], x, w != nullptr);
            if (ok) out = topk_key(mode, x, key, e);
        }
        key_out[i] = out;
        eligible_out[i] = ok ? 1 : 0;
    }
}

// the arguments are the caller's to check (legion_topk_keys)
void launch_topk_keys(hipStream_t s, const int32_t* col, int64_t num_edges, const float* w, const int64_t* eids, int64_t n, int32_t mode,
                      uint64_t key, uint64_t* key_out, uint8_t* eligible_out)
{
    if (n <= 0) return;
    int64_t grid = (n + 255) / 256;
    if (grid > 2048) grid = 2048;
    topk_keys_kernel<<<(uint32_t)grid, 256, 0, s>>>(col, num_edges, w, eids, n, mode, key, key_out, eligible_out);
    hipCheckError();
}

}  // namespace lg
