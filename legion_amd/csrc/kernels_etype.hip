// kernels_etype.hip -- typed edges and a fan-out per edge type (legion_graph_set_edge_types, legion_etype_degrees,
// legion_etype_sample_count, legion_etype_sample_edges; DGL's sample_etype_neighbors with etype_sorted=True) for gfx950 (CDNA4, wave64).
// The rules are the contracts in include/legion_hip.h, their text etype_rule.h, which runs here on the device.
// The shape: a wave per row, a LANE PER TYPE (T <= 64), grid-strided under a grid of at most LG_ETYPE_GRID workgroups of four waves, as
// kernels_topk.hip's first class.  Nothing is kept between the passes but the rows' offsets: the count and the write pass both find the
// row's segments again (an n x (T + 1) table would be half a gigabyte at n = 2^20, T = 64).
//   * row_segments, written once: the row's D entries are sampled at 64 positions ceil(D / 64) apart, lane j loading ONE type byte (a
//     row of at most 64 entries is read whole, coalesced, and that is already the answer).  A lane whose sample's type differs from its
//     lower neighbour's (__shfl_up) records its lane number under its type in a 65-entry LDS row of its wave, preset to "none"; the row's
//     end records under T.  Lane t reads entry t back and a suffix-minimum over the lanes (six shuffles) gives it the first sample whose
//     type is >= t: its segment starts inside the ceil(D / 64) - 1 entries before that sample, where every lane runs the same number,
//     ceil(log2(D / 64)), of binary-search steps of one dependent byte load each, neighbouring lanes in neighbouring brackets.  Lane
//     t + 1's start, by shuffle, is lane t's end.  Whatever the bytes hold, every position stays inside the row;
//   * the fan-outs are seven 64-bit kernel arguments (EtypeFanouts): a lane shifts its type's out of scalar registers;
//   * count: lane t's slots (etype_slots), a wave sum, one int64 per row; launch_scan_int64 turns them into offsets;
//   * write: lane t's slots become the pair's place in the row by a wave prefix sum; then the non-empty pairs in type order (a ballot,
//     the pair's numbers by v_readlane): a pair taken whole is copied in strides of 64, coalesced on both sides; a sampled pair has lane
//     k draw for slot k, and without replacement Floyd's chain is resolved in at most f - 1 steps of one broadcast and one ballot (slot k
//     falls back to j iff a lane below it holds its draw), no LDS; then one scattered col load and coalesced stores per lane.  The
//     slots [M, cap) are filled by the same launch.
// A whole-row run on a hub (fan-out -1) is copied by its wave alone: known limit, in_edges is the op for whole neighbourhoods.
// Bound: the scattered type bytes and col entries, a 64-byte sector each.  No floating point, no MFMA.
#include "legion_core.h"
#include "etype_rule.h"

namespace lg {

#define LG_ETYPE_WAVES (LG_ETYPE_THREADS / 64)
#define LG_ETYPE_NONE 64               // no sample: past every lane number

// LDS written by some lanes of a wave is read by others of it
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t wave_bcast(int64_t v, int32_t from)
{
    const uint32_t lo = __builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v & 0xFFFFFFFFull), from);
    const uint32_t hi = __builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v >> 32), from);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the wave's row of this trip, the same in every lane
__device__ __forceinline__ int32_t first_row() { return (int32_t)blockIdx.x * LG_ETYPE_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6)); }

// (vertex, start, D) of rows[i]: D = 0 for a row outside the graph, for which nothing is read
__device__ __forceinline__ void row_extent(const EtypeRows& g, int32_t i, int32_t& r, int64_t& lo, int64_t& D)
{
    r = g.rows[i];
    lo = 0;
    D = 0;
    if (r >= 0 && r < g.node_num) {
        lo = g.indptr[r];
        D = g.indptr[r + 1] - lo;
        if (D < 0) D = 0;
    }
}

// Segment `lane` of the row [lo, lo + D) is [b, nb), positions inside the row; lanes >= T get [D, D).  s_row: the wave's 65 words
__device__ __forceinline__ void row_segments(const uint8_t* __restrict__ etype, int64_t lo, int64_t D, int32_t T, int32_t lane, int32_t* s_row,
                                             int64_t& b, int64_t& nb)
{
    b = nb = 0;
    if (D <= 0) return;                                               // (the whole wave alike)
    const int64_t step = (D + 63) >> 6;
    const int64_t at = (int64_t)lane * step;
    int32_t ty = T;                                                   // past the row: its end, recorded under T
    if (at < D) {
        ty = etype[lo + at];
        if (ty > T) ty = T;                                           // (never after legion_graph_set_edge_types; the LDS row has 65 words)
    }
    const int32_t below = __shfl_up(ty, 1);
    s_row[lane] = LG_ETYPE_NONE;
    if (lane == 0) s_row[64] = LG_ETYPE_NONE;
    wave_lds_sync();
    if (lane == 0 || ty != below) s_row[ty] = lane;
    wave_lds_sync();
    int32_t J = s_row[lane];
    const int32_t end = s_row[64];
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
        const int32_t o = __shfl_down(J, d);
        if (lane + d < 64 && o < J) J = o;
    }
    if (end < J) J = end;
    // the first entry of type >= lane lies in ((J - 1) step, J step], clipped to the row; sample J - 1 is of a lower type
    int64_t a = 0, h = 0;
    if (J > 0) {
        h = (int64_t)J * step;
        if (h > D) h = D;
        a = (int64_t)(J - 1) * step + 1;
        if (a > h) a = h;
    }
    if (lane >= T) a = h = D;
    const int32_t trips = step > 1 ? 64 - __builtin_clzll((unsigned long long)(step - 1)) : 0;      // h - a <= step - 1 < 2^trips
    for (int32_t it = 0; it < trips; it++) {
        if (a < h) {
            const int64_t mid = (a + h) >> 1;                         // a <= mid < h <= D
            if ((int32_t)etype[lo + mid] < lane) a = mid + 1; else h = mid;
        }
    }
    b = a;
    nb = __shfl_down(b, 1);
    if (lane == 63) nb = D;
    if (nb < b) nb = b;                                               // (never for sorted types)
}

__device__ __forceinline__ int32_t lane_fanout(const uint64_t* planes, int32_t lane)
{
    uint32_t v = 0;
#pragma unroll
    for (int32_t bit = 0; bit < 7; bit++) v |= (uint32_t)((planes[bit] >> lane) & 1ull) << bit;
    return (int32_t)v - 1;
}

// ------------------------------------------------------------------------------------------
// the segments alone
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ETYPE_THREADS) void etype_degrees_kernel(EtypeRows g, int64_t* __restrict__ deg)
{
    __shared__ int32_t s_rows[LG_ETYPE_WAVES][65];
    const int32_t lane = threadIdx.x & 63;
    int32_t* s_row = s_rows[threadIdx.x >> 6];
    for (int32_t i = first_row(); i < g.n; i += (int32_t)gridDim.x * LG_ETYPE_WAVES) {
        int32_t r;
        int64_t lo, D, b, nb;
        row_extent(g, i, r, lo, D);
        row_segments(g.etype, lo, D, g.num_types, lane, s_row, b, nb);
        if (lane < g.num_types) deg[(int64_t)i * g.num_types + lane] = nb - b;
    }
}

// ------------------------------------------------------------------------------------------
// the count pass
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ETYPE_THREADS) void etype_count_kernel(EtypeSampleParams p)
{
    __shared__ int32_t s_rows[LG_ETYPE_WAVES][65];
    const int32_t lane = threadIdx.x & 63;
    int32_t* s_row = s_rows[threadIdx.x >> 6];
    const int32_t f = lane_fanout(p.planes, lane);
    for (int32_t i = first_row(); i < p.g.n; i += (int32_t)gridDim.x * LG_ETYPE_WAVES) {
        int32_t r;
        int64_t lo, D, b, nb;
        row_extent(p.g, i, r, lo, D);
        row_segments(p.g.etype, lo, D, p.g.num_types, lane, s_row, b, nb);
        int64_t s = etype_slots(nb - b, f, p.replace);
#pragma unroll
        for (int32_t d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
        if (lane == 0) p.offsets[i] = s;
    }
}

// ------------------------------------------------------------------------------------------
// the write pass
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_slot(const EtypeSampleParams& p, int64_t q, int32_t i, int64_t e, int32_t t)
{
    if (q < 0 || q >= p.cap) return;
    p.dst[q] = i;
    p.src[q] = p.g.col[e];
    if (p.eid) p.eid[q] = e;
    if (p.etype_out) p.etype_out[q] = (uint8_t)t;
}

__global__ __launch_bounds__(LG_ETYPE_THREADS) void etype_edges_kernel(EtypeSampleParams p)
{
    __shared__ int32_t s_rows[LG_ETYPE_WAVES][65];
    const int32_t lane = threadIdx.x & 63;
    int32_t* s_row = s_rows[threadIdx.x >> 6];
    const int32_t f = lane_fanout(p.planes, lane);
    for (int32_t i = first_row(); i < p.g.n; i += (int32_t)gridDim.x * LG_ETYPE_WAVES) {
        int32_t r;
        int64_t lo, D, b, nb;
        row_extent(p.g, i, r, lo, D);
        row_segments(p.g.etype, lo, D, p.g.num_types, lane, s_row, b, nb);
        const int64_t Dt = nb - b;
        const int64_t s = etype_slots(Dt, f, p.replace);
        int64_t upto = s;                                             // the inclusive prefix sum over the lanes
#pragma unroll
        for (int32_t d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(upto, d);
            if (lane >= d) upto += o;
        }
        const int64_t row_base = p.offsets[i];
        unsigned long long todo = __ballot(s > 0);
        while (todo != 0ull) {
            const int32_t t = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int64_t seg = lo + wave_bcast(b, t), Ds = wave_bcast(Dt, t), slots = wave_bcast(s, t);
            const int64_t base = row_base + wave_bcast(upto - s, t);
            if (slots == Ds) {                                        // taken whole, in CSR order
                for (int64_t k0 = 0; k0 < slots; k0 += 64) {
                    const int64_t k = k0 + lane;
                    if (k < slots) store_slot(p, base + k, i, seg + k, t);
                }
                continue;
            }
            const int32_t ft = (int32_t)slots;                        // the pair's fan-out, 1 .. 64, below Ds
            const bool mine = lane < ft;
            int64_t pick = -1;
            if (p.replace != 0) {
                if (mine) pick = (int64_t)etype_draw(p.key, r, t, lane, (uint64_t)Ds);
            } else {
                const int64_t j = etype_floyd_j(Ds, ft, lane);
                const int64_t c = mine ? (int64_t)etype_draw(p.key, r, t, lane, (uint64_t)(j + 1)) : -1;
                pick = c;
                // slot k's pick is final after step k: the lanes below k hold theirs, and j is above every earlier pick
                for (int32_t k = 1; k < ft; k++) {
                    const int64_t ck = wave_bcast(c, k);
                    if (__ballot(lane < k && pick == ck) != 0ull && lane == k) pick = j;
                }
            }
            if (mine) store_slot(p, base + lane, i, seg + pick, t);   // 0 <= pick < Ds
        }
    }
    // [M, cap)
    int64_t M = p.offsets[p.g.n];
    M = M < 0 ? 0 : M > p.cap ? p.cap : M;
    for (int64_t q = M + (int64_t)blockIdx.x * LG_ETYPE_THREADS + threadIdx.x; q < p.cap; q += (int64_t)gridDim.x * LG_ETYPE_THREADS) {
        p.dst[q] = -1;
        p.src[q] = -1;
        if (p.eid) p.eid[q] = -1;
        if (p.etype_out) p.etype_out[q] = 255;
    }
}

static int32_t etype_grid(int32_t n)
{
    const int32_t grid = (n + LG_ETYPE_WAVES - 1) / LG_ETYPE_WAVES;
    return grid > LG_ETYPE_GRID ? LG_ETYPE_GRID : grid < 1 ? 1 : grid;
}

// the arguments are the caller's to check (legion_etype_degrees)
void launch_etype_degrees(hipStream_t s, const EtypeRows& g, int64_t* deg)
{
    if (g.n <= 0) return;
    etype_degrees_kernel<<<etype_grid(g.n), LG_ETYPE_THREADS, 0, s>>>(g, deg);
    hipCheckError();
}

// the arguments are the caller's to check (legion_etype_sample_count); n == 0: the scan alone writes offsets[0] = 0
void launch_etype_count(hipStream_t s, const EtypeSampleParams& p, void* scratch, int64_t n_tiles)
{
    if (p.g.n > 0) etype_count_kernel<<<etype_grid(p.g.n), LG_ETYPE_THREADS, 0, s>>>(p);
    hipCheckError();
    launch_scan_int64(s, p.offsets, p.g.n, static_cast<int64_t*>(scratch), (int32_t)n_tiles, false, p.offsets + p.g.n, nullptr);
}

// the arguments are the caller's to check (legion_etype_sample_edges)
void launch_etype_edges(hipStream_t s, const EtypeSampleParams& p)
{
    if (p.cap <= 0) return;
    etype_edges_kernel<<<etype_grid(p.g.n), LG_ETYPE_THREADS, 0, s>>>(p);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// Are the types legal and sorted inside the rows?  One coalesced pass, no thread walks a row: the entries of type >= T, the adjacent
// pairs of the whole array that decrease, and those of them that lie across a row's first entry (position indptr[v] of a row with
// entries, past position 0).  The last two equal: no pair inside a row decreases (etype_set_verdict).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_wave_sum(unsigned long long c, unsigned long long* to)
{
    for (int32_t off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(to, c);
}

__global__ __launch_bounds__(256) void etype_check_kernel(const int64_t* __restrict__ indptr, const uint8_t* __restrict__ etype, int32_t n_rows,
                                                          int64_t num_edges, int32_t num_types, unsigned long long* counts)
{
    unsigned long long range = 0, descents = 0, starts = 0;
    const int64_t most = num_edges > n_rows ? num_edges : (int64_t)n_rows;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < most; x += (int64_t)gridDim.x * 256) {
        if (x < num_edges) {
            const int32_t ty = etype[x];
            range += ty >= num_types;
            if (x > 0) descents += (int32_t)etype[x - 1] > ty;
        }
        if (x < n_rows) {
            const int64_t s = indptr[x], e = indptr[x + 1];
            if (e > s && s > 0 && s < num_edges) starts += etype[s - 1] > etype[s];
        }
    }
    add_wave_sum(range, counts);
    add_wave_sum(descents, counts + 1);
    add_wave_sum(starts, counts + 2);
}

void launch_etype_check(hipStream_t s, const int64_t* indptr, const uint8_t* etype, int32_t n_rows, int64_t num_edges, int32_t num_types,
                        unsigned long long* counts)
{
    if (num_edges < 1) return;
    const int64_t most = num_edges > n_rows ? num_edges : (int64_t)n_rows;
    const int64_t blocks = (most + 255) / 256;
    etype_check_kernel<<<(uint32_t)(blocks < 4096 ? blocks : 4096), 256, 0, s>>>(indptr, etype, n_rows, num_edges, num_types, counts);
    hipCheckError();
}

}  // namespace lg
