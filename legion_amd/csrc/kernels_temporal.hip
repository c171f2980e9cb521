// kernels_temporal.hip -- temporal neighbour sampling (legion_graph_set_edge_times, legion_temporal_sample_count,
// legion_temporal_sample_edges; GraphBolt's temporal_sample_neighbors, PyG's NeighborLoader(time_attr=, temporal_strategy="uniform" |
// "last"), TGL's most recent k neighbours) for gfx950 (CDNA4, wave64).  The rules are the contracts in include/legion_hip.h, their text
// temporal_rule.h, which runs here on the device.
// The shape: a wave per row, grid-strided under a grid of at most LG_TEMPORAL_GRID workgroups of four waves, as kernels_etype.hip.  A
// row's candidates are its entries with time < bound; C is their number, a slot picks a RANK among them (temporal_rule.h), and the two
// classes differ only in how a rank becomes a position of the row:
//   * the sorted class (every row non-decreasing in time): the candidates are the row's first C entries, rank = position.  C is the
//     cut, found by ONE search that all 64 lanes run together: the bracket [a, h) is probed at 64 positions ceil((h - a) / 64) apart,
//     lane j loading one time; the ballot of time < bound is a prefix of ones, its popcount J says between which two probes the cut
//     lies, and the bracket shrinks to the entries between them.  One round for D <= 64, two up to 4 096, three up to 262 144, the same
//     number in every lane, no LDS (kernels_etype.hip searches for 64 boundaries at once, a lane each, and so samples one step and
//     goes on with binary steps; here there is one boundary, and the whole wave narrows it);
//   * the scan class (some row decreases): the count pass streams the row's times in coalesced strides of 64 and sums the popcounts
//     of the ballots; the write pass streams them again under a running base, and a lane whose rank lies in [base, base + cnt) of a
//     chunk takes the position of set bit rank - base of the chunk's ballot: a select-in-word by six popcount halvings, no loop over
//     bits.  A row taken whole writes each candidate at base + popc(mask & lanes below).  The loop ends once every slot is placed.
// Both count passes write C to cand[i] and the slots to offsets[i] (launch_scan_int64 turns them into offsets); both write passes
// read C back, clamped to the row, so no row is searched or counted a third time.  A lane's rank: the slot number for a row taken
// whole, C - slots + k under LAST, otherwise the draw of slot k; without replacement Floyd's chain is resolved as in
// etype_edges_kernel, in at most f - 1 steps of one broadcast and one ballot.  Then one scattered col (and time) load and coalesced
// stores per lane.  The slots [M, cap) are filled by the write launch.
// A hub of the scan class is streamed by its wave alone, and so is a whole-row copy (fan-out -1) of either class: known limit.
// Bound: the scattered probes and picks, a 64-byte sector each; in the scan class two reads of the rows' time bytes.  No floating
// point, no MFMA.
#include "legion_core.h"
#include "temporal_rule.h"

namespace lg {

#define LG_TEMPORAL_WAVES (LG_TEMPORAL_THREADS / 64)

namespace {

__device__ __forceinline__ int64_t bcast64(int64_t v, int32_t from)
{
    const uint32_t lo = __builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v & 0xFFFFFFFFull), from);
    const uint32_t hi = __builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v >> 32), from);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the wave's row of this trip, the same in every lane
__device__ __forceinline__ int32_t wave_row() { return (int32_t)blockIdx.x * LG_TEMPORAL_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6)); }

// (vertex, start, D) of rows[i]: D = 0 for a row outside the graph, for which nothing is read
__device__ __forceinline__ void row_extent(const TemporalParams& p, int32_t i, int32_t& r, int64_t& lo, int64_t& D)
{
    r = p.rows[i];
    lo = 0;
    D = 0;
    if (r >= 0 && r < p.node_num) {
        lo = p.indptr[r];
        D = p.indptr[r + 1] - lo;
        if (D < 0) D = 0;
    }
}

// The first position of the sorted row t[0 .. D) whose time is >= bound: the 64-ary search on ballots.  All of a, h, step and J are
// the same in every lane.  Before and after every round the cut lies in [a, h], every entry below a is a candidate and none from h
// on is.  Whatever the times hold (a caller that broke its promise), J is at most the number of probes below h: a and h stay in [0, D]
// and h - a falls below step every round.
__device__ __forceinline__ int64_t sorted_cut(const int64_t* __restrict__ t, int64_t D, int64_t bound, int32_t lane)
{
    int64_t a = 0, h = D;
    while (a < h) {
        const int64_t step = (h - a + 63) >> 6;
        const int64_t at = a + (int64_t)lane * step;
        const bool before = at < h && temporal_candidate(t[at], bound);
        const int32_t J = __popcll(__ballot(before));
        if (J == 0) {
            h = a;
        } else {
            const int64_t top = a + (int64_t)J * step;                // the first probe that is no candidate, or past the bracket
            a += (int64_t)(J - 1) * step + 1;                         // probe J - 1 is a candidate
            if (top < h) h = top;
        }
    }
    return a;
}

// the candidates of the row by streaming it: the scan class
__device__ __forceinline__ int64_t scanned_count(const int64_t* __restrict__ t, int64_t D, int64_t bound, int32_t lane)
{
    int64_t C = 0;
    for (int64_t p0 = 0; p0 < D; p0 += 64) {
        const int64_t at = p0 + lane;
        C += __popcll(__ballot(at < D && temporal_candidate(t[at], bound)));
    }
    return C;
}

// the position of set bit number r (from bit 0) of mask, r < popc(mask): six halvings, each a popcount of the lower half
__device__ __forceinline__ int32_t select_bit(unsigned long long mask, int32_t r)
{
    int32_t at = 0;
#pragma unroll
    for (int32_t w = 32; w > 0; w >>= 1) {
        const int32_t below = __popcll(mask & ((1ull << w) - 1ull));
        if (r >= below) {
            r -= below;
            mask >>= w;
            at += w;
        }
    }
    return at;
}

__device__ __forceinline__ void store_slot(const TemporalParams& p, int64_t q, int32_t i, int64_t e)
{
    if (q < 0 || q >= p.cap) return;
    p.dst[q] = i;
    p.src[q] = p.col[e];
    if (p.eid) p.eid[q] = e;
    if (p.time_out) p.time_out[q] = p.time[e];
}

}  // namespace

// ------------------------------------------------------------------------------------------
// the count pass
// ------------------------------------------------------------------------------------------
template <bool SORTED>
__global__ __launch_bounds__(LG_TEMPORAL_THREADS) void temporal_count_kernel(TemporalParams p)
{
    const int32_t lane = threadIdx.x & 63;
    for (int32_t i = wave_row(); i < p.n; i += (int32_t)gridDim.x * LG_TEMPORAL_WAVES) {
        int32_t r;
        int64_t lo, D;
        row_extent(p, i, r, lo, D);
        const int64_t bound = p.bounds[i];
        const int64_t C = SORTED ? sorted_cut(p.time + lo, D, bound, lane) : scanned_count(p.time + lo, D, bound, lane);
        if (lane == 0) {
            p.cand[i] = C;
            p.offsets[i] = temporal_slots(C, p.fanout, p.replace);
        }
    }
}

// ------------------------------------------------------------------------------------------
// the write pass
// ------------------------------------------------------------------------------------------
template <bool SORTED>
__global__ __launch_bounds__(LG_TEMPORAL_THREADS) void temporal_edges_kernel(TemporalParams p)
{
    const int32_t lane = threadIdx.x & 63;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    for (int32_t i = wave_row(); i < p.n; i += (int32_t)gridDim.x * LG_TEMPORAL_WAVES) {
        int32_t r;
        int64_t lo, D;
        row_extent(p, i, r, lo, D);
        int64_t C = p.cand[i];
        C = C < 0 ? 0 : C > D ? D : C;                                // (the count pass's; whatever it holds, every rank stays inside the row)
        const int64_t slots = temporal_slots(C, p.fanout, p.replace);
        if (slots <= 0) continue;                                     // (the whole wave alike)
        const int64_t base = p.offsets[i];
        const int64_t* t = p.time + lo;
        const int64_t bound = p.bounds[i];
        if (p.strategy == LEGION_TEMPORAL_LAST || slots == C) {       // the ranks [first, C), in CSR order, without a draw
            const int64_t first = temporal_last_rank(C, slots, 0);
            if (SORTED) {
                for (int64_t k0 = 0; k0 < slots; k0 += 64) {
                    const int64_t k = k0 + lane;
                    if (k < slots) store_slot(p, base + k, i, lo + first + k);
                }
            } else {
                int64_t seen = 0;
                for (int64_t p0 = 0; p0 < D && seen < C; p0 += 64) {
                    const int64_t at = p0 + lane;
                    const bool is = at < D && temporal_candidate(t[at], bound);
                    const unsigned long long mask = __ballot(is);
                    const int64_t rank = seen + __popcll(mask & lanes_below);
                    if (is && rank >= first && rank < C) store_slot(p, base + rank - first, i, lo + at);
                    seen += __popcll(mask);
                }
            }
            continue;
        }
        const int32_t f = (int32_t)slots;                             // the fan-out, 1 .. 64, below C
        const bool mine = lane < f;
        int64_t rank = -1;
        if (p.replace != 0) {
            if (mine) rank = temporal_uniform_draw(p.key, r, C, f, 1, lane);
        } else {
            const int64_t j = etype_floyd_j(C, f, lane);
            const int64_t c = mine ? temporal_uniform_draw(p.key, r, C, f, 0, lane) : -1;
            rank = c;
            // slot k's rank is final after step k: the lanes below k hold theirs, and j is above every earlier rank
            for (int32_t k = 1; k < f; k++) {
                const int64_t ck = bcast64(c, k);
                if (__ballot(lane < k && rank == ck) != 0ull && lane == k) rank = j;
            }
        }
        int64_t at = SORTED ? rank : -1;                              // 0 <= rank < C <= D
        if (!SORTED) {
            int64_t seen = 0;
            for (int64_t p0 = 0; p0 < D; p0 += 64) {
                const int64_t probe = p0 + lane;
                const unsigned long long mask = __ballot(probe < D && temporal_candidate(t[probe], bound));
                const int64_t cnt = __popcll(mask);
                if (mine && at < 0 && rank >= seen && rank < seen + cnt) at = p0 + select_bit(mask, (int32_t)(rank - seen));
                seen += cnt;
                if (__ballot(mine && at < 0) == 0ull) break;
            }
        }
        if (mine && at >= 0) store_slot(p, base + lane, i, lo + at);
    }
    // [M, cap)
    int64_t M = p.offsets[p.n];
    M = M < 0 ? 0 : M > p.cap ? p.cap : M;
    for (int64_t q = M + (int64_t)blockIdx.x * LG_TEMPORAL_THREADS + threadIdx.x; q < p.cap; q += (int64_t)gridDim.x * LG_TEMPORAL_THREADS) {
        p.dst[q] = -1;
        p.src[q] = -1;
        if (p.eid) p.eid[q] = -1;
        if (p.time_out) p.time_out[q] = -1;
    }
}

static int32_t temporal_grid(int32_t n)
{
    const int32_t grid = (n + LG_TEMPORAL_WAVES - 1) / LG_TEMPORAL_WAVES;
    return grid > LG_TEMPORAL_GRID ? LG_TEMPORAL_GRID : grid < 1 ? 1 : grid;
}

// the arguments are the caller's to check (legion_temporal_sample_count); n == 0: the scan alone writes offsets[0] = 0
void launch_temporal_count(hipStream_t s, const TemporalParams& p, void* scratch, int64_t n_tiles)
{
    if (p.n > 0) {
        if (p.sorted != 0) temporal_count_kernel<true><<<temporal_grid(p.n), LG_TEMPORAL_THREADS, 0, s>>>(p);
        else temporal_count_kernel<false><<<temporal_grid(p.n), LG_TEMPORAL_THREADS, 0, s>>>(p);
    }
    hipCheckError();
    launch_scan_int64(s, p.offsets, p.n, static_cast<int64_t*>(scratch), (int32_t)n_tiles, false, p.offsets + p.n, nullptr);
}

// the arguments are the caller's to check (legion_temporal_sample_edges)
void launch_temporal_edges(hipStream_t s, const TemporalParams& p)
{
    if (p.cap <= 0) return;
    if (p.sorted != 0) temporal_edges_kernel<true><<<temporal_grid(p.n), LG_TEMPORAL_THREADS, 0, s>>>(p);
    else temporal_edges_kernel<false><<<temporal_grid(p.n), LG_TEMPORAL_THREADS, 0, s>>>(p);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// Is every row non-decreasing in time?  One coalesced pass, no thread walks a row: the adjacent pairs of the whole array that
// decrease, and those of them that lie across a row's first entry (position indptr[v] of a row with entries, past position 0).
// The two equal: no pair inside a row decreases (temporal_sorted_verdict).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void time_check_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ time, int32_t n_rows,
                                                         int64_t num_edges, unsigned long long* counts)
{
    unsigned long long descents = 0, starts = 0;
    const int64_t most = num_edges > n_rows ? num_edges : (int64_t)n_rows;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < most; x += (int64_t)gridDim.x * 256) {
        if (x > 0 && x < num_edges) descents += time[x - 1] > time[x];
        if (x < n_rows) {
            const int64_t s = indptr[x], e = indptr[x + 1];
            if (e > s && s > 0 && s < num_edges) starts += time[s - 1] > time[s];
        }
    }
    for (int32_t off = 32; off > 0; off >>= 1) {
        descents += __shfl_down(descents, off, 64);
        starts += __shfl_down(starts, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (descents != 0) atomicAdd(counts, descents);
        if (starts != 0) atomicAdd(counts + 1, starts);
    }
}

void launch_time_check(hipStream_t s, const int64_t* indptr, const int64_t* time, int32_t n_rows, int64_t num_edges, unsigned long long* counts)
{
    if (num_edges < 1) return;
    const int64_t most = num_edges > n_rows ? num_edges : (int64_t)n_rows;
    const int64_t blocks = (most + 255) / 256;
    time_check_kernel<<<(uint32_t)(blocks < 4096 ? blocks : 4096), 256, 0, s>>>(indptr, time, n_rows, num_edges, counts);
    hipCheckError();
}

}  // namespace lg
