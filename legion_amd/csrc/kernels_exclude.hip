// kernels_exclude.hip -- seed-edge exclusion for gfx950 (CDNA4, wave64): the reverse edge id of an edge (the pairing behind DGL's
// as_edge_prediction_sampler(exclude="reverse_id")), a set of edge ids, and the filter that drops the set's members from an edge list
// (DGL's ExcludeCertainEdges after sample_neighbors).  The rules are the contracts in include/legion_hip.h (legion_reverse_edge_ids,
// legion_edge_set_build, legion_edge_set_contains, legion_edge_filter_count, legion_edge_filter_edges), their text exclude_rule.h.  The
// layout is find_edges' and in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides (walk_grid), every edge
// offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * reverse_edge_ids   ONE kernel, a lane per four edge ids, 256 apart.  First half: find_edges_kernel's interleaved upper bound over
//                        indptr gives row(e) = v beside u = col[e].  Second half: a lower-bound search of the target row for the key
//                        -- row u of the graph for v (via 0: the graph's rows are sorted), or row v of the reverse CSR for u (via 1:
//                        reverse rows are sorted by vertex, then by ascending edge id) -- the four chains again interleaved.  The first
//                        entry that is not below the key is the LEAST e' when it equals the key.  A row has up to 2^31 - 1 entries: at
//                        most 32 trips; indptr has up to 2^28 + 1: at most 29.  Bound by dependent random loads: about 2 log2 of them
//                        per id in a chain, four chains in flight per lane; no arithmetic to speak of;
//   * set clear          the table's S int64 keys all-ones, one launch (captured and ordered with the rest);
//   * set insert         a lane per id: at most S probes of a 64-bit atomicCAS from the id's home slot (S >= 2 k: a free slot exists).
//                        Which slot a key lands in depends on arrival order; membership does not;
//   * set contains       a grid-stride lane per id, edge_set_members<1>;
//   * filter count       the kept-slot compaction (kept_slots.h) over a list in place of a row expansion: a tile's 1 024 triples, four
//                        per lane, 256 apart, and their four probe chains interleaved (edge_set_members<4>);
//   * filter write       loads and probes again; a tile that keeps nothing is skipped, the tail [K, cap) is filled with -1.
// Neither a key nor a hash is ever cut to 32 bits: edge ids pass 2^32.
// Bound: the dependent random loads of the searches and the probes (a set of at most 32 MB: the Infinity Cache holds it); no MFMA.
#include "legion_core.h"
#include "exclude_rule.h"
#include "kept_slots.h"

namespace lg {

#define LG_EXCLUDE_THREADS 256
#define LG_REVERSE_IDS_ILP 4      // edge ids per lane, searched for at once: find_edges' choice

static_assert(LG_EXCLUDE_THREADS == LG_WALK_THREADS && LG_EXCLUDE_THREADS == LG_ROW_THREADS, "the grids below are walk_grid's: a tile of 256 outputs, the walks' cap");

// ------------------------------------------------------------------------------------------
// reverse edge ids
// ------------------------------------------------------------------------------------------
// a tile is 256 x ILP edge ids; a lane's ILP ids lie 256 apart, so consecutive lanes read and write consecutive entries
__global__ __launch_bounds__(LG_EXCLUDE_THREADS, 8) void reverse_edge_ids_kernel(ReverseIdsParams p)
{
    constexpr int32_t ILP = LG_REVERSE_IDS_ILP;
    constexpr int64_t TILE = (int64_t)LG_EXCLUDE_THREADS * ILP;
    const int64_t rows1 = (int64_t)p.node_num + 1;                    // indptr's entries
    for (int64_t i0 = (int64_t)blockIdx.x * TILE + threadIdx.x; i0 < p.n; i0 += (int64_t)gridDim.x * TILE) {
        int64_t e[ILP], lo[ILP], len[ILP];
        int32_t c[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const int64_t i = i0 + (int64_t)j * LG_EXCLUDE_THREADS;
            e[j] = i < p.n ? p.eids[i] : -1;
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) c[j] = e[j] >= 0 && e[j] < p.num_edges ? p.col[e[j]] : -1;      // else: no memory is read for e
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {                           // the range of indptr to count in; none for a dead entry or one outside the graph
            lo[j] = 0;
            len[j] = (uint32_t)c[j] < (uint32_t)p.node_num ? rows1 : 0;
        }
        bool more = true;
        for (int32_t trip = 0; more && trip < 64; trip++) {           // upper bound: lo ends at #{ v in [0, N] : indptr[v] <= e }; len halves
            more = false;
            int64_t v[ILP];
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) v[j] = p.indptr[len[j] > 0 ? lo[j] + (len[j] >> 1) : 0];      // (lo + len / 2 < lo + len <= rows1)
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) {
                if (len[j] > 0) {
                    const int64_t half = len[j] >> 1;
                    if (v[j] <= e[j]) { lo[j] += half + 1; len[j] -= half + 1; }
                    else len[j] = half;
                    more |= len[j] > 0;
                }
            }
        }
        // the target row t and the key: (u, v) in the graph, (v, u) in the reverse CSR; v = row(e) lies in [0, N) or there is no answer
        int32_t key[ILP];
        int64_t end[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const int32_t u = c[j], v = (int32_t)(lo[j] - 1);
            const bool live = (uint32_t)u < (uint32_t)p.node_num && (uint32_t)v < (uint32_t)p.node_num;
            const int32_t t = p.via ? v : u;
            key[j] = p.via ? u : v;
            lo[j] = 0;
            len[j] = 0;
            if (live) {
                const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.t_indptr + t);      // (t + 1 <= node_num: inside t_indptr)
                lo[j] = row.s;
                len[j] = row.e > row.s ? row.e - row.s : 0;
            }
            end[j] = lo[j] + len[j];
        }
        more = true;
        for (int32_t trip = 0; more && trip < 64; trip++) {           // lower bound: lo ends at the first entry of the row not below the key
            more = false;
            int32_t w[ILP];
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) w[j] = len[j] > 0 ? p.t_col[lo[j] + (len[j] >> 1)] : 0;      // (inside the row)
#pragma unroll
            for (int32_t j = 0; j < ILP; j++) {
                if (len[j] > 0) {
                    const int64_t half = len[j] >> 1;
                    if (w[j] < key[j]) { lo[j] += half + 1; len[j] -= half + 1; }
                    else len[j] = half;
                    more |= len[j] > 0;
                }
            }
        }
        int32_t at[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) at[j] = lo[j] < end[j] ? p.t_col[lo[j]] : -1;                   // (an empty range: end == lo)
        int64_t r[ILP];
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const bool hit = lo[j] < end[j] && at[j] == key[j];
            r[j] = !hit ? -1 : p.via ? p.t_eid[lo[j]] : lo[j];
        }
#pragma unroll
        for (int32_t j = 0; j < ILP; j++) {
            const int64_t i = i0 + (int64_t)j * LG_EXCLUDE_THREADS;
            if (i < p.n) p.out[i] = r[j];
        }
    }
}

// the arguments are the caller's to check (legion_reverse_edge_ids)
void launch_reverse_edge_ids(hipStream_t s, const ReverseIdsParams& p)
{
    if (p.n <= 0) return;
    const dim3 grid = walk_grid((p.n + LG_REVERSE_IDS_ILP - 1) / LG_REVERSE_IDS_ILP);
    reverse_edge_ids_kernel<<<grid, LG_EXCLUDE_THREADS, 0, s>>>(p);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the set
// ------------------------------------------------------------------------------------------
// is e[j] a member?  K ids at once, their chains of dependent loads interleaved (as node_set_positions<K>).  e[j] < 0 is tested before any
// probe: -1 has the bit pattern of the empty key and never matches it.  A chain stops at the key, at an empty key, or after S probes.
// Whatever the table holds, nothing is read outside keys[0 .. S).
template <int32_t K>
__device__ __forceinline__ void edge_set_members(const EdgeSetView& s, const int64_t (&e)[K], bool (&member)[K])
{
    uint64_t h[K];
    bool open[K];
    bool more = false;
#pragma unroll
    for (int32_t j = 0; j < K; j++) {
        member[j] = false;
        open[j] = e[j] >= 0;
        h[j] = edge_set_home(e[j], s.shift) & s.mask;                 // (below S by the shift already; the mask keeps that whatever s holds)
        more |= open[j];
    }
    for (uint64_t probe = 0; more && probe <= s.mask; probe++) {      // at most S probes a chain
        more = false;
        int64_t key[K];
#pragma unroll
        for (int32_t j = 0; j < K; j++) key[j] = open[j] ? s.keys[h[j]] : EDGE_SET_EMPTY_KEY;
#pragma unroll
        for (int32_t j = 0; j < K; j++) {
            if (open[j]) {
                if (key[j] == e[j]) { member[j] = true; open[j] = false; }
                else if (key[j] == EDGE_SET_EMPTY_KEY) open[j] = false;
                else { h[j] = (h[j] + 1ull) & s.mask; more = true; }
            }
        }
    }
}

__global__ __launch_bounds__(LG_EXCLUDE_THREADS) void edge_set_clear_kernel(int64_t* keys, int64_t slots)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_EXCLUDE_THREADS + threadIdx.x; i < slots; i += (int64_t)gridDim.x * LG_EXCLUDE_THREADS)
        keys[i] = EDGE_SET_EMPTY_KEY;
}

__global__ __launch_bounds__(LG_EXCLUDE_THREADS) void edge_set_insert_kernel(const int64_t* eids, int32_t k, int64_t* keys, uint64_t mask, int32_t shift)
{
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the claim is one 64-bit compare-and-swap");
    for (int64_t i = (int64_t)blockIdx.x * LG_EXCLUDE_THREADS + threadIdx.x; i < k; i += (int64_t)gridDim.x * LG_EXCLUDE_THREADS) {
        const int64_t id = eids[i];
        if (id < 0) continue;                                         // a negative id is a member of nothing ("no reverse edge")
        uint64_t h = edge_set_home(id, shift) & mask;
        for (uint64_t probe = 0; probe <= mask; probe++) {            // at most S probes; a free slot exists (S >= 2 k)
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(keys + h), (unsigned long long)EDGE_SET_EMPTY_KEY,
                                                     (unsigned long long)id);
            if (old == (unsigned long long)EDGE_SET_EMPTY_KEY || old == (unsigned long long)id) break;
            h = (h + 1ull) & mask;
        }
    }
}

__global__ __launch_bounds__(LG_EXCLUDE_THREADS) void edge_set_contains_kernel(EdgeSetView s, const int64_t* eids, int64_t m, int32_t* out)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_EXCLUDE_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * LG_EXCLUDE_THREADS) {
        const int64_t e[1] = {eids[i]};
        bool member[1];
        edge_set_members<1>(s, e, member);
        out[i] = member[0] ? 1 : 0;
    }
}

// the arguments are the caller's to check (legion_edge_set_build); set holds edge_set_bytes(k) bytes
void launch_edge_set_build(hipStream_t s, const int64_t* eids, int32_t k, void* set)
{
    const int64_t slots = edge_set_slots(k);
    int64_t* keys = static_cast<int64_t*>(set);
    edge_set_clear_kernel<<<walk_grid(slots), LG_EXCLUDE_THREADS, 0, s>>>(keys, slots);
    if (k > 0) edge_set_insert_kernel<<<walk_grid(k), LG_EXCLUDE_THREADS, 0, s>>>(eids, k, keys, (uint64_t)(slots - 1), edge_set_shift(slots));
    hipCheckError();
}

// the arguments are the caller's to check (legion_edge_set_contains)
void launch_edge_set_contains(hipStream_t s, const EdgeSetView& set, const int64_t* eids, int64_t m, int32_t* out)
{
    if (m <= 0) return;
    edge_set_contains_kernel<<<walk_grid(m), LG_EXCLUDE_THREADS, 0, s>>>(set, eids, m, out);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the filter
// ------------------------------------------------------------------------------------------
// a lane's four triples of a tile and the rule for them: what kept_slots.h asks of an op's slots (i, e, kept, source)
struct FilterSlots {
    int64_t e[LG_ROW_ILP];          // the entry's edge id
    int32_t i[LG_ROW_ILP];          // its dst, -1: no entry (past m) or the -1 tail of a capacity call
    int32_t src[LG_ROW_ILP];        // its src, -1: a dead entry
    bool keep[LG_ROW_ILP];

    // The tile's 1 024 consecutive triples, four per lane, 256 apart, then the membership of their ids (an entry without a dst is never
    // probed for).  One barrier inside, as resolve_row_slots has: the passes of kept_slots.h reuse their LDS words behind it
    __device__ __forceinline__ void resolve(const EdgeFilterParams& p, int64_t tile, int64_t*)
    {
        __syncthreads();
        int64_t probe[LG_ROW_ILP];
        bool member[LG_ROW_ILP];
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) {
            const int64_t q = tile * LG_ROW_TILE + threadIdx.x + (int64_t)j * LG_ROW_THREADS;
            const bool live = q < p.m;
            i[j] = live ? p.dst[q] : -1;
            src[j] = live ? p.src[q] : -1;
            e[j] = live ? p.eid[q] : -1;
        }
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) probe[j] = i[j] >= 0 ? e[j] : -1;
        edge_set_members<LG_ROW_ILP>(p.set, probe, member);
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) keep[j] = i[j] >= 0 && !member[j];
    }
    __device__ __forceinline__ bool kept(int32_t j) const { return keep[j]; }
    __device__ __forceinline__ int32_t source(int32_t j) const { return src[j]; }
};

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void edge_filter_count_kernel(EdgeFilterParams p)
{
    kept_count_tiles<FilterSlots>(p);
}

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void edge_filter_edges_kernel(EdgeFilterParams p)
{
    kept_write_tiles<FilterSlots>(p);
}

// the arguments are the caller's to check (legion_edge_filter_count, legion_edge_filter_edges)
void launch_edge_filter_count(hipStream_t s, const EdgeFilterParams& p) { launch_kept_count(s, edge_filter_count_kernel, p); }
void launch_edge_filter_edges(hipStream_t s, const EdgeFilterParams& p) { launch_kept_write(s, edge_filter_edges_kernel, p); }

}  // namespace lg
