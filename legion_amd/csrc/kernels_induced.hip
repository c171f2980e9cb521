// kernels_induced.hip -- a vertex set and the subgraph it induces (DGL's node_subgraph; the ops behind ClusterGCN, GraphSAINT and
// ShaDow-GNN) for gfx950 (CDNA4, wave64).  The set is the id table of node_set.h (its carve, its clear and its probe) as an object of
// its own.  The edges are the kept-slot compaction (kept_slots.h: count, scan, write) with the predicate "the source is a member of the
// set" and the member's position in the set as the written source.  The rules are the contracts in include/legion_hip.h, their text
// induced_rule.h.  The layout is in_edges': 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides, every offset 64
// bits wide, no workgroup waits for another and every loop carries its bound.
//   * clear    the table's 2 S words all-ones and the distinct count 0, one launch (captured and ordered with the rest);
//   * insert   a lane per node: at most S probes of atomicCAS, then atomicMin on first.  The one inserter that saw the empty key counts
//              the key: a ballot per wave, one atomicAdd per wave that claimed any;
//   * lookup   a grid-stride lane per id, node_set_positions<1>;
//   * count    after a tile resolves, a lane's four probe chains run interleaved (node_set_positions<4>: each probe step is a dependent
//              load -- of four keys at once where the table starts at a 16-byte boundary -- and four are in flight per lane);
//   * write    resolves and probes again.  For a small set on a large graph most tiles keep nothing and are skipped.  66 VGPRs: seven
//              waves per SIMD (at eight the four key groups spilled);
//   * offsets  a lane per i in [0, n]: a lower-bound search over dst[0 .. L) of at most 31 trips, one 8-byte store.
// Bound: the col reads and the probes' dependent loads (a table of at most 16 MB: the Infinity Cache holds it); no MFMA.
#include "legion_core.h"
#include "induced_rule.h"
#include "kept_slots.h"
#include "node_set.h"

namespace lg {

// ------------------------------------------------------------------------------------------
// the set
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_clear_kernel(uint32_t* table, int64_t words, int32_t* distinct)
{
    id_table_clear(table, words, distinct);
}

__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_insert_kernel(const int32_t* nodes, int32_t k, int32_t* keys, uint32_t* first,
                                                                         uint32_t mask, int32_t shift, int32_t* distinct)
{
    // the trip count is the wave's, not the lane's: every lane of a wave reaches the ballot
    for (int64_t base = (int64_t)blockIdx.x * LG_ROW_THREADS; base < k; base += (int64_t)gridDim.x * LG_ROW_THREADS) {
        const int64_t i = base + threadIdx.x;
        const int32_t id = i < k ? nodes[i] : -1;
        bool claimed = false;
        if (id >= 0) {                                                // a negative entry is a member of nothing
            uint32_t h = id_table_home(id, shift) & mask;
            for (uint32_t probe = 0; probe <= mask; probe++) {        // at most S probes; a free slot exists (S >= 2 k)
                const int32_t old = atomicCAS(keys + h, ID_TABLE_EMPTY_KEY, id);
                if (old == ID_TABLE_EMPTY_KEY || old == id) {
                    claimed = old == ID_TABLE_EMPTY_KEY;              // exactly one inserter of a key sees the empty key
                    atomicMin(first + h, (uint32_t)i);
                    break;
                }
                h = (h + 1u) & mask;
            }
        }
        const unsigned long long b = __ballot(claimed);
        if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(distinct, __popcll(b));
    }
}

__global__ __launch_bounds__(LG_ROW_THREADS) void node_set_lookup_kernel(NodeSetView s, const int32_t* ids, int64_t m, int32_t* local)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * LG_ROW_THREADS) {
        const int32_t v[1] = {ids[i]};
        int32_t pos[1];
        node_set_positions<1>(s, v, pos);
        local[i] = pos[0];
    }
}

// the arguments are the caller's to check (legion_node_set_build); set holds node_set_bytes(k) bytes
void launch_node_set_build(hipStream_t s, const int32_t* nodes, int32_t k, void* set, int32_t* distinct)
{
    const int64_t slots = node_set_slots(k);
    const IdTable t = id_table_carve(set, slots);
    node_set_clear_kernel<<<walk_grid(2 * slots), LG_ROW_THREADS, 0, s>>>(reinterpret_cast<uint32_t*>(t.keys), 2 * slots, distinct);
    if (k > 0) node_set_insert_kernel<<<walk_grid(k), LG_ROW_THREADS, 0, s>>>(nodes, k, t.keys, t.first, t.mask, t.shift, distinct);
    hipCheckError();
}

// the arguments are the caller's to check (legion_node_set_lookup)
void launch_node_set_lookup(hipStream_t s, const NodeSetView& set, const int32_t* ids, int64_t m, int32_t* local)
{
    if (m <= 0) return;
    node_set_lookup_kernel<<<walk_grid(m), LG_ROW_THREADS, 0, s>>>(set, ids, m, local);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the edges
// ------------------------------------------------------------------------------------------
// a lane's four slots and rule 3 for them
struct InducedSlots : LaneSlots {
    int32_t pos[LG_ROW_ILP];        // pos(src), -1: not kept

    // Rules 1 -- 3 for the slots of a tile: the resolution, then the membership of src (a dead entry and a slot without an entry have
    // src == -1 and are never probed for).  One barrier inside, resolve_row_slots'
    __device__ __forceinline__ void resolve(const InducedParams& p, int64_t tile, int64_t* s_off)
    {
        resolve_row_slots(p.slots, tile, s_off, *this);
        node_set_positions<LG_ROW_ILP>(p.set, src, pos);              // (src is -1 wherever e is: no entry, no probe)
    }
    __device__ __forceinline__ bool kept(int32_t j) const { return pos[j] >= 0; }
    __device__ __forceinline__ int32_t source(int32_t j) const { return pos[j]; }
};

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void induced_count_kernel(InducedParams p)
{
    kept_count_tiles<InducedSlots>(p);
}

__global__ __launch_bounds__(LG_ROW_THREADS, 7) void induced_edges_kernel(InducedParams p)
{
    kept_write_tiles<InducedSlots>(p);
}

// the arguments are the caller's to check (legion_induced_count, legion_induced_edges)
void launch_induced_count(hipStream_t s, const InducedParams& p) { launch_kept_count(s, induced_count_kernel, p); }
void launch_induced_edges(hipStream_t s, const InducedParams& p) { launch_kept_write(s, induced_edges_kernel, p); }

// ------------------------------------------------------------------------------------------
// the row pointers
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS) void dst_offsets_kernel(const int32_t* dst, int64_t cap, const int64_t* count, int32_t n, int64_t* indptr)
{
    const int64_t total = count[0];
    const int64_t L = total < 0 ? 0 : total > cap ? cap : total;      // <= 2^31 - 1
    for (int64_t i = (int64_t)blockIdx.x * LG_ROW_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * LG_ROW_THREADS) {
        int64_t lo = 0, len = L;                                      // #{ p in [0, L) : dst[p] < i }: the answer lies in [lo, lo + len]
        for (int32_t trip = 0; trip < 32 && len > 0; trip++) {        // len halves: at most 31 trips
            const int64_t half = len >> 1;
            if ((int64_t)dst[lo + half] < i) { lo += half + 1; len -= half + 1; }      // (lo + half < lo + len <= L <= cap)
            else len = half;
        }
        indptr[i] = lo;
    }
}

// the arguments are the caller's to check (legion_dst_offsets)
void launch_dst_offsets(hipStream_t s, const int32_t* dst, int64_t cap, const int64_t* count, int32_t n, int64_t* indptr)
{
    dst_offsets_kernel<<<walk_grid((int64_t)n + 1), LG_ROW_THREADS, 0, s>>>(dst, cap, count, n, indptr);
    hipCheckError();
}

}  // namespace lg
