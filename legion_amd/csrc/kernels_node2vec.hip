// kernels_node2vec.hip -- node2vec walks over the full CSR for gfx950 (CDNA4, wave64): DGL's dgl.sampling.node2vec_random_walk, and
// the count that tells whether the graph's rows are sorted (what the walk's membership search needs).
//
// The rule is the contract in include/legion_hip.h (legion_node2vec_walk): a step from v draws candidates as legion_random_walk draws
// its step and accepts one with probability wt / Mx, wt = 1/p for the vertex t the walk came from, 1 for a neighbour of t, 1/q for
// any other vertex; the first step and the max_tries-th try accept unconditionally.  The layout is the walk's (kernels_walk.hip,
// DESIGN.md 4.11) and the tile is the same code (WalkTile, walk_step.h).  What the rejection loop adds:
//   * the loop is FLAT: within a chunk a lane iterates over tries, not steps, and its position k in the chunk is lane state -- a lane
//     on try 3 of step 5 runs beside a lane on try 0 of step 7, and lanes meet only at the chunk's barrier.  A step-synchronous loop
//     pays the slowest lane's tries at every step; this one pays the largest per-lane SUM of tries over a chunk, which concentrates.
//     An iteration ends a step (k advances) or rejects a candidate (i advances, i < max_tries), so the loop runs at most
//     chunk * max_tries times, and it carries that bound.  An ended lane writes its -1s, one position an iteration, and idles;
//   * nothing is reloaded per try: the row {s, D} (and its total T) is loaded at a step's first try, the previous row {st, Dt} is the
//     last step's, kept in registers;
//   * no table look-up after a step's first draw: x_{i+1} = x_i * 48271^(2^23) and y_i = x_i * 48271^(2^22) (mod 2^31 - 1), both
//     factors compile-time constants of make_pow_tables() (kPow23, kPow22: walk_step.h);
//   * decide before searching: a candidate u != t has weight 1 or 1/q.  ry * Mx below the smaller accepts in either class, at or above
//     the larger rejects in either class; only in between does the search of t's row run (row_has).  With q == 1 it never runs.
//     u == t has one weight: no search.  No result changes.
// Bound: the part's rate of random requests at eight workgroups per CU (five with edge ids), as for the walk; no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"

namespace lg {

template <bool WEIGHTED, bool EIDS>
__global__ __launch_bounds__(LG_WALK_THREADS, 8) void node2vec_walk_kernel(Node2vecParams q)
{
    using Tile = WalkTile<EIDS>;
    __shared__ int32_t s_trace[Tile::TRACE];
    __shared__ int64_t s_eid[Tile::EID];
    Tile tile{s_trace, s_eid};
    const WalkParams& p = q.walk;
    for (int64_t tl = blockIdx.x; tl < walk_tiles(p.num_walks); tl += gridDim.x) {
        // the walk's state, in registers across tries, steps and chunks
        int32_t v;                                        // the lane's walk: where it is, and n + 1 of its next draw index n
        uint32_t n1;
        tile.begin(p, tl, v, n1);
        int32_t t = -1;                                   // the vertex before v, and its row {st, Dt}: set by the first accepted step
        int64_t s = 0, st = 0;
        int32_t D = 0, Dt = 0;
        float T = 0.0f;
        uint32_t x = 0;                                   // the candidate draw of try i
        int32_t i = 0;
        for (int32_t p0 = 0; p0 < Tile::row_len(p); p0 += Tile::CHUNK) {
            const int32_t cw = Tile::width(p, p0);
            int32_t k = 0;                                // the lane's position in the chunk
            // one position done: val at k (with its edge id), on to the next step's first try
            auto emit = [&](int32_t val, int64_t eid) {
                tile.stage(k, val, eid);
                k++;
                n1++;
                i = 0;
            };
            if (p0 == 0) {                                // position 0 is the seed, copied as given: no step, no draw index
                tile.stage(0, v, -1);
                k = 1;
            }
            const int32_t bound = cw * q.max_tries;
            for (int32_t it = 0; it < bound && k < cw; it++) {
                if ((uint32_t)v >= (uint32_t)p.node_num) { v = -1; emit(-1, -1); continue; }      // 1. ended (or a bad seed): before any load
                if (i == 0) {                             // 2. a step's first try: its row, once
                    if (!walk_row<WEIGHTED>(p, v, s, D, T)) { v = -1; emit(-1, -1); continue; }
                    x = minstd_pow(n1);
                }
                const int32_t pick = walk_candidate<WEIGHTED>(p, s, D, T, x);                      // 3. the candidate
                const int32_t u = p.col[s + pick];
                if (u < 0) { v = -1; emit(-1, -1); continue; }                                     // a dead entry ends the walk at once
                bool accept = p0 + k == 1 || i == q.max_tries - 1;                                 // the first step; the last try
                if (!accept) {
                    const double z = unit_draw(mulmod31(x, kPow22)) * q.mx;
                    if (z < (u == t ? q.a : q.lo)) accept = true;                                  // below the weight of either class u can be in
                    else if (u != t && z < q.hi)                                                   // between the two: is u in t's row?
                        accept = z < (row_has(p.col + st, Dt, u) ? 1.0 : q.b);                     // (st + Dt <= E: probes inside col)
                }
                if (accept) {                             // 4.
                    t = v; st = s; Dt = D;
                    v = u;
                    emit(u, s + pick);
                } else {
                    x = mulmod31(x, kPow23);
                    i++;
                }
            }
            tile.flush(p, p0, cw);
        }
    }
}

// the arguments are the caller's to check (legion_node2vec_walk): this only picks the instance
void launch_node2vec_walk(hipStream_t s, const Node2vecParams& q)
{
    if (q.walk.num_walks <= 0) return;
    const dim3 grid = walk_grid(q.walk.num_walks);
    const bool weighted = q.walk.edge_cdf != nullptr, eids = q.walk.edge_ids != nullptr;
    if (weighted) { if (eids) node2vec_walk_kernel<true, true><<<grid, LG_WALK_THREADS, 0, s>>>(q); else node2vec_walk_kernel<true, false><<<grid, LG_WALK_THREADS, 0, s>>>(q); }
    else          { if (eids) node2vec_walk_kernel<false, true><<<grid, LG_WALK_THREADS, 0, s>>>(q); else node2vec_walk_kernel<false, false><<<grid, LG_WALK_THREADS, 0, s>>>(q); }
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// Are the rows sorted?  Two coalesced counts, no thread walks a row: the adjacent pairs of the whole column array that decrease, and
// those of them that lie across a row boundary (position indptr[v] of a row with entries, past position 0).  Equal counts: no pair
// inside a row decreases.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_wave_count(unsigned long long c, unsigned long long* to)
{
    for (int32_t off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(to, c);
}

__global__ __launch_bounds__(256) void edge_inversions_kernel(const int32_t* col, int64_t num_edges, unsigned long long* counts)
{
    unsigned long long c = 0;
    for (int64_t e = 1 + (int64_t)blockIdx.x * 256 + threadIdx.x; e < num_edges; e += (int64_t)gridDim.x * 256) c += col[e - 1] > col[e];
    add_wave_count(c, counts);
}

__global__ __launch_bounds__(256) void boundary_inversions_kernel(const int64_t* indptr, const int32_t* col, int32_t n_rows, int64_t num_edges,
                                                                   unsigned long long* counts)
{
    unsigned long long c = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_rows; v += (int64_t)gridDim.x * 256) {
        const int64_t s = indptr[v], e = indptr[v + 1];
        if (e > s && s > 0 && s < num_edges) c += col[s - 1] > col[s];
    }
    add_wave_count(c, counts + 1);
}

void launch_row_inversion_counts(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t n_rows, int64_t num_edges,
                                 unsigned long long* counts)
{
    if (num_edges < 2 || n_rows < 1) return;
    const int64_t eb = (num_edges + 255) / 256, rb = ((int64_t)n_rows + 255) / 256;
    edge_inversions_kernel<<<dim3((uint32_t)(eb < 2048 ? eb : 2048)), 256, 0, s>>>(col, num_edges, counts);
    boundary_inversions_kernel<<<dim3((uint32_t)(rb < 2048 ? rb : 2048)), 256, 0, s>>>(indptr, col, n_rows, num_edges, counts);
    hipCheckError();
}

}  // namespace lg
