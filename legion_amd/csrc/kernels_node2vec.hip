// kernels_node2vec.hip -- node2vec walks over the full CSR for gfx950 (CDNA4, wave64): DGL's dgl.sampling.node2vec_random_walk, and
// the count that tells whether the graph's rows are sorted (what the walk's membership search needs).
//
// The rule is the contract in include/legion_hip.h (legion_node2vec_walk): a step from v draws candidates as legion_random_walk draws
// its step and accepts one with probability wt / Mx, wt = 1/p for the vertex t the walk came from, 1 for a neighbour of t, 1/q for
// any other vertex; the first step and the max_tries-th try accept unconditionally.  The layout is the walk's (kernels_walk.hip,
// DESIGN.md 4.11): one lane per walk, 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles, trace rows
// (and edge ids) staged in LDS a chunk of positions at a time at an odd pitch and flushed as runs.  What the rejection loop adds:
//   * the loop is FLAT: within a chunk a lane iterates over tries, not steps, and its position k in the chunk is lane state -- a lane
//     on try 3 of step 5 runs beside a lane on try 0 of step 7, and lanes meet only at the chunk's barrier.  A step-synchronous loop
//     pays the slowest lane's tries at every step; this one pays the largest per-lane SUM of tries over a chunk, which concentrates.
//     An iteration ends a step (k advances) or rejects a candidate (i advances, i < max_tries), so the loop runs at most
//     chunk * max_tries times, and it carries that bound.  An ended lane writes its -1s, one position an iteration, and idles;
//   * nothing is reloaded per try: the row {s, D} (and its total T) is loaded at a step's first try, the previous row {st, Dt} is the
//     last step's, kept in registers;
//   * no table look-up after a step's first draw: x_{i+1} = x_i * 48271^(2^23) and y_i = x_i * 48271^(2^22) (mod 2^31 - 1), both
//     factors compile-time constants of make_pow_tables();
//   * decide before searching: a candidate u != t has weight 1 or 1/q.  ry * Mx below the smaller accepts in either class, at or above
//     the larger rejects in either class; only in between does the search of t's row run (ceil(log2(Dt + 1)) dependent 4-byte
//     loads, ended early by a hit).  With q == 1 it never runs.  u == t has one weight: no search.  No result changes.
// Bound: the part's rate of random requests at eight workgroups per CU (five with edge ids), as for the walk; no MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"

namespace lg {

#define LG_N2V_THREADS 256
#define LG_N2V_MAX_WG 2048       // 256 CUs x 8 resident workgroups: every further tile is a stride of the grid

static constexpr uint32_t kPow22 = make_pow_tables().t2[1];      // 48271^(2^22): from a try's candidate draw to its accept draw
static constexpr uint32_t kPow23 = make_pow_tables().t2[2];      // 48271^(2^23): from a try's candidate draw to the next try's

template <bool WEIGHTED, bool EIDS>
__global__ __launch_bounds__(LG_N2V_THREADS, 8) void node2vec_walk_kernel(Node2vecParams q)
{
    constexpr int32_t CHUNK = EIDS ? 8 : 16;             // trace positions staged per flush (kernels_walk.hip: 8 and 5 workgroups per CU)
    constexpr int32_t PITCH = CHUNK + 1;
    __shared__ int32_t s_trace[LG_N2V_THREADS * PITCH];
    __shared__ int64_t s_eid[EIDS ? LG_N2V_THREADS * PITCH : 1];
    const WalkParams& p = q.walk;
    const int32_t tid = threadIdx.x;
    const int32_t row_len = p.length + 1;                // positions 0 .. length of a trace row
    const int64_t n_tiles = ((int64_t)p.num_walks + LG_N2V_THREADS - 1) / LG_N2V_THREADS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t w0 = tile * LG_N2V_THREADS;
        const int64_t w = w0 + tid;
        const int32_t live_rows = (int32_t)min((int64_t)LG_N2V_THREADS, (int64_t)p.num_walks - w0);
        // the walk's state, in registers across tries, steps and chunks
        int32_t v = tid < live_rows ? p.seeds[w] : -1;    // (a lane past the last walk is an ended walk: no load, no store)
        int32_t t = -1;                                   // the vertex before v, and its row {st, Dt}: set by the first accepted step
        int64_t s = 0, st = 0;
        int32_t D = 0, Dt = 0;
        float T = 0.0f;
        uint32_t x = 0;                                   // the candidate draw of try i
        int32_t i = 0;
        uint32_t n1 = (uint32_t)(p.base + w * p.length) + 1u;
        for (int32_t p0 = 0; p0 < row_len; p0 += CHUNK) {
            const int32_t cw = min(CHUNK, row_len - p0);
            int32_t k = 0;                                // the lane's position in the chunk
            // one position done: val at k (with its edge id), on to the next step's first try
            auto emit = [&](int32_t val, int64_t eid) {
                s_trace[tid * PITCH + k] = val;
                if (EIDS) s_eid[tid * PITCH + k] = eid;
                k++;
                n1++;
                i = 0;
            };
            if (p0 == 0) {                                // position 0 is the seed, copied as given: no step, no draw index
                s_trace[tid * PITCH] = v;
                if (EIDS) s_eid[tid * PITCH] = -1;
                k = 1;
            }
            const int32_t bound = cw * q.max_tries;
            for (int32_t it = 0; it < bound && k < cw; it++) {
                if ((uint32_t)v >= (uint32_t)p.node_num) { v = -1; emit(-1, -1); continue; }      // 1. ended (or a bad seed): before any load
                if (i == 0) {                             // 2. a step's first try: its row, once
                    const WalkRowPair row = *reinterpret_cast<const WalkRowPair*>(p.indptr + v);   // (v + 1 <= node_num: inside indptr)
                    s = row.s;
                    D = (int32_t)(row.e - s);
                    if (D <= 0) { v = -1; emit(-1, -1); continue; }
                    if (WEIGHTED) {
                        T = p.edge_cdf[s + D - 1];
                        if (!(T > 0.0f)) { v = -1; emit(-1, -1); continue; }
                    }
                    x = minstd_pow(n1);
                }
                int32_t pick;                             // 3. the candidate
                if (WEIGHTED) {
                    const float* c = p.edge_cdf + s;
                    const double target = weighted_target(x, T);
                    int32_t lo = 0, m = D;
                    while (m > 0) weighted_step(c[lo + (m >> 1)], target, lo, m);                  // probes lo + m / 2 < lo + m <= D
                    pick = min(lo, D - 1);
                } else {
                    pick = draw_from_x(x, D);             // r < 1: pick <= D - 1
                }
                const int32_t u = p.col[s + pick];
                if (u < 0) { v = -1; emit(-1, -1); continue; }                                     // a dead entry ends the walk at once
                bool accept = p0 + k == 1 || i == q.max_tries - 1;                                 // the first step; the last try
                if (!accept) {
                    const uint32_t y = mulmod31(x, kPow22);
                    double z = (double)(uint32_t)(y - 1u);
                    z /= 2147483646.0;
                    z *= q.mx;
                    if (z < (u == t ? q.a : q.lo)) {
                        accept = true;                    // below the weight of either class u can be in
                    } else if (u != t && z < q.hi) {      // between the two: is u in t's row?  (st + Dt <= E: probes inside col)
                        const int32_t* c = p.col + st;
                        int32_t lo = 0, m = Dt;
                        bool found = false;
                        while (m > 0) {
                            const int32_t half = m >> 1, cv = c[lo + half];
                            if (cv == u) { found = true; break; }
                            if (cv < u) { lo += half + 1; m -= half + 1; }
                            else m = half;
                        }
                        accept = z < (found ? 1.0 : q.b);
                    }
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
            __syncthreads();
            // the tile's rows x this chunk's positions, consecutive lanes on consecutive positions of a row
            for (int32_t e = tid; e < LG_N2V_THREADS * CHUNK; e += LG_N2V_THREADS) {
                const int32_t r = e / CHUNK, c = e % CHUNK;
                if (r < live_rows && c < cw) {
                    p.traces[(w0 + r) * row_len + p0 + c] = s_trace[r * PITCH + c];
                    if (EIDS && p0 + c > 0) p.edge_ids[(w0 + r) * p.length + p0 + c - 1] = s_eid[r * PITCH + c];
                }
            }
            __syncthreads();
        }
    }
}

// the arguments are the caller's to check (legion_node2vec_walk): this only picks the instance
void launch_node2vec_walk(hipStream_t s, const Node2vecParams& q)
{
    if (q.walk.num_walks <= 0) return;
    const int64_t n_tiles = ((int64_t)q.walk.num_walks + LG_N2V_THREADS - 1) / LG_N2V_THREADS;
    const dim3 grid((uint32_t)(n_tiles < LG_N2V_MAX_WG ? n_tiles : LG_N2V_MAX_WG));
    const bool weighted = q.walk.edge_cdf != nullptr, eids = q.walk.edge_ids != nullptr;
    if (weighted) { if (eids) node2vec_walk_kernel<true, true><<<grid, LG_N2V_THREADS, 0, s>>>(q); else node2vec_walk_kernel<true, false><<<grid, LG_N2V_THREADS, 0, s>>>(q); }
    else          { if (eids) node2vec_walk_kernel<false, true><<<grid, LG_N2V_THREADS, 0, s>>>(q); else node2vec_walk_kernel<false, false><<<grid, LG_N2V_THREADS, 0, s>>>(q); }
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
