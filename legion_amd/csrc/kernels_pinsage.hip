// kernels_pinsage.hip -- PinSAGE's neighbour sampler for gfx950 (CDNA4, wave64): DGL's RandomWalkNeighborSampler / PinSAGESampler on a
// homogeneous graph.  R walks of T steps per seed, the visited vertices counted, the k most visited out -- one launch, no traces.
//
// The rule is the contract in include/legion_hip.h (legion_pinsage_neighbors).  The walks are those of kernels_walk.hip, step by step
// (walk_step.h), except that a walk's first step takes no restart draw.
//
// A workgroup of 256 lanes takes a tile of S consecutive seeds; the grid strides over tiles.  A seed owns a segment of VPAD visit slots
// in LDS, VPAD = R * T rounded up to one of 32 / 64 / 256 / 1024, and S = 2048 / VPAD (64 / 32 / 8 / 2): two int32 arrays of 2 048
// entries and their padding, 18 KiB, which keeps eight workgroups per CU beside at most 64 VGPRs -- the occupancy of the walk kernel,
// for the same reason: the walk phase is a chain of dependent random loads and its rate comes from walks in flight.
//   1. walk: the tile's S * R walks flat over the lanes (lane t takes walks t, t + 256, ...: R = 1 does not idle 255 lanes of 256);
//      visit j of walk r lands in s_vis[seed][r * T + j - 1].  Slots of ended steps, padding and seeds past the last keep the
//      INT32_MAX they were filled with.
//   2. sort: every segment at once, bitonic by vertex id, ascending -- the sentinel sorts last.  A lane holds eight entries in
//      registers per pass over LDS, which covers three stages of a merge (strides 4 j, 2 j, j: the entries {base + m j}, m < 8); the
//      merges of runs of 2, 4 and 8 are one pass.  1 024 entries take 20 passes, not 55 stages; 32 take 5, not 15.  A wave's cubes
//      lie inside entries [512 w, 512 w + 512), so for VPAD <= 256 a segment never leaves its wave and the passes need no workgroup
//      barrier: LDS operations of one wave execute in order, and a wavefront fence keeps the compiler from reordering them.
//      Entry i lives at i + 8 (i >> 6): a pass at j = 8 reads, per instruction, entries that differ in bits 0-2 and 6-8, which
//      without the padding share eight banks of 32; with it the passes at j = 8 and j = 64 are conflict-free, the one- and two-stage
//      passes at the top of a merge 2-way, and the last pass of a merge (j = 1) is two 16-byte reads and writes per lane.
//   3. count: an element that differs from its left neighbour heads a run; its length is an upper-bound search to the right, at most
//      log2(VPAD) probes.  The head at sorted position q with count c gets the key (1024 - c) << 10 | q: ascending in the key is
//      count descending, then position -- that is vertex id -- ascending.  Everything else gets INT32_MAX.
//   4. sort the keys the same way.
//   5. out: lanes take the tile's (seed, m) slots flat, which are consecutive in both outputs; slot m < VPAD with a key gives
//      {s_vis[seed][q], c}, any other {-1, 0}.
// The second array is what a total order by (count, id) costs: one 32-bit key cannot hold 11 bits of count beside 31 of id, but it can
// hold the id's rank (10 bits), and the id stays where the first sort left it.  One array of 4 096 slots and a packed 64-bit key
// would need 32 KiB for the second sort: five workgroups per CU.
// Bound: the walk phase by the part's rate of random requests, as kernels_walk.hip; the sorts by LDS issue and the VALU's min / max
// (DESIGN.md 4.12 has the measured split).  No MFMA.
#include "legion_core.h"
#include "draw_rule.h"
#include "walk_step.h"

namespace lg {

#define LG_PINSAGE_THREADS 256
#define LG_PINSAGE_SLOTS 2048        // visit slots of a tile: S * VPAD
#define LG_PINSAGE_EMPTY 0x7FFFFFFF  // no vertex (ids are below node_num <= INT32_MAX) and no key (keys are below 2^20)

static_assert(LEGION_PINSAGE_MAX_VISITS == 1024, "the key holds 1024 - count and a position in 10 bits each");
static_assert(LG_PINSAGE_SLOTS == 8 * LG_PINSAGE_THREADS, "a lane owns eight entries of a tile");

// between two steps that exchange data inside segments: wave-wide where a segment stays inside a wave, else the workgroup's barrier
template <bool WAVE_LOCAL>
__device__ __forceinline__ void segment_sync()
{
    if (WAVE_LOCAL) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// where entry i of a tile's array lives: eight entries of padding after every 64, so that entries whose indices differ in bits 6 .. 8
// alone fall in distinct banks (merge_group's reads at strides 8 .. 32)
__device__ __forceinline__ int32_t lds_at(int32_t i) { return i + ((i >> 6) << 3); }
#define LG_PINSAGE_LDS_ENTRIES (LG_PINSAGE_SLOTS + (LG_PINSAGE_SLOTS >> 6) * 8)

__device__ __forceinline__ void order_pair(int32_t& x, int32_t& y, bool up)
{
    const int32_t mn = min(x, y), mx = max(x, y);
    x = up ? mn : mx;
    y = up ? mx : mn;
}

// The first three merges (k = 2, 4, 8) of every aligned run of eight entries, in registers: lane t of wave w owns entries
// [512 w + 8 t, 512 w + 8 t + 8).  Afterwards the runs of eight alternate ascending / descending inside a segment.
template <int VPAD>
__device__ __forceinline__ void sort_eights(int32_t* a, int32_t tid)
{
    const int32_t base = tid * 8;
    const bool up8 = (base & 8 & (VPAD - 1)) == 0;
    int32_t x[8];
#pragma unroll
    for (int32_t m = 0; m < 8; m++) x[m] = a[lds_at(base + m)];
#pragma unroll
    for (int32_t lk = 1; lk <= 3; lk++)                                      // k = 1 << lk, j = 1 << lj (counted, so that the loops unroll
#pragma unroll                                                               // and x stays in registers)
        for (int32_t lj = lk - 1; lj >= 0; lj--)
#pragma unroll
            for (int32_t m = 0; m < 8; m++)
                if (!(m & (1 << lj))) order_pair(x[m], x[m | (1 << lj)], lk < 3 ? (m & (1 << lk)) == 0 : up8);
#pragma unroll
    for (int32_t m = 0; m < 8; m++) a[lds_at(base + m)] = x[m];
}

// G consecutive stages of the merge of runs of k, strides jlow << (G - 1) .. jlow, in one pass over LDS: a lane holds 8 >> G cubes of
// 1 << G entries {base + m * jlow} in registers.  Wave w's cubes lie inside [512 w, 512 w + 512) while jlow << G <= 512.
template <int VPAD, int G>
__device__ __forceinline__ void merge_group(int32_t* a, int32_t tid, int32_t k, int32_t jlow)
{
    constexpr int32_t E = 1 << G, CUBES = 8 >> G;
    const int32_t c0 = (tid >> 6) * (64 * CUBES) + (tid & 63);
#pragma unroll
    for (int32_t c = 0; c < CUBES; c++) {
        const int32_t ci = c0 + c * 64;                                      // < 2048 / E
        const int32_t base = ((ci & ~(jlow - 1)) << G) | (ci & (jlow - 1));  // G zero bits put in at log2(jlow): base + (E - 1) jlow < 2048
        const bool up = (base & k & (VPAD - 1)) == 0;                        // (the last merge, k == VPAD, is ascending in every segment)
        int32_t x[E];
#pragma unroll
        for (int32_t m = 0; m < E; m++) x[m] = a[lds_at(base + m * jlow)];
#pragma unroll
        for (int32_t ls = G - 1; ls >= 0; ls--)
#pragma unroll
            for (int32_t m = 0; m < E; m++)
                if (!(m & (1 << ls))) order_pair(x[m], x[m | (1 << ls)], up);
#pragma unroll
        for (int32_t m = 0; m < E; m++) a[lds_at(base + m * jlow)] = x[m];
    }
}

// every aligned run of VPAD entries of a tile's array ascending: a bitonic sort, three stages to a pass over LDS
template <int VPAD, bool WAVE_LOCAL>
__device__ __forceinline__ void segment_sort(int32_t* a, int32_t tid)
{
    sort_eights<VPAD>(a, tid);
    segment_sync<WAVE_LOCAL>();
#pragma nounroll
    for (int32_t L = 4; (1 << L) <= VPAD; L++) {                             // the merge of runs of k = 1 << L: stages at bits L - 1 .. 0
        const int32_t k = 1 << L;
        int32_t top = L;
        if (L % 3 == 1) { merge_group<VPAD, 1>(a, tid, k, 1 << (L - 1)); top -= 1; segment_sync<WAVE_LOCAL>(); }
        if (L % 3 == 2) { merge_group<VPAD, 2>(a, tid, k, 1 << (L - 2)); top -= 2; segment_sync<WAVE_LOCAL>(); }
#pragma nounroll
        for (; top > 3; top -= 3) { merge_group<VPAD, 3>(a, tid, k, 1 << (top - 3)); segment_sync<WAVE_LOCAL>(); }
        merge_group<VPAD, 3>(a, tid, k, 1);                                  // (a constant stride of 1: the lane's eight entries are two 16-byte reads)
        segment_sync<WAVE_LOCAL>();
    }
}

template <int VPAD, bool WEIGHTED, bool RESTART>
__global__ __launch_bounds__(LG_PINSAGE_THREADS, 8) void pinsage_neighbors_kernel(PinsageParams p)
{
    constexpr int32_t S = LG_PINSAGE_SLOTS / VPAD;       // seeds of a tile
    constexpr bool WAVE_LOCAL = VPAD <= 256;
    __shared__ __attribute__((aligned(16))) int32_t s_vis[LG_PINSAGE_LDS_ENTRIES];      // visits; after the first sort ascending per segment
    __shared__ __attribute__((aligned(16))) int32_t s_key[LG_PINSAGE_LDS_ENTRIES];      // (1024 - count) << 10 | position of the run heads
    const int32_t tid = threadIdx.x;
    const int32_t R = p.walks_per_seed, T = p.walk.length, K = p.num_neighbors;
    const int64_t n = p.walk.num_walks;
    const int64_t n_tiles = (n + S - 1) / S;
    const int32_t elem0 = (tid >> 6) * 512 + (tid & 63); // the lane's elements: elem0 + 64 q, inside its wave's 512
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t seed0 = tile * S;
        const int32_t live = (int32_t)min((int64_t)S, n - seed0);
#pragma unroll
        for (int32_t q = 0; q < 8; q++) s_vis[lds_at(tid + q * LG_PINSAGE_THREADS)] = LG_PINSAGE_EMPTY;
        __syncthreads();
        // 1. the walks of the tile's live seeds: live * R <= S * VPAD
        for (int32_t wl = tid; wl < live * R; wl += LG_PINSAGE_THREADS) {
            const int32_t sl = wl / R, r = wl - sl * R;
            const int64_t w = (seed0 + sl) * R + r;
            int32_t v = p.walk.seeds[seed0 + sl];
            uint32_t n1 = (uint32_t)(p.walk.base + w * T) + 1u;
            const int32_t out = sl * VPAD + r * T;                           // r * T + T <= R * T <= VPAD
            int64_t eid;
            v = walk_step<WEIGHTED, false>(p.walk, v, n1++, eid);            // the first traversal has no restart
            for (int32_t j = 0; v >= 0;) {
                s_vis[lds_at(out + j)] = v;
                if (++j == T) break;
                v = walk_step<WEIGHTED, RESTART>(p.walk, v, n1++, eid);
            }
        }
        __syncthreads();
        // 2.
        segment_sort<VPAD, WAVE_LOCAL>(s_vis, tid);
        // 3. (reads s_vis inside the element's segment, writes s_key at the element)
#pragma nounroll                                                             // (unrolled, its addresses are hoisted over the walk phase and spill there)
        for (int32_t q = 0; q < 8; q++) {
            const int32_t e = elem0 + q * 64;
            const int32_t pos = e & (VPAD - 1);
            const int32_t seg = e - pos;
            const int32_t v = s_vis[lds_at(e)];
            int32_t key = LG_PINSAGE_EMPTY;
            if (v != LG_PINSAGE_EMPTY && (pos == 0 || s_vis[lds_at(e - 1)] != v)) {
                int32_t lo = pos + 1, hi = VPAD;                             // the first entry right of pos that is not v
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (s_vis[lds_at(seg + mid)] == v) lo = mid + 1; else hi = mid;
                }
                key = ((LEGION_PINSAGE_MAX_VISITS - (lo - pos)) << 10) | pos;
            }
            s_key[lds_at(e)] = key;
        }
        segment_sync<WAVE_LOCAL>();
        // 4.
        segment_sort<VPAD, WAVE_LOCAL>(s_key, tid);
        if (WAVE_LOCAL) __syncthreads();                                     // (the sort's last pass ended with the barrier otherwise)
        // 5. the tile's rows are consecutive in both outputs: live * K <= 64 * 1024
        int32_t* nb = p.neighbors + seed0 * K;
        int32_t* ct = p.counts + seed0 * K;
        for (int32_t o = tid; o < live * K; o += LG_PINSAGE_THREADS) {
            const int32_t sl = o / K, m = o - sl * K;
            int32_t u = -1, c = 0;
            if (m < VPAD) {
                const int32_t key = s_key[lds_at(sl * VPAD + m)];
                if (key != LG_PINSAGE_EMPTY) {
                    u = s_vis[lds_at(sl * VPAD + (key & 1023))];
                    c = LEGION_PINSAGE_MAX_VISITS - (key >> 10);
                }
            }
            nb[o] = u;
            ct[o] = c;
        }
        __syncthreads();                                                     // (the next tile's fill overwrites what these lanes read)
    }
}

template <int VPAD>
static void launch_pinsage_class(hipStream_t s, const PinsageParams& p)
{
    constexpr int64_t S = LG_PINSAGE_SLOTS / VPAD;
    const int64_t n_tiles = ((int64_t)p.walk.num_walks + S - 1) / S;
    const dim3 grid((uint32_t)(n_tiles < LG_WALK_MAX_WG ? n_tiles : LG_WALK_MAX_WG));
    const bool weighted = p.walk.edge_cdf != nullptr, restart = p.walk.restart_prob > 0.0f;
    if (weighted) {
        if (restart) pinsage_neighbors_kernel<VPAD, true, true><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
        else pinsage_neighbors_kernel<VPAD, true, false><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
    } else {
        if (restart) pinsage_neighbors_kernel<VPAD, false, true><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
        else pinsage_neighbors_kernel<VPAD, false, false><<<grid, LG_PINSAGE_THREADS, 0, s>>>(p);
    }
}

// the arguments are the caller's to check (legion_pinsage_neighbors): this only picks the instance by R * T
void launch_pinsage_neighbors(hipStream_t s, const PinsageParams& p)
{
    if (p.walk.num_walks <= 0) return;
    const int32_t visits = p.walks_per_seed * p.walk.length;                 // <= LEGION_PINSAGE_MAX_VISITS
    if (visits <= 32) launch_pinsage_class<32>(s, p);
    else if (visits <= 64) launch_pinsage_class<64>(s, p);
    else if (visits <= 256) launch_pinsage_class<256>(s, p);
    else launch_pinsage_class<1024>(s, p);
    hipCheckError();
}

}  // namespace lg
