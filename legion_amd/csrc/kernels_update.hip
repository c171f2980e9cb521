// kernels_update.hip -- sparse row updates of the float32 feature table for gfx950 (CDNA4, wave64): a batch of per-row gradients with
// duplicate ids is combined per id and applied by SGD, Adagrad or Adam to the table, its cache copy and the optimizer's state
// (legion_row_update; DGL's NodeEmbedding with SparseAdagrad / SparseAdam).  The rule is the contract in include/legion_hip.h; the
// passes, the tiles and the scratch layout are update_rule.h's, the chunk rule and the lane split of a row aggregate_rule.h's.
// The layout: 256 lanes per workgroup, a grid of at most LG_WALK_MAX_WG workgroups that strides over tiles, no workgroup waits for
// another, no floating-point atomic, every loop carries its bound.
//   * keys     pair[i] = {ids[i] if live else N, i}: dead entries sort last;
//   * sort     a stable LSD radix sort of the pairs, 8 bits a pass, ping-pong between two buffers.  A pass: the histogram of every tile
//              of 1 024 consecutive pairs to int64[256][tiles], digit-major (LDS integer counters); launch_scan_int64 over those counts;
//              the scatter, whose in-tile rank is stable: a wave takes 256 consecutive pairs of the tile, 64 at a time in index order,
//              a lane's rank among its wave's equal digits is eight ballots (one per digit bit) and an mbcnt on top of the wave's
//              running count of the digit in LDS, and a lane per digit adds the waves' counts in wave order to the scanned base.
//              Stability is what makes the positions ascend inside every group of equal ids: nothing else orders them;
//   * groups   a head is the first pair of a run of equal keys below N; the heads of a tile (four consecutive pairs a lane) are summed,
//              ONE workgroup scans the tiles' sums (tile_scan.h) and leaves U, the distinct live ids, on the device; a second walk
//              writes group_id[U] and group_off[U + 1].  The host never learns U;
//   * chunks   aggregate_chunks(len) per group (0 past U) to first_chunk, scanned as the aggregation scans its own;
//   * reduce   a wave strides over chunk numbers up to the device's total and finds its group by an upper-bound search (row_slots.h).
//              It stages the chunk's positions in LDS, then is G = 64 / C groups of C lanes, 16 bytes of a gradient row a lane (one
//              float where D % 4 != 0), LG_AGG_UNROLL rows in flight, rows past 64 units in column blocks; the groups combine by the
//              butterfly.  A single-chunk group applies the optimizer in the same lanes: w and the state rows as 16-byte units, the
//              ordered epilogue, stores to the table, the cache copy and the state.  A chunk of a longer group parks a partial row;
//   * finish   a wave per chunk the groups have too many; the first of a group adds its partial rows in chunk order, a lane per
//              column, and ends in the same epilogue (update_apply, templated on the optimizer).
// This file is compiled with -ffp-contract=off (legion_amd/build.py): the header's __fmul_rn and __fadd_rn are a plain product and a
// plain sum, which the default contraction would fuse into one fused multiply-add and so change the rule's bits.
// Bound: by the m x D gradient read and the sort's 2 x passes x 8 m bytes; no MFMA.
#include "legion_core.h"
#include "update_rule.h"
#include "row_slots.h"
#include "tile_scan.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_UPD_THREADS == LG_WALK_THREADS && LG_UPD_THREADS == LG_SCAN_THREADS, "the grids are walk_grid's, the scans tile_scan.h's");
static_assert(LG_AGG_MAX_WG == LG_WALK_MAX_WG && LG_AGG_THREADS == LG_UPD_THREADS, "the reduce's grid is the aggregation's");

// the int64 scan's outer launches (kernels_in_edges.hip)
__global__ void scan_sum_kernel(const int64_t* values, int32_t n, int32_t n_sums, int64_t* sums);
__global__ void scan_apply_kernel(int64_t* values, int32_t n, int32_t n_sums, const int64_t* sums);

struct UpdatePair {
    int32_t key;                    // the id, N for a dead entry
    int32_t pos;                    // the entry's index in ids and grads
};
static_assert(sizeof(UpdatePair) == 8, "a pair is one 8-byte word of the scratch");

struct UpdateKernelParams {
    UpdateParams u;
    UpdatePair* pairs[2];
    const UpdatePair* sorted;       // the buffer the last pass wrote
    int64_t* counts;                // int64[256 x tiles]
    int32_t* tile_heads;            // int32[tiles]
    int32_t* groups;                // U
    int32_t* group_id;              // int32[m]
    int32_t* group_off;             // int32[m + 1]
    int64_t* first_chunk;           // int64[m + 1]
    float* partial;                 // float[partial_rows x D]
    int64_t partial_rows;
    int32_t tiles;
    int32_t units;                  // lane-units of a row
    int32_t lanes_log2;             // log2 C
};

// LDS written by some lanes of a wave is read by others of it
__device__ __forceinline__ void update_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------
// keys and sort
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_UPD_THREADS) void update_keys_kernel(const int32_t* ids, int32_t m, int32_t N, UpdatePair* pairs)
{
    const int64_t tiles = walk_tiles(m);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i = tile * LG_UPD_THREADS + threadIdx.x;
        if (i < m) {
            const int32_t id = ids[i];
            pairs[i] = UpdatePair{(uint32_t)id < (uint32_t)N ? id : N, (int32_t)i};
        }
    }
}

__device__ __forceinline__ int32_t update_digit(int32_t key, int32_t shift) { return (int32_t)(((uint32_t)key >> shift) & (LG_UPD_RADIX - 1)); }

__global__ __launch_bounds__(LG_UPD_THREADS) void update_histogram_kernel(const UpdatePair* in, int32_t m, int32_t tiles, int32_t shift,
                                                                          int64_t* counts)
{
    __shared__ int32_t s_hist[LG_UPD_RADIX];
    for (int32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        s_hist[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int32_t k = 0; k < LG_UPD_ILP; k++) {
            const int64_t j = (int64_t)tile * LG_UPD_TILE + k * LG_UPD_THREADS + threadIdx.x;
            if (j < m) atomicAdd(&s_hist[update_digit(in[j].key, shift)], 1);
        }
        __syncthreads();
        counts[(int64_t)threadIdx.x * tiles + tile] = s_hist[threadIdx.x];
        __syncthreads();                                              // the next tile clears s_hist
    }
}

// counts: the scanned histogram, the first slot of the tile's digit in out
__global__ __launch_bounds__(LG_UPD_THREADS) void update_scatter_kernel(const UpdatePair* in, UpdatePair* out, int32_t m, int32_t tiles,
                                                                        int32_t shift, const int64_t* counts)
{
    __shared__ int32_t s_cnt[LG_SCAN_WAVES][LG_UPD_RADIX];            // a wave's pairs of each digit so far
    __shared__ int32_t s_base[LG_SCAN_WAVES][LG_UPD_RADIX];           // the slot of a wave's first pair of each digit
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (int32_t d = lane; d < LG_UPD_RADIX; d += 64) s_cnt[wave][d] = 0;
        update_wave_sync();
        UpdatePair pr[LG_UPD_ILP];
        int32_t digit[LG_UPD_ILP], rank[LG_UPD_ILP];
        bool valid[LG_UPD_ILP];
#pragma unroll
        for (int32_t k = 0; k < LG_UPD_ILP; k++) {                    // index order: the wave, then k, then the lane
            const int64_t j = (int64_t)tile * LG_UPD_TILE + wave * LG_AGG_K + k * 64 + lane;
            valid[k] = j < m;
            pr[k] = valid[k] ? in[j] : UpdatePair{0, 0};
            digit[k] = update_digit(pr[k].key, shift);
        }
#pragma unroll
        for (int32_t k = 0; k < LG_UPD_ILP; k++) {
            uint64_t peers = __ballot(valid[k]);                      // the valid lanes whose digit is this lane's
#pragma unroll
            for (int32_t b = 0; b < LG_UPD_RADIX_BITS; b++) {
                const bool bit = (digit[k] >> b) & 1;
                const uint64_t set = __ballot(valid[k] && bit);
                peers &= bit ? set : ~set;
            }
            const int32_t below = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
            const int32_t before = s_cnt[wave][digit[k]];
            rank[k] = before + below;
            update_wave_sync();
            if (valid[k] && below == 0) s_cnt[wave][digit[k]] = before + __popcll(peers);
            update_wave_sync();
        }
        __syncthreads();
        int32_t base = (int32_t)counts[(int64_t)threadIdx.x * tiles + tile];      // a lane per digit: the waves in wave order
#pragma unroll
        for (int32_t w = 0; w < LG_SCAN_WAVES; w++) {
            s_base[w][threadIdx.x] = base;
            base += s_cnt[w][threadIdx.x];
        }
        __syncthreads();
#pragma unroll
        for (int32_t k = 0; k < LG_UPD_ILP; k++) {
            const int32_t dest = s_base[wave][digit[k]] + rank[k];
            if (valid[k] && (uint32_t)dest < (uint32_t)m) out[dest] = pr[k];      // (always inside: the counts are this buffer's)
        }
        __syncthreads();                                              // the next tile clears s_cnt
    }
}

// ------------------------------------------------------------------------------------------
// groups
// ------------------------------------------------------------------------------------------
// a lane's four consecutive pairs of a tile: their keys (N past m), which of them open a group, and the key after them
__device__ __forceinline__ int32_t update_heads(const UpdatePair* sorted, int32_t m, int32_t N, int64_t j0, int32_t (&key)[LG_UPD_ILP + 1],
                                                bool (&head)[LG_UPD_ILP])
{
    int32_t prev = (j0 > 0 && j0 - 1 < m) ? sorted[j0 - 1].key : -1, cnt = 0;      // (keys are >= 0: entry 0 opens)
#pragma unroll
    for (int32_t k = 0; k <= LG_UPD_ILP; k++) key[k] = j0 + k < m ? sorted[j0 + k].key : N;
#pragma unroll
    for (int32_t k = 0; k < LG_UPD_ILP; k++) {
        head[k] = (uint32_t)key[k] < (uint32_t)N && key[k] != prev;
        prev = key[k];
        cnt += head[k];
    }
    return cnt;
}

__global__ __launch_bounds__(LG_UPD_THREADS) void update_head_count_kernel(UpdateKernelParams p)
{
    __shared__ int32_t s_wave[LG_SCAN_WAVES];
    for (int32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        int32_t key[LG_UPD_ILP + 1];
        bool head[LG_UPD_ILP];
        const int32_t cnt = update_heads(p.sorted, p.u.m, p.u.N, (int64_t)tile * LG_UPD_TILE + threadIdx.x * LG_UPD_ILP, key, head);
        const int32_t sum = tile_sum<int32_t>(cnt, s_wave);
        if (threadIdx.x == 0) p.tile_heads[tile] = sum;
    }
}

__global__ __launch_bounds__(LG_UPD_THREADS) void update_head_scan_kernel(UpdateKernelParams p)
{
    __shared__ int32_t s_wave[LG_SCAN_WAVES];
    tile_scan_in_place<int32_t>(p.tile_heads, p.tiles, p.groups, nullptr, s_wave);
}

__global__ __launch_bounds__(LG_UPD_THREADS) void update_head_write_kernel(UpdateKernelParams p)
{
    __shared__ int32_t s_wave[LG_SCAN_WAVES];
    const int32_t m = p.u.m, N = p.u.N;
    for (int32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        int32_t key[LG_UPD_ILP + 1];
        bool head[LG_UPD_ILP];
        const int64_t j0 = (int64_t)tile * LG_UPD_TILE + threadIdx.x * LG_UPD_ILP;
        const int32_t cnt = update_heads(p.sorted, m, N, j0, key, head);
        int32_t g = p.tile_heads[tile] + tile_exclusive<int32_t>(cnt, s_wave);      // the groups opened before this lane's pairs
        if (j0 == 0 && (uint32_t)key[0] >= (uint32_t)N) p.group_off[0] = 0;         // no live entry at all: U = 0
#pragma unroll
        for (int32_t k = 0; k < LG_UPD_ILP; k++) {
            if (head[k] && g < m) {                                   // (g < U <= m)
                p.group_id[g] = key[k];
                p.group_off[g] = (int32_t)(j0 + k);
            }
            g += head[k];
            // the last live pair closes the last group: g is U here
            if ((uint32_t)key[k] < (uint32_t)N && (uint32_t)key[k + 1] >= (uint32_t)N && g <= m) p.group_off[g] = (int32_t)(j0 + k + 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// chunks and scan
// ------------------------------------------------------------------------------------------
// the entries [s, e) of group g inside the sorted pairs, whatever group_off holds
__device__ __forceinline__ void update_group(const UpdateKernelParams& p, int64_t g, int32_t& s, int32_t& e)
{
    s = min(max(p.group_off[g], 0), p.u.m);
    e = min(max(p.group_off[g + 1], s), p.u.m);
}

__global__ __launch_bounds__(LG_UPD_THREADS) void update_chunks_kernel(UpdateKernelParams p)
{
    const int64_t tiles = walk_tiles(p.u.m);
    const int32_t U = min(max(p.groups[0], 0), p.u.m);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t g = tile * LG_UPD_THREADS + threadIdx.x;
        if (g < p.u.m) {
            int32_t s = 0, e = 0;
            if (g < U) update_group(p, g, s, e);
            p.first_chunk[g] = g < U ? aggregate_chunks(e - s) : 0;
        }
    }
}

// first_chunk[0 .. m) holds the counts: they become their exclusive prefix sums and first_chunk[m] their total (the aggregation's scan)
static void update_scan(hipStream_t s, int64_t* first_chunk, int32_t m, int64_t* sums)
{
    const int32_t n_sums = (int32_t)aggregate_scan_sums(m);
    if (aggregate_scan_levels(m) < 2) {
        launch_scan_int64(s, first_chunk, m, sums, n_sums, false, first_chunk + m, nullptr);
        return;
    }
    int64_t* sums2 = sums + n_sums;
    scan_sum_kernel<<<walk_grid(m), LG_SCAN_THREADS, 0, s>>>(first_chunk, m, n_sums, sums);
    launch_scan_int64(s, sums, n_sums, sums2, (n_sums + 255) / 256, false, first_chunk + m, nullptr);
    scan_apply_kernel<<<walk_grid(m), LG_SCAN_THREADS, 0, s>>>(first_chunk, m, n_sums, sums);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// the epilogue
// ------------------------------------------------------------------------------------------
template <int32_t W>
__device__ __forceinline__ void update_load(const float* row, float (&x)[W])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    if constexpr (W == 4) {
        const f4 v = *(const LG_G f4*)row;                            // D % 4 == 0: units are 16-byte aligned
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = row[0];
    }
}

template <int32_t W>
__device__ __forceinline__ void update_store(float* row, const float (&x)[W])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    if constexpr (W == 4) *(LG_G f4*)row = f4{x[0], x[1], x[2], x[3]};
    else row[0] = x[0];
}

// The correctly rounded square root: this toolchain's __fsqrt_rn is the native instruction (3 ulp), sqrtf is the rounded one
__device__ __forceinline__ float update_sqrt_rn(float x) { return sqrtf(x); }

// Adam's running products of row v, read before and written after the row's columns
struct UpdatePow {
    float p1, p2;
};

template <int32_t OPT>
__device__ __forceinline__ UpdatePow update_pow(const UpdateParams& a, int64_t v)
{
    if constexpr (OPT != LEGION_UPDATE_ADAM) return UpdatePow{0.f, 0.f};
    else return UpdatePow{__fmul_rn(a.state_pow[2 * v], a.beta1), __fmul_rn(a.state_pow[2 * v + 1], a.beta2)};
}

// Columns [col0, col0 + W) of row v (all below D): g from the combined sum of `len` rows, then rule 5 of legion_row_update, every step
// one correctly rounded float32 operation in the rule's order.  slot: node_map[v], or -1
template <int32_t OPT, int32_t W>
__device__ __forceinline__ void update_apply(const UpdateParams& a, int64_t v, int32_t slot, int32_t col0, const float (&sum)[W], int32_t len,
                                             const UpdatePow& pw)
{
    const int64_t at = v * a.D + col0;
    float w[W], s1[W], s2[W];
    update_load<W>(a.full_table + at, w);
    if constexpr (OPT != LEGION_UPDATE_SGD) update_load<W>(a.state1 + at, s1);
    if constexpr (OPT == LEGION_UPDATE_ADAM) update_load<W>(a.state2 + at, s2);
#pragma unroll
    for (int32_t k = 0; k < W; k++) {
        const float g = a.combine == LEGION_REDUCE_MEAN ? __fdiv_rn(sum[k], (float)len) : sum[k];
        if constexpr (OPT == LEGION_UPDATE_SGD) {
            w[k] = __fsub_rn(w[k], __fmul_rn(a.lr, g));
        } else if constexpr (OPT == LEGION_UPDATE_ADAGRAD) {
            s1[k] = __fadd_rn(s1[k], __fmul_rn(g, g));
            w[k] = __fsub_rn(w[k], __fdiv_rn(__fmul_rn(a.lr, g), __fadd_rn(update_sqrt_rn(s1[k]), a.eps)));
        } else {
            const float omb1 = __fsub_rn(1.f, a.beta1), omb2 = __fsub_rn(1.f, a.beta2);
            s1[k] = __fadd_rn(__fmul_rn(a.beta1, s1[k]), __fmul_rn(omb1, g));
            s2[k] = __fadd_rn(__fmul_rn(a.beta2, s2[k]), __fmul_rn(omb2, __fmul_rn(g, g)));
            const float mhat = __fdiv_rn(s1[k], __fsub_rn(1.f, pw.p1)), uhat = __fdiv_rn(s2[k], __fsub_rn(1.f, pw.p2));
            w[k] = __fsub_rn(w[k], __fdiv_rn(__fmul_rn(a.lr, mhat), __fadd_rn(update_sqrt_rn(uhat), a.eps)));
        }
    }
    update_store<W>(a.full_table + at, w);
    if (slot >= 0) update_store<W>(a.cache_table + (int64_t)slot * a.D + col0, w);
    if constexpr (OPT != LEGION_UPDATE_SGD) update_store<W>(a.state1 + at, s1);
    if constexpr (OPT == LEGION_UPDATE_ADAM) update_store<W>(a.state2 + at, s2);
}

// ------------------------------------------------------------------------------------------
// reduce and apply
// ------------------------------------------------------------------------------------------
template <int32_t OPT, int32_t W>
__global__ __launch_bounds__(LG_AGG_THREADS) void update_reduce_kernel(UpdateKernelParams p)
{
    __shared__ int32_t s_pos[LG_AGG_WAVES][LG_AGG_K];                 // 4 KiB a workgroup
    const UpdateParams& a = p.u;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t C = 1 << p.lanes_log2, G = 64 >> p.lanes_log2, g = lane >> p.lanes_log2, cl = lane & (C - 1);
    const int32_t U = min(max(p.groups[0], 0), a.m);
    const int64_t total = p.first_chunk[a.m];
    for (int64_t c = (int64_t)blockIdx.x * LG_AGG_WAVES + wave; c < total; c += (int64_t)gridDim.x * LG_AGG_WAVES) {
        // the chunk's group: the last d with first_chunk[d] <= c (first_chunk[0] = 0 and the counts below U are >= 1)
        const int64_t q[1] = {c};
        const bool all[1] = {true};
        int32_t ub[1];
        upper_counts<1>(p.first_chunk, U, q, all, ub);
        const int64_t d = max(ub[0] - 1, 0);
        if (d >= U) continue;
        const int64_t fc = p.first_chunk[d], chunks = p.first_chunk[d + 1] - fc, j = c - fc;
        int32_t s, e;
        update_group(p, d, s, e);
        const int64_t e0 = s + j * LG_AGG_K;
        const int32_t cnt = (int32_t)max(min(e - e0, (int64_t)LG_AGG_K), (int64_t)0);
#pragma unroll
        for (int32_t t = 0; t < 4; t++) {                             // the chunk's positions: ascending, the sort is stable
            const int32_t i = lane + 64 * t;
            const int32_t pos = i < cnt ? p.sorted[e0 + i].pos : -1;  // (e0 + i < e <= m)
            s_pos[wave][i] = (uint32_t)pos < (uint32_t)a.m ? pos : -1;
        }
        update_wave_sync();

        const int32_t v = p.group_id[d];
        const bool single = chunks == 1 && (uint32_t)v < (uint32_t)a.N;        // else: no memory is read or written for v
        const int64_t prow = aggregate_partial_row(fc, d, j);
        const bool park = chunks > 1 && prow < p.partial_rows;
        const int32_t slot = (single && a.node_map) ? a.node_map[v] : -1;
        UpdatePow pw{0.f, 0.f};
        if (single) pw = update_pow<OPT>(a, v);
        for (int32_t u0 = 0; u0 < p.units; u0 += C) {
            const int32_t u = u0 + cl;
            const bool has = u < p.units;
            float acc[W];
#pragma unroll
            for (int32_t k = 0; k < W; k++) acc[k] = 0.f;
            for (int32_t i = g; i < cnt; i += G * LG_AGG_UNROLL) {    // group g takes entries g, g + G, ... in that order
                int32_t pos[LG_AGG_UNROLL];
                float x[LG_AGG_UNROLL][W];
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++) pos[k] = (has && i + k * G < cnt) ? s_pos[wave][i + k * G] : -1;
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++)
                    if (pos[k] >= 0) update_load<W>(a.grads + (int64_t)pos[k] * a.D + u * W, x[k]);
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++) {
                    if (pos[k] >= 0) {
#pragma unroll
                        for (int32_t n = 0; n < W; n++) acc[n] = __fadd_rn(acc[n], x[k][n]);
                    }
                }
            }
            // the groups combine: lane distances C, 2C, ... 32, both sides of a pair computing the same sum
            for (int32_t off = C; off < 64; off <<= 1) {
#pragma unroll
                for (int32_t n = 0; n < W; n++) acc[n] = __fadd_rn(acc[n], __shfl_xor(acc[n], off, 64));
            }
            if (g == 0 && has) {
                if (single) update_apply<OPT, W>(a, v, slot, u * W, acc, cnt, pw);
                else if (park) update_store<W>(p.partial + prow * a.D + u * W, acc);
            }
        }
        if (OPT == LEGION_UPDATE_ADAM && single && lane == 0) {       // after every column has read the old products
            a.state_pow[2 * (int64_t)v] = pw.p1;
            a.state_pow[2 * (int64_t)v + 1] = pw.p2;
        }
        update_wave_sync();                                           // the next chunk stages over s_pos
    }
}

// ------------------------------------------------------------------------------------------
// finish and apply
// ------------------------------------------------------------------------------------------
// A wave per chunk a group has too many, found as the aggregation's finish finds its segment: x = first_chunk[d] - d steps at the
// multi-chunk groups, and the wave whose x is a group's first adds that group's partial rows in chunk order and applies the optimizer
template <int32_t OPT>
__global__ __launch_bounds__(LG_AGG_THREADS) void update_finish_kernel(UpdateKernelParams p)
{
    const UpdateParams& a = p.u;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t U = min(max(p.groups[0], 0), a.m);
    const int64_t extras = p.first_chunk[a.m] - U;
    for (int64_t x = (int64_t)blockIdx.x * LG_AGG_WAVES + wave; x < extras; x += (int64_t)gridDim.x * LG_AGG_WAVES) {
        int64_t d = 0, hi = U;                                        // first_chunk[0] - 0 = 0 <= x
        while (hi - d > 1) {
            const int64_t mid = d + ((hi - d) >> 1);
            if (p.first_chunk[mid] - mid <= x) d = mid;
            else hi = mid;
        }
        const int64_t fc = p.first_chunk[d], chunks = p.first_chunk[d + 1] - fc, row0 = aggregate_partial_row(fc, d, 0);
        if (fc - d != x || chunks <= 1 || row0 + chunks > p.partial_rows) continue;
        int32_t s, e;
        update_group(p, d, s, e);
        const int32_t v = p.group_id[d];
        if ((uint32_t)v >= (uint32_t)a.N) continue;
        const int32_t slot = a.node_map ? a.node_map[v] : -1;
        const UpdatePow pw = update_pow<OPT>(a, v);
        for (int32_t col = lane; col < a.D; col += 64) {
            const float* part = p.partial + row0 * a.D + col;
            float acc[1] = {part[0]};
#pragma unroll 8
            for (int64_t j = 1; j < chunks; j++) acc[0] = __fadd_rn(acc[0], part[j * a.D]);      // chunk order
            update_apply<OPT, 1>(a, v, slot, col, acc, e - s, pw);
        }
        if (OPT == LEGION_UPDATE_ADAM && lane == 0) {
            a.state_pow[2 * (int64_t)v] = pw.p1;
            a.state_pow[2 * (int64_t)v + 1] = pw.p2;
        }
    }
}

template <int32_t OPT>
static void update_launch_apply(hipStream_t s, const UpdateKernelParams& p)
{
    const int32_t m = p.u.m;
    // the most chunks the call can have sizes the grid; the device's own total bounds the walk
    const int64_t most = (int64_t)m + m / LG_AGG_K, wgs = (most + LG_AGG_WAVES - 1) / LG_AGG_WAVES;
    const dim3 grid((uint32_t)(wgs < LG_AGG_MAX_WG ? wgs : LG_AGG_MAX_WG));
    if (p.u.D % 4 == 0) update_reduce_kernel<OPT, 4><<<grid, LG_AGG_THREADS, 0, s>>>(p);
    else update_reduce_kernel<OPT, 1><<<grid, LG_AGG_THREADS, 0, s>>>(p);
    hipCheckError();
    if (p.partial_rows > 0) {
        const int64_t fwgs = (m / LG_AGG_K + LG_AGG_WAVES - 1) / LG_AGG_WAVES;      // the most chunks groups can have too many
        update_finish_kernel<OPT><<<dim3((uint32_t)(fwgs < LG_AGG_MAX_WG ? fwgs : LG_AGG_MAX_WG)), LG_AGG_THREADS, 0, s>>>(p);
        hipCheckError();
    }
}

// the arguments are the caller's to check (update_refusal); scratch holds update_scratch_bytes(m, N, D) bytes
void launch_row_update(hipStream_t s, const UpdateParams& u, void* scratch)
{
    if (u.m <= 0) return;
    const int32_t m = u.m;
    const UpdateScratch at = update_scratch(m);
    int64_t* words = static_cast<int64_t*>(scratch);
    UpdateKernelParams p;
    p.u = u;
    p.pairs[0] = reinterpret_cast<UpdatePair*>(words + at.pairs0);
    p.pairs[1] = reinterpret_cast<UpdatePair*>(words + at.pairs1);
    p.counts = words + at.counts;
    p.tile_heads = reinterpret_cast<int32_t*>(words + at.tile_heads);
    p.groups = reinterpret_cast<int32_t*>(words + at.groups);
    p.group_id = reinterpret_cast<int32_t*>(words + at.group_id);
    p.group_off = reinterpret_cast<int32_t*>(words + at.group_off);
    p.first_chunk = words + at.first_chunk;
    p.partial = reinterpret_cast<float*>(words + at.partial);
    p.partial_rows = aggregate_partial_rows(m);
    p.tiles = (int32_t)update_tiles(m);
    p.units = u.D % 4 == 0 ? u.D / 4 : u.D;
    p.lanes_log2 = 0;
    while ((1 << p.lanes_log2) < aggregate_lanes(p.units)) p.lanes_log2++;

    update_keys_kernel<<<walk_grid(m), LG_UPD_THREADS, 0, s>>>(u.ids, m, u.N, p.pairs[0]);
    hipCheckError();
    const dim3 tile_grid((uint32_t)(p.tiles < LG_WALK_MAX_WG ? p.tiles : LG_WALK_MAX_WG));
    const int32_t passes = update_passes(u.N), values = (int32_t)update_count_values(m);
    for (int32_t pass = 0; pass < passes; pass++) {
        const UpdatePair* in = p.pairs[pass & 1];
        UpdatePair* out = p.pairs[(pass + 1) & 1];
        update_histogram_kernel<<<tile_grid, LG_UPD_THREADS, 0, s>>>(in, m, p.tiles, pass * LG_UPD_RADIX_BITS, p.counts);
        hipCheckError();
        launch_scan_int64(s, p.counts, values, words + at.count_sums, p.tiles, false, words + at.count_total, nullptr);
        update_scatter_kernel<<<tile_grid, LG_UPD_THREADS, 0, s>>>(in, out, m, p.tiles, pass * LG_UPD_RADIX_BITS, p.counts);
        hipCheckError();
    }
    p.sorted = p.pairs[passes & 1];

    update_head_count_kernel<<<tile_grid, LG_UPD_THREADS, 0, s>>>(p);
    update_head_scan_kernel<<<1, LG_UPD_THREADS, 0, s>>>(p);
    update_head_write_kernel<<<tile_grid, LG_UPD_THREADS, 0, s>>>(p);
    update_chunks_kernel<<<walk_grid(m), LG_UPD_THREADS, 0, s>>>(p);
    hipCheckError();
    update_scan(s, p.first_chunk, m, words + at.chunk_sums);

    switch (u.optimizer) {
    case LEGION_UPDATE_SGD: update_launch_apply<LEGION_UPDATE_SGD>(s, p); break;
    case LEGION_UPDATE_ADAGRAD: update_launch_apply<LEGION_UPDATE_ADAGRAD>(s, p); break;
    default: update_launch_apply<LEGION_UPDATE_ADAM>(s, p); break;
    }
}

}  // namespace lg
