// kernels_aggregate.hip -- the fused neighbour aggregation for gfx950 (CDNA4, wave64): out[d] = sum / mean / max over a segment of
// source ids of their (weighted) feature rows (legion_aggregate_rows; DGL's copy_u_sum / copy_u_mean / copy_u_max and u_mul_e_sum).
// The rule is the contract in include/legion_hip.h; the constants, the chunk rule and the scratch layout are aggregate_rule.h's.
// A segmented reduction over skewed segment lengths, bound by the scattered row reads; no MFMA, no floating-point atomic.
//   * chunks   a lane per segment: its wave-chunks (at most LG_AGG_K entries each, an empty segment keeps one) to first_chunk[d];
//   * scan     first_chunk in place, the total to first_chunk[n]: launch_scan_int64 alone up to 2^20 segments, else at two levels,
//              as the reverse CSR's scan;
//   * reduce   a grid of at most LG_AGG_MAX_WG workgroups of four waves; a wave strides over chunk numbers up to the total the scan
//              left on the device and finds its segment by an upper-bound search of first_chunk (row_slots.h).  It reads the chunk's ids
//              and weights coalesced, four a lane; every lane resolves its own entries (the bounds check, node_map[id], the row's
//              address) and parks {address, weight} in LDS, 12 bytes an entry, a skipped entry as address 0; the live count is a sum
//              of ballots.  Then the wave is G = 64 / C groups of C lanes, C the lanes that cover a row at one unit (16 bytes, or one
//              float32 where D % 4 != 0) each; group g takes entries g, g + G, ... of the chunk in that order, LG_AGG_UNROLL rows in
//              flight, into float32 registers (fmaf(w, x, acc) or fmaxf); rows past 64 units are walked in column blocks.  The groups
//              combine by a butterfly over lane distances C, 2C, ... 32: a fixed tree.  A single-chunk segment's result goes to out
//              (the division, the narrowing); a chunk of a longer one writes its partial row and live count to the scratch;
//   * finish   a wave per chunk the segments have too many (first_chunk[d] - d counts them) finds its segment by a binary search and,
//              if it is that segment's first, reduces it, a lane per column, over its partial rows in chunk order: the finishes of a
//              call's long segments are spread over the grid.
// Every sum has one order, fixed by the segment's length and D alone: the result is bit-identical from run to run.
#include "aggregate_device.h"

namespace lg {

struct AggregateKernelParams {
    AggregateParams a;
    int64_t* first_chunk;           // int64[n + 1]
    float* partial;                 // float[partial_rows x D]
    int32_t* partial_live;          // int32[partial_rows]
    int64_t partial_rows;
    int64_t row_bytes;              // of a stored row
    int32_t units;                  // lane-units of a row
    int32_t lanes_log2;             // log2 C
};

// ------------------------------------------------------------------------------------------
// chunks
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_AGG_THREADS) void aggregate_chunks_kernel(AggregateParams a, int64_t* first_chunk)
{
    const int64_t tiles = ((int64_t)a.n + LG_AGG_THREADS - 1) / LG_AGG_THREADS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t d = tile * LG_AGG_THREADS + threadIdx.x;
        if (d < a.n) {
            int64_t s, e;
            aggregate_segment(a, d, s, e);
            first_chunk[d] = aggregate_chunks(e - s);
        }
    }
}

// ------------------------------------------------------------------------------------------
// reduce
// ------------------------------------------------------------------------------------------
// (a unit of a stored row as W float32 and the stores of a lane's columns: aggregate_device.h)

// what out holds for a reduced value of a segment with `live` entries: zeros for none, the mean's correctly rounded division
__device__ __forceinline__ float aggregate_final(float acc, int64_t live, int32_t reduce)
{
    if (live <= 0) return 0.f;
    return reduce == LEGION_REDUCE_MEAN ? __fdiv_rn(acc, (float)live) : acc;
}

template <int32_t W>
__device__ __forceinline__ void aggregate_store_out(const AggregateParams& a, int64_t d, int32_t col0, const float (&acc)[W], int64_t live)
{
    float v[W];
#pragma unroll
    for (int32_t k = 0; k < W; k++) v[k] = aggregate_final(acc[k], live, a.reduce);
    if (a.out_dtype == LEGION_FEATURE_BF16) aggregate_store_bf16<W>(static_cast<uint16_t*>(a.out) + d * a.D, a.D, col0, v);
    else aggregate_store_f32<W>(static_cast<float*>(a.out) + d * a.D, a.D, col0, v);
}

template <AggregateRow ROW, bool IS_MAX>
__global__ __launch_bounds__(LG_AGG_THREADS) void aggregate_reduce_kernel(AggregateKernelParams p)
{
    constexpr int32_t W = aggregate_unit_width(ROW);
    __shared__ uint64_t s_row[LG_AGG_WAVES][LG_AGG_K];                // 12 bytes an entry, 12 KiB a workgroup
    __shared__ float s_w[LG_AGG_WAVES][LG_AGG_K];
    const AggregateParams& a = p.a;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t C = 1 << p.lanes_log2, G = 64 >> p.lanes_log2, g = lane >> p.lanes_log2, cl = lane & (C - 1);
    const int64_t total = p.first_chunk[a.n];
    for (int64_t c = (int64_t)blockIdx.x * LG_AGG_WAVES + wave; c < total; c += (int64_t)gridDim.x * LG_AGG_WAVES) {
        // the chunk's segment: the last d with first_chunk[d] <= c (first_chunk[0] = 0 and the counts are >= 1: 0 <= d < n)
        const int64_t q[1] = {c};
        const bool all[1] = {true};
        int32_t ub[1];
        upper_counts<1>(p.first_chunk, a.n, q, all, ub);
        const int64_t d = max(ub[0] - 1, 0);
        const int64_t fc = p.first_chunk[d], chunks = p.first_chunk[d + 1] - fc, j = c - fc;
        int64_t s, e;
        aggregate_segment(a, d, s, e);
        const int64_t e0 = s + j * LG_AGG_K;
        const int32_t cnt = (int32_t)max(min(e - e0, (int64_t)LG_AGG_K), (int64_t)0);

        // resolve in lanes: entries lane, lane + 64, ...
        int32_t id[4], slot[4];
        float w[4];
#pragma unroll
        for (int32_t t = 0; t < 4; t++) {
            const int32_t i = lane + 64 * t;
            id[t] = i < cnt ? a.ids[e0 + i] : -1;                     // (e0 + i < e <= M)
            w[t] = (i < cnt && a.weights) ? a.weights[e0 + i] : 1.f;
        }
        int32_t live = 0;
#pragma unroll
        for (int32_t t = 0; t < 4; t++) {
            const bool ok = (uint32_t)id[t] < (uint32_t)a.N;          // else: no memory is read for id
            slot[t] = (ok && a.node_map) ? a.node_map[id[t]] : -1;
            live += __popcll(__ballot(ok));
        }
#pragma unroll
        for (int32_t t = 0; t < 4; t++) {
            const bool ok = (uint32_t)id[t] < (uint32_t)a.N;
            const uint64_t base = (uint64_t)(uintptr_t)(slot[t] >= 0 ? a.cache_table : a.full_table);
            const int64_t r = slot[t] >= 0 ? slot[t] : id[t];
            s_row[wave][lane + 64 * t] = ok ? base + (uint64_t)(r * p.row_bytes) : 0;
            s_w[wave][lane + 64 * t] = w[t];
        }
        aggregate_wave_sync();

        // read in groups: group g takes entries g, g + G, ... in that order
        const bool single = chunks == 1;
        const int64_t prow = aggregate_partial_row(fc, d, j);
        const bool park = !single && prow < p.partial_rows;           // (always, for non-decreasing offsets)
        for (int32_t u0 = 0; u0 < p.units; u0 += C) {
            const int32_t u = u0 + cl;
            const bool has = u < p.units;
            float acc[W];
#pragma unroll
            for (int32_t k = 0; k < W; k++) acc[k] = IS_MAX ? -INFINITY : 0.f;
            for (int32_t i = g; i < cnt; i += G * LG_AGG_UNROLL) {
                uint64_t row[LG_AGG_UNROLL];
                float rw[LG_AGG_UNROLL], x[LG_AGG_UNROLL][W];
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++) {
                    const int32_t ik = i + k * G;
                    row[k] = (has && ik < cnt) ? s_row[wave][ik] : 0;
                    rw[k] = ik < cnt ? s_w[wave][ik] : 0.f;
                }
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++)
                    if (row[k] != 0) AggregateUnit<ROW>::load(row[k], u, x[k]);
#pragma unroll
                for (int32_t k = 0; k < LG_AGG_UNROLL; k++) {
                    if (row[k] != 0) {
#pragma unroll
                        for (int32_t m = 0; m < W; m++) acc[m] = IS_MAX ? fmaxf(acc[m], x[k][m]) : fmaf(rw[k], x[k][m], acc[m]);
                    }
                }
            }
            // the groups combine: lane distances C, 2C, ... 32, both sides of a pair computing the same sum
            for (int32_t off = C; off < 64; off <<= 1) {
#pragma unroll
                for (int32_t m = 0; m < W; m++) {
                    const float y = __shfl_xor(acc[m], off, 64);
                    acc[m] = IS_MAX ? fmaxf(acc[m], y) : acc[m] + y;
                }
            }
            if (g == 0 && has) {
                if (single) aggregate_store_out<W>(a, d, u * W, acc, live);
                else if (park) aggregate_store_f32<W>(p.partial + prow * a.D, a.D, u * W, acc);
            }
        }
        if (park && lane == 0) p.partial_live[prow] = live;
        aggregate_wave_sync();                                        // the next chunk stages over s_row and s_w
    }
}

// ------------------------------------------------------------------------------------------
// finish
// ------------------------------------------------------------------------------------------
// A wave per chunk a segment has too many: x = first_chunk[d] - d is non-decreasing in d and steps at the multi-chunk segments, so
// the last d with first_chunk[d] - d <= x is the segment x falls into, and the wave whose x is that segment's first finishes it.  The
// finishes of a call's long segments are therefore spread over the grid like its chunks.
template <bool IS_MAX>
__global__ __launch_bounds__(LG_AGG_THREADS) void aggregate_finish_kernel(AggregateKernelParams p)
{
    const AggregateParams& a = p.a;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t extras = p.first_chunk[a.n] - a.n;
    for (int64_t x = (int64_t)blockIdx.x * LG_AGG_WAVES + wave; x < extras; x += (int64_t)gridDim.x * LG_AGG_WAVES) {
        int64_t d = 0, hi = a.n;                                      // first_chunk[0] - 0 = 0 <= x
        while (hi - d > 1) {
            const int64_t mid = d + ((hi - d) >> 1);
            if (p.first_chunk[mid] - mid <= x) d = mid;
            else hi = mid;
        }
        const int64_t fc = p.first_chunk[d], chunks = p.first_chunk[d + 1] - fc, row0 = aggregate_partial_row(fc, d, 0);
        if (fc - d != x || chunks <= 1 || row0 + chunks > p.partial_rows) continue;      // (the last: never, for non-decreasing offsets)
        int64_t live = 0;
        for (int64_t j = lane; j < chunks; j += 64) live += p.partial_live[row0 + j];
        for (int32_t off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
        for (int32_t col = lane; col < a.D; col += 64) {
            const float* part = p.partial + row0 * a.D + col;
            float acc = part[0];
#pragma unroll 8
            for (int64_t j = 1; j < chunks; j++) acc = IS_MAX ? fmaxf(acc, part[j * a.D]) : acc + part[j * a.D];      // chunk order
            const float v = aggregate_final(acc, live, a.reduce);
            if (a.out_dtype == LEGION_FEATURE_BF16) static_cast<uint16_t*>(a.out)[d * a.D + col] = (uint16_t)aggregate_bf16_rne(v);
            else static_cast<float*>(a.out)[d * a.D + col] = v;
        }
    }
}

template <AggregateRow ROW>
static void aggregate_launch_reduce(hipStream_t s, dim3 grid, const AggregateKernelParams& p)
{
    if (p.a.reduce == LEGION_REDUCE_MAX) aggregate_reduce_kernel<ROW, true><<<grid, LG_AGG_THREADS, 0, s>>>(p);
    else aggregate_reduce_kernel<ROW, false><<<grid, LG_AGG_THREADS, 0, s>>>(p);
}

// the arguments are the caller's to check (aggregate_refusal); scratch holds aggregate_scratch_bytes(n, M, D) bytes
void launch_aggregate_rows(hipStream_t s, const AggregateParams& a, void* scratch)
{
    if (a.n <= 0) return;
    AggregateKernelParams p;
    p.a = a;
    p.first_chunk = static_cast<int64_t*>(scratch);
    int64_t* sums = p.first_chunk + a.n + 1;
    p.partial = reinterpret_cast<float*>(p.first_chunk + aggregate_first_words(a.n));
    p.partial_rows = aggregate_partial_rows(a.M);
    p.partial_live = reinterpret_cast<int32_t*>(p.partial + p.partial_rows * a.D);
    p.row_bytes = lg_feature_row_bytes(a.dtype, a.D);
    p.units = aggregate_units(a.dtype, a.D);
    p.lanes_log2 = 0;
    while ((1 << p.lanes_log2) < aggregate_lanes(p.units)) p.lanes_log2++;

    aggregate_chunks_kernel<<<walk_grid(a.n), LG_AGG_THREADS, 0, s>>>(a, p.first_chunk);
    hipCheckError();
    aggregate_scan(s, p.first_chunk, a.n, sums);

    // the most chunks the call can have sizes the grid; the device's own total bounds the walk
    const int64_t most = (int64_t)a.n + a.M / LG_AGG_K, wgs = (most + LG_AGG_WAVES - 1) / LG_AGG_WAVES;
    const dim3 grid((uint32_t)(wgs < LG_AGG_MAX_WG ? wgs : LG_AGG_MAX_WG));
    switch (aggregate_row(a.dtype, a.D)) {
    case AggregateRow::F32x4: aggregate_launch_reduce<AggregateRow::F32x4>(s, grid, p); break;
    case AggregateRow::F32x1: aggregate_launch_reduce<AggregateRow::F32x1>(s, grid, p); break;
    case AggregateRow::Bf16x8: aggregate_launch_reduce<AggregateRow::Bf16x8>(s, grid, p); break;
    }
    hipCheckError();
    if (p.partial_rows > 0) {
        const int64_t fwgs = (a.M / LG_AGG_K + LG_AGG_WAVES - 1) / LG_AGG_WAVES;      // the most chunks segments can have too many
        const dim3 fgrid((uint32_t)(fwgs < LG_AGG_MAX_WG ? fwgs : LG_AGG_MAX_WG));
        if (a.reduce == LEGION_REDUCE_MAX) aggregate_finish_kernel<true><<<fgrid, LG_AGG_THREADS, 0, s>>>(p);
        else aggregate_finish_kernel<false><<<fgrid, LG_AGG_THREADS, 0, s>>>(p);
        hipCheckError();
    }
}

}  // namespace lg
