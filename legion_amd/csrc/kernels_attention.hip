// kernels_attention.hip -- the fused attention aggregation for gfx950 (CDNA4, wave64): per segment of source ids and head, a logit per
// entry (a dot of the destination's query with the source's stored row, plus a bias), a softmax over the segment and the weighted sum
// of the rows (legion_attention_rows; DGL's u_dot_v + edge_softmax + u_mul_e_sum).  The rule is the contract in include/legion_hip.h;
// the refusals, the register plan and the scratch layout are attention_rule.h's, the chunk rule and the row formats aggregate_rule.h's.
// A batch of skinny GEMVs with an operand of their own per destination, bound by the scattered row reads; no MFMA, no floating-point
// atomic.
//   * chunks, scan   the aggregation's: a segment's wave-chunks (at most LG_AGG_K entries each) to first_chunk[d], scanned in place;
//   * reduce   a grid of at most LG_AGG_MAX_WG workgroups of four waves; a wave strides over chunk numbers, finds its segment by an
//              upper-bound search of first_chunk and resolves the chunk's entries in lanes, four a lane, into LDS (a row's address, 0 for
//              a dead entry).  Then the wave is G = 64 / C groups of C lanes; lane cl of a group holds units cl, cl + C, ... (U of them,
//              16 bytes of a row each) of the segment's HP query rows and of HP accumulator rows in registers for the whole chunk.
//              Group g takes entries g, g + G, ... in blocks of B rows: the B rows are loaded once (B x U loads in flight) and serve
//              every head, the dot and the weighted sum; the dots' partial sums cross the C lanes by an xor butterfly, so every lane
//              has every logit; then per head one new running maximum, one rescale of l and the accumulators, B exponentials and
//              B fmas a column.  The groups' states (m, l, acc) merge by a butterfly over lane distances C, 2C, ... 32, the lower group
//              first: a fixed tree.  A single-chunk segment's result goes to out and lse_out (the division, the narrowing); a chunk of a
//              longer one writes its partial record to the scratch.  scores_out is written by lane 0 of the group that holds the logit;
//   * finish   a wave per chunk the segments have too many finds its segment by a binary search and, if it is that segment's first,
//              merges its records in chunk order, a lane per column.
// Every sum and every merge has one order, fixed by the segment's length, D and heads alone: the result is bit-identical from run to
// run.
#include "aggregate_device.h"
#include "attention_rule.h"

namespace lg {

// the chunk counts (kernels_aggregate.hip)
__global__ void aggregate_chunks_kernel(AggregateParams a, int64_t* first_chunk);

struct AttentionKernelParams {
    AttentionParams t;
    int64_t* first_chunk;           // int64[n + 1]
    float* partial;                 // float[partial_rows x record]
    int64_t partial_rows;
    int64_t record;                 // floats of a record: (m, l)[heads], then heads x D
    int64_t row_bytes;              // of a stored row
    int32_t units;                  // lane-units of a row
    int32_t lanes_log2;             // log2 C
};

// exp(m - ref) of a state's maximum: an empty state (m = -inf) weighs nothing, whatever ref is
__device__ __forceinline__ float attention_weight(float m, float ref) { return m == -INFINITY ? 0.f : expf(m - ref); }

// the reference maximum of a merge: 0 while every state is empty, so that no -inf - -inf is formed
__device__ __forceinline__ float attention_ref(float m) { return m == -INFINITY ? 0.f : m; }

__device__ __forceinline__ float attention_out(float acc, float l) { return l > 0.f ? __fdiv_rn(acc, l) : 0.f; }
__device__ __forceinline__ float attention_lse(float m, float l) { return l > 0.f ? m + logf(l) : -INFINITY; }

// columns [col0, col0 + W) of row (d, h) of out
template <int32_t W>
__device__ __forceinline__ void attention_store_out(const AttentionParams& t, int64_t d, int32_t h, int32_t col0, const float (&v)[W])
{
    const AggregateParams& a = t.rows;
    const int64_t row = (d * t.heads + h) * a.D;
    if (a.out_dtype == LEGION_FEATURE_BF16) aggregate_store_bf16<W>(static_cast<uint16_t*>(a.out) + row, a.D, col0, v);
    else aggregate_store_f32<W>(static_cast<float*>(a.out) + row, a.D, col0, v);
}

// ------------------------------------------------------------------------------------------
// reduce
// ------------------------------------------------------------------------------------------
template <AggregateRow ROW, int32_t HP, int32_t U>
__global__ __launch_bounds__(LG_AGG_THREADS) void attention_reduce_kernel(AttentionKernelParams p)
{
    constexpr int32_t W = aggregate_unit_width(ROW), B = attention_unroll(U * W);
    static_assert(HP * U * W <= LG_ATT_MAX_LANE_FLOATS && U <= LG_ATT_MAX_LANE_UNITS, "the register plan (attention_rule.h)");
    typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
    __shared__ uint64_t s_row[LG_AGG_WAVES][LG_AGG_K];                // 8 bytes an entry, 8 KiB a workgroup
    const AttentionParams& t = p.t;
    const AggregateParams& a = t.rows;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t C = 1 << p.lanes_log2, G = 64 >> p.lanes_log2, g = lane >> p.lanes_log2, cl = lane & (C - 1);
    const int32_t heads = t.heads;
    bool has[U];
#pragma unroll
    for (int32_t u = 0; u < U; u++) has[u] = cl + C * u < p.units;
    const int64_t total = p.first_chunk[a.n];
    for (int64_t c = (int64_t)blockIdx.x * LG_AGG_WAVES + wave; c < total; c += (int64_t)gridDim.x * LG_AGG_WAVES) {
        // the chunk's segment: the last d with first_chunk[d] <= c (first_chunk[0] = 0 and the counts are >= 1: 0 <= d < n)
        const int64_t qc[1] = {c};
        const bool all[1] = {true};
        int32_t ub[1];
        upper_counts<1>(p.first_chunk, a.n, qc, all, ub);
        const int64_t d = max(ub[0] - 1, 0);
        const int64_t fc = p.first_chunk[d], chunks = p.first_chunk[d + 1] - fc, j = c - fc;
        int64_t s, e;
        aggregate_segment(a, d, s, e);
        const int64_t e0 = s + j * LG_AGG_K;
        const int32_t cnt = (int32_t)max(min(e - e0, (int64_t)LG_AGG_K), (int64_t)0);

        // resolve in lanes: entries lane, lane + 64, ...
        int32_t id[4], slot[4];
#pragma unroll
        for (int32_t k = 0; k < 4; k++) {
            const int32_t i = lane + 64 * k;
            id[k] = i < cnt ? a.ids[e0 + i] : -1;                     // (e0 + i < e <= M)
        }
#pragma unroll
        for (int32_t k = 0; k < 4; k++) {
            const bool ok = (uint32_t)id[k] < (uint32_t)a.N;          // else: no memory is read for id
            slot[k] = (ok && a.node_map) ? a.node_map[id[k]] : -1;
        }
#pragma unroll
        for (int32_t k = 0; k < 4; k++) {
            const bool ok = (uint32_t)id[k] < (uint32_t)a.N;
            const uint64_t base = (uint64_t)(uintptr_t)(slot[k] >= 0 ? a.cache_table : a.full_table);
            const int64_t r = slot[k] >= 0 ? slot[k] : id[k];
            s_row[wave][lane + 64 * k] = ok ? base + (uint64_t)(r * p.row_bytes) : 0;
        }
        aggregate_wave_sync();

        // the segment's queries, this lane's columns of every head; 0 for a pad head and for a column past D (a bf16 row's pad)
        float q[HP][U][W];
#pragma unroll
        for (int32_t h = 0; h < HP; h++) {
#pragma unroll
            for (int32_t u = 0; u < U; u++) {
#pragma unroll
                for (int32_t w = 0; w < W; w++) q[h][u][w] = 0.f;
                if (!t.queries || h >= heads || !has[u]) continue;
                const int32_t col0 = (cl + C * u) * W;
                const float* qr = t.queries + (d * heads + h) * a.D + col0;
                if constexpr (W >= 4) {
                    if (col0 + W <= a.D) {
#pragma unroll
                        for (int32_t w = 0; w < W; w += 4) {
                            const v4u v = *(const LG_G v4u*)(qr + w);
                            q[h][u][w] = v.x; q[h][u][w + 1] = v.y; q[h][u][w + 2] = v.z; q[h][u][w + 3] = v.w;
                        }
                        continue;
                    }
                }
#pragma unroll
                for (int32_t w = 0; w < W; w++)
                    if (col0 + w < a.D) q[h][u][w] = qr[w];
            }
        }

        // read in groups: group g takes entries g, g + G, ... in that order, B at a time
        float m[HP], l[HP], acc[HP][U][W];
#pragma unroll
        for (int32_t h = 0; h < HP; h++) {
            m[h] = -INFINITY;
            l[h] = 0.f;
#pragma unroll
            for (int32_t u = 0; u < U; u++)
#pragma unroll
                for (int32_t w = 0; w < W; w++) acc[h][u][w] = 0.f;
        }
        for (int32_t i0 = 0; i0 < cnt; i0 += G * B) {                 // (the same trips for every group: the butterflies are whole)
            uint64_t row[B];
            float x[B][U][W], sc[B][HP];
#pragma unroll
            for (int32_t k = 0; k < B; k++) {
                const int32_t ik = i0 + g + k * G;
                row[k] = ik < cnt ? s_row[wave][ik] : 0;
            }
#pragma unroll
            for (int32_t k = 0; k < B; k++) {
#pragma unroll
                for (int32_t u = 0; u < U; u++) {
                    if (row[k] != 0 && has[u]) AggregateUnit<ROW>::load(row[k], cl + C * u, x[k][u]);
                    else {
#pragma unroll
                        for (int32_t w = 0; w < W; w++) x[k][u][w] = 0.f;
                    }
                }
#pragma unroll
                for (int32_t h = 0; h < HP; h++)
                    sc[k][h] = (t.bias && row[k] != 0 && h < heads) ? t.bias[(e0 + i0 + g + k * G) * heads + h] : 0.f;
            }
            // the block's logits: a lane's columns in order, the C lanes by a butterfly (every lane of the group ends with the same bits)
            if (t.queries) {
                float dot[B][HP];
#pragma unroll
                for (int32_t k = 0; k < B; k++) {
#pragma unroll
                    for (int32_t h = 0; h < HP; h++) {
                        float v = 0.f;
#pragma unroll
                        for (int32_t u = 0; u < U; u++)
#pragma unroll
                            for (int32_t w = 0; w < W; w++) v = fmaf(q[h][u][w], x[k][u][w], v);
                        dot[k][h] = v;
                    }
                }
                for (int32_t off = 1; off < C; off <<= 1) {
#pragma unroll
                    for (int32_t k = 0; k < B; k++)
#pragma unroll
                        for (int32_t h = 0; h < HP; h++) dot[k][h] += __shfl_xor(dot[k][h], off, 64);
                }
#pragma unroll
                for (int32_t k = 0; k < B; k++)
#pragma unroll
                    for (int32_t h = 0; h < HP; h++) sc[k][h] = fmaf(t.scale, dot[k][h], sc[k][h]);
            }
            if (t.scores_out && cl == 0) {
#pragma unroll
                for (int32_t k = 0; k < B; k++) {
                    const int32_t ik = i0 + g + k * G;
                    if (ik >= cnt) continue;
#pragma unroll
                    for (int32_t h = 0; h < HP; h++)
                        if (h < heads) t.scores_out[(e0 + ik) * heads + h] = row[k] != 0 ? sc[k][h] : 0.f;
                }
            }
            // the online softmax: one new maximum and one rescale a block
#pragma unroll
            for (int32_t h = 0; h < HP; h++) {
                float mn = m[h];
#pragma unroll
                for (int32_t k = 0; k < B; k++)
                    if (row[k] != 0) mn = fmaxf(mn, sc[k][h]);
                const float ref = attention_ref(mn), keep = attention_weight(m[h], ref);
                float pk[B];
#pragma unroll
                for (int32_t k = 0; k < B; k++) pk[k] = row[k] != 0 ? expf(sc[k][h] - ref) : 0.f;
                float lv = l[h] * keep;
#pragma unroll
                for (int32_t k = 0; k < B; k++) lv += pk[k];
                l[h] = lv;
                m[h] = mn;
#pragma unroll
                for (int32_t u = 0; u < U; u++) {
#pragma unroll
                    for (int32_t w = 0; w < W; w++) {
                        float v = acc[h][u][w] * keep;
#pragma unroll
                        for (int32_t k = 0; k < B; k++) v = fmaf(pk[k], x[k][u][w], v);
                        acc[h][u][w] = v;
                    }
                }
            }
        }
        // the groups merge: lane distances C, 2C, ... 32, the lower group first on both sides of a pair
        for (int32_t off = C; off < 64; off <<= 1) {
            const bool upper = (lane & off) != 0;
#pragma unroll
            for (int32_t h = 0; h < HP; h++) {
                const float m2 = __shfl_xor(m[h], off, 64), l2 = __shfl_xor(l[h], off, 64);
                const float mn = fmaxf(m[h], m2), ref = attention_ref(mn);
                const float w1 = attention_weight(m[h], ref), w2 = attention_weight(m2, ref);
                const float wl = upper ? w2 : w1, wh = upper ? w1 : w2;
                l[h] = fmaf(upper ? l2 : l[h], wl, (upper ? l[h] : l2) * wh);
                m[h] = mn;
#pragma unroll
                for (int32_t u = 0; u < U; u++) {
#pragma unroll
                    for (int32_t w = 0; w < W; w++) {
                        const float y = __shfl_xor(acc[h][u][w], off, 64);
                        acc[h][u][w] = fmaf(upper ? y : acc[h][u][w], wl, (upper ? acc[h][u][w] : y) * wh);
                    }
                }
            }
        }
        const bool single = chunks == 1;
        const int64_t prow = aggregate_partial_row(fc, d, j);
        const bool park = !single && prow < p.partial_rows;           // (always, for non-decreasing offsets)
        if (g == 0 && (single || park)) {
            float* rec = p.partial + prow * p.record;                 // (followed only when park)
#pragma unroll
            for (int32_t h = 0; h < HP; h++) {
                if (h >= heads) continue;
#pragma unroll
                for (int32_t u = 0; u < U; u++) {
                    if (!has[u]) continue;
                    const int32_t col0 = (cl + C * u) * W;
                    if (single) {
                        float v[W];
#pragma unroll
                        for (int32_t w = 0; w < W; w++) v[w] = attention_out(acc[h][u][w], l[h]);
                        attention_store_out<W>(t, d, h, col0, v);
                    } else {
                        aggregate_store_f32<W>(rec + 2 * heads + (int64_t)h * a.D, a.D, col0, acc[h][u]);
                    }
                }
                if (cl == 0) {
                    if (!single) {
                        rec[2 * h] = m[h];
                        rec[2 * h + 1] = l[h];
                    } else if (t.lse_out) {
                        t.lse_out[d * heads + h] = attention_lse(m[h], l[h]);
                    }
                }
            }
        }
        aggregate_wave_sync();                                        // the next chunk stages over s_row
    }
}

// ------------------------------------------------------------------------------------------
// finish
// ------------------------------------------------------------------------------------------
// A wave per chunk a segment has too many, as aggregate_finish_kernel: the wave whose x = first_chunk[d] - d is segment d's first merges
// its records in chunk order, a lane per column; every lane forms the same weights and the same l.
__global__ __launch_bounds__(LG_AGG_THREADS) void attention_finish_kernel(AttentionKernelParams p)
{
    const AttentionParams& t = p.t;
    const AggregateParams& a = t.rows;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, heads = t.heads;
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
        const float* rec0 = p.partial + row0 * p.record;
        for (int32_t h = 0; h < heads; h++) {
            float mx = -INFINITY;                                     // (a maximum has no order)
            for (int64_t j = lane; j < chunks; j += 64) mx = fmaxf(mx, rec0[j * p.record + 2 * h]);
            for (int32_t off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            const float ref = attention_ref(mx);
            for (int32_t c0 = 0; c0 < a.D; c0 += 64) {
                const int32_t col = c0 + lane;
                const float* part = rec0 + 2 * heads + (int64_t)h * a.D + (col < a.D ? col : 0);
                float acc = 0.f, l = 0.f;
#pragma unroll 4
                for (int64_t j = 0; j < chunks; j++) {                // chunk order
                    const float* rec = rec0 + j * p.record;
                    const float w = attention_weight(rec[2 * h], ref);
                    l = fmaf(rec[2 * h + 1], w, l);
                    acc = fmaf(part[j * p.record], w, acc);
                }
                if (col < a.D) {
                    const float v = attention_out(acc, l);
                    const int64_t o = (d * heads + h) * a.D + col;
                    if (a.out_dtype == LEGION_FEATURE_BF16) static_cast<uint16_t*>(a.out)[o] = (uint16_t)aggregate_bf16_rne(v);
                    else static_cast<float*>(a.out)[o] = v;
                }
                if (col == 0 && t.lse_out) t.lse_out[d * heads + h] = attention_lse(mx, l);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// the launch: one reduce kernel per row format, padded head count and units a lane holds that the register plan allows
// ------------------------------------------------------------------------------------------
template <AggregateRow ROW, int32_t HP, int32_t U>
static void attention_launch_plan(hipStream_t s, dim3 grid, const AttentionKernelParams& p)
{
    if constexpr (HP * U * aggregate_unit_width(ROW) <= LG_ATT_MAX_LANE_FLOATS)
        attention_reduce_kernel<ROW, HP, U><<<grid, LG_AGG_THREADS, 0, s>>>(p);
}

template <AggregateRow ROW, int32_t HP>
static void attention_launch_units(hipStream_t s, dim3 grid, const AttentionKernelParams& p)
{
    switch (attention_lane_units(p.units)) {
    case 1: attention_launch_plan<ROW, HP, 1>(s, grid, p); break;
    case 2: attention_launch_plan<ROW, HP, 2>(s, grid, p); break;
    case 4: attention_launch_plan<ROW, HP, 4>(s, grid, p); break;
    }
}

template <AggregateRow ROW>
static void attention_launch_heads(hipStream_t s, dim3 grid, const AttentionKernelParams& p)
{
    switch (attention_heads_padded(p.t.heads)) {
    case 1: attention_launch_units<ROW, 1>(s, grid, p); break;
    case 2: attention_launch_units<ROW, 2>(s, grid, p); break;
    case 4: attention_launch_units<ROW, 4>(s, grid, p); break;
    case 8: attention_launch_units<ROW, 8>(s, grid, p); break;
    }
}

// the arguments are the caller's to check (attention_refusal); scratch holds attention_scratch_bytes(n, M, D, heads) bytes
void launch_attention_rows(hipStream_t s, const AttentionParams& t, void* scratch)
{
    const AggregateParams& a = t.rows;
    if (a.n <= 0) return;
    AttentionKernelParams p;
    p.t = t;
    p.first_chunk = static_cast<int64_t*>(scratch);
    int64_t* sums = p.first_chunk + a.n + 1;
    p.partial = reinterpret_cast<float*>(p.first_chunk + aggregate_first_words(a.n));
    p.partial_rows = aggregate_partial_rows(a.M);
    p.record = attention_record_floats(a.D, t.heads);
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
    case AggregateRow::F32x4: attention_launch_heads<AggregateRow::F32x4>(s, grid, p); break;
    case AggregateRow::F32x1: attention_launch_heads<AggregateRow::F32x1>(s, grid, p); break;
    case AggregateRow::Bf16x8: attention_launch_heads<AggregateRow::Bf16x8>(s, grid, p); break;
    }
    hipCheckError();
    if (p.partial_rows > 0) {
        const int64_t fwgs = (a.M / LG_AGG_K + LG_AGG_WAVES - 1) / LG_AGG_WAVES;      // the most chunks segments can have too many
        const dim3 fgrid((uint32_t)(fwgs < LG_AGG_MAX_WG ? fwgs : LG_AGG_MAX_WG));
        attention_finish_kernel<<<fgrid, LG_AGG_THREADS, 0, s>>>(p);
        hipCheckError();
    }
}

}  // namespace lg
