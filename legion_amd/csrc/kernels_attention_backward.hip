// kernels_attention_backward.hip -- the backward pass of the fused attention aggregation for gfx950 (CDNA4, wave64): from the gradient
// of out, the gradients of the queries, the bias and of every entry's source row (legion_attention_rows_backward).  The rule is the
// contract in include/legion_hip.h; the refusals, the register plan and the scratch layout are attention_backward_rule.h's, the chunk
// rule and the row formats aggregate_rule.h's, the lane geometry kernels_attention.hip's.  As the forward: a batch of skinny GEMVs with
// an operand of their own per destination, bound by the scattered row reads and here by the M x D store; no MFMA, no floating-point
// atomic.
//   * chunks, scan   the aggregation's: a segment's wave-chunks (at most LG_AGG_K entries each) to first_chunk[d], scanned in place;
//   * reduce   the forward's grid, chunk walk and entry resolution (a row's address in LDS, 0 for a dead entry).  The wave is
//              G = 64 / C groups of C lanes; lane cl of a group holds units cl, cl + C, ... of the segment's HP query rows, HP dO rows
//              and HP grad_queries sums in registers for the whole chunk: three row sets (one, dO, without queries).  At the chunk's
//              start it also reads its columns of out and forms delta[h] = dO . out: its columns in order, then the xor butterfly
//              over the C lanes.  Group g takes entries g, g + G, ... in blocks of B rows: the B rows are loaded once and serve every
//              head; the two dots a head, q . x and dO . x, cross the C lanes in one butterfly pass; then one expf an entry and head,
//              p = expf(s - lse), dS = p (t - delta).  Lane 0 of the group writes the entry's grad_bias, the group's C lanes its
//              grad_rows row, formed head by head in registers and stored 16 bytes at a time, and every lane adds dS x to its
//              grad_queries sums, an fma a column.  The groups' sums combine by a butterfly over lane distances C, 2C, ... 32.  A
//              single-chunk segment's sums go to grad_queries, times scale; a chunk of a longer one parks them in the scratch;
//   * finish   a wave per chunk the segments have too many finds its segment by a binary search and, if it is that segment's first,
//              adds its records in chunk order, a lane per column.  Not launched without grad_queries.
// Every sum has one order, fixed by the segment's length, D and heads alone: the result is bit-identical from run to run.
#include "aggregate_device.h"
#include "attention_backward_rule.h"

namespace lg {

// the chunk counts (kernels_aggregate.hip)
__global__ void aggregate_chunks_kernel(AggregateParams a, int64_t* first_chunk);

struct AttentionBackwardKernelParams {
    AttentionBackwardParams t;
    int64_t* first_chunk;           // int64[n + 1]
    float* partial;                 // float[partial_rows x record]
    int64_t partial_rows;
    int64_t record;                 // floats of a record: heads x D
    int64_t row_bytes;              // of a stored row
    int32_t units;                  // lane-units of a row
    int32_t lanes_log2;             // log2 C
};

// this lane's columns of a float32 row of D (units cl, cl + C, ...); 0 for a null row (a pad head), a unit the row does not have and
// a column past D (a bf16 row's pad)
template <int32_t U, int32_t W>
__device__ __forceinline__ void attention_lane_columns(const float* row, int32_t D, int32_t cl, int32_t C, const bool (&has)[U], float (&v)[U][W])
{
    typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
    for (int32_t u = 0; u < U; u++) {
#pragma unroll
        for (int32_t w = 0; w < W; w++) v[u][w] = 0.f;
        if (!row || !has[u]) continue;
        const int32_t col0 = (cl + C * u) * W;
        const float* r = row + col0;
        if constexpr (W >= 4) {
            if (col0 + W <= D) {
#pragma unroll
                for (int32_t w = 0; w < W; w += 4) {
                    const v4u x = *(const LG_G v4u*)(r + w);
                    v[u][w] = x.x; v[u][w + 1] = x.y; v[u][w + 2] = x.z; v[u][w + 3] = x.w;
                }
                continue;
            }
        }
#pragma unroll
        for (int32_t w = 0; w < W; w++)
            if (col0 + w < D) v[u][w] = r[w];
    }
}

// ------------------------------------------------------------------------------------------
// reduce
// ------------------------------------------------------------------------------------------
template <AggregateRow ROW, int32_t HP, int32_t U, bool QUERIES>
__global__ __launch_bounds__(LG_AGG_THREADS) void attention_backward_kernel(AttentionBackwardKernelParams p)
{
    constexpr int32_t W = aggregate_unit_width(ROW), B = attention_backward_unroll(U * W), HQ = QUERIES ? HP : 1;
    static_assert(HP * U * W <= LG_ATTB_MAX_LANE_FLOATS && U <= LG_ATT_MAX_LANE_UNITS, "the register plan (attention_backward_rule.h)");
    __shared__ uint64_t s_row[LG_AGG_WAVES][LG_AGG_K];                // 8 bytes an entry, 8 KiB a workgroup
    const AttentionBackwardParams& t = p.t;
    const AggregateParams& a = t.rows;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t C = 1 << p.lanes_log2, G = 64 >> p.lanes_log2, g = lane >> p.lanes_log2, cl = lane & (C - 1);
    const int32_t heads = t.heads;
    const bool want_q = QUERIES && t.grad_queries != nullptr;
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

        // resolve in lanes, as the forward: entries lane, lane + 64, ...
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

        // the segment's rows, this lane's columns of every head: q and dO stay, out only until delta is formed.  A pad head is zeros
        float q[HQ][U][W], gq[HQ][U][W], dO[HP][U][W], delta[HP], lse[HP];
#pragma unroll
        for (int32_t h = 0; h < HP; h++) {
            const bool real = h < heads;
            const int64_t r = (d * heads + h) * a.D;
            attention_lane_columns<U, W>(real ? t.grad_out + r : nullptr, a.D, cl, C, has, dO[h]);
            if constexpr (QUERIES) {
                attention_lane_columns<U, W>(real ? t.queries + r : nullptr, a.D, cl, C, has, q[h]);
#pragma unroll
                for (int32_t u = 0; u < U; u++)
#pragma unroll
                    for (int32_t w = 0; w < W; w++) gq[h][u][w] = 0.f;
            }
            float o[U][W], v = 0.f;
            attention_lane_columns<U, W>(real ? t.out + r : nullptr, a.D, cl, C, has, o);
#pragma unroll
            for (int32_t u = 0; u < U; u++)
#pragma unroll
                for (int32_t w = 0; w < W; w++) v = fmaf(dO[h][u][w], o[u][w], v);
            delta[h] = v;
            lse[h] = real ? t.lse[d * heads + h] : 0.f;
        }
        for (int32_t off = 1; off < C; off <<= 1) {
#pragma unroll
            for (int32_t h = 0; h < HP; h++) delta[h] += __shfl_xor(delta[h], off, 64);
        }

        // read in groups: group g takes entries g, g + G, ... in that order, B at a time
        for (int32_t i0 = 0; i0 < cnt; i0 += G * B) {                 // (the same trips for every group: the butterflies are whole)
            uint64_t row[B];
            float x[B][U][W], sc[B][HP], dt[B][HP];
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
            // the block's two dots a head: a lane's columns in order, then both cross the C lanes in one butterfly pass
            float dq[B][HQ];
#pragma unroll
            for (int32_t k = 0; k < B; k++) {
#pragma unroll
                for (int32_t h = 0; h < HP; h++) {
                    float v = 0.f, y = 0.f;
#pragma unroll
                    for (int32_t u = 0; u < U; u++) {
#pragma unroll
                        for (int32_t w = 0; w < W; w++) {
                            if constexpr (QUERIES) v = fmaf(q[h][u][w], x[k][u][w], v);
                            y = fmaf(dO[h][u][w], x[k][u][w], y);
                        }
                    }
                    if constexpr (QUERIES) dq[k][h] = v;
                    dt[k][h] = y;
                }
            }
            for (int32_t off = 1; off < C; off <<= 1) {
#pragma unroll
                for (int32_t k = 0; k < B; k++) {
#pragma unroll
                    for (int32_t h = 0; h < HP; h++) {
                        if constexpr (QUERIES) dq[k][h] += __shfl_xor(dq[k][h], off, 64);
                        dt[k][h] += __shfl_xor(dt[k][h], off, 64);
                    }
                }
            }
            // p = expf(s - lse) and dS = p (t - delta); a dead entry weighs nothing, whatever lse is.  sc becomes p, dt becomes dS
#pragma unroll
            for (int32_t k = 0; k < B; k++) {
#pragma unroll
                for (int32_t h = 0; h < HP; h++) {
                    if constexpr (QUERIES) sc[k][h] = fmaf(t.scale, dq[k][h], sc[k][h]);
                    const float pr = row[k] != 0 ? expf(sc[k][h] - lse[h]) : 0.f;
                    sc[k][h] = pr;
                    dt[k][h] = row[k] != 0 ? pr * (dt[k][h] - delta[h]) : 0.f;
                }
            }
            if (t.grad_bias && cl == 0) {
#pragma unroll
                for (int32_t k = 0; k < B; k++) {
                    const int32_t ik = i0 + g + k * G;
                    if (ik >= cnt) continue;
#pragma unroll
                    for (int32_t h = 0; h < HP; h++)
                        if (h < heads) t.grad_bias[(e0 + ik) * heads + h] = dt[k][h];
                }
            }
            // the entry's grad_rows row: the heads in order, p dO then (scale dS) q, straight from registers
            if (t.grad_rows) {
#pragma unroll
                for (int32_t k = 0; k < B; k++) {
                    const int32_t ik = i0 + g + k * G;
                    if (ik >= cnt) continue;
                    float* gr = t.grad_rows + (e0 + ik) * a.D;
                    float cs[HQ];
                    if constexpr (QUERIES) {
#pragma unroll
                        for (int32_t h = 0; h < HP; h++) cs[h] = t.scale * dt[k][h];
                    }
#pragma unroll
                    for (int32_t u = 0; u < U; u++) {
                        if (!has[u]) continue;
                        float v[W];
#pragma unroll
                        for (int32_t w = 0; w < W; w++) {
                            float y = 0.f;
#pragma unroll
                            for (int32_t h = 0; h < HP; h++) {
                                y = fmaf(sc[k][h], dO[h][u][w], y);
                                if constexpr (QUERIES) y = fmaf(cs[h], q[h][u][w], y);
                            }
                            v[w] = row[k] != 0 ? y : 0.f;
                        }
                        aggregate_store_f32<W>(gr, a.D, (cl + C * u) * W, v);
                    }
                }
            }
            if constexpr (QUERIES) {
                if (want_q) {
#pragma unroll
                    for (int32_t h = 0; h < HP; h++) {
#pragma unroll
                        for (int32_t u = 0; u < U; u++) {
#pragma unroll
                            for (int32_t w = 0; w < W; w++) {
                                float v = gq[h][u][w];
#pragma unroll
                                for (int32_t k = 0; k < B; k++) v = fmaf(dt[k][h], x[k][u][w], v);
                                gq[h][u][w] = v;
                            }
                        }
                    }
                }
            }
        }
        if constexpr (QUERIES) {
            if (want_q) {
                // the groups' sums: lane distances C, 2C, ... 32 (a + b on both sides of a pair: the same bits)
                for (int32_t off = C; off < 64; off <<= 1) {
#pragma unroll
                    for (int32_t h = 0; h < HP; h++)
#pragma unroll
                        for (int32_t u = 0; u < U; u++)
#pragma unroll
                            for (int32_t w = 0; w < W; w++) gq[h][u][w] += __shfl_xor(gq[h][u][w], off, 64);
                }
                const bool single = chunks == 1;
                const int64_t prow = aggregate_partial_row(fc, d, j);
                const bool park = !single && prow < p.partial_rows;   // (always, for non-decreasing offsets)
                if (g == 0 && (single || park)) {
                    float* rec = p.partial + prow * p.record;         // (followed only when park)
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
                                for (int32_t w = 0; w < W; w++) v[w] = gq[h][u][w] * t.scale;
                                aggregate_store_f32<W>(t.grad_queries + (d * heads + h) * a.D, a.D, col0, v);
                            } else {
                                aggregate_store_f32<W>(rec + (int64_t)h * a.D, a.D, col0, gq[h][u]);
                            }
                        }
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
// A wave per chunk a segment has too many, as aggregate_finish_kernel: the wave whose x = first_chunk[d] - d is segment d's first adds
// its records in chunk order from 0, a lane per column, and stores the sum times scale.
__global__ __launch_bounds__(LG_AGG_THREADS) void attention_backward_finish_kernel(AttentionBackwardKernelParams p)
{
    const AttentionBackwardParams& t = p.t;
    const AggregateParams& a = t.rows;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t extras = p.first_chunk[a.n] - a.n, width = (int64_t)t.heads * a.D;
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
        for (int64_t col = lane; col < width; col += 64) {            // (a record is the segment's heads x D block of grad_queries)
            float acc = 0.f;
#pragma unroll 4
            for (int64_t j = 0; j < chunks; j++) acc += rec0[j * p.record + col];        // chunk order
            t.grad_queries[d * width + col] = acc * t.scale;
        }
    }
}

// ------------------------------------------------------------------------------------------
// the launch: one kernel per row format, padded head count and units a lane holds that the register plan allows, with and without queries
// ------------------------------------------------------------------------------------------
template <AggregateRow ROW, int32_t HP, int32_t U>
static void attention_backward_launch_plan(hipStream_t s, dim3 grid, const AttentionBackwardKernelParams& p)
{
    if constexpr (HP * U * aggregate_unit_width(ROW) <= LG_ATTB_MAX_LANE_FLOATS) {
        if (p.t.queries) attention_backward_kernel<ROW, HP, U, true><<<grid, LG_AGG_THREADS, 0, s>>>(p);
        else attention_backward_kernel<ROW, HP, U, false><<<grid, LG_AGG_THREADS, 0, s>>>(p);
    }
}

template <AggregateRow ROW, int32_t HP>
static void attention_backward_launch_units(hipStream_t s, dim3 grid, const AttentionBackwardKernelParams& p)
{
    switch (attention_lane_units(p.units)) {
    case 1: attention_backward_launch_plan<ROW, HP, 1>(s, grid, p); break;
    case 2: attention_backward_launch_plan<ROW, HP, 2>(s, grid, p); break;
    case 4: attention_backward_launch_plan<ROW, HP, 4>(s, grid, p); break;
    }
}

template <AggregateRow ROW>
static void attention_backward_launch_heads(hipStream_t s, dim3 grid, const AttentionBackwardKernelParams& p)
{
    switch (attention_heads_padded(p.t.heads)) {
    case 1: attention_backward_launch_units<ROW, 1>(s, grid, p); break;
    case 2: attention_backward_launch_units<ROW, 2>(s, grid, p); break;
    case 4: attention_backward_launch_units<ROW, 4>(s, grid, p); break;
    case 8: attention_backward_launch_units<ROW, 8>(s, grid, p); break;
    }
}

// the arguments are the caller's to check (attention_backward_refusal); scratch holds attention_backward_scratch_bytes(n, M, D, heads) bytes
void launch_attention_rows_backward(hipStream_t s, const AttentionBackwardParams& t, void* scratch)
{
    const AggregateParams& a = t.rows;
    if (a.n <= 0) return;
    AttentionBackwardKernelParams p;
    p.t = t;
    p.first_chunk = static_cast<int64_t*>(scratch);
    int64_t* sums = p.first_chunk + a.n + 1;
    p.partial = reinterpret_cast<float*>(p.first_chunk + aggregate_first_words(a.n));
    p.partial_rows = aggregate_partial_rows(a.M);
    p.record = attention_backward_record_floats(a.D, t.heads);
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
    case AggregateRow::F32x4: attention_backward_launch_heads<AggregateRow::F32x4>(s, grid, p); break;
    case AggregateRow::F32x1: attention_backward_launch_heads<AggregateRow::F32x1>(s, grid, p); break;
    case AggregateRow::Bf16x8: attention_backward_launch_heads<AggregateRow::Bf16x8>(s, grid, p); break;
    }
    hipCheckError();
    if (t.grad_queries && p.partial_rows > 0) {
        const int64_t fwgs = (a.M / LG_AGG_K + LG_AGG_WAVES - 1) / LG_AGG_WAVES;      // the most chunks segments can have too many
        const dim3 fgrid((uint32_t)(fwgs < LG_AGG_MAX_WG ? fwgs : LG_AGG_MAX_WG));
        attention_backward_finish_kernel<<<fgrid, LG_AGG_THREADS, 0, s>>>(p);
        hipCheckError();
    }
}

}  // namespace lg
