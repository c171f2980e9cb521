// kernels_weights.hip -- the per-row prefix-sum table of weighted neighbour sampling (GraphStorage::SetEdgeWeights), gfx950, wave64.
//
//   edge_cdf[s + i] = (float)( sum_{j <= i} (double) w'[s + j] ),  s = indptr[v],  w'[e] = w[e] if w[e] is finite and > 0, else 0
//
// one pass over w: sanitise + a segmented inclusive scan, the sum carried in double and rounded once.  Set-up, once per graph; the
// sampler (sample_kernel<.., SampleDraw::Weighted, ..>) only reads the table.
//   * rows of up to LG_W_LONG entries: a wave per row, 64 entries per step (one coalesced 256-byte load and store), a shuffle scan
//     and a double carried from step to step.  A wave takes 64 CONSECUTIVE rows: their row pointers are one coalesced load, and
//     the rows' entries are consecutive in memory;
//   * longer rows (RMAT hubs have millions of entries) are only listed there, and a second launch gives each a workgroup of 16
//     waves: 1024 entries per step, the waves' totals combined through LDS, the same carried double.
// No thread ever walks a row alone.
// What the contract asks of the table beyond the sum (include/legion_hip.h): non-decreasing inside a row, and a zero weight repeats
// its predecessor's value (so that the pick can never land on it).  A scan's partial sums come from differently associated
// additions, so two neighbours' doubles may differ by an ulp the wrong way, and once in ~2^29 entries that straddles a float32
// rounding boundary.  Hence the second, exact, scan: a zero weight contributes 0 and every entry takes the running maximum of the
// rounded sums up to it.  Where the partial sums are exactly representable this changes nothing.
#include "legion_core.h"

#include <cmath>

namespace lg {

#define LG_W_LONG 4096                 // rows above this many entries get a workgroup of their own
#define LG_W_THREADS 256
#define LG_W_LONG_THREADS 1024
#define LG_W_LONG_WAVES (LG_W_LONG_THREADS / 64)

int64_t lg_weights_long_rows_cap(int64_t num_edges) { return num_edges / (LG_W_LONG + 1) + 1; }

__device__ __forceinline__ float sanitise_weight(float w) { return (w > 0.0f && w < INFINITY) ? w : 0.0f; }      // (NaN, -0, negatives, +-inf: 0)

__device__ __forceinline__ double wave_inclusive_sum(double v, int32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) { const double o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
__device__ __forceinline__ float wave_inclusive_max(float v, int32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_up(v, d); if (lane >= d) v = fmaxf(v, o); }
    return v;
}

__global__ __launch_bounds__(LG_W_THREADS) void edge_cdf_rows_kernel(const int64_t* __restrict__ indptr, int32_t n_rows, const float* __restrict__ w,
                                                                      float* __restrict__ cdf, int32_t* __restrict__ long_rows, int32_t long_cap)
{
    const int32_t lane = threadIdx.x & 63;
    const int32_t n_blocks = (n_rows + 63) / 64;                                  // blocks of 64 consecutive rows, one per wave and step
    const int32_t wave0 = (int32_t)(blockIdx.x * (LG_W_THREADS / 64) + (threadIdx.x >> 6));
    for (int32_t rb = wave0; rb < n_blocks; rb += (int32_t)gridDim.x * (LG_W_THREADS / 64)) {
        const int32_t r = rb * 64 + lane;
        const int64_t my_start = r < n_rows ? indptr[r] : 0;
        const int64_t my_end = r < n_rows ? indptr[r + 1] : 0;
        const int32_t n_here = min(64, n_rows - rb * 64);
        for (int32_t j = 0; j < n_here; j++) {
            const int64_t s = __shfl(my_start, j);
            const int64_t D = __shfl(my_end, j) - s;
            if (D <= 0) continue;
            if (D > LG_W_LONG) {
                if (lane == 0) {
                    const int32_t at = atomicAdd(long_rows, 1);
                    if (at < long_cap) long_rows[1 + at] = rb * 64 + j;          // (always: a listed row has more than LG_W_LONG of the E entries)
                }
                continue;
            }
            double carry = 0.0;
            float cmax = 0.0f;
            for (int64_t i0 = 0; i0 < D; i0 += 64) {
                const int64_t i = i0 + lane;
                const float x = i < D ? sanitise_weight(w[s + i]) : 0.0f;
                const double v = carry + wave_inclusive_sum((double)x, lane);
                const float m = fmaxf(cmax, wave_inclusive_max(x > 0.0f ? (float)v : 0.0f, lane));
                if (i < D) cdf[s + i] = m;
                carry = __shfl(v, 63);
                cmax = __shfl(m, 63);
            }
        }
    }
}

__global__ __launch_bounds__(LG_W_LONG_THREADS) void edge_cdf_long_rows_kernel(const int64_t* __restrict__ indptr, const float* __restrict__ w,
                                                                                float* __restrict__ cdf, const int32_t* __restrict__ long_rows, int32_t long_cap)
{
    __shared__ double s_sum[LG_W_LONG_WAVES];
    __shared__ float s_max[LG_W_LONG_WAVES];
    const int32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t n_long = min(long_rows[0], long_cap);
    for (int32_t k = blockIdx.x; k < n_long; k += gridDim.x) {
        const int32_t row = long_rows[1 + k];
        const int64_t s = indptr[row];
        const int64_t D = indptr[row + 1] - s;
        double carry = 0.0;
        float cmax = 0.0f;
        for (int64_t i0 = 0; i0 < D; i0 += LG_W_LONG_THREADS) {
            const int64_t i = i0 + tid;
            const float x = i < D ? sanitise_weight(w[s + i]) : 0.0f;
            double v = wave_inclusive_sum((double)x, lane);
            if (lane == 63) s_sum[wave] = v;
            __syncthreads();
            double base = carry, total = carry;              // every thread adds the waves' totals in the same order: one carry for all
            for (int32_t o = 0; o < LG_W_LONG_WAVES; o++) {
                total += s_sum[o];
                if (o + 1 == wave) base = total;
            }
            v += base;
            float m = wave_inclusive_max(x > 0.0f ? (float)v : 0.0f, lane);
            if (lane == 63) s_max[wave] = m;
            __syncthreads();
            float mbase = cmax, mtotal = cmax;
            for (int32_t o = 0; o < LG_W_LONG_WAVES; o++) {
                mtotal = fmaxf(mtotal, s_max[o]);
                if (o + 1 == wave) mbase = mtotal;
            }
            m = fmaxf(m, mbase);
            if (i < D) cdf[s + i] = m;
            carry = total;
            cmax = mtotal;
            __syncthreads();                                 // (the next step writes s_sum / s_max again)
        }
    }
}

void build_edge_cdf(hipStream_t s, const int64_t* indptr, int32_t n_rows, const float* w, float* cdf, int32_t* long_rows, int32_t long_cap)
{
    if (n_rows <= 0) return;
    HIP_CALL(hipMemsetAsync(long_rows, 0, sizeof(int32_t), s));
    const int32_t n_blocks = (n_rows + 63) / 64;
    int32_t grid = (n_blocks + LG_W_THREADS / 64 - 1) / (LG_W_THREADS / 64);
    if (grid > 8192) grid = 8192;
    edge_cdf_rows_kernel<<<grid, LG_W_THREADS, 0, s>>>(indptr, n_rows, w, cdf, long_rows, long_cap);
    hipCheckError();
    edge_cdf_long_rows_kernel<<<512, LG_W_LONG_THREADS, 0, s>>>(indptr, w, cdf, long_rows, long_cap);
    hipCheckError();
}

}  // namespace lg
