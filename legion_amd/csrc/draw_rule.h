// draw_rule.h -- the sampler's draw, shared by its kernels (kernels_sample.hip) and the random walk (kernels_walk.hip): the
// table-driven minstd power, the uniform pick, the weighted pick's target and search step, and the distinct picks' draw and
// resolution (Floyd's algorithm: the sampler alone uses it).  Device code only; every source that
// includes it carries its own copy of the power tables (20 KiB of constant device memory).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lg {

// ------------------------------------------------------------------------------------------
// minstd_rand (48271^n mod 2^31-1) by three power tables: n = n0 + 2^11 n1 + 2^22 n2.
// ------------------------------------------------------------------------------------------
static constexpr uint32_t kM31 = 2147483647u;

__host__ __device__ constexpr uint32_t mulmod31(uint32_t a, uint32_t b)
{
    uint64_t p = (uint64_t)a * (uint64_t)b;           // < 2^62
    uint64_t s = (p & kM31) + (p >> 31);              // 2^31 == 1 (mod M)  -> < 2^32
    s = (s & kM31) + (s >> 31);                       // <= 2^31
    return (uint32_t)(s >= kM31 ? s - kM31 : s);
}

struct PowTables {
    uint32_t t0[2048];   // 48271^i
    uint32_t t1[2048];   // 48271^(i * 2^11)
    uint32_t t2[1024];   // 48271^(i * 2^22)
};

static constexpr PowTables make_pow_tables()
{
    PowTables t{};
    uint32_t v = 1;
    for (int i = 0; i < 2048; i++) { t.t0[i] = v; v = mulmod31(v, 48271u); }
    const uint32_t step1 = v;                          // 48271^2048
    v = 1;
    for (int i = 0; i < 2048; i++) { t.t1[i] = v; v = mulmod31(v, step1); }
    const uint32_t step2 = v;                          // 48271^(2^22)
    v = 1;
    for (int i = 0; i < 1024; i++) { t.t2[i] = v; v = mulmod31(v, step2); }
    return t;
}

static __device__ const PowTables g_pow = make_pow_tables();

__device__ __forceinline__ uint32_t minstd_pow(uint32_t n)
{
    uint32_t x = mulmod31(g_pow.t0[n & 2047u], g_pow.t1[(n >> 11) & 2047u]);
    return mulmod31(x, g_pow.t2[n >> 22]);
}

// thrust::uniform_int_distribution<int>(0, deg-1) over minstd_rand, see oracle/legion_oracle.c.
__device__ __forceinline__ int32_t draw_from_x(uint32_t x, int32_t deg)
{
    double r = (double)(uint32_t)(x - 1u);
    r /= 2147483646.0;                                 // IEEE divide (no fast-math in this build)
    return (int32_t)(r * (((double)(deg - 1) + 1.0) - 0.0) + 0.0);
}

// ------------------------------------------------------------------------------------------
// Weighted sampling (SampleMode::weighted == 1, DGL's prob=; with replacement).  cdf is the graph's prefix-sum table (kernels_weights.hip):
// per row the inclusive sums of the sanitised weights, float32, indexed like the full CSR's column array.  Slot idx of a row
// {s, D} with total T = cdf[s + D - 1]:  t = r * (double)T with the r of draw_from_x, and
//   pick = #{ i in [0, D) : (double)cdf[s + i] <= t }
// an upper-bound binary search, ceil(log2(D + 1)) dependent 4-byte loads.  t < T, so pick <= D - 1, and cdf[pick] > t >= cdf[pick - 1]:
// an entry of weight zero is never drawn.  T == 0: the row yields no edge.  With unit weights (D < 2^24) cdf[s + i] = i + 1 and the
// pick is floor(r * D): draw_from_x.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double weighted_target(uint32_t x, float total)      // x = minstd_pow(idx + 1)
{
    double r = (double)(uint32_t)(x - 1u);
    r /= 2147483646.0;
    return r * (double)total;
}
// one probe of the search over [lo, lo + n): the entry at lo + n / 2 is v
__device__ __forceinline__ void weighted_step(float v, double t, int32_t& lo, int32_t& n)
{
    const int32_t half = n >> 1;
    if ((double)v <= t) { lo += half + 1; n -= half + 1; }
    else n = half;
}

// ------------------------------------------------------------------------------------------
// Sampling without replacement (SampleMode::replace == 0, DGL's replace=False).  Frontier entry q of a hop with fan-out f owns
// slots q*f + k, k < f, as with replacement; its row of degree D yields min(f, D) picks:
//   D <= f: position k (every neighbour in CSR order, no draw);
//   D >  f: Floyd's algorithm in slot order -- t_k = draw(q*f + k, j_k + 1) with j_k = D - f + k, and pick_k = t_k unless one
//           of pick_0 .. pick_{k-1} took it, then j_k.  A uniform f-subset of [0, D): distinct adjacency positions.
// The draws are independent (one per slot, in parallel); only the resolution is serial per entry, ~f^2/2 comparisons.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t floyd_draw(uint32_t x, int32_t deg, int32_t f, int32_t k)      // t_k from slot's x = minstd_pow(idx + 1)
{
    return draw_from_x(x, deg - f + k + 1);
}

// the picks of one entry with D > f: p[0 .. n) hold t_0 .. t_{n-1} and are replaced, in place, by pick_0 .. pick_{n-1}
// (n <= f: a super tile resolves the slots it owns and those before them; later picks never change earlier ones)
template <typename T>
__device__ __forceinline__ void floyd_resolve(T* p, int32_t n, int32_t jbase)                      // jbase = D - f
{
    for (int32_t k = 1; k < n; k++) {
        const int32_t t = p[k];
        bool taken = false;
        for (int32_t i = 0; i < k; i++) taken |= (p[i] == t);
        if (taken) p[k] = jbase + k;
    }
}

}  // namespace lg
