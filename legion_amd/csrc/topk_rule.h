// topk_rule.h -- the rule of the per-row selection of the k smallest keys (legion_row_topk, legion_topk_keys, include/legion_hip.h):
// the monotone integer made of a float32 weight, the exponential variate of an entry, the three keys, which entries are eligible, which
// arguments are legal, how large the scratch is, and the two constants of the kernels a test must know.  No HIP, all constexpr:
// kernels_topk.hip evaluates this text on the device, operators.hip asks it before it enqueues anything,
// tests/cpu/topk_rule_test.cpp pins it over a literal table with g++.
// The floating point here is double, and every *, +, - and / is ONE IEEE operation rounded on its own: g++, hipcc's host pass and its
// device pass must produce the same bits, so contraction to fused multiply-adds is switched off inside each function that computes.
#pragma once

#include <cstdint>

#include "../../include/legion_hip.h"
#include "labor_rule.h"

#ifdef __clang__
#define TOPK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TOPK_NO_CONTRACT                                       // (g++ in ISO mode does not contract across statements or within them)
#endif

#define LG_TOPK_LONG 4096              // rows above this many entries get a workgroup of their own (kernels_topk.hip)
#define LG_TOPK_GRID 2048              // workgroup cap of the wave-per-row launch, four waves each: 8 192 rows a trip
#define LG_TOPK_LONG_GRID 256          // workgroups of the long-row launch: one hub row each a trip

constexpr uint32_t topk_float_bits(float w) { return __builtin_bit_cast(uint32_t, w); }
constexpr bool topk_is_nan(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

// a uint32 that orders as the float does, -0 taken as +0: negative floats reversed below the positive ones, +-inf at the ends
constexpr uint32_t topk_float_order(float w)
{
    uint32_t b = topk_float_bits(w);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the sanitise_weight rule of weighted sampling (kernels_weights.hip): finite and > 0
constexpr bool topk_weight_samples(float w) { return w > 0.0f && topk_float_bits(w) < 0x7F800000u; }

// Exp(1) from 52 hashed bits: u = (2 j + 1) 2^-53 in (0, 1), then -ln u by an exponent split and the atanh series to z^10.  frexp is
// spelled out in integers: 2 j + 1 < 2^53 converts exactly, its mantissa with the exponent of 0.5 is m in [0.5, 1).
constexpr double topk_exp_variate(uint64_t x)
{
    TOPK_NO_CONTRACT
    const uint64_t j = x >> 12;
    const double d = (double)(2 * j + 1);
    const uint64_t bits = __builtin_bit_cast(uint64_t, d);
    double m = __builtin_bit_cast(double, (bits & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull);
    int32_t ex = (int32_t)(bits >> 52) - 1075;                   // u = m 2^ex
    if (m < 0.7071067811865476) { m = 2.0 * m; ex -= 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0 / 1.0;
    return -((double)ex * 0.6931471805599453 + (2.0 * s) * p);
}

// E(e, salt): the variate of position e of col; the salt is hashed first, as LABOR's
constexpr double topk_exp_keyed(uint64_t key, int64_t e) { return topk_exp_variate(splitmix64(key ^ (uint64_t)e)); }
constexpr double topk_exp(int64_t e, int64_t salt) { return topk_exp_keyed(labor_key(salt), e); }

constexpr bool topk_mode_legal(int32_t mode) { return mode >= LEGION_TOPK_LARGEST && mode <= LEGION_TOPK_SAMPLE; }

// is the entry (src = col[e], its weight) one that can be picked?  has_w false: SAMPLE with all weights 1
constexpr bool topk_eligible(int32_t mode, int32_t src, float w, bool has_w)
{
    if (src < 0) return false;
    if (mode == LEGION_TOPK_SAMPLE) return !has_w || topk_weight_samples(w);
    return !topk_is_nan(topk_float_bits(w));
}

// the key of an eligible entry: smaller is better.  SAMPLE: a positive finite double, whose bits order as its value
constexpr uint64_t topk_key(int32_t mode, float w, uint64_t key, int64_t e)
{
    TOPK_NO_CONTRACT
    if (mode == LEGION_TOPK_LARGEST) return (uint64_t)(0xFFFFFFFFu - topk_float_order(w));
    if (mode == LEGION_TOPK_SMALLEST) return (uint64_t)topk_float_order(w);
    return __builtin_bit_cast(uint64_t, topk_exp_keyed(key, e) / (double)w);
}

// what no key equals: above every float order and every finite double
constexpr uint64_t TOPK_NO_KEY = ~0ull;

enum class TopkRefusal { Ok, Count, TooMany, KSmall, KLarge, Mode, Weights, Pointer, Scratch };

// a counter and one list position per row
constexpr int64_t topk_scratch_bytes(int32_t n)
{
    if (n < 0 || n > LEGION_IN_EDGES_MAX_ROWS) return -1;
    return 4 * ((int64_t)n + 1);
}

// what legion_row_topk checks, in this order; pointers: graph, rows, src_out and scratch are all given
constexpr TopkRefusal topk_refusal(int32_t n, int32_t k, int32_t mode, bool has_w, bool pointers, int64_t scratch_bytes)
{
    if (n < 0) return TopkRefusal::Count;
    if (n > LEGION_IN_EDGES_MAX_ROWS) return TopkRefusal::TooMany;
    if (k < 1) return TopkRefusal::KSmall;
    if (k > LEGION_TOPK_MAX_K) return TopkRefusal::KLarge;
    if (!topk_mode_legal(mode)) return TopkRefusal::Mode;
    if (!has_w && mode != LEGION_TOPK_SAMPLE) return TopkRefusal::Weights;
    if (!pointers) return TopkRefusal::Pointer;
    if (scratch_bytes < topk_scratch_bytes(n)) return TopkRefusal::Scratch;
    return TopkRefusal::Ok;
}

// what legion_topk_keys checks; pointers: graph, eids, key_out and eligible_out are all given
constexpr TopkRefusal topk_keys_refusal(int64_t n, int32_t mode, bool has_w, bool pointers)
{
    if (n < 0) return TopkRefusal::Count;
    if (n > (int64_t)0x7FFFFFFF) return TopkRefusal::TooMany;
    if (!topk_mode_legal(mode)) return TopkRefusal::Mode;
    if (!has_w && mode != LEGION_TOPK_SAMPLE) return TopkRefusal::Weights;
    if (!pointers) return TopkRefusal::Pointer;
    return TopkRefusal::Ok;
}

static_assert(LEGION_IN_EDGES_MAX_ROWS == (1 << 20) && LEGION_TOPK_MAX_K == 64, "topk_refusal_text spells the limits out; a wave holds 64 picks");
static_assert(LEGION_TOPK_LARGEST == 0 && LEGION_TOPK_SMALLEST == 1 && LEGION_TOPK_SAMPLE == 2, "topk_mode_legal is a range");
constexpr const char* topk_refusal_text(TopkRefusal r)
{
    switch (r) {
    case TopkRefusal::Ok: return "ok";
    case TopkRefusal::Count: return "n is >= 0";
    case TopkRefusal::TooMany: return "at most 2^20 rows a call (keys: 2^31 - 1 positions)";
    case TopkRefusal::KSmall: return "k is at least 1";
    case TopkRefusal::KLarge: return "k is at most 64";
    case TopkRefusal::Mode: return "mode is LEGION_TOPK_LARGEST, _SMALLEST or _SAMPLE";
    case TopkRefusal::Weights: return "only LEGION_TOPK_SAMPLE runs without weights";
    case TopkRefusal::Pointer: return "a required pointer is null";
    case TopkRefusal::Scratch: return "scratch_bytes is at least legion_row_topk_scratch_bytes(n)";
    }
    return "";
}
