// pinsage_tile.h -- what PinSAGE's two kernels share (kernels_pinsage.hip, kernels_metapath.hip), each piece once: a tile's visit slots in
// LDS and where an entry lives, the bitonic sort of every segment at once, and phases 2-5 of kernels_pinsage.hip's header comment --
// sort the visits, count the runs, sort the keys, write the k most visited -- as pinsage_rank_and_emit.  A kernel fills s_vis with
// LG_PINSAGE_EMPTY, runs its walks into it (phase 1, its own), holds the workgroup's barrier and calls pinsage_rank_and_emit; every
// lane of the workgroup makes the call.  Device code only.
#pragma once

#include "legion_core.h"

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

// phases 2-5 for the tile of `live` seeds from seed0 on, whose visits lie in s_vis: both arrays hold LG_PINSAGE_LDS_ENTRIES entries,
// 16-byte aligned; neighbors and counts are the op's outputs, int32[n x K]
template <int VPAD>
__device__ __forceinline__ void pinsage_rank_and_emit(int32_t* s_vis, int32_t* s_key, int32_t tid, int64_t seed0, int32_t live, int32_t K,
                                                      int32_t* neighbors, int32_t* counts)
{
    constexpr bool WAVE_LOCAL = VPAD <= 256;
    const int32_t elem0 = (tid >> 6) * 512 + (tid & 63); // the lane's elements: elem0 + 64 q, inside its wave's 512
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
    int32_t* nb = neighbors + seed0 * K;
    int32_t* ct = counts + seed0 * K;
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
}

}  // namespace lg
