// node_set.h -- the open-addressing table of ids (its sizes and its hash: id_table_rule.h), each piece once: the carve of the table out of
// a buffer and its clear, which unique_ids (kernels_link.hip) and the build of a vertex set (kernels_induced.hip) share (the two insert
// kernels keep their own claim loops: DESIGN.md 4.22), and the probe of a vertex set (legion_node_set_build's table,
// include/legion_hip.h), which the lookup kernel and the edge kernels of kernels_induced.hip share.  Device code and the carve; include
// inside namespace lg's files after legion_core.h.
#pragma once

#include "legion_core.h"
#include "id_table_rule.h"
#include "walk_step.h"

namespace lg {

// the table of `slots` slots at the head of a buffer of id_table_bytes(slots) bytes: keys, then first
inline IdTable id_table_carve(void* table, int64_t slots)
{
    int32_t* keys = static_cast<int32_t*>(table);
    return IdTable{.keys = keys, .first = reinterpret_cast<uint32_t*>(keys + slots), .mask = (uint32_t)(slots - 1), .shift = id_table_shift(slots)};
}

// The body of a clear kernel (a kernel of the call's own: it is captured with the rest and ordered like it): the table's 2 S words
// all-ones -- an empty key is -1, a first index nobody has lowered 0xFFFFFFFF -- and, unless null, the distinct count 0.  Its kernels
// run LG_ROW_THREADS and LG_LINK_THREADS lanes, which row_slots.h and kernels_link.hip assert equal to LG_WALK_THREADS
__device__ __forceinline__ void id_table_clear(uint32_t* table, int64_t words, int32_t* distinct)
{
    for (int64_t i = (int64_t)blockIdx.x * LG_WALK_THREADS + threadIdx.x; i < words; i += (int64_t)gridDim.x * LG_WALK_THREADS) table[i] = 0xFFFFFFFFu;
    if (distinct && blockIdx.x == 0 && threadIdx.x == 0) distinct[0] = 0;
}

// pos(v[j]) for K ids at once, their chains of dependent loads interleaved (as upper_counts<K> interleaves its searches): the first
// position of v[j] in the nodes the set was built from, -1 for v[j] < 0 (tested before any probe: a dead column entry has the bit
// pattern of the empty key and never matches it) and for a v[j] that is no member.  A chain stops at the key, at an empty key, or after
// S probes.  Whatever the table holds, nothing is read outside keys[0 .. S) and first[0 .. S), and each result lies in {-1} u [0, k).
template <int32_t K>
__device__ __forceinline__ void node_set_positions(const NodeSetView& s, const int32_t (&v)[K], int32_t (&pos)[K])
{
    uint32_t h[K];
    bool open[K], hit[K];
    bool more = false;
#pragma unroll
    for (int32_t j = 0; j < K; j++) {
        pos[j] = -1;
        hit[j] = false;
        open[j] = v[j] >= 0;
        h[j] = id_table_home(v[j], s.shift) & s.mask;                 // (below S by the shift already; the mask keeps that whatever s holds)
        more |= open[j];
    }
    if (s.wide) {
        // the table starts at a 16-byte boundary: a probe step loads the aligned group of four keys that holds h and looks at them from
        // h on, in order -- one load where up to four 4-byte loads would wait for one another (a miss at a load near one half looks at
        // 2 -- 3 slots).  S / 4 + 1 steps look at all S slots from any h on (the step past S / 4 comes back to the first group for the
        // slots below h; those from h on it has seen, and they end no chain now either): a chain stops after S slots, as key by key
        for (uint32_t trip = 0; more && trip <= (s.mask >> 2) + 1u; trip++) {
            more = false;
            int4 key[K];
#pragma unroll
            for (int32_t j = 0; j < K; j++)
                key[j] = open[j] ? *reinterpret_cast<const int4*>(s.keys + (h[j] & ~3u)) : make_int4(-1, -1, -1, -1);      // (S is a multiple of 4)
#pragma unroll
            for (int32_t j = 0; j < K; j++) {
                if (open[j]) {
                    const uint32_t base = h[j] & ~3u, from = h[j] & 3u;
                    const int32_t q[4] = {key[j].x, key[j].y, key[j].z, key[j].w};
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++) {
                        if (open[j] && c >= from) {
                            if (q[c] == v[j]) { hit[j] = true; open[j] = false; h[j] = base + c; }
                            else if (q[c] == ID_TABLE_EMPTY_KEY) open[j] = false;
                        }
                    }
                    if (open[j]) { h[j] = (base + 4u) & s.mask; more = true; }
                }
            }
        }
    } else {
        for (uint32_t probe = 0; more && probe <= s.mask; probe++) {  // at most S probes a chain
            more = false;
            int32_t key[K];
#pragma unroll
            for (int32_t j = 0; j < K; j++) key[j] = open[j] ? s.keys[h[j]] : ID_TABLE_EMPTY_KEY;
#pragma unroll
            for (int32_t j = 0; j < K; j++) {
                if (open[j]) {
                    if (key[j] == v[j]) { hit[j] = true; open[j] = false; }
                    else if (key[j] == ID_TABLE_EMPTY_KEY) open[j] = false;
                    else { h[j] = (h[j] + 1u) & s.mask; more = true; }
                }
            }
        }
    }
    uint32_t f[K];
#pragma unroll
    for (int32_t j = 0; j < K; j++) f[j] = hit[j] ? s.first[h[j]] : 0xFFFFFFFFu;
#pragma unroll
    for (int32_t j = 0; j < K; j++)
        if (f[j] < (uint32_t)s.k) pos[j] = (int32_t)f[j];             // accepted only inside [0, k)
}

}  // namespace lg
