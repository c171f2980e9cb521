// kernels_gather.hip -- feature-cache lookup + row gather for gfx950.
//
// Computes what multiGPU_feat_cache_lookup does (SS/cache/cache_impl.cuh:239-272, launched from
// SS/cache/cache.cu:726-748) with PreSCCacheController::FindFeat (SS/cache/cache.cu:180-215)
// fused in front of it: for row r of the current new-node range
//     id = sampled_ids[off + r];  g = node_map[id] (or -2)          -> cache_index[r] = g
//     g <  0 : dst[off + r] = full_table[id % N]                    (miss: full table tier)
//     g >= 0 : dst[off + r] = cache_tables[g / cap][g % cap]        (hit: local or peer HBM)
// and, with GatherParams.hybrid, what feat_cache_lookup does (SS/cache/cache_impl.cuh:202-235):
//     0 <= g < cpu_cap : dst[off + r] = cpu_cache[g]                (hit in the mapped pinned CPU cache)
//     g >= cpu_cap     : dst[off + r] = gpu_cache[(g - cpu_cap) % gpu_cap]
//     g <  0           : left to the storage tier (the full table when one is bound, else the row is not written)
// Rows are copied verbatim (byte-identical, no arithmetic), or converted by the row format (GatherRow below).
//
// The reference runs one thread per float on a fixed 32x1024 grid with a 64-bit div/mod per
// element.  Here a workgroup owns a tile of ROWS consecutive output rows (gather_plan.h): ROWS lanes resolve the
// tile's ids to source row pointers once (the id->slot table is direct mapped, one 4-byte read)
// and park them in LDS; then all 256 lanes stream the tile as 16-byte chunks, four independent
// loads in flight per lane, so that consecutive lanes read consecutive 16 B of one source row
// and write consecutive 16 B of the (contiguous) destination.  No divides in the copy loop.
//
// Roofline: HBM.  Algorithmic bytes per row = 8*D + 8 for float32 rows (D*4 read + D*4 written + id + index); the bf16 formats'
// are on their GatherRow.
#include "legion_core.h"
#include "gather_plan.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace lg {

#define LG_GATHER_THREADS 256

// ------------------------------------------------------------------------------------------
// Hand-over of a finished mini-batch from a lane of a launch group to one of the two trainer-visible pipe
// slots (SS/engine/ipc_service.cu:134-211: ids, labels, agg_src, agg_dst, node_counter, edge_counter; the
// feature rows are gathered straight into the slot by gather_kernel).  Sizes come from the lane's counters on
// the device.  The counters also go to the slot's host-visible mirror (ipc_env.hip), with node_counter[2..3]
// already holding what the last gather op leaves there (counter_update(op%3==1), operator_impl.cu:83-85).
// ------------------------------------------------------------------------------------------
// slice `part` of `parts` of the hand-over, done by one workgroup (all of it when parts == 1)
__device__ __forceinline__ void deliver_slice(const LanePtrs& L, const DeliverParams& d, int32_t part, int32_t parts)
{
    const LG_G int32_t* nc = LG_GPTR(const int32_t, L.node_counter);
    const LG_G int32_t* ec = LG_GPTR(const int32_t, L.edge_counter);
    const LG_G int32_t* hs = LG_GPTR(const int32_t, L.hop_scratch);
    const int32_t hop_num = nc[INTRABATCH_CON * 3 - 1];
    int32_t n = nc[INTRABATCH_CON * 3 + hop_num], e = ec[INTRABATCH_CON * 3 + hop_num], b = nc[INTRABATCH_CON * 3];
    n = n < 0 ? 0 : (n > d.num_ids ? d.num_ids : n);
    e = e < 0 ? 0 : (e > d.num_ids ? d.num_ids : e);
    b = b < 0 ? 0 : (b > d.batch_cap ? d.batch_cap : b);
    const int32_t tid = threadIdx.x, nthr = blockDim.x;
    typedef int32_t v4 __attribute__((ext_vector_type(4)));
    auto copy = [&](const int32_t* src, int32_t* dst, int32_t count) {
        const int32_t per = (((count + parts - 1) / parts) + 3) & ~3;     // slices start 16-byte aligned
        const int32_t lo = part * per, hi = min(lo + per, count);
        if (lo >= hi) return;
        const LG_G v4* s4 = (const LG_G v4*)(src + lo);
        LG_G v4* d4 = (LG_G v4*)(dst + lo);
        const int32_t q = (hi - lo) >> 2;
        for (int32_t i = tid; i < q; i += nthr) d4[i] = s4[i];
        for (int32_t i = lo + (q << 2) + tid; i < hi; i += nthr) LG_GPTR(int32_t, dst)[i] = LG_GPTR(const int32_t, src)[i];
    };
    copy(L.sampled_ids, d.sampled_ids, n);
    copy(L.agg_src_off, d.agg_src_off, e);
    copy(L.agg_dst_off, d.agg_dst_off, e);
    copy(L.labels, d.labels, b);
    if (part == 0 && tid < 32) {
        int32_t v = tid < 16 ? nc[tid] : ec[tid - 16];
        if (tid == 2) v = hs[HS_RANGE + 2 * hop_num];
        if (tid == 3) v = hs[HS_RANGE + 2 * hop_num + 1];
        LG_GPTR(int32_t, tid < 16 ? d.node_counter : d.edge_counter)[tid & 15] = v;
        if (d.mirror != nullptr) LG_GPTR(int32_t, d.mirror)[tid] = v;      // host memory: visible once the batch's event completed
    }
}

__global__ __launch_bounds__(256) void deliver_kernel(const LanePtrs* __restrict__ lane_p, DeliverParams d)
{
    deliver_slice(*lane_p, d, blockIdx.x, gridDim.x);
}

void launch_deliver(hipStream_t s, const LanePtrs* d_lane, const DeliverParams& d)
{
    int32_t grid = (d.num_ids / 4 + 1023) / 1024;
    if (grid > 512) grid = 512;
    if (grid < 1) grid = 1;
    deliver_kernel<<<grid, 256, 0, s>>>(d_lane, d);
    hipCheckError();
}

// Row formats (gather_plan.h): gather_kernel<VecT, ROWS, UNROLL, TAIL, LASTOP> takes the loads and stores of its rows from
// GatherRow<VecT, TAIL>, keyed on its own template arguments so that the instances keep their names.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// float32 -> float32 (F32, F32Tail: VecT = f32x4; F32Scalar: float), rows copied verbatim.  F32Tail (D = 602: 2408-byte rows) moves
// the same 16 bytes per lane at 4-byte alignment -- gfx950 global loads / stores of 16 bytes need dword alignment only; the compiler
// emits global_load_dwordx4 for both -- and the D % 4 trailing floats of each row in the kernel's TAIL pass (0.65 of peak at D = 602,
// instead of the 8- / 4-byte vector paths of rounds 1-2).  Its VecT is F32's: an aligned(4) typedef does not survive as a template
// argument (both mangle as Dv4_f), so TAIL alone tells the two apart.
template <typename VecT, bool TAIL> struct GatherRow {
    static_assert(std::is_same<VecT, f32x4>::value || std::is_same<VecT, float>::value, "float32 rows; bf16 rows have no TAIL pass");
    typedef float Out;
    static __device__ int32_t chunks(const GatherParams& gp) { return gp.D / (int32_t)(sizeof(VecT) / sizeof(float)); }
    static __device__ const LG_G float* row_at(const GatherParams& gp, const float* base, int64_t x) { return LG_GPTR(const float, base) + x * gp.D; }
    static __device__ VecT load(const LG_G float* p, bool, LG_G float* dst_tile, int32_t r, int32_t c, int32_t D)
    {
        if (p == nullptr) p = dst_tile + (int64_t)r * D;     // id < 0: nothing to fetch; read what is there
        return ((const LG_G VecT*)p)[c];      // plain loads: measured 74% of HBM peak vs 63% nontemporal
    }
    static __device__ void store(const VecT& v, bool ok, LG_G float* dst_tile, int32_t r, int32_t c, int32_t D)
    {
        if (ok) __builtin_nontemporal_store(v, (LG_G VecT*)(dst_tile + (int64_t)r * D) + c);     // write-once output: nontemporal stores
    }
};

// bf16 source rows (LEGION_FEATURE_BF16 storage) of pitch P: 16 bytes = 8 elements per chunk.  A missing row loads a 16-byte zero line
// instead of the destination (a destination row of D < 4 is shorter than a chunk).
struct Bf16x8 {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    u4 w;
};
struct Bf16Copy : Bf16x8 {};
__device__ __attribute__((aligned(16))) Bf16x8 lg_gather_zero_line;
template <typename VecT, typename OutT> struct GatherRowBf16Src {
    typedef OutT Out;
    static __device__ int32_t chunks(const GatherParams& gp) { return gp.pitch / 8; }
    static __device__ const LG_G float* row_at(const GatherParams& gp, const float* base, int64_t x)
    {
        return (const LG_G float*)(LG_GPTR(const uint16_t, (const uint16_t*)base) + x * gp.pitch);
    }
    static __device__ VecT load(const LG_G float* p, bool has, LG_G Out*, int32_t, int32_t c, int32_t)
    {
        VecT v;
        v.w = has ? ((const LG_G VecT*)p)[c].w : LG_GPTR(const Bf16x8, &lg_gather_zero_line)->w;
        return v;
    }
};

// bf16 -> float32: a chunk's 8 elements widened to 32 bytes of float32 (bits << 16, exact) and stored as two dword-aligned 16-byte
// stores -- output rows are 4*D bytes, so at any D they are only dword aligned, as in F32Tail.  The last chunk of a row with D % 8 != 0
// stores its first D % 8 elements one by one (the source's pad elements are never stored), so every D takes the same instance and no
// TAIL pass.  Algorithmic bytes per row 2*P + 4*D + 8, P = D rounded up to 8.
template <> struct GatherRow<Bf16x8, false> : GatherRowBf16Src<Bf16x8, float> {
    static __device__ void store(const Bf16x8& v, bool ok, LG_G float* dst_tile, int32_t r, int32_t c, int32_t D)
    {
        typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
        typedef Bf16x8::u4 u4;
        const u4 lo = v.w << 16, hi = v.w & 0xFFFF0000u;      // elements 2k, 2k+1 of the chunk
        const int32_t e0 = c * 8;
        LG_G float* d = dst_tile + (int64_t)r * D + e0;
        if (ok && e0 + 8 <= D) {
            __builtin_nontemporal_store(__builtin_bit_cast(v4u, u4{lo.x, hi.x, lo.y, hi.y}), (LG_G v4u*)d);
            __builtin_nontemporal_store(__builtin_bit_cast(v4u, u4{lo.z, hi.z, lo.w, hi.w}), (LG_G v4u*)d + 1);
        } else if (ok) {                               // the partial last chunk of a row: D - e0 < 8 elements
            const uint32_t f[8] = {lo.x, hi.x, lo.y, hi.y, lo.z, hi.z, lo.w, hi.w};
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (e0 + k < D) d[k] = __uint_as_float(f[k]);
        }
    }
};

// bf16 OUTPUT rows (GatherParams.out_dtype = LEGION_FEATURE_BF16): D elements per row, stride D, no pad; a chunk is 8 elements, 16
// bytes of output, w[k] its elements 2k (low half) and 2k+1 (high half).  Output rows are 2*D bytes: with D even a full chunk is one
// dword-aligned 16-byte store (16-byte aligned when D % 8 == 0), a partial one stores its dwords one by one; with D odd rows are only
// 2-byte aligned and every element is stored on its own (correct, not fast).
__device__ __forceinline__ void gather_store_bf16(const uint32_t (&w)[4], bool ok, LG_G uint16_t* dst_tile, int32_t r, int32_t c, int32_t D)
{
    typedef uint32_t u4u __attribute__((ext_vector_type(4), aligned(4)));
    const int32_t e0 = c * 8;
    LG_G uint16_t* d = dst_tile + (int64_t)r * D + e0;
    if (ok && (D & 1) == 0) {                      // dword-aligned rows
        if (e0 + 8 <= D) {
            __builtin_nontemporal_store(u4u{w[0], w[1], w[2], w[3]}, (LG_G u4u*)d);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e0 + 2 * k < D) ((LG_G uint32_t*)d)[k] = w[k];
        }
    } else if (ok) {                               // odd D: 2-byte aligned rows
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (e0 + k < D) d[k] = (uint16_t)(w[k >> 1] >> ((k & 1) * 16));
    }
}

// bf16 -> bf16: the stored bits copied verbatim (16-byte load, 16-byte store).  A missing row stores nothing.  Algorithmic bytes per
// row 2*P + 2*D + 8.
template <> struct GatherRow<Bf16Copy, false> : GatherRowBf16Src<Bf16Copy, uint16_t> {
    static __device__ void store(const Bf16Copy& v, bool ok, LG_G uint16_t* dst_tile, int32_t r, int32_t c, int32_t D)
    {
        gather_store_bf16({v.w.x, v.w.y, v.w.z, v.w.w}, ok, dst_tile, r, c, D);
    }
};
// torch's float32 -> bfloat16 rounding (kernels_cache.hip bf16_rne_bits: round to nearest even, NaNs kept quiet NaNs)
__device__ __forceinline__ uint32_t gather_bf16_rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// float32 -> bf16: a source row of D floats, two dword-aligned 16-byte loads per chunk narrowed with gather_bf16_rne (the integer
// path of convert_f32_to_bf16_kernel, not v_cvt_pk_bf16_f32).  A row's partial last chunk loads only its D % 8 floats, as the row may
// be the table's last.  A missing row loads zeros and stores nothing.  Algorithmic bytes per row 6*D + 8.
struct F32Narrow {
    typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
    v4u a, b;
};
template <> struct GatherRow<F32Narrow, false> {
    typedef uint16_t Out;
    typedef F32Narrow::v4u v4u;
    static __device__ int32_t chunks(const GatherParams& gp) { return (gp.D + 7) / 8; }
    static __device__ const LG_G float* row_at(const GatherParams& gp, const float* base, int64_t x) { return LG_GPTR(const float, base) + x * gp.D; }
    static __device__ F32Narrow load(const LG_G float* p, bool, LG_G uint16_t*, int32_t, int32_t c, int32_t D)
    {
        F32Narrow v;
        const int32_t e0 = c * 8;
        if (p == nullptr) {
            v.a = v.b = v4u{0.f, 0.f, 0.f, 0.f};
        } else if (e0 + 8 <= D) {
            v.a = ((const LG_G v4u*)(p + e0))[0];
            v.b = ((const LG_G v4u*)(p + e0))[1];
        } else {                                          // the partial last chunk: no load past the row's end
            float f[8];
#pragma unroll
            for (int k = 0; k < 8; k++) f[k] = e0 + k < D ? p[e0 + k] : 0.f;
            v.a = v4u{f[0], f[1], f[2], f[3]};
            v.b = v4u{f[4], f[5], f[6], f[7]};
        }
        return v;
    }
    static __device__ void store(const F32Narrow& v, bool ok, LG_G uint16_t* dst_tile, int32_t r, int32_t c, int32_t D)
    {
        gather_store_bf16({gather_bf16_rne(v.a.x) | (gather_bf16_rne(v.a.y) << 16), gather_bf16_rne(v.a.z) | (gather_bf16_rne(v.a.w) << 16),
                           gather_bf16_rne(v.b.x) | (gather_bf16_rne(v.b.y) << 16), gather_bf16_rne(v.b.z) | (gather_bf16_rne(v.b.w) << 16)},
                          ok, dst_tile, r, c, D);
    }
};

// A workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its lane and keeps the walk software-pipelined: while
// tile t is being copied, the first ROWS threads already hold the ids of tile t+1 (loaded one step earlier), have its
// slot lookups (node_map[id], the one scattered read of the resolve) in flight together with the copy's loads, and fetch the
// ids of tile t+2.  The copy of a tile therefore never waits for its own resolve chain (id -> slot -> pointer): with one tile
// per workgroup that chain was 40 % of a workgroup's life during which it streamed nothing.  Loads of the copy loop are
// unconditional (a missing row loads what its format says, chunks past the tile's end re-read its last chunk), so no
// branch sits between the prefetch and the copy and all of them are in flight together; only the stores are predicated.
#ifndef LG_GATHER_MIN_WAVES
#define LG_GATHER_MIN_WAVES 8        // waves per SIMD the register allocation must leave room for
#endif
#ifndef LG_GATHER_TARGET_WG
#define LG_GATHER_TARGET_WG 8192     // workgroups of a full launch: four rounds of what is resident, so the dispatcher evens out lanes of different length
#endif

// LASTOP: the gather of a batch's last op (the dominant launch; traces and counters tell it from the early hops' gathers by
// name) -- the only one that can carry a hand-over to a trainer-visible pipe slot.
template <typename VecT, int ROWS, int UNROLL, bool TAIL, bool LASTOP>
__global__ __launch_bounds__(LG_GATHER_THREADS, LG_GATHER_MIN_WAVES) void gather_kernel(GatherParams gp, const LanePtrs* __restrict__ lanes,
                                                                   bool copy_range)
{
    typedef GatherRow<VecT, TAIL> Row;
    typedef typename Row::Out Out;
    constexpr int VEC = sizeof(VecT) / sizeof(float);
    static_assert(ROWS <= LG_GATHER_THREADS, "one resolving thread per row of a tile");
    __shared__ const LG_G float* s_ptr[2][ROWS];

    const LanePtrs& L = lanes[blockIdx.y];
    // {offset, count} of the new-node range: the live counters, or the per-hop snapshot
    const LG_G int32_t* range = LG_GPTR(const int32_t, gp.hop >= 0 ? L.hop_scratch + HS_RANGE + 2 * gp.hop : L.node_counter);
    const LG_G int32_t* sampled_ids = LG_GPTR(const int32_t, L.sampled_ids);
    const LG_G int32_t* node_slot = (L.node_slot != nullptr && gp.node_map != nullptr) ? LG_GPTR(const int32_t, L.node_slot) : nullptr;
    LG_G int32_t* cache_search_buffer = LG_GPTR(int32_t, L.cache_search_buffer);
    int32_t off = range[0];
    int32_t rows = range[1];
    if (copy_range && blockIdx.x == 0 && threadIdx.x == 0) {   // counter_update(op%3==1), operator_impl.cu:83-85
        LG_GPTR(int32_t, L.node_counter)[2] = off;
        LG_GPTR(int32_t, L.node_counter)[3] = rows;
    }
    if (gp.hop >= 0 && gp.first_hop < gp.hop) {                // earlier hops' ranges ride along (adjacent rows)
        const int32_t off0 = LG_GPTR(const int32_t, L.hop_scratch)[HS_RANGE + 2 * gp.first_hop];
        rows += off - off0;
        off = off0;
    }
    if (rows > gp.max_rows) rows = gp.max_rows;
    if (rows > L.feature_rows - off) {     // never write past the feature buffer (the reference sizes it 1.2 x the PreSC
        rows = L.feature_rows - off;       // maximum and would overrun, SS/engine/server.cu:277): stop at its end and say so
        if (blockIdx.x == 0 && threadIdx.x == 0 && L.hop_scratch != nullptr) {
            __hip_atomic_fetch_or(LG_GPTR(int32_t, L.hop_scratch) + HS_ERROR, LG_ERR_FEATURE_ROWS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (L.err_flag) __hip_atomic_fetch_or(LG_GPTR(int32_t, L.err_flag), LG_ERR_FEATURE_ROWS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const int32_t ntiles = (rows + ROWS - 1) / ROWS;
    const int32_t step = gridDim.x;
    if (LASTOP && L.deliver != nullptr)        // this lane's gather also hands the batch over to a pipe slot: every workgroup a slice
        deliver_slice(L, *static_cast<const DeliverParams*>(L.deliver), blockIdx.x, step);
    const int32_t tid = threadIdx.x;
    const int32_t D = gp.D;
    const int32_t C = Row::chunks(gp);
    const int32_t dr = LG_GATHER_THREADS / C;          // row / chunk advance per 256-chunk step
    const int32_t dc = LG_GATHER_THREADS - dr * C;
    int32_t tile = blockIdx.x;
    if (tile >= ntiles) return;                        // (surplus workgroups of a short lane)

    // row-source statistics: armed by the host (UnifiedCache::GatherStats) and switched by a DEVICE word, so that a launch
    // captured in a hipGraph follows the switch too (a pointer baked in at capture time kept counting through every replay)
    const bool counting = gp.stats != nullptr && gp.Kg > 1 && gp.stats[3] != 0ull;
    // a row's source: FindFeat (cache.cu:180-215) + the address arithmetic of cache_impl.cuh:259-268
    auto source_of = [&](int32_t id, int32_t g) -> const LG_G float* {
        const LG_G float* p = nullptr;
        if (g < 0) {
            if (id >= 0 && gp.full_table != nullptr)     // :262-266 (the modulo only where it does anything)
                p = Row::row_at(gp, gp.full_table, (int64_t)(id < gp.total_num_nodes ? id : id % gp.total_num_nodes));
        } else if (gp.hybrid) {      // feat_cache_lookup, cache_impl.cuh:224-231: CPU cache below cpu_cap, this GPU's cache above
            if (g < gp.hybrid_cpu_cap)
                p = Row::row_at(gp, gp.hybrid_cpu_cache, (int64_t)g);       // (g % cpu_cap == g)
            else
                p = Row::row_at(gp, gp.local_table, (int64_t)((g - gp.hybrid_cpu_cap) % gp.hybrid_gpu_cap));
        } else {
            int32_t didx = 0, fidx = g;                                                      // :259-260 (one division, and
            if (gp.striped) { didx = g / gp.node_capacity; fidx = g - didx * gp.node_capacity; }  // none without striping)
            const int64_t rank = (int64_t)fidx * gp.Kg + didx;                               // hotness rank of the row (cache_impl.cuh:104-109)
            const bool local_copy = gp.replica != nullptr && rank < gp.replica_rows;
            if (local_copy)      // the clique's hottest rows are also kept locally: same row, no xGMI hop
                p = Row::row_at(gp, gp.replica, rank);
            else if (didx == gp.member && gp.local_table != nullptr)     // own stripe: its address came with the launch
                p = Row::row_at(gp, gp.local_table, (int64_t)fidx);
            else if (gp.skip_remote)     // peer_gather = bulk: the owner pushes this row (bulk_push_kernel); nothing to fetch here
                p = nullptr;
            else
                p = Row::row_at(gp, gp.cache_tables[didx], (int64_t)fidx);                  // :268
            if (counting) {    // tests / diagnostics / the computed xGMI count: [0] rows read through a stripe pointer, [1] from the
                               // replica, [2] the part of [0] from a peer's stripe -- one atomic per wave and counter
                const unsigned long long m_rep = __ballot(local_copy), m_str = __ballot(!local_copy);
                const unsigned long long m_peer = __ballot(!local_copy && didx != gp.member);
                if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)(m_rep | m_str)) - 1) {
                    if (m_str) atomicAdd(gp.stats + 0, (unsigned long long)__popcll(m_str));
                    if (m_rep) atomicAdd(gp.stats + 1, (unsigned long long)__popcll(m_rep));
                    if (m_peer) atomicAdd(gp.stats + 2, (unsigned long long)__popcll(m_peer));
                }
            }
        }
        return p;
    };
    // the row's feature-cache slot: carried from the sampler where the column slots are in use (a coalesced read), else --
    // seeds, rows sampled from a cached-topology CSR, no column slots -- the FindFeat lookup (a 128-byte line per row)
    auto lookup = [&](int32_t id, int32_t carried) -> int32_t {
        if (carried != LG_FS_UNKNOWN) return carried;
        return (gp.node_map != nullptr && id >= 0) ? gp.node_map[id] : CACHEMISS_FLAG;
    };

    // prologue: this workgroup's first tile resolved, the second tile's ids in hand
    int32_t id_n = -1, fs_n = LG_FS_UNKNOWN;           // ids / carried slots of the NEXT tile (threads < ROWS)
    bool have_n = false;
    if (tid < ROWS) {
        const int32_t r = tile * ROWS + tid;
        if (r < rows) {
            const int32_t id = sampled_ids[off + r];
            const int32_t g = lookup(id, node_slot != nullptr ? node_slot[off + r] : LG_FS_UNKNOWN);
            cache_search_buffer[r] = g;                // FindFeat writes from index 0 each hop
            s_ptr[0][tid] = source_of(id, g);
        }
        const int32_t rn = (tile + step) * ROWS + tid;
        have_n = tile + step < ntiles && rn < rows;
        if (have_n) {
            id_n = sampled_ids[off + rn];
            if (node_slot != nullptr) fs_n = node_slot[off + rn];
        }
    }
    __syncthreads();

    int buf = 0;
    for (; tile < ntiles; tile += step) {
        const int32_t r0 = tile * ROWS;
        const int32_t nr = min(ROWS, rows - r0);
        // resolve of the next tile: its one scattered read goes out before the copy's loads; the ids of the tile after it too
        int32_t g_n = CACHEMISS_FLAG, id_nn = -1, fs_nn = LG_FS_UNKNOWN;
        bool have_nn = false;
        if (tid < ROWS) {
            if (have_n) g_n = lookup(id_n, fs_n);
            const int32_t rnn = (tile + 2 * step) * ROWS + tid;
            have_nn = tile + 2 * step < ntiles && rnn < rows;
            if (have_nn) {
                id_nn = sampled_ids[off + rnn];
                if (node_slot != nullptr) fs_nn = node_slot[off + rnn];
            }
        }

        const int32_t nchunks = nr * C;
        LG_G Out* dst_tile = LG_GPTR(Out, (Out*)L.float_features) + (int64_t)(off + r0) * D;
        int32_t q = tid;
        int32_t r = q / C;
        int32_t c = q - r * C;
        while (q < nchunks) {
            VecT v[UNROLL];
            int32_t rr[UNROLL], cc[UNROLL];
            bool ok[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const bool in = q < nchunks;
                rr[u] = in ? r : nr - 1;               // past the end: the tile's last chunk again (loaded, not stored)
                cc[u] = in ? c : C - 1;
                const LG_G float* p = s_ptr[buf][rr[u]];
                ok[u] = in && p != nullptr;
                v[u] = Row::load(p, p != nullptr, dst_tile, rr[u], cc[u], D);
                q += LG_GATHER_THREADS;
                r += dr;
                c += dc;
                if (c >= C) { c -= C; r += 1; }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) Row::store(v[u], ok[u], dst_tile, rr[u], cc[u], D);
        }
        if constexpr (TAIL) {            // the last D % VEC floats of every row
            const int32_t tail = D - C * VEC;
            for (int32_t i = tid; i < nr * tail; i += LG_GATHER_THREADS) {
                const int32_t tr = i / tail, k = C * VEC + (i - tr * tail);
                const LG_G float* p = s_ptr[buf][tr];
                if (p != nullptr) dst_tile[(int64_t)tr * D + k] = p[k];
            }
        }
        if (tid < ROWS && have_n) {
            cache_search_buffer[(tile + step) * ROWS + tid] = g_n;
            s_ptr[buf ^ 1][tid] = source_of(id_n, g_n);
        }
        id_n = id_nn;
        fs_n = fs_nn;
        have_n = have_nn;
        __syncthreads();
        buf ^= 1;
    }
}

// ------------------------------------------------------------------------------------------
// peer_gather = bulk, requester side: every row of the group's batches that is a hit in ANOTHER member's stripe (and not in the
// local replica) is listed for its owner -- {row inside the owner's stripe, byte offset of the destination row inside this
// GPU's lane arena} -- one reservation per wave and owner (ballot + popcount).  The order inside a list is arbitrary; what lands
// where is not.  Same lookup as the gather's (FindFeat: carried slot or node_map[id]).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bulk_bucket_kernel(GatherParams gp, const LanePtrs* __restrict__ lanes, BulkLists b, const char* arena_base)
{
    const LanePtrs& L = lanes[blockIdx.y];
    const LG_G int32_t* nc = LG_GPTR(const int32_t, L.node_counter);
    const int32_t hop_num = nc[INTRABATCH_CON * 3 - 1];
    int32_t n = nc[INTRABATCH_CON * 3 + hop_num];
    if (n > L.feature_rows) n = L.feature_rows;
    if (n > gp.max_rows) n = gp.max_rows;
    const LG_G int32_t* sampled_ids = LG_GPTR(const int32_t, L.sampled_ids);
    const LG_G int32_t* node_slot = (L.node_slot != nullptr && gp.node_map != nullptr) ? LG_GPTR(const int32_t, L.node_slot) : nullptr;
    const int32_t lane = threadIdx.x & 63;
    for (int32_t r0 = (blockIdx.x * 256 + (threadIdx.x & ~63)); r0 < n; r0 += gridDim.x * 256) {     // a wave takes 64 consecutive rows
        const int32_t r = r0 + lane;
        int32_t owner = -1, fidx = 0;
        if (r < n) {
            const int32_t id = sampled_ids[r];
            int32_t g = node_slot != nullptr ? node_slot[r] : LG_FS_UNKNOWN;
            if (g == LG_FS_UNKNOWN) g = (gp.node_map != nullptr && id >= 0) ? gp.node_map[id] : CACHEMISS_FLAG;
            if (g >= 0) {
                const int32_t didx = g / gp.node_capacity;
                fidx = g - didx * gp.node_capacity;
                const int64_t rank = (int64_t)fidx * gp.Kg + didx;
                const bool local_copy = gp.replica != nullptr && rank < gp.replica_rows;
                if (!local_copy && didx != gp.member) owner = didx;
            }
        }
        for (int32_t o = 0; o < b.Kg; o++) {
            const unsigned long long m = __ballot(owner == o);
            if (m == 0ull) continue;
            unsigned long long base = 0;
            if (lane == __ffsll((long long)m) - 1) base = atomicAdd(b.cnt + o, (unsigned long long)__popcll(m));
            base = __shfl(base, __ffsll((long long)m) - 1);
            if (owner == o) {
                const int64_t at = (int64_t)base + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
                if (at < b.cap) {
                    b.fidx[(int64_t)o * b.cap + at] = fidx;
                    b.dst[(int64_t)o * b.cap + at] = (const char*)(L.float_features + (int64_t)r * gp.D) - arena_base;
                }
            }
        }
    }
}

void launch_bulk_bucket(hipStream_t s, const GatherParams& g, const LanePtrs* d_lanes, int32_t n_lanes, const BulkLists& lists,
                        const char* arena_base)
{
    if (g.D <= 0 || g.max_rows <= 0 || g.node_map == nullptr || g.Kg <= 1) return;
    GatherParams gp = g;
    if (gp.node_capacity < 1) gp.node_capacity = 1;
    int32_t gx = (g.max_rows + 255) / 256;
    while (gx > 16 && (int64_t)gx * n_lanes > 16384) gx = (gx + 1) / 2;
    bulk_bucket_kernel<<<dim3(gx, n_lanes), 256, 0, s>>>(gp, d_lanes, lists, arena_base);
    hipCheckError();
}

// ------------------------------------------------------------------------------------------
// peer_gather = bulk, owner side: the rows a requester listed for THIS GPU's stripe, read from local HBM and written straight to
// their destination rows in the requester's lane arena -- whole rows, 16-byte chunks, consecutive lanes on consecutive chunks:
// over xGMI these are posted stores of contiguous 512-1024-byte runs instead of the requester's scattered load round trips.
// The lists (12 bytes per row) are read through the requester's peer mapping.  float32 stripes only: a bf16 cache is refused together
// with peer_gather = bulk where the transfer is set up (the arena's rows are float32; this copy does not widen).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bulk_push_kernel(const float* __restrict__ stripe, int32_t D, const int32_t* __restrict__ fidx,
                                                       const int64_t* __restrict__ dst, const unsigned long long* __restrict__ cnt,
                                                       int64_t cap, char* __restrict__ peer_arena)
{
    typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
    int64_t n = (int64_t)cnt[0];
    if (n > cap) n = cap;
    const int32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * 256) >> 6;
    const int32_t C = D / 4;
    for (int64_t i = wave; i < n; i += nwaves) {
        const LG_G float* src = LG_GPTR(const float, stripe) + (int64_t)fidx[i] * D;
        LG_G float* out = (LG_G float*)(peer_arena + dst[i]);
        for (int32_t c = lane; c < C; c += 64) ((LG_G v4u*)out)[c] = ((const LG_G v4u*)src)[c];
        for (int32_t k = C * 4 + lane; k < D; k += 64) out[k] = src[k];
    }
}

void launch_bulk_push(hipStream_t s, const float* stripe, int32_t D, const int32_t* fidx, const int64_t* dst,
                      const unsigned long long* cnt, int64_t cap, char* peer_arena)
{
    if (stripe == nullptr || D <= 0 || cap <= 0) return;
    bulk_push_kernel<<<2048, 256, 0, s>>>(stripe, D, fidx, dst, cnt, cap, peer_arena);
    hipCheckError();
}

// tiles of a lane are walked by gx workgroups: about LG_GATHER_TARGET_WG workgroups per launch, never more than tiles
static inline int32_t gather_grid_x(int32_t max_rows, int32_t rows_per_tile, int32_t n_lanes)
{
    const int32_t tiles = (max_rows + rows_per_tile - 1) / rows_per_tile;
    int32_t gx = (LG_GATHER_TARGET_WG + n_lanes - 1) / n_lanes;
    if (gx > tiles) gx = tiles;
    return gx < 1 ? 1 : gx;
}

// the instance of format F with the plan's tile size (walking ROWS = 16, 32, ... 256 over the sizes gather_info(F).tiles has); the
// LASTOP instance for the gather of a batch's last op.  Returns the launch's grid x (0: the format has no such tile size).
template <typename VecT, GatherFormat F, int ROWS = 16>
static int32_t launch_format(hipStream_t s, int32_t rows, const GatherParams& gk, int32_t grid_rows, const LanePtrs* d_lanes, int32_t n_lanes, bool copy_range)
{
    constexpr GatherFormatInfo fi = gather_info(F);
    if constexpr ((fi.tiles & ROWS) != 0) {
        if (rows == ROWS) {
            const dim3 grid(gather_grid_x(grid_rows, ROWS, n_lanes), n_lanes);
            if (gk.last_op) gather_kernel<VecT, ROWS, fi.unroll, fi.tail, true><<<grid, LG_GATHER_THREADS, 0, s>>>(gk, d_lanes, copy_range);
            else gather_kernel<VecT, ROWS, fi.unroll, fi.tail, false><<<grid, LG_GATHER_THREADS, 0, s>>>(gk, d_lanes, copy_range);
            return (int32_t)grid.x;
        }
    }
    if constexpr (ROWS < 256) return launch_format<VecT, F, ROWS * 2>(s, rows, gk, grid_rows, d_lanes, n_lanes, copy_range);
    return 0;
}

// the plan of a gather launch over n_lanes lanes; grid_rows: what sizes the launch, the rows a lane typically has (GatherParams.grid_rows)
static GatherPlan plan_of_launch(const GatherParams& gk, int32_t n_lanes, int32_t& grid_rows)
{
    grid_rows = gk.grid_rows > 0 && gk.grid_rows < gk.max_rows ? gk.grid_rows : gk.max_rows;
    return gather_plan(gk.dtype, gk.out_dtype, gk.D, gk.pitch, grid_rows, n_lanes, tuning().gather_rows_per_wg);
}

// gk: what the kernel gets (max_rows = the clamp).  Returns the plan it launched and sets grid_x to the launch's grid x (0: nothing to
// launch).
static GatherPlan launch_gather_impl(hipStream_t s, GatherParams gk, const LanePtrs* d_lanes, int32_t n_lanes, bool copy_range, int32_t* grid_x = nullptr)
{
    if (grid_x != nullptr) *grid_x = 0;
    if (gk.D <= 0 || gk.max_rows <= 0) return {GatherPlan::OK, GatherFormat::F32, 0};      // :256 float_feature_len > 0
    if (gk.node_capacity < 1) gk.node_capacity = 1;
    int32_t grid_rows, gx = 0;
    const GatherPlan p = plan_of_launch(gk, n_lanes, grid_rows);
    if (p.error == GatherPlan::BAD_DTYPE) printf("gather: unknown feature dtype %d or output dtype %d\n", gk.dtype, gk.out_dtype);
    if (p.error == GatherPlan::BAD_PITCH) printf("gather: bf16 rows need a pitch that is a multiple of 8 and at least D (pitch %d, D %d)\n", gk.pitch, gk.D);
    if (p.error != GatherPlan::OK) exit(EXIT_FAILURE);
    typedef GatherFormat GF;
    switch (p.format) {     // the row type of each format
        case GF::F32:       gx = launch_format<f32x4, GF::F32>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
        case GF::F32Tail:   gx = launch_format<f32x4, GF::F32Tail>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
        case GF::F32Scalar: gx = launch_format<float, GF::F32Scalar>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
        case GF::Bf16x8:    gx = launch_format<Bf16x8, GF::Bf16x8>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
        case GF::Bf16Copy:  gx = launch_format<Bf16Copy, GF::Bf16Copy>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
        case GF::F32Narrow: gx = launch_format<F32Narrow, GF::F32Narrow>(s, p.rows, gk, grid_rows, d_lanes, n_lanes, copy_range); break;
    }
    hipCheckError();
    if (grid_x != nullptr) *grid_x = gx;
    return p;
}

void launch_gather(hipStream_t s, const GatherParams& g, const LanePtrs* d_lanes, int32_t n_lanes)
{
    launch_gather_impl(s, g, d_lanes, n_lanes, true);
}

// stand-alone form (tests, probes): explicit arrays; a one-lane descriptor is staged on the stream.  node_slot: the lane's carried
// slots or null; g.last_op picks the instance; plan_out: null, or host {format, rows per tile, grid x} of the launch made ({-1, 0, 0}
// where there was nothing to launch).  Returns 0, or -1 with nothing enqueued for a dtype or pitch the plan refuses.
int32_t launch_gather_explicit(hipStream_t s, const GatherParams& g, const int32_t* sampled_ids, const int32_t* node_slot,
                               int32_t* cache_index_out, const int32_t* range, void* dst, int32_t dst_rows, int32_t* plan_out)
{
    int32_t grid_rows, gx = 0;
    if (plan_of_launch(g, 1, grid_rows).error != GatherPlan::OK) return -1;
    static thread_local LanePtrs* d_lane = nullptr;
    if (d_lane == nullptr) HIP_CALL(hipMalloc(&d_lane, sizeof(LanePtrs)));
    LanePtrs h;
    memset(&h, 0, sizeof(h));
    h.sampled_ids = const_cast<int32_t*>(sampled_ids);
    h.node_slot = const_cast<int32_t*>(node_slot);
    h.cache_search_buffer = cache_index_out;
    h.node_counter = const_cast<int32_t*>(range);
    h.float_features = static_cast<float*>(dst);
    h.feature_rows = dst_rows;
    GatherParams ge = g;
    ge.hop = -1;
    ge.first_hop = -1;
    HIP_CALL(hipMemcpyAsync(d_lane, &h, sizeof(h), hipMemcpyHostToDevice, s));   // pageable source: staged before return
    const GatherPlan p = launch_gather_impl(s, ge, d_lane, 1, false, &gx);
    if (plan_out != nullptr) {
        plan_out[0] = gx > 0 ? (int32_t)p.format : -1;
        plan_out[1] = gx > 0 ? p.rows : 0;
        plan_out[2] = gx;
    }
    return 0;
}

}  // namespace lg
