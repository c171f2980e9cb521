// kernels_reverse.hip -- the reverse CSR for gfx950 (CDNA4, wave64): the transpose of the full CSR, built once on the device
// (legion_graph_build_reverse; DGL's dgl.reverse, and through it g.out_edges, g.out_degrees and g.successors).  The rule is the
// contract in include/legion_hip.h; the classes, the passes and the refusals are reverse_rule.h's.
// The layout: 256 lanes per workgroup, a grid of at most 2 048 workgroups that strides over tiles (the walks' cap, walk_step.h), every
// edge offset 64 bits wide, no workgroup waits for another and every loop carries its bound.
//   * count     tiles of 1 024 consecutive entries e, four per lane, 256 apart (in_edges' tile): a live col[e] adds 1 to
//               rindptr[col[e]], a no-return 64-bit atomic on the output itself, zeroed on the stream first;
//   * scan      the counts in place, the total E' to rindptr[N]: launch_scan_int64 alone up to 2^20 vertices, else the same three
//               kernels at two levels -- the sums per 256 counts, those scanned by launch_scan_int64, the apply;
//   * scatter   the same tiles; row(e) is an upper-bound search over the graph's own indptr, the tile's range of it staged in LDS as
//               row_slots.h stages a list's offsets (upper_counts is its), so a hub row is spread over lanes like any other entries;
//               each live entry takes pos = cursor[col[e]]++ by a returning atomic and writes reid[pos] = e, rcol[pos] = row(e).  The
//               cursors are an N-sized copy of rindptr; there is no E-sized temporary;
//   * sort      every reverse row by reid, rcol its payload, which makes the result a function of the graph whatever order the atomics
//               arrived in.  A wave takes 64 consecutive rows: those of 2 .. 64 entries it sorts in registers one after the other (a
//               bitonic network over the lanes), those of up to LG_REVERSE_TILE it appends to a list and the longer ones, with their
//               place and length, to another.  A workgroup per listed row sorts it in LDS.  A long row is sorted in runs of
//               LG_REVERSE_TILE the same way, then merged in passes between its segment of the output and a scratch as long as the
//               long rows together; a merge is cut by merge path into pieces of LG_REVERSE_CHUNK outputs, a workgroup each, so a hub
//               is every workgroup's job, and the passes are counted so that the last lands in the output.  The lists are read back
//               once (the call synchronises); the pieces of every pass are planned on the host.
// Integer atomics on hot keys were unmeasured on this chip when this was written (the guides at hand measure float atomics only), so
// nothing here was chosen on a predicted rate; tools/reverse_rate.py measured them: on RMAT graphs the count's
// no-return adds run at 8.5 G a second and the scatter's returning adds at 7.0 G, and the two passes are three quarters of a build.
// Bound: count and scatter by their atomics, not by the col reads; the sorts by LDS; no MFMA.
#include <algorithm>
#include <cstring>
#include <vector>

#include "legion_core.h"
#include "reverse_rule.h"
#include "row_slots.h"
#include "tile_scan.h"
#include "walk_step.h"

namespace lg {

static_assert(LG_ROW_THREADS == 256 && LG_SCAN_THREADS == 256, "one workgroup shape for every kernel below");
static_assert(LG_REVERSE_WAVE == 64, "a wave sorts a row of its class with one entry per lane");
static_assert((LG_REVERSE_TILE & (LG_REVERSE_TILE - 1)) == 0 && LG_REVERSE_TILE >= 2 * LG_ROW_THREADS, "the LDS sort is bitonic over a power of two");
static_assert(LG_REVERSE_TILE * 12 <= 64 * 1024 && LG_REVERSE_CHUNK * 12 <= 64 * 1024, "the static LDS of one workgroup");

// the scan's kernels (kernels_in_edges.hip)
__global__ void scan_sum_kernel(const int64_t* values, int32_t n, int32_t n_sums, int64_t* sums);
__global__ void scan_apply_kernel(int64_t* values, int32_t n, int32_t n_sums, const int64_t* sums);

#define LG_REVERSE_NO_KEY 0x7FFFFFFFFFFFFFFFll                // above every edge id

// ------------------------------------------------------------------------------------------
// count
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LG_ROW_THREADS) void reverse_count_kernel(const int32_t* col, int64_t num_edges, int32_t node_num,
                                                                        unsigned long long* counts)
{
    const int64_t n_tiles = (num_edges + LG_ROW_TILE - 1) / LG_ROW_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int32_t u[LG_ROW_ILP];
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) {
            const int64_t e = tile * LG_ROW_TILE + threadIdx.x + (int64_t)j * LG_ROW_THREADS;
            u[j] = e < num_edges ? col[e] : -1;
        }
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++)
            if ((uint32_t)u[j] < (uint32_t)node_num) atomicAdd(counts + u[j], 1ull);      // (the value is not used: no return)
    }
}

// ------------------------------------------------------------------------------------------
// scatter
// ------------------------------------------------------------------------------------------
// row(e) of the tile's entries: the v with indptr[v] <= e < indptr[v + 1], -1 where there is none (an indptr that does not start at 0 or
// end at num_edges).  The first and the last row the tile touches come from two searches over indptr in global memory; that range is
// staged in s_off if it has at most LG_ROW_STAGE entries, else each entry searches it in global memory.  Whatever indptr holds,
// nothing is read outside indptr[0 .. node_num].  One barrier inside; the caller puts another before the next tile stages
__device__ __forceinline__ void reverse_tile_rows(const int64_t* indptr, int32_t node_num, int64_t num_edges, int64_t tile, int64_t* s_off,
                                                  int64_t (&e)[LG_ROW_ILP], bool (&live)[LG_ROW_ILP], int32_t (&row)[LG_ROW_ILP])
{
    const int32_t n1 = node_num + 1;
    const int64_t e0 = tile * LG_ROW_TILE;
    const int64_t ends[2] = {e0, min(e0 + LG_ROW_TILE - 1, num_edges - 1)};
    const bool both[2] = {true, true};
    int32_t ub[2];
    upper_counts<2>(indptr, n1, ends, both, ub);
    const int32_t a = max(ub[0] - 1, 0), b = min(ub[1], node_num);
    const int32_t cnt = max(b - a + 1, 0);                            // indptr[a .. b]: inside indptr[0 .. node_num]
    const bool staged = cnt <= LG_ROW_STAGE;
    if (staged)
        for (int32_t k = threadIdx.x; k < cnt; k += LG_ROW_THREADS) s_off[k] = indptr[a + k];
    __syncthreads();
#pragma unroll
    for (int32_t j = 0; j < LG_ROW_ILP; j++) {
        e[j] = e0 + threadIdx.x + (int64_t)j * LG_ROW_THREADS;
        live[j] = e[j] < num_edges;
    }
    int32_t c[LG_ROW_ILP];
    if (staged) upper_counts<LG_ROW_ILP>(s_off, cnt, e, live, c);
    else upper_counts<LG_ROW_ILP>(indptr + a, cnt, e, live, c);
#pragma unroll
    for (int32_t j = 0; j < LG_ROW_ILP; j++) {
        row[j] = c[j] > 0 ? a + c[j] - 1 : -1;                        // (c == 0: before the range, no row)
        if (row[j] >= node_num) row[j] = -1;                          // past indptr[node_num]: no row
    }
}

__global__ __launch_bounds__(LG_ROW_THREADS, 8) void reverse_scatter_kernel(const int64_t* indptr, const int32_t* col, int32_t node_num,
                                                                             int64_t num_edges, unsigned long long* cursor,
                                                                             int64_t live_edges, int64_t* reid, int32_t* rcol)
{
    __shared__ int64_t s_off[LG_ROW_STAGE];
    const int64_t n_tiles = (num_edges + LG_ROW_TILE - 1) / LG_ROW_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t e[LG_ROW_ILP];
        bool live[LG_ROW_ILP];
        int32_t row[LG_ROW_ILP], u[LG_ROW_ILP];
        reverse_tile_rows(indptr, node_num, num_edges, tile, s_off, e, live, row);
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) u[j] = live[j] ? col[e[j]] : -1;
#pragma unroll
        for (int32_t j = 0; j < LG_ROW_ILP; j++) {
            if ((uint32_t)u[j] < (uint32_t)node_num) {
                const int64_t pos = (int64_t)atomicAdd(cursor + u[j], 1ull);
                if (pos >= 0 && pos < live_edges) {                   // (always, while col is what the count read)
                    reid[pos] = e[j];
                    rcol[pos] = row[j];
                }
            }
        }
        __syncthreads();                                              // the next tile stages over s_off
    }
}

// ------------------------------------------------------------------------------------------
// sort: the wave class, and the lists of the other two
// ------------------------------------------------------------------------------------------
struct ReverseKey {
    int64_t eid;
    int32_t v;
};

// one compare-exchange with the lane `stride` away: this lane keeps the smaller edge id iff keep_min (edge ids of a row are distinct)
__device__ __forceinline__ void reverse_exchange(ReverseKey& k, int32_t stride, bool keep_min)
{
    const int64_t oe = __shfl_xor(k.eid, stride, 64);
    const int32_t ov = __shfl_xor(k.v, stride, 64);
    if ((oe < k.eid) == keep_min) {
        k.eid = oe;
        k.v = ov;
    }
}

// the wave's 64 keys sorted ascending across the lanes: 21 exchanges
__device__ __forceinline__ void reverse_wave_sort(ReverseKey& k, int32_t lane)
{
#pragma unroll
    for (int32_t size = 2; size <= 64; size <<= 1) {
        const bool up = (lane & size) == 0;                           // (size 64: every lane, the final direction)
#pragma unroll
        for (int32_t stride = size >> 1; stride > 0; stride >>= 1) reverse_exchange(k, stride, ((lane & stride) == 0) == up);
    }
}

// the lists a build reads back: counters, then the long rows
struct ReverseLists {
    unsigned long long* counters;   // [0] rows of the Tile class, [1] long rows, [2] the long rows' entries together
    int32_t* tile_rows;             // the Tile class: int32[tile_cap]
    int64_t* long_rows;             // the Long class: {start, length} int64[2 * long_cap]
    int64_t tile_cap, long_cap;     // reverse_tile_rows_cap(E'), reverse_long_rows_cap(E')
};

__global__ __launch_bounds__(LG_ROW_THREADS) void reverse_sort_wave_kernel(const int64_t* rindptr, int32_t node_num, int64_t* reid,
                                                                            int32_t* rcol, ReverseLists lists)
{
    const int32_t lane = threadIdx.x & 63;
    const int64_t n_groups = ((int64_t)node_num + 63) / 64;           // a wave per 64 consecutive rows
    const int64_t waves = (int64_t)gridDim.x * (LG_ROW_THREADS / 64);
    for (int64_t g = (int64_t)blockIdx.x * (LG_ROW_THREADS / 64) + (threadIdx.x >> 6); g < n_groups; g += waves) {
        const int64_t r = g * 64 + lane;
        int64_t start = 0, len = 0;
        if (r < node_num) {
            start = rindptr[r];
            len = rindptr[r + 1] - start;
        }
        const ReverseClass cls = reverse_class(len);
        if (cls == ReverseClass::Tile) {
            const int64_t k = (int64_t)atomicAdd(lists.counters + 0, 1ull);
            if (k < lists.tile_cap) lists.tile_rows[k] = (int32_t)r;                      // (always: the rows of the class are disjoint)
        } else if (cls == ReverseClass::Long) {
            const int64_t k = (int64_t)atomicAdd(lists.counters + 1, 1ull);
            atomicAdd(lists.counters + 2, (unsigned long long)len);
            if (k < lists.long_cap) {
                lists.long_rows[2 * k] = start;
                lists.long_rows[2 * k + 1] = len;
            }
        }
        uint64_t todo = __ballot(cls == ReverseClass::Wave);
        while (todo != 0) {                                           // at most 64 trips: each clears a bit
            const int32_t src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int64_t s = __shfl(start, src, 64);
            const int32_t l = (int32_t)__shfl(len, src, 64);          // 2 .. 64
            ReverseKey k{LG_REVERSE_NO_KEY, -1};
            if (lane < l) {
                k.eid = reid[s + lane];
                k.v = rcol[s + lane];
            }
            reverse_wave_sort(k, lane);
            if (lane < l) {
                reid[s + lane] = k.eid;
                rcol[s + lane] = k.v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// sort: a row, or a run of a long row, in LDS
// ------------------------------------------------------------------------------------------
// ONE workgroup: the len <= LG_REVERSE_TILE entries at src_* sorted by edge id to dst_* (which may be src_*): a bitonic network over
// the next power of two, the tail filled with LG_REVERSE_NO_KEY.  Both barriers inside: every lane of the workgroup calls it
__device__ __forceinline__ void reverse_sort_lds(const int64_t* src_eid, const int32_t* src_v, int64_t* dst_eid, int32_t* dst_v, int32_t len,
                                                 int64_t* s_eid, int32_t* s_v)
{
    int32_t n2 = 2 * LG_ROW_THREADS;                                  // every lane has a pair in every stage
    while (n2 < len) n2 <<= 1;                                        // len <= LG_REVERSE_TILE: at most 3 trips
    for (int32_t k = threadIdx.x; k < n2; k += LG_ROW_THREADS) {
        s_eid[k] = k < len ? src_eid[k] : LG_REVERSE_NO_KEY;
        s_v[k] = k < len ? src_v[k] : -1;
    }
    __syncthreads();
    for (int32_t size = 2; size <= n2; size <<= 1) {
        for (int32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (int32_t t = threadIdx.x; t < (n2 >> 1); t += LG_ROW_THREADS) {
                const int32_t i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;      // i < j < n2
                const bool up = (i & size) == 0;
                const int64_t a = s_eid[i], b = s_eid[j];
                if ((b < a) == up) {
                    s_eid[i] = b;
                    s_eid[j] = a;
                    const int32_t va = s_v[i];
                    s_v[i] = s_v[j];
                    s_v[j] = va;
                }
            }
            __syncthreads();
        }
    }
    for (int32_t k = threadIdx.x; k < len; k += LG_ROW_THREADS) {
        dst_eid[k] = s_eid[k];
        dst_v[k] = s_v[k];
    }
    __syncthreads();                                                  // the next call stages over s_eid and s_v
}

__global__ __launch_bounds__(LG_ROW_THREADS) void reverse_sort_tile_kernel(const int64_t* rindptr, int32_t node_num, const int32_t* rows,
                                                                            int64_t n_rows, int64_t* reid, int32_t* rcol)
{
    __shared__ int64_t s_eid[LG_REVERSE_TILE];
    __shared__ int32_t s_v[LG_REVERSE_TILE];
    for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
        const int32_t r = rows[i];
        int64_t start = 0, len = 0;
        if ((uint32_t)r < (uint32_t)node_num) {
            start = rindptr[r];
            len = rindptr[r + 1] - start;
        }
        if (len < 0 || len > LG_REVERSE_TILE) len = 0;                // (never: the list holds rows of the class)
        reverse_sort_lds(reid + start, rcol + start, reid + start, rcol + start, (int32_t)len, s_eid, s_v);
    }
}

// a run of a long row: read from the output at src, written to the output or (to_scratch) the scratch at dst
struct ReverseRun {
    int64_t src, dst;
    int32_t len;                    // 1 .. LG_REVERSE_TILE
    int32_t to_scratch;
};

__global__ __launch_bounds__(LG_ROW_THREADS) void reverse_sort_runs_kernel(const ReverseRun* runs, int64_t n_runs, int64_t* reid, int32_t* rcol,
                                                                            int64_t* scratch_eid, int32_t* scratch_v)
{
    __shared__ int64_t s_eid[LG_REVERSE_TILE];
    __shared__ int32_t s_v[LG_REVERSE_TILE];
    for (int64_t i = blockIdx.x; i < n_runs; i += gridDim.x) {
        const ReverseRun run = runs[i];
        reverse_sort_lds(reid + run.src, rcol + run.src, (run.to_scratch ? scratch_eid : reid) + run.dst,
                         (run.to_scratch ? scratch_v : rcol) + run.dst, run.len, s_eid, s_v);
    }
}

// ------------------------------------------------------------------------------------------
// sort: the merge passes of the long rows
// ------------------------------------------------------------------------------------------
// A piece of one merge: the sorted runs A = src[a .. a + la) and B = src[a + la .. a + la + lb) become dst[d .. d + la + lb); this piece
// writes the outputs d0 .. min(d0 + LG_REVERSE_CHUNK, la + lb) - 1 of them.  lb == 0: a run without a partner is copied.  from_scratch:
// src is the scratch and dst the output, else the other way round
struct ReversePiece {
    int64_t a, d, la, lb, d0;
    int32_t from_scratch;
    int32_t pad;
};

// merge path: how many of the first diag outputs of the merge of A[0 .. la) and B[0 .. lb) come from A (the keys are distinct).
// Reads A and B inside their lengths only; at most 63 trips
__device__ __forceinline__ int64_t reverse_merge_split(const int64_t* A, int64_t la, const int64_t* B, int64_t lb, int64_t diag)
{
    int64_t lo = max(diag - lb, (int64_t)0), hi = min(diag, la);
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);                    // lo <= mid < hi <= la; 0 <= diag - 1 - mid < lb
        if (A[mid] < B[diag - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// #{ k in [0, n) : a[k] < key } for an ascending a (in LDS): at most 12 trips
__device__ __forceinline__ int32_t reverse_lower_count(const int64_t* a, int32_t n, int64_t key)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LG_ROW_THREADS) void reverse_merge_kernel(const ReversePiece* pieces, int64_t n_pieces, int64_t* reid, int32_t* rcol,
                                                                        int64_t* scratch_eid, int32_t* scratch_v)
{
    __shared__ int64_t s_eid[LG_REVERSE_CHUNK];
    __shared__ int32_t s_v[LG_REVERSE_CHUNK];
    __shared__ int64_t s_split[2];
    for (int64_t i = blockIdx.x; i < n_pieces; i += gridDim.x) {
        const ReversePiece p = pieces[i];
        const int64_t* src_eid = (p.from_scratch ? scratch_eid : reid) + p.a;
        const int32_t* src_v = (p.from_scratch ? scratch_v : rcol) + p.a;
        int64_t* dst_eid = (p.from_scratch ? reid : scratch_eid) + p.d;
        int32_t* dst_v = (p.from_scratch ? rcol : scratch_v) + p.d;
        const int64_t d1 = min(p.d0 + LG_REVERSE_CHUNK, p.la + p.lb);
        if (threadIdx.x < 2) s_split[threadIdx.x] = reverse_merge_split(src_eid, p.la, src_eid + p.la, p.lb, threadIdx.x == 0 ? p.d0 : d1);
        __syncthreads();
        const int64_t i0 = s_split[0], i1 = s_split[1], j0 = p.d0 - i0;
        const int32_t na = (int32_t)(i1 - i0), n = (int32_t)(d1 - p.d0), nb = n - na;      // na + nb = n <= LG_REVERSE_CHUNK
        for (int32_t k = threadIdx.x; k < n; k += LG_ROW_THREADS) {
            const int64_t at = k < na ? i0 + k : p.la + j0 + (k - na);                    // inside A, or inside B behind it
            s_eid[k] = src_eid[at];
            s_v[k] = src_v[at];
        }
        __syncthreads();
        // an entry's place among the piece's outputs: its place in its own part plus the entries of the other part below it
        for (int32_t k = threadIdx.x; k < n; k += LG_ROW_THREADS) {
            const int64_t key = s_eid[k];
            const int32_t rank = k < na ? k + reverse_lower_count(s_eid + na, nb, key) : (k - na) + reverse_lower_count(s_eid, na, key);
            dst_eid[p.d0 + rank] = key;
            dst_v[p.d0 + rank] = s_v[k];
        }
        __syncthreads();                                              // the next piece stages over s_eid, s_v and s_split
    }
}

// ------------------------------------------------------------------------------------------
// the build
// ------------------------------------------------------------------------------------------
// a grid of one workgroup per item, at most the walks' cap
static inline dim3 reverse_item_grid(int64_t items) { return dim3((uint32_t)(items < LG_WALK_MAX_WG ? items : LG_WALK_MAX_WG)); }

// rindptr[0 .. node_num) holds the counts: they become their exclusive prefix sums and rindptr[node_num] their total (reverse_rule.h:
// the levels and the scratch, reverse_scan_scratch(node_num) int64)
static void reverse_scan(hipStream_t s, int64_t* rindptr, int32_t node_num, int64_t* sums)
{
    const int32_t n_sums = (int32_t)reverse_scan_sums(node_num);
    if (reverse_scan_levels(node_num) < 2) {
        launch_scan_int64(s, rindptr, node_num, sums, n_sums, false, rindptr + node_num, nullptr);
        return;
    }
    int64_t* sums2 = sums + n_sums;
    scan_sum_kernel<<<walk_grid(node_num), LG_SCAN_THREADS, 0, s>>>(rindptr, node_num, n_sums, sums);
    launch_scan_int64(s, sums, n_sums, sums2, (n_sums + 255) / 256, false, rindptr + node_num, nullptr);
    scan_apply_kernel<<<walk_grid(node_num), LG_SCAN_THREADS, 0, s>>>(rindptr, node_num, n_sums, sums);
    hipCheckError();
}

// the long rows ({start, length} pairs) as runs and as the pieces of every merge pass; returns the scratch's entries
static int64_t reverse_plan_long(const std::vector<int64_t>& rows, std::vector<ReverseRun>& runs, std::vector<std::vector<ReversePiece>>& passes)
{
    int64_t scratch = 0;
    for (size_t r = 0; r + 1 < rows.size(); r += 2) {
        const int64_t start = rows[r], len = rows[r + 1], at[2] = {start, scratch};      // the row in the output, and in the scratch
        const int32_t P = reverse_passes(len);
        const int32_t first = reverse_buffer_after(P, 0);
        for (int64_t k = 0; k < reverse_runs(len); k++) {
            const int64_t off = k * LG_REVERSE_TILE;
            runs.push_back(ReverseRun{start + off, at[first] + off, (int32_t)std::min<int64_t>(LG_REVERSE_TILE, len - off), first});
        }
        if ((int32_t)passes.size() < P) passes.resize(P);
        for (int32_t p = 1; p <= P; p++) {
            const int64_t W = reverse_run_width(p);
            const int32_t from = reverse_buffer_after(P, p - 1), to = reverse_buffer_after(P, p);
            for (int64_t off = 0; off < len; off += 2 * W) {
                const int64_t la = std::min(W, len - off), lb = std::min(W, len - off - la);
                for (int64_t c = 0; c < reverse_merge_chunks(la, lb); c++)
                    passes[p - 1].push_back(ReversePiece{at[from] + off, at[to] + off, la, lb, c * LG_REVERSE_CHUNK, from, 0});
            }
        }
        scratch += len;
    }
    return scratch;
}

// the arguments are the caller's to check (reverse_refusal); the three arrays are the caller's to free with d_free_space
int64_t build_reverse_csr(hipStream_t s, const int64_t* indptr, const int32_t* col, int32_t node_num, int64_t num_edges, int64_t** rindptr_out,
                          int32_t** rcol_out, int64_t** reid_out)
{
    const int32_t N = node_num > 0 ? node_num : 0;
    const int64_t E = N > 0 && num_edges > 0 ? num_edges : 0;
    int64_t* rindptr = (int64_t*)d_alloc_space(((int64_t)N + 1) * sizeof(int64_t));
    HIP_CALL(hipMemsetAsync(rindptr, 0, ((size_t)N + 1) * sizeof(int64_t), s));
    int64_t live = 0;
    if (E > 0) {
        int64_t* sums = (int64_t*)d_alloc_space(reverse_scan_scratch(N) * sizeof(int64_t));
        reverse_count_kernel<<<walk_grid((E + LG_ROW_ILP - 1) / LG_ROW_ILP), LG_ROW_THREADS, 0, s>>>(col, E, N, (unsigned long long*)rindptr);
        hipCheckError();
        reverse_scan(s, rindptr, N, sums);
        HIP_CALL(hipMemcpyAsync(&live, rindptr + N, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_CALL(hipStreamSynchronize(s));
        d_free_space(sums);
    }
    int64_t* reid = (int64_t*)d_alloc_space(live * sizeof(int64_t));
    int32_t* rcol = (int32_t*)d_alloc_space(live * sizeof(int32_t));
    *rindptr_out = rindptr;
    *rcol_out = rcol;
    *reid_out = reid;
    if (live <= 0) return 0;

    unsigned long long* cursor = (unsigned long long*)d_alloc_space((int64_t)N * sizeof(int64_t));
    HIP_CALL(hipMemcpyAsync(cursor, rindptr, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    reverse_scatter_kernel<<<walk_grid((E + LG_ROW_ILP - 1) / LG_ROW_ILP), LG_ROW_THREADS, 0, s>>>(indptr, col, N, E, cursor, live, reid, rcol);
    hipCheckError();

    // the wave class, and the lists of the other two: read back once
    ReverseLists lists;
    lists.tile_cap = reverse_tile_rows_cap(live);
    lists.long_cap = reverse_long_rows_cap(live);
    const int64_t back_words = 4 + 2 * lists.long_cap;                // counters (one word spare), then the long rows
    unsigned long long* back = (unsigned long long*)d_alloc_space(back_words * sizeof(int64_t));
    lists.counters = back;
    lists.long_rows = (int64_t*)(back + 4);
    lists.tile_rows = (int32_t*)d_alloc_space(lists.tile_cap * sizeof(int32_t));
    HIP_CALL(hipMemsetAsync(back, 0, 4 * sizeof(int64_t), s));
    reverse_sort_wave_kernel<<<walk_grid(((int64_t)N + 63) / 64 * 64), LG_ROW_THREADS, 0, s>>>(rindptr, N, reid, rcol, lists);      // a lane per row
    hipCheckError();
    std::vector<int64_t> host(back_words);
    HIP_CALL(hipMemcpyAsync(host.data(), back, back_words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CALL(hipStreamSynchronize(s));
    const int64_t n_tile = std::min<int64_t>(host[0], lists.tile_cap), n_long = std::min<int64_t>(host[1], lists.long_cap);
    if (n_tile > 0) {
        reverse_sort_tile_kernel<<<reverse_item_grid(n_tile), LG_ROW_THREADS, 0, s>>>(rindptr, N, lists.tile_rows, n_tile, reid, rcol);
        hipCheckError();
    }
    void* plan_dev = nullptr;
    int64_t* scratch_eid = nullptr;
    int32_t* scratch_v = nullptr;
    if (n_long > 0) {
        std::vector<ReverseRun> runs;
        std::vector<std::vector<ReversePiece>> passes;
        const std::vector<int64_t> rows(host.begin() + 4, host.begin() + 4 + 2 * n_long);
        const int64_t scratch = reverse_plan_long(rows, runs, passes);      // == host[2], the sum the device counted
        scratch_eid = (int64_t*)d_alloc_space(scratch * sizeof(int64_t));
        scratch_v = (int32_t*)d_alloc_space(scratch * sizeof(int32_t));
        static_assert(sizeof(ReverseRun) % 8 == 0 && sizeof(ReversePiece) % 8 == 0, "the plan's parts lie 8-byte aligned behind each other");
        size_t bytes = runs.size() * sizeof(ReverseRun);
        for (const auto& p : passes) bytes += p.size() * sizeof(ReversePiece);
        std::vector<char> plan(bytes);
        size_t at = runs.size() * sizeof(ReverseRun);
        memcpy(plan.data(), runs.data(), at);
        for (const auto& p : passes) {
            memcpy(plan.data() + at, p.data(), p.size() * sizeof(ReversePiece));
            at += p.size() * sizeof(ReversePiece);
        }
        plan_dev = d_alloc_space((int64_t)bytes);
        HIP_CALL(hipMemcpyAsync(plan_dev, plan.data(), bytes, hipMemcpyHostToDevice, s));
        HIP_CALL(hipStreamSynchronize(s));                            // (the plan's host copy goes with this block)
        reverse_sort_runs_kernel<<<reverse_item_grid((int64_t)runs.size()), LG_ROW_THREADS, 0, s>>>((const ReverseRun*)plan_dev, (int64_t)runs.size(), reid, rcol,
                                                                                                     scratch_eid, scratch_v);
        at = runs.size() * sizeof(ReverseRun);
        for (const auto& p : passes) {
            reverse_merge_kernel<<<reverse_item_grid((int64_t)p.size()), LG_ROW_THREADS, 0, s>>>((const ReversePiece*)((const char*)plan_dev + at), (int64_t)p.size(),
                                                                                                  reid, rcol, scratch_eid, scratch_v);
            at += p.size() * sizeof(ReversePiece);
        }
        hipCheckError();
    }
    HIP_CALL(hipStreamSynchronize(s));                                // the temporaries go before the call returns
    d_free_space(plan_dev);
    d_free_space(scratch_eid);
    d_free_space(scratch_v);
    d_free_space(lists.tile_rows);
    d_free_space(back);
    d_free_space(cursor);
    return live;
}

}  // namespace lg
