// kmc_sketch_query.hip — a set of query sketches against a set of reference
// sketches: the whole rectangle of Mash distances (kmc_sketch_distances_rect) and
// the `top` nearest references of every query without that rectangle
// (kmc_sketch_nearest).  A pair's shared, denom and float are those of
// kmc_sketch_distances: both calls run the tile loop, pair_counts and mash_distance
// of kmc_sketch_pair.h.
//
// kmc_sketch_distances_rect: the m x n rectangle is cut into tiles of Tq query rows
// by Tr reference rows; a workgroup stages the Tq + Tr rows of a tile in LDS and its
// 16 wavefronts take the tile's pairs, one wavefront per pair: sketch_tile_kernel of
// kmc_sketch_pair.h, the triangle's kernel and consumer, with the shape Rectangle of
// kmc_sketch_rectangle.h (shared with the pair list, kmc_sketch_links.hip).  T is the
// triangle's edge (tile_edge over kDistElems), Tq = min(T, m), Tr = min(kTileMax,
// kDistElems / s - Tq, n) (tile_shape): a short query set leaves its room to the
// references.  Below kStageMinTile (s > 2048 shipped) the rows stay in global memory.
//
// kmc_sketch_nearest: reference r takes part for query q iff denom > 0 and shared >=
// min_shared; the references that do are ordered by J = shared / denom, descending,
// then by r.  shared <= denom <= 16384, so two distinct fractions differ by at least
// 2^-28 and code = floor(shared * 2^30 / denom) orders them exactly; the 64-bit key
//     ((2^30 - code) << 32) | r
// ascends in the required order and is never UINT64_MAX, the fill.  The search is
// "the `top` smallest keys of every query":
//   slab    grid (query tiles) x (reference slabs).  A workgroup stages its Tq query
//           rows once, then streams its slab in chunks of Tr reference rows (staged
//           beside them); a wavefront takes a pair, forms the key and appends it to
//           the query's candidate buffer in LDS (C keys, C the power of two >= top +
//           kTileMax) unless the key is above the query's threshold.  Before a chunk
//           that could overflow a buffer (count + Tr > C) every buffer is sorted
//           (bitonic_sort of kmc_sketch_pair.h, a segment each), cut to its `top` smallest,
//           and a buffer that holds `top` keys sets the threshold to its largest.
//           After the slab the survivors go to the workspace: keys[q][slab][top]
//           and count[q][slab].
//   merge   one workgroup per query keeps the P = pow2(top) smallest keys so far in
//           the front of an LDS buffer of M keys, fills the rest with the next M - P
//           slab survivors and sorts, until all S * top slots are seen.  The first
//           `top` keys are the hits; shared, denom and the float of each are
//           computed again from the two rows (top pairs per query, not n).
// tile_shape over kQueryElems with the query rows also capped by the candidate buffers:
// Tq = min(tile edge, kCandElems / C, m); Tr = min(kTileMax, kQueryElems / s - Tq, n),
// or the global tile edge when the rows are not staged.
// Slabs: S = ceil(n / per), per a multiple of Tr with (query tiles) * S <= 2 CUs
// (one slab when there are more query tiles than that), so the workspace is
//     num_queries * S * (8 top + 4) bytes, S <= max(1, 2 CUs / query tiles).
//
// Constants, shipped / under -DKMC_DIAG_HOOKS (a few dozen references then cross
// many chunks, compactions, slabs and merge passes; no new symbol):
//   kQueryElems  LDS capacity of the staged rows, values     14336 / 512
//   kCandElems   LDS capacity of the candidate buffers, keys 4096 / 4096
//   kMergeElems  LDS buffer of the merge at most, keys       4096 / 2 (M = 2 P)
//   kSlabMinRefs references per slab at least                1 / 8
//   slabs at most                                            2 CUs / query tiles / 32768
//   kDistElems, kTileMax (kmc_sketch_pair.h)                 16384, 32 / 512, 4
// LDS, shipped: rectangle tile 128 KB; slab 112 KB of rows + 32 KB of candidates;
// merge 32 KB.  One workgroup of 1024 threads per CU for the first two.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_rectangle.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

#ifdef KMC_DIAG_HOOKS
constexpr int kQueryElems = 512;
constexpr int kMergeElems = 2;
constexpr int64_t kSlabMinRefs = 8;
#else
constexpr int kQueryElems = 14336;
constexpr int kMergeElems = 4096;
constexpr int64_t kSlabMinRefs = 1;
#endif
constexpr int kCandElems = 4096;
constexpr int kMergeBlock = 256;
constexpr int kMergeCap = 4096;  // the merge buffer as declared: >= kMergeElems and >= 2 pow2(KMC_NEAREST_MAX_TOP)
constexpr uint64_t kMaxRefs = 0xFFFFFFFEull;  // the index is 32 bits and UINT32_MAX marks an empty slot

static_assert(2 * KMC_NEAREST_MAX_TOP <= kMergeCap && kMergeElems <= kMergeCap, "merge buffer");
static_assert(2 * KMC_NEAREST_MAX_TOP <= kCandElems, "one candidate buffer holds top + kTileMax keys");

// (the rectangle: the shape Rectangle and rectangle_tiling of kmc_sketch_rectangle.h)
// ---------------------------------------------------------------------------
// the nearest references
// ---------------------------------------------------------------------------
struct NParams {
    const uint64_t *q, *r;
    const uint32_t *qs, *rs;
    int64_t m, n;
    int64_t nqt;  // query tiles
    int64_t per;  // references per slab, a multiple of Tr
    int64_t S;    // slabs
    uint32_t s, top, min_shared;
    int k, Tq, Tr;
    int C;     // keys of one candidate buffer: a power of two >= top + Tr
    int P, M;  // merge: pow2(top) kept, buffer of M keys
    uint64_t *ws_keys;  // [m][S][top]
    uint32_t *ws_cnt;   // [m][S]
    uint32_t *hit_refs, *hit_shared, *hit_denom, *hit_counts;
    float *hit_dist;
};

__device__ __forceinline__ uint64_t hit_key(uint32_t shared, uint32_t denom, uint32_t ref) {
    const uint64_t code = ((uint64_t)shared << 30) / denom;  // <= 2^30
    return (((1ull << 30) - code) << 32) | ref;
}

// Every candidate buffer sorted and cut to its `top` smallest keys; a buffer that
// holds `top` of them sets its query's threshold.  Called by the whole workgroup,
// after a barrier that follows the last append.
__device__ __forceinline__ void compact(uint64_t *cand, uint32_t *cnt, uint64_t *thr, int *full, int Tq, int C,
                                        int top, int tid) {
    for (int e = tid; e < Tq * C; e += kDistBlock) {
        const int a = e / C, i = e - a * C;
        if ((uint32_t)i >= cnt[a]) cand[e] = kFill;
    }
    __syncthreads();
    bitonic_sort<kDistBlock>(cand, Tq, C, tid, [] { __syncthreads(); });
    if (tid < Tq) {
        const uint32_t c = cnt[tid] < (uint32_t)top ? cnt[tid] : (uint32_t)top;
        cnt[tid] = c;
        if (c == (uint32_t)top) thr[tid] = cand[tid * C + top - 1];
    }
    if (tid == 0) *full = 0;
    __syncthreads();
}

template <bool STAGE>
__global__ __launch_bounds__(kDistBlock) void nearest_slab_kernel(NParams p) {
    __shared__ uint64_t rows[STAGE ? kQueryElems : 1];  // query rows: [a * s], the chunk's reference rows: [(Tq + b) * s]
    __shared__ uint64_t cand[kCandElems];                // query a's candidates: [a * C, a * C + cnt[a])
    __shared__ uint64_t thr[kTileMax];                   // only keys below it can still be among the top
    __shared__ uint32_t cnt[kTileMax];
    __shared__ int full;
    const int tid = threadIdx.x;
    const int Tq = p.Tq, Tr = p.Tr, C = p.C, s = (int)p.s, top = (int)p.top;
    const int64_t slab = blockIdx.y;
    const int64_t r_lo = slab * p.per;
    const int64_t r_hi = r_lo + p.per < p.n ? r_lo + p.per : p.n;
    for (int64_t qt = blockIdx.x; qt < p.nqt; qt += gridDim.x) {
        const int64_t i0 = qt * Tq;
        const TileRows A{p.q, p.qs, i0, p.m, rows};
        __syncthreads();  // the last tile's readers are done
        if (tid < Tq) {
            cnt[tid] = 0;
            thr[tid] = kFill;
        }
        if (tid == 0) full = 0;
        if constexpr (STAGE) stage_rows(A, Tq, s, tid);
        for (int64_t j0 = r_lo; j0 < r_hi; j0 += Tr) {
            const TileRows B{p.r, p.rs, j0, r_hi, rows + Tq * s};
            __syncthreads();  // the last chunk's pairs are done, the counts final
            if (tid < Tq && cnt[tid] + (uint32_t)Tr > (uint32_t)C) full = 1;
            if constexpr (STAGE) stage_rows(B, Tr, s, tid);
            __syncthreads();
            if (full) compact(cand, cnt, thr, &full, Tq, C, top, tid);  // (the same answer in every thread)
            tile_pairs<STAGE>(A, B, Tq, Tr, s, tid, [](int64_t, int64_t) { return true; },
                              [&](int a, int, int64_t, int64_t j, uint32_t sh, uint32_t dn) {
                                  if (dn == 0 || sh < p.min_shared) return;
                                  const uint64_t key = hit_key(sh, dn, (uint32_t)j);
                                  if (key < thr[a]) {
                                      // at most Tr appends per query and chunk, and count + Tr <= C before it
                                      const uint32_t at = atomicAdd(&cnt[a], 1u);
                                      if (at < (uint32_t)C) cand[a * C + at] = key;
                                  }
                              });
        }
        __syncthreads();
        compact(cand, cnt, thr, &full, Tq, C, top, tid);
        for (int e = tid; e < Tq * top; e += kDistBlock) {
            const int a = e / top, x = e - a * top;
            const int64_t i = i0 + a;
            if (i < p.m && (uint32_t)x < cnt[a]) p.ws_keys[(i * p.S + slab) * top + x] = cand[a * C + x];
        }
        if (tid < Tq && i0 + tid < p.m) p.ws_cnt[(i0 + tid) * p.S + slab] = cnt[tid];
    }
}

// One workgroup per query: the `top` smallest of the slabs' survivors, then the hit arrays.
__global__ __launch_bounds__(kMergeBlock) void nearest_merge_kernel(NParams p) {
    __shared__ uint64_t buf[kMergeCap];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int top = (int)p.top, P = p.P, M = p.M, s = (int)p.s;
    const int64_t total = p.S * top;  // slots of one query in the workspace
    for (int64_t q = blockIdx.x; q < p.m; q += gridDim.x) {
        __syncthreads();  // the last query's readers are done
        for (int i = tid; i < P; i += kMergeBlock) buf[i] = kFill;
        for (int64_t e0 = 0; e0 < total; e0 += M - P) {
            for (int i = tid; i < M - P; i += kMergeBlock) {
                const int64_t e = e0 + i;
                uint64_t v = kFill;
                if (e < total) {
                    const int64_t sl = e / top;
                    const int x = (int)(e - sl * top);
                    if ((uint32_t)x < p.ws_cnt[q * p.S + sl]) v = p.ws_keys[(q * p.S + sl) * top + x];
                }
                buf[P + i] = v;
            }
            __syncthreads();
            bitonic_sort<kMergeBlock>(buf, 1, M, tid, [] { __syncthreads(); });
        }
        __syncthreads();
        // ascending, the fill last: the hits are the keys before the first fill among the first `top`
        for (int i = tid; i < top; i += kMergeBlock) {
            const uint64_t key = buf[i];
            const bool hit = key != kFill;
            const int64_t o = q * top + i;
            p.hit_refs[o] = hit ? (uint32_t)key : UINT32_MAX;
            if (!hit) {
                if (p.hit_shared) p.hit_shared[o] = 0;
                if (p.hit_denom) p.hit_denom[o] = 0;
                if (p.hit_dist) p.hit_dist[o] = __uint_as_float(0x7fc00000u);
                if (i == 0) p.hit_counts[q] = 0;
            } else if (i == top - 1 || buf[i + 1] == kFill) {
                p.hit_counts[q] = (uint32_t)i + 1;
            }
        }
        if (total == 0 || (!p.hit_shared && !p.hit_denom && !p.hit_dist)) continue;  // (no reference: no rows at all)
        const int na = row_size(p.qs, q, s);
        for (int i = wave; i < top; i += kMergeBlock / 64) {
            const uint64_t key = buf[i];
            if (key == kFill) break;
            const int64_t j = (int64_t)(uint32_t)key;
            uint32_t sh, dn;
            pair_counts(p.q + q * s, na, p.r + j * s, row_size(p.rs, j, s), s, lane, &sh, &dn);
            if (lane == 0) {
                const int64_t o = q * top + i;
                if (p.hit_shared) p.hit_shared[o] = sh;
                if (p.hit_denom) p.hit_denom[o] = dn;
                if (p.hit_dist) p.hit_dist[o] = mash_distance(sh, dn, p.k);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// The shapes of one kmc_sketch_nearest call: what the launches and the workspace follow.
struct NPlan {
    bool stage;
    int Tq, Tr, C, P, M;
    int64_t nqt, per, S;
};

inline NPlan plan(int64_t m, int64_t n, uint32_t s, uint32_t top, int cus) {
    NPlan L;
    L.C = pow2_at_least((int64_t)top + kTileMax);
    // a query tile is also at most the candidate buffers that fit, before Tr takes the room it leaves
    const TileShape ts = tile_shape(kQueryElems, s, m < kCandElems / L.C ? m : kCandElems / L.C, n);
    L.stage = ts.stage;
    L.Tq = ts.Tq;
    L.Tr = ts.Tr;
    const int64_t Tr = L.Tr;
    L.nqt = ceil_div(m, L.Tq);
#ifdef KMC_DIAG_HOOKS
    int64_t smax = kMaxGridY;
    (void)cus;
#else
    int64_t smax = 2LL * cus / L.nqt;
    if (smax > kMaxGridY) smax = kMaxGridY;
    if (smax < 1) smax = 1;
#endif
    const int64_t chunks = ceil_div(n, Tr);
    int64_t per_chunks = ceil_div(chunks, smax);
    if (per_chunks < ceil_div(kSlabMinRefs, Tr)) per_chunks = ceil_div(kSlabMinRefs, Tr);
    if (per_chunks < 1) per_chunks = 1;
    L.per = per_chunks * Tr;
    L.S = ceil_div(n, L.per);
    L.P = pow2_at_least(top);
    const int fit = pow2_at_least(L.P + L.S * (int64_t)top < kMergeElems ? L.P + L.S * (int64_t)top : kMergeElems);
    L.M = fit > 2 * L.P ? fit : 2 * L.P;
    if (L.M > kMergeCap) L.M = kMergeCap;  // (2 P <= kMergeCap: static_assert above)
    return L;
}

struct NLayout {
    uint64_t *keys;
    uint32_t *cnt;
    size_t bytes;
};

// the one layout behind the size query (base = null) and the bind
inline NLayout layout(void *base, int64_t m, const NPlan &L, uint32_t top) {
    Carver c(base);
    NLayout W;
    W.keys = c.take<uint64_t>((size_t)m * (size_t)L.S * top);
    W.cnt = c.take<uint32_t>((size_t)m * (size_t)L.S);
    W.bytes = c.total();
    return W;
}

inline bool nearest_args_ok(uint64_t num_queries, uint64_t num_refs, uint32_t sketch_size, uint32_t top) {
    return sketch_size_ok(sketch_size) && top >= 1 && top <= KMC_NEAREST_MAX_TOP && num_refs <= kMaxRefs &&
           num_queries <= KMC_SPARSE_MAX_SEQS;
}

DeviceCache n_ws;  // library-owned workspace

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" int kmc_sketch_distances_rect(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                                         const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                         uint32_t sketch_size, int k, float *out, uint32_t *shared, uint32_t *denom,
                                         hipStream_t stream) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (num_queries == 0 || num_refs == 0) return KMC_OK;
    if (!q_sketches || !q_sizes || !r_sketches || !r_sizes || !out) return KMC_ERR_INVALID_ARG;
    if (!sketch_size_ok(sketch_size)) return KMC_ERR_INVALID_ARG;
    if (num_queries > KMC_SPARSE_MAX_SEQS || num_refs > KMC_SPARSE_MAX_SEQS) return KMC_ERR_INVALID_ARG;
    Tiling p;
    const bool stage = rectangle_tiling(p, q_sketches, q_sizes, (int64_t)num_queries, r_sketches, r_sizes,
                                        (int64_t)num_refs, sketch_size);
    launch_tiles<Rectangle>(p, stage, DistOut{out, shared, denom, k}, stream);
    return (int)hipGetLastError();
}

extern "C" size_t kmc_sketch_nearest_workspace_size(uint64_t num_queries, uint64_t num_refs, uint32_t sketch_size,
                                                    uint32_t top, int device) {
    if (!nearest_args_ok(num_queries, num_refs, sketch_size, top) || device < 0) return 0;
    if (num_queries == 0 || num_refs == 0) return 0;  // no slab, no workspace
    int cus = 0;  // (the arguments are checked before any HIP call)
    if (device_cus(device, &cus)) return 0;
    const int64_t m = (int64_t)num_queries;
    return layout(nullptr, m, plan(m, (int64_t)num_refs, sketch_size, top, cus), top).bytes;
}

extern "C" int kmc_sketch_nearest(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                                  const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                  uint32_t sketch_size, int k, uint32_t top, uint32_t min_shared, uint32_t *hit_refs,
                                  uint32_t *hit_shared, uint32_t *hit_denom, float *hit_dist, uint32_t *hit_counts,
                                  void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (!nearest_args_ok(num_queries, num_refs, sketch_size, top)) return KMC_ERR_INVALID_ARG;
    if (num_queries == 0) return KMC_OK;
    if (!hit_refs || !hit_counts) return KMC_ERR_INVALID_ARG;
    if (num_refs > 0 && (!q_sketches || !q_sizes || !r_sketches || !r_sizes)) return KMC_ERR_INVALID_ARG;
    NParams p;
    p.q = q_sketches;
    p.qs = q_sizes;
    p.r = r_sketches;
    p.rs = r_sizes;
    p.m = (int64_t)num_queries;
    p.n = (int64_t)num_refs;
    p.s = sketch_size;
    p.top = top;
    p.min_shared = min_shared;
    p.k = k;
    p.hit_refs = hit_refs;
    p.hit_shared = hit_shared;
    p.hit_denom = hit_denom;
    p.hit_dist = hit_dist;
    p.hit_counts = hit_counts;
    p.ws_keys = nullptr;
    p.ws_cnt = nullptr;
    p.nqt = p.per = p.S = 0;
    p.Tq = p.Tr = p.C = 0;
    p.P = pow2_at_least(top);
    p.M = 2 * p.P;
    if (p.n > 0) {
        int device = 0, cus = 0;
        if (int e = current_device_cus(&device, &cus)) return e;
        const NPlan L = plan(p.m, p.n, sketch_size, top, cus);
        NLayout W;
        if (int e = bind_layout(n_ws, device, workspace, workspace_bytes, 0,
                                [&](void *b) { return layout(b, p.m, L, top); }, &W))
            return e;
        p.ws_keys = W.keys;
        p.ws_cnt = W.cnt;
        p.nqt = L.nqt;
        p.per = L.per;
        p.S = L.S;
        p.Tq = L.Tq;
        p.Tr = L.Tr;
        p.C = L.C;
        p.P = L.P;
        p.M = L.M;
        // every count[q][slab] is written by its workgroup, and only keys below a count are read
        const dim3 grid((unsigned)(L.nqt < kMaxGridX ? L.nqt : kMaxGridX), (unsigned)L.S);
        if (L.stage)
            hipLaunchKernelGGL(nearest_slab_kernel<true>, grid, dim3(kDistBlock), 0, stream, p);
        else
            hipLaunchKernelGGL(nearest_slab_kernel<false>, grid, dim3(kDistBlock), 0, stream, p);
    }
    // without a reference: no slab, every row filled
    const unsigned mgrid = (unsigned)(p.m < kMaxGridX ? p.m : kMaxGridX);
    hipLaunchKernelGGL(nearest_merge_kernel, dim3(mgrid), dim3(kMergeBlock), 0, stream, p);
    return (int)hipGetLastError();
}
