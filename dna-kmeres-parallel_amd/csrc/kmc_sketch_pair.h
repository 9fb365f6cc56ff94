// kmc_sketch_pair.h — what the sketch translation units share (device code and host
// rules, no entry point), one definition each so that a fix reaches every user:
//   rows and sets   lower_bound and bitonic_sort, for global and LDS pointers
//   a pair          pair_counts, mash_distance and linked: a pair has the same shared,
//                   denom, float and link wherever it is computed
//   a tile          stage_rows, tile_pairs (one wavefront per pair of a Tq x Tr tile)
//                   and sketch_tile_kernel, the one loop over the tiles of a Tiling:
//                   the packed triangle and the query x reference rectangle are its
//                   shape policies (kmc_sketch_triangle.h, kmc_sketch_rectangle.h);
//                   the distances (DistOut, here), the clustering and the pair list
//                   are its consumers, each beside its entry point; launch_tiles
//                   launches it.  The top-hits search streams its own tiles through
//                   tile_pairs
//   host            tile_edge / tile_shape, for_cap, pow2_at_least, ceil_div and the
//                   argument checks the entry points share
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kmc.h"
#include "kmc_internal.h"

namespace kmc {
namespace {

// shipped / under -DKMC_DIAG_HOOKS (see kmc_sketch.hip)
#ifdef KMC_DIAG_HOOKS
constexpr int kDistElems = 512;  // LDS capacity of a distance tile, values
constexpr int kTileMax = 4;      // tile edge at most, rows
#else
constexpr int kDistElems = 16384;
constexpr int kTileMax = 32;
#endif
constexpr int kDistBlock = 1024;
constexpr int kStageMinTile = 4;  // a smaller staged tile leaves most of the 16 wavefronts idle
constexpr int kGlobalTile = 8;
constexpr uint64_t kFill = ~0ull;  // after a row's values, and the padding of every sort

inline bool sketch_size_ok(uint32_t s) { return s >= 1 && s <= KMC_SKETCH_MAX_SIZE; }
inline bool canon_k_ok(int k) { return k >= 1 && k <= KMC_CANON_MAX_K; }
inline bool min_jaccard_ok(double x) { return x >= 0.0 && x <= 1.0; }  // (NaN: no)

__host__ __device__ inline int pow2_at_least(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// f(the LDS capacity a kernel is built with for sketch size s, as an integral constant)
template <class F>
inline void for_cap(uint32_t s, F &&f) {
    if (s <= 1024) f(std::integral_constant<int, 1024>{});
    else if (s <= 4096) f(std::integral_constant<int, 4096>{});
    else f(std::integral_constant<int, KMC_SKETCH_MAX_SIZE>{});
}

// The edge of a square tile whose 2T rows of s values fit `elems` values of LDS, at
// most kTileMax; below kStageMinTile the rows stay in global memory (*stage =
// false) and the edge is kGlobalTile, for locality only.  The triangle's tile:
// T = min(edge, n), square whatever elems / s is.
inline int tile_edge(int elems, uint32_t s, bool *stage) {
    int T = elems / (int)s / 2;
    if (T > kTileMax) T = kTileMax;
    *stage = T >= kStageMinTile;
    if (!*stage) T = kGlobalTile < kTileMax ? kGlobalTile : kTileMax;
    return T;
}

// A tile of m x n pairs of two row sets: Tq = min(edge, m) rows of the first, and
// the room they leave for the second, Tr = min(kTileMax, elems / s - Tq, n) (the
// edge when the rows are not staged).
struct TileShape {
    bool stage;
    int Tq, Tr;
};

inline TileShape tile_shape(int elems, uint32_t s, int64_t m, int64_t n) {
    TileShape L;
    const int T = tile_edge(elems, s, &L.stage);
    const int64_t Tq = T < m ? T : m;
    int64_t Tr = T;
    if (L.stage) {
        Tr = elems / (int)s - Tq;
        if (Tr > kTileMax) Tr = kTileMax;
    }
    if (Tr > n) Tr = n;
    L.Tq = (int)Tq;
    L.Tr = (int)(Tr < 1 ? 1 : Tr);
    return L;
}

// first index in a[0, n) whose value is not below v
template <class P>
__device__ __forceinline__ int lower_bound(P a, int n, uint64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Ascending bitonic sort of `segs` consecutive segments of `len` keys (a power of
// two >= 2) each, by BLOCK threads; `barrier` orders the steps (and the caller's
// writes of buf before the first).  The segments are one network over segs * len
// keys that stops at len: a thread's pair never leaves its segment, and the
// direction bit is taken inside the segment.  ONE_PASS: the caller promises segs *
// len <= 2 BLOCK, a pair per thread at most, and a step has no loop (the set merge,
// whose steps run back to back in one workgroup, was 13-16 % slower through the loop).
template <int BLOCK, bool ONE_PASS = false, class Barrier>
__device__ __forceinline__ void bitonic_sort(uint64_t *buf, int segs, int len, int tid, Barrier barrier) {
    const int pairs = segs * (len >> 1);
    for (int kk = 2; kk <= len; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < pairs; t += BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t x = buf[i], y = buf[l];
                const bool up = (i & kk & (len - 1)) == 0;
                if ((x > y) == up) {
                    buf[i] = y;
                    buf[l] = x;
                }
                if constexpr (ONE_PASS) break;
            }
            barrier();
        }
    }
}

__device__ __forceinline__ float mash_distance(uint32_t shared, uint32_t denom, int k) {
    if (denom == 0) return __uint_as_float(0x7fc00000u);
    if (shared == 0) return 1.0f;
    if (shared == denom) return 0.0f;
    const double j = (double)shared / (double)denom;
    double d = -log(2.0 * j / (1.0 + j)) / (double)k;
    if (d > 1.0) d = 1.0;
    return (float)d;
}

// The link rule of kmc_sketch_cluster and kmc_sketch_links[_rect] on a pair's counts: one
// IEEE double product and one compare, the same on host and device.  (That neither row
// is empty is the caller's `counts` predicate: the tile loop never hands such a pair on.)
__host__ __device__ inline bool linked(uint32_t shared, uint32_t denom, double min_jaccard) {
    return denom > 0 && (double)shared >= min_jaccard * (double)denom;
}

// the values of row r that count: its size, at most s
__device__ __forceinline__ int row_size(const uint32_t *sizes, int64_t r, int s) {
    const uint32_t n = sizes[r];
    return n < (uint32_t)s ? (int)n : s;
}

// One wavefront, one pair: A = row i (na values), B = row j (nb values), ascending.
template <class PA, class PB>
__device__ __forceinline__ void pair_counts(PA A, int na, PB B, int nb, int s, int lane, uint32_t *shared_out,
                                            uint32_t *denom_out) {
    const bool known = na == s || nb == s;  // the union holds at least s values
    int M = 0, sh = 0;
    for (int x0 = 0; x0 < na; x0 += 64) {
        const int x = x0 + lane;
        const bool act = x < na;
        int pos = 0;
        bool match = false;
        if (act) {
            const uint64_t v = A[x];
            pos = lower_bound(B, nb, v);
            match = pos < nb && B[pos] == v;
        }
        const unsigned long long mm = __ballot(match);
        const int before = __popcll(mm & (~0ull >> (63 - lane)));  // matches among A[0..x]
        const int rank = x + 1 + pos + (match ? 1 : 0) - (M + before);
        const bool in_u = act && rank <= s;
        sh += __popcll(__ballot(match && in_u));
        M += __popcll(mm);
        if (known && __ballot(act && !in_u)) break;  // ranks only grow
    }
    const int uni = na + nb - M;  // |A u B| when the loop ran to its end
    *shared_out = (uint32_t)sh;
    *denom_out = (uint32_t)(known ? s : (uni < s ? uni : s));
}

// One of the two row sets of a tile: the rows [row0, row0 + T) of sk below `end`,
// staged at lds[slot * s] when the kernel stages.
struct TileRows {
    const uint64_t *sk;
    const uint32_t *sizes;
    int64_t row0, end;
    uint64_t *lds;
};

// the first sizes[row] values of each of R's T rows into its LDS slots
__device__ __forceinline__ void stage_rows(const TileRows &R, int T, int s, int tid) {
    for (int e = tid; e < T * s; e += kDistBlock) {
        const int slot = e / s, x = e - slot * s;
        const int64_t row = R.row0 + slot;
        if (row < R.end && (uint32_t)x < R.sizes[row]) R.lds[e] = R.sk[row * s + x];
    }
}

// The pairs (i, j) of the Tq x Tr tile of A's and B's rows that exist and that
// `counts`, one wavefront per pair; lane 0 hands sink(a, b, i, j, shared, denom) the
// counts of the pair of slots (a, b).  Called by the whole workgroup, the staged
// rows behind a barrier.
template <bool STAGE, class Counts, class Sink>
__device__ __forceinline__ void tile_pairs(const TileRows &A, const TileRows &B, int Tq, int Tr, int s, int tid,
                                           Counts counts, Sink sink) {
    const int lane = tid & 63;
    for (int pp = tid >> 6; pp < Tq * Tr; pp += kDistBlock / 64) {
        const int a = pp / Tr, b = pp - a * Tr;
        const int64_t i = A.row0 + a, j = B.row0 + b;
        if (i >= A.end || j >= B.end || !counts(i, j)) continue;
        const int na = row_size(A.sizes, i, s), nb = row_size(B.sizes, j, s);
        uint32_t sh, dn;
        if constexpr (STAGE)
            pair_counts(A.lds + a * s, na, B.lds + b * s, nb, s, lane, &sh, &dn);
        else
            pair_counts(A.sk + i * s, na, B.sk + j * s, nb, s, lane, &sh, &dn);
        if (lane == 0) sink(a, b, i, j, sh, dn);
    }
}

// The tiling of m query rows against n reference rows in tiles of Tq x Tr, filled by
// the shape's host function (triangle_tiling, rectangle_tiling): the rows and the
// geometry, nothing of what a consumer does with a pair.
struct Tiling {
    const uint64_t *q, *r;
    const uint32_t *qs, *rs;
    int64_t m, n;
    int64_t nrt, ntiles;  // tile columns; tiles
    uint32_t s;
    int Tq, Tr;
};

struct NoLds {};  // the LDS state of a consumer that has no epilogue

// All pairs that a shape counts, tile by tile, handed to a consumer: the one tile loop
// of the distances, the clustering and the pair list.  A Shape gives
//   tile    the two row sets of tile t, staged at buf and buf + Tq * s
//   counts  whether the pair (i, j) is one of the shape's
//   index   where a pair's results go in the shape's own output order
// A Consumer is a small struct passed by value (its outputs and its threshold) with
//   counts(p, i, j)                     what else a pair must meet to be counted at all
//   sink<Shape>(p, L, i, j, sh, dn)     lane 0 of the pair's wavefront, with its counts
//   kEpilogue, Lds                      whether the whole workgroup runs a step after a
//       tile's pairs, behind a barrier, on LDS state L of the consumer's own type:
//       begin(L, tid) before the first tile, top<STAGE>() where a tile starts (the
//       staged loop has a barrier there; what the consumer needs beyond it is its own),
//       epilogue(p, L, tid) after the barrier behind the pairs.  Without one (NoLds)
//       the loop holds none of these, no LDS and no barrier for it.
template <class Shape, bool STAGE, class Consumer>
__global__ __launch_bounds__(kDistBlock) void sketch_tile_kernel(Tiling p, Consumer c) {
    __shared__ uint64_t buf[STAGE ? kDistElems : 1];  // query rows: [a * s], reference rows: [(Tq + b) * s]
    __shared__ typename Consumer::Lds L;
    const int tid = threadIdx.x, Tq = p.Tq, Tr = p.Tr, s = (int)p.s;
    if constexpr (Consumer::kEpilogue) c.begin(L, tid);
    for (int64_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        TileRows A, B;
        Shape::tile(p, t, buf, A, B);
        if constexpr (Consumer::kEpilogue) c.template top<STAGE>();
        if constexpr (STAGE) {
            __syncthreads();  // the last tile's readers are done
            stage_rows(A, Tq, s, tid);
            stage_rows(B, Tr, s, tid);
            __syncthreads();
        }
        tile_pairs<STAGE>(A, B, Tq, Tr, s, tid,
                          [&](int64_t i, int64_t j) { return Shape::counts(i, j) && c.counts(p, i, j); },
                          [&](int, int, int64_t i, int64_t j, uint32_t sh, uint32_t dn) {
                              c.template sink<Shape>(p, L, i, j, sh, dn);
                          });
        if constexpr (Consumer::kEpilogue) {
            __syncthreads();  // the tile's pairs went through the sink
            c.epilogue(p, L, tid);
        }
    }
}

// staged or not, one workgroup per tile up to the grid's limit (the caller reads the
// launch's error with its others)
template <class Shape, class Consumer>
inline void launch_tiles(const Tiling &p, bool stage, const Consumer &c, hipStream_t stream) {
    const unsigned grid = (unsigned)(p.ntiles < kMaxGridX ? p.ntiles : kMaxGridX);
    if (stage)
        hipLaunchKernelGGL((sketch_tile_kernel<Shape, true, Consumer>), dim3(grid), dim3(kDistBlock), 0, stream, p, c);
    else
        hipLaunchKernelGGL((sketch_tile_kernel<Shape, false, Consumer>), dim3(grid), dim3(kDistBlock), 0, stream, p, c);
}

// The consumer of kmc_sketch_distances and kmc_sketch_distances_rect: every pair of the
// shape, its distance (and counts, where asked for) at the shape's index.
struct DistOut {
    static constexpr bool kEpilogue = false;
    using Lds = NoLds;
    float *out;
    uint32_t *shared, *denom;  // or null
    int k;
    __device__ __forceinline__ bool counts(const Tiling &, int64_t, int64_t) const { return true; }
    template <class Shape>
    __device__ __forceinline__ void sink(const Tiling &p, Lds &, int64_t i, int64_t j, uint32_t sh, uint32_t dn) const {
        const int64_t o = Shape::index(p, i, j);
        out[o] = mash_distance(sh, dn, k);
        if (shared) shared[o] = sh;
        if (denom) denom[o] = dn;
    }
};

}  // namespace
}  // namespace kmc
