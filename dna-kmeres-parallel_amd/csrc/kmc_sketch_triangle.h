// kmc_sketch_triangle.h — all pairs i < j of one row set as a shape of the tile loop of
// kmc_sketch_pair.h, and the tiling all of its users launch with: the packed triangle
// of distances (kmc_sketch.hip), the links of the clustering (kmc_sketch_cluster.hip) and
// the list of those links (kmc_sketch_links.hip).
// One definition, so that all visit the same pairs in the same tiles.
#pragma once

#include "kmc_dist_common.h"
#include "kmc_sketch_pair.h"

namespace kmc {
namespace {

// The packed upper triangle as a shape of sketch_tile_kernel (kmc_sketch_pair.h): both
// row sets are the one set, the tiles are square, and tile t is the t-th of the nt
// tile rows' upper triangle, diagonal included.
struct Triangle {
    static __device__ __forceinline__ void tile(const Tiling &p, int64_t t, uint64_t *buf, TileRows &A, TileRows &B) {
        // with its diagonal it is the strict triangle of nt + 1: b nt - b (b - 1) / 2 = (nt + 1) b - b (b + 1) / 2
        const int64_t bi = tri_row(t, p.nrt + 1), bj = bi + (t - tri_row_start(bi, p.nrt + 1));
        A = TileRows{p.q, p.qs, bi * p.Tq, p.n, buf};
        B = TileRows{p.q, p.qs, bj * p.Tq, p.n, buf + p.Tq * (int)p.s};
    }
    static __device__ __forceinline__ bool counts(int64_t i, int64_t j) { return i < j; }
    static __device__ __forceinline__ int64_t index(const Tiling &p, int64_t i, int64_t j) {
        return tri_index(i, j, p.n);
    }
};

// The rows, the tile edge and the tile count of the triangle over n >= 1 rows of s
// values into p; returns whether the rows are staged.
inline bool triangle_tiling(Tiling &p, const uint64_t *sketches, const uint32_t *sizes, int64_t n, uint32_t s) {
    p.q = p.r = sketches;
    p.qs = p.rs = sizes;
    p.m = p.n = n;
    p.s = s;
    bool stage = false;
    int T = tile_edge(kDistElems, s, &stage);  // square: not the rectangle's Tr
    if ((int64_t)T > n) T = (int)n;
    p.Tq = p.Tr = T;
    p.nrt = ceil_div(n, T);
    p.ntiles = p.nrt * (p.nrt + 1) / 2;
    return stage;
}

}  // namespace
}  // namespace kmc
