// kmc_sketch_rectangle.h — every pair of a query row and a reference row as a shape of the
// tile loop of kmc_sketch_pair.h, and the tiling both of its users launch with: the
// rectangle of distances (kmc_sketch_query.hip) and the rectangle's pair list
// (kmc_sketch_links.hip).  One definition, so that both visit the same pairs in the same
// tiles.
#pragma once

#include "kmc_sketch_pair.h"

namespace kmc {
namespace {

// The m x n rectangle as a shape of sketch_tile_kernel (kmc_sketch_pair.h): nrt tiles
// per tile row, every pair of a tile, row-major results.
struct Rectangle {
    static __device__ __forceinline__ void tile(const Tiling &p, int64_t t, uint64_t *buf, TileRows &A, TileRows &B) {
        const int64_t bi = t / p.nrt, bj = t - bi * p.nrt;
        A = TileRows{p.q, p.qs, bi * p.Tq, p.m, buf};
        B = TileRows{p.r, p.rs, bj * p.Tr, p.n, buf + p.Tq * (int)p.s};
    }
    static __device__ __forceinline__ bool counts(int64_t, int64_t) { return true; }
    static __device__ __forceinline__ int64_t index(const Tiling &p, int64_t i, int64_t j) { return i * p.n + j; }
};

// The rows, the tile shape (tile_shape over kDistElems) and the tile count of m >= 1 query
// rows against n >= 1 reference rows of s values into p; returns whether the rows are staged.
inline bool rectangle_tiling(Tiling &p, const uint64_t *q, const uint32_t *qs, int64_t m, const uint64_t *r,
                             const uint32_t *rs, int64_t n, uint32_t s) {
    p.q = q;
    p.qs = qs;
    p.r = r;
    p.rs = rs;
    p.m = m;
    p.n = n;
    p.s = s;
    const TileShape ts = tile_shape(kDistElems, s, m, n);
    p.Tq = ts.Tq;
    p.Tr = ts.Tr;
    p.nrt = ceil_div(n, ts.Tr);
    p.ntiles = ceil_div(m, ts.Tq) * p.nrt;
    return ts.stage;
}

}  // namespace
}  // namespace kmc
