// kmc_sketch_links.hip — the pairs of sketch rows within a distance, as a list, without
// the triangle or the rectangle of all distances: kmc_sketch_links (pairs i < j of one row
// set) and kmc_sketch_links_rect (every query against every reference).
//
// A pair is listed iff neither row is empty and linked(shared, denom, min_jaccard)
// (kmc_sketch_pair.h): kmc_sketch_cluster's rule on pair_counts' values, so the triangle's
// list is exactly the edge set whose components the clustering returns.  An entry is
// {i, j, shared, denom} and, beside it, mash_distance(shared, denom, k): the float of
// kmc_sketch_distances[_rect] for that pair.
//
// The tile loop of kmc_sketch_pair.h (sketch_tile_kernel) over both shapes (Triangle of
// kmc_sketch_triangle.h, Rectangle of kmc_sketch_rectangle.h), staged or not, with the
// tiling of the distance kernels and the consumer LinkOut, the only one with an epilogue.
// tile_pairs hands its sink one pair per wavefront, from lane 0 (LinkOut::sink); a listed
// pair goes to the tile's buffer in LDS (at most
// Tq x Tr <= kTileMax^2 entries of 16 bytes) at a position taken from an LDS counter.
// Behind a barrier one thread reserves the tile's block of the output,
//     base = atomic add(*num_links, count)       (64-bit, relaxed, agent scope)
// and behind a second barrier the workgroup writes entry base + t for every t < count
// with base + t < capacity: one 16-byte store and one float per entry, consecutive
// threads to consecutive entries.  One global atomic per tile that lists anything, none
// for a tile that lists nothing; *num_links ends as the number of listed pairs whether
// they fit or not; a block that straddles `capacity` writes the part below it.  The
// order of the entries is the order in which the tiles reserve: unspecified.
//
// The LDS counter is never zeroed after the launch's first tile: every thread keeps the
// value it had before the tile (`seen`), positions are taken relative to it, and the
// tile's count is its growth (uint32, wrap-around is harmless).  Barriers per tile: the
// top one (the last tile's readers of the rows, the buffer and `base` are done; the
// staged kernel has it anyway), the staged kernel's second one, one after the pairs and,
// only for a tile that lists a pair, one after the reservation.  The trip count of the
// tile loop and the tile's count are the same in every thread, so every thread reaches
// every barrier.
//
// LDS: the distance tile's kDistElems values (128 KiB shipped, 4 KiB under
// -DKMC_DIAG_HOOKS) and the buffer (16 KiB / 256 B), the counter and the base.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_rectangle.h"
#include "kmc_sketch_triangle.h"

namespace kmc {
namespace {

constexpr int kLinkTile = kTileMax * kTileMax;  // entries of one tile at most

static_assert(sizeof(kmc_sketch_link) == 16 && sizeof(kmc_sketch_link) == sizeof(uint4), "one 16-byte store per entry");
static_assert(kLinkTile <= kDistBlock, "a thread per entry of a tile");  // (tile_edge and tile_shape cap both edges at kTileMax)

// The consumer of both entry points (sketch_tile_kernel over either shape): the pairs
// of two non-empty rows; a linked one goes to the tile's buffer, and the epilogue
// reserves the tile's block of the output and writes it.
struct LinkOut {
    static constexpr bool kEpilogue = true;
    struct Lds {
        uint4 found[kLinkTile];   // the tile's listed pairs: {i, j, shared, denom}
        uint32_t taken;           // positions handed out since the launch began
        unsigned long long base;  // the tile's first entry in the output
    };
    double min_jaccard;
    int k;
    uint4 *links;  // kmc_sketch_link[capacity], or null
    float *dist;   // [capacity], or null
    uint64_t capacity;
    unsigned long long *num_links;
    uint32_t seen;  // `taken` before this tile, every thread's own (the host: 0)

    __device__ __forceinline__ void begin(Lds &L, int tid) const {
        if (tid == 0) L.taken = 0;  // (published by the first tile's top barrier)
    }
    // the last tile's readers are done, of found and of base too: the unstaged loop
    // has no barrier of its own here
    template <bool STAGE>
    __device__ __forceinline__ void top() const {
        if constexpr (!STAGE) __syncthreads();
    }
    __device__ __forceinline__ bool counts(const Tiling &p, int64_t i, int64_t j) const {
        return p.qs[i] > 0 && p.rs[j] > 0;
    }
    template <class Shape>
    __device__ __forceinline__ void sink(const Tiling &, Lds &L, int64_t i, int64_t j, uint32_t sh, uint32_t dn) const {
        if (!linked(sh, dn, min_jaccard)) return;
        // a pair is handed over once: fewer than Tq * Tr <= kLinkTile positions per tile
        const uint32_t at = atomicAdd(&L.taken, 1u) - seen;
        if (at < (uint32_t)kLinkTile) L.found[at] = make_uint4((uint32_t)i, (uint32_t)j, sh, dn);
    }
    // (behind the barrier after the tile's pairs: they are in found)
    __device__ __forceinline__ void epilogue(const Tiling &, Lds &L, int tid) {
        const uint32_t now = L.taken;  // (the same in every thread: nothing is appended before the next top barrier)
        const uint32_t count = now - seen;
        seen = now;
        if (count == 0) return;
        if (tid == 0)
            L.base = __hip_atomic_fetch_add(num_links, (unsigned long long)count, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint64_t at = (uint64_t)L.base + (uint64_t)tid;
        if ((uint32_t)tid < count && tid < kLinkTile && at < capacity) {
            const uint4 e = L.found[tid];
            links[at] = e;
            if (dist) dist[at] = mash_distance(e.z, e.w, k);
        }
    }
};

// what both entry points refuse before the rows are looked at, in the header's order
inline int links_args(uint64_t rows_a, uint64_t rows_b, uint32_t sketch_size, int k, double min_jaccard,
                      const kmc_sketch_link *links, uint64_t capacity, const uint64_t *num_links) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (!sketch_size_ok(sketch_size)) return KMC_ERR_INVALID_ARG;
    if (rows_a > KMC_SPARSE_MAX_SEQS || rows_b > KMC_SPARSE_MAX_SEQS) return KMC_ERR_INVALID_ARG;
    if (!min_jaccard_ok(min_jaccard)) return KMC_ERR_INVALID_ARG;
    if (!num_links) return KMC_ERR_INVALID_ARG;
    if (!links && capacity > 0) return KMC_ERR_INVALID_ARG;
    return KMC_OK;
}

inline LinkOut link_out(double min_jaccard, int k, kmc_sketch_link *links, float *dist, uint64_t capacity,
                        uint64_t *num_links) {
    // (null links: capacity is 0, links_args saw to it, and nothing is written)
    return LinkOut{min_jaccard, k, reinterpret_cast<uint4 *>(links), dist, capacity,
                   reinterpret_cast<unsigned long long *>(num_links), 0u};
}

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" int kmc_sketch_links(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                                uint32_t sketch_size, int k, double min_jaccard, kmc_sketch_link *links, float *dist,
                                uint64_t capacity, uint64_t *num_links, hipStream_t stream) {
    if (int e = links_args(num_seqs, num_seqs, sketch_size, k, min_jaccard, links, capacity, num_links)) return e;
    const bool pairs = num_seqs >= 2;
    if (pairs && (!sketches || !sketch_sizes)) return KMC_ERR_INVALID_ARG;
    if ((uintptr_t)links % 16) return KMC_ERR_ALIGNMENT;
    if (hipError_t he = hipMemsetAsync(num_links, 0, sizeof(uint64_t), stream)) return (int)he;
    if (!pairs) return KMC_OK;
    Tiling p;
    const bool stage = triangle_tiling(p, sketches, sketch_sizes, (int64_t)num_seqs, sketch_size);
    launch_tiles<Triangle>(p, stage, link_out(min_jaccard, k, links, dist, capacity, num_links), stream);
    return (int)hipGetLastError();
}

extern "C" int kmc_sketch_links_rect(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                                     const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                     uint32_t sketch_size, int k, double min_jaccard, kmc_sketch_link *links,
                                     float *dist, uint64_t capacity, uint64_t *num_links, hipStream_t stream) {
    if (int e = links_args(num_queries, num_refs, sketch_size, k, min_jaccard, links, capacity, num_links)) return e;
    const bool pairs = num_queries > 0 && num_refs > 0;
    if (pairs && (!q_sketches || !q_sizes || !r_sketches || !r_sizes)) return KMC_ERR_INVALID_ARG;
    if ((uintptr_t)links % 16) return KMC_ERR_ALIGNMENT;
    if (hipError_t he = hipMemsetAsync(num_links, 0, sizeof(uint64_t), stream)) return (int)he;
    if (!pairs) return KMC_OK;
    Tiling p;
    const bool stage = rectangle_tiling(p, q_sketches, q_sizes, (int64_t)num_queries, r_sketches, r_sizes,
                                        (int64_t)num_refs, sketch_size);
    launch_tiles<Rectangle>(p, stage, link_out(min_jaccard, k, links, dist, capacity, num_links), stream);
    return (int)hipGetLastError();
}
