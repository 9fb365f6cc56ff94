// kmc_sketch_cluster.hip — single-linkage clusters of one set of sketch rows at a
// Jaccard threshold, without the matrix of their distances: kmc_sketch_cluster, its
// size query, and the host-only kmc_mash_jaccard_of_distance.
//
// Records i < j are linked iff neither row is empty (so denom > 0) and (double)shared
// >= min_jaccard * (double)denom, shared and denom being kmc_sketch_distances'
// (pair_counts of kmc_sketch_pair.h); the clusters are the connected components of that
// graph, and labels[i] is the smallest index of i's component.  An empty row has
// shared 0 of denom > 0 with every row that is not: only min_jaccard == 0 would accept
// that, and the tile loop does not count such a pair at all, so an empty row is a
// cluster of its own at every threshold.
//
//   init     parent[i] = i
//   link     the tile loop of kmc_sketch_pair.h (sketch_tile_kernel, staged or not) over
//            the triangle's tiling (Triangle and triangle_tiling of
//            kmc_sketch_triangle.h), with a consumer that applies the rule and, on a
//            link, unites the two records in the forest `parent`:
//                find both roots (follow parent until parent[x] == x);
//                hook the larger root under the smaller by a compare-and-swap that
//                succeeds only while parent[larger] == larger;
//                otherwise go on from what the compare-and-swap found there.
//            Every write of parent is that compare-and-swap, and it only ever
//            replaces parent[x] == x by a smaller index: parent[x] <= x always holds, a
//            record that is no root is never written again (parent[x] holds two values
//            in its life, x and then one smaller index), and the root of a tree is its
//            smallest index.  Every read of parent is a relaxed agent-scope atomic
//            load.  Such a load may return an older value of parent[x]; the only older
//            value is x itself, so all a stale read can do is stop a walk
//            early at a record that was a root once and no longer is.  That record is
//            still in the same tree, the compare-and-swap on it fails, returns its
//            present parent, and the walk goes on from there; every retry moves to
//            a strictly smaller index, so it ends.  A link is complete when its
//            compare-and-swap succeeds or both walks reach one root; either way the
//            two records are in one tree from then on.  No fence, no flag, no order
//            between workgroups is needed: a union-find forest is the same
//            partition whatever the order of its unions.
//   flatten  a launch of its own, so that the kernel boundary publishes every link:
//            labels[i] = the root of i, and is_rep[i] = (root == i) when ranks are asked for
//   rank     exclusive scan of is_rep (kmc_scan.h), cluster_index[i] = scan[labels[i]],
//            *num_clusters = scan[n]; skipped when both outputs are NULL
//
// Workspace: parent and is_rep, 4 B per record each; the scan, 8 (n + 1) B; its
// partials, 8 B per 4096 records.  LDS: the distance tile's (kmc_sketch.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "kmc.h"
#include "kmc_internal.h"
#include "kmc_scan.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_triangle.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

constexpr int kLabelBlock = 256;

// (the link rule: linked() of kmc_sketch_pair.h, shared with kmc_sketch_links.hip)

__device__ __forceinline__ uint32_t parent_of(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (x <= the start; parent values only fall)
__device__ __forceinline__ uint32_t root_seen(const uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t up = parent_of(parent, x);
        if (up == x) return x;
        x = up;
    }
}

__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
    a = root_seen(parent, a);
    b = root_seen(parent, b);
    while (a != b) {
        const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
        uint32_t found = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &found, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // hi was hooked meanwhile (found < hi): on from its parent; lo may have been, too
        a = root_seen(parent, found);
        b = root_seen(parent, lo);
    }
}

__global__ __launch_bounds__(kLabelBlock) void cluster_init_kernel(uint32_t *parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLabelBlock)
        parent[i] = (uint32_t)i;
}

// The consumer of the link launch (sketch_tile_kernel over the triangle): the pairs of
// two non-empty rows, and a union for every one that is linked.
struct LinkUnion {
    static constexpr bool kEpilogue = false;
    using Lds = NoLds;
    uint32_t *parent;
    double min_jaccard;
    __device__ __forceinline__ bool counts(const Tiling &p, int64_t i, int64_t j) const {
        return p.qs[i] > 0 && p.qs[j] > 0;  // (the triangle: one row set)
    }
    template <class Shape>
    __device__ __forceinline__ void sink(const Tiling &, Lds &, int64_t i, int64_t j, uint32_t sh, uint32_t dn) const {
        if (linked(sh, dn, min_jaccard)) unite(parent, (uint32_t)i, (uint32_t)j);
    }
};

// after the link launch: plain loads see every hook
__global__ __launch_bounds__(kLabelBlock) void cluster_flatten_kernel(const uint32_t *parent, int64_t n,
                                                                      uint32_t *labels, uint32_t *is_rep) {
    for (int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLabelBlock) {
        uint32_t x = (uint32_t)i;
        for (uint32_t up = parent[x]; up != x; up = parent[x]) x = up;
        labels[i] = x;
        if (is_rep) is_rep[i] = x == (uint32_t)i ? 1u : 0u;
    }
}

// scan[i]: the representatives below i; scan[n]: all of them
__global__ __launch_bounds__(kLabelBlock) void cluster_rank_kernel(const uint32_t *labels, const uint64_t *scan,
                                                                   int64_t n, uint32_t *cluster_index,
                                                                   uint32_t *num_clusters) {
    const int64_t first = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
    if (num_clusters && first == 0) *num_clusters = (uint32_t)scan[n];
    if (!cluster_index) return;
    for (int64_t i = first; i < n; i += (int64_t)gridDim.x * kLabelBlock) cluster_index[i] = (uint32_t)scan[labels[i]];
}

struct CLayout {
    uint32_t *parent, *is_rep;
    uint64_t *scan, *partials;
    size_t bytes;
};

// the one layout behind the size query (base = null) and the bind
inline CLayout layout(void *base, int64_t n) {
    Carver c(base);
    CLayout L;
    L.parent = c.take<uint32_t>((size_t)n);
    L.is_rep = c.take<uint32_t>((size_t)n);
    L.scan = c.take<uint64_t>((size_t)n + 1);
    L.partials = c.take<uint64_t>((size_t)scan_tiles(n));
    L.bytes = c.total();
    return L;
}

inline bool cluster_args_ok(uint64_t num_seqs, uint32_t sketch_size) {
    return sketch_size_ok(sketch_size) && num_seqs <= KMC_SPARSE_MAX_SEQS;
}

DeviceCache c_ws;  // library-owned workspace

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" double kmc_mash_jaccard_of_distance(double max_dist, int k) {
    if (!(max_dist >= 0.0 && max_dist <= 1.0) || !canon_k_ok(k)) return std::numeric_limits<double>::quiet_NaN();
    const double e = std::exp(-(double)k * max_dist);
    return e / (2.0 - e);
}

extern "C" size_t kmc_sketch_cluster_workspace_size(uint64_t num_seqs, int device) {
    if (num_seqs == 0 || num_seqs > KMC_SPARSE_MAX_SEQS || device < 0) return 0;
    return layout(nullptr, (int64_t)num_seqs).bytes;
}

extern "C" int kmc_sketch_cluster(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                                  uint32_t sketch_size, double min_jaccard, uint32_t *labels, uint32_t *cluster_index,
                                  uint32_t *num_clusters, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!cluster_args_ok(num_seqs, sketch_size)) return KMC_ERR_INVALID_ARG;
    if (!min_jaccard_ok(min_jaccard)) return KMC_ERR_INVALID_ARG;
    if (!labels) return KMC_ERR_INVALID_ARG;
    if (num_seqs == 0) return num_clusters ? (int)hipMemsetAsync(num_clusters, 0, sizeof(uint32_t), stream) : KMC_OK;
    if (!sketches || !sketch_sizes) return KMC_ERR_INVALID_ARG;
    int device = 0;
    if (hipError_t he = hipGetDevice(&device)) return (int)he;
    const int64_t n = (int64_t)num_seqs;
    CLayout L;
    if (int e = bind_layout(c_ws, device, workspace, workspace_bytes, 8, [&](void *b) { return layout(b, n); }, &L))
        return e;
    const int64_t blocks = ceil_div(n, kLabelBlock);
    const unsigned grid = (unsigned)(blocks < kMaxGridX ? blocks : kMaxGridX);
    hipLaunchKernelGGL(cluster_init_kernel, dim3(grid), dim3(kLabelBlock), 0, stream, L.parent, n);
    if (n > 1) {
        Tiling p;
        const bool stage = triangle_tiling(p, sketches, sketch_sizes, n, sketch_size);
        launch_tiles<Triangle>(p, stage, LinkUnion{L.parent, min_jaccard}, stream);
    }
    const bool rank = cluster_index || num_clusters;
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(grid), dim3(kLabelBlock), 0, stream, L.parent, n, labels,
                       rank ? L.is_rep : nullptr);
    if (rank) {
        excl_scan_u32(L.is_rep, n, L.partials, L.scan, stream);
        hipLaunchKernelGGL(cluster_rank_kernel, dim3(cluster_index ? grid : 1u), dim3(kLabelBlock), 0, stream, labels,
                           L.scan, n, cluster_index, num_clusters);
    }
    return (int)hipGetLastError();
}
