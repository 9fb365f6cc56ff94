// kmc_sketch_walk.h — the geometry of the sketch path's walks over the record buffer,
// shared by the direct sketcher (kmc_sketch_seq.hip), the screen
// (kmc_sketch_screen.hip) and the abundance accumulator (kmc_sketch_accum.hip): the
// workgroup shape, the number of ranges of a call, the walk's view for
// kmc_canon_walk.h, the offsets read as they are clamped and the hash a window
// stores.  One definition each, so that all walk the same bytes with the same launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc_internal.h"

namespace kmc {
namespace {

// shipped / under -DKMC_DIAG_HOOKS (libkmc_diag.so: a few thousand bases pass through
// many ranges)
//   kBlock      threads of a workgroup                     1024 / 64
//   kMinChunks  16-byte chunks per range, at least         1024 / 16  (16 KB / 256 B)
//   kWgPerCu    ranges per CU at most                      1 / 2
#ifdef KMC_DIAG_HOOKS
constexpr int kBlock = 64;
constexpr int64_t kMinChunks = 16;
constexpr int kWgPerCu = 2;
#else
constexpr int kBlock = 1024;
constexpr int64_t kMinChunks = 1024;
constexpr int kWgPerCu = 1;
#endif
constexpr uint64_t kMaxSeqs = 1ull << 40;

// The walk's view (kmc_canon_walk.h) with the geometry of a call; Idx: what idx[r]
// reads the offset of record r from
template <class Idx>
struct WalkOf {
    const char *data;
    Idx idx;
    int64_t n, lo, hi;
    int k;
    uint32_t flags;
    int64_t c_lo, cpw;
};

// record offsets as kmc_sketch_from_sequences' prep writes them, computed as they are
// read: clamp(indices[r], 0, data_bytes) + (data & 15); the walks that keep no
// per-record state (the screen, the abundance accumulator) need no workspace for them
struct Offsets {
    const int64_t *p;
    int64_t bytes, mis;
    __device__ __forceinline__ int64_t operator[](int64_t r) const {
        const int64_t x = p[r];
        return (x < 0 ? 0 : (x > bytes ? bytes : x)) + mis;
    }
};

// the view of a call over all n records of `idx`, cut into G ranges
template <class Idx>
__device__ __forceinline__ WalkOf<Idx> walk_of(const char *data, const Idx &idx, int64_t n, int k, uint32_t flags, int G) {
    WalkOf<Idx> W;
    W.data = data;
    W.idx = idx;
    W.n = n;
    W.lo = idx[0];
    W.hi = idx[n];
    if (W.hi < W.lo) W.hi = W.lo;
    W.k = k;
    W.flags = flags;
    W.c_lo = W.lo >> 4;
    const int64_t chunks = W.hi > W.lo ? ((W.hi + 15) >> 4) - W.c_lo : 0;
    const int64_t cpw = (chunks + G - 1) / G;
    W.cpw = cpw > 1 ? cpw : 1;
    return W;
}

struct HashOf {
    uint64_t seed;
    __device__ __forceinline__ unsigned long long operator()(uint64_t key) const { return sketch_hash(key, seed); }
};

// walking workgroups: one range of at least kMinChunks chunks each over the chunks
// data_bytes can hold (for any alignment of `data`), kWgPerCu per CU at most
inline int walk_groups(uint64_t data_bytes, int cus) {
    const uint64_t chunks = data_bytes / 16 + 3;
    const uint64_t cap = (uint64_t)kWgPerCu * (uint64_t)(cus > 0 ? cus : 1);
    uint64_t g = (chunks + kMinChunks - 1) / kMinChunks;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace
}  // namespace kmc
