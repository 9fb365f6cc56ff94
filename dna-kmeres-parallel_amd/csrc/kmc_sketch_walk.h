// kmc_sketch_walk.h — the sketch path's walks over the record buffer, shared by the
// direct sketcher (kmc_sketch_seq.hip), the screen (kmc_sketch_screen.hip) and the
// abundance accumulator (kmc_sketch_accum.hip).  One definition each, so that all walk
// the same bytes with the same launch and a fix reaches all three:
//   geometry   the workgroup shape, the number of ranges of a call, the walk's view for
//              kmc_canon_walk.h, the offsets read as they are clamped, the hash a
//              window stores
//   device     for_each_chunk, the chunk loop of a record piece with its prefetch, and
//              add_runs, one atomic add per run of equal values among a thread's windows
//              for_each_wave_piece and for_each_wave_chunk, the same two loops with a wave
//              as the unit that owns a record piece (the per-record match of the
//              abundance accumulator)
//   host       the arguments every walk takes (WalkArgs, walk_args), the checks of the
//              caller's input and for_walk, the dispatch on orientation and key width
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kmc.h"
#include "kmc_canon_walk.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"

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

// The chunk loop of record piece [ps, pe) (for_each_piece of kmc_canon_walk.h): a
// round is kBlock consecutive 16-byte chunks, one per thread, whose 48 bytes were
// loaded a round ahead (chunk_raw: the next round's loads are issued before this
// round's keys are made, so one chunk per thread stays in flight).  body(h, pend) gets
// out(key) of the chunk's 16 windows and the mask of those that exist, in EVERY thread
// in EVERY round, pend == 0 (past the piece) included: the trip count is the
// workgroup's, so a body may hold a barrier.  A body with nothing to do returns.
template <bool FWD, bool BIGK, class Idx, class Out, class Body>
__device__ __forceinline__ void for_each_chunk(const WalkOf<Idx> &W, int64_t ps, int64_t pe, int64_t rend, Out out,
                                               Body &&body) {
    const int tid = threadIdx.x;
    const int64_t c0 = ps >> 4, c1 = ((pe - 1) >> 4) + 1;
    ChunkRaw nx = chunk_raw(W, (c0 + tid) << 4);
    for (int64_t cb = c0; cb < c1; cb += kBlock) {
        const int64_t c = cb + tid;
        unsigned long long h[16];
        const ChunkRaw cr = nx;
        nx = chunk_raw(W, (c + kBlock) << 4);  // next round's chunk
        body(h, chunk_keys<FWD, BIGK>(W, cr, c << 4, ps, pe, rend, out, h));  // (past the piece: 0)
    }
}

// The windows of `pend` among a thread's 16, counted: equal neighbours are one run,
// find(value) says where the value's count is kept (null: nowhere), and a run is one
// relaxed agent-scope add of its length (a homopolymer run is one add of 16, not 16).
template <class Find>
__device__ __forceinline__ void add_runs(const unsigned long long (&v)[16], uint32_t pend, Find find) {
    unsigned long long last = 0;
    uint32_t *at = nullptr;
    uint32_t run = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!((pend >> j) & 1u)) continue;
        if (run && v[j] == last) {
            ++run;
            continue;
        }
        if (run && at) __hip_atomic_fetch_add(at, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = v[j];
        at = find(last);
        run = 1u;
    }
    if (run && at) __hip_atomic_fetch_add(at, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// the wave as the unit (the per-record walks: a piece of a 150-base read fills 10 of
// a wave's 64 lanes, not 10 of a workgroup's 1024)
// ---------------------------------------------------------------------------
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlock / kWave;  // the units of a workgroup: 16 / 1

// a 64-bit value of the wave's first lane, in every lane (and in scalar registers)
__device__ __forceinline__ int64_t wave_first(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)((uint64_t)lo | ((uint64_t)hi << 32));
}

// the sum of x over the wave's lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

// for_each_piece of kmc_canon_walk.h with the wave as the unit: the wave's chunk range
// and its record pieces, f(r, ps, pe, rend, whole); whole: the piece is all of the
// record's windows, so no other wave has a piece of r.  The first record is found by
// the wave's first lane and broadcast; r, ps, pe and rend are the same in every lane.
// No barrier and no LDS: the waves of a workgroup do not wait for each other.
template <class P, class F>
__device__ __forceinline__ void for_each_wave_piece(const P &p, F &&f) {
    const int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t cb = p.c_lo + u * p.cpw;
    const int64_t wlo = std::max<int64_t>(cb << 4, p.lo), whi = std::min<int64_t>((cb + p.cpw) << 4, p.hi);
    if (wlo >= whi) return;
    int64_t a = 0;
    if ((threadIdx.x & (kWave - 1)) == 0) {  // last record r with idx[r] <= wlo
        int64_t b = p.n - 1;
        while (a < b) {
            const int64_t m = (a + b + 1) >> 1;
            if (p.idx[m] <= wlo) a = m; else b = m - 1;
        }
    }
    for (int64_t r = wave_first(a); r < p.n; ++r) {
        const int64_t s = p.idx[r], e = p.idx[r + 1];
        if (s >= whi) break;
        const int64_t nw = e - s - p.k > 0 ? e - s - p.k : 0;
        const int64_t ps = std::max(s, wlo), pe = std::min(s + nw, whi);
        if (ps >= pe) continue;
        f(r, ps, pe, e, ps == s && pe == s + nw);
    }
}

// for_each_chunk with the wave as the unit: a round is kWave consecutive chunks, one
// per lane, loaded a round ahead; body(h, pend) in every lane in every round of the
// wave's own trip count.
template <bool FWD, bool BIGK, class Idx, class Out, class Body>
__device__ __forceinline__ void for_each_wave_chunk(const WalkOf<Idx> &W, int64_t ps, int64_t pe, int64_t rend, Out out,
                                                    Body &&body) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c0 = ps >> 4, c1 = ((pe - 1) >> 4) + 1;
    ChunkRaw nx = chunk_raw(W, (c0 + lane) << 4);
    for (int64_t cb = c0; cb < c1; cb += kWave) {
        const int64_t c = cb + lane;
        unsigned long long h[16];
        const ChunkRaw cr = nx;
        if (cb + kWave < c1) nx = chunk_raw(W, (c + kWave) << 4);  // next round's chunk (wave-uniform)
        body(h, chunk_keys<FWD, BIGK>(W, cr, c << 4, ps, pe, rend, out, h));  // (past the piece: 0)
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// walking workgroups: one range of at least kMinChunks chunks each over the chunks
// data_bytes can hold (for any alignment of `data`), kWgPerCu per CU at most
inline int walk_groups(uint64_t data_bytes, int cus) {
    const uint64_t chunks = data_bytes / 16 + 3;
    const uint64_t cap = (uint64_t)kWgPerCu * (uint64_t)(cus > 0 ? cus : 1);
    uint64_t g = (chunks + kMinChunks - 1) / kMinChunks;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

// What every walk's kernel takes of the caller's input.  Any `data` pointer: it is
// rounded down to 16 bytes and every offset moved up by the difference
// (kmc_count_canonical_hash's rule), as the offsets are read.
struct WalkArgs {
    const char *data;  // rounded down to 16 bytes
    Offsets idx;       // [n + 1]
    int64_t n;
    int k;
    uint32_t flags;
    int G;
};

inline WalkArgs walk_args(const char *data, const int64_t *indices, uint64_t num_seqs, uint64_t data_bytes, int k,
                          unsigned flags, int cus) {
    const uintptr_t mis = reinterpret_cast<uintptr_t>(data) & 15u;
    return WalkArgs{data - mis, Offsets{indices, (int64_t)data_bytes, (int64_t)mis}, (int64_t)num_seqs, k, flags,
                    walk_groups(data_bytes, cus)};
}

__device__ __forceinline__ WalkOf<Offsets> walk_of(const WalkArgs &a) {
    return walk_of(a.data, a.idx, a.n, a.k, a.flags, a.G);
}

// the same view cut into one range per WAVE of the G workgroups (for_each_wave_piece:
// W.cpw is a wave's chunks)
__device__ __forceinline__ WalkOf<Offsets> wave_walk_of(const WalkArgs &a) {
    return walk_of(a.data, a.idx, a.n, a.k, a.flags, a.G * kWavesPerBlock);
}

// The checks of a walk's input, one definition each; an entry point applies them in
// the order its contract states.
inline bool walk_sizes_ok(uint64_t num_seqs, uint64_t data_bytes) {
    return num_seqs <= kMaxSeqs && data_bytes < (1ull << 62);
}
inline bool walk_flags_ok(unsigned flags) { return !(flags & ~(KMC_CANON_SOFTMASK | KMC_CANON_FORWARD)); }
inline bool walk_ptrs_ok(const char *data, const int64_t *indices, uint64_t data_bytes) {
    return indices && (data_bytes == 0 || data);
}
// k, then the sizes, then the flags: what the sketcher and the screen refuse first
inline int walk_check(int k, uint64_t num_seqs, uint64_t data_bytes, unsigned flags) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    return walk_sizes_ok(num_seqs, data_bytes) && walk_flags_ok(flags) ? KMC_OK : KMC_ERR_INVALID_ARG;
}

// f(FWD, BIGK), the orientation and the key width of a call as std::bool_constants (for_cap's style)
template <class F>
inline void for_walk(unsigned flags, int k, F &&f) {
    const bool fwd = flags & KMC_CANON_FORWARD, big = k >= 16;
    if (fwd) {
        if (big) f(std::true_type{}, std::true_type{});
        else f(std::true_type{}, std::false_type{});
    } else {
        if (big) f(std::false_type{}, std::true_type{});
        else f(std::false_type{}, std::false_type{});
    }
}

}  // namespace
}  // namespace kmc
