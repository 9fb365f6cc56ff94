// kmc_sketch_seq.hip — bottom-s MinHash sketches straight from the record buffer.
// kmc_sketch_from_sequences writes, per record, the rows and sizes
// kmc_sketch_from_counts writes for the lists of kmc_count_canonical_hash, without
// those lists; kmc_sketch_from_sequences_grouped writes one row per group of
// consecutive records, the bottom-s of the union of their windows' hashes.  Both are
// one code path over units, a compile-time policy of the kernels (Records, Groups
// below): a unit is a record or a group, and a record is a group of one.  The bases
// are walked once (kmc_canon_walk.h, the canonical counter's walk), every valid
// window's key is hashed (sketch_hash) and a workgroup keeps the s smallest distinct
// hashes of the unit it is in as a sorted set in LDS.  Exact for any content: there
// is no table, no capacity and no retry.  Asynchronous, no host read-back; the
// launches depend on the host arguments only.
//
// Where a unit's set goes follows from one rule, its span: a byte interval taken from
// the offsets alone, clipped to the walked bytes [lo, hi), that holds every window
// start of the unit.  A span inside one range of the walk is that range's workgroup's
// to write to row u.  A span over the ranges w0 < .. < w1 leaves partial sets in slot
// 2 w0 + 1 and the slots 2w, w0 < w <= w1, of `part` (sizes in `psize`), and the
// workgroup of cut w0 folds them and always writes the row.
//   Records  unit u is record u, of n.  Span: the record's window starts,
//            [widx[u], widx[u] + nw), nw = max(widx[u + 1] - widx[u] - k, 0).  Exact:
//            non-empty iff the record has a window, so a record whose last k - 1
//            bytes alone cross a cut is one range's.  No offsets array.
//   Groups   unit g is the records [gofs[g], gofs[g + 1]), of ng (gofs: group_offsets
//            clamped to [0, n]; a descending pair is an empty group).  Span:
//            [widx[gofs[g]], widx[gofs[g + 1]]).  Conservative: a non-empty span may
//            hold no window, and telling so would cost a scan of the group's records.
//
//   prep    widx[r] = clamp(indices[r], 0, data_bytes) + (data & 15) (Offsets of
//           kmc_sketch_walk.h): the offsets over the 16-byte aligned buffer, as the
//           canonical counter's host does; gofs for Groups
//   fill    size 0 and a row of UINT64_MAX for every unit that neither the cut merge
//           (a span over a cut) nor the walk (an exact, non-empty span) is certain to
//           write: the records of no window; every group inside one range, of which
//           the walk overwrites those it meets a window of.  256 threads per unit, no
//           LDS.  A record with a window is never filled: no row is written twice.
//   walk    G workgroups; workgroup w walks cpw = ceil(chunks / G) 16-byte chunks of
//           the units' records (both ends read on the device), record piece by piece
//           (walk_piece, a body of for_each_chunk of kmc_sketch_walk.h, the chunk loop
//           of all three walks).  A valid window with hash h is a
//           candidate iff the set is not full or h < T (T: the set's largest value
//           once it holds s), and h is not in the set (a binary search, so a repeated
//           key is staged once per merge at most and low-complexity input costs
//           searches, not merges).  Candidates are appended to a staging buffer of
//           kStage values through an LDS counter; when it is full it is sorted
//           (bitonic_sort of kmc_sketch_pair.h) and merged into the set: every staged value not equal to its
//           predecessor nor in the set is kept, set values move up by the kept values
//           below them, kept values land behind the set values below them, positions
//           >= s fall off.  Lanes whose candidates did not fit filter them against the
//           new T and append again.  After N random windows about s / N of the windows
//           are candidates, so merges become rare and the walk's VALU work bounds the
//           kernel.  The set, T and the staged candidates live as long as the unit:
//           they are carried from one record piece to the next and written out and
//           reset (flush) when the piece's record belongs to another unit, and at the
//           end of the range: to row u if the span lies inside this range, else to
//           slot 2w (the span starts before this range) or 2w + 1 (it starts here).
//   merge   one workgroup per cut between two ranges (G - 1): spans are disjoint, so
//           at most one contains the cut, the last unit that starts before it.  If
//           its span crosses the cut and starts in the range before it (a span over
//           several cuts belongs to the first) its slots are folded with the same
//           merge, kStage values at a time, and the row, its tail and its size written.
//
// What holds for both kinds of unit:
// - Every slot read was written or zeroed by this call's walk: each walking workgroup
//   first zeroes its two psize words (those that return early included, by the thread
//   that may write them later: program order), a flush then writes the slot and its
//   size, and the merge reads psize[slot] values of a slot.  So the slot of a range
//   that holds no window of the crossing group (a stretch of records shorter than k,
//   longer than a range) reads as an empty set, nothing in the workspace is
//   accumulated into, and nothing a former call left there is read.
// - The zeroing costs Records nothing but the two stores: a crossing record has a
//   window in every range from w0 to w1, so each of its slots is written by a flush
//   after it was zeroed.
// - Offsets that do not ascend give unspecified rows, but every search result, row,
//   slot and range index is clamped to the launch, so nothing strays.
// - The record number and the unit's state (u, its end, m, T, the staged count) are
//   wave-uniform (uniform64): the unit search and the span are scalar loads and SGPRs.
//
// Constants, shipped / under -DKMC_DIAG_HOOKS (libkmc_diag.so: a few thousand bases
// pass through many ranges, merges and partial sets; no new symbol; the first, third
// and fourth are the walk geometry of kmc_sketch_walk.h, shared with the screen):
//   kBlock      threads of a workgroup                     1024 / 64
//   kStage      staged candidates per merge (= kBlock)     1024 / 64
//   kMinChunks  16-byte chunks per range, at least         1024 / 16  (16 KB / 256 B)
//   kWgPerCu    ranges per CU at most                      1 / 2
// LDS: 8 s' + 12 kStage bytes and a few words; s' = 1024 / 4096 / 16384 for
// s <= 1024 / 4096 / 16384: 20 / 44 / 140 KB shipped.
// Workspace: 8 (n + 1) B of offsets + G (8 + 16 s) B of partial sets,
// G = min(kWgPerCu * CUs, ceil((data_bytes / 16 + 3) / kMinChunks)); Groups:
// + 8 (ng + 1) B of group offsets.
//
// kmc_sketch_merge_groups: one workgroup per group folds the group's input rows, in
// order, into the LDS set with the same merge, kStage values at a time, and leaves a
// row at its first staged run that starts at or above T.  No workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc.h"
#include "kmc_canon_walk.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_walk.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

// (kBlock, kMinChunks, kWgPerCu, kMaxSeqs: kmc_sketch_walk.h)
constexpr int kStage = kBlock;
constexpr int kWaves = kBlock / 64;

struct Args {
    WalkArgs w;     // (w.idx: the caller's offsets, read by prep only)
    int64_t *widx;  // [n + 1] offsets over w.data
    uint32_t s;
    uint64_t seed;
    uint64_t *part;   // [2 G][s]
    uint32_t *psize;  // [2 G]
    uint64_t *sketches;  // one row per unit
    uint32_t *sizes;
    // Groups (Records: null, null, -1)
    const int64_t *group_offsets;  // the caller's
    int64_t *gofs;                 // [ng + 1] clamped to [0, n]
    int64_t ng;
};

struct MArgs {  // kmc_sketch_merge_groups
    const uint64_t *in;
    const uint32_t *sizes_in;
    int64_t rows;
    const int64_t *group_offsets;
    int64_t ng;
    uint32_t s;
    uint64_t *out;
    uint32_t *sizes_out;
};

// What a unit is (the header comment has the two span rules).  Each policy gives
//   count       the units of the call
//   records     the records [r0, r1) the units cover: what is walked
//   start       the byte unit u starts at (ascending in u)
//   bytes       the span of unit u, unclipped; empty: ge <= gs
//   kExactSpan  a non-empty span holds a window
//   unit_of     the unit of record R, at or after unit `from`; end: its records end
struct Records {
    static constexpr bool kExactSpan = true;
    static __device__ __forceinline__ int64_t count(const Args &a) { return a.w.n; }
    static __device__ __forceinline__ void records(const Args &a, int64_t &r0, int64_t &r1) {
        r0 = 0;
        r1 = a.w.n;
    }
    static __device__ __forceinline__ int64_t start(const Args &a, int64_t u) { return a.widx[u]; }
    static __device__ __forceinline__ void bytes(const Args &a, int64_t u, int64_t &gs, int64_t &ge) {
        const int64_t ra = a.widx[u], re = a.widx[u + 1];
        gs = ra;
        ge = ra + (re - ra - a.w.k > 0 ? re - ra - a.w.k : 0);
    }
    static __device__ __forceinline__ int64_t unit_of(const Args &, int64_t R, int64_t) { return R; }
    static __device__ __forceinline__ int64_t end(const Args &, int64_t u) { return u + 1; }
};

struct Groups {
    static constexpr bool kExactSpan = false;
    static __device__ __forceinline__ int64_t count(const Args &a) { return a.ng; }
    static __device__ __forceinline__ void records(const Args &a, int64_t &r0, int64_t &r1) {
        r0 = a.gofs[0];
        r1 = a.gofs[a.ng];
        if (r1 < r0) r1 = r0;
    }
    static __device__ __forceinline__ int64_t start(const Args &a, int64_t u) { return a.widx[a.gofs[u]]; }
    static __device__ __forceinline__ void bytes(const Args &a, int64_t u, int64_t &gs, int64_t &ge) {
        const int64_t ga = a.gofs[u], gb = a.gofs[u + 1];
        gs = a.widx[ga];
        ge = gb > ga ? a.widx[gb] : gs;
    }
    // the last group that starts at or before R (groups ascend: from `from` on)
    static __device__ __forceinline__ int64_t unit_of(const Args &a, int64_t R, int64_t from) {
        int64_t lo = from, hi = a.ng - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.gofs[mid] <= R) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
    static __device__ __forceinline__ int64_t end(const Args &a, int64_t u) { return a.gofs[u + 1]; }
};

// The walk's view (kmc_canon_walk.h) with the geometry of this call, over the offsets prep wrote
using Walk = WalkOf<const int64_t *>;

// over the records of the call's units
template <class Units>
__device__ __forceinline__ Walk make_walk(const Args &a) {
    int64_t r0, r1;
    Units::records(a, r0, r1);
    return walk_of<const int64_t *>(a.w.data, a.widx + r0, r1 - r0, a.w.k, a.w.flags, a.w.G);
}

// The span of unit u clipped to the walked bytes; empty: ge <= gs.
struct Span {
    int64_t gs, ge;
    __device__ __forceinline__ bool any() const { return ge > gs; }
};

template <class Units>
__device__ __forceinline__ Span unit_span(const Walk &W, const Args &a, int64_t u) {
    Span S;
    Units::bytes(a, u, S.gs, S.ge);
    S.gs = S.gs > W.lo ? S.gs : W.lo;
    S.ge = S.ge < W.hi ? S.ge : W.hi;
    return S;
}

// The ranges w0 <= w1 that hold the first and the last byte of a non-empty span.  The
// walking workgroup w decides the same without a division: w0 == w iff gs is at or
// past its range's first byte, w1 == w iff ge is at or before its end.
__device__ __forceinline__ void span_ranges(const Walk &W, int G, const Span &S, int64_t &w0, int64_t &w1) {
    const int64_t top = G - 1;
    w0 = ((S.gs >> 4) - W.c_lo) / W.cpw;
    w1 = (((S.ge - 1) >> 4) - W.c_lo) / W.cpw;
    // (guard) the slots of this launch only
    w0 = w0 < 0 ? 0 : (w0 > top ? top : w0);
    w1 = w1 < w0 ? w0 : (w1 > top ? top : w1);
}

// ng < 0: no groups
__global__ __launch_bounds__(256) void sketch_prep_kernel(Args a) {
    const int64_t top = a.w.n > a.ng ? a.w.n : a.ng;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= top; i += (int64_t)gridDim.x * 256) {
        if (i <= a.w.n) a.widx[i] = a.w.idx[i];
        if (i <= a.ng) {
            const int64_t x = a.group_offsets[i];
            a.gofs[i] = x < 0 ? 0 : (x > a.w.n ? a.w.n : x);
        }
    }
}

template <int CAP>
struct SetLds {
    uint64_t set[CAP];        // ascending, distinct; the first m are valid
    uint64_t stage[kStage];
    uint32_t kp[kStage + 1];  // kept staged values before each staged value; [c]: all of them
    uint32_t wsum[kWaves];
    uint32_t ctr[3];          // staged counts of the walk's rounds, in rotation
    int64_t first;
};
static_assert(sizeof(SetLds<KMC_SKETCH_MAX_SIZE>) <= 160 * 1024, "the set and its staging buffer fit the CU's LDS");

// (lower_bound and bitonic_sort: kmc_sketch_pair.h)
__device__ __forceinline__ bool in_set(const uint64_t *set, int m, uint64_t v) {
    const int i = lower_bound(set, m, v);
    return i < m && set[i] == v;
}

// Merges stage[0, c) (any order, repeats allowed, written before the caller's last
// barrier) into set[0, m): returns the new m = min(s, distinct values of both).
// Every thread of the workgroup calls it with the same arguments.
template <int CAP>
__device__ __forceinline__ int merge_stage(SetLds<CAP> &L, int m, int s, int c) {
    constexpr int R = CAP / kBlock < 1 ? 1 : (CAP / kBlock > 4 ? 4 : CAP / kBlock);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = pow2_at_least(c);  // <= kStage = kBlock
    if (tid >= c && tid < P) L.stage[tid] = kFill;
    lds_barrier();
    // LDS-only barriers: a __syncthreads() would wait for the walk's chunk prefetch
    bitonic_sort<kBlock, true>(L.stage, 1, P, tid, [] { lds_barrier(); });
    // staged value tid: kept unless it repeats its predecessor or is in the set
    uint64_t v = 0;
    int lb = 0;
    bool keep = false;
    if (tid < c) {
        v = L.stage[tid];
        lb = lower_bound(L.set, m, v);
        keep = !(tid > 0 && L.stage[tid - 1] == v) && !(lb < m && L.set[lb] == v);
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) L.wsum[wave] = (uint32_t)__popcll(bal);
    lds_barrier();
    uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
        const uint32_t t = L.wsum[q];
        if (q < wave) before += t;
        kept += t;
    }
    if (kept == 0) {
        lds_barrier();  // wsum is free again
        return m;
    }
    if (tid < c) L.kp[tid] = before;
    if (tid == 0) L.kp[c] = kept;
    lds_barrier();
    // set values move up by the kept values below them: from the top down in runs of
    // R * kBlock, read then written, so that no value is overwritten before it is read
    for (int hi = m; hi > 0; hi -= R * kBlock) {
        const int lo = hi - R * kBlock > 0 ? hi - R * kBlock : 0;
        uint64_t x[R];
        int np[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int i = lo + t * kBlock + tid;
            np[t] = -1;
            x[t] = 0;
            if (i < hi) {
                x[t] = L.set[i];
                const int up = (int)L.kp[lower_bound(L.stage, c, x[t])];
                if (up > 0 && i + up < s) np[t] = i + up;
            }
        }
        lds_barrier();
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (np[t] >= 0) L.set[np[t]] = x[t];
        lds_barrier();
    }
    if (keep && lb + (int)before < s) L.set[lb + (int)before] = v;
    lds_barrier();
    const int total = m + (int)kept;
    return total < s ? total : s;
}

// a wave-uniform 64-bit value as the compiler can see it (scalar registers and loads)
__device__ __forceinline__ int64_t uniform64(int64_t x) {
    const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)h << 32) | l);
}

// The set as a row: its m values, the tail of UINT64_MAX and the size.
template <int CAP>
__device__ __forceinline__ void write_row(const SetLds<CAP> &L, uint64_t *row, uint32_t *size, int m, int s) {
    for (int i = threadIdx.x; i < s; i += kBlock) row[i] = i < m ? L.set[i] : kFill;
    if (threadIdx.x == 0) *size = (uint32_t)m;
}

// The set as a partial set: its m values and the size.
template <int CAP>
__device__ __forceinline__ void write_part(const SetLds<CAP> &L, uint64_t *dst, uint32_t *size, int m) {
    for (int i = threadIdx.x; i < m; i += kBlock) dst[i] = L.set[i];
    if (threadIdx.x == 0) *size = (uint32_t)m;
}

// Folds the first min(pm, s) values of the ascending row `src` into the set, kStage
// at a time, up to the first run that starts at or above T.
template <int CAP>
__device__ __forceinline__ void fold_row(SetLds<CAP> &L, const uint64_t *src, uint32_t pm, int s, int &m, uint64_t &T) {
    const int tid = threadIdx.x;
    if (pm > (uint32_t)s) pm = (uint32_t)s;
    for (int c0 = 0; c0 < (int)pm; c0 += kStage) {
        if (m == s && src[c0] >= T) break;  // ascending: nothing below T is left
        const int c = (int)pm - c0 < kStage ? (int)pm - c0 : kStage;
        if (tid < c) L.stage[tid] = src[c0 + tid];
        lds_barrier();
        m = merge_stage(L, m, s, c);
        T = m == s ? L.set[s - 1] : kFill;
    }
}

// The windows of record piece [ps, pe): every candidate hash goes through the staging
// buffer into the set (m values, threshold T, `staged` values left in the buffer,
// ci: the counter of the next round).  Every thread of the workgroup calls it.
template <bool FWD, bool BIGK, int CAP>
__device__ __forceinline__ void walk_piece(SetLds<CAP> &L, const Walk &W, const HashOf hf, int64_t ps, int64_t pe,
                                           int64_t rend, int s, int &m, uint32_t &staged, uint64_t &T, int &ci) {
    const int tid = threadIdx.x;
    // (entered by every thread in every round, pend == 0 included: the barriers below)
    for_each_chunk<FWD, BIGK>(W, ps, pe, rend, hf, [&](const unsigned long long(&h)[16], uint32_t pend) {
        for (;;) {
            const bool full = m == s;
            uint32_t cm = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) cm |= (uint32_t)(!full || h[j] < T) << j;
            pend &= cm;
            if (pend) {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (((pend >> j) & 1u) && in_set(L.set, m, h[j])) pend &= ~(1u << j);
            }
            const uint32_t cnt = (uint32_t)__popc(pend);
            if (cnt) {
                uint32_t at = staged + __hip_atomic_fetch_add(&L.ctr[ci], cnt, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if ((pend >> j) & 1u) {
                        if (at < (uint32_t)kStage) {
                            L.stage[at] = h[j];
                            pend &= ~(1u << j);
                        }
                        ++at;
                    }
                }
            }
            lds_barrier();
            const uint32_t total = staged + L.ctr[ci];
            // the counter of the round before: every thread has read it (it passed this
            // barrier), and its next adds come after the next barrier
            if (tid == 0) L.ctr[(ci + 2) % 3] = 0u;
            ci = (ci + 1) % 3;
            if (total < (uint32_t)kStage) {
                staged = total;
                break;
            }
            m = merge_stage(L, m, s, kStage);
            T = m == s ? L.set[s - 1] : kFill;
            staged = 0;
            if (total == (uint32_t)kStage) break;  // (else some lanes still hold candidates)
        }
    });
}

// Size 0 and a row of UINT64_MAX, before the walk, for every unit whose row neither
// the cut merge nor the walk is certain to write (no LDS).
template <class Units>
__global__ __launch_bounds__(256) void sketch_fill_kernel(Args a) {
    const Walk W = make_walk<Units>(a);
    const int s = (int)a.s;
    for (int64_t u = blockIdx.x; u < Units::count(a); u += gridDim.x) {
        const Span S = unit_span<Units>(W, a, u);
        if (S.any()) {
            if (Units::kExactSpan) continue;  // the walk meets a window of it
            int64_t w0, w1;
            span_ranges(W, a.w.G, S, w0, w1);
            if (w1 > w0) continue;  // the cut merge's
        }
        uint64_t *row = a.sketches + u * (int64_t)s;
        for (int i = threadIdx.x; i < s; i += 256) row[i] = kFill;
        if (threadIdx.x == 0) a.sizes[u] = 0u;
    }
}

// The set, its threshold and the staged candidates outlive the record piece; they are
// written out (flush) and reset when the piece's record belongs to another unit than
// the one before, and at the end of the range.
template <class Units, bool FWD, bool BIGK, int CAP>
__global__ __launch_bounds__(kBlock) void sketch_walk_kernel(Args a) {
    __shared__ SetLds<CAP> L;
    const Walk W = make_walk<Units>(a);
    const int tid = threadIdx.x, s = (int)a.s, w = blockIdx.x;
    const HashOf hf{a.seed};
    const int64_t b0 = (W.c_lo + (int64_t)w * W.cpw) << 4, b1 = b0 + (W.cpw << 4);  // this range's bytes
    // a slot of this range that no flush writes reads as empty (zeroed by the thread
    // that may write it later: program order)
    if (tid == 0) a.psize[2 * w] = a.psize[2 * w + 1] = 0u;
    if (tid < 3) L.ctr[tid] = 0u;
    int ci = 0;  // the counter of the next round (the one after it is zero already)
    int m = 0;
    uint32_t staged = 0;  // values in the staging buffer (workgroup-uniform)
    uint64_t T = kFill;
    int64_t u = -1, u_end = 0;  // (wave-uniform) the records below u_end are unit u's
    const auto flush = [&]() {
        if (staged) m = merge_stage(L, m, s, (int)staged);
        const Span S = unit_span<Units>(W, a, u);
        const bool first = S.gs >= b0;  // the span starts in this range
        if (first && S.ge <= b1) {      // and ends in it, the whole unit: its row
            write_row(L, a.sketches + u * (int64_t)s, a.sizes + u, m, s);
        } else {
            const int64_t slot = 2 * (int64_t)w + (first ? 1 : 0);
            write_part(L, a.part + slot * (int64_t)s, a.psize + slot, m);
        }
        lds_barrier();  // the set is read out before the next unit's merges
        m = 0;
        staged = 0;
        T = kFill;
    };
    __syncthreads();
    for_each_piece(W, &L.first, [&](int64_t r, int64_t ps, int64_t pe, int64_t rend) {
        const int64_t R = uniform64(r + (W.idx - a.widx));  // the record in the call's numbering
        if (R >= u_end) {
            if (u >= 0) flush();
            u = Units::unit_of(a, R, u < 0 ? 0 : u);
            u_end = Units::end(a, u);
            if (u_end <= R) u_end = R + 1;  // (guard: offsets that do not ascend)
        }
        walk_piece<FWD, BIGK>(L, W, hf, ps, pe, rend, s, m, staged, T, ci);
    });
    if (u >= 0) flush();
}

// One workgroup per cut between two ranges (G - 1 of them): the last unit that starts
// before cut b, if its span crosses the cut and b is the first cut it crosses, has its
// partial sets folded and its row written (a slot no window went to has size 0).
template <class Units, int CAP>
__global__ __launch_bounds__(kBlock) void sketch_cut_merge_kernel(Args a) {
    __shared__ SetLds<CAP> L;
    const Walk W = make_walk<Units>(a);
    const int s = (int)a.s;
    const int64_t b = blockIdx.x;
    const int64_t cut = (W.c_lo + (b + 1) * W.cpw) << 4;  // first byte of range b + 1
    if (cut <= W.lo || cut >= W.hi) return;
    int64_t lo = 0, hi = Units::count(a) - 1;  // (wave-uniform: scalar loads)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (Units::start(a, mid) < cut) lo = mid; else hi = mid - 1;
    }
    const int64_t u = lo;
    const Span S = unit_span<Units>(W, a, u);
    if (S.gs >= cut || S.ge <= cut) return;  // nothing before the cut, or nothing from it on
    int64_t w0, w1;
    span_ranges(W, a.w.G, S, w0, w1);
    if (w0 != b) return;  // an earlier cut's workgroup has the unit
    int m = 0;
    uint64_t T = kFill;
    for (int64_t w = w0; w <= w1; ++w) {
        const int64_t slot = 2 * w + (w == w0 ? 1 : 0);
        fold_row(L, a.part + slot * (int64_t)s, a.psize[slot], s, m, T);
    }
    write_row(L, a.sketches + u * (int64_t)s, a.sizes + u, m, s);
}

// kmc_sketch_merge_groups: a workgroup folds the rows of its groups, one group at a time.
template <int CAP>
__global__ __launch_bounds__(kBlock) void sketch_merge_groups_kernel(MArgs a) {
    __shared__ SetLds<CAP> L;
    const int s = (int)a.s;
    for (int64_t g = blockIdx.x; g < a.ng; g += gridDim.x) {
        int64_t ra = a.group_offsets[g], rb = a.group_offsets[g + 1];
        ra = ra < 0 ? 0 : (ra > a.rows ? a.rows : ra);
        rb = rb < 0 ? 0 : (rb > a.rows ? a.rows : rb);
        int m = 0;
        uint64_t T = kFill;
        for (int64_t r = ra; r < rb; ++r) fold_row(L, a.in + r * (int64_t)s, a.sizes_in[r], s, m, T);
        write_row(L, a.out + g * (int64_t)s, a.sizes_out + g, m, s);
        lds_barrier();  // the set is read out before the next group's merges
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct SLayout {
    int64_t *widx;
    uint32_t *psize;
    uint64_t *part;
    int64_t *gofs;  // the grouped call's only
    size_t bytes;
};

// (walk_groups, the walking workgroups of a call: kmc_sketch_walk.h)
// the one layout behind the size queries (base = null) and the binds; ng < 0: no groups
inline SLayout layout(void *base, int64_t n, int G, uint32_t s, int64_t ng = -1) {
    Carver c(base);
    SLayout L;
    L.widx = c.take<int64_t>((size_t)n + 1);
    L.psize = c.take<uint32_t>(2 * (size_t)G);
    L.part = c.take<uint64_t>(2 * (size_t)G * s);
    L.gofs = c.take_if<int64_t>(ng >= 0, (size_t)(ng < 0 ? 0 : ng) + 1);
    L.bytes = c.total();
    return L;
}

inline bool seq_args_ok(uint64_t num_seqs, uint64_t data_bytes, uint32_t sketch_size) {
    return sketch_size_ok(sketch_size) && walk_sizes_ok(num_seqs, data_bytes);
}

// what both entry points refuse before anything else: k, then every other argument
inline int seq_check(int k, uint64_t num_seqs, uint64_t data_bytes, uint32_t sketch_size, unsigned flags) {
    if (int e = walk_check(k, num_seqs, data_bytes, flags)) return e;
    return sketch_size_ok(sketch_size) ? KMC_OK : KMC_ERR_INVALID_ARG;
}

DeviceCache q_ws;  // library-owned workspace

// Both entry points after their argument checks: the workspace of the call (Records:
// group_offsets null, ng = -1) and the launches.
template <class Units>
int sketch_units(const char *data, const int64_t *indices, uint64_t num_seqs, uint64_t data_bytes,
                 const int64_t *group_offsets, int64_t ng, int k, unsigned flags, uint32_t sketch_size, uint64_t seed,
                 uint64_t *sketches, uint32_t *sketch_sizes, void *workspace, size_t workspace_bytes, hipStream_t st) {
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const int64_t n = (int64_t)num_seqs;
    Args a;
    a.w = walk_args(data, indices, num_seqs, data_bytes, k, flags, cus);  // (the offsets' rule: applied by prep)
    const int G = a.w.G;
    SLayout L;
    if (int e = bind_layout(q_ws, device, workspace, workspace_bytes, 8,
                            [&](void *b) { return layout(b, n, G, sketch_size, ng); }, &L))
        return e;
    a.widx = L.widx;
    a.s = sketch_size;
    a.seed = seed;
    a.part = L.part;
    a.psize = L.psize;
    a.sketches = sketches;
    a.sizes = sketch_sizes;
    a.group_offsets = group_offsets;
    a.gofs = L.gofs;
    a.ng = ng;
    const int64_t top = n > ng ? n : ng, pg = (top + 1 + 255) / 256, units = ng < 0 ? n : ng;
    hipLaunchKernelGGL(sketch_prep_kernel, dim3((unsigned)(pg < 4096 ? pg : 4096)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sketch_fill_kernel<Units>, dim3((unsigned)(units < kMaxGridX ? units : kMaxGridX)), dim3(256), 0,
                       st, a);
    for_cap(sketch_size, [&](auto cap) {
        constexpr int CAP = decltype(cap)::value;
        const dim3 g((unsigned)G), b(kBlock);
        for_walk(flags, k, [&](auto fwd, auto big) {
            hipLaunchKernelGGL((sketch_walk_kernel<Units, decltype(fwd)::value, decltype(big)::value, CAP>), g, b, 0, st, a);
        });
        if (G > 1) hipLaunchKernelGGL((sketch_cut_merge_kernel<Units, CAP>), dim3((unsigned)G - 1), b, 0, st, a);
    });
    return (int)hipGetLastError();
}

// [p, p + bytes) and [q, q + qbytes) share a byte
inline bool overlap(const void *p, uint64_t bytes, const void *q, uint64_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + bytes;
}

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" size_t kmc_sketch_from_sequences_workspace_size(uint64_t num_seqs, uint64_t data_bytes, uint32_t sketch_size,
                                                           int device) {
    if (!seq_args_ok(num_seqs, data_bytes, sketch_size) || num_seqs == 0 || device < 0) return 0;
    int cus = 0;  // (the arguments are checked before any HIP call)
    if (device_cus(device, &cus)) return 0;
    return layout(nullptr, (int64_t)num_seqs, walk_groups(data_bytes, cus), sketch_size).bytes;
}

extern "C" int kmc_sketch_from_sequences(const char *data, const int64_t *indices, uint64_t num_seqs,
                                         uint64_t data_bytes, int k, unsigned flags, uint32_t sketch_size,
                                         uint64_t seed, uint64_t *sketches, uint32_t *sketch_sizes, void *workspace,
                                         size_t workspace_bytes, hipStream_t stream) {
    if (int e = seq_check(k, num_seqs, data_bytes, sketch_size, flags)) return e;
    if (num_seqs == 0) return KMC_OK;
    if (!walk_ptrs_ok(data, indices, data_bytes) || !sketches || !sketch_sizes) return KMC_ERR_INVALID_ARG;
    return sketch_units<Records>(data, indices, num_seqs, data_bytes, nullptr, -1, k, flags, sketch_size, seed,
                                 sketches, sketch_sizes, workspace, workspace_bytes, stream);
}

extern "C" size_t kmc_sketch_from_sequences_grouped_workspace_size(uint64_t num_seqs, uint64_t num_groups,
                                                                   uint64_t data_bytes, uint32_t sketch_size,
                                                                   int device) {
    if (!seq_args_ok(num_seqs, data_bytes, sketch_size) || num_seqs == 0 || num_groups == 0 ||
        num_groups > kMaxSeqs || device < 0)
        return 0;
    int cus = 0;  // (the arguments are checked before any HIP call)
    if (device_cus(device, &cus)) return 0;
    return layout(nullptr, (int64_t)num_seqs, walk_groups(data_bytes, cus), sketch_size, (int64_t)num_groups).bytes;
}

extern "C" int kmc_sketch_from_sequences_grouped(const char *data, const int64_t *indices, uint64_t num_seqs,
                                                 uint64_t data_bytes, const int64_t *group_offsets,
                                                 uint64_t num_groups, int k, unsigned flags, uint32_t sketch_size,
                                                 uint64_t seed, uint64_t *sketches, uint32_t *sketch_sizes,
                                                 void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (int e = seq_check(k, num_seqs, data_bytes, sketch_size, flags)) return e;
    if (num_groups > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (num_groups == 0) return KMC_OK;
    if (!group_offsets) return KMC_ERR_INVALID_ARG;
    if (num_seqs == 0) return KMC_OK;
    if (!walk_ptrs_ok(data, indices, data_bytes) || !sketches || !sketch_sizes) return KMC_ERR_INVALID_ARG;
    return sketch_units<Groups>(data, indices, num_seqs, data_bytes, group_offsets, (int64_t)num_groups, k, flags,
                                sketch_size, seed, sketches, sketch_sizes, workspace, workspace_bytes, stream);
}

extern "C" int kmc_sketch_merge_groups(const uint64_t *sketches_in, const uint32_t *sizes_in, uint64_t num_rows,
                                       const int64_t *group_offsets, uint64_t num_groups, uint32_t sketch_size,
                                       uint64_t *sketches_out, uint32_t *sizes_out, hipStream_t stream) {
    if (!sketch_size_ok(sketch_size) || num_rows > kMaxSeqs || num_groups > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (num_groups == 0) return KMC_OK;
    if (!group_offsets || !sketches_out || !sizes_out) return KMC_ERR_INVALID_ARG;
    if (num_rows > 0 && (!sketches_in || !sizes_in)) return KMC_ERR_INVALID_ARG;
    const uint64_t row = 8ull * sketch_size;
    if (num_rows > 0 && (overlap(sketches_out, num_groups * row, sketches_in, num_rows * row) ||
                         overlap(sizes_out, num_groups * 4, sizes_in, num_rows * 4)))
        return KMC_ERR_INVALID_ARG;
    MArgs a;
    a.in = sketches_in;
    a.sizes_in = sizes_in;
    a.rows = (int64_t)num_rows;
    a.group_offsets = group_offsets;
    a.ng = (int64_t)num_groups;
    a.s = sketch_size;
    a.out = sketches_out;
    a.sizes_out = sizes_out;
    const dim3 g((unsigned)(a.ng < kMaxGridX ? a.ng : kMaxGridX)), b(kBlock);
    for_cap(sketch_size, [&](auto cap) {
        hipLaunchKernelGGL((sketch_merge_groups_kernel<decltype(cap)::value>), g, b, 0, stream, a);
    });
    return (int)hipGetLastError();
}
