// kmc_sketch.hip — bottom-s MinHash sketches of per-record key lists and the
// all-pairs Mash distance of such sketches: the distance path whose n x n step
// touches n * s values instead of every distinct k-mer of every record.
//
//     h(key)  = splitmix64_at(key ^ seed, 0)          (a bijection: distinct keys, distinct hashes)
//     sketch  = the min(s, entries) smallest h of a record, ascending, UINT64_MAX after them
//     d(i, j) = -log(2J / (1 + J)) / k,  J = shared / denom over the s smallest of the union
//
// Everything but the last float is integer-exact, for any content: the selection
// is a radix select, not a table with a capacity.
//
// kmc_sketch_from_counts, all on the caller's stream, no host read-back, launches
// fixed by the host arguments:
//   hist     G workgroups walk contiguous entry ranges (kmc_walk.h, the walk of
//            kmc_dist_sparse.hip) in chunks of kChunk entries; an entry that takes
//            part (count >= min_count) and whose hash agrees with the record's
//            prefix fixed so far adds one to the current digit's bin.  The
//            workgroup keeps an LDS histogram for one record, the one its range
//            opened with or the one the last chunk ended in, and flushes it to
//            hist[record][digit] (64-bit global atomics, non-zero bins only) when a
//            chunk ends in another record; entries of other records (the tail of
//            a short record, many tiny records in one chunk) go to hist directly.
//   decide   one 256-thread workgroup per record scans the 256 bins, finds the
//            digit at which the running count reaches the rank still needed,
//            extends the prefix, and zeroes the bins for the next level.  Level 0
//            also gives the number of participating entries, hence sketch_sizes;
//            a record with at most s of them skips the search (T = UINT64_MAX).
//   ... 64 / kDigitBits = 8 levels, most significant digit first; afterwards T_r is
//            the exact s-th smallest hash of record r
//   collect  the walk once more appends every participating h <= T_r to the row
//            through a per-record cursor (a global atomic per kept entry; the write
//            is skipped at or past sketch_sizes[r], which only a repeated key reaches)
//   sort     one workgroup per record: bitonic sort of the row in LDS (bitonic_sort of
//            kmc_sketch_pair.h), padded to a power of two with UINT64_MAX, then the
//            row with its tail fill
// Per entry and level 8 B are re-read (12 B with min_count > 1), 9 times in all.
// Digit width: 8 bits is the only width run so far (profiles/pr_sketch.jsonl); a wider
// digit needs fewer passes and a larger table (kDigitBits = 11: 6 levels, 16 KB per record).
//
// kmc_sketch_distances: the packed triangle is cut into T x T tiles of row
// pairs; a workgroup stages the 2T rows of a tile in LDS and its 16 wavefronts
// take the tile's pairs.  The kernel, its tile loop and the pair's counts are
// kmc_sketch_pair.h's, shared with the rectangle and the search of
// kmc_sketch_query.hip; the shape is Triangle of kmc_sketch_triangle.h (which tile,
// which pairs, where a result goes).  For a pair (A, B) the lanes take 64 consecutive
// elements x of A, lower-bound them in B (pos, match), and with the matches
// before x (a ballot prefix) get the element's rank in the union,
//     rank = (x + 1) + (pos + match) - matches(A[0..x]),
// so x is one of the s smallest of the union iff rank <= s: shared = matches with
// rank <= s, denom = min(s, |A| + |B| - matches).  Ranks grow with x, so when
// denom is known beforehand (a full row) the loop stops at the first rank > s.
// No 2s-step sequential merge; s * log2(s) / 64 LDS reads per lane and pair.
// T = min(kTileMax, kDistElems / s / 2); below T = 4 (s > 2048 shipped) the rows
// stay in global memory (L2) and the tile is 8 x 8, for locality only.
//
// Constants, shipped / under -DKMC_DIAG_HOOKS (libkmc_diag.so; small, so that a
// few hundred entries span many walking workgroups, chunks and flushes, and a
// few records many tiles; no new symbol):
//   kWalkBlock   threads of a walking workgroup           1024 / 64
//   kChunk       entries per chunk (kWalkBlock * kItems)  4096 / 64
//   kWalkPer     entries per walking workgroup, at least  16384 / 256
//   kDistElems   LDS capacity of a distance tile, values  16384 / 512   (kmc_sketch_pair.h)
//   kTileMax     tile edge at most, rows                  32 / 4        (kmc_sketch_pair.h)
// LDS, shipped: walk 1 KB; sort 8 / 32 / 128 KB for s <= 1024 / 4096 / 16384;
// distance tile 128 KB (one workgroup of 1024 threads per CU of 160 KB).
// Workspace: 2 KB of bins + 16 B per record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc.h"
#include "kmc_dist_common.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_triangle.h"
#include "kmc_walk.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

#ifdef KMC_DIAG_HOOKS
constexpr int kWalkBlock = 64;
constexpr int kItems = 1;
constexpr int64_t kWalkPer = 256;
#else
constexpr int kWalkBlock = 1024;
constexpr int kItems = 4;
constexpr int64_t kWalkPer = 16384;
#endif
constexpr int64_t kChunk = (int64_t)kWalkBlock * kItems;
constexpr int kDigitBits = 8;
constexpr int kDigits = 1 << kDigitBits;
constexpr int kLevels = 64 / kDigitBits;
constexpr uint64_t kMaxEntries = 1ull << 40;

struct KParams {
    const uint64_t *keys;
    const uint32_t *counts;
    const uint64_t *rec_off;
    int64_t E;  // num_entries
    int64_t n;
    int64_t per;  // entries per walking workgroup
    uint32_t s, min_count;
    uint64_t seed;
    unsigned long long *hist;  // [n * kDigits]
    uint64_t *thr;             // [n] prefix fixed so far; after the last level T_r
    uint32_t *need;            // [n] rank still looked for among the hashes under the prefix; 0: no search
    uint32_t *cursor;          // [n]
    uint64_t *sketches;
    uint32_t *sizes;
};

__device__ __forceinline__ bool takes_part(const KParams &p, int64_t e) {
    return p.min_count <= 1 || p.counts[e] >= p.min_count;
}

__device__ __forceinline__ uint64_t hash_of(const KParams &p, uint64_t key) { return sketch_hash(key, p.seed); }

// One digit level: bins of bits [shift, shift + kDigitBits) of the hashes that agree
// with thr[record] above them (FIRST: the top digit, every participating hash).
template <bool FIRST>
__global__ __launch_bounds__(kWalkBlock) void sketch_hist_kernel(KParams p, int shift) {
    __shared__ uint32_t lh[kDigits];
    __shared__ int64_t win[2];
    __shared__ int64_t last_rec;
    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    const int64_t e0 = w * p.per < p.E ? w * p.per : p.E;
    const int64_t e1 = e0 + p.per < p.E ? e0 + p.per : p.E;
    for (int d = tid; d < kDigits; d += kWalkBlock) lh[d] = 0;
    range_window(p, e0, e1, win);
    __syncthreads();
    int64_t cur = win[0];  // the record lh belongs to (in [0, n]; n: none)
    for (int64_t c0 = e0; c0 < e1; c0 += kChunk) {
        const int64_t c1 = c0 + kChunk < e1 ? c0 + kChunk : e1;
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int64_t e = c0 + (int64_t)it * kWalkBlock + tid;
            if (e >= c1) continue;
            const int64_t r = rec_of(p, e, win);
            if (e == c1 - 1) last_rec = r;
            if (r < 0 || !takes_part(p, e)) continue;
            const uint64_t h = hash_of(p, p.keys[e]);
            if constexpr (!FIRST) {
                if (p.need[r] == 0) continue;
                if ((h ^ p.thr[r]) >> (shift + kDigitBits)) continue;
            }
            const int d = (int)((h >> shift) & (kDigits - 1));
            if (r == cur)
                atomicAdd(&lh[d], 1u);
            else
                atomicAdd(&p.hist[r * kDigits + d], 1ull);
        }
        __syncthreads();
        const int64_t lr = last_rec;
        const bool moves = lr >= 0 && lr != cur;
        if (moves || c1 == e1) {
            for (int d = tid; d < kDigits; d += kWalkBlock) {
                const uint32_t v = lh[d];
                if (v && cur < p.n) atomicAdd(&p.hist[cur * kDigits + d], (unsigned long long)v);
                lh[d] = 0;
            }
            if (moves) cur = lr;
        }
        __syncthreads();
    }
}

// The digit at which the running count of record r's bins reaches need[r]; the bins
// are left zero for the next level.
__global__ __launch_bounds__(kDigits) void sketch_decide_kernel(KParams p, int shift, int first) {
    __shared__ unsigned long long wsum[kDigits / 64];
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    for (int64_t r = blockIdx.x; r < p.n; r += gridDim.x) {
        const unsigned long long v = p.hist[r * kDigits + d];
        p.hist[r * kDigits + d] = 0;
        unsigned long long incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long total = 0;
        for (int q = 0; q < kDigits / 64; ++q) {
            if (q < wave) incl += wsum[q];
            total += wsum[q];
        }
        const unsigned long long excl = incl - v;
        uint32_t need;
        uint64_t prefix;
        if (first) {
            need = total > p.s ? p.s : 0u;
            prefix = 0;
        } else {
            need = p.need[r];
            prefix = p.thr[r];
        }
        __syncthreads();  // every thread has read need / thr / wsum
        if (first && d == 0) {
            p.sizes[r] = total > p.s ? p.s : (uint32_t)total;
            if (need == 0) {
                p.need[r] = 0;
                p.thr[r] = kFill;
            }
        }
        if (need != 0 && excl < need && need <= incl) {
            p.thr[r] = prefix | ((uint64_t)d << shift);
            p.need[r] = need - (uint32_t)excl;
        }
    }
}

__global__ __launch_bounds__(kWalkBlock) void sketch_collect_kernel(KParams p) {
    __shared__ int64_t win[2];
    const int64_t w = blockIdx.x;
    const int64_t e0 = w * p.per < p.E ? w * p.per : p.E;
    const int64_t e1 = e0 + p.per < p.E ? e0 + p.per : p.E;
    range_window(p, e0, e1, win);
    __syncthreads();
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kWalkBlock) {
        const int64_t r = rec_of(p, e, win);
        if (r < 0 || !takes_part(p, e)) continue;
        const uint64_t h = hash_of(p, p.keys[e]);
        if (h > p.thr[r]) continue;
        const uint32_t at = atomicAdd(&p.cursor[r], 1u);
        // distinct keys: exactly sizes[r] entries come here; a repeated key may bring more
        if (at < p.sizes[r]) p.sketches[r * (int64_t)p.s + at] = h;
    }
}

// Sorts row r's sizes[r] collected values (bitonic, in LDS) and writes the whole row.
template <int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void sketch_sort_kernel(KParams p) {
    __shared__ uint64_t buf[CAP];
    const int tid = threadIdx.x;
    const int s = (int)p.s;  // <= CAP
    for (int64_t r = blockIdx.x; r < p.n; r += gridDim.x) {
        uint64_t *row = p.sketches + r * (int64_t)s;
        const int m = row_size(p.sizes, r, s), P = pow2_at_least(m);
        for (int i = tid; i < P; i += BLOCK) buf[i] = i < m ? row[i] : kFill;
        __syncthreads();
        bitonic_sort<BLOCK>(buf, 1, P, tid, [] { __syncthreads(); });
        for (int i = tid; i < s; i += BLOCK) row[i] = i < m ? buf[i] : kFill;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// distances
// ---------------------------------------------------------------------------
// The packed upper triangle is the shape Triangle of kmc_sketch_triangle.h, which the
// clustering (kmc_sketch_cluster.hip) walks as well.

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct KLayout {
    unsigned long long *hist;
    uint64_t *thr;
    uint32_t *need, *cursor;
    size_t bytes;
};

// the one layout behind the size query (base = null) and the bind
inline KLayout layout(void *base, int64_t n) {
    Carver c(base);
    KLayout L;
    L.hist = c.take<unsigned long long>((size_t)n * kDigits);
    L.thr = c.take<uint64_t>((size_t)n);
    L.need = c.take<uint32_t>((size_t)n);
    L.cursor = c.take<uint32_t>((size_t)n);
    L.bytes = c.total();
    return L;
}

inline bool sketch_args_ok(uint64_t num_entries, uint32_t sketch_size) {
    return sketch_size_ok(sketch_size) && num_entries <= kMaxEntries;
}

DeviceCache s_ws;  // library-owned workspace

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" size_t kmc_sketch_workspace_size(uint64_t num_seqs, uint64_t num_entries, uint32_t sketch_size,
                                            int device) {
    if (!sketch_args_ok(num_entries, sketch_size) || device < 0 || num_seqs == 0 || num_seqs > kMaxEntries) return 0;
    return layout(nullptr, (int64_t)num_seqs).bytes;
}

extern "C" int kmc_sketch_from_counts(const uint64_t *keys, const uint32_t *counts, const uint64_t *rec_offsets,
                                      uint64_t num_entries, uint64_t num_seqs, uint32_t sketch_size, uint64_t seed,
                                      uint32_t min_count, uint64_t *sketches, uint32_t *sketch_sizes, void *workspace,
                                      size_t workspace_bytes, hipStream_t stream) {
    if (!sketch_args_ok(num_entries, sketch_size)) return KMC_ERR_INVALID_ARG;
    if (num_seqs == 0) return KMC_OK;
    if (!rec_offsets || !sketches || !sketch_sizes) return KMC_ERR_INVALID_ARG;
    if (num_entries > 0 && !keys) return KMC_ERR_INVALID_ARG;
    if (min_count > 1 && !counts) return KMC_ERR_INVALID_ARG;
    if (num_seqs > kMaxEntries) return KMC_ERR_INVALID_ARG;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const int64_t n = (int64_t)num_seqs, E = (int64_t)num_entries;
    KLayout L;
    if (int e = bind_layout(s_ws, device, workspace, workspace_bytes, 0, [&](void *b) { return layout(b, n); }, &L))
        return e;
    int64_t g = (E + kWalkPer - 1) / kWalkPer;
    if (g > 2LL * cus) g = 2LL * cus;
    if (g < 1) g = 1;
    KParams p;
    p.keys = keys;
    p.counts = counts;
    p.rec_off = rec_offsets;
    p.E = E;
    p.n = n;
    p.per = (E + g - 1) / g;
    p.s = sketch_size;
    p.min_count = min_count;
    p.seed = seed;
    p.hist = L.hist;
    p.thr = L.thr;
    p.need = L.need;
    p.cursor = L.cursor;
    p.sketches = sketches;
    p.sizes = sketch_sizes;
    // the bins and the cursors are accumulated into; thr and need are written by level 0's decide
    // (the whole workspace: hist is its first array)
    if (hipError_t he = hipMemsetAsync(L.hist, 0, L.bytes, stream)) return (int)he;
    const unsigned rec_grid = (unsigned)(n < kMaxGridX ? n : kMaxGridX);
    for (int level = 0; level < kLevels; ++level) {
        const int shift = 64 - kDigitBits * (level + 1);
        if (E > 0) {
            if (level == 0)
                hipLaunchKernelGGL(sketch_hist_kernel<true>, dim3((unsigned)g), dim3(kWalkBlock), 0, stream, p, shift);
            else
                hipLaunchKernelGGL(sketch_hist_kernel<false>, dim3((unsigned)g), dim3(kWalkBlock), 0, stream, p, shift);
        }
        hipLaunchKernelGGL(sketch_decide_kernel, dim3(rec_grid), dim3(kDigits), 0, stream, p, shift, level == 0 ? 1 : 0);
    }
    if (E > 0) hipLaunchKernelGGL(sketch_collect_kernel, dim3((unsigned)g), dim3(kWalkBlock), 0, stream, p);
    for_cap(sketch_size, [&](auto cap) {
        constexpr int CAP = decltype(cap)::value, BLOCK = CAP <= 1024 ? 256 : 1024;
        hipLaunchKernelGGL((sketch_sort_kernel<CAP, BLOCK>), dim3(rec_grid), dim3(BLOCK), 0, stream, p);
    });
    return (int)hipGetLastError();
}

extern "C" int kmc_sketch_distances(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                                    uint32_t sketch_size, int k, float *out, uint32_t *shared, uint32_t *denom,
                                    hipStream_t stream) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (num_seqs < 2) return KMC_OK;
    if (!sketches || !sketch_sizes || !out) return KMC_ERR_INVALID_ARG;
    if (!sketch_size_ok(sketch_size)) return KMC_ERR_INVALID_ARG;
    if (num_seqs > KMC_SPARSE_MAX_SEQS) return KMC_ERR_INVALID_ARG;
    Tiling p;
    const bool stage = triangle_tiling(p, sketches, sketch_sizes, (int64_t)num_seqs, sketch_size);
    launch_tiles<Triangle>(p, stage, DistOut{out, shared, denom, k}, stream);
    return (int)hipGetLastError();
}
