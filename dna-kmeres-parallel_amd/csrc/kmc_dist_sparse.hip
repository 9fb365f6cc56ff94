// kmc_dist_sparse.hip — pairwise k-mer distance from sparse per-record
// (key, count) lists: step 2 for the canonical counter (k <= 31), where no
// 4^k x num_seqs matrix exists.
//
//     d(i, j) = 1 - S_ij / (min(len_i, len_j) - k + 1),
//     S_ij    = sum over keys present in both i and j of min(c_i, c_j)   (exact, uint64),
//
// with the packing, length and float expression of the dense path
// (kmc_dist_common.h), so the result equals kmc_pair_distances bit for bit when
// the entries are the non-zero bins of a dense matrix.
//
// Records list their keys in no order, so S_ij is a multi-way set intersection.
// As in kmc_hash.hip, equal keys are brought together by hash partitioning and
// matched in LDS; no hash table lives in HBM.  Pipeline, all on the caller's
// stream, no host read-back:
//   count    G workgroups walk contiguous entry ranges [e0, e1) of [0, num_entries);
//            the record of an entry comes from one search of rec_offsets per range
//            (then a search inside that window per entry); bucket = top bits of
//            mix(key); per-workgroup LDS histogram -> cnt[bucket * G + workgroup]
//   scan     kmc_scan.h over cnt: every (bucket, workgroup) segment gets its place
//   scatter  the same walk again writes 16-byte (key, rec << 32 | count) entries
//            into the workgroup's own segment of each bucket (LDS cursors only)
//   match    workgroups stride over buckets.  A bucket is taken in P passes (P a
//            power of two, 1 when it fits): pass p keeps the entries whose low hash
//            bits equal p, re-reading the bucket.  The kept entries go into an LDS
//            table with per-slot chains (one ds atomic exchange per entry; a sort
//            would need log^2 barrier rounds for the same grouping); every entry
//            then walks the chain below it and adds min(c_a, c_b) for each equal
//            key, so each of the g(g-1)/2 pairs of a key group is met once.
//            A pass that keeps more than the LDS capacity -- an unlucky hash, or
//            one key group larger than the capacity, which no hash bit can split --
//            takes the tiled path instead: tiles of the bucket are compacted into
//            LDS one after another and every later entry of the pass is streamed
//            from HBM against the tile.  Quadratic, and correct for any content.
//            Pair sums go to a workgroup-private LDS matrix while num_seqs <=
//            kPairLdsSeqs (flushed with one global 64-bit atomic per non-zero pair
//            per workgroup), else straight to global atomics on acc[npairs].
//   finish   pair_finish_kernel: acc -> out.
//
// Entries are only ever addressed by the walk's own index e < num_entries;
// rec_offsets values are clamped to num_entries and merely compared against, so
// whatever they hold, keys/counts are never read at or beyond num_entries.  An
// entry no record claims (before rec_offsets[0], or at or after rec_offsets[n])
// is dropped.
//
// Constants, shipped / under -DKMC_DIAG_HOOKS (libkmc_diag.so; small, so that a
// few hundred entries reach the multi-pass and the tiled paths; no new symbol):
//   kBucketTarget  entries per bucket aimed at           1024 / 64
//   kMaxBuckets    buckets at most (LDS histogram)       32768 / 256
//   kCap           LDS capacity of a pass, entries       4096 / 256
//   kHeads         chain heads (2 * kCap)                8192 / 512
// LDS, shipped: the walk's histogram is 128 KB; a match workgroup (1024 threads)
// holds 32 + 32 + 16 + 32 KB of table and a 15.8 KB pair matrix = 128 KB, so one
// workgroup per CU (160 KB) of either.  Past 32768 * 1024 entries the buckets
// outgrow the target and the pass count grows instead: at 4e8 entries a bucket
// holds 12 K entries and is read 8 times (from L2: it is 195 KB).  With 8192
// buckets and kCap 2048 that was 64 reads and 3.2 times the run time.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kmc.h"
#include "kmc_dist_common.h"
#include "kmc_internal.h"
#include "kmc_scan.h"
#include "kmc_walk.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

#ifdef KMC_DIAG_HOOKS
constexpr int64_t kBucketTarget = 64;
constexpr int kMaxBuckets = 256;
constexpr int kCap = 256;
#else
constexpr int64_t kBucketTarget = 1024;
constexpr int kMaxBuckets = 32768;
constexpr int kCap = 4096;
#endif
constexpr int kHeads = 2 * kCap;
constexpr int kWalkBlock = 1024;       // count / scatter threads per workgroup
constexpr int64_t kWalkPer = 8192;     // entries per walking workgroup aimed at (at least)
constexpr int kMatchBlock = 1024;
constexpr int kPairLdsSeqs = 64;       // LDS pair matrix up to this many records
constexpr int kPairLds = kPairLdsSeqs * (kPairLdsSeqs - 1) / 2;
constexpr int kMaxPassLg = 20;         // pass bits: hash bits 0..19; chain slot: bits 20..; bucket: top bits
constexpr uint32_t kNil = ~0u;

struct __attribute__((aligned(16))) Ent {
    uint64_t key, val;  // val = rec << 32 | count
};

struct SParams {
    const uint64_t *keys;
    const uint32_t *counts;
    const uint64_t *rec_off;
    int64_t E;  // num_entries
    int64_t n;
    int64_t per;  // entries per walking workgroup
    int G;        // walking workgroups
    int B, lgB;   // buckets (power of two)
    uint32_t *cnt;          // [B * G]
    const uint64_t *off;    // [B * G + 1], exclusive scan of cnt
    Ent *ent;               // [E]
    unsigned long long *acc;  // [npairs]
};

__device__ __forceinline__ uint64_t mix_key(uint64_t key) { return splitmix64_at(key, 0); }

__device__ __forceinline__ int bucket_of(uint64_t h, int lgB) { return lgB ? (int)(h >> (64 - lgB)) : 0; }

// the walk itself (off_c, find_rec, range_window, rec_of over rec_off, E, n): kmc_walk.h

__global__ __launch_bounds__(kWalkBlock) void sparse_count_kernel(SParams p) {
    __shared__ uint32_t hist[kMaxBuckets];
    __shared__ int64_t win[2];
    const int w = blockIdx.x;
    const int64_t e0 = (int64_t)w * p.per < p.E ? (int64_t)w * p.per : p.E;
    const int64_t e1 = e0 + p.per < p.E ? e0 + p.per : p.E;
    for (int b = threadIdx.x; b < p.B; b += kWalkBlock) hist[b] = 0;
    range_window(p, e0, e1, win);
    __syncthreads();
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kWalkBlock) {
        if (rec_of(p, e, win) < 0) continue;
        atomicAdd(&hist[bucket_of(mix_key(p.keys[e]), p.lgB)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < p.B; b += kWalkBlock) p.cnt[(int64_t)b * p.G + w] = hist[b];
}

__global__ __launch_bounds__(kWalkBlock) void sparse_scatter_kernel(SParams p) {
    __shared__ uint32_t cur[kMaxBuckets];
    __shared__ int64_t win[2];
    const int w = blockIdx.x;
    const int64_t e0 = (int64_t)w * p.per < p.E ? (int64_t)w * p.per : p.E;
    const int64_t e1 = e0 + p.per < p.E ? e0 + p.per : p.E;
    for (int b = threadIdx.x; b < p.B; b += kWalkBlock) cur[b] = 0;
    range_window(p, e0, e1, win);
    __syncthreads();
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kWalkBlock) {
        const int64_t r = rec_of(p, e, win);
        if (r < 0) continue;
        const uint64_t key = p.keys[e];
        const int b = bucket_of(mix_key(key), p.lgB);
        const int64_t seg = (int64_t)b * p.G + w;
        const uint32_t local = atomicAdd(&cur[b], 1u);
        const uint64_t pos = p.off[seg] + local;
        // the count walk saw the same entries, so the segment holds them: checked anyway
        if (local < p.cnt[seg] && pos < (uint64_t)p.E) {
            Ent x;
            x.key = key;
            x.val = ((uint64_t)r << 32) | (uint64_t)p.counts[e];
            p.ent[pos] = x;
        }
    }
}

template <bool LDSP>
__device__ __forceinline__ void add_pair(const SParams &p, unsigned long long *pm, uint64_t va, uint64_t vb) {
    int64_t i = (int64_t)(va >> 32), j = (int64_t)(vb >> 32);
    if (i == j) return;  // a key twice in one record: unspecified result, no pair of its own
    if (i > j) {
        const int64_t t = i;
        i = j;
        j = t;
    }
    if (j >= p.n) return;
    const uint32_t ca = (uint32_t)va, cb = (uint32_t)vb;
    const unsigned long long m = ca < cb ? ca : cb;
    const int64_t q = tri_index(i, j, p.n);
    if constexpr (LDSP)
        atomicAdd(&pm[q], m);
    else
        atomicAdd(&p.acc[q], m);
}

template <bool LDSP>
__global__ __launch_bounds__(kMatchBlock) void sparse_match_kernel(SParams p) {
    __shared__ uint64_t skey[kCap];
    __shared__ uint64_t sval[kCap];
    __shared__ uint32_t nxt[kCap];  // chain link (LDS pass) or position in the tile (tiled pass)
    __shared__ uint32_t heads[kHeads];
    __shared__ uint32_t kept;
    __shared__ unsigned long long pm[LDSP ? kPairLds : 1];
    const int tid = threadIdx.x;
    const int npairs = LDSP ? (int)(p.n * (p.n - 1) / 2) : 0;
    for (int q = tid; q < npairs; q += kMatchBlock) pm[q] = 0;

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int64_t bs = (int64_t)p.off[(int64_t)b * p.G], be0 = (int64_t)p.off[(int64_t)(b + 1) * p.G];
        const int64_t be = be0 < p.E ? be0 : p.E;
        const int64_t size = be - bs;
        if (size <= 0) continue;
        int lgP = 0;
        if (size > kCap)
            while (lgP < kMaxPassLg && size > ((int64_t)(kCap / 2) << lgP)) ++lgP;
        const uint64_t pmask = (1ull << lgP) - 1ull;
        for (uint64_t pass = 0; pass <= pmask; ++pass) {
            __syncthreads();
            for (int s = tid; s < kHeads; s += kMatchBlock) heads[s] = kNil;
            if (tid == 0) kept = 0;
            __syncthreads();
            for (int64_t q = bs + tid; q < be; q += kMatchBlock) {
                const Ent x = p.ent[q];
                const uint64_t h = mix_key(x.key);
                if ((h & pmask) != pass) continue;
                const uint32_t at = atomicAdd(&kept, 1u);
                if (at < (uint32_t)kCap) {
                    skey[at] = x.key;
                    sval[at] = x.val;
                    nxt[at] = atomicExch(&heads[(h >> kMaxPassLg) & (kHeads - 1)], at);
                }
            }
            __syncthreads();
            const uint32_t m = kept;
            if (m <= (uint32_t)kCap) {
                // every entry against the entries below it in its chain: each pair once
                for (uint32_t a = tid; a < m; a += kMatchBlock) {
                    const uint64_t key = skey[a], va = sval[a];
                    for (uint32_t c = nxt[a]; c != kNil; c = nxt[c])
                        if (skey[c] == key) add_pair<LDSP>(p, pm, va, sval[c]);
                }
                continue;
            }
            // tiled pass: more kept entries than LDS holds
            for (int64_t a0 = bs; a0 < be; a0 += kCap) {
                const int64_t a1 = a0 + kCap < be ? a0 + kCap : be;
                __syncthreads();
                if (tid == 0) kept = 0;
                __syncthreads();
                for (int64_t q = a0 + tid; q < a1; q += kMatchBlock) {
                    const Ent x = p.ent[q];
                    if ((mix_key(x.key) & pmask) != pass) continue;
                    const uint32_t at = atomicAdd(&kept, 1u);  // < kCap: the tile spans kCap positions
                    skey[at] = x.key;
                    sval[at] = x.val;
                    nxt[at] = (uint32_t)(q - a0);
                }
                __syncthreads();
                const uint32_t ta = kept;
                if (ta == 0) continue;
                for (int64_t q = a0 + tid; q < be; q += kMatchBlock) {
                    const Ent x = p.ent[q];
                    if ((mix_key(x.key) & pmask) != pass) continue;
                    const bool later = q >= a1;
                    const uint32_t rel = later ? 0u : (uint32_t)(q - a0);
                    for (uint32_t c = 0; c < ta; ++c)
                        if (skey[c] == x.key && (later || nxt[c] < rel)) add_pair<LDSP>(p, pm, x.val, sval[c]);
                }
            }
        }
    }
    if constexpr (LDSP) {
        __syncthreads();
        for (int q = tid; q < npairs; q += kMatchBlock) {
            const unsigned long long v = pm[q];
            if (v) atomicAdd(&p.acc[q], v);
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct SPlan {
    int G, B, lgB;
    int64_t per;
};

inline SPlan plan_for(int64_t E, int cus) {
    SPlan P;
    int64_t g = (E + kWalkPer - 1) / kWalkPer;
    if (g > 2LL * cus) g = 2LL * cus;
    if (g < 1) g = 1;
    P.G = (int)g;
    P.per = (E + g - 1) / g;
    P.lgB = 0;
    while ((1 << P.lgB) < kMaxBuckets && ((int64_t)kBucketTarget << P.lgB) < E) ++P.lgB;
    P.B = 1 << P.lgB;
    return P;
}

struct SLayout {
    unsigned long long *acc;
    uint32_t *cnt;
    uint64_t *bsum, *off;
    Ent *ent;
    size_t bytes, acc_bytes;
};

// the one layout behind the size query (base = null) and the bind
inline SLayout layout(void *base, int64_t n, int64_t E, const SPlan &P) {
    Carver c(base);
    SLayout L;
    const size_t npairs = (size_t)(n * (n - 1) / 2), m = (size_t)P.B * (size_t)P.G;
    L.acc = c.take<unsigned long long>(npairs);
    L.cnt = c.take<uint32_t>(m);
    L.bsum = c.take<uint64_t>((size_t)scan_tiles((int64_t)m));
    L.off = c.take<uint64_t>(m + 1);
    L.ent = c.take<Ent>((size_t)E);
    L.bytes = c.total();
    L.acc_bytes = npairs * sizeof(unsigned long long);
    return L;
}

constexpr uint64_t kMaxSeqs = KMC_SPARSE_MAX_SEQS;
constexpr uint64_t kMaxEntries = 1ull << 40;

DeviceCache s_ws;  // library-owned workspace

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" size_t kmc_pair_distances_sparse_workspace_size(uint64_t num_seqs, uint64_t num_entries, int device) {
    if (num_seqs < 2 || num_seqs > kMaxSeqs || num_entries > kMaxEntries) return 0;
    int cus = 0;
    if (device_cus(device, &cus)) return 0;
    const SPlan P = plan_for((int64_t)num_entries, cus);
    return layout(nullptr, (int64_t)num_seqs, (int64_t)num_entries, P).bytes;
}

extern "C" int kmc_pair_distances_sparse(const uint64_t *keys, const uint32_t *counts, const uint64_t *rec_offsets,
                                         uint64_t num_entries, const int64_t *indices, uint64_t num_seqs, int k,
                                         float *out, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (k < 1 || k > KMC_CANON_MAX_K) return KMC_ERR_UNSUPPORTED_K;
    if (num_seqs < 2) return KMC_OK;
    if (!rec_offsets || !indices || !out) return KMC_ERR_INVALID_ARG;
    if (num_entries > 0 && (!keys || !counts)) return KMC_ERR_INVALID_ARG;
    if (num_seqs > kMaxSeqs || num_entries > kMaxEntries) return KMC_ERR_INVALID_ARG;
    int device = 0, cus = 0;
    int e = current_device_cus(&device, &cus);
    if (e) return e;
    const int64_t n = (int64_t)num_seqs, E = (int64_t)num_entries;
    const SPlan P = plan_for(E, cus);
    const size_t need = layout(nullptr, n, E, P).bytes;
    void *ws = nullptr;
    if ((e = bind_workspace(s_ws, device, need, workspace, workspace_bytes, 0, &ws))) return e;
    const SLayout L = layout(ws, n, E, P);
    SParams p;
    p.keys = keys;
    p.counts = counts;
    p.rec_off = rec_offsets;
    p.E = E;
    p.n = n;
    p.per = P.per;
    p.G = P.G;
    p.B = P.B;
    p.lgB = P.lgB;
    p.cnt = L.cnt;
    p.off = L.off;
    p.ent = L.ent;
    p.acc = L.acc;
    // acc is the only array accumulated into; cnt, off and ent are written whole before they are read
    const hipError_t he = hipMemsetAsync(L.acc, 0, L.acc_bytes, stream);
    if (he != hipSuccess) return (int)he;
    if (E > 0) {
        hipLaunchKernelGGL(sparse_count_kernel, dim3((unsigned)P.G), dim3(kWalkBlock), 0, stream, p);
        excl_scan_u32(L.cnt, (int64_t)P.B * P.G, L.bsum, L.off, stream);
        hipLaunchKernelGGL(sparse_scatter_kernel, dim3((unsigned)P.G), dim3(kWalkBlock), 0, stream, p);
        int mg = 2 * cus < P.B ? 2 * cus : P.B;
        if (n <= kPairLdsSeqs)
            hipLaunchKernelGGL(sparse_match_kernel<true>, dim3((unsigned)mg), dim3(kMatchBlock), 0, stream, p);
        else
            hipLaunchKernelGGL(sparse_match_kernel<false>, dim3((unsigned)mg), dim3(kMatchBlock), 0, stream, p);
    }
    launch_pair_finish(L.acc, indices, n, k, out, stream);
    return (int)hipGetLastError();
}
