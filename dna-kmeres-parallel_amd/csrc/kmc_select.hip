// kmc_select.hip — stable compaction of byte records on the device
// (kmc_select_records) and the selection rule of `kmc --recruit` as a device call
// (kmc_match_select), with the assignment rule of `kmc --recruit --classify` beside it
// (kmc_classify_select).  No reference counterpart: the reference keeps no read text.
//
// The selected bytes are a monotone compaction of the source bytes, the situation
// of fq_write_kernel (kmc_fastq_gpu.hip), and the shape is the same.  Passes:
//   1. per record (sel_flag_kernel): the selection flag (uint32) and the kept length
//      (uint64: the record's clamped length when selected, else 0);
//   2. their exclusive scans (kmc_scan.h): rank[r], the selected records before r,
//      and pos[r], the kept bytes before r, in 64 bits;
//   3. per record (sel_offsets_kernel): dst_offsets[rank[r]] = pos[r] for a selected
//      r, the end entry and counts;
//   4. one pass over 16 KiB source tiles (sel_copy_kernel), skipped when dst_cap is 0:
//      a tile finds the records of its first and last byte by binary search in
//      `offsets`, computes its output range [ob, oe) from pos[] and leaves before its
//      loads when the range is empty; else every thread finds the record of its
//      first byte (a search between the tile's two), walks its 64 bytes, stages the
//      kept ones in LDS, and the block stores whole dwords (store_staged).
// Per source byte pass 4 reads one byte and writes one byte per kept byte; per record
// the passes 1-3 move 4 + 8 (keep, offsets) + 12 (flag, length) + 28 (the scans'
// reads and writes) + 16 (rank and pos read again) + 8 (dst_offsets) bytes, and pass
// 4 reads 16 bytes of offsets and pos per record boundary it crosses.  A record longer
// than a tile and thousands of records inside a tile take the same path: the unit
// of work is the source byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kmc.h"
#include "kmc_scan.h"
#include "kmc_text.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

constexpr int kSelBlock = 256;            // records per block of the per-record kernels
constexpr unsigned kSelMaxGrid = 1u << 30;  // blocks of a launch; the kernels stride over more
constexpr uint64_t kSelMaxRecs = 1ull << 40;
constexpr uint64_t kSelMaxBytes = 1ull << 62;

struct SParams {
    const uint8_t *base;   // src rounded down to 16 bytes
    int64_t mis;           // src - base
    int64_t n;             // src_bytes
    int64_t ntiles;        // tiles of base[0, mis + n)
    const int64_t *off;    // [nrec + 1]
    uint64_t nrec;
    const uint32_t *keep;  // [nrec]
    int invert;
    uint32_t *flag;        // [nrec] 1: selected
    uint64_t *klen;        // [nrec] kept bytes of the record
    uint64_t *rank;        // [nrec + 1] selected records before r
    uint64_t *pos;         // [nrec + 1] kept bytes before r
    uint8_t *out;          // dst rounded down to 4 bytes
    uint64_t dmis;         // dst - out
    uint64_t cap;          // dst_cap
    int64_t *dst_off;      // [nrec + 1] or null
    uint64_t *counts;      // [2]
};

// offsets[i] clamped to [0, src_bytes]
__device__ __forceinline__ int64_t offc(const SParams &p, uint64_t i) {
    return std::min<int64_t>(std::max<int64_t>(p.off[i], 0), p.n);
}

// 1. flag and kept length
__global__ __launch_bounds__(kSelBlock) void sel_flag_kernel(SParams p) {
    for (uint64_t r = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x; r < p.nrec; r += (uint64_t)gridDim.x * kSelBlock) {
        const int64_t lo = offc(p, r), hi = offc(p, r + 1);
        const bool sel = (p.keep[r] != 0u) != (p.invert != 0);
        p.flag[r] = sel ? 1u : 0u;
        p.klen[r] = sel && hi > lo ? (uint64_t)(hi - lo) : 0ull;
    }
}

// 3. output offsets and counts; thread nrec writes the end entry
__global__ __launch_bounds__(kSelBlock) void sel_offsets_kernel(SParams p) {
    for (uint64_t r = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x; r <= p.nrec; r += (uint64_t)gridDim.x * kSelBlock) {
        if (r < p.nrec) {
            if (p.dst_off && p.flag[r]) p.dst_off[p.rank[r]] = (int64_t)p.pos[r];
        } else {
            if (p.dst_off) p.dst_off[p.rank[r]] = (int64_t)p.pos[r];
            p.counts[0] = p.rank[r];
            p.counts[1] = p.pos[r];
        }
    }
}

// first index i in [a, b] with i == b or offsets[i] > x (ascending offsets; any
// offsets give an index in [a, b])
__device__ __forceinline__ uint64_t sel_upper(const SParams &p, int64_t x, uint64_t a, uint64_t b) {
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (offc(p, mid) <= x) a = mid + 1;
        else b = mid;
    }
    return a;
}

// record r = -1 (before the first), 0 .. nrec - 1, nrec (after the last): where it
// starts, where the next starts, its first output byte and its kept bytes
struct SelRec {
    int64_t lo, next;
    uint64_t a, kept;
};

__device__ __forceinline__ SelRec sel_rec(const SParams &p, int64_t r) {
    SelRec s;
    if (r < 0) {
        s.lo = 0; s.next = offc(p, 0); s.a = 0; s.kept = 0;
    } else if ((uint64_t)r >= p.nrec) {
        s.lo = 0; s.next = INT64_MAX; s.a = 0; s.kept = 0;
    } else {
        s.lo = offc(p, (uint64_t)r);
        s.next = offc(p, (uint64_t)r + 1);
        s.a = p.pos[r];
        s.kept = p.pos[r + 1] - s.a;
    }
    return s;
}

// Output bytes written before source position x, u = sel_upper(x) over all the offsets
// (the kept bytes are a monotone compaction of the source bytes).
__device__ __forceinline__ uint64_t sel_out_before(const SParams &p, int64_t x, uint64_t u) {
    if (u == 0) return 0;
    if (u > p.nrec) return p.pos[p.nrec];
    const SelRec s = sel_rec(p, (int64_t)u - 1);
    return s.a + std::min<uint64_t>((uint64_t)(x - s.lo), s.kept);
}

// 4. copy
__global__ __launch_bounds__(kFpBlock) void sel_copy_kernel(SParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kFpTile + 8];
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        // source positions [t0, t1) (t0 < 0 in the first tile of a misaligned src)
        const int64_t t0 = tile * kFpTile - p.mis, t1 = std::min<int64_t>(t0 + kFpTile, p.n);
        const int64_t f0 = std::max<int64_t>(t0, 0);
        // the tile's records and output range (block-uniform)
        const uint64_t u0 = sel_upper(p, f0, 0, p.nrec + 1), u1 = sel_upper(p, t1, u0, p.nrec + 1);
        const uint64_t ob = sel_out_before(p, f0, u0), oe = sel_out_before(p, t1, u1);
        if (oe <= ob) continue;  // nothing kept (before any barrier of this round)
        const uint64_t gb = ob + p.dmis;  // in bytes of p.out
        const uint32_t shift = (uint32_t)(gb & 3u);
        const int64_t q = t0 + (int64_t)threadIdx.x * kFpPer;
        if (q < t1 && q + kFpPer > 0) {
            uint32_t w[16];
            load64(p.base, p.n + p.mis, q + p.mis, w);
            int64_t r = (int64_t)sel_upper(p, std::max<int64_t>(q, 0), u0, u1) - 1;
            SelRec s = sel_rec(p, r);
            if (s.kept != 0 || s.next < q + kFpPer) {  // else: 64 bytes of one dropped record
                for (int i = 0; i < kFpPer; ++i) {
                    const int64_t at_src = q + i;
                    if (at_src < 0) continue;
                    if (at_src >= p.n) break;
                    if (at_src >= s.next) {  // the next record that holds a byte: mostly r + 1
                        if ((uint64_t)(r + 2) >= u1 || offc(p, (uint64_t)(r + 2)) > at_src) r = r + 1;
                        else r = (int64_t)sel_upper(p, at_src, (uint64_t)(r + 3), u1) - 1;
                        s = sel_rec(p, r);
                    }
                    const uint64_t o = (uint64_t)(at_src - s.lo);
                    if (o < s.kept) {
                        const uint64_t at = s.a + o - ob;  // < the tile's kept bytes
                        if (at < (uint64_t)kFpTile) stage[shift + at] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
                    }
                }
            }
        }
        __syncthreads();
        const uint64_t end = std::min<uint64_t>(oe, p.cap);
        const uint32_t tk = end > ob ? (uint32_t)std::min<uint64_t>(end - ob, (uint64_t)kFpTile) : 0u;
        store_staged(p.out, stage, gb, tk);
        __syncthreads();  // before the next round's bytes are staged
    }
}

// kmc_match_select
__global__ __launch_bounds__(kSelBlock) void match_select_kernel(const uint32_t *sampled, const uint32_t *hits, uint64_t n,
                                                                uint32_t min_hits, double min_fraction, uint32_t *keep,
                                                                uint64_t *num_kept) {
    uint64_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kSelBlock) {
        const uint32_t hit = hits[r], smp = sampled ? sampled[r] : 0u;
        const bool k = hit >= min_hits && (double)hit >= min_fraction * (double)smp;
        keep[r] = k ? 1u : 0u;
        mine += k;
    }
    if (num_kept) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd((unsigned long long *)num_kept, (unsigned long long)mine);
    }
}

// kmc_classify_select (keep may be listed: a thread reads its word before it writes it)
__global__ __launch_bounds__(kSelBlock) void classify_select_kernel(const uint32_t *listed, const uint32_t *best,
                                                                   const uint32_t *best_hits, const uint32_t *next_hits,
                                                                   uint64_t n, uint32_t source, uint32_t min_margin,
                                                                   uint32_t *keep, uint64_t *num_kept) {
    uint64_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kSelBlock) {
        const bool in = listed ? listed[r] != 0u : true;
        const bool k = in && best[r] == source && best_hits[r] - next_hits[r] >= min_margin;
        keep[r] = k ? 1u : 0u;
        mine += k;
    }
    if (num_kept) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd((unsigned long long *)num_kept, (unsigned long long)mine);
    }
}

unsigned sel_grid(uint64_t items, uint64_t per_block) {
    const uint64_t b = (items + per_block - 1) / per_block;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), kSelMaxGrid);
}

DeviceCache sel_ws;

struct SelLayout {
    uint32_t *flag;
    uint64_t *klen, *rank, *pos, *bsum;
    size_t bytes;
};

SelLayout sel_layout(void *base, uint64_t nrec) {
    Carver c(base);
    SelLayout l;
    l.flag = c.take<uint32_t>((size_t)nrec);
    l.klen = c.take<uint64_t>((size_t)nrec);
    l.rank = c.take<uint64_t>((size_t)nrec + 1);
    l.pos = c.take<uint64_t>((size_t)nrec + 1);
    l.bsum = c.take<uint64_t>((size_t)scan_tiles((int64_t)nrec) + 1);  // of one scan after the other
    l.bytes = c.total();
    return l;
}

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" size_t kmc_select_records_workspace_size(uint64_t num_recs, uint64_t src_bytes) {
    if (num_recs > kSelMaxRecs || src_bytes >= kSelMaxBytes) return 0;
    return sel_layout(nullptr, num_recs).bytes;
}

extern "C" int kmc_select_records(const char *src, const int64_t *offsets, uint64_t num_recs, uint64_t src_bytes,
                                  const uint32_t *keep, int invert, char *dst, uint64_t dst_cap, int64_t *dst_offsets,
                                  uint64_t *counts, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!offsets || !keep || !counts) return KMC_ERR_INVALID_ARG;
    if ((!src && src_bytes > 0) || (!dst && dst_cap > 0)) return KMC_ERR_INVALID_ARG;
    if (num_recs > kSelMaxRecs || src_bytes >= kSelMaxBytes) return KMC_ERR_INVALID_ARG;
    if (src_bytes > 0 && dst_cap > 0) {  // the byte ranges share a byte
        const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
        const uintptr_t dend = dst_cap > UINTPTR_MAX - d ? UINTPTR_MAX : d + (uintptr_t)dst_cap;
        if (s < dend && d < s + (uintptr_t)src_bytes) return KMC_ERR_INVALID_ARG;
    }
    if (workspace) {  // (judged with the other arguments: no device is needed for it)
        if (workspace_bytes < sel_layout(nullptr, num_recs).bytes) return KMC_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 7u) return KMC_ERR_ALIGNMENT;
    }
    hipError_t he;
    if (num_recs == 0) {
        if ((he = hipMemsetAsync(counts, 0, 16, stream))) return (int)he;
        if (dst_offsets && (he = hipMemsetAsync(dst_offsets, 0, 8, stream))) return (int)he;
        return 0;
    }
    int device = 0;
    if ((he = hipGetDevice(&device))) return (int)he;
    SelLayout l;
    if (int e = bind_layout(sel_ws, device, workspace, workspace_bytes, 8,
                            [&](void *b) { return sel_layout(b, num_recs); }, &l))
        return e;
    SParams p{};
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    p.mis = (int64_t)(s & 15u);
    p.base = reinterpret_cast<const uint8_t *>(s - (uintptr_t)p.mis);
    p.n = (int64_t)src_bytes;
    p.ntiles = (p.n + p.mis + kFpTile - 1) / kFpTile;
    p.off = offsets;
    p.nrec = num_recs;
    p.keep = keep;
    p.invert = invert != 0;
    p.flag = l.flag;
    p.klen = l.klen;
    p.rank = l.rank;
    p.pos = l.pos;
    p.dmis = (uint64_t)(d & 3u);
    p.out = reinterpret_cast<uint8_t *>(d - (uintptr_t)p.dmis);
    p.cap = dst_cap;
    p.dst_off = dst_offsets;
    p.counts = counts;
    hipLaunchKernelGGL(sel_flag_kernel, dim3(sel_grid(num_recs, kSelBlock)), dim3(kSelBlock), 0, stream, p);
    excl_scan_u32(l.flag, (int64_t)num_recs, l.bsum, l.rank, stream);
    excl_scan_u64(l.klen, (int64_t)num_recs, l.bsum, l.pos, stream);
    hipLaunchKernelGGL(sel_offsets_kernel, dim3(sel_grid(num_recs + 1, kSelBlock)), dim3(kSelBlock), 0, stream, p);
    if (dst_cap > 0 && p.ntiles > 0)
        hipLaunchKernelGGL(sel_copy_kernel, dim3(sel_grid((uint64_t)p.ntiles, 1)), dim3(kFpBlock), 0, stream, p);
    return (int)hipGetLastError();
}

extern "C" int kmc_match_select(const uint32_t *sampled, const uint32_t *hits, uint64_t num_seqs, uint32_t min_hits,
                                double min_fraction, uint32_t *keep, uint64_t *num_kept, hipStream_t stream) {
    if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return KMC_ERR_INVALID_ARG;  // (NaN too)
    if (num_seqs > 0 && (!hits || !keep)) return KMC_ERR_INVALID_ARG;
    if (num_seqs > 0 && !sampled && min_fraction != 0.0) return KMC_ERR_INVALID_ARG;
    if (num_seqs > kSelMaxRecs) return KMC_ERR_INVALID_ARG;
    hipError_t he;
    if (num_kept && (he = hipMemsetAsync(num_kept, 0, 8, stream))) return (int)he;
    if (num_seqs == 0) return 0;
    hipLaunchKernelGGL(match_select_kernel, dim3(sel_grid(num_seqs, kSelBlock)), dim3(kSelBlock), 0, stream, sampled, hits,
                       num_seqs, min_hits, min_fraction, keep, num_kept);
    return (int)hipGetLastError();
}

extern "C" int kmc_classify_select(const uint32_t *listed, const uint32_t *best, const uint32_t *best_hits,
                                   const uint32_t *next_hits, uint64_t num_seqs, uint32_t source, uint32_t min_margin,
                                   uint32_t *keep, uint64_t *num_kept, hipStream_t stream) {
    if (source >= KMC_CLASSIFY_MAX_SOURCES) return KMC_ERR_INVALID_ARG;
    if (num_seqs > 0 && (!best || !best_hits || !next_hits || !keep)) return KMC_ERR_INVALID_ARG;
    if (num_seqs > kSelMaxRecs) return KMC_ERR_INVALID_ARG;
    hipError_t he;
    if (num_kept && (he = hipMemsetAsync(num_kept, 0, 8, stream))) return (int)he;
    if (num_seqs == 0) return 0;
    hipLaunchKernelGGL(classify_select_kernel, dim3(sel_grid(num_seqs, kSelBlock)), dim3(kSelBlock), 0, stream, listed,
                       best, best_hits, next_hits, num_seqs, source, min_margin, keep, num_kept);
    return (int)hipGetLastError();
}
