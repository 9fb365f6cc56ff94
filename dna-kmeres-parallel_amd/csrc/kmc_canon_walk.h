// kmc_canon_walk.h — the canonical window walk shared by the canonical counter
// (kmc_hash.hip: K1, K3a) and the direct sketcher (kmc_sketch_seq.hip): a
// workgroup's 16-byte chunk range cut into record pieces (for_each_piece), the 48
// bytes behind a chunk's 16 window starts (chunk_raw) and their 16 canonical keys
// with the validity mask (chunk_keys).  Device code only.  (The dense and radix
// kernels, k <= 13, walk 1 KiB tiles instead: for_each_tile_piece, kmc_stream.h.)
//
// The parameter block P of a kernel supplies
//   data, idx, n       the bytes (data[p] is byte p), the record offsets, the records
//   lo, hi             window starts lie in [lo, hi) (= [idx[0], idx[n]))
//   k, flags           KMC_CANON_*
//   c_lo, cpw          first chunk of workgroup 0, chunks per workgroup
// and chunk_keys takes what a window stores as a functor of its key (Out): the
// counter's partition value, the sketcher's hash.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kmc.h"
#include "kmc_stream.h"

namespace kmc {

// LE 2-bit code (first base in the low bits, the dense path's order) -> MSB-first
__device__ __forceinline__ uint64_t reverse_groups(uint64_t c, int k) {
    uint64_t x = __builtin_bitreverse64(c);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    return x >> (64 - 2 * k);
}

__device__ __forceinline__ uint4 load16(const char *data, int64_t q, int64_t hi_byte) {
    // 16 bytes at q (16-aligned); bytes at or past hi_byte read as 0
    if (q + 16 <= hi_byte) return *reinterpret_cast<const uint4 *>(data + q);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (q + i < hi_byte) v[i >> 2] |= (uint32_t)(uint8_t)data[q + i] << (8 * (i & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void chunk_codes(uint4 r, bool soft, uint32_t &code, uint32_t &bad) {
    if (soft) {  // lowercase acgt -> ACGT (clearing bit 5 maps no other byte onto a base letter)
        r.x &= 0xDFDFDFDFu; r.y &= 0xDFDFDFDFu; r.z &= 0xDFDFDFDFu; r.w &= 0xDFDFDFDFu;
    }
    uint32_t any;
    decode16(r, code, any);
    bad = any ? bad_mask16(r) : 0u;
}

// The hashed keys of the (up to 16) valid windows starting in 16-byte chunk q of
// record piece [ps, pe) (window starts) of a record whose terminator is at
// rend - 1: bit j of the result is set when h[j] holds window q + j.
// The 48 bytes chunk_keys decodes for chunk q (its 16 window starts + 32 halo bytes),
// loaded ahead of use by the input walks
struct ChunkRaw {
    uint4 r[3];
};
// Round 4: three unconditional raw buffer loads over [the wave's first chunk, the
// end of the last record rounded up to 16 bytes): the hardware range check returns
// zeros past it, so no lane branches around its loads.  (load16's per-lane bounds
// branch made the compiler wait for the prefetched chunk -- s_waitcnt vmcnt(0) at
// the bottom of every iteration -- so the walks had one chunk in flight per thread
// and paid the full HBM latency per round.)  Bytes between the last record's end
// and the next 16-byte boundary are read but never reach a counted window (every
// counted window ends before its record's terminator), and that block never
// crosses a page.  q is 16-aligned; the wave's lane 0 holds its smallest q.
template <class P>
__device__ __forceinline__ ChunkRaw chunk_raw(const P &p, int64_t q) {
    const int64_t hi16 = (p.hi + 15) & ~(int64_t)15;  // p.hi = idx[n] (wave-uniform)
    // (both halves zero-extended: a sign-extended low half would corrupt q >= 2^31)
    const int64_t base = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)q) |
                                   ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)q >> 32))
                                    << 32));
    int64_t nrec = hi16 - base;
    nrec = nrec < 0 ? 0 : (nrec > (1ll << 31) ? (1ll << 31) : nrec);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(p.data) + base, (short)0, (int)nrec, 0x00020000);
    const int off = (int)(q - base);
    ChunkRaw c;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16 * i, 0, 0);
        c.r[i] = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return c;
}

// Round 4: templated on the orientation (FWD: KMC_CANON_FORWARD) and on the key
// width (BIGK: 16 <= k <= 31, so the low dword of the 2k-bit mask is all ones; else
// k <= 15 and the key fits one dword), and written dword by dword -- the forward key
// rolled with one funnel shift (v_alignbit) and one shift-or, the reverse
// complement one funnel shift of the complemented codes per dword -- so that no
// 64-bit mask, shift or orientation select is left per window (the walks are
// VALU-bound: K1 24 -> 18 VALU per window).  h[j] = out(key of window j).
template <bool FWD, bool BIGK, class P, class Out>
__device__ __forceinline__ uint32_t chunk_keys(const P &p, const ChunkRaw &raw, int64_t q, int64_t ps, int64_t pe,
                                               int64_t rend, Out out, unsigned long long (&h)[16]) {
    const int k = p.k;
    const bool soft = p.flags & KMC_CANON_SOFTMASK;
    // the low 2k bits: mh of the high dword and all of the low one (BIGK), or ml of the low one
    const uint32_t mh = BIGK ? (uint32_t)((1ull << (2 * k - 32)) - 1ull) : 0u;
    const uint32_t ml = BIGK ? 0xFFFFFFFFu : (uint32_t)((1ull << (2 * k)) - 1ull);
    uint32_t cd[3], bd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) chunk_codes(raw.r[i], soft, cd[i], bd[i]);
    const uint64_t badm = (uint64_t)bd[0] | ((uint64_t)bd[1] << 16) | ((uint64_t)bd[2] << 32);
    const int64_t last = std::min<int64_t>(pe, rend - k);  // window starts < last
    // window starts [ps, last) of this chunk as a mask (32-bit compares: the
    // chunk's offsets are 0..15)
    const int64_t lo_j = ps - q, hi_j = last - q;
    const uint32_t lo_m = lo_j <= 0 ? 0xFFFFu : (lo_j >= 16 ? 0u : (0xFFFFu << lo_j) & 0xFFFFu);
    const uint32_t hi_m = hi_j >= 16 ? 0xFFFFu : (hi_j <= 0 ? 0u : (1u << hi_j) - 1u);
    uint32_t vm = lo_m & hi_m;
    // windows holding an invalid base: bit j of the smeared mask = OR of badm's bits
    // j .. j+k-1 (log2 k wave-uniform doubling steps per chunk, instead of a 64-bit
    // shift, mask and compare per window)
    {
        uint64_t sm = badm;
        for (int c = 1; c < k;) {
            const int st = c < k - c ? c : k - c;
            sm |= sm >> st;
            c += st;
        }
        vm &= ~(uint32_t)sm;
    }
    // window 0's MSB-first key by bit reversal; window j's last base (j + k - 1) is
    // bits 2j of tl = the codes from base k - 1 on (2j <= 30: the low dword)
    const uint64_t lo64 = (uint64_t)cd[0] | ((uint64_t)cd[1] << 32);
    const uint64_t fw0 = reverse_groups(lo64 & (((uint64_t)mh << 32) | ml), k);
    uint32_t fl = (uint32_t)fw0, fh = (uint32_t)(fw0 >> 32);
    const int sk = 2 * (k - 1);
    const uint32_t tl = sk < 32 ? __builtin_amdgcn_alignbit(cd[1], cd[0], sk) : __builtin_amdgcn_alignbit(cd[2], cd[1], sk - 32);
    const uint32_t n0 = ~cd[0], n1 = ~cd[1], n2 = ~cd[2];  // complemented codes: the reverse complement's key
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j > 0) {  // roll the forward key one base
            const uint32_t b = (tl >> (2 * j)) & 3u;
            if (BIGK) {
                fh = __builtin_amdgcn_alignbit(fh, fl, 30) & mh;
                fl = (fl << 2) | b;
            } else {
                fl = ((fl << 2) | b) & ml;
            }
        }
        const uint64_t f = ((uint64_t)fh << 32) | fl;
        uint64_t key = f;
        if (!FWD) {  // the reverse complement's key = the complemented LE code of the window
            uint32_t rl = j == 0 ? n0 : __builtin_amdgcn_alignbit(n1, n0, 2 * j);
            uint32_t rh = 0u;
            if (BIGK) rh = (j == 0 ? n1 : __builtin_amdgcn_alignbit(n2, n1, 2 * j)) & mh;
            else rl &= ml;
            const uint64_t r = ((uint64_t)rh << 32) | rl;
            key = f < r ? f : r;
        }
        h[j] = out(key);
    }
    return vm;
}

// The workgroup's chunk range and its record pieces: f(r, ps, pe, rend).
template <class P, class F>
__device__ __forceinline__ void for_each_piece(const P &p, int64_t *s_first, F &&f) {
    const int w = blockIdx.x;
    const int64_t cb = p.c_lo + (int64_t)w * p.cpw;
    const int64_t wlo = std::max<int64_t>(cb << 4, p.lo), whi = std::min<int64_t>((cb + p.cpw) << 4, p.hi);
    if (wlo >= whi) return;
    if (threadIdx.x == 0) {  // last record r with idx[r] <= wlo
        int64_t a = 0, b = p.n - 1;
        while (a < b) {
            const int64_t m = (a + b + 1) >> 1;
            if (p.idx[m] <= wlo) a = m; else b = m - 1;
        }
        *s_first = a;
    }
    __syncthreads();
    for (int64_t r = *s_first; r < p.n; ++r) {
        const int64_t a = p.idx[r], e = p.idx[r + 1];
        if (a >= whi) break;
        const int64_t nw = e - a - p.k > 0 ? e - a - p.k : 0;
        const int64_t ps = std::max(a, wlo), pe = std::min(a + nw, whi);
        if (ps >= pe) continue;
        f(r, ps, pe, e);
    }
}

}  // namespace kmc
