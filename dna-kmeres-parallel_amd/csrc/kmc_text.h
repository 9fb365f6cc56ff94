// kmc_text.h — device pieces shared by the two text parsers (kmc_fasta_gpu.hip,
// kmc_fastq_gpu.hip): the raw bytes are cut into 16 KiB tiles, one per block of
// 256 threads, 64 bytes per thread; a thread's bytes as 16 words, the SWAR newline
// count, the block's exclusive sum, and the store of a tile's output bytes staged
// in LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace kmc {
namespace {

constexpr int kFpBlock = 256;
constexpr int kFpPer = 64;                        // raw bytes per thread
constexpr int64_t kFpTile = kFpBlock * kFpPer;    // 16 KiB per block

// bytes [q, q + 64) of raw[0, n) as 16 little-endian words (bytes past n read as 0);
// raw is 16-byte aligned and q a multiple of 64
__device__ __forceinline__ void load64(const uint8_t *raw, int64_t n, int64_t q, uint32_t w[16]) {
    if (q + kFpPer <= n) {
        const uint4 *s = reinterpret_cast<const uint4 *>(raw + q);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = s[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = 0u;
        for (int i = 0; i < kFpPer; ++i)
            if (q + i < n) w[i >> 2] |= (uint32_t)raw[q + i] << (8 * (i & 3));
    }
}

__device__ __forceinline__ uint32_t nl_bits(uint32_t x) {  // bit 8i+7 set iff byte i == '\n'
    const uint32_t y = x ^ 0x0A0A0A0Au;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}

__device__ __forceinline__ uint32_t count_nl(const uint32_t w[16]) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c += __popc(nl_bits(w[i]));
    return c;
}

// block exclusive sum of a per-thread value (kFpBlock threads); total returned
__device__ __forceinline__ uint32_t block_excl_u32(uint32_t v, uint32_t *sh, uint32_t &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int i = 0; i < kFpBlock / 64; ++i) {
        if (i < wid) before += sh[i];
        total += sh[i];
    }
    __syncthreads();
    return before + x - v;
}

// A tile's output bytes [ob, ob + tk), staged so that stage[(ob & 3) + i] is output
// byte ob + i (stage 16-byte aligned, written by the whole block before the
// barrier that precedes this call): whole dwords, except the first and last
// partial dword of the range
__device__ __forceinline__ void store_staged(uint8_t *out, const uint8_t *stage, uint64_t ob, uint32_t tk) {
    const uint64_t gbeg = ob, gend = ob + tk;
    const uint64_t d0 = (gbeg + 3) >> 2, d1 = gend >> 2;  // whole output dwords [d0, d1)
    const uint32_t *st32 = reinterpret_cast<const uint32_t *>(stage);
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
    const uint64_t sbase = gbeg & ~(uint64_t)3;  // output address of stage[0]
    for (uint64_t d = d0 + threadIdx.x; d < d1; d += kFpBlock) out32[d] = st32[(d * 4 - sbase) >> 2];
    if (threadIdx.x == 0) {
        const uint64_t hend = std::min<uint64_t>(d0 * 4, gend);
        for (uint64_t g = gbeg; g < hend; ++g) out[g] = stage[g - sbase];
        const uint64_t tbeg = std::max<uint64_t>(d1 * 4, hend);
        for (uint64_t g = tbeg; g < gend; ++g) out[g] = stage[g - sbase];
    }
}

}  // namespace
}  // namespace kmc
