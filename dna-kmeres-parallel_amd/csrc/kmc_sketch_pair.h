// kmc_sketch_pair.h — what the sketch distance kernels share (device code and the
// tile rule, no entry point): the counts of one pair of sketch rows, the Mash
// distance of those counts, and the capacity rule of a staged tile.  One
// definition for the packed triangle (kmc_sketch.hip), the query x reference
// rectangle and the top-hits search (kmc_sketch_query.hip), so that a pair has the
// same shared, denom and float wherever it is computed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kmc {
namespace {

// shipped / under -DKMC_DIAG_HOOKS (see kmc_sketch.hip)
#ifdef KMC_DIAG_HOOKS
constexpr int kDistElems = 512;  // LDS capacity of a distance tile, values
constexpr int kTileMax = 4;      // tile edge at most, rows
#else
constexpr int kDistElems = 16384;
constexpr int kTileMax = 32;
#endif
constexpr int kDistBlock = 1024;
constexpr int kStageMinTile = 4;  // a smaller staged tile leaves most of the 16 wavefronts idle
constexpr int kGlobalTile = 8;

// The edge of a square tile whose 2T rows of s values fit `elems` values of LDS, at
// most kTileMax; below kStageMinTile the rows stay in global memory (*stage =
// false) and the edge is kGlobalTile, for locality only.
inline int tile_edge(int elems, uint32_t s, bool *stage) {
    int T = elems / (int)s / 2;
    if (T > kTileMax) T = kTileMax;
    *stage = T >= kStageMinTile;
    if (!*stage) T = kGlobalTile < kTileMax ? kGlobalTile : kTileMax;
    return T;
}

__device__ __forceinline__ float mash_distance(uint32_t shared, uint32_t denom, int k) {
    if (denom == 0) return __uint_as_float(0x7fc00000u);
    if (shared == 0) return 1.0f;
    if (shared == denom) return 0.0f;
    const double j = (double)shared / (double)denom;
    double d = -log(2.0 * j / (1.0 + j)) / (double)k;
    if (d > 1.0) d = 1.0;
    return (float)d;
}

// One wavefront, one pair: A = row i (na values), B = row j (nb values), ascending.
template <class PA, class PB>
__device__ __forceinline__ void pair_counts(PA A, int na, PB B, int nb, int s, int lane, uint32_t *shared_out,
                                            uint32_t *denom_out) {
    const bool known = na == s || nb == s;  // the union holds at least s values
    int M = 0, sh = 0;
    for (int x0 = 0; x0 < na; x0 += 64) {
        const int x = x0 + lane;
        const bool act = x < na;
        int pos = 0;
        bool match = false;
        if (act) {
            const uint64_t v = A[x];
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (B[mid] < v)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            pos = lo;
            match = pos < nb && B[pos] == v;
        }
        const unsigned long long mm = __ballot(match);
        const int before = __popcll(mm & (~0ull >> (63 - lane)));  // matches among A[0..x]
        const int rank = x + 1 + pos + (match ? 1 : 0) - (M + before);
        const bool in_u = act && rank <= s;
        sh += __popcll(__ballot(match && in_u));
        M += __popcll(mm);
        if (known && __ballot(act && !in_u)) break;  // ranks only grow
    }
    const int uni = na + nb - M;  // |A u B| when the loop ran to its end
    *shared_out = (uint32_t)sh;
    *denom_out = (uint32_t)(known ? s : (uni < s ? uni : s));
}

}  // namespace
}  // namespace kmc
