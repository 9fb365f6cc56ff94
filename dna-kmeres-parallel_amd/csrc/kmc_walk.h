// kmc_walk.h — the entry walk shared by the kernels that read per-record
// (key, count) lists (kmc_dist_sparse.hip, kmc_sketch.hip): workgroups walk
// contiguous entry ranges [e0, e1) of [0, num_entries); the record of an entry
// comes from one search of rec_offsets per range (range_window), then a search
// inside that window per entry (rec_of).
//
// Entries are only ever addressed by the walk's own index e < num_entries;
// rec_offsets values are clamped to num_entries and merely compared against, so
// whatever they hold, nothing is read at or beyond num_entries.  An entry no
// record claims (before rec_offsets[0], or at or after rec_offsets[n]) has record -1.
//
// P is the kernel's parameter struct; it provides
//   const uint64_t *rec_off;  int64_t E (num_entries), n (num_seqs).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kmc {
namespace {

// rec_offsets[s] clamped to the entry count; s in [0, n]
template <class P>
__device__ __forceinline__ int64_t off_c(const P &p, int64_t s) {
    const uint64_t v = p.rec_off[s];
    return v < (uint64_t)p.E ? (int64_t)v : p.E;
}

// largest s in [lo, hi] with off_c(s) <= e, lo - 1 if none (0 <= lo, hi <= n: any
// offsets, sorted or not, keep every read inside rec_offsets[0..n])
template <class P>
__device__ __forceinline__ int64_t find_rec(const P &p, int64_t e, int64_t lo, int64_t hi) {
    int64_t a = lo, b = hi + 1;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (off_c(p, m) <= e)
            a = m + 1;
        else
            b = m;
    }
    return a - 1;
}

// the record window of a workgroup's entry range, found once per range
template <class P>
__device__ __forceinline__ void range_window(const P &p, int64_t e0, int64_t e1, int64_t *win) {
    if (threadIdx.x == 0) {
        int64_t lo = 0, hi = 0;
        if (e0 < e1) {
            lo = find_rec(p, e0, 0, p.n);
            hi = find_rec(p, e1 - 1, 0, p.n);
            if (lo < 0) lo = 0;
            if (hi < lo) hi = lo;
        }
        win[0] = lo;
        win[1] = hi;
    }
}

// record of entry e, or -1 when no record claims it
template <class P>
__device__ __forceinline__ int64_t rec_of(const P &p, int64_t e, const int64_t *win) {
    const int64_t r = find_rec(p, e, win[0], win[1]);
    return (r >= 0 && r < p.n) ? r : -1;
}

}  // namespace
}  // namespace kmc
