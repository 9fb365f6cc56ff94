// kmc_sketch_accum.hip — the accumulating abundance sketcher: the bottom-s MinHash
// sketch of the k-mers seen at least min_count times over any number of batches (a
// read set of any size, Mash's -m).  It counts only the k-mers whose hash lies below a
// threshold, in a device hash table the handle owns; finish hands the counted keys to
// the select of kmc_sketch_from_counts.  Every device call is asynchronous with no
// host read-back; the launches depend on the host arguments and the handle's host
// state only.
//
// The handle's device memory (one allocation, each array rounded up to 256 bytes):
//   header  256 B        lost      the smallest hash of a refused insert (UINT64_MAX: none)
//                        tracked   entries of table 0 and of table 1
//                        rec_off   {0, the length of finish's list}: the offsets of the
//                                  one record kmc_sketch_from_counts selects from
//                        qual      list entries with count >= min_count
//                        spec      the spectrum's scratch: {entries, sum of counts}
//   keys    uint64[C] x 2   open addressing, linear probing, the slot of a key is the
//   counts  uint32[C] x 2   low log2_slots bits of its HASH; UINT64_MAX: empty (a
//                           canonical key has at most 62 bits)
//   select  the workspace of kmc_sketch_from_counts for one record
// One table is active (host state); the other is the purge's target and, between
// purges, the place of finish's list.
//
// The threshold is the host's: N = the bytes added so far, j the smallest integer with
// ceil(N / 2^j) <= C / 4, and a window takes part iff its hash is below 2^(64 - j) (one
// compare against a kernel argument; j = 0: every window).  N bounds the windows, so
// with a fixed hash the expected number of tracked keys stays at or below C / 4.
//
//   add     the walk of kmc_sketch_walk.h (for_each_piece of kmc_canon_walk.h, then
//           for_each_chunk with the identity functor, so a window keeps its key; the
//           launch shape and walk_of).  A window whose hash passes the threshold
//           probes from its slot: its key found, the count takes a vector atomic add
//           (no return value), once per run of equal keys among a thread's 16
//           windows (add_runs); an empty slot found, the thread reserves an entry (the one
//           returning atomic, on `tracked`, that only a new key pays) and inserts the
//           key with a 64-bit compare-and-swap; a slot that went to another thread
//           gives the reservation back.  A new key is refused when C / 2 entries are
//           reserved or the chain is kChain slots long: the refusal is one 64-bit
//           atomic minimum of its hash into `lost`, no retry, no spin.  So a table
//           never holds more than C / 2 keys, and more distinct keys than that below
//           the bound always leave a mark in `lost`; two threads that bring the same
//           new key when one entry is left may cost the second its window, which
//           `lost` then records like any other refusal.
//   purge   when an add raises j: the other table is cleared (memsets), every entry of
//           the active one whose hash is still below the bound is inserted there with
//           its count under the same chain bound (a failure goes to `lost` like any
//           other), and the tables swap roles.
//   compact finish: limit = min(2^(64 - j), lost); every entry with hash < limit (all
//           of them when j = 0 and nothing was lost) is appended to one (key, count)
//           list in the inactive table's arrays through a cursor; every key below
//           `limit` was tracked from its first window on, so its count is exact.
//   select  kmc_sketch_from_counts over that list as one record: num_entries is C (a
//           host number), the list's length is rec_off[1] on the device, and entries
//           no record claims are skipped by the walk (kmc_walk.h).  So the row is
//           bit for bit the count -> sketch path's, and the radix select, its sort
//           and the row format stay in kmc_sketch.hip.
//   stats   one thread writes the four words.
// finish writes the header's rec_off and qual, the inactive table and the select
// workspace only: the accumulator is as it was.
//
//   spectrum  kmc_spectrum_from_accum: the histogram of the counts of the entries
//           below the same `limit`, a uniform sample of the set's distinct k-mers with
//           exact multiplicities.  One pass over the active table: a workgroup bins
//           its slots in a private uint32 histogram in LDS (it sees C / 4096 <= 2^18
//           slots at most), then adds its non-zero bins to `hist` with 64-bit atomics
//           and its entry count and count sum to the header's `spec` words, once.  It
//           writes hist, stats and `spec` only.
//
//   match   kmc_match_from_accum: per record, how many of its windows are valid, how
//           many of those are sampled (all of them, or hash < the same `limit`) and how
//           many of those are in the active table with count >= min_count.  The table is
//           only read.  A lookup probes from hash & mask and ends at the first empty slot
//           or after kChain probes; that is exact, because insertion (add and purge
//           alike) never places a key further than that from its slot and past no empty
//           slot, and nothing is ever deleted from a table in place: a key that is in the
//           table is found, and a key below `limit` that was added is in the table.
//           The unit that owns a record piece is a WAVE (for_each_wave_piece and
//           for_each_wave_chunk of kmc_sketch_walk.h): the call's chunk range is cut
//           into G * kBlock / 64 ranges, a round is 64 chunks, and a piece ends with a
//           wave reduction of three popcounts, no barrier and no LDS.  The outputs are
//           cleared on the stream first; the wave's first lane stores a record's three
//           numbers when the record lies wholly in its range and adds them with vector
//           atomics when the record is cut between waves.  Equal neighbouring keys among
//           a lane's sampled windows are one probe (add_runs' rule), and stats[2..3]
//           take one 64-bit add per wave.
//
//   label   kmc_label_accum: which source holds a key, a uint32 bitmask per slot
//           of the active table in a second allocation of 4 C bytes that the first
//           label call makes.  The walk is add's (for_each_piece, for_each_chunk); a
//           sampled window (all, or hash < the same `limit`) is looked up with match's
//           probe (table_slot) and its slot's label takes a vector atomic OR of the
//           source's bit, once per run of equal keys.  The tables and the header are
//           only read.  Whether the labels describe the table is host state: an add of
//           records and a reset drop them, and the next label call clears the array on
//           its stream first.
//
//   classify  kmc_classify_from_accum: match's wave walk, and per record the number of
//           hit windows whose label has bit g, for every source g, with the best source,
//           its score and the runner-up's.  A lane adds the labels of its chunk's hit
//           windows into five bit planes (16 windows: counts of 0 .. 16 per source), and
//           once per chunk adds the count of every source it saw to its wave's score row
//           in LDS (32 words per wave, LDS atomics).  A piece ends with the wave's lanes
//           0 .. 31 taking the row back (and zeroing it) and a wave-wide argmax; no
//           barrier: the waves of a workgroup stay independent.  A record that lies
//           wholly in the wave's range is stored; at most two pieces of a range are not
//           whole records, its first (cut at the start) and its last (cut at the end),
//           and their rows go to the workspace: two rows per wave of the launch, each
//           tagged with its record, the tags invalidated on the stream before the walk.
//           A record's first piece is always a range's last one, so the fix-up kernel
//           (classify_cut_kernel) has one workgroup per wave whose last row is tagged:
//           it adds the first rows of the following waves with the same tag, 32 lanes a
//           row, until a row of another record shows, and writes the record's results.
//           A piece with no hit skips the votes and the fold; best, best_hits, next_hits
//           and scores are cleared to "none" on the stream first, as match's outputs are.
//
// The device code trusts the host arguments only: every slot index is masked, every
// chain is bounded by kChain <= C, the list's cursor is checked against C.
//
// Constants (the same in libkmc_diag.so, whose walk has 64-thread workgroups and
// 256-byte ranges through kmc_sketch_walk.h; the tests force the table's paths with
// log2_slots = 4 .. 8):
//   kChain         probes of one key at most           256 (C when smaller)
//   kDefaultPer    slots per sketch value, at least    4096 (log2_slots = 0)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "kmc.h"
#include "kmc_canon_walk.h"
#include "kmc_internal.h"
#include "kmc_sketch_pair.h"
#include "kmc_sketch_walk.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

constexpr uint32_t kChain = 256;
constexpr uint64_t kDefaultPer = KMC_SKETCH_ACCUM_DEFAULT_SLOTS_PER_VALUE;
constexpr size_t kHeaderBytes = 256;
constexpr int kSlotBlock = 256;  // threads of the kernels that walk the slots

struct Header {
    unsigned long long lost;
    uint32_t tracked[2];
    unsigned long long rec_off[2];
    unsigned long long qual;
    unsigned long long spec[2];
};
static_assert(sizeof(Header) <= kHeaderBytes, "the header has its 256 bytes");

struct ALayout {
    Header *hd;
    unsigned long long *keys[2];
    uint32_t *counts[2];
    void *select;
    size_t select_bytes, bytes;
};

inline bool log2_slots_ok(uint32_t lg) {
    return lg == 0 || (lg >= KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS && lg <= KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS);
}

// log2_slots = 0: the power of two at or above kDefaultPer * sketch_size
inline uint32_t resolve_log2(uint32_t sketch_size, uint32_t lg) {
    if (lg) return lg;
    lg = KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS;
    while ((1ull << lg) < kDefaultPer * sketch_size) ++lg;
    return lg;  // <= 26 for KMC_SKETCH_MAX_SIZE
}

// the one layout behind the size query (base = null) and create
inline ALayout layout(void *base, uint32_t sketch_size, uint32_t lg) {
    const uint64_t C = 1ull << lg;
    Carver c(base);
    ALayout L;
    L.hd = reinterpret_cast<Header *>(c.take<char>(kHeaderBytes));
    for (int t = 0; t < 2; ++t) {
        L.keys[t] = c.take<unsigned long long>((size_t)C);
        L.counts[t] = c.take<uint32_t>((size_t)C);
    }
    L.select_bytes = kmc_sketch_workspace_size(1, C, sketch_size, 0);  // (host numbers only)
    L.select = c.take<char>(L.select_bytes);
    L.bytes = c.total();
    return L;
}

// The smallest j >= 0 with ceil(N / 2^j) <= C / 4.
inline uint32_t level_of(uint64_t N, uint32_t lg) {
    const uint64_t quarter = 1ull << (lg - 2);
    uint32_t j = 0;
    while (((N + ((1ull << j) - 1)) >> j) > quarter) ++j;
    return j;  // N < 2^62, quarter >= 4: j <= 60
}

// the largest hash that takes part at level j: 2^(64 - j) - 1
inline uint64_t max_hash(uint32_t j) { return j == 0 ? ~0ull : (1ull << (64 - j)) - 1ull; }

// One table as a kernel sees it, all from the host.
struct Table {
    unsigned long long *keys;
    uint32_t *counts;
    uint32_t *tracked;
    unsigned long long *lost;
    uint32_t mask, chain, half;
};

// Where the count of `key` (hash h) is kept, inserting the key when it is new; null:
// refused, and h has gone to `lost`.  CAP: new keys are refused at T.half tracked.
template <bool CAP>
__device__ __forceinline__ uint32_t *find_or_insert(const Table &T, unsigned long long key, unsigned long long h) {
    uint32_t i = (uint32_t)h & T.mask;
    for (uint32_t step = 0; step < T.chain; ++step) {
        // (a stale empty reading only costs the compare-and-swap; a key never changes)
        const unsigned long long x = __hip_atomic_load(T.keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (x == key) return T.counts + i;
        if (x == kFill) {
            // the entry is reserved before the slot is taken (the purge only counts)
            const uint32_t had = __hip_atomic_fetch_add(T.tracked, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (CAP && had >= T.half) {
                __hip_atomic_fetch_sub(T.tracked, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            const unsigned long long was = atomicCAS(T.keys + i, (unsigned long long)kFill, key);
            if (was == kFill) return T.counts + i;
            __hip_atomic_fetch_sub(T.tracked, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // another thread's slot
            if (was == key) return T.counts + i;
        }
        i = (i + 1) & T.mask;
    }
    __hip_atomic_fetch_min(T.lost, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return nullptr;
}

// ---------------------------------------------------------------------------
// add
// ---------------------------------------------------------------------------
using Walk = WalkOf<Offsets>;

struct KeyOf {  // a window keeps its key: the slot needs the hash, the table the key
    __device__ __forceinline__ unsigned long long operator()(uint64_t key) const { return key; }
};

struct AArgs {
    WalkArgs w;
    uint64_t seed;
    uint64_t maxh;  // hashes above it leave
    Table T;
};

template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kBlock) void accum_add_kernel(AArgs a) {
    __shared__ int64_t s_first;
    const Walk W = walk_of(a.w);
    for_each_piece(W, &s_first, [&](int64_t, int64_t ps, int64_t pe, int64_t rend) {
        for_each_chunk<FWD, BIGK>(W, ps, pe, rend, KeyOf{}, [&](const unsigned long long(&key)[16], uint32_t pend) {
            uint32_t cm = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) cm |= (uint32_t)(sketch_hash(key[j], a.seed) <= a.maxh) << j;
            pend &= cm;
            if (pend)
                add_runs(key, pend, [&](unsigned long long v) {
                    return find_or_insert<true>(a.T, v, sketch_hash(v, a.seed));
                });
        });
    });
}

// ---------------------------------------------------------------------------
// purge, compact, stats
// ---------------------------------------------------------------------------
struct PArgs {
    const unsigned long long *keys;  // the table that is left, C slots
    const uint32_t *counts;
    uint64_t C, seed, maxh;
    Table T;  // the cleared table
};

__global__ __launch_bounds__(kSlotBlock) void accum_purge_kernel(PArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * kSlotBlock + threadIdx.x; i < a.C; i += (uint64_t)gridDim.x * kSlotBlock) {
        const unsigned long long key = a.keys[i];
        if (key == kFill) continue;
        const unsigned long long h = sketch_hash(key, a.seed);
        if (h > a.maxh) continue;
        uint32_t *at = find_or_insert<false>(a.T, key, h);
        if (at) __hip_atomic_fetch_add(at, a.counts[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct FArgs {
    const unsigned long long *keys;  // the active table, C slots
    const uint32_t *counts;
    uint64_t C, seed, maxh;
    uint32_t j, min_count, s;
    Header *hd;
    unsigned long long *list_keys;  // [C]
    uint32_t *list_counts;
    const uint32_t *size_out;
    uint64_t *stats;
};

// the exclusive bound of the hashes whose counts are exact; *all: nothing bounds them
template <class Args>
__device__ __forceinline__ unsigned long long limit_of(const Args &a, bool *all) {
    const unsigned long long lost = a.hd->lost;
    *all = a.j == 0 && lost == kFill;
    if (a.j == 0) return lost;
    const unsigned long long bound = a.maxh + 1ull;
    return lost < bound ? lost : bound;
}

__global__ __launch_bounds__(kSlotBlock) void accum_compact_kernel(FArgs a) {
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    const uint32_t m = a.min_count > 1 ? a.min_count : 1u;
    for (uint64_t i = (uint64_t)blockIdx.x * kSlotBlock + threadIdx.x; i < a.C; i += (uint64_t)gridDim.x * kSlotBlock) {
        const unsigned long long key = a.keys[i];
        if (key == kFill) continue;
        if (!all && sketch_hash(key, a.seed) >= limit) continue;
        const uint32_t cnt = a.counts[i];
        const unsigned long long at = atomicAdd(&a.hd->rec_off[1], 1ull);
        if (at < a.C) {  // (guard: at most C slots hold a key)
            a.list_keys[at] = key;
            a.list_counts[at] = cnt;
        }
        if (cnt >= m) atomicAdd(&a.hd->qual, 1ull);
    }
}

__global__ void accum_stats_kernel(FArgs a) {
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    a.stats[0] = (all || *a.size_out == a.s) ? 1u : 0u;
    a.stats[1] = limit;
    a.stats[2] = a.hd->rec_off[1];
    a.stats[3] = a.hd->qual;
}

// ---------------------------------------------------------------------------
// spectrum
// ---------------------------------------------------------------------------
struct SArgs {
    const unsigned long long *keys;  // the active table, C slots
    const uint32_t *counts;
    uint64_t C, seed, maxh;
    uint32_t j, bins;  // bins in 2 .. KMC_SPECTRUM_MAX_BINS
    Header *hd;
    unsigned long long *hist;  // [bins], cleared
    uint64_t *stats;
};

__global__ __launch_bounds__(kSlotBlock) void accum_spectrum_kernel(SArgs a) {
    extern __shared__ uint32_t s_hist[];  // [bins]
    __shared__ unsigned long long s_sum[2];
    const uint32_t tid = threadIdx.x, top = a.bins - 1u;
    for (uint32_t b = tid; b < a.bins; b += kSlotBlock) s_hist[b] = 0u;
    if (tid < 2) s_sum[tid] = 0ull;
    __syncthreads();
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    unsigned long long n = 0ull, sum = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * kSlotBlock + tid; i < a.C; i += (uint64_t)gridDim.x * kSlotBlock) {
        const unsigned long long key = a.keys[i];
        if (key == kFill) continue;
        if (!all && sketch_hash(key, a.seed) >= limit) continue;
        const uint32_t cnt = a.counts[i];
        atomicAdd(&s_hist[cnt < top ? cnt : top], 1u);
        ++n;
        sum += cnt;
    }
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        n += __shfl_down(n, off);
        sum += __shfl_down(sum, off);
    }
    if ((tid & (warpSize - 1)) == 0 && n) {
        atomicAdd(&s_sum[0], n);
        atomicAdd(&s_sum[1], sum);
    }
    __syncthreads();
    for (uint32_t b = tid; b < a.bins; b += kSlotBlock) {
        const uint32_t v = s_hist[b];
        if (v) atomicAdd(a.hist + b, (unsigned long long)v);
    }
    if (tid == 0 && s_sum[0]) {
        atomicAdd(&a.hd->spec[0], s_sum[0]);
        atomicAdd(&a.hd->spec[1], s_sum[1]);
    }
}

__global__ void accum_spectrum_stats_kernel(SArgs a) {
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    a.stats[0] = all ? 1u : 0u;
    a.stats[1] = limit;
    a.stats[2] = a.hd->spec[0];
    a.stats[3] = a.hd->spec[1];
}

// ---------------------------------------------------------------------------
// match
// ---------------------------------------------------------------------------
struct MArgs {
    WalkArgs w;
    uint64_t seed, maxh;
    uint32_t j, min_count;
    const Header *hd;
    const unsigned long long *keys;  // the active table
    const uint32_t *counts;
    uint32_t mask, chain;
    uint32_t *windows, *sampled, *hits;  // [n], cleared; windows and sampled may be null
    unsigned long long *stats;           // [4] or null; [2] and [3] cleared
};

// whether the table holds `key` (hash h) with a count of at least m: the chain from the
// key's slot to the first empty slot, kChain probes at most
__device__ __forceinline__ bool table_has(const MArgs &a, unsigned long long key, unsigned long long h, uint32_t m) {
    uint32_t i = (uint32_t)h & a.mask;
    for (uint32_t step = 0; step < a.chain; ++step) {
        const unsigned long long x = a.keys[i];
        if (x == key) return a.counts[i] >= m;
        if (x == kFill) return false;
        i = (i + 1) & a.mask;
    }
    return false;
}

// one record's word: no other wave has a piece of the record (a plain store over the
// cleared word), or a relaxed agent-scope add
__device__ __forceinline__ void credit(uint32_t *out, int64_t r, uint32_t v, bool whole) {
    if (!out) return;
    if (whole) out[r] = v;
    else if (v) __hip_atomic_fetch_add(out + r, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kBlock) void accum_match_kernel(MArgs a) {
    const Walk W = wave_walk_of(a.w);
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    const uint32_t m = a.min_count > 1 ? a.min_count : 1u;
    const bool first = (threadIdx.x & (kWave - 1)) == 0;
    unsigned long long tot_s = 0ull, tot_h = 0ull;  // this lane's share of the wave's sums
    for_each_wave_piece(W, [&](int64_t r, int64_t ps, int64_t pe, int64_t rend, bool whole) {
        uint32_t nv = 0u, ns = 0u, nh = 0u;
        for_each_wave_chunk<FWD, BIGK>(W, ps, pe, rend, KeyOf{}, [&](const unsigned long long(&key)[16], uint32_t pend) {
            if (!pend) return;
            uint32_t sm = pend;
            if (!all) {
                uint32_t cm = 0u;
#pragma unroll
                for (int j = 0; j < 16; ++j) cm |= (uint32_t)(sketch_hash(key[j], a.seed) < limit) << j;
                sm &= cm;
            }
            // the sampled windows that are hits: equal neighbours are one run, one probe
            uint32_t hm = 0u;
            unsigned long long last = 0ull;
            bool run = false, hit = false;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (!((sm >> j) & 1u)) continue;
                if (!(run && key[j] == last)) {
                    last = key[j];
                    hit = table_has(a, last, sketch_hash(last, a.seed), m);
                    run = true;
                }
                hm |= (uint32_t)hit << j;
            }
            nv += __popc(pend);
            ns += __popc(sm);
            nh += __popc(hm);
        });
        tot_s += ns;
        tot_h += nh;
        const uint32_t v = a.windows ? wave_sum(nv) : 0u, s = a.sampled ? wave_sum(ns) : 0u, h = wave_sum(nh);
        if (first) {
            credit(a.windows, r, v, whole);
            credit(a.sampled, r, s, whole);
            credit(a.hits, r, h, whole);
        }
    });
    if (a.stats) {  // one add per wave and word
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            tot_s += __shfl_xor(tot_s, off, kWave);
            tot_h += __shfl_xor(tot_h, off, kWave);
        }
        if (first && tot_s) atomicAdd(a.stats + 2, tot_s);
        if (first && tot_h) atomicAdd(a.stats + 3, tot_h);
    }
}

// stats of a match before its walk: {all, limit, 0, 0}
__global__ void accum_match_stats_kernel(MArgs a) {
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    a.stats[0] = all ? 1u : 0u;
    a.stats[1] = limit;
    a.stats[2] = 0ull;
    a.stats[3] = 0ull;
}

// ---------------------------------------------------------------------------
// label
// ---------------------------------------------------------------------------
constexpr uint32_t kNoSlot = ~0u;
constexpr int kSources = KMC_CLASSIFY_MAX_SOURCES;
static_assert(kSources == 32 && kSources <= kWave, "a label is one word, a score row half a wave");

// the slot of `key` (hash h) in a table, by table_has' chain: from the key's slot to the
// first empty slot, `chain` probes at most; kNoSlot: the table does not hold it
__device__ __forceinline__ uint32_t table_slot(const unsigned long long *keys, uint32_t mask, uint32_t chain,
                                               unsigned long long key, unsigned long long h) {
    uint32_t i = (uint32_t)h & mask;
    for (uint32_t step = 0; step < chain; ++step) {
        const unsigned long long x = keys[i];
        if (x == key) return i;
        if (x == kFill) return kNoSlot;
        i = (i + 1) & mask;
    }
    return kNoSlot;
}

// the windows of `pend` whose hash is below `limit`
__device__ __forceinline__ uint32_t sampled_of(const unsigned long long (&key)[16], uint32_t pend, uint64_t seed,
                                               unsigned long long limit) {
    uint32_t cm = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) cm |= (uint32_t)(sketch_hash(key[j], seed) < limit) << j;
    return pend & cm;
}

struct LArgs {
    WalkArgs w;
    uint64_t seed, maxh;
    uint32_t j, bit;  // bit: 1 << source
    const Header *hd;
    const unsigned long long *keys;  // the active table: only read
    uint32_t mask, chain;
    uint32_t *labels;  // [C]
};

template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kBlock) void accum_label_kernel(LArgs a) {
    __shared__ int64_t s_first;
    const Walk W = walk_of(a.w);
    bool all;
    const unsigned long long limit = limit_of(a, &all);
    for_each_piece(W, &s_first, [&](int64_t, int64_t ps, int64_t pe, int64_t rend) {
        for_each_chunk<FWD, BIGK>(W, ps, pe, rend, KeyOf{}, [&](const unsigned long long(&key)[16], uint32_t pend) {
            if (!pend) return;
            const uint32_t sm = all ? pend : sampled_of(key, pend, a.seed, limit);
            unsigned long long last = 0ull;
            bool run = false;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (!((sm >> j) & 1u)) continue;
                if (run && key[j] == last) continue;  // equal neighbours: one probe, one OR
                last = key[j];
                run = true;
                const uint32_t at = table_slot(a.keys, a.mask, a.chain, last, sketch_hash(last, a.seed));
                // (a stale reading of a word that has the bit only costs the atomic)
                if (at != kNoSlot && !(a.labels[at] & a.bit))
                    __hip_atomic_fetch_or(a.labels + at, a.bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        });
    });
}

// ---------------------------------------------------------------------------
// classify
// ---------------------------------------------------------------------------
#ifdef KMC_DIAG_HOOKS
constexpr int kCutBlock = 64;  // two rows a round: a cut record takes several rounds
#else
constexpr int kCutBlock = 1024;
#endif
constexpr int kCutRows = kCutBlock / kSources;  // workspace rows a round of the fix-up reads

struct CArgs {
    MArgs m;
    const uint32_t *labels;  // [C]
    uint32_t ns, srcmask;    // the sources 1 .. 32 and the label bits below ns
    uint32_t *best, *best_hits, *next_hits;  // [n], cleared to none
    uint32_t *scores;                        // [n * ns], cleared, or null
    // the pieces that are no whole record: row 2 u is wave u's first piece (its record
    // began before the range), row 2 u + 1 its last (its record goes on after it)
    long long *tags;  // [2 * waves] the row's record; negative: no row
    uint32_t *rows;   // [2 * waves][kSources]
    int64_t waves;
};

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x = std::max(x, (uint32_t)__shfl_xor(x, off, kWave));
    return x;
}

// Record r's results from its score row: v is score(r, lane), 0 in the lanes at or above
// ns.  All 64 lanes of a wave call it.
__device__ __forceinline__ void store_votes(const CArgs &a, int64_t r, uint32_t v, int lane) {
    const uint32_t mx = wave_max(v);
    const int b = __ffsll((unsigned long long)__ballot(v == mx)) - 1;  // the smallest source with the largest score
    const uint32_t nx = wave_max(lane == b ? 0u : v);
    if (a.scores && lane < (int)a.ns) a.scores[(uint64_t)r * a.ns + lane] = v;
    if (lane == 0) {
        a.best[r] = mx ? (uint32_t)b : KMC_CLASSIFY_NONE;
        a.best_hits[r] = mx;
        a.next_hits[r] = nx;  // (mx == 0: every score is 0)
    }
}

template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kBlock) void accum_classify_kernel(CArgs a) {
    __shared__ uint32_t s_row[kWavesPerBlock][kSources];  // a wave's score row; no other wave touches it
    const MArgs &g = a.m;
    const Walk W = wave_walk_of(g.w);
    bool all;
    const unsigned long long limit = limit_of(g, &all);
    const uint32_t m = g.min_count > 1 ? g.min_count : 1u;
    const int lane = threadIdx.x & (kWave - 1);
    const bool first = lane == 0;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    uint32_t *row = s_row[wv];
    if (lane < kSources) __hip_atomic_store(row + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    unsigned long long tot_s = 0ull, tot_h = 0ull;
    for_each_wave_piece(W, [&](int64_t r, int64_t ps, int64_t pe, int64_t rend, bool whole) {
        uint32_t nv = 0u, ns = 0u, nh = 0u;
        for_each_wave_chunk<FWD, BIGK>(W, ps, pe, rend, KeyOf{}, [&](const unsigned long long(&key)[16], uint32_t pend) {
            if (!pend) return;
            const uint32_t sm = all ? pend : sampled_of(key, pend, g.seed, limit);
            // match's runs; a hit window adds its label to the lane's bit planes: plane p
            // holds bit p of the count of every source among the chunk's 16 windows
            uint32_t hm = 0u, lab = 0u, c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, c4 = 0u;
            unsigned long long last = 0ull;
            bool run = false, hit = false;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (!((sm >> j) & 1u)) continue;
                if (!(run && key[j] == last)) {
                    last = key[j];
                    const uint32_t at = table_slot(g.keys, g.mask, g.chain, last, sketch_hash(last, g.seed));
                    hit = at != kNoSlot && g.counts[at] >= m;
                    lab = hit ? a.labels[at] & a.srcmask : 0u;
                    run = true;
                }
                hm |= (uint32_t)hit << j;
                uint32_t carry = lab, t;
                t = c0 & carry; c0 ^= carry; carry = t;
                t = c1 & carry; c1 ^= carry; carry = t;
                t = c2 & carry; c2 ^= carry; carry = t;
                t = c3 & carry; c3 ^= carry; carry = t;
                c4 ^= carry;
            }
            nv += __popc(pend);
            ns += __popc(sm);
            nh += __popc(hm);
            for (uint32_t seen = c0 | c1 | c2 | c3 | c4; seen; seen &= seen - 1u) {  // the sources this lane saw
                const int s = __ffs(seen) - 1;
                const uint32_t cnt = ((c0 >> s) & 1u) | (((c1 >> s) & 1u) << 1) | (((c2 >> s) & 1u) << 2) |
                                     (((c3 >> s) & 1u) << 3) | (((c4 >> s) & 1u) << 4);
                __hip_atomic_fetch_add(row + s, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        });
        tot_s += ns;
        tot_h += nh;
        const uint32_t v = g.windows ? wave_sum(nv) : 0u, s = g.sampled ? wave_sum(ns) : 0u, h = wave_sum(nh);
        if (first) {
            credit(g.windows, r, v, whole);
            credit(g.sampled, r, s, whole);
            credit(g.hits, r, h, whole);
        }
        if (whole && h == 0u) return;  // no vote: the cleared outputs stand
        // the wave's row, taken back by its own lanes (a wave's LDS operations keep their order)
        uint32_t score = 0u;
        if (h) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (lane < kSources) {
                score = __hip_atomic_load(row + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_store(row + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        if (whole) {
            store_votes(a, r, score, lane);
        } else {
            const int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // < a.waves
            const int64_t at = 2 * u + (ps > W.idx[r] ? 0 : 1);
            if (lane < kSources) a.rows[at * kSources + lane] = score;
            if (first) a.tags[at] = (long long)r;
        }
    });
    if (g.stats) {  // one add per wave and word
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            tot_s += __shfl_xor(tot_s, off, kWave);
            tot_h += __shfl_xor(tot_h, off, kWave);
        }
        if (first && tot_s) atomicAdd(g.stats + 2, tot_s);
        if (first && tot_h) atomicAdd(g.stats + 3, tot_h);
    }
}

// The cut records.  A record's first piece is the last piece of its wave (tag 2 u + 1);
// its other pieces are the first pieces of the waves after it (tags 2 w, w > u), with
// nothing but rowless waves in between, and the first row of another record ends them.
// One workgroup per tagged last row: kCutRows rows a round, kSources lanes a row.
__global__ __launch_bounds__(kCutBlock) void classify_cut_kernel(CArgs a) {
    __shared__ uint32_t s_tot[kSources];
    const int tid = threadIdx.x, src = tid & (kSources - 1), q = tid / kSources;
    for (int64_t u = blockIdx.x; u < a.waves; u += gridDim.x) {
        const long long r = a.tags[2 * u + 1];
        if (r < 0 || r >= a.m.w.n) continue;  // (workgroup-uniform, before this round's barriers)
        if (tid < kSources) s_tot[tid] = a.rows[(2 * u + 1) * kSources + tid];
        __syncthreads();
        uint32_t mine = 0u;
        for (int64_t b = u + 1; b < a.waves; b += kCutRows) {
            const int64_t w = b + q;
            const long long t = w < a.waves ? a.tags[2 * w] : -1ll;
            if (t == r) mine += a.rows[2 * w * kSources + src];
            if (__syncthreads_or(t >= 0 && t != r)) break;
        }
        if (mine) atomicAdd(&s_tot[src], mine);
        __syncthreads();
        if (tid < kWave) store_votes(a, r, tid < kSources ? s_tot[tid] : 0u, tid);
        __syncthreads();  // before the next round's totals
    }
}

struct CLayout {
    long long *tags;
    uint32_t *rows;
    size_t bytes;
};

// two rows per wave of a launch of G workgroups
inline CLayout classify_layout(void *base, int G) {
    const size_t rows = 2 * (size_t)G * kWavesPerBlock;
    Carver c(base);
    CLayout l;
    l.tags = c.take<long long>(rows);
    l.rows = c.take<uint32_t>(rows * kSources);
    l.bytes = c.total();
    return l;
}

DeviceCache classify_ws;

inline unsigned slot_grid(uint64_t C) {
    const uint64_t b = (C + kSlotBlock - 1) / kSlotBlock;
    return (unsigned)(b < 4096 ? b : 4096);
}

}  // namespace
}  // namespace kmc

using namespace kmc;

struct kmc_sketch_accum {
    uint32_t s, lg;
    int k;
    unsigned flags;
    uint64_t seed;
    void *base;
    ALayout L;
    // what the adds so far have made of the table
    uint64_t N;  // bytes added
    uint32_t j;  // the threshold's level: it never falls
    int active;  // the table the adds go to
    // the sources of the active table's keys (kmc_label_accum)
    uint32_t *labels;  // [C], a second allocation made by the first label call; null before it
    bool labelled;     // the labels describe the table as it stands
};

namespace {

Table table_of(const kmc_sketch_accum *a, int t) {
    const uint64_t C = 1ull << a->lg;
    Table T;
    T.keys = a->L.keys[t];
    T.counts = a->L.counts[t];
    T.tracked = &a->L.hd->tracked[t];
    T.lost = &a->L.hd->lost;
    T.mask = (uint32_t)(C - 1);
    T.chain = C < kChain ? (uint32_t)C : kChain;
    T.half = (uint32_t)(C / 2);
    return T;
}

// table t empty, with no tracked entry
int clear_table(const kmc_sketch_accum *a, int t, hipStream_t st) {
    const size_t C = (size_t)1 << a->lg;
    if (hipError_t he = hipMemsetAsync(a->L.keys[t], 0xFF, C * 8, st)) return (int)he;
    if (hipError_t he = hipMemsetAsync(a->L.counts[t], 0, C * 4, st)) return (int)he;
    return (int)hipMemsetAsync(&a->L.hd->tracked[t], 0, 4, st);
}

// the state after create: table 0 empty and active, nothing lost, N = 0, j = 0
int start_over(kmc_sketch_accum *a, hipStream_t st) {
    if (hipError_t he = hipMemsetAsync(a->L.hd, 0, kHeaderBytes, st)) return (int)he;
    if (hipError_t he = hipMemsetAsync(&a->L.hd->lost, 0xFF, 8, st)) return (int)he;
    if (int e = clear_table(a, 0, st)) return e;
    a->N = 0;
    a->j = 0;
    a->active = 0;
    a->labelled = false;
    return KMC_OK;
}

}  // namespace

extern "C" size_t kmc_sketch_accum_device_bytes(uint32_t sketch_size, uint32_t log2_slots) {
    if (!sketch_size_ok(sketch_size) || !log2_slots_ok(log2_slots)) return 0;
    return layout(nullptr, sketch_size, resolve_log2(sketch_size, log2_slots)).bytes;
}

extern "C" int kmc_sketch_accum_create(uint32_t sketch_size, int k, unsigned flags, uint64_t seed, uint32_t log2_slots,
                                       kmc_sketch_accum **out) {
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (!sketch_size_ok(sketch_size) || !log2_slots_ok(log2_slots) || !out) return KMC_ERR_INVALID_ARG;
    if (!walk_flags_ok(flags)) return KMC_ERR_INVALID_ARG;
    *out = nullptr;
    kmc_sketch_accum *a = new (std::nothrow) kmc_sketch_accum();
    if (!a) return KMC_ERR_NOMEM;
    a->s = sketch_size;
    a->lg = resolve_log2(sketch_size, log2_slots);
    a->k = k;
    a->flags = flags;
    a->seed = seed;
    a->base = nullptr;
    a->labels = nullptr;
    a->labelled = false;
    if (hipMalloc(&a->base, layout(nullptr, a->s, a->lg).bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete a;
        return KMC_ERR_NOMEM;
    }
    a->L = layout(a->base, a->s, a->lg);
    int e = start_over(a, nullptr);
    if (!e) e = (int)hipStreamSynchronize(nullptr);  // the clearing is done before any stream's first add
    if (e) {
        kmc_sketch_accum_free(a);
        return e;
    }
    *out = a;
    return KMC_OK;
}

extern "C" int kmc_sketch_accum_add(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                    uint64_t data_bytes, hipStream_t stream) {
    if (!a || num_seqs > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (num_seqs == 0) return KMC_OK;
    if (!walk_ptrs_ok(data, indices, data_bytes)) return KMC_ERR_INVALID_ARG;
    if (!walk_sizes_ok(num_seqs, data_bytes) || a->N + data_bytes >= (1ull << 62)) return KMC_ERR_INVALID_ARG;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const uint64_t C = 1ull << a->lg, N = a->N + data_bytes;
    const uint32_t j = level_of(N, a->lg);
    if (j > a->j) {  // purge: what stays below the new bound moves to the other table
        const int from = a->active, to = from ^ 1;
        if (int e = clear_table(a, to, stream)) return e;
        PArgs p;
        p.keys = a->L.keys[from];
        p.counts = a->L.counts[from];
        p.C = C;
        p.seed = a->seed;
        p.maxh = max_hash(j);
        p.T = table_of(a, to);
        hipLaunchKernelGGL(accum_purge_kernel, dim3(slot_grid(C)), dim3(kSlotBlock), 0, stream, p);
        if (hipError_t he = hipGetLastError()) return (int)he;
        a->j = j;
        a->active = to;
    }
    const AArgs g{walk_args(data, indices, num_seqs, data_bytes, a->k, a->flags, cus), a->seed, max_hash(a->j),
                  table_of(a, a->active)};
    for_walk(a->flags, a->k, [&](auto fwd, auto big) {
        hipLaunchKernelGGL((accum_add_kernel<decltype(fwd)::value, decltype(big)::value>), dim3((unsigned)g.w.G),
                           dim3(kBlock), 0, stream, g);
    });
    if (hipError_t he = hipGetLastError()) return (int)he;
    a->N = N;
    a->labelled = false;  // the labels described the table before these records
    return KMC_OK;
}

extern "C" int kmc_sketch_accum_finish(kmc_sketch_accum *a, uint32_t min_count, uint64_t *sketch_row,
                                       uint32_t *sketch_size_out, uint64_t *stats, hipStream_t stream) {
    if (!a || !sketch_row || !sketch_size_out) return KMC_ERR_INVALID_ARG;
    const uint64_t C = 1ull << a->lg;
    const int list = a->active ^ 1;  // cleared by the next purge before it is a table again
    FArgs f;
    f.keys = a->L.keys[a->active];
    f.counts = a->L.counts[a->active];
    f.C = C;
    f.seed = a->seed;
    f.maxh = max_hash(a->j);
    f.j = a->j;
    f.min_count = min_count;
    f.s = a->s;
    f.hd = a->L.hd;
    f.list_keys = a->L.keys[list];
    f.list_counts = a->L.counts[list];
    f.size_out = sketch_size_out;
    f.stats = stats;
    if (hipError_t he = hipMemsetAsync(a->L.hd->rec_off, 0, sizeof(a->L.hd->rec_off) + sizeof(a->L.hd->qual), stream))
        return (int)he;
    hipLaunchKernelGGL(accum_compact_kernel, dim3(slot_grid(C)), dim3(kSlotBlock), 0, stream, f);
    if (hipError_t he = hipGetLastError()) return (int)he;
    // the list as the one record of the count -> sketch path: C entries to walk, of
    // which the device's rec_off claims the first rec_off[1]
    if (int e = kmc_sketch_from_counts(reinterpret_cast<const uint64_t *>(f.list_keys), f.list_counts,
                                       reinterpret_cast<const uint64_t *>(a->L.hd->rec_off), C, 1, a->s, a->seed,
                                       min_count, sketch_row, sketch_size_out, a->L.select, a->L.select_bytes, stream))
        return e;
    if (stats) hipLaunchKernelGGL(accum_stats_kernel, dim3(1), dim3(1), 0, stream, f);
    return (int)hipGetLastError();
}

extern "C" int kmc_spectrum_from_accum(kmc_sketch_accum *a, uint32_t num_bins, uint64_t *hist, uint64_t *stats,
                                       hipStream_t stream) {
    if (!a || !hist || num_bins < 2 || num_bins > KMC_SPECTRUM_MAX_BINS) return KMC_ERR_INVALID_ARG;
    const uint64_t C = 1ull << a->lg;
    SArgs g;
    g.keys = a->L.keys[a->active];
    g.counts = a->L.counts[a->active];
    g.C = C;
    g.seed = a->seed;
    g.maxh = max_hash(a->j);
    g.j = a->j;
    g.bins = num_bins;
    g.hd = a->L.hd;
    g.hist = reinterpret_cast<unsigned long long *>(hist);
    g.stats = stats;
    if (hipError_t he = hipMemsetAsync(hist, 0, (size_t)num_bins * 8, stream)) return (int)he;
    if (hipError_t he = hipMemsetAsync(a->L.hd->spec, 0, sizeof(a->L.hd->spec), stream)) return (int)he;
    hipLaunchKernelGGL(accum_spectrum_kernel, dim3(slot_grid(C)), dim3(kSlotBlock), (size_t)num_bins * 4, stream, g);
    if (hipError_t he = hipGetLastError()) return (int)he;
    if (stats) hipLaunchKernelGGL(accum_spectrum_stats_kernel, dim3(1), dim3(1), 0, stream, g);
    return (int)hipGetLastError();
}

extern "C" int kmc_match_from_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                    uint64_t data_bytes, uint32_t min_count, uint32_t *windows, uint32_t *sampled,
                                    uint32_t *hits, uint64_t *stats, hipStream_t stream) {
    if (!a || !hits || num_seqs > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (!walk_ptrs_ok(data, indices, data_bytes) || !walk_sizes_ok(num_seqs, data_bytes)) return KMC_ERR_INVALID_ARG;
    MArgs g;
    g.seed = a->seed;
    g.maxh = max_hash(a->j);
    g.j = a->j;
    g.min_count = min_count;
    g.hd = a->L.hd;
    g.keys = a->L.keys[a->active];
    g.counts = a->L.counts[a->active];
    const Table T = table_of(a, a->active);
    g.mask = T.mask;
    g.chain = T.chain;
    g.windows = windows;
    g.sampled = sampled;
    g.hits = hits;
    g.stats = reinterpret_cast<unsigned long long *>(stats);
    g.w = WalkArgs{};
    if (stats) {
        hipLaunchKernelGGL(accum_match_stats_kernel, dim3(1), dim3(1), 0, stream, g);
        if (hipError_t he = hipGetLastError()) return (int)he;
    }
    if (num_seqs == 0) return KMC_OK;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    g.w = walk_args(data, indices, num_seqs, data_bytes, a->k, a->flags, cus);
    for (uint32_t *out : {windows, sampled, hits})
        if (out)
            if (hipError_t he = hipMemsetAsync(out, 0, (size_t)num_seqs * 4, stream)) return (int)he;
    for_walk(a->flags, a->k, [&](auto fwd, auto big) {
        hipLaunchKernelGGL((accum_match_kernel<decltype(fwd)::value, decltype(big)::value>), dim3((unsigned)g.w.G),
                           dim3(kBlock), 0, stream, g);
    });
    return (int)hipGetLastError();
}

extern "C" int kmc_label_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                      uint64_t data_bytes, uint32_t source, hipStream_t stream) {
    if (!a || source >= KMC_CLASSIFY_MAX_SOURCES || num_seqs > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (num_seqs > 0 && (!walk_ptrs_ok(data, indices, data_bytes) || !walk_sizes_ok(num_seqs, data_bytes)))
        return KMC_ERR_INVALID_ARG;
    const size_t C = (size_t)1 << a->lg;
    if (!a->labels && hipMalloc(reinterpret_cast<void **>(&a->labels), C * 4) != hipSuccess) {
        (void)hipGetLastError();
        a->labels = nullptr;
        return KMC_ERR_NOMEM;
    }
    if (!a->labelled) {  // the first label of the table as it stands
        if (hipError_t he = hipMemsetAsync(a->labels, 0, C * 4, stream)) return (int)he;
        a->labelled = true;
    }
    if (num_seqs == 0) return KMC_OK;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const Table T = table_of(a, a->active);
    LArgs g;
    g.w = walk_args(data, indices, num_seqs, data_bytes, a->k, a->flags, cus);
    g.seed = a->seed;
    g.maxh = max_hash(a->j);
    g.j = a->j;
    g.bit = 1u << source;
    g.hd = a->L.hd;
    g.keys = T.keys;
    g.mask = T.mask;
    g.chain = T.chain;
    g.labels = a->labels;
    for_walk(a->flags, a->k, [&](auto fwd, auto big) {
        hipLaunchKernelGGL((accum_label_kernel<decltype(fwd)::value, decltype(big)::value>), dim3((unsigned)g.w.G),
                           dim3(kBlock), 0, stream, g);
    });
    return (int)hipGetLastError();
}

extern "C" size_t kmc_classify_workspace_size(uint64_t num_seqs, uint64_t data_bytes, uint32_t num_sources, int device) {
    if (!walk_sizes_ok(num_seqs, data_bytes) || num_sources < 1 || num_sources > KMC_CLASSIFY_MAX_SOURCES || device < 0)
        return 0;
    int cus = 0;  // (the arguments are checked before any HIP call)
    if (device_cus(device, &cus)) return 0;
    return classify_layout(nullptr, walk_groups(data_bytes, cus)).bytes;
}

extern "C" int kmc_classify_from_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                       uint64_t data_bytes, uint32_t num_sources, uint32_t min_count, uint32_t *windows,
                                       uint32_t *sampled, uint32_t *hits, uint32_t *best, uint32_t *best_hits,
                                       uint32_t *next_hits, uint32_t *scores, uint64_t *stats, void *workspace,
                                       size_t workspace_bytes, hipStream_t stream) {
    if (!a || !hits || num_seqs > kMaxSeqs) return KMC_ERR_INVALID_ARG;
    if (!walk_ptrs_ok(data, indices, data_bytes) || !walk_sizes_ok(num_seqs, data_bytes)) return KMC_ERR_INVALID_ARG;
    if (!best || !best_hits || !next_hits) return KMC_ERR_INVALID_ARG;
    if (num_sources < 1 || num_sources > KMC_CLASSIFY_MAX_SOURCES || !a->labelled) return KMC_ERR_INVALID_ARG;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const int G = walk_groups(data_bytes, cus);
    if (workspace) {
        if (workspace_bytes < classify_layout(nullptr, G).bytes) return KMC_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 7u) return KMC_ERR_ALIGNMENT;
    }
    CArgs c;
    MArgs &g = c.m;
    g.seed = a->seed;
    g.maxh = max_hash(a->j);
    g.j = a->j;
    g.min_count = min_count;
    g.hd = a->L.hd;
    g.keys = a->L.keys[a->active];
    g.counts = a->L.counts[a->active];
    const Table T = table_of(a, a->active);
    g.mask = T.mask;
    g.chain = T.chain;
    g.windows = windows;
    g.sampled = sampled;
    g.hits = hits;
    g.stats = reinterpret_cast<unsigned long long *>(stats);
    g.w = WalkArgs{};
    if (stats) {
        hipLaunchKernelGGL(accum_match_stats_kernel, dim3(1), dim3(1), 0, stream, g);
        if (hipError_t he = hipGetLastError()) return (int)he;
    }
    if (num_seqs == 0) return KMC_OK;
    CLayout l;
    if (int e = bind_layout(classify_ws, device, workspace, workspace_bytes, 8,
                            [&](void *b) { return classify_layout(b, G); }, &l))
        return e;
    g.w = walk_args(data, indices, num_seqs, data_bytes, a->k, a->flags, cus);
    c.labels = a->labels;
    c.ns = num_sources;
    c.srcmask = num_sources == 32 ? ~0u : (1u << num_sources) - 1u;
    c.best = best;
    c.best_hits = best_hits;
    c.next_hits = next_hits;
    c.scores = scores;
    c.tags = l.tags;
    c.rows = l.rows;
    c.waves = (int64_t)G * kWavesPerBlock;
    const size_t n4 = (size_t)num_seqs * 4;
    for (uint32_t *out : {windows, sampled, hits, best_hits, next_hits})
        if (out)
            if (hipError_t he = hipMemsetAsync(out, 0, n4, stream)) return (int)he;
    if (hipError_t he = hipMemsetAsync(best, 0xFF, n4, stream)) return (int)he;  // KMC_CLASSIFY_NONE
    if (scores)
        if (hipError_t he = hipMemsetAsync(scores, 0, n4 * num_sources, stream)) return (int)he;
    if (hipError_t he = hipMemsetAsync(l.tags, 0xFF, 2 * (size_t)c.waves * sizeof(long long), stream)) return (int)he;
    for_walk(a->flags, a->k, [&](auto fwd, auto big) {
        hipLaunchKernelGGL((accum_classify_kernel<decltype(fwd)::value, decltype(big)::value>), dim3((unsigned)g.w.G),
                           dim3(kBlock), 0, stream, c);
    });
    if (hipError_t he = hipGetLastError()) return (int)he;
    hipLaunchKernelGGL(classify_cut_kernel, dim3((unsigned)c.waves), dim3(kCutBlock), 0, stream, c);
    return (int)hipGetLastError();
}

extern "C" int kmc_sketch_accum_reset(kmc_sketch_accum *a, hipStream_t stream) {
    if (!a) return KMC_ERR_INVALID_ARG;
    return start_over(a, stream);
}

extern "C" void kmc_sketch_accum_free(kmc_sketch_accum *a) {
    if (!a) return;
    if (a->base) (void)hipFree(a->base);
    if (a->labels) (void)hipFree(a->labels);
    delete a;
}
