// kmc_hash.hip — canonical k-mer counting for k <= 31 (BASELINE config C4,
// SURVEY.md §8(b) kmc_count_canonical_hash).  No reference counterpart: the
// reference stops at dense 4^k tables (permutationsCountAll, main.cu:636-646), which
// are infeasible beyond k ~ 13.  Same window and record rules as the dense path;
// the key of a valid window is its 2-bit MSB-first encoding (A0 C1 G2 T3, first
// base most significant, i.e. lexicographic), canonicalised to
// min(key(window), key(reverse complement)) unless KMC_CANON_FORWARD is given.
//
// Hash-partitioned counting, so that no table lives in HBM and no k-mer costs a
// device-scope atomic.  The input walks partition a window by m = key x C (one
// multiply, invertible); the lists hold h = feistel(key) (one Feistel round on
// the 62-bit key, its own inverse: the distinct keys are mapped back on output).  Record r has 2^lg_r lists (top lg_r
// bits of m, about 4 K windows each, lg_r <= 15), grouped in 2^lgc_r coarse
// buckets (top lgc_r = min(lg_r, 7) bits):
//   K1 count    workgroups walk contiguous chunk ranges record piece by record
//               piece; per-piece LDS counters -> windows per (r, list, workgroup)
//               and per (r, coarse bucket, workgroup)
//   K2 scan     exclusive prefix sums of both (kmc_scan.h): lists contiguous,
//               coarse buckets = runs of lists, workgroup segments inside each
//   K3a coarse  the same walk; each round of 16 K windows is counting-sorted by
//               coarse bucket in LDS and written out in runs (whole lines) to the
//               workgroup's segment of each bucket (straight to the lists when a
//               bucket is one list)
//   K3b fine    one workgroup per coarse bucket of the records with more lists than
//               buckets: bucket -> its lists through per-list LDS rings flushed as
//               whole 64-byte segments (Ring8; the radix path's R3 scheme)
//   K4 count    two 512-thread workgroups per CU stride over the lists; a list
//               (held in registers) is counted in an LDS table (4 096 slots,
//               double hashing, 64-bit CAS claim, 32-bit add for repeats) in as
//               many passes as keep a pass near 2 K keys (selected by hash bits
//               below the list bits); each wave stages its keys of the pass in LDS
//               and its lanes take them as their probe chains end; the slots each
//               wave claimed are written (claim order) to the list's segment and
//               cleared
//   K5 place    exclusive scan of the distinct counts; each list's pairs are copied
//               to their final place; records are contiguous runs of lists (K4
//               writes 8 bytes per pair, encode_pair: counts 1..3 in the key's two
//               spare top bits, larger ones in a side array)
// Bytes per window: the input twice (K1, K3a), an 8-byte h written and read twice
// (K3a -> K3b -> K4), 12 bytes of pairs written, read and written again.
//
// Host side (end of the file): kmc_count_canonical_hash_ex is a list of steps --
// fetch_offsets, canon_plan (geometry), bind_canon_workspace (canon_carve: the one place
// the workspace layout is written, also behind the size query), upload_plan,
// run_front (K1 .. K3b), then run_direct or run_placed (K4 and the output), which
// share read_result for the error word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "kmc.h"
#include "kmc_canon_walk.h"
#include "kmc_internal.h"
#include "kmc_scan.h"
#include "kmc_stream.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

constexpr uint64_t kEmptyH = ~0ull;  // no list value: those are feistel outputs, < 2^62
constexpr int kWalkBlock = 1024;             // K1 / K3a / K3b threads per workgroup
constexpr int kMaxLg = 15;                   // at most 32 768 lists per record (K1's LDS counters)
constexpr int kCoarseLg = 7;                 // at most 128 coarse buckets per record
constexpr int kMaxBk = 1 << (kMaxLg - kCoarseLg);  // buckets of one staged round (coarse, or lists per bucket)
constexpr int64_t kListTarget = 4096;        // windows per list aimed at
constexpr int kRound = 16 * kWalkBlock;      // K3a / K3b windows per staged round
constexpr int kCountBlock = 512;  // K4 threads per workgroup (1024 / kCountBlock workgroups per CU)
constexpr int kTableLg = 12;
constexpr int kTableSlots = 1 << kTableLg;   // K4 LDS table: 4 096 x (8 + 4) B, double hashing
constexpr int kWaves4 = kCountBlock / 64;
constexpr int kStage = 320;                  // K4 per-wave keys staged for one probe loop
constexpr int kClaimW = 320;                 // K4 per-wave claims per pass (2-byte slot ids)
constexpr uint32_t kMaxInitPasses = 16;
// K4 passes: pass_of takes the P-quantile of bits [32, kPassTop) of h times an odd
// constant (17 bits), so a list splits into at most 2^17 passes
constexpr int kPassTop = 64 - kMaxLg;
constexpr uint32_t kMaxPasses = 1u << (kPassTop - 32);
constexpr int kPassDistinct = 2048;          // keys per K4 pass aimed at (table load <= 0.47)
constexpr int kRes = 16;                     // K4 keys per thread held in registers
constexpr int64_t kResKeys = (int64_t)kRes * kCountBlock;
// Bits of the call's error word (HParams::err), read by the host after the last kernel.
constexpr uint32_t kErrPasses = 1u;  // a list beyond K4's pass bits (KMC_ERR_INVALID_ARG)
constexpr uint32_t kErrBound = 2u;   // a queue count, list id, range or output offset out of its
                                     // allocation: the access is skipped (KMC_ERR_INTERNAL)
static_assert(kPassDistinct <= kWaves4 * kClaimW && kTableSlots < 65536 , "K4 sizes");

// A list left to another kernel: its id and its keys ent[begin, end).  A queue of
// them has room for one entry per list (each list is queued there at most once);
// push_list writes it, list_count reads its count and list_ref_ok checks an entry.
struct ListRef { uint64_t list, begin, end; };
struct ListQueue { ListRef *at; unsigned long long *n; };  // [lists] entries, and how many were pushed
// Pairs left in pk[src, src + pairs), to be copied to offset `off` of record rec
// (direct output; queue_copy writes them, canon_fallback_kernel reads them)
struct CopyRef { uint64_t src, rec, off, pairs; };

struct HParams {
    const char *data;        // global offsets (data[p] is byte p)
    const int64_t *idx;      // device, n + 1
    int64_t n;
    int64_t lo, hi;          // window starts in [lo, hi) (= [idx[0], idx[n]))
    int k;
    uint32_t flags;
    int G;                   // K1 / K3a workgroups
    int64_t c_lo, cpw;       // chunk range start, chunks per workgroup
    const uint8_t *lg;       // [n] log2 lists of each record
    const int64_t *cbase;    // [n] cnt index of (r, list 0, its first workgroup)
    const int64_t *ccbase;   // [n] cnt_c index of (r, coarse bucket 0, its first workgroup)
    const int32_t *w0;       // [n] first workgroup holding windows of r
    const int32_t *nwg;      // [n] workgroups holding windows of r
    const int64_t *lbase;    // [n + 1] global id of list 0 of record r (lbase[n] = lists)
    uint32_t *cnt;           // [M] windows per (record, list, workgroup)
    uint64_t *off;           // [M + 1] exclusive scan of cnt
    uint32_t *cnt_c;         // [Mc] windows per (record, coarse bucket, workgroup)
    uint64_t *off_c;         // [Mc + 1] exclusive scan of cnt_c
    uint64_t *ent;           // [windows] h, list by list
    uint64_t *ent_c;         // [windows] partition values, coarse bucket by bucket (K3a -> K3b; aliases pk)
    uint64_t *list_start;    // [lists + 1]
    const int2 *fsplit;      // [K3b workgroups] (record, coarse bucket)
    uint64_t *pk;            // [windows] K4 pairs: keys
    uint32_t *pc;            // [windows] K4 pairs: counts
    uint32_t *ndist;         // [lists] distinct keys per list
    uint64_t *dist_off;      // [lists + 1] exclusive scan of ndist
    int64_t lists;
    uint64_t win_cap;        // entries of ent / pk (the call's windows) and, in direct mode, the least
                             // capacity of out_keys / out_counts: the bound of every queued range and copy
    uint32_t *err;           // kErrPasses: a list exceeds what K4 can split; kErrBound: a bound guard fired
    uint32_t claim_cap;      // K4 claims per wave and pass (kClaimW; smaller only in tests)
    uint32_t sort_cap;       // K4s takes lists of at most this many keys (kSortCap; 0 in tests: none)
    uint32_t sort_cap_big;   // the big K4s instance takes the longer ones up to this (kSortCapBig; 0: none)
    ListQueue big;           // the lists K4s hands to its big instance
    ListQueue defer;         // for the table kernel: without direct output the lists either K4s instance
                             // hands back; with it, only the lists longer than the big instance's cap
                             // (canon_classify_kernel; the first launch)
    uint64_t *rec_off;       // [n + 1] output offsets
    uint64_t *out_keys;
    uint32_t *out_counts;
    // direct output (round 5, section 4.4 of DESIGN.md): the counting kernels write
    // each list's pairs to their final place in record r's output region, reserved
    // from the record's cursor, once r's start is known; otherwise to pk, copied by
    // canon_fallback_kernel at the end
    int direct;
    int32_t *lrec;                // [lists] record of each list
    unsigned long long *rstate;   // [n] bits 0-39: pairs reserved in r; 40-63: lists of r not yet reserved,
                                  // counted up from 2^24 - lists(r) (0 once every list has reserved)
    unsigned long long *rbase;    // [n + 1] start of record r's pairs once known (~0 before)
    CopyRef *fq;                  // [2 lists] the copies canon_fallback_kernel makes
    unsigned long long *nfq;      // their number
    ListQueue tq;                 // the queue this canon_table_kernel launch drains (defer or defer2)
    ListQueue defer2;             // direct mode: the lists either K4s instance hands back (too many
                                  // crowded slots), drained by the table kernel's second launch
    int64_t l_lo, l_hi;           // direct mode: the lists of this launch of the common instance
};

// Raises bit `b` of the call's error word (any thread; the host reads it after the
// last kernel).  Round 6: every queue count, queued list id / key range, record id
// and output offset that a kernel takes from the workspace is checked against its
// allocation before it is used, and a value outside it raises kErrBound and skips
// the access (the call returns KMC_ERR_INTERNAL) instead of faulting the queue
// (section 4.4 of DESIGN.md, "The round-5 memory-aperture fault").
__device__ __forceinline__ void raise_err(const HParams &p, uint32_t b) {
    __hip_atomic_fetch_or(p.err, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Appends list l and its key range to q (one thread).
__device__ __forceinline__ void push_list(const HParams &p, const ListQueue &q, int64_t l, uint64_t b, uint64_t e) {
    const unsigned long long i = atomicAdd(q.n, 1ull);
    if (i >= (uint64_t)p.lists) {  // (guard)
        raise_err(p, kErrBound);
        return;
    }
    q.at[i] = ListRef{(uint64_t)l, b, e};
}

// A count of queued lists taken from the workspace (every thread of the launch
// passes the same word), or -1: (guard) a queue holds at most one entry per list.
__device__ __forceinline__ int64_t list_count(const HParams &p, unsigned long long n) {
    if (n <= (uint64_t)p.lists) return (int64_t)n;
    if (blockIdx.x == 0 && threadIdx.x == 0) raise_err(p, kErrBound);
    return -1;
}

// (guard) a queue entry's list id and key range inside the call's lists and entries
__device__ __forceinline__ bool list_ref_ok(const HParams &p, const ListRef &r) {
    return r.list < (uint64_t)p.lists && r.begin <= r.end && r.end <= p.win_cap;
}

// Partition value of a key: K1 / K3a / K3b bucket and list by its top bits.  A
// multiplicative hash (one 64-bit multiply, invertible) in the two input walks;
// K3b (or K3a for single-list buckets) turns it into feistel(key) when writing the
// lists, which is what K4s / K4 hash and the output maps back to the key.
constexpr uint64_t kMulC = 0x9E3779B97F4A7C15ull, kMulCinv = 0xF1DE83E19937733Dull;
__device__ __forceinline__ uint64_t part_of(uint64_t key);
__device__ __forceinline__ uint64_t list_value(uint64_t m);

// A k <= 31 key uses at most 62 bits, and so does its list value (below): the top
// two bits carry the count tag of the pair format.
constexpr uint64_t kM62 = (1ull << 62) - 1ull;

// One Feistel round on a key's 62 bits: the low 17 bits XORed with the top 17 bits
// of (key >> 17) * kFeiC.  The high 45 bits pass unchanged, so the map is its own
// inverse (~8 VALU ops either way).  The low 17 bits are what K4s (slot + sub) and
// K4 (slot) hash: two keys that agree on their first 22-23 bases differ there, the
// others collide at random.  Round 5: it replaces MurmurHash3's fmix64 rounds on
// 62 bits, whose ~20-op inverse ran in K4s's write-out once the place kernel was
// gone (a timing-only build without it: C4 -1.05, C4R -0.7 ms): same box, C4
// 33.1-33.2 -> 32.3-32.4 ms, C4R 44.2-44.3 -> 43.6-44.0 ms
// (profiles/r05ar_feistel_list_value_ab.txt).
constexpr uint64_t kFeiC = 0x9FB21C651E98DF25ull;
__device__ __forceinline__ uint64_t feistel(uint64_t x) {
    const uint64_t hi = x >> 17;
    return x ^ ((hi * kFeiC) >> 47);
}

__device__ __forceinline__ uint64_t part_of(uint64_t key) { return key * kMulC; }

__device__ __forceinline__ uint64_t list_value(uint64_t m) {  // partition value -> list value
    return feistel(m * kMulCinv);
}

// The pair format (K4s, K4 -> K5 or the fallback copy): pk[o] is a list value h
// with its count in the two spare top bits -- tag 0..2 for 1..3 occurrences, tag 3
// for more, and only then is the count itself in pc[o].  One test decides both the
// tag and the escape.
static_assert(2 * KMC_CANON_MAX_K <= 62, "pair format: keys must leave the top two bits free");
struct Pair { unsigned long long word; bool escaped; };  // for pk; whether the count goes to pc
__device__ __forceinline__ Pair encode_pair(unsigned long long h, uint32_t cnt) {
    const uint32_t c = cnt - 1u;
    const bool small = c < 3u;
    return Pair{h | ((unsigned long long)(small ? c : 3u) << 62), !small};
}
// the store form: (h, cnt) at pair offset o
__device__ __forceinline__ void emit_pair(const HParams &p, uint64_t o, unsigned long long h, uint32_t cnt) {
    const Pair e = encode_pair(h, cnt);
    p.pk[o] = e.word;
    if (e.escaped) p.pc[o] = cnt;
}
// the pair at offset o, whose word x the caller has loaded: its key (the list
// value mapped back) and count
struct KeyCount { uint64_t key; uint32_t count; };
__device__ __forceinline__ KeyCount decode_pair(const HParams &p, uint64_t o, unsigned long long x) {
    const uint32_t tag = (uint32_t)(x >> 62);
    return KeyCount{feistel(x & kM62), tag < 3u ? tag + 1u : p.pc[o]};
}

// The input walk (chunk_raw / chunk_keys / for_each_piece) is kmc_canon_walk.h's;
// a window stores its key's partition value here.
struct PartOf {
    __device__ __forceinline__ unsigned long long operator()(uint64_t key) const { return part_of(key); }
};

// Top nb bits (nb <= 15) of a partition value's high dword (nb = 0: 0) -- one v_bfe_u32
__device__ __forceinline__ uint32_t top_bits(unsigned long long x, int nb) {
    return __builtin_amdgcn_ubfe((uint32_t)(x >> 32), (uint32_t)(32 - nb), (uint32_t)nb);
}

__device__ __forceinline__ int coarse_lg(int lg) { return lg < kCoarseLg ? lg : kCoarseLg; }

// K1: windows per (record, list, workgroup) and per (record, coarse bucket, workgroup).
// Invalid windows add to a per-lane dummy counter past the lists (no branch per window).
constexpr uint32_t kK1Dummy = 1u << kMaxLg;
template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kWalkBlock) void canon_count_kernel(HParams p) {
    __shared__ uint32_t c[(1 << kMaxLg) + 64];
    __shared__ int64_t s_first;
    const int w = blockIdx.x;
    for_each_piece(p, &s_first, [&](int64_t r, int64_t ps, int64_t pe, int64_t rend) {
        const int lg = p.lg[r], lgc = coarse_lg(lg);
        const int nb = 1 << lg;
        for (int b = threadIdx.x; b < nb; b += kWalkBlock) c[b] = 0u;
        __syncthreads();
        const int64_t qs = (int64_t)kWalkBlock << 4;
        int64_t q = ((ps >> 4) + threadIdx.x) << 4;
        ChunkRaw nx = chunk_raw(p, q);  // (unconditional: past the piece it reads harmlessly)
        for (; q < pe; q += qs) {
            unsigned long long h[16];
            const ChunkRaw cr = nx;
            nx = chunk_raw(p, q + qs);  // the next chunk, in flight
            const uint32_t vm = chunk_keys<FWD, BIGK>(p, cr, q, ps, pe, rend, PartOf{}, h);
            const uint32_t dummy = kK1Dummy + (threadIdx.x & 63u);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t sel = (uint32_t)__builtin_amdgcn_sbfe((int)vm, j, 1);  // window j valid: all ones
                uint32_t idx;  // (v_bfi_b32 as asm: the compiler would turn the select into a compare + v_cndmask)
                asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(idx) : "v"(sel), "v"(top_bits(h[j], lg)), "v"(dummy));
                __hip_atomic_fetch_add(&c[idx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        const int64_t nwg = p.nwg[r];
        const int64_t base = p.cbase[r] + (w - p.w0[r]);
        for (int b = threadIdx.x; b < nb; b += kWalkBlock) p.cnt[base + (int64_t)b * nwg] = c[b];
        const int F = 1 << (lg - lgc);
        const int64_t cbase = p.ccbase[r] + (w - p.w0[r]);
        for (int b = threadIdx.x; b < (1 << lgc); b += kWalkBlock) {
            uint32_t s = 0u;
            for (int f = 0; f < F; ++f) s += c[b * F + f];
            p.cnt_c[cbase + (int64_t)b * nwg] = s;
        }
        __syncthreads();
    });
}

// One staged round of K3a / K3b: the block's (up to 16 per thread) hashes h[j]
// (valid where bit j of vm) go to bucket bk(h) < nbk; each bucket's run is written
// to dst at the bucket's cursor, which advances.  The round is counting-sorted in
// LDS first, so that consecutive lanes store consecutive entries of one bucket.
//   cnt[2][kMaxBk + 1]  bucket counts -> offsets (double-buffered by round parity)
//   cur[kMaxBk]         global position of each bucket's next entry
//   del[kMaxBk]         this round: global position of stage index 0 of each run
// Entries go out as h (lists = false: coarse buckets) or as list values (lists).
// Round 6: pin() (an empty asm that redefines the prefetched next chunk's
// registers) runs before the write-out, so the compiler waits for those loads
// there -- issued a round earlier -- instead of at the loop latch behind this
// round's stores: vmcnt counts stores on gfx9 and the write-out issues a variable
// number of them, so a wait placed after them is vmcnt(0), i.e. for their
// acknowledgements, once per 16 K windows.  The write-out is one call (lists a
// uniform flag, not two calls): with two, the structurized CFG has a path through
// neither call -- so through no pin -- and the compiler kept a wait on it.
struct Stage {
    unsigned long long *stage;  // [kRound]
    uint32_t (*cnt)[kMaxBk + 1];
    unsigned long long *cur;
    unsigned long long *del;
};

template <class Bk, class Pin>
__device__ __forceinline__ void staged_round(const Stage &s, int par, int nbk, const unsigned long long (&h)[16],
                                             uint32_t vm, Bk bk, bool lists, uint64_t *dst, Pin pin) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t *cn = s.cnt[par];
    uint32_t rk[8];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t r = 0u;
        if ((vm >> j) & 1u)
            r = __hip_atomic_fetch_add(&cn[bk(h[j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (j & 1) rk[j >> 1] |= r << 16;
        else rk[j >> 1] = r;
    }
    lds_barrier();
    if (tid < 64) {  // exclusive scan of the nbk <= kMaxBk counts, kPerLane per lane; cn[nbk] = total
        constexpr int kPerLane = kMaxBk / 64;
        const int b = kPerLane * lane;
        uint32_t a[kPerLane], t = 0u;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) {
            a[i] = b + i < nbk ? cn[b + i] : 0u;
            t += a[i];
        }
        const uint32_t x = wave_incl_scan(t);
        uint32_t run = x - t;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) {
            if (b + i < nbk) cn[b + i] = run;
            run += a[i];
        }
        if (lane == 63) cn[nbk] = x;
    }
    lds_barrier();
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if ((vm >> j) & 1u) s.stage[cn[bk(h[j])] + ((rk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu)] = h[j];
    for (int b = tid; b < nbk; b += kWalkBlock) {
        const uint32_t o0 = cn[b], o1 = cn[b + 1];
        const unsigned long long g = s.cur[b];
        s.del[b] = g - o0;
        s.cur[b] = g + (o1 - o0);
    }
    const uint32_t total = cn[nbk];
    uint32_t *nx = s.cnt[par ^ 1];  // next round's counts (last read before this round's first barrier)
    for (int b = tid; b <= nbk; b += kWalkBlock) nx[b] = 0u;
    lds_barrier();
    pin();
    if (lists) {  // (uniform) buckets are the lists: list values
        for (uint32_t i = tid; i < total; i += kWalkBlock) {
            const unsigned long long x = s.stage[i];
            dst[s.del[bk(x)] + i] = list_value(x);
        }
    } else {
        for (uint32_t i = tid; i < total; i += kWalkBlock) {
            const unsigned long long x = s.stage[i];
            dst[s.del[bk(x)] + i] = x;
        }
    }
    // the next round writes stage / del only after two barriers, which every
    // thread reaches after this write-out
}

// Ring scatter of 8-byte entries (K3b): the same scheme as
// the radix path's R3 (kmc_radix.hip): a ring of RING = 16 384 / nbk entries per
// bucket in LDS (128 KB in all), entries appended by one returning LDS add on the
// bucket's word W[b] (ring half base << 16 | fill of the current 8-entry segment +
// rank) and one ds_write_b64, whole 64-byte segments (8 entries) written to HBM
// by the bucket's 1024 / nbk owner threads after a barrier, the other W buffer set
// up by them (no third barrier).  Entries that do not fit the ring (a bucket
// taking more than RING - 7 of a round's entries: skewed input) go straight to
// their position in a cold path.  nbk = 2^lgb <= kMaxBk.
constexpr int kRingEnt = 16384;  // 8-byte ring entries in LDS (128 KB)
constexpr uint32_t kSeg = 16;  // entries per HBM segment: a whole 128-byte line (8, 64 bytes, until round 4)
static_assert(kSeg == 8 || kSeg == 16, "K3b segments");
struct Ring8Lds {
    unsigned long long ring[kRingEnt];
    uint32_t W[2][kMaxBk];
    unsigned long long gH[kMaxBk];
    unsigned long long dummy[64];
};

struct Ring8 {
    Ring8Lds *L;
    uint64_t *dst;
    int lgb;              // log2 buckets
    int rlg;              // log2 ring entries per bucket
    uint32_t par;
    unsigned long long F, V;  // owner state of bucket tid >> (10 - lgb)

    __device__ __forceinline__ uint32_t rmask() const { return (1u << rlg) - 1u; }
    __device__ __forceinline__ uint32_t bucket_of_thread() const { return threadIdx.x >> (10 - lgb); }
    __device__ __forceinline__ uint32_t member() const { return threadIdx.x & ((1u << (10 - lgb)) - 1u); }
    __device__ __forceinline__ uint32_t rot(uint32_t b) const { return (kSeg * (b & 3u)) & rmask(); }
    __device__ __forceinline__ uint32_t word(uint32_t b, unsigned long long f) const {
        const uint32_t f0 = (uint32_t)f & (kSeg - 1u);
        const uint32_t half = ((uint32_t)f - f0 + rot(b)) & rmask();
        return (((b << rlg) + half) << 16) | f0;
    }
    // Start of a piece: bucket b's entries go to dst[f0 ...].  The caller
    // synchronises before the first add.
    __device__ __forceinline__ void init(Ring8Lds *lds, uint64_t *d, int lg_buckets, unsigned long long f0) {
        L = lds;
        dst = d;
        lgb = lg_buckets;
        rlg = 14 - lg_buckets;
        par = 0;
        F = f0;
        V = f0;
        if (member() == 0) {
            const uint32_t b = bucket_of_thread();
            L->W[0][b] = word(b, f0);
            L->gH[b] = f0 & ~(unsigned long long)(kSeg - 1u);
        }
    }
    // Phase A: entries val[j] (bit j of vm) to buckets bk[j].
    template <int N>
    __device__ __forceinline__ void add(const unsigned long long (&val)[N], const uint32_t (&bk)[N], uint32_t vm) {
        const int lane = threadIdx.x & 63;
        uint32_t *w = L->W[par];
        uint32_t old[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            old[j] = 0u;
            if ((vm >> j) & 1u)
                old[j] = __hip_atomic_fetch_add(&w[bk[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        uint64_t ovf = 0u;
        const uint32_t R = 1u << rlg;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t lo = old[j] & 0xFFFFu, hi = old[j] >> 16;
            const uint32_t idx = (hi & ~rmask()) | ((hi + lo) & rmask());
            const bool v = (vm >> j) & 1u;
            const bool ok = v && lo < R;
            ovf |= __ballot(v && !ok);
            unsigned long long *d = ok ? &L->ring[idx] : &L->dummy[lane];
            *d = val[j];
        }
        if (__builtin_expect(ovf != 0u, 0)) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const uint32_t lo = old[j] & 0xFFFFu;
                if (((vm >> j) & 1u) && lo >= R) dst[L->gH[bk[j]] + lo] = val[j];
            }
        }
    }
    // Phase B (the caller brackets it with barriers).  Round 4: complete segments
    // leave as whole 64-byte stores by lane quads, as R3's do -- in pass t every
    // quad stores the segment of its lane t, 16 bytes per lane, its ring chunk and
    // list position broadcast by DPP -- instead of each lane storing its own
    // segment in four 16-byte pieces (64 scattered pieces per store instruction,
    // about half the HBM write rate: scripts/write_microbench.hip).
    __device__ __forceinline__ void flush() {
        const uint32_t b = bucket_of_thread(), j = member(), tpb = 1u << (10 - lgb);
        const uint32_t f0 = (uint32_t)F & (kSeg - 1u);
        const uint32_t n = (L->W[par][b] & 0xFFFFu) - f0;
        const unsigned long long F1 = F + n, H = F - f0;
        const uint32_t R = 1u << rlg;
        const unsigned long long top = F1 < H + R ? F1 : H + R;
        const uint32_t nseg = (uint32_t)((top - H) / kSeg);
        const uint32_t rt = rot(b);
        const uint32_t q = threadIdx.x & 3u;
        const uint4 *ring4 = reinterpret_cast<const uint4 *>(&L->ring[0]);  // 2 entries per uint4
        for (uint32_t i = j; __any(i < nseg); i += tpb) {  // (wave-uniform trip count: the quads need every lane)
            const unsigned long long g0 = H + (unsigned long long)kSeg * i;
            const bool seg = i < nseg;
            if (seg && g0 < V) {  // partly before V (a piece start after an overflow): entry by entry
                for (uint32_t e = 0; e < kSeg; ++e)
                    if (g0 + e >= V) dst[g0 + e] = L->ring[(b << rlg) + (((uint32_t)(g0 + e) + rt) & rmask())];
            }
            // this lane's segment: uint4 index of its chunk 0 in the ring (bit 31: a
            // whole segment to store) and its list position / 8
            const uint32_t c0 = ((b << rlg) + (((uint32_t)g0 + rt) & rmask())) >> 1;
            const uint32_t A = c0 | (seg && g0 >= V ? 0x80000000u : 0u);
            const uint64_t gs = g0 / kSeg;
            uint32_t a[4], glo[4], ghi[4];
            quad_bcast4(A, a);
            quad_bcast4((uint32_t)gs, glo);
            quad_bcast4((uint32_t)(gs >> 32), ghi);
            // 16-byte pieces q (and q + 4 for 16-entry segments) of each lane's segment
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t at = a[t];
                const uint4 v0 = ring4[(at & 0x7FFFFFFFu) + q];  // (a quad without a segment reads harmlessly)
                const uint4 v1 = kSeg == 16 ? ring4[(at & 0x7FFFFFFFu) + 4 + q] : v0;
                if (at & 0x80000000u) {
                    uint4 *sd = reinterpret_cast<uint4 *>(dst + kSeg * ((uint64_t)glo[t] | ((uint64_t)ghi[t] << 32)));
                    sd[q] = v0;
                    if (kSeg == 16) sd[4 + q] = v1;
                }
            }
        }
        if (F1 > H + R) V = F1;  // [H + R, F1) went straight to dst
        F = F1;
        if (j == 0) {
            L->W[par ^ 1u][b] = word(b, F1);
            L->gH[b] = F1 & ~(unsigned long long)(kSeg - 1u);
        }
        par ^= 1u;
    }
    __device__ __forceinline__ void round_end() {
        lds_barrier();
        flush();
        lds_barrier();
    }
    // End of a piece: the partial segment left in each ring, entry by entry.
    __device__ __forceinline__ void finish() {
        const uint32_t b = bucket_of_thread(), j = member(), tpb = 1u << (10 - lgb);
        const unsigned long long H = F & ~(unsigned long long)(kSeg - 1u), lo = H > V ? H : V;
        const uint32_t rt = rot(b);
        for (unsigned long long g = lo + j; g < F; g += tpb)
            dst[g] = L->ring[(b << rlg) + (((uint32_t)g + rt) & rmask())];
    }
};

// (A ring version of K3a, as K3b's below, measured 10.5 -> 11.5 ms per C4 call: K3a
// is bound by the key hashing of its input walk, and the rings' 8-entry rounds
// need 4 barriers per 16 K windows against the staged sort's 3.)
// K3a: every window's h at its coarse bucket's position (ent_c), or at its list
// position (ent) for records whose buckets are single lists
template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kWalkBlock) void canon_coarse_kernel(HParams p) {
    __shared__ unsigned long long s_stage[kRound];
    __shared__ uint32_t s_cnt[2][kMaxBk + 1];
    __shared__ unsigned long long s_cur[kMaxBk], s_del[kMaxBk];
    __shared__ int64_t s_first;
    const Stage st{s_stage, s_cnt, s_cur, s_del};
    const int w = blockIdx.x;
    int par = 0;
    for_each_piece(p, &s_first, [&](int64_t r, int64_t ps, int64_t pe, int64_t rend) {
        const int lg = p.lg[r], lgc = coarse_lg(lg);
        const int nbk = 1 << lgc;
        const int64_t nwg = p.nwg[r];
        const int64_t base = p.ccbase[r] + (w - p.w0[r]);
        for (int b = threadIdx.x; b < nbk; b += kWalkBlock) s_cur[b] = p.off_c[base + (int64_t)b * nwg];
        for (int b = threadIdx.x; b < 2 * (kMaxBk + 1); b += kWalkBlock) (&s_cnt[0][0])[b] = 0u;
        __syncthreads();
        uint64_t *dst = lg > lgc ? p.ent_c : p.ent;
        const auto bk = [lgc](unsigned long long x) { return top_bits(x, lgc); };
        const int64_t c0 = ps >> 4, c1 = ((pe - 1) >> 4) + 1;
        const bool lists = __builtin_amdgcn_readfirstlane(lg) <= lgc;
        ChunkRaw nx = chunk_raw(p, (c0 + threadIdx.x) << 4);
        const auto pin = [&nx]() {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                asm volatile("" : "+v"(nx.r[i].x), "+v"(nx.r[i].y), "+v"(nx.r[i].z), "+v"(nx.r[i].w));
        };
        pin();
        for (int64_t cb = c0; cb < c1; cb += kWalkBlock) {
            const int64_t c = cb + threadIdx.x;
            unsigned long long h[16];
            const ChunkRaw cr = nx;
            nx = chunk_raw(p, (c + kWalkBlock) << 4);  // next round's chunk
            const uint32_t vm = chunk_keys<FWD, BIGK>(p, cr, c << 4, ps, pe, rend, PartOf{}, h);  // (past the piece: vm = 0, h defined)
            staged_round(st, par, nbk, h, vm, bk, lists, dst, pin);
            par ^= 1;
        }
        __syncthreads();
    });
}


// list boundaries: list (r, b) = off[cbase_r + b*nwg_r] .. off[cbase_r + (b+1)*nwg_r];
// one thread per list (lbase is sorted: the record is a binary search)
__global__ void canon_list_start_kernel(HParams p) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > p.lists) return;
    if (l == p.lists) {
        p.list_start[l] = p.off[p.cbase[p.n]];  // = off[M], every entry
        return;
    }
    int64_t a = 0, b = p.n - 1;  // last record r with lbase[r] <= l
    while (a < b) {
        const int64_t m = (a + b + 1) >> 1;
        if (p.lbase[m] <= l) a = m; else b = m - 1;
    }
    p.list_start[l] = p.off[p.cbase[a] + (l - p.lbase[a]) * p.nwg[a]];
    if (p.lrec) p.lrec[l] = (int32_t)a;
}

// K3b: one workgroup per coarse bucket of a record with several lists per bucket;
// the bucket's entries (ent_c) to its lists (ent), 8 K entries per round through
// the LDS rings (Ring8)
__global__ __launch_bounds__(kWalkBlock) void canon_fine_kernel(HParams p) {
    __shared__ Ring8Lds R;
    const int2 rc = p.fsplit[blockIdx.x];
    const int lg = p.lg[rc.x], lgc = coarse_lg(lg);
    const int lf = lg - lgc;  // log2 lists per coarse bucket (>= 1)
    const int64_t F = (int64_t)1 << lf;
    const int64_t lb = p.lbase[rc.x] + (int64_t)rc.y * F;
    const uint64_t a0 = p.list_start[lb], a1 = p.list_start[lb + F];
    Ring8 rg;
    rg.init(&R, p.ent, lf, p.list_start[lb + (threadIdx.x >> (10 - lf))]);
    __syncthreads();
    // The entries of the next two rounds are in flight while this round is ranked
    // and flushed (one workgroup per CU whose waves meet at every round's barriers
    // would otherwise wait on HBM once per round).  Round 6: two register sets that
    // swap roles every round (no copy of registers still loading), the next round's
    // set pinned (as staged_round's pin) before this round's flush, so no wait
    // follows the flush's stores, and unconditional raw buffer loads -- the range
    // check returns zeros from a1 on -- so every round issues its 8 loads and the
    // compiler's waits on them count exactly (per-lane guarded loads made it
    // vmcnt(0)).  K3b 9.10-9.19 -> 9.00-9.03 ms on C4, with K3a's pin 6.50-6.60 ->
    // 6.42-6.47 ms (profiles/r06s_store_ack_pins_ab.txt).
    const auto fetch = [&](unsigned long long (&xn)[8], uint64_t i0) {
        const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)i0) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(i0 >> 32)) << 32);
        int64_t nrec = ((int64_t)a1 - (int64_t)u) * 8;
        nrec = nrec < 0 ? 0 : (nrec > (1ll << 31) ? (1ll << 31) : nrec);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(p.ent_c + u, (short)0, (int)nrec, 0x00020000);
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(rs, (j * kWalkBlock + (int)threadIdx.x) * 8, 0, 0);
            xn[j] = (unsigned long long)x[0] | ((unsigned long long)x[1] << 32);
        }
    };
    const auto pin = [](unsigned long long (&xn)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(xn[j]));
    };
    // round i0: its entries cur (loaded); cur is refilled with round i0 + 2 rounds' and
    // nxt (round i0 + 1 round's) is waited for before this round's stores
    const auto round = [&](uint64_t i0, unsigned long long (&cur)[8], unsigned long long (&nxt)[8]) {
        unsigned long long v[8], x[8];
        uint32_t bk[8], vm = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = cur[j];
        fetch(cur, i0 + 16 * kWalkBlock);  // (past a1: zeros, never counted)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t i = i0 + (uint64_t)j * kWalkBlock + threadIdx.x;
            vm |= i < a1 ? 1u << j : 0u;
            bk[j] = __builtin_amdgcn_ubfe((uint32_t)(x[j] >> 32), (uint32_t)(32 - lg), (uint32_t)lf);  // list bits below the bucket's
            v[j] = list_value(x[j]);
        }
        rg.add<8>(v, bk, vm);
        pin(nxt);
        rg.round_end();
    };
    unsigned long long xa[8], xb[8];
    fetch(xa, a0);
    pin(xa);
    fetch(xb, a0 + 8 * kWalkBlock);
    for (uint64_t i0 = a0; i0 < a1; i0 += 16 * kWalkBlock) {
        round(i0, xa, xb);
        if (i0 + 8 * kWalkBlock >= a1) break;
        round(i0 + 8 * kWalkBlock, xb, xa);
    }
    rg.finish();
}

// ---------------------------------------------------------------------------
// Direct output (round 5).  Record r's pairs occupy [F_r, F_r + D_r) of the output,
// F_r = D_0 + ... + D_{r-1}; a list reserves its D_l pairs at an offset of r's
// cursor (rstate) -- the order within a record is unspecified, so any order of
// reservations is a valid layout -- and writes them to F_r + offset when F_r is
// already known (rbase[r] != ~0), else to pk for canon_fallback_kernel.  F_r
// becomes known when every list of records 0 .. r-1 has reserved: the list whose
// reservation completes record r extends the chain rbase[r + 1] = rbase[r] + D_r
// as far as the records after it are complete.  Correctness never depends on the
// chain (a list that finds F_r unknown takes the pk path, and the final scan sets
// every F_r); the chain only decides how many pairs avoid the copy.
constexpr int kPairsBits = 40;
constexpr unsigned long long kPairsMask = (1ull << kPairsBits) - 1ull;
constexpr unsigned long long kUnknown = ~0ull;

// The chain's words are read and written with read-modify-write atomics only: a
// plain agent-scope load can be served from this XCD's L2 (MI355X: one L2 per
// XCD, not coherent with the others within a kernel), where a line cached before
// another XCD's update still holds the old word -- with loads, C4's chain stopped
// at record 2 in one run (scripts/canon_direct_probe.py).  The atomics are
// performed where every XCD's atomics on the word are ordered.
__device__ __forceinline__ unsigned long long ld_agent(unsigned long long *a) {
    return __hip_atomic_fetch_add(a, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0), gfx9 encoding

// From record r, whose start F is known: publish the starts of the records after
// it while they are complete.  Each store is waited for before the next record's
// state is read, and a completing list reads rbase[r] only after its own
// reservation returned, so one of the two sees the other's write (the chain never
// stops at a record that completed while it was being extended).
__device__ __forceinline__ void chain_from(const HParams &p, int64_t r, unsigned long long F) {
    for (; r < p.n; ++r) {
        const unsigned long long v = ld_agent(&p.rstate[r]);
        if ((v >> kPairsBits) != 0ull) return;  // record r has lists still to reserve
        F += v & kPairsMask;
        (void)__hip_atomic_exchange(&p.rbase[r + 1], F, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wait_vm();
    }
}

// Reserve `cnt` pairs for one list of record r (one thread): returns the list's
// offset in the record and sets F to the record's start, or kUnknown.
__device__ __forceinline__ unsigned long long reserve_pairs(const HParams &p, int64_t r, uint32_t cnt,
                                                            unsigned long long &F) {
    if ((uint64_t)r >= (uint64_t)p.n) {  // (guard) not a record of this call
        raise_err(p, kErrBound);
        F = kUnknown;
        return 0;
    }
    const unsigned long long old = __hip_atomic_fetch_add(&p.rstate[r], (unsigned long long)cnt + (1ull << kPairsBits),
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long f = ld_agent(&p.rbase[r]);  // (issued before the add returned: independent)
    wait_vm();
    if ((old >> kPairsBits) == (1ull << (64 - kPairsBits)) - 1ull) {  // the last list of r
        const unsigned long long fr = ld_agent(&p.rbase[r]);        // (after the add)
        if (fr != kUnknown) chain_from(p, r, fr);
    }
    F = f;
    return old & kPairsMask;
}

// A list's pairs left in pk[src, src + cnt), to be copied to record r's offset c
__device__ __forceinline__ void queue_copy(const HParams &p, uint64_t src, int64_t r, uint64_t c, uint64_t cnt) {
    if (cnt == 0) return;
    const unsigned long long i = atomicAdd(p.nfq, 1ull);
    if (i >= 2ull * (uint64_t)p.lists) {  // (guard) at most two copies per list
        raise_err(p, kErrBound);
        return;
    }
    p.fq[i] = CopyRef{src, (uint64_t)r, c, cnt};
}

// A counted list l whose pairs lie in pk[b0, b0 + pairs) (one thread): its count
// for K5's scan, or with direct output reserved in its record and queued for the
// copy at the end.
__device__ __forceinline__ void finish_list(const HParams &p, int64_t l, uint64_t b0, uint32_t pairs) {
    if (p.direct) {
        unsigned long long F;
        const int64_t r = p.lrec[l];
        queue_copy(p, b0, r, reserve_pairs(p, r, pairs, F), pairs);
    } else {
        p.ndist[l] = pairs;
    }
}

// The workgroup's per-wave totals w[0 .. NW): their sum over the waves before
// wave wv, and over all
template <int NW>
__device__ __forceinline__ void wave_totals(const uint32_t (&w)[NW], int wv, uint32_t &before, uint32_t &total) {
    before = total = 0u;
#pragma unroll
    for (int v = 0; v < NW; ++v) {
        const uint32_t x = w[v];
        before += v < wv ? x : 0u;
        total += x;
    }
}

// Wave-aggregated reservation on an LDS counter: n (wave-uniform) entries for the
// wave by one add of lane 0; returns their start
__device__ __forceinline__ uint32_t wave_reserve_n(uint32_t *counter, uint32_t n) {
    uint32_t wb = 0u;
    if ((threadIdx.x & 63u) == 0u && n) wb = atomicAdd(counter, n);
    return __builtin_amdgcn_readlane(wb, 0);  // (a v_readlane, where __shfl is a ds_bpermute)
}
// ... one entry for each lane of mask (a ballot): the lane's own
__device__ __forceinline__ uint32_t wave_reserve(uint32_t *counter, uint64_t mask) {
    const uint64_t lt = (1ull << (threadIdx.x & 63u)) - 1ull;
    return wave_reserve_n(counter, (uint32_t)__popcll(mask)) + (uint32_t)__popcll(mask & lt);
}

// K4: lists counted in an LDS table, workgroups striding over the lists.  Its
// barriers are LDS-only (lds_barrier): __syncthreads would also wait for the pair
// stores.
//
// An LDS 64-bit CAS costs the LDS ~21 cycles per wave instruction however few
// lanes are active (scripts/lds_microbench.hip, modes 14/16), so the probe loop
// keeps every lane busy: each wave stages its keys of the pass in a private LDS
// queue and its lanes take queue entries as they finish their probe chains.
// Each wave lists the slots its lanes claimed, so that the write-out and the
// table clear touch only the pass's distinct keys.  Measured per pass and wave
// (scripts/c4_prof.py): ~6 probe rounds for ~150 staged keys; the kernel is
// bound by the LDS round trips of those rounds and by the barrier waits of the
// pass structure, not by HBM.
__device__ __forceinline__ void load_keys(const uint64_t *ent, uint64_t i0, uint64_t end,
                                          unsigned long long (&kh)[kRes]) {
#pragma unroll
    for (int j = 0; j < kRes; ++j) {
        const uint64_t i = i0 + (uint64_t)j * kCountBlock + threadIdx.x;
        kh[j] = i < end ? ent[i] : kEmptyH;
    }
}

struct K4Lds {
    unsigned long long tk[kTableSlots];          // slot keys (h), kEmptyH when free
    uint32_t tc[kTableSlots];                    // slot occurrences - 1
    unsigned long long qk[kWaves4][kStage];      // per wave: keys being inserted
    uint16_t cl[kWaves4][kClaimW + 1];           // per wave: slots claimed this pass (+ a spare entry)
    uint32_t ncl[2][kWaves4];                    // per wave: claims (by pass parity)
    uint32_t ovf[2];                             // pass overflow flags (by pass parity)
    unsigned long long dummy[64];                // per lane: CAS target of an idle lane
};

// LDS byte offset of a __shared__ object
template <class T>
__device__ __forceinline__ uint32_t lds_off(T *p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) T *)p;
}

// ds_cmpst_rtn_b64: the old value at LDS byte offset off (stores val if it was cmp)
__device__ __forceinline__ unsigned long long lds_cas64(uint32_t off, unsigned long long cmp,
                                                        unsigned long long val) {
    unsigned long long old;
    asm volatile("ds_cmpst_rtn_b64 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=v"(old) : "v"(off), "v"(cmp), "v"(val) : "memory");
    return old;
}

// Inserts the nq keys staged in qk[wv]: a lane without a key takes the next one,
// so the wave's CAS instructions stay full until the queue drains (an LDS CAS
// costs the same however few lanes are active).  The loop body is branch-free
// but for repeats: an idle lane's CAS goes to its dummy slot (never kEmptyH, so
// it fails), its claim record to the spare entry.  The slots claimed are appended
// to cl[wv] (ncl: wave-uniform count); a wave that claims more than kClaimW
// raises *ovf and stops (the pass is redone split in two), which also bounds the
// table's load below one: no probe chain can wrap.
__device__ __forceinline__ void probe_staged(K4Lds &L, int wv, uint32_t nq, uint32_t cap, uint32_t *ovf,
                                             uint32_t &ncl) {
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1ull;
    const unsigned long long *qk = L.qk[wv];
    uint16_t *cl = L.cl[wv];
    const uint32_t tk0 = lds_off(&L.tk[0]), dummy = lds_off(&L.dummy[lane]);
    if (ncl > cap) return;  // this pass already overflowed
    uint32_t cursor = 0;
    bool busy = false;
    unsigned long long h = 0;
    uint32_t s = 0, step = 1;
    for (;;) {
        const uint64_t mn = __ballot(!busy);
        const uint32_t at = cursor + (uint32_t)__popcll(mn & lt);
        cursor += (uint32_t)__popcll(mn);
        const bool take = !busy && at < nq;
        const unsigned long long nk = qk[take ? at : 0u];
        h = take ? nk : h;
        s = take ? ((uint32_t)nk & (kTableSlots - 1)) : s;
        step = take ? (((uint32_t)(nk >> kTableLg) & (kTableSlots - 1)) | 1u) : step;  // odd: visits every slot
        busy = busy || take;
        if (!__ballot(busy)) break;
        const unsigned long long cur = lds_cas64(busy ? tk0 + 8u * s : dummy, kEmptyH, h);
        const bool claimed = busy && cur == kEmptyH;  // first occurrence (tc holds occurrences - 1)
        const bool dup = busy && cur == h;
        if (__ballot(dup)) {
            if (dup) __hip_atomic_fetch_add(&L.tc[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const uint64_t mc = __ballot(claimed);
        const uint32_t ca = ncl + (uint32_t)__popcll(mc & lt);
        cl[claimed && ca < cap ? ca : (uint32_t)kClaimW] = (uint16_t)s;
        ncl += (uint32_t)__popcll(mc);
        busy = busy && !claimed && !dup;
        s = busy ? ((s + step) & (kTableSlots - 1)) : s;
        if (ncl > cap) {
            if (lane == 0) *ovf = 1u;
            break;
        }
    }
}

// Pass of h among P: the P-quantile of h's bits [32, kPassTop) (above them: the
// list bits), so that splitting pass q of P gives passes 2q and 2q + 1 of 2P
__device__ __forceinline__ uint32_t pass_of(unsigned long long h, uint32_t P) {
    constexpr int kBits = kPassTop - 32;
    const uint64_t x = h * 0xD6E8FEB86659FD93ull;  // (the list value's high bits are raw key bits)
    return (uint32_t)((((x >> 32) & ((1ull << kBits) - 1ull)) * (uint64_t)P) >> kBits);
}

// The wave's keys of pass q / P, staged in its LDS queue and probed; a queue that
// fills up (repeats beyond the pass target) is probed and refilled.
__device__ __forceinline__ void wave_insert(const unsigned long long (&kh)[kRes], uint32_t q, uint32_t P, K4Lds &L,
                                            int wv, uint32_t cap, uint32_t *ovf, uint32_t &ncl) {
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1ull;
    unsigned long long *qk = L.qk[wv];
    int next = 0;  // first key slot not yet staged (wave-uniform)
    do {
        uint32_t nq = 0;  // wave-uniform
#pragma unroll
        for (int j = 0; j < kRes; ++j) {
            if (j >= next && nq <= (uint32_t)(kStage - 64)) {
                const unsigned long long h = kh[j];
                const bool in = h != kEmptyH && pass_of(h, P) == q;
                const uint64_t m = __ballot(in);
                if (in) qk[nq + (uint32_t)__popcll(m & lt)] = h;
                nq += (uint32_t)__popcll(m);
                next = j + 1;
            }
        }
        if (nq) probe_staged(L, wv, nq, cap, ovf, ncl);
    } while (next < kRes && ncl <= cap);
}

__device__ __forceinline__ void clear_table(K4Lds &L) {
    for (int i = threadIdx.x; i < kTableSlots; i += kCountBlock) {
        L.tk[i] = kEmptyH;
        L.tc[i] = 0u;
    }
}

__global__ __launch_bounds__(kCountBlock) __attribute__((amdgpu_waves_per_eu(4))) void canon_table_kernel(HParams p) {
    __shared__ K4Lds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    clear_table(L);
    if (tid < 2) L.ovf[tid] = 0u;
    if (tid < 64) L.dummy[tid] = 0ull;
    lds_barrier();
    // the lists canon_sort_kernel left: longer than its capacity, or a key repeated
    // more often than its dedup takes (defer, or in direct mode defer2)
    const int64_t G = gridDim.x, nl = list_count(p, *p.tq.n);
    const ListRef *dl = p.tq.at;
    int64_t i = blockIdx.x;
    if (i >= nl) return;
    // list bounds two lists ahead, keys one list ahead: entry j's bounds (none: 0,
    // 0), and one list on
    const auto bounds = [&](int64_t j, uint64_t &b, uint64_t &e) {
        b = e = 0;
        if (j < nl) b = dl[j].begin, e = dl[j].end;
    };
    uint64_t b0, e0, b1, e1, b2, e2;
    const auto advance = [&]() { b0 = b1, e0 = e1, b1 = b2, e1 = e2; };
    bounds(i, b0, e0);
    bounds(i + G, b1, e1);
    unsigned long long kr[kRes];
    int par = 0;
    for (; i < nl; i += G, advance()) {
        const int64_t l = (int64_t)dl[i].list;
        bounds(i + 2 * G, b2, e2);
        // (workgroup-uniform: every thread read the same entry)
        if (!list_ref_ok(p, ListRef{(uint64_t)l, b0, e0})) {
            if (tid == 0) raise_err(p, kErrBound);
            continue;
        }
        if (e0 - b0 <= (uint64_t)kResKeys) load_keys(p.ent, b0, e0, kr);
        const uint64_t n = e0 - b0;
        const bool resident = n <= (uint64_t)kResKeys;
        // passes from the list length, capped: repeats do not need passes, and a
        // pass with too many distinct keys overflows and splits
        uint32_t P = 1;
        if (n > (uint64_t)kPassDistinct)
            P = (uint32_t)std::min<uint64_t>(kMaxInitPasses, (n + kPassDistinct - 1) / kPassDistinct);
        uint64_t out = b0;  // next free pair of this list's segment
        for (uint32_t q = 0; q < P;) {
            uint32_t ncl = 0;
            if (resident) {
                wave_insert(kr, q, P, L, wv, p.claim_cap, &L.ovf[par], ncl);
            } else {
                for (uint64_t i0 = b0; i0 < e0; i0 += (uint64_t)kResKeys) {
                    load_keys(p.ent, i0, e0, kr);
                    wave_insert(kr, q, P, L, wv, p.claim_cap, &L.ovf[par], ncl);
                }
            }
            if (lane == 0) L.ncl[par][wv] = ncl;
            lds_barrier();
            const bool ovf = L.ovf[par] != 0u;
            if (tid == 0) L.ovf[par ^ 1] = 0u;  // last read before this barrier
            if (ovf) {
                // clear the table and redo with twice the passes (pass q -> passes 2q,
                // 2q+1); the pairs of the passes already written stay, the split refines
                clear_table(L);
                lds_barrier();
                par ^= 1;
                if (P >= kMaxPasses) {  // > 2^17 x 2 560 distinct keys in one list: out of pass bits
                    if (tid == 0) raise_err(p, kErrPasses);
                    break;
                }
                P <<= 1;
                q <<= 1;
                continue;
            }
            uint32_t before, total;
            wave_totals(L.ncl[par], wv, before, total);
            // the wave's claimed slots, in claim order (coalesced), cleared; the
            // pass's pairs stay inside the list's segment (guard: distinct <= keys)
            const bool fits = out + total <= e0;
            if (!fits && tid == 0) raise_err(p, kErrBound);
            const uint16_t *cl = L.cl[wv];
            for (uint32_t i = lane; i < ncl; i += 64) {
                const uint32_t sl = cl[i];
                const unsigned long long h = L.tk[sl];
                const uint32_t c = L.tc[sl];
                L.tk[sl] = kEmptyH;
                L.tc[sl] = 0u;
                if (fits) emit_pair(p, out + before + i, h, c + 1u);  // (tc holds occurrences - 1; the + 1 folds away)
            }
            out += total;
            lds_barrier();
            par ^= 1;
            ++q;
        }
        if (tid == 0) finish_list(p, l, b0, (uint32_t)(out - b0));
    }
}

// K4s (round 2): the common list, n <= sort_cap keys with no key repeated more than
// kSortMaxM times, counted by a counting sort in LDS instead of the probed table:
//   rank     one returning LDS add per key on its slot's word (slot = the low
//            kSlotsLg bits of h, uniform: the list is cut by other bits), which
//            counts the slot's keys and tests them for distinctness (round 4)
//   scan     exclusive prefix of the 4 096 counts (8 per thread, one block scan)
//   scatter  a key of a distinct slot leaves with count 1; the others go to
//            sk[start(slot) + rank]: those keys sorted by slot
//   dedup    position p (p = tid + 512 j: a wave reads consecutive keys) compares
//            its key with the other keys of its slot (m - 1 of them, m ~ Poisson(<1));
//            the first occurrence is emitted with the slot's count of its key,
//            compacted per wave (one LDS add per wave and round)
// Per key: 2 LDS atomics/reads + 1 scattered 8-byte write + ~m reads, 5 barriers per
// list and no probe chains: the table kernel's CAS round trips (~21 cycles per wave
// instruction) and pass structure are what bound it (section 4.4 of DESIGN.md).
// A list that does not fit (longer than sort_cap, or a slot holding more than
// kSortMaxM keys: a key repeated that often) is appended to p.defer and counted by
// canon_table_kernel, which handles any length and any repeat count.
// Two instances (round 4): the common one, two 512-thread workgroups per CU, takes
// lists of up to 6 080 keys; a big one, one 1 024-thread workgroup per CU with a
// 8 192-slot table, takes the lists of 6 081 .. 12 288 keys that the
// first hands it (chromosome-sized records: 2^15 lists of ~7.6 K keys), which
// until round 3 went to the probed table kernel.
template <int BLOCK, int RES, uint32_t CAP, int SLOTS_LG, uint32_t SK, uint32_t RC, uint32_t HParams::*RUN_CAP>
struct SortCfg {
    // the call's cap on the lists this instance takes (kCap, or what the test hooks lowered it to)
    static __device__ __forceinline__ uint32_t cap(const HParams &p) { return p.*RUN_CAP; }
    static constexpr uint32_t kSk = SK;                 // sk entries: the list's keys, then staged results
    static constexpr uint32_t kRc = RC;                 // direct output: staged results' counts
    static constexpr int kBlock = BLOCK;
    static constexpr int kRes = RES;                    // keys per thread
    static constexpr uint32_t kCap = CAP;               // <= kBlock * kRes
    static constexpr int kSlotsLg = SLOTS_LG;
    static constexpr int kSlots = 1 << SLOTS_LG;        // one 32-bit word per slot
    static_assert(CAP <= (uint32_t)(BLOCK * RES) && CAP < 32768u && CAP <= SK, "K4s sizes");
    static_assert(kSlots == BLOCK * 8, "K4s scan: 8 slot words per thread");
};
using SortSmall = SortCfg<512, 12, 6080, 12, 7456, 1024, &HParams::sort_cap>;       // LDS: 2 workgroups per CU
using SortBig = SortCfg<1024, 12, 12288, 13, 15232, 2048, &HParams::sort_cap_big>;  // LDS: 1 workgroup per CU
constexpr int kSortBlock = SortSmall::kBlock;
constexpr uint32_t kSortCap = SortSmall::kCap;
constexpr uint32_t kSortCapBig = SortBig::kCap;
constexpr uint32_t kSortMaxM = 16;                    // keys per slot handled by the pairwise dedup
constexpr uint32_t kHotMax = 128;                     // crowded slots per list handled by wave rounds

template <class C>
struct K4sLds {
    unsigned long long sk[C::kSk];    // the keys of the slots that fail the distinctness test, sorted by slot
                                      // (direct output: then the distinct slots' keys, then staged results)
    uint32_t sc[C::kSlots];           // slot words: count | sub-hash sum, then start | count | distinct
    uint32_t hot[kHotMax];            // failing slots holding more than kSortMaxM keys (crowded)
    uint32_t wsum[C::kBlock / 64];
    uint32_t pfs[64];                 // scratch target of the next list's L2 prefetch (never read)
    uint32_t out;                     // distinct keys emitted (direct output: of the distinct slots)
    uint32_t nhot;
    uint32_t nres;                    // direct output: (key, count) results of the failing slots
    uint32_t mode;                    // direct output: the results to their final place (1) or to pk (0)
    unsigned long long gbase;         // direct output: where the list's pairs go
    uint32_t rc[C::kRc];              // direct output: the staged results' counts (their keys: sk[n, ...))
};
static_assert(sizeof(K4sLds<SortBig>) <= 160 * 1024, "big K4s instance: one workgroup per CU");
static_assert(sizeof(K4sLds<SortSmall>) <= 80 * 1024, "common K4s instance: two workgroups per CU");

__device__ __forceinline__ uint32_t half16(uint32_t w, uint32_t hi) { return hi ? (w >> 16) : (w & 0xFFFFu); }

// A slot word after the scan: the slot's start in sk (bits 0-15), its key count
// (16-30) and bit 31 set when its keys are known to be distinct (section 4.4).
constexpr uint32_t kSlotDistinct = 0x80000000u;
__device__ __forceinline__ uint32_t slot_count(uint32_t w) { return (w >> 16) & 0x7FFFu; }

// One list of n <= C::kCap keys [b0, e0) counted by the counting sort (the
// workgroup calls it uniformly).  A list with too many crowded slots is deferred
// to the table kernel.
// DIRECT (round 5): the list's pairs are staged in LDS -- the keys of the
// distinct slots (count 1) in sk after the failing slots' keys, the failing
// slots' results after those (keys in sk[n, ...), counts in rc, as many as fit:
// the rest go to pk) -- and reserved in the record once the list's total is
// known, then written out in one coalesced pass: to their final place when the
// record's start is known, else to pk, whose pairs canon_fallback_kernel copies
// at the end.  (Two reservations -- the distinct slots' keys right
// after the scan, written from registers -- measured C4 38.7 ms against 35.1 ms,
// scripts/canon_direct_probe.py.)
template <class C, bool DIRECT>
__device__ __forceinline__ void sort_list(const HParams &p, K4sLds<C> &S, int64_t l, uint64_t b0, uint64_t e0,
                                          uint32_t n, const uint64_t *nxt, uint64_t &nb0, uint64_t &ne0) {
    constexpr int kRes = C::kRes, kBlk = C::kBlock, kSlots = C::kSlots;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t rec = DIRECT ? (int64_t)p.lrec[l] : 0;  // (loaded with the keys)
    unsigned long long kh[kRes];
#pragma unroll
    for (int j = 0; j < kRes; ++j) {
        const uint32_t i = (uint32_t)(j * kBlk + tid);
        kh[j] = i < n ? p.ent[b0 + i] : kEmptyH;
    }
    // the bounds of the workgroup's next list (nxt: its begin and end, or null),
    // loaded with the keys so that they cost no wait of their own; the caller
    // starts the next list with them instead of loading them there (a dependent
    // round trip before that list's key loads)
    nb0 = ne0 = 0;
    if (nxt) {
        nb0 = nxt[0];
        ne0 = nxt[1];
    }
    reinterpret_cast<uint4 *>(S.sc)[2 * tid] = make_uint4(0u, 0u, 0u, 0u);
    reinterpret_cast<uint4 *>(S.sc)[2 * tid + 1] = make_uint4(0u, 0u, 0u, 0u);
    lds_barrier();  // A: counters zero; the previous list is done
    // Round 4: every key of the list waited for here, outside any branch.  The
    // loads above and the uses below sit in per-key branches, so the compiler's
    // wait tracking lost them at the joins and waited vmcnt(0) before every key's
    // use -- in the scatter, right after the previous key's emit store: a store
    // acknowledgement per key (gfx9 counts stores in vmcnt).  Same box: K4s
    // 15.45-15.55 -> 15.05-15.16 ms on C4 (profiles/r04g_c4_ab.txt).  Issuing the
    // rank adds and the scatter's slot reads all before their first use, and one
    // output reservation per wave, measured no further change and was not kept.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), gfx9 encoding
    if (nxt) {
        // (round 4) the workgroup's next list [nb0, ne0) touched once per 128-byte
        // line now, so that its key loads above find it in L2 / MALL one list later
        // (same box: K4s 15.1 -> 14.5 ms on C4).  An LDS-DMA dword per line into a
        // scratch block nothing reads, written as asm: no register receives it, and
        // the compiler, which does not see it, neither sinks it to a use nor makes
        // later LDS accesses wait for it (the builtin did both).  An operation it
        // does not count only makes its own vmcnt waits stricter (completion is in
        // order), and the next list's vmcnt(0) above retires it; the last list
        // prefetches nothing, so none is in flight when the workgroup ends.
        // (a list this instance will not take -- longer than its cap, which the test
        // hooks may lower below kCap -- is another kernel's: not prefetched, so no
        // DMA into this workgroup's LDS is left in flight by a list it skips)
        const uint64_t lim = C::cap(p);
        const uint64_t nn = ne0 - nb0 <= (lim < (uint64_t)C::kCap ? lim : (uint64_t)C::kCap) ? ne0 - nb0 : 0;
        if ((uint64_t)tid * 16u < nn) {
            const uint64_t a = (uint64_t)(p.ent + nb0 + (uint64_t)tid * 16u);
            // (m0, which the compiler reserves, is saved in an SGPR of our own and put
            // back; s_nop 0: the wait state between an SALU write of m0 and the LDS-DMA
            // that reads it)
            uint32_t m0s;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(m0s)
                         : "v"(a), "s"(lds_off(&S.pfs[0]))
                         : "memory");
        }
    }
    if (tid == 0) {
        S.out = 0u;
        S.nhot = 0u;
        S.nres = 0u;
    }
    // rank: one returning add per key on its slot's word, 1 + 2^(16 + sub) with sub
    // four more bits of the key's hash: the low half counts the slot's keys (the
    // key's rank), the high half sums one power of two per key.  A sum of m powers
    // of two has m bits set only if no two are equal (every carry, and every bit
    // carried out of the word, leaves fewer), so popcount(high) == count proves the
    // slot's keys distinct: each is a key of count 1, as a key alone in its slot.
    // Only the slots that fail the test (a repeated key, or two keys on the same
    // sub: ~6 % of the keys at 0.75 keys per slot, against 31 % of the keys sharing
    // a slot with twice the slots) are sorted and compared key by key.
    uint32_t rk[kRes / 2];  // ranks (< 2^16), two per register
#pragma unroll
    for (int j = 0; j < kRes; ++j) {
        if ((j & 1) == 0) rk[j >> 1] = 0u;
        if ((uint32_t)(j * kBlk + tid) < n) {
            const uint32_t lo = (uint32_t)kh[j];
            const uint32_t sl = lo & (kSlots - 1);
            const uint32_t inc = 1u + (0x10000u << __builtin_amdgcn_ubfe(lo, C::kSlotsLg, 4));
            const uint32_t o = __hip_atomic_fetch_add(&S.sc[sl], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            rk[j >> 1] |= (o & 0xFFFFu) << (16 * (j & 1));
        }
    }
    lds_barrier();  // B: every key ranked
    // scan: thread t owns slot words 8t .. 8t+7; a slot of distinct keys takes
    // no room in sk
    const uint4 w0 = reinterpret_cast<const uint4 *>(S.sc)[2 * tid];
    const uint4 w1 = reinterpret_cast<const uint4 *>(S.sc)[2 * tid + 1];
    uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    uint32_t run = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t c = w[i] & 0xFFFFu;
        const bool dist = (uint32_t)__builtin_popcount(w[i] >> 16) == c;
        if (__builtin_expect(!dist && c > kSortMaxM, 0)) {
            const uint32_t x = atomicAdd(&S.nhot, 1u);
            if (x < kHotMax) S.hot[x] = 8u * tid + i;
        }
        w[i] = run | (c << 16) | (dist ? kSlotDistinct : 0u);  // exclusive start, relative to the thread
        run += dist ? 0u : c;
    }
    const uint32_t incl = wave_incl_scan(run);
    if (lane == 63) S.wsum[wv] = incl;
    lds_barrier();  // C1: wave totals
    uint32_t before, nsk;  // nsk: keys of the slots that failed the test
    wave_totals(S.wsum, wv, before, nsk);
    const uint32_t base = incl - run + before;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] += base;  // starts < 2^15: no carry into the count
    reinterpret_cast<uint4 *>(S.sc)[2 * tid] = make_uint4(w[0], w[1], w[2], w[3]);
    reinterpret_cast<uint4 *>(S.sc)[2 * tid + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    lds_barrier();  // C2: slot starts
    const uint32_t nhot = S.nhot;
    if (nhot > kHotMax) {  // too many crowded slots: the probed table counts this list (uniform)
        // (direct output: to the table kernel's second launch, after every other
        // list; its first takes the lists too long for the big instance)
        if (tid == 0) push_list(p, DIRECT ? p.defer2 : p.defer, l, b0, e0);
        return;  // (the next list's barrier A orders the LDS reuse)
    }
    const uint32_t na = n - nsk;  // keys of the distinct slots (each a pair of count 1)
    constexpr bool staged = DIRECT;  // (the distinct slots' keys always fit: n <= kCap <= kSk)
    // results staged in LDS (the rest to pk[b0 + na + o])
    const uint32_t rcap = DIRECT ? (C::kSk - n < C::kRc ? C::kSk - n : C::kRc) : 0u;
    // result o of the failing slots (counted in nres_at): staged after the distinct
    // slots' keys (its count in rc), or as a pair in pk
    uint32_t *const nres_at = DIRECT ? &S.nres : &S.out;
    const auto put_result = [&](uint32_t o, unsigned long long h, uint32_t cnt) {
        if (DIRECT && o < rcap) {
            S.sk[n + o] = h;
            S.rc[o] = cnt;
        } else {
            emit_pair(p, b0 + (DIRECT ? na : 0u) + o, h, cnt);
        }
    };
    // scatter: a key of a distinct slot (alone in it, or all its keys on
    // different subs: ~94 % of the keys of distinct 2-4 K-key lists over 4 096
    // slots) is a key of count 1 and leaves at once; the others go to sk
#pragma unroll
    for (int j = 0; j < kRes; ++j) {
        bool alone = false;
        if ((uint32_t)(j * kBlk + tid) < n) {
            const uint32_t sw = S.sc[(uint32_t)kh[j] & (kSlots - 1)];
            alone = (sw & kSlotDistinct) != 0u;
            if (!alone) S.sk[(sw & 0xFFFFu) + half16(rk[j >> 1], j & 1)] = kh[j];
        }
        const uint64_t am = __ballot(alone);
        if (am) {
            const uint32_t o = wave_reserve(&S.out, am);
            if (alone) {
                if (staged) S.sk[nsk + o] = kh[j];  // (sk[0, nsk): the failing slots' keys)
                else emit_pair(p, b0 + o, kh[j], 1u);
            }
        }
    }
    lds_barrier();  // D: the keys of the failing slots sorted by slot
    // those keys, sk[0, nsk), spread over all threads: a key of a slot of at most
    // kSortMaxM keys is compared with the others of its slot, and the first
    // occurrence is emitted with the slot's count of its key (crowded slots: below)
    for (uint32_t p0 = 0; p0 < nsk; p0 += kBlk) {  // workgroup-uniform
        const uint32_t pos = p0 + (uint32_t)tid;
        bool first = false;
        uint32_t cnt = 1u;
        unsigned long long h = 0;
        if (pos < nsk) {
            h = S.sk[pos];
            const uint32_t sw = S.sc[(uint32_t)h & (kSlots - 1)];
            const uint32_t a = sw & 0xFFFFu, e = a + slot_count(sw);
            first = e - a <= kSortMaxM;
            if (first) {
                // the slot's keys read all at once (2 <= m <= kSortMaxM; past the slot:
                // this key's own position, excluded below), not one round trip each --
                // eight, and eight more only in a wave where some slot holds more
                // (round 5: slots of 9-16 keys, repeats in C4R, compared here instead
                // of in the crowded-slot rounds; same box C4R 43.7-43.9 -> 42.5-42.8 ms,
                // C4 unchanged, profiles/r05av_k4s_pairwise_limit_ab.txt)
                const auto cmp = [&](uint32_t t) {
                    const uint32_t q = a + t;
                    const unsigned long long x = S.sk[q < e ? q : pos];
                    if (q < e && q != pos && x == h) {
                        ++cnt;
                        first = first && q > pos;
                    }
                };
#pragma unroll
                for (uint32_t t = 0; t < 8; ++t) cmp(t);
#pragma unroll
                for (uint32_t t0 = 8; t0 < kSortMaxM; t0 += 8) {
                    if (e - a > t0) {
#pragma unroll
                        for (uint32_t t = t0; t < t0 + 8; ++t) cmp(t);
                    }
                }
            }
        }
        const uint32_t o = wave_reserve(nres_at, __ballot(first));
        if (first) put_result(o, h, cnt);
    }
    if (nhot) lds_barrier();  // (uniform) the loop above has read sk before the crowded slots' marks
    // crowded slots (a key repeated more than kSortMaxM times hashes there), one
    // per wave: each round counts the copies of a pivot key 128 at a time, marks
    // them (kEmptyH) and finds the next pivot -- the first key left -- in the same
    // pass: O(m) per distinct key.  Each lane keeps one of the slot's (key, count)
    // results, emitted 64 at a time with one reservation.  (Round 4: the pivot
    // search was a pass of its own, the pivot a ds_bpermute, and every distinct key
    // its own reservation round trip.)
    for (uint32_t hs = (uint32_t)wv; hs < nhot; hs += kBlk / 64) {
        const uint32_t sw = S.sc[S.hot[hs]];
        const uint32_t a = sw & 0xFFFFu, e = a + slot_count(sw);
        uint32_t c = a, nd = 0u;  // nd: distinct keys found (wave-uniform)
        unsigned long long piv = S.sk[a], myk = 0;  // (the same address in every lane: a broadcast)
        uint32_t myc = 0u;
        for (;;) {
            uint32_t cnt = 0u, nx = e;
            for (uint32_t q0 = c; q0 < e; q0 += 128) {
                const uint32_t q1 = q0 + (uint32_t)lane, q2 = q1 + 64u;
                const unsigned long long x1 = q1 < e ? S.sk[q1] : kEmptyH;
                const unsigned long long x2 = q2 < e ? S.sk[q2] : kEmptyH;
                const bool e1 = x1 == piv, e2 = x2 == piv;
                cnt += (uint32_t)__popcll(__ballot(e1)) + (uint32_t)__popcll(__ballot(e2));
                if (e1) S.sk[q1] = kEmptyH;
                if (e2) S.sk[q2] = kEmptyH;
                if (nx == e) {  // (uniform) the first key of another value
                    const uint64_t n1 = __ballot(!e1 && x1 != kEmptyH), n2 = __ballot(!e2 && x2 != kEmptyH);
                    if (n1) nx = q0 + (uint32_t)__builtin_ctzll(n1);
                    else if (n2) nx = q0 + 64u + (uint32_t)__builtin_ctzll(n2);
                }
            }
            if (lane == (int)(nd & 63u)) {
                myk = piv;
                myc = cnt;
            }
            ++nd;
            const bool last = nx >= e;
            if ((nd & 63u) == 0u || last) {  // (uniform) this batch of results out
                const uint32_t nb = ((nd - 1u) & 63u) + 1u;
                const uint32_t wb = wave_reserve_n(nres_at, nb);
                if ((uint32_t)lane < nb) put_result(wb + (uint32_t)lane, myk, myc);
            }
            if (last) break;
            c = nx;
            piv = S.sk[nx];  // (not marked: a value other than piv's)
        }
    }
    lds_barrier();  // E: every key emitted
    if constexpr (DIRECT) {
        // the list's pairs -- the na distinct slots' keys, then the results, of
        // which those past rcap are in pk[b0 + na + rcap, ...) -- reserved in the
        // record with the list's completion, then the staged ones written out
        const uint32_t nres = S.nres, D = na + nres, Ds = na + (nres < rcap ? nres : rcap);
        if (tid == 0) {
            unsigned long long F;
            const unsigned long long c = reserve_pairs(p, rec, D, F);
            bool fin = F != kUnknown;
            if (fin && F + c + D > p.win_cap) {  // (guard) past the caller's arrays: not written there
                raise_err(p, kErrBound);
                fin = false;
            }
            S.mode = fin ? 1u : 0u;
            S.gbase = fin ? F + c : b0;
            if (!fin) queue_copy(p, b0, rec, c, D);  // the whole list from pk
            else queue_copy(p, b0 + Ds, rec, c + Ds, D - Ds);  // (the results past rcap, if any)
        }
        lds_barrier();
        {
            const bool fin = S.mode != 0u;
            const unsigned long long g = S.gbase;
            if (fin) {
                // two loops -- the distinct slots' keys (count 1), then the results --
                // instead of one with a per-pair select of source and count, on
                // pointers set up once (round 5, same box: C4 32.5-32.6 -> 31.9-32.0 ms,
                // C4R 42.6-42.7 -> 41.9-42.0 ms, profiles/r05ax_k4s_writeout_loops_ab.txt;
                // the issue-bound tail pays for every VALU op per pair).  A staged (h, cnt)
                // never takes the pair format: what decode_pair gives of its encoding is
                // feistel(h) and cnt, stored as such
                uint64_t *ko = p.out_keys + g;
                uint32_t *co = p.out_counts + g;
                const unsigned long long *sa = S.sk + nsk;
                for (uint32_t i = (uint32_t)tid; i < na; i += kBlk) {
                    ko[i] = feistel(sa[i]);
                    co[i] = 1u;
                }
                const unsigned long long *sr = S.sk + n;
                uint64_t *kr = ko + na;
                uint32_t *cr = co + na;
                for (uint32_t i = (uint32_t)tid; i < Ds - na; i += kBlk) {
                    kr[i] = feistel(sr[i]);
                    cr[i] = S.rc[i];
                }
            } else {
                for (uint32_t i = (uint32_t)tid; i < Ds; i += kBlk) {
                    const bool a = i < na;
                    const unsigned long long h = S.sk[a ? nsk + i : n + (i - na)];
                    emit_pair(p, g + i, h, a ? 1u : S.rc[i - na]);
                }
            }
        }
    } else {
        if (tid == 0) p.ndist[l] = S.out;
    }
}

// K4s, common instance: every list; those longer than sort_cap go to the big
// instance (up to sort_cap_big keys) or to the table kernel (DIRECT: already
// queued there by canon_classify_kernel, which runs first).
template <bool DIRECT>
__global__ __launch_bounds__(SortSmall::kBlock) __attribute__((amdgpu_waves_per_eu(4))) void canon_sort_kernel(
    HParams p) {
    __shared__ __attribute__((aligned(16))) K4sLds<SortSmall> S;
    uint64_t b0 = 0, e0 = 0;  // this list's bounds (the previous one loaded them)
    // lists [l_lo, l_hi): all of them, or (DIRECT) one group of records per launch
    const int64_t l_lo = DIRECT ? p.l_lo : 0, l_hi = DIRECT ? p.l_hi : p.lists;
    if (l_lo + (int64_t)blockIdx.x < l_hi) {
        b0 = p.list_start[l_lo + blockIdx.x];
        e0 = p.list_start[l_lo + blockIdx.x + 1];
    }
    for (int64_t l = l_lo + blockIdx.x; l < l_hi; l += gridDim.x) {
        const uint32_t n = (uint32_t)(e0 - b0 < 0xFFFFFFFFull ? e0 - b0 : 0xFFFFFFFFull);
        const uint64_t *nxt = l + gridDim.x < l_hi ? p.list_start + l + gridDim.x : nullptr;
        if (n > p.sort_cap) {  // workgroup-uniform
            if (!DIRECT && threadIdx.x == 0) push_list(p, n <= p.sort_cap_big ? p.big : p.defer, l, b0, e0);
            if (nxt) {
                b0 = nxt[0];
                e0 = nxt[1];
            }
            continue;
        }
        // (the next list of this workgroup: its bounds loaded and its keys
        // prefetched into L2 during this one)
        uint64_t nb0, ne0;
        sort_list<SortSmall, DIRECT>(p, S, l, b0, e0, n, nxt, nb0, ne0);
        b0 = nb0;
        e0 = ne0;
    }
}

// K4s, big instance: the lists the common instance handed over (workgroups beyond
// their number exit at once).
template <bool DIRECT>
__global__ __launch_bounds__(SortBig::kBlock) void canon_sort_big_kernel(HParams p) {
    __shared__ __attribute__((aligned(16))) K4sLds<SortBig> S;
    // DIRECT: one group of records per launch, its segment of the (list-ordered) queue
    const int64_t q_lo = DIRECT ? (int64_t)p.dist_off[p.l_lo] : 0;
    const int64_t nl = list_count(p, DIRECT ? p.dist_off[p.l_hi] : *p.big.n);
    if (q_lo > nl) {  // (guard; also where list_count refused the count)
        if (blockIdx.x == 0 && threadIdx.x == 0) raise_err(p, kErrBound);
        return;
    }
    static_assert(offsetof(ListRef, end) == offsetof(ListRef, begin) + 8, "sort_list reads nxt[0], nxt[1]");
    for (int64_t i = q_lo + blockIdx.x; i < nl; i += gridDim.x) {
        const ListRef r = p.big.at[i];
        const int64_t in = i + gridDim.x;
        uint64_t nb0, ne0;  // (few lists here: the entries are reloaded per list)
        sort_list<SortBig, DIRECT>(p, S, (int64_t)r.list, r.begin, r.end, (uint32_t)(r.end - r.begin),
                                   in < nl ? &p.big.at[in].begin : nullptr, nb0, ne0);
    }
}

// K5: pairs to their final place; record offsets.  Four loads in flight per thread
// (1 and 8 measured, and non-temporal loads / stores: C4R place 9.4 / 8.1 ms against 8.3, C4 within the
// box noise; four consecutive pairs per thread with 16-byte stores: no gain either).
constexpr int kPlaceU = 4;
__global__ __launch_bounds__(256) void canon_place_kernel(HParams p) {
    const int64_t l = blockIdx.x;
    const uint64_t src = p.list_start[l], dst = p.dist_off[l], m = p.ndist[l];
    for (uint64_t i0 = threadIdx.x; i0 < m; i0 += 256 * kPlaceU) {
        unsigned long long x[kPlaceU];
#pragma unroll
        for (int u = 0; u < kPlaceU; ++u) {
            const uint64_t i = i0 + 256u * u;
            x[u] = i < m ? p.pk[src + i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kPlaceU; ++u) {
            const uint64_t i = i0 + 256u * u;
            if (i < m) {
                const KeyCount kc = decode_pair(p, src + i, x[u]);
                p.out_keys[dst + i] = kc.key;
                p.out_counts[dst + i] = kc.count;
            }
        }
    }
}

__global__ void canon_recoff_kernel(HParams p) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= p.n) p.rec_off[r] = p.dist_off[p.lbase[r]];
}

// Direct output: per-record state -- no pairs reserved, 2^24 - lists(r) in the
// list field, so that the last list's reservation carries it to 0 -- and the
// record starts unknown but the first.
__global__ void canon_direct_setup_kernel(HParams p) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < p.n) p.rstate[r] = ((1ull << (64 - kPairsBits)) - (unsigned long long)(p.lbase[r + 1] - p.lbase[r]))
                               << kPairsBits;
    if (r <= p.n) p.rbase[r] = r == 0 ? 0ull : kUnknown;
    if (r == 0) *p.nfq = 0ull;
}

// Direct output: the lists the common K4s instance does not take, by length: a
// flag per list for the big instance (ndist, scanned into dist_off, then compacted
// in list order by canon_big_queue_kernel: each group of records takes its own
// segment), the longer ones to the table kernel's first launch.
__global__ void canon_classify_kernel(HParams p) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= p.lists) return;
    const uint64_t b = p.list_start[l], e = p.list_start[l + 1];
    const bool big = e - b > (uint64_t)p.sort_cap && e - b <= (uint64_t)p.sort_cap_big;
    p.ndist[l] = big ? 1u : 0u;
    if (e - b > (uint64_t)p.sort_cap && !big) push_list(p, p.defer, l, b, e);
}

__global__ void canon_big_queue_kernel(HParams p) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l == p.lists) *p.big.n = p.dist_off[l];
    if (l >= p.lists || !p.ndist[l]) return;
    p.big.at[p.dist_off[l]] = ListRef{(uint64_t)l, p.list_start[l], p.list_start[l + 1]};
}

// Direct output, after every list: each record's start (exclusive scan of the
// records' pair counts: the same values the chain published) -> rbase, rec_off.
// One workgroup of kScanBlock threads, that many records per step.
__global__ __launch_bounds__(kScanBlock) void canon_direct_final_kernel(HParams p) {
    __shared__ uint64_t ws[kScanBlock / 64];
    __shared__ unsigned long long carry;  // the pairs of the steps before this one
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (int64_t r0 = 0; r0 <= p.n; r0 += kScanBlock) {
        const int64_t r = r0 + tid;
        const uint64_t d = r < p.n ? (p.rstate[r] & kPairsMask) : 0ull;
        const unsigned long long before = carry;  // (every thread, ahead of the scan's barriers)
        uint64_t total;
        const unsigned long long start = before + block_excl_scan(d, ws, total);
        if (r <= p.n) {
            p.rbase[r] = start;
            p.rec_off[r] = start;
        }
        if (tid == 0) carry = before + total;
        __syncthreads();
    }
}

// Direct output: the pairs left in pk (lists whose record start was not yet known,
// or that the table kernel counted) to their place; one workgroup per queue entry.
__global__ __launch_bounds__(256) void canon_fallback_kernel(HParams p) {
    int64_t nq = (int64_t)*p.nfq;
    if ((uint64_t)nq > 2ull * (uint64_t)p.lists) {  // (guard) queue_copy stops there
        if (blockIdx.x == 0 && threadIdx.x == 0) raise_err(p, kErrBound);
        nq = 2 * p.lists;
    }
    for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const CopyRef c = p.fq[q];
        const uint64_t src = c.src, r = c.rec, m = c.pairs;
        // (guard, workgroup-uniform) a record of the call, source and target inside their arrays
        const uint64_t dst = r < (uint64_t)p.n ? p.rbase[r] + c.off : ~0ull;
        if (r >= (uint64_t)p.n || src > p.win_cap || m > p.win_cap - src || dst > p.win_cap || m > p.win_cap - dst) {
            if (threadIdx.x == 0) raise_err(p, kErrBound);
            continue;
        }
        for (uint64_t i = threadIdx.x; i < m; i += 256) {
            const KeyCount kc = decode_pair(p, src + i, p.pk[src + i]);
            p.out_keys[dst + i] = kc.key;
            p.out_counts[dst + i] = kc.count;
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
DeviceCache h_ws;  // library-owned workspace
std::mutex h_mu;   // the settings below
uint32_t h_claim_cap = kClaimW;
uint32_t h_sort_cap = kSortCap;
uint32_t h_sort_cap_big = kSortCapBig;
int h_direct = 1;  // direct output when the caller's arrays hold every window (kmc_diag_canon_direct)
constexpr int64_t kGroupLists = 8192;  // direct output: lists per launch of the common K4s instance (at least)
#ifdef KMC_DIAG_HOOKS
// the last direct-output call's fallback copies: queue entries, pairs (kmc_diag_canon_fallback)
unsigned long long h_fb_entries = 0, h_fb_pairs = 0;
std::vector<unsigned long long> h_fb_rec;  // fallback pairs per record
unsigned long long h_fb_defer[3] = {0, 0, 0};  // lists queued: big instance, table (long / big's), table (common's)
// kmc_diag_canon_stale_queue: >= 0 -> the table kernel's second queue count starts the
// call at this value instead of 0 (a counter left un-reset: entries it covers were
// never written by this call); -1: off
long long h_stale_queue = -1;
int64_t h_list_target = kListTarget;  // windows per list canon_plan aims at (kmc_diag_canon_list_target)
#endif

// K1 / K3a instances by orientation and key width
struct WalkCount {
    template <bool F, bool B>
    static void go(const HParams &p, hipStream_t st) {
        hipLaunchKernelGGL((canon_count_kernel<F, B>), dim3(p.G), dim3(kWalkBlock), 0, st, p);
    }
};
struct WalkCoarse {
    template <bool F, bool B>
    static void go(const HParams &p, hipStream_t st) {
        hipLaunchKernelGGL((canon_coarse_kernel<F, B>), dim3(p.G), dim3(kWalkBlock), 0, st, p);
    }
};
template <class W>
void launch_walk(const HParams &p, hipStream_t st) {
    const bool fwd = p.flags & KMC_CANON_FORWARD, big = p.k >= 16;
    if (fwd) big ? W::template go<true, true>(p, st) : W::template go<true, false>(p, st);
    else big ? W::template go<false, true>(p, st) : W::template go<false, false>(p, st);
}

}  // namespace
}  // namespace kmc

using namespace kmc;

#ifdef KMC_DIAG_HOOKS
// Test hook (diagnostic library only, not in kmc.h): K4's per-wave claim capacity, lowered so that the
// pass-overflow split runs often; 0 restores the default.
extern "C" KMC_DIAG_API int kmc_diag_canon_claim_cap(unsigned cap) {
    if (cap > (unsigned)kClaimW) return KMC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h_mu);
    h_claim_cap = cap ? cap : kClaimW;
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): the longest list canon_sort_kernel takes (0: none, so
// every list goes to canon_table_kernel); any value above kSortCap restores the default.
extern "C" KMC_DIAG_API int kmc_diag_canon_sort_cap(unsigned cap) {
    std::lock_guard<std::mutex> lk(h_mu);
    h_sort_cap = cap > kSortCap ? kSortCap : cap;
    h_sort_cap_big = cap == 0 ? 0u : kSortCapBig;  // 0: no counting sort at all (every list to the table)
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): 0 = the pairs always go
// through pk and canon_place_kernel (the layout before round 5), 1 = direct output
// whenever the caller's capacity holds every window (the default).
extern "C" KMC_DIAG_API int kmc_diag_canon_direct(int on) {
    if (on < 0 || on > 1) return KMC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h_mu);
    h_direct = on;
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): the pairs of the last direct-
// output call that went through pk and the fallback copy (their queue entries and
// pairs), i.e. the lists that found their record's start unknown or counted in the
// table kernel.
extern "C" KMC_DIAG_API int kmc_diag_canon_fallback(unsigned long long *entries, unsigned long long *pairs) {
    std::lock_guard<std::mutex> lk(h_mu);
    *entries = h_fb_entries;
    *pairs = h_fb_pairs;
    return KMC_OK;
}

// Test hook (diagnostic library only): per record (up to cap) the fallback pairs of
// the last direct-output call, and the lists queued to the big instance, the
// table kernel's first and second launches.
extern "C" KMC_DIAG_API int kmc_diag_canon_fallback_detail(unsigned long long *per_rec, unsigned cap,
                                                            unsigned long long *queued3) {
    std::lock_guard<std::mutex> lk(h_mu);
    for (unsigned i = 0; i < cap && i < h_fb_rec.size(); ++i) per_rec[i] = h_fb_rec[i];
    for (int j = 0; j < 3; ++j) queued3[j] = h_fb_defer[j];
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): the defect class behind the
// round-5 fault -- a queue counter that a call does not reset,
// so that the table kernel's second launch takes entries this call never wrote
// (in a reused or caller workspace: stale or arbitrary bytes).  v >= 0: the count
// of defer2 starts at v; -1 restores the reset.  With the bound guards the call
// returns KMC_ERR_INTERNAL instead of faulting.
extern "C" KMC_DIAG_API int kmc_diag_canon_stale_queue(long long v) {
    std::lock_guard<std::mutex> lk(h_mu);
    h_stale_queue = v < 0 ? -1 : v;
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): the longest list the big K4s
// instance takes (0: none, so the lists above the common instance's cap go to the
// table kernel); any value above kSortCapBig restores the default.  Call after
// kmc_diag_canon_sort_cap, which resets it.
extern "C" KMC_DIAG_API int kmc_diag_canon_sort_cap_big(unsigned cap) {
    std::lock_guard<std::mutex> lk(h_mu);
    h_sort_cap_big = cap > kSortCapBig ? kSortCapBig : cap;
    return KMC_OK;
}

// Test hook (diagnostic library only, not in kmc.h): the windows per list that
// canon_plan aims at, 16 .. kListTarget (0 restores kListTarget), so that records of
// a few hundred kilobytes have the lists per coarse bucket -- K3b's ring geometry --
// of records of up to 128 M windows.  Host geometry only: no kernel reads it, and
// the size query follows it.
extern "C" KMC_DIAG_API int kmc_diag_canon_list_target(unsigned t) {
    if (t != 0 && (t < 16 || t > (unsigned)kListTarget)) return KMC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h_mu);
    h_list_target = t ? (int64_t)t : kListTarget;
    return KMC_OK;
}
#endif

namespace {
// Geometry of one canonical call, from the host copy of the (biased) record
// offsets: K1 / K3a chunk split, per-record lists / coarse buckets / workgroups,
// cnt layouts, list ids, K3b workgroups.
struct CanonPlan {
    int64_t c_lo = 0, cpw = 1;
    int G = 1;
    std::vector<uint8_t> lg;
    std::vector<int32_t> w0, nwg;
    std::vector<int64_t> cbase, ccbase, lbase;
    std::vector<int2> fsplit;
    int64_t M = 0, Mc = 0, L = 0, windows = 0;
};

void canon_plan(const int64_t *hidx, int64_t n, int k, int cus, CanonPlan &P) {
    const int64_t lo = hidx[0], hi = hidx[n];
    P.c_lo = lo >> 4;
    const int64_t chunks = hi > lo ? ((hi + 15) >> 4) - P.c_lo : 0;
    P.G = (int)std::max<int64_t>(1, std::min<int64_t>(cus, chunks));
    P.cpw = std::max<int64_t>(1, (chunks + P.G - 1) / P.G);
    P.lg.assign(n, 0);
    P.w0.assign(n, 0);
    P.nwg.assign(n, 0);
    P.cbase.assign(n + 1, 0);
    P.ccbase.assign(n + 1, 0);
    P.lbase.assign(n + 1, 0);
    P.fsplit.clear();
    int64_t M = 0, Mc = 0, L = 0, windows = 0;
#ifdef KMC_DIAG_HOOKS
    int64_t target;
    {
        std::lock_guard<std::mutex> lk(h_mu);
        target = h_list_target;
    }
#else
    constexpr int64_t target = kListTarget;
#endif
    for (int64_t r = 0; r < n; ++r) {
        const int64_t a = hidx[r], nw = std::max<int64_t>(0, hidx[r + 1] - a - k);
        windows += nw;
        int g = 0;
        while (g < kMaxLg && (target << g) < nw) ++g;
        const int gc = g < kCoarseLg ? g : kCoarseLg;
        P.lg[r] = (uint8_t)g;
        if (nw > 0) {
            const int64_t cf = a >> 4, cl = (a + nw - 1) >> 4;
            P.w0[r] = (int32_t)((cf - P.c_lo) / P.cpw);
            P.nwg[r] = (int32_t)((cl - P.c_lo) / P.cpw) - P.w0[r] + 1;
        }
        P.cbase[r] = M;
        P.ccbase[r] = Mc;
        P.lbase[r] = L;
        M += ((int64_t)1 << g) * P.nwg[r];
        Mc += ((int64_t)1 << gc) * P.nwg[r];
        L += (int64_t)1 << g;
        if (g > gc && nw > 0)
            for (int c = 0; c < (1 << gc); ++c) P.fsplit.push_back(make_int2((int)r, c));
    }
    P.cbase[n] = M;
    P.ccbase[n] = Mc;
    P.lbase[n] = L;
    P.M = M;
    P.Mc = Mc;
    P.L = L;
    P.windows = windows;
}

// The workspace of a call with plan P over n records: every array of it carved
// from `base` into p (and the scans' block sums into bsum); returns its bytes
// (base null: only those mean anything).  A new array is added here and nowhere else.
size_t canon_carve(const CanonPlan &P, int64_t n, void *base, HParams &p, uint64_t *&bsum) {
    const size_t M = (size_t)P.M, Mc = (size_t)P.Mc, L = (size_t)P.L;
    const size_t M1 = std::max<size_t>(M, 1), Mc1 = std::max<size_t>(Mc, 1), L1 = std::max<size_t>(L, 1);
    const size_t cap_w = (size_t)std::max<int64_t>(P.windows, 1);
    Carver c(base);
    p.idx = c.take<int64_t>(n + 1);
    p.lg = c.take<uint8_t>(n);
    p.cbase = c.take<int64_t>(n + 1);
    p.ccbase = c.take<int64_t>(n + 1);
    p.w0 = c.take<int32_t>(n);
    p.nwg = c.take<int32_t>(n);
    p.lbase = c.take<int64_t>(n + 1);
    p.fsplit = c.take<int2>(std::max<size_t>(P.fsplit.size(), 1));
    p.cnt = c.take<uint32_t>(M1);
    p.off = c.take<uint64_t>(M + 1);
    p.cnt_c = c.take<uint32_t>(Mc1);
    p.off_c = c.take<uint64_t>(Mc + 1);
    bsum = c.take<uint64_t>((size_t)scan_tiles(std::max<int64_t>(P.M, P.L)) + 1);
    p.ent = c.take<uint64_t>(cap_w);
    p.list_start = c.take<uint64_t>(L + 1);
    p.pk = c.take<uint64_t>(cap_w);
    p.ent_c = p.pk;  // dead before K4 writes the pairs
    p.pc = c.take<uint32_t>(cap_w);
    p.ndist = c.take<uint32_t>(L);
    p.dist_off = c.take<uint64_t>(L + 1);
    p.err = c.take<uint32_t>(1);
    p.defer.n = c.take<unsigned long long>(1);
    p.defer.at = c.take<ListRef>(L1);
    p.big.n = c.take<unsigned long long>(1);
    p.big.at = c.take<ListRef>(L1);
    // direct output (round 5)
    p.lrec = c.take<int32_t>(L1);
    p.rstate = c.take<unsigned long long>(n);
    p.rbase = c.take<unsigned long long>(n + 1);
    // (at most two copies per list: its distinct slots' keys and its results; a
    // list the table kernel counts has one)
    p.fq = c.take<CopyRef>(2 * L1);
    p.nfq = c.take<unsigned long long>(1);
    p.defer2.n = c.take<unsigned long long>(1);
    p.defer2.at = c.take<ListRef>(L1);
    p.tq = p.defer;  // the table kernel's first launch
    return c.total();
}

// The record offsets on the host, checked, every one moved up by `mis`.
int fetch_offsets(const int64_t *indices, int64_t n, int64_t mis, hipStream_t stream, std::vector<int64_t> &hidx) {
    hidx.resize(n + 1);
    hipError_t he = hipMemcpyAsync(hidx.data(), indices, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return (int)he;
    for (int64_t r = 0; r < n; ++r)
        if (hidx[r + 1] < hidx[r]) return KMC_ERR_INVALID_ARG;
    for (auto &x : hidx) x += mis;
    return 0;
}

// The caller's workspace (checked) or the library's, bound into p.
int bind_canon_workspace(const CanonPlan &P, int64_t n, int device, void *workspace, size_t workspace_bytes,
                         HParams &p, uint64_t *&bsum) {
    const size_t total = canon_carve(P, n, nullptr, p, bsum);
    // 256: the layout's offsets are 256-byte multiples, and K3b / K4s move whole
    // 16-byte pieces (and LDS-DMA dwords) of it
    if (int e = bind_workspace(h_ws, device, total, workspace, workspace_bytes, 256, &workspace)) return e;
    canon_carve(P, n, workspace, p, bsum);
    return 0;
}

// The plan's arrays to the device; the error word and the queue counts to 0.
int upload_plan(const HParams &p, const CanonPlan &P, const std::vector<int64_t> &hidx, hipStream_t stream) {
    const int64_t n = p.n, NF = (int64_t)P.fsplit.size();
    hipError_t he;
    if ((he = hipMemcpyAsync((void *)p.idx, hidx.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.lg, P.lg.data(), n, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.cbase, P.cbase.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.ccbase, P.ccbase.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.w0, P.w0.data(), n * 4, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.nwg, P.nwg.data(), n * 4, hipMemcpyHostToDevice, stream)) ||
        (he = hipMemcpyAsync((void *)p.lbase, P.lbase.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream)) ||
        (NF && (he = hipMemcpyAsync((void *)p.fsplit, P.fsplit.data(), NF * sizeof(int2), hipMemcpyHostToDevice,
                                    stream))))
        return (int)he;
    if ((he = hipMemsetAsync(p.err, 0, 4, stream)) || (he = hipMemsetAsync(p.defer.n, 0, 8, stream)) ||
        (he = hipMemsetAsync(p.big.n, 0, 8, stream)) || (he = hipMemsetAsync(p.defer2.n, 0, 8, stream)))
        return (int)he;
#ifdef KMC_DIAG_HOOKS
    {
        static unsigned long long stale;  // (static: the async copy reads it after this frame)
        std::lock_guard<std::mutex> lk(h_mu);
        if (h_stale_queue >= 0) {
            stale = (unsigned long long)h_stale_queue;
            if ((he = hipMemcpyAsync(p.defer2.n, &stale, 8, hipMemcpyHostToDevice, stream))) return (int)he;
        }
    }
#endif
    return 0;
}

// The front both back ends share: K1, the two scans, K3a, the list starts, K3b.
int run_front(const HParams &p, const CanonPlan &P, uint64_t *bsum, hipStream_t stream) {
    const int64_t n = p.n, NF = (int64_t)P.fsplit.size();
    hipError_t he;
    if (p.direct)
        hipLaunchKernelGGL(canon_direct_setup_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, p);
    if (P.M > 0) {
        if ((he = hipMemsetAsync(p.cnt, 0, (size_t)P.M * 4, stream)) ||
            (he = hipMemsetAsync(p.cnt_c, 0, (size_t)P.Mc * 4, stream)))
            return (int)he;
        launch_walk<WalkCount>(p, stream);
    }
    excl_scan_u32(p.cnt, P.M, bsum, p.off, stream);
    excl_scan_u32(p.cnt_c, P.Mc, bsum, p.off_c, stream);
    launch_walk<WalkCoarse>(p, stream);
    hipLaunchKernelGGL(canon_list_start_kernel, dim3((unsigned)((P.L + 1 + 255) / 256)), dim3(256), 0, stream, p);
    if (NF > 0) hipLaunchKernelGGL(canon_fine_kernel, dim3((unsigned)NF), dim3(kWalkBlock), 0, stream, p);
    return 0;
}

// A grid of `per_cu` workgroups per CU striding over L lists (at most one per list)
dim3 list_grid(int64_t L, int per_cu, int cus) {
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(L, (int64_t)per_cu * cus)));
}

// After the last counting kernel: the launch status, the distinct keys (read from
// `total`) and the call's error word.
int read_result(const HParams &p, const void *total, hipStream_t stream, uint64_t *distinct) {
    hipError_t he;
    uint32_t err = 0;
    if ((he = hipGetLastError()) || (he = hipMemcpyAsync(distinct, total, 8, hipMemcpyDeviceToHost, stream)) ||
        (he = hipMemcpyAsync(&err, p.err, 4, hipMemcpyDeviceToHost, stream)) || (he = hipStreamSynchronize(stream)))
        return (int)he;
    if (err & kErrBound) return KMC_ERR_INTERNAL;
    if (err) return KMC_ERR_INVALID_ARG;  // a record far beyond any genome (see kMaxPasses)
    return 0;
}

#ifdef KMC_DIAG_HOOKS
// What kmc_diag_canon_fallback(_detail) report of a direct-output call: its fallback
// copies in all and per record, and the lists each queue took.
int diag_read_back(const HParams &p) {
    hipError_t he;
    unsigned long long ne = 0;
    if ((he = hipMemcpy(&ne, p.nfq, 8, hipMemcpyDeviceToHost))) return (int)he;
    std::vector<CopyRef> q(ne);
    if (ne && (he = hipMemcpy(q.data(), p.fq, sizeof(CopyRef) * ne, hipMemcpyDeviceToHost))) return (int)he;
    unsigned long long np = 0;
    std::vector<unsigned long long> per(p.n, 0);
    for (const CopyRef &c : q) {
        np += c.pairs;
        per[c.rec] += c.pairs;
    }
    unsigned long long dq[3] = {0, 0, 0};
    if ((he = hipMemcpy(&dq[0], p.big.n, 8, hipMemcpyDeviceToHost)) ||
        (he = hipMemcpy(&dq[1], p.defer.n, 8, hipMemcpyDeviceToHost)) ||
        (he = hipMemcpy(&dq[2], p.defer2.n, 8, hipMemcpyDeviceToHost)))
        return (int)he;
    std::lock_guard<std::mutex> lk(h_mu);
    h_fb_entries = ne;
    h_fb_pairs = np;
    h_fb_rec.swap(per);
    for (int j = 0; j < 3; ++j) h_fb_defer[j] = dq[j];
    return 0;
}
#endif

// Back end with direct output (the caller's arrays hold every window): the pairs go
// to their final place as the lists are counted.
int run_direct(const HParams &p, const CanonPlan &P, const std::vector<int64_t> &hidx, uint64_t *bsum, int cus,
               hipStream_t stream, uint64_t *num_distinct) {
    const int64_t n = p.n, L = P.L;
    const auto &lbase = P.lbase;
    // the table kernel: two workgroups per CU (their tables fill the LDS) striding
    // over the queued lists (count on the device); workgroups beyond it exit at once
    const dim3 g_big = list_grid(L, 1, cus), g_table = list_grid(L, 1024 / kCountBlock, cus);
    // the lists by length: the big instance's, in list order (a flag scan), and
    // the ones too long for it, which the table kernel counts first
    hipLaunchKernelGGL(canon_classify_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, p);
    excl_scan_u32(p.ndist, L, bsum, p.dist_off, stream);
    hipLaunchKernelGGL(canon_big_queue_kernel, dim3((unsigned)((L + 1 + 255) / 256)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(canon_table_kernel, g_table, dim3(kCountBlock), 0, stream, p);
    // the common instance one group of records per launch: a group's lists find
    // the start of their record known (every earlier record complete at the
    // launch boundary) -- within one launch over every list, workgroups drift
    // apart by more than a record's share of lists, and half of C4's pairs found
    // their record's start unknown (scripts/canon_direct_probe.py).  A record
    // with kGroupLists lists or more is a group of its own; smaller records are
    // grouped up to that many lists (within such a group some lists take the pk
    // path).
    for (int64_t r0 = 0; r0 < n;) {
        int64_t r1 = r0 + 1;
        if (lbase[r1] - lbase[r0] < kGroupLists)
            while (r1 < n && lbase[r1 + 1] - lbase[r0] <= kGroupLists && lbase[r1 + 1] - lbase[r1] < kGroupLists)
                ++r1;
        HParams pg = p;
        pg.l_lo = lbase[r0];
        pg.l_hi = lbase[r1];
        // the group's long lists (big instance) first, then the others; a group
        // whose records are shorter than the common instance's cap has none
        int64_t wmax = 0;
        for (int64_t r = r0; r < r1; ++r) wmax = std::max<int64_t>(wmax, hidx[r + 1] - hidx[r] - p.k);
        if (wmax > (int64_t)p.sort_cap)
            hipLaunchKernelGGL(canon_sort_big_kernel<true>, g_big, dim3(SortBig::kBlock), 0, stream, pg);
        hipLaunchKernelGGL(canon_sort_kernel<true>, list_grid(pg.l_hi - pg.l_lo, 2, cus), dim3(kSortBlock), 0, stream,
                           pg);
        r0 = r1;
    }
    HParams p2 = p;  // the lists both K4s instances handed back (defer2)
    p2.tq = p.defer2;
    hipLaunchKernelGGL(canon_table_kernel, g_table, dim3(kCountBlock), 0, stream, p2);
    hipLaunchKernelGGL(canon_direct_final_kernel, dim3(1), dim3(kScanBlock), 0, stream, p);
    hipLaunchKernelGGL(canon_fallback_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(L, 4096))),
                       dim3(256), 0, stream, p);
    uint64_t distinct = 0;
    if (int e = read_result(p, p.rbase + n, stream, &distinct)) return e;
    *num_distinct = distinct;
#ifdef KMC_DIAG_HOOKS
    if (int e = diag_read_back(p)) return e;
#endif
    return KMC_OK;
}

// Back end through pk: the lists' pairs are counted into pk / pc, the total is
// checked against the caller's capacity, then canon_place_kernel copies them out.
int run_placed(const HParams &p, const CanonPlan &P, uint64_t *bsum, int cus, uint64_t capacity, hipStream_t stream,
               uint64_t *num_distinct) {
    const int64_t n = p.n, L = P.L;
    // persistent, two workgroups per CU (64 KB of LDS each), striding over the lists
    hipLaunchKernelGGL(canon_sort_kernel<false>, list_grid(L, 2, cus), dim3(kSortBlock), 0, stream, p);
    // the lists it handed to its big instance (workgroups beyond their number exit at
    // once), before the table kernel, which also takes the big instance's deferrals
    hipLaunchKernelGGL(canon_sort_big_kernel<false>, list_grid(L, 1, cus), dim3(SortBig::kBlock), 0, stream, p);
    // (two workgroups per CU: their tables fill the LDS)
    hipLaunchKernelGGL(canon_table_kernel, list_grid(L, 1024 / kCountBlock, cus), dim3(kCountBlock), 0, stream, p);
    excl_scan_u32(p.ndist, L, bsum, p.dist_off, stream);
    hipLaunchKernelGGL(canon_recoff_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, p);
    uint64_t distinct = 0;
    if (int e = read_result(p, p.dist_off + L, stream, &distinct)) return e;
    *num_distinct = distinct;
    if (distinct > capacity) return KMC_ERR_CAPACITY;
    if (distinct && (!p.out_keys || !p.out_counts)) return KMC_ERR_INVALID_ARG;
    hipLaunchKernelGGL(canon_place_kernel, dim3((unsigned)L), dim3(256), 0, stream, p);
    hipError_t he;
    if ((he = hipGetLastError()) || (he = hipStreamSynchronize(stream))) return (int)he;
    return KMC_OK;
}
}  // namespace

extern "C" size_t kmc_count_canonical_workspace_size(const int64_t *host_indices, uint64_t num_seqs, int k,
                                                    int device) {
    if (!host_indices || k < 1 || k > KMC_CANON_MAX_K || num_seqs == 0) return 0;
    const int64_t n = (int64_t)num_seqs;
    for (int64_t r = 0; r < n; ++r)
        if (host_indices[r + 1] < host_indices[r]) return 0;
    int cus = 0;  // (the arguments are checked before any HIP call)
    if (device_cus(device, &cus)) return 0;
    // the size for every alignment of `data` (a misaligned pointer shifts the offsets
    // by up to 15 bytes, which can move a record's chunks to another workgroup)
    std::vector<int64_t> b(n + 1);
    size_t best = 0;
    CanonPlan P;
    HParams p{};
    uint64_t *bsum;
    for (int mis = 0; mis < 16; ++mis) {
        for (int64_t r = 0; r <= n; ++r) b[r] = host_indices[r] + mis;
        canon_plan(b.data(), n, k, cus, P);
        best = std::max(best, canon_carve(P, n, nullptr, p, bsum));
    }
    return best;
}

extern "C" int kmc_count_canonical_hash(const char *data, const int64_t *indices, uint64_t num_seqs, int k,
                                        unsigned flags, uint64_t *keys, uint32_t *counts, uint64_t capacity,
                                        uint64_t *rec_offsets, uint64_t *num_distinct, hipStream_t stream) {
    return kmc_count_canonical_hash_ex(data, indices, num_seqs, k, flags, keys, counts, capacity, rec_offsets,
                                       num_distinct, nullptr, 0, stream);
}

extern "C" int kmc_count_canonical_hash_ex(const char *data, const int64_t *indices, uint64_t num_seqs, int k,
                                           unsigned flags, uint64_t *keys, uint32_t *counts, uint64_t capacity,
                                           uint64_t *rec_offsets, uint64_t *num_distinct, void *workspace,
                                           size_t workspace_bytes, hipStream_t stream) {
    if (k < 1 || k > KMC_CANON_MAX_K) return KMC_ERR_UNSUPPORTED_K;
    if (!num_distinct) return KMC_ERR_INVALID_ARG;
    *num_distinct = 0;
    if (num_seqs == 0) return KMC_OK;
    if (!data || !indices || !rec_offsets) return KMC_ERR_INVALID_ARG;
    const int64_t n = (int64_t)num_seqs;
    // any `data` pointer: rounded down to 16 bytes, every offset moved up by the
    // difference (the kernels read whole 16-byte chunks of the aligned buffer; the
    // rounded-down bytes share data's page and lie outside every record)
    const uintptr_t mis = reinterpret_cast<uintptr_t>(data) & 15u;
    std::vector<int64_t> hidx;
    if (int e = fetch_offsets(indices, n, (int64_t)mis, stream, hidx)) return e;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    CanonPlan P;
    canon_plan(hidx.data(), n, k, cus, P);
    HParams p{};
    p.data = data - mis;
    p.n = n;
    p.lo = hidx[0];
    p.hi = hidx[n];
    p.k = k;
    p.flags = flags;
    p.c_lo = P.c_lo;
    p.G = P.G;
    p.cpw = P.cpw;
    p.lists = P.L;
    p.win_cap = (uint64_t)P.windows;
    p.claim_cap = h_claim_cap;
    p.sort_cap = h_sort_cap;
    p.sort_cap_big = h_sort_cap_big;
    p.rec_off = rec_offsets;
    p.out_keys = keys;
    p.out_counts = counts;
    {
        std::lock_guard<std::mutex> lk(h_mu);
        p.direct = h_direct;
    }
    // direct output writes pairs before the total is known: only into arrays that
    // hold every window (the distinct keys are at most that many)
    p.direct = p.direct && keys && counts && capacity >= (uint64_t)P.windows;
    uint64_t *bsum = nullptr;
    if (int e = bind_canon_workspace(P, n, device, workspace, workspace_bytes, p, bsum)) return e;
    if (int e = upload_plan(p, P, hidx, stream)) return e;
    if (int e = run_front(p, P, bsum, stream)) return e;
    return p.direct ? run_direct(p, P, hidx, bsum, cus, stream, num_distinct)
                    : run_placed(p, P, bsum, cus, capacity, stream, num_distinct);
}
