// kmc_sketch_screen.hip — containment of reference sketches in a sequence set (what Mash
// calls a screen): for every reference row, how many of its values occur among the
// hashes of ALL valid windows of a mixture, and how often.  Four steps, three of them
// on the device, all asynchronous with no host read-back; the launches depend on the
// host arguments only; no library-owned buffer (the index is the caller's).
//
// The index (an opaque blob of kmc_sketch_screen_index_size bytes):
//   header  256 B   maxv      the largest indexed value other than UINT64_MAX
//                   has_ff    UINT64_MAX is an indexed value (it is the empty marker of
//                             the slots, so it lives here), ff_mult its multiplicity
//                   log2cap   the slot count C = 2^log2cap as build laid it out
//   mult    uint32[C]  the multiplicity of the value in the same slot
//   slots   uint64[C]  open addressing, linear probing, the slot of v is the low
//                      log2cap bits of v (sketch values are the smallest hashes of a
//                      set: their low bits are the mixed ones); UINT64_MAX: empty
// C is a power of two of at least kRoom * num_refs * sketch_size slots, so a probe
// chain always ends at an empty slot.
//
//   build   the blob is cleared (two memsets: header and mult to 0, slots to
//           UINT64_MAX; nothing a former use left is read), then one thread per row
//           value inserts it with a 64-bit compare-and-swap: equal values of several
//           rows meet in one slot.  The largest value goes through an LDS maximum per
//           workgroup into one 64-bit atomic maximum.
//   count   the walk of kmc_sketch_walk.h (for_each_piece of kmc_canon_walk.h, then
//           for_each_chunk with the hash functor) over the ranges and the launch shape
//           of the sketcher, with no per-record state, no LDS set, no barrier inside
//           a piece and no cut merge: a record matters only for which windows exist.
//           A window's hash h leaves after one compare when h > maxv (reference rows
//           are bottom-s sets: almost every window of a mixture); the others probe
//           the table and add to the multiplicity with a vector global atomic (no
//           return value), once per run of equal hashes among a thread's 16 windows
//           (add_runs).
//           The offsets are clamped to [0, data_bytes] and moved by data & 15 as they
//           are read (Offsets), so the call needs no workspace.
//   results one workgroup per reference row: each value is looked up, the found
//           multiplicities (as 64-bit words, absent values as UINT64_MAX) are sorted
//           in LDS (bitonic_sort of kmc_sketch_pair.h) and the lower median is taken.
//
//   winners the results with every found value credited to one row only, the best
//           that holds it (include/kmc.h has the rule): the first pass is results
//           itself (all[r], no median), claim raises the owner word of every found
//           value's slot to its best holder with a 64-bit atomic maximum, recount is
//           results again, taking a value only where the row owns it.  The owner
//           words are the call's workspace (one per slot the blob can hold, one more
//           for UINT64_MAX, and all[]); the index is only read.
//
// The device code trusts nothing in the blob: count and results read log2cap, check
// that the layout of that many slots fits index_bytes and return otherwise; every
// slot index is masked to the table and a probe chain is left after C steps, so a
// blob that was never built gives an unspecified result and no stray access or hang.
// claim and recount also check the slot count against the owner words they were given
// and return without touching anything when it does not fit.
//
// Constants, shipped / under -DKMC_DIAG_HOOKS (no new symbol):
//   kBlock, kMinChunks, kWgPerCu   the sketcher's (kmc_sketch_walk.h): 64-thread
//                                  workgroups and 256-byte ranges in the diag build
//   kRoom   slots per indexed value, at least    4 / 2  (the diag table is only just
//           large enough: chains are long and wrap round the table's end)
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

#ifdef KMC_DIAG_HOOKS
constexpr uint64_t kRoom = 2;
#else
constexpr uint64_t kRoom = 4;
#endif
constexpr uint64_t kMinSlots = 8;
constexpr uint32_t kMaxLog2Cap = 32;  // KMC_SCREEN_MAX_VALUES * 4 slots
constexpr size_t kHeaderBytes = 256;
constexpr int kBuildBlock = 256;

struct Header {
    unsigned long long maxv;
    uint32_t has_ff, ff_mult;
    uint32_t log2cap;
};
static_assert(sizeof(Header) <= kHeaderBytes, "the header has its 256 bytes");

// the one layout: header, mult[C], slots[C], each rounded up to 256 bytes
__host__ __device__ inline size_t slots_offset(uint64_t cap) { return kHeaderBytes + (((size_t)cap * 4 + 255) & ~(size_t)255); }
__host__ __device__ inline size_t layout_bytes(uint64_t cap) { return slots_offset(cap) + (size_t)cap * 8; }

inline uint32_t log2cap_of(uint64_t num_refs, uint32_t sketch_size) {
    const uint64_t want = kRoom * num_refs * sketch_size;
    uint32_t lg = 3;  // kMinSlots
    while ((1ull << lg) < want) ++lg;
    return lg;
}
static_assert(kMinSlots == 8, "log2cap_of starts at 2^3 slots");

inline bool screen_rows_ok(uint64_t num_refs, uint32_t sketch_size) {
    return sketch_size_ok(sketch_size) && num_refs <= KMC_SCREEN_MAX_VALUES &&
           num_refs * sketch_size <= KMC_SCREEN_MAX_VALUES;
}

// The table as the device sees it; ok: the header's slot count fits the blob.
struct Table {
    Header *hd;
    uint32_t *mult;
    unsigned long long *slots;
    uint64_t cap;
    uint32_t mask;
    bool ok;
};

__device__ __forceinline__ Table open_table(void *index, uint64_t index_bytes) {
    Table T;
    T.hd = static_cast<Header *>(index);
    const uint32_t lg = T.hd->log2cap;
    T.ok = lg >= 3 && lg <= kMaxLog2Cap;
    T.cap = 1ull << (T.ok ? lg : 3);
    T.ok = T.ok && layout_bytes(T.cap) <= index_bytes;
    T.mask = (uint32_t)(T.cap - 1);
    T.mult = reinterpret_cast<uint32_t *>(static_cast<char *>(index) + kHeaderBytes);
    T.slots = reinterpret_cast<unsigned long long *>(static_cast<char *>(index) + slots_offset(T.cap));
    return T;
}

// Where the multiplicity of v is kept, or null when v is not indexed.
__device__ __forceinline__ uint32_t *find(const Table &T, uint64_t v, bool has_ff) {
    if (v == kFill) return has_ff ? &T.hd->ff_mult : nullptr;
    uint32_t i = (uint32_t)v & T.mask;
    for (uint64_t step = 0; step < T.cap; ++step) {  // (guard: a table with no empty slot)
        const uint64_t x = T.slots[i];
        if (x == v) return T.mult + i;
        if (x == kFill) return nullptr;
        i = (i + 1) & T.mask;
    }
    return nullptr;
}

// ---------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------
struct BArgs {
    const uint64_t *rows;
    const uint32_t *sizes;
    int64_t n;
    uint32_t s, log2cap;
    void *index;
};

__global__ __launch_bounds__(kBuildBlock) void screen_build_kernel(BArgs a) {
    __shared__ unsigned long long s_max;
    __shared__ uint32_t s_ff;
    Header *hd = static_cast<Header *>(a.index);
    if (threadIdx.x == 0) {
        s_max = 0ull;
        s_ff = 0u;
        if (blockIdx.x == 0) hd->log2cap = a.log2cap;
    }
    __syncthreads();
    const uint64_t cap = 1ull << a.log2cap;
    const uint32_t mask = (uint32_t)(cap - 1);
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(static_cast<char *>(a.index) + slots_offset(cap));
    const int64_t total = a.n * (int64_t)a.s;
    unsigned long long mx = 0ull;
    bool any = false, ff = false;
    for (int64_t e = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBuildBlock) {
        const int64_t r = e / a.s;
        const int i = (int)(e - r * a.s);
        if (i >= row_size(a.sizes, r, (int)a.s)) continue;
        const unsigned long long v = a.rows[e];
        if (v == kFill) {
            ff = true;
            continue;
        }
        any = true;
        mx = v > mx ? v : mx;
        uint32_t at = (uint32_t)v & mask;
        for (uint64_t step = 0; step < cap; ++step) {  // (guard; cap >= 2 x the values: an empty slot exists)
            const unsigned long long was = atomicCAS(slots + at, (unsigned long long)kFill, v);
            if (was == kFill || was == v) break;
            at = (at + 1) & mask;
        }
    }
    if (any) atomicMax(&s_max, mx);
    if (ff) s_ff = 1u;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_max) atomicMax(&hd->maxv, s_max);
        if (s_ff) hd->has_ff = 1u;
    }
}

// ---------------------------------------------------------------------------
// count
// ---------------------------------------------------------------------------
// (Offsets, the record offsets computed as they are read, and walk_of: kmc_sketch_walk.h)
using Walk = WalkOf<Offsets>;

struct CArgs {
    WalkArgs w;
    uint64_t seed;
    void *index;
    uint64_t index_bytes;
};

// Every window's hash at or below maxv (or UINT64_MAX, when that is indexed) is looked
// up and counted.
template <bool FWD, bool BIGK>
__global__ __launch_bounds__(kBlock) void screen_count_kernel(CArgs a) {
    __shared__ int64_t s_first;
    const Table T = open_table(a.index, a.index_bytes);
    if (!T.ok) return;
    const uint64_t maxv = T.hd->maxv;
    const bool has_ff = T.hd->has_ff != 0u;
    const Walk W = walk_of(a.w);
    const HashOf hf{a.seed};
    for_each_piece(W, &s_first, [&](int64_t, int64_t ps, int64_t pe, int64_t rend) {
        for_each_chunk<FWD, BIGK>(W, ps, pe, rend, hf, [&](const unsigned long long(&h)[16], uint32_t pend) {
            uint32_t cm = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) cm |= (uint32_t)(h[j] <= maxv) << j;
            if (has_ff) {
#pragma unroll
                for (int j = 0; j < 16; ++j) cm |= (uint32_t)(h[j] == kFill) << j;
            }
            pend &= cm;
            if (pend) add_runs(h, pend, [&](uint64_t v) { return find(T, v, has_ff); });
        });
    });
}

// ---------------------------------------------------------------------------
// results
// ---------------------------------------------------------------------------
struct RArgs {
    void *index;  // (read only)
    uint64_t index_bytes;
    const uint64_t *rows;
    const uint32_t *sizes;
    int64_t n;
    uint32_t s;
    int k;
    uint32_t *shared, *median;
    float *identity;
    // winners only (claim and the recount): the owner word of every slot, then UINT64_MAX's
    unsigned long long *owner;
    uint64_t owner_slots;
    const uint32_t *all;
};

__device__ __forceinline__ float containment_identity(uint32_t shared, uint32_t size, int k) {
    if (size == 0) return __uint_as_float(0x7fc00000u);
    if (shared == 0) return 0.0f;
    if (shared == size) return 1.0f;
    return (float)pow((double)shared / (double)size, 1.0 / (double)k);
}

// The owner word of a found value: the best row that holds it, as one number a 64-bit
// atomic maximum can raise.  Row r with all of its size values found (all >= 1) offers
//   q = floor(all * 2^32 / size)   above   2^30 - 1 - r   (30 bits; r < 2^30)
// and the largest offer is the rule's first row (include/kmc.h):
//   - all <= size <= 2^14, so 2^18 <= q <= 2^32: 33 bits, 63 with the low field, and
//     never 0, which is the cleared word: nobody claimed the value
//   - two fractions all/size that differ have denominators of at most 2^14 each, so they
//     differ by at least 2^-28, times 2^32 by at least 16: their floors differ and keep
//     the order of all[a] * size[b] against all[b] * size[a]
//   - equal fractions are the same rational and give the same q; the low field then
//     prefers the smaller r
// so the word depends on the row alone and the maximum on the set of holders, not on
// the order the device meets them in.
constexpr uint32_t kRowBits = 30;
constexpr unsigned long long kRowMask = (1ull << kRowBits) - 1;
static_assert(KMC_SCREEN_MAX_VALUES <= (1ull << kRowBits), "a row index fits the owner word's low field");
static_assert(KMC_SKETCH_MAX_SIZE <= (1 << 14), "the fractions of two rows differ by 2^-28 at least");

__device__ __forceinline__ unsigned long long owner_word(uint32_t all, uint32_t size, int64_t r) {
    return ((((unsigned long long)all << 32) / size) << kRowBits) | (kRowMask - (unsigned long long)r);
}

__device__ __forceinline__ bool owned_by(unsigned long long word, int64_t r) {
    return word != 0ull && (word & kRowMask) == kRowMask - (unsigned long long)r;
}

// The owner word of the value whose multiplicity is kept at `at` (find): its slot's, or
// the one after the last slot's for UINT64_MAX.
__device__ __forceinline__ unsigned long long *owner_of(const Table &T, const RArgs &a, const uint32_t *at) {
    return a.owner + (at == &T.hd->ff_mult ? a.owner_slots : (uint64_t)(at - T.mult));
}

// claim: one workgroup per row, a thread per value (coalesced over the row); every found
// value's owner word is raised to the row's offer with a vector atomic of agent scope
// (no return value).  a.all is the first pass's shared[]; a row with none found offers
// nothing.
__global__ __launch_bounds__(kBlock) void screen_claim_kernel(RArgs a) {
    const Table T = open_table(a.index, a.index_bytes);
    if (!T.ok || T.cap > a.owner_slots) return;
    const bool has_ff = T.hd->has_ff != 0u;
    const int tid = threadIdx.x, s = (int)a.s;
    for (int64_t r = blockIdx.x; r < a.n; r += gridDim.x) {
        const int n = row_size(a.sizes, r, s);
        const uint32_t all = a.all[r];
        if (all == 0u || all > (uint32_t)n) continue;  // (uniform; all <= n unless the blob changed under the call)
        const unsigned long long word = owner_word(all, (uint32_t)n, r);
        const uint64_t *row = a.rows + r * (int64_t)s;
        for (int i = tid; i < n; i += kBlock) {
            const uint32_t *at = find(T, row[i], has_ff);
            if (at && *at) __hip_atomic_fetch_max(owner_of(T, a, at), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// results, and with WON the recount of winners: a found value counts only where its
// owner word names the row.
template <int CAP, bool WON>
__global__ __launch_bounds__(kBlock) void screen_results_kernel(RArgs a) {
    __shared__ uint64_t buf[CAP];  // the multiplicities of the row's values, UINT64_MAX: absent
    __shared__ uint32_t s_shared;
    const Table T = open_table(a.index, a.index_bytes);
    if constexpr (WON) {
        if (!T.ok || T.cap > a.owner_slots) return;
    }
    const bool has_ff = T.ok && T.hd->has_ff != 0u;
    const int tid = threadIdx.x, s = (int)a.s;
    for (int64_t r = blockIdx.x; r < a.n; r += gridDim.x) {
        const int n = row_size(a.sizes, r, s);
        const int P = n > 2 ? pow2_at_least(n) : 2;  // <= CAP
        const uint64_t *row = a.rows + r * (int64_t)s;
        if (tid == 0) s_shared = 0u;
        __syncthreads();  // (and the last row's readers of buf are done)
        uint32_t found = 0u;
        for (int i = tid; i < P; i += kBlock) {
            uint64_t m = kFill;
            if (i < n && T.ok) {
                const uint32_t *at = find(T, row[i], has_ff);
                uint32_t c = at ? *at : 0u;
                if constexpr (WON) {
                    if (c && !owned_by(*owner_of(T, a, at), r)) c = 0u;
                }
                if (c) {
                    m = c;
                    ++found;
                }
            }
            buf[i] = m;
        }
        if (found) atomicAdd(&s_shared, found);
        __syncthreads();
        const uint32_t shared = s_shared;
        uint32_t med = 0u;
        if (a.median) {  // (uniform)
            bitonic_sort<kBlock>(buf, 1, P, tid, [] { __syncthreads(); });
            if (shared) med = (uint32_t)buf[(shared - 1) / 2];
        }
        if (tid == 0) {
            a.shared[r] = shared;
            if (a.median) a.median[r] = med;
            if (a.identity) a.identity[r] = containment_identity(shared, (uint32_t)n, a.k);
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// what the three device calls ask of the blob, in this order; `need`: the bytes it must hold
inline int index_check(const void *index, size_t index_bytes, size_t need) {
    if (!index) return KMC_ERR_INVALID_ARG;
    if (index_bytes < need) return KMC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(index) & 255u) return KMC_ERR_ALIGNMENT;
    return KMC_OK;
}

// what results and winners ask of their arguments, in this order
inline int results_check(const void *index, size_t index_bytes, const uint64_t *r_sketches, const uint32_t *r_sizes,
                         uint64_t num_refs, uint32_t sketch_size, int k, const uint32_t *counts, bool *nothing) {
    *nothing = false;
    if (!canon_k_ok(k)) return KMC_ERR_UNSUPPORTED_K;
    if (!screen_rows_ok(num_refs, sketch_size)) return KMC_ERR_INVALID_ARG;
    if (num_refs == 0) return *nothing = true, KMC_OK;
    if (!r_sketches || !r_sizes || !counts) return KMC_ERR_INVALID_ARG;
    return index_check(index, index_bytes, layout_bytes(kMinSlots));
}

inline void launch_results(const RArgs &a, bool won, hipStream_t stream) {
    const dim3 g((unsigned)(a.n < kMaxGridX ? a.n : kMaxGridX)), b(kBlock);
    for_cap(a.s, [&](auto cap) {
        if (won) hipLaunchKernelGGL((screen_results_kernel<decltype(cap)::value, true>), g, b, 0, stream, a);
        else hipLaunchKernelGGL((screen_results_kernel<decltype(cap)::value, false>), g, b, 0, stream, a);
    });
}

// the slots of the largest table whose layout fits index_bytes (>= the smallest layout)
inline uint64_t slots_within(size_t index_bytes) {
    uint32_t lg = 3;
    while (lg < kMaxLog2Cap && layout_bytes(1ull << (lg + 1)) <= index_bytes) ++lg;
    return 1ull << lg;
}

// the workspace of winners: the one layout behind the size query (base = null) and the bind
struct WLayout {
    unsigned long long *owner;  // [slots + 1]: the last is UINT64_MAX's
    uint32_t *all;
    size_t bytes;
};

inline WLayout winners_layout(void *base, uint64_t slots, uint64_t num_refs) {
    Carver c(base);
    WLayout L;
    L.owner = c.take<unsigned long long>((size_t)slots + 1);
    L.all = c.take<uint32_t>((size_t)num_refs);
    L.bytes = c.total();
    return L;
}

DeviceCache w_ws;  // library-owned workspace of winners

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" size_t kmc_sketch_screen_index_size(uint64_t num_refs, uint32_t sketch_size) {
    if (!screen_rows_ok(num_refs, sketch_size)) return 0;
    return layout_bytes(1ull << log2cap_of(num_refs, sketch_size));
}

extern "C" int kmc_sketch_screen_build(const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                       uint32_t sketch_size, void *index, size_t index_bytes, hipStream_t stream) {
    if (!screen_rows_ok(num_refs, sketch_size)) return KMC_ERR_INVALID_ARG;
    if (num_refs == 0 && !index) return KMC_OK;
    if (num_refs > 0 && (!r_sketches || !r_sizes)) return KMC_ERR_INVALID_ARG;
    const uint32_t lg = log2cap_of(num_refs, sketch_size);
    const uint64_t cap = 1ull << lg;
    if (int e = index_check(index, index_bytes, layout_bytes(cap))) return e;
    char *base = static_cast<char *>(index);
    if (hipError_t he = hipMemsetAsync(base, 0, slots_offset(cap), stream)) return (int)he;
    if (hipError_t he = hipMemsetAsync(base + slots_offset(cap), 0xFF, (size_t)cap * 8, stream)) return (int)he;
    BArgs a;
    a.rows = r_sketches;
    a.sizes = r_sizes;
    a.n = (int64_t)num_refs;
    a.s = sketch_size;
    a.log2cap = lg;
    a.index = index;
    const int64_t blocks = ceil_div(a.n * (int64_t)a.s, kBuildBlock);
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks < kMaxGridX ? blocks : kMaxGridX));
    hipLaunchKernelGGL(screen_build_kernel, dim3(grid), dim3(kBuildBlock), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int kmc_sketch_screen_count(void *index, size_t index_bytes, const char *data, const int64_t *indices,
                                       uint64_t num_seqs, uint64_t data_bytes, int k, unsigned flags, uint64_t seed,
                                       hipStream_t stream) {
    if (int e = walk_check(k, num_seqs, data_bytes, flags)) return e;
    if (num_seqs == 0) return KMC_OK;
    if (!walk_ptrs_ok(data, indices, data_bytes)) return KMC_ERR_INVALID_ARG;
    if (int e = index_check(index, index_bytes, layout_bytes(kMinSlots))) return e;
    int device = 0, cus = 0;
    if (int e = current_device_cus(&device, &cus)) return e;
    const CArgs a{walk_args(data, indices, num_seqs, data_bytes, k, flags, cus), seed, index, index_bytes};
    for_walk(flags, k, [&](auto fwd, auto big) {
        hipLaunchKernelGGL((screen_count_kernel<decltype(fwd)::value, decltype(big)::value>), dim3((unsigned)a.w.G),
                           dim3(kBlock), 0, stream, a);
    });
    return (int)hipGetLastError();
}

extern "C" int kmc_sketch_screen_results(const void *index, size_t index_bytes, const uint64_t *r_sketches,
                                         const uint32_t *r_sizes, uint64_t num_refs, uint32_t sketch_size, int k,
                                         uint32_t *shared, uint32_t *median_mult, float *identity,
                                         hipStream_t stream) {
    bool nothing;
    if (int e = results_check(index, index_bytes, r_sketches, r_sizes, num_refs, sketch_size, k, shared, &nothing)) return e;
    if (nothing) return KMC_OK;
    RArgs a{};
    a.index = const_cast<void *>(index);
    a.index_bytes = index_bytes;
    a.rows = r_sketches;
    a.sizes = r_sizes;
    a.n = (int64_t)num_refs;
    a.s = sketch_size;
    a.k = k;
    a.shared = shared;
    a.median = median_mult;
    a.identity = identity;
    launch_results(a, false, stream);
    return (int)hipGetLastError();
}

extern "C" size_t kmc_sketch_screen_winners_workspace_size(size_t index_bytes, uint64_t num_refs) {
    if (num_refs == 0 || num_refs > KMC_SCREEN_MAX_VALUES || index_bytes < layout_bytes(kMinSlots)) return 0;
    return winners_layout(nullptr, slots_within(index_bytes), num_refs).bytes;
}

extern "C" int kmc_sketch_screen_winners(const void *index, size_t index_bytes, const uint64_t *r_sketches,
                                         const uint32_t *r_sizes, uint64_t num_refs, uint32_t sketch_size, int k,
                                         uint32_t *won, uint32_t *median_won, float *identity_won,
                                         uint32_t *shared_all, void *workspace, size_t workspace_bytes,
                                         hipStream_t stream) {
    bool nothing;
    if (int e = results_check(index, index_bytes, r_sketches, r_sizes, num_refs, sketch_size, k, won, &nothing)) return e;
    if (nothing) return KMC_OK;
    const uint64_t slots = slots_within(index_bytes);
    int device = 0;  // (a caller's workspace is judged, and bound, without one)
    if (!workspace)
        if (hipError_t he = hipGetDevice(&device)) return (int)he;
    WLayout L;
    if (int e = bind_layout(w_ws, device, workspace, workspace_bytes, 8,
                            [&](void *b) { return winners_layout(b, slots, num_refs); }, &L))
        return e;
    if (hipError_t he = hipMemsetAsync(L.owner, 0, ((size_t)slots + 1) * 8, stream)) return (int)he;
    RArgs a{};
    a.index = const_cast<void *>(index);
    a.index_bytes = index_bytes;
    a.rows = r_sketches;
    a.sizes = r_sizes;
    a.n = (int64_t)num_refs;
    a.s = sketch_size;
    a.k = k;
    a.shared = shared_all ? shared_all : L.all;  // the first pass: results' shared, nothing else
    launch_results(a, false, stream);
    a.all = a.shared;
    a.owner = L.owner;
    a.owner_slots = slots;
    hipLaunchKernelGGL(screen_claim_kernel, dim3((unsigned)(a.n < kMaxGridX ? a.n : kMaxGridX)), dim3(kBlock), 0, stream, a);
    a.shared = won;
    a.median = median_won;
    a.identity = identity_won;
    launch_results(a, true, stream);
    return (int)hipGetLastError();
}
