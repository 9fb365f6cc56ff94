/*
 * kmc.h — C ABI of the MI355X-native k-mer counter (libkmc.so).
 *
 * Drop-in boundary for the hot path of axlwild/dna-kmeres-parallel: the step-1
 * launch of sumKmereCoincidencesGlobalMemory (kernels.h:113, launched at
 * main.cu:290) and its host-side feeders.  Plain C: pointers, sizes and int
 * error codes only (0 = success, hipError_t values pass through, library codes
 * are >= 1000).  Every device entry point is asynchronous on the given stream
 * and never calls exit(); the ones that return a size to the host say
 * "Synchronous" in their own comment (kmc_count_canonical_hash[_ex],
 * kmc_fasta_parse_device, kmc_fasta_load_device, kmc_fastq_parse_device,
 * kmc_fastq_load_device, kmc_fastq_next, and kmc_count_multi, which takes host
 * buffers).
 *
 * Count layout (identical to the reference, kernels.h:142): int32
 * sum[s + ld*code] ("k-mer-major, record-minor"), ld = num_seqs unless stated,
 * code = sum_p code(x[i+p]) * 4^p with A=0,C=1,G=2,T=3 (first base least
 * significant: the bin order of permutation(), utils.h:21-50).  Windows holding
 * any byte other than uppercase A/C/G/T are not counted (kernels.h:136-139);
 * their number per record is the reference CPU path's bin 0 (main.cu:643-644)
 * and is available through the optional `invalid` output.
 *
 * Records follow the reference's buffer convention (main.cu:474-545): record s
 * occupies data[indices[s] .. indices[s+1]), whose last byte is a terminator;
 * windows start at offsets 0 .. (indices[s+1]-indices[s]) - k - 1.
 */
#ifndef KMC_H
#define KMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libkmc.so is built with hidden visibility: exactly the entry points declared
 * here are exported (tests/test_abi.py compares `nm -D` with this header). */
#if defined(__GNUC__) || defined(__clang__)
#define KMC_API __attribute__((visibility("default")))
#else
#define KMC_API
#endif

#ifndef KMC_HIP_STREAM_T_DEFINED
#define KMC_HIP_STREAM_T_DEFINED
typedef struct ihipStream_t *hipStream_t; /* identical to HIP's own typedef */
#endif

/* Compile-time k of the exact drop-in entry point (the reference's K, kernels.h:11-15). */
#ifndef KMC_DROPIN_K
#define KMC_DROPIN_K 3
#endif

/* Largest k of the dense (4^k-bin) histogram path. */
#define KMC_DENSE_MAX_K 13

/* Reference loader cap (main.cu:30). */
#define KMC_MAX_SEQS_REFERENCE 100

enum kmc_status {
    KMC_OK = 0,
    KMC_ERR_INVALID_ARG = 1001,   /* null pointer, bad size, bad range */
    KMC_ERR_UNSUPPORTED_K = 1002, /* k outside the supported range of the entry point */
    KMC_ERR_ALIGNMENT = 1003,     /* pointer not aligned as the entry point requires */
    KMC_ERR_WORKSPACE = 1004,     /* caller workspace smaller than *_workspace_size() */
    KMC_ERR_IO = 1005,            /* file cannot be opened/read */
    KMC_ERR_NOMEM = 1006,         /* host or device allocation failed */
    KMC_ERR_RCCL = 1007,          /* RCCL call failed */
    KMC_ERR_NO_DEVICE = 1008,     /* no HIP device visible */
    KMC_ERR_CAPACITY = 1009,      /* caller output smaller than the result (size reported) */
    KMC_ERR_RECORD_TOO_LONG = 1010, /* a record has >= 2^31 windows in one dense call: int32 counts could wrap */
    KMC_ERR_INTERNAL = 1011,        /* a device-side bound check fired (a library defect): the access was
                                       skipped and the call's outputs are not valid (kmc_count_canonical_hash) */
    KMC_ERR_FORMAT = 1012           /* input is not well-formed FASTQ (kmc_fastq_*: the record's index is reported) */
};

/* Human-readable text for a kmc_status or hipError_t code (static storage). */
KMC_API const char *kmc_error_string(int code);

/* Library version: major*10000 + minor*100 + patch.  200 (0.2.0): kmc_dense_args
 * ends with `status` (below) and KMC_ERR_INTERNAL exists; a caller built against
 * an older header (0.1.0, a shorter kmc_dense_args) must not call
 * kmc_count_dense_ex on this library -- check kmc_version() >= 200 first. */
#define KMC_VERSION 200
KMC_API int kmc_version(void);

/* ------------------------------------------------------------------------ */
/* Exact drop-in for the reference launch
 *     sumKmereCoincidencesGlobalMemory<<<54018, PERMS_KMERES>>>(data, indices, num_seqs, sum)
 * (kernels.h:113, main.cu:290).  Same arguments, same meaning, same layout:
 *   data     device (or managed) bytes, '\0'-terminated records
 *   indices  device (or managed) int[num_seqs + 1] record offsets
 *   sum      device (or managed) int[4^KMC_DROPIN_K * num_seqs]; every entry
 *            (s < num_seqs, code < 4^K) is overwritten
 * k = KMC_DROPIN_K (3, like the reference).  No pattern table (c_perms) is
 * needed: codes are computed arithmetically in the reference's bin order.
 * Like the reference's char *data, `data` may point anywhere in a buffer (for
 * example data + off): the library rounds it down to 16 bytes internally and
 * biases the offsets (the rounded-down bytes share data's page and are never
 * counted).  Uses a library-owned device workspace (allocated on first use per device).
 * Asynchronous on `stream` (0 = the null stream); the reference synchronises
 * after the launch (main.cu:291), so should the caller. */
KMC_API int sumKmereCoincidencesGlobalMemory_hip(char *data, int *indices, unsigned num_seqs, int *sum,
                                         hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* k-generic, 64-bit-offset dense counter: the generalisation the reference's CPU
 * path (permutationsCountAll, main.cu:636-646) computes for any k, on the GPU.
 *   data        device pointer (any alignment), readable for [0, data_bytes)
 *   indices     device int64[num_seqs + 1]
 *   k           1 .. KMC_DENSE_MAX_K
 *   sum         device int32[4^k * num_seqs], overwritten (layout above)
 *   invalid     optional device int32[num_seqs]: invalid windows (CPU bin 0)
 *   workspace   device scratch of kmc_count_dense_workspace_size() bytes, or
 *               NULL to use a library-owned buffer, one per device, shared by
 *               every NULL-workspace call on that device: such calls must not
 *               overlap (one stream, or the caller serialises them), and they are
 *               not graph-capture safe.  Concurrent calls pass their own workspace.
 * The same holds for the NULL workspace of kmc_pair_distances.
 * Counts are int32 like the reference's (main.cu:598,637: int counters, and the
 * kernel's int sum, kernels.h:142), which never meets a record of 2^31 windows
 * (its loader's int offsets stop at 2 GiB).  The 64-bit offsets here do, so a call
 * in which some record has 2^31 or more windows in range (valid or not) reports
 * KMC_ERR_RECORD_TOO_LONG through the call's deferred status (below) rather than
 * passing bins or invalid counts that may have wrapped as valid: count such a record in
 * window ranges of fewer than 2^31 windows (kmc_count_dense_ex) and add the parts
 * in 64-bit integers.  The offsets live on the device, so the check runs there. */
KMC_API size_t kmc_count_dense_workspace_size(int k, uint64_t num_seqs, uint64_t data_bytes, int device);

KMC_API int kmc_count_dense(const char *data, const int64_t *indices, uint64_t num_seqs, uint64_t data_bytes,
                    int k, int32_t *sum, int32_t *invalid, void *workspace, size_t workspace_bytes,
                    hipStream_t stream);

/* Extended form used for sharding: counts only the windows whose start offset
 * lies in [win_lo, win_hi), reading only data[read_lo, read_hi) (a shard plus its
 * (k-1)-byte halo), and writes sum[s + sum_ld*code] for every record s (zeros for
 * records with no window in range).  Sums of shards covering disjoint window
 * ranges equal the unsharded counts. */
typedef struct kmc_dense_args {
    const char *data;        /* device; global byte p is data[p] (only [read_lo, read_hi) is read) */
    const int64_t *indices;  /* device int64[num_seqs + 1], global offsets */
    uint64_t num_seqs;
    int k;
    int32_t *sum;            /* device */
    uint64_t sum_ld;         /* row stride of sum (>= num_seqs); 0 -> num_seqs */
    int32_t *invalid;        /* optional device int32[num_seqs] */
    uint64_t read_lo, read_hi;
    uint64_t win_lo, win_hi;
    void *workspace;
    size_t workspace_bytes;
    int32_t *status;         /* optional device-visible int32 (device memory or host-mapped), zeroed by
                                the caller before the call: this call's kernels store a kmc_status code
                                in it (KMC_ERR_CAPACITY, KMC_ERR_RECORD_TOO_LONG) when its counts are
                                not valid; read it after the stream has synchronised.  NULL: the
                                device's library flag, reported by kmc_dense_status(). */
} kmc_dense_args;

KMC_API size_t kmc_count_dense_ex_workspace_size(const kmc_dense_args *args, int device);
KMC_API int kmc_count_dense_ex(const kmc_dense_args *args, hipStream_t stream);

/* Deferred device-side status of the asynchronous dense calls on `device` that
 * passed no status word of their own (kmc_count_dense, the drop-in, and
 * kmc_count_dense_ex with status == NULL).  Two conditions are detected on the
 * device, where the offsets live: (1) the k = 8 kernel keeps its 16-bit counters
 * exact with spill entries whose number per workgroup is bounded analytically (one
 * per >= 4096 windows); should a workgroup ever emit more than its workspace holds,
 * the counts would be short: KMC_ERR_CAPACITY; (2) a record with 2^31 or more
 * windows in range: KMC_ERR_RECORD_TOO_LONG (above).  The kernels store the code in
 * a host-mapped word of the device.  This call (after the stream has synchronised)
 * returns the code stored since the last query, KMC_OK if none, and clears it.
 * No other entry point reads or clears it, so a failure is never reported to an
 * unrelated later call; callers that run dense calls concurrently on one device
 * pass each call its own status word instead. */
KMC_API int kmc_dense_status(int device);

/* ------------------------------------------------------------------------ */
/* Sharding.  A shard counts the windows starting in
 * [win_lo, win_hi) and reads data[read_lo, read_hi) = its bytes plus a k-1 byte
 * halo.  kmc_plan_shards cuts the buffer [indices[0], indices[num_seqs]) into
 * nshards contiguous, byte-balanced ranges whose inner cut points are multiples
 * of `align` (0 -> 4096); a shard may be empty.  Host memory, no device needed. */
typedef struct kmc_shard {
    uint64_t win_lo, win_hi;
    uint64_t read_lo, read_hi;
} kmc_shard;

KMC_API int kmc_plan_shards(const int64_t *indices, uint64_t num_seqs, int k, int nshards, uint64_t align,
                    kmc_shard *out);

/* Single-process multi-GPU count of a host buffer (the C++ host driver's path):
 * shards the buffer over `ndev` devices (kmc_plan_shards), copies each shard +
 * halo to its device, counts it there (kmc_count_dense_ex) and sums the per-device
 * matrices with one RCCL all-reduce (int32, sum) over xGMI; the result
 * sum[s + num_seqs*code] (and optional invalid[s]) is copied back to host
 * memory.  devices == NULL -> 0 .. ndev-1 (distinct devices).  Synchronous.
 * One host thread per device streams its shard through pinned staging buffers,
 * so all devices load concurrently.  The RCCL communicators of a device set (keyed
 * by the sorted device list) are created on its first call, and each device's
 * stream, pinned staging and device buffers (grow-only) on its first use; all are
 * reused until kmc_multi_release().  Thread-safe: a call holds its devices (locked
 * in ascending order) from load to copy-back, so calls whose sets share a device
 * take turns (RCCL communicators are not reentrant), calls on disjoint sets run
 * concurrently, and a set whose collective failed is rebuilt by the next call.
 * Each shard's count carries its own status word: KMC_ERR_CAPACITY /
 * KMC_ERR_RECORD_TOO_LONG (kmc_count_dense_ex) are returned by this call.  A record
 * of 2^31 or more windows is refused up front (KMC_ERR_RECORD_TOO_LONG, checked on
 * the host offsets before any device work): its shards would each hold fewer, but
 * the all-reduce would add their int32 parts.  HIP failures after the all-reduce
 * return their hipError_t; KMC_ERR_RCCL only when an RCCL call failed.
 * Retention: the cached per-device buffers are sized to the largest shard + halo
 * seen (GBs per device for Gbase inputs) plus 64 MB of pinned staging, and are
 * held until kmc_multi_release().  kmc_set_reserved_cus does not apply here (the
 * worker threads count with every CU). */
KMC_API int kmc_count_multi(const char *data, const int64_t *indices, uint64_t num_seqs, uint64_t data_bytes, int k,
                    int ndev, const int *devices, int32_t *sum, int32_t *invalid);
/* Destroys the communicators and frees the per-device state cached by
 * kmc_count_multi (waits for calls in flight). */
KMC_API int kmc_multi_release(void);

/* ------------------------------------------------------------------------ */
/* Pairwise k-mer distance (the reference's step 2).
 * For every pair of records i < j:
 *     d(i,j) = 1 - (float)S_ij / (float)(min(len_i, len_j) - k + 1)
 *     S_ij   = sum over the 4^k codes of min(sum[i + ld*code], sum[j + ld*code])
 *     len_s  = indices[s+1] - indices[s] - 1
 * written to out[n*i - i*(i-1)/2 + (j-i) - (i+1)], the packed upper triangle of
 * getIdxTriangularMatrixRowMajor(i+1, j-i, n) (kernels.h:46-48), n(n-1)/2 floats.
 * S_ij is summed exactly in 64-bit integers, so the result is that of the CPU
 * path (sequentialKmerCount2, main.cu:604-619) bit for bit; it replaces the host
 * loop of num_seqs minKmeres2 launches (main.cu:326-335) with one launch.
 *   sum       device int32 count matrix of kmc_count_dense (row stride sum_ld,
 *             0 -> num_seqs); counts are taken as unsigned
 *   indices   device int64[num_seqs + 1]
 *   out       device float[num_seqs*(num_seqs-1)/2]
 *   workspace device scratch of kmc_pair_distances_workspace_size() bytes (0 when
 *             the pair matrix alone fills the GPU), or NULL for a library buffer
 * Exact while every record has fewer than 2^32 windows. */
KMC_API size_t kmc_pair_distances_workspace_size(uint64_t num_seqs, int k, int device);
KMC_API int kmc_pair_distances(const int32_t *sum, uint64_t sum_ld, const int64_t *indices, uint64_t num_seqs, int k,
                       float *out, void *workspace, size_t workspace_bytes, hipStream_t stream);

/* Exact drop-in for one reference launch
 *     minKmeres2<<<blocks, threads>>>(sums, mins, num_seqs, current_seq, indexes)
 * (kernels.h:85-109, launched per row at main.cu:327): the distances of record
 * current_seq to every later record, 4^KMC_DROPIN_K codes, summed in float in
 * code order as kernels.h:103 does (so bit-identical to the reference kernel
 * also when that float sum rounds).  Device int sums/indexes, float mins. */
KMC_API int minKmeres2_hip(int *sums, float *mins, int num_seqs, int current_seq, int *indexes, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Canonical k-mer counting, k <= 31 (BASELINE config C4).  No
 * reference counterpart (the reference's dense tables stop being feasible past
 * k ~ 13); window and record rules are the dense path's (windows i < len_s - k + 1
 * of each record, bytes other than A/C/G/T invalid).  Key of a valid window: its
 * 2-bit encoding A0 C1 G2 T3 with the FIRST base MOST significant (so key order is
 * lexicographic order), replaced by the key of its reverse complement when that is
 * smaller.  Flags:
 *   KMC_CANON_SOFTMASK  lowercase a/c/g/t count as their bases (soft-masked genomes)
 *   KMC_CANON_FORWARD   no reverse-complement folding (key = the window itself;
 *                       for k <= 13 these counts equal the dense histogram)
 * Output, per record s: the distinct keys of s and their counts in
 * keys/counts[rec_offsets[s] .. rec_offsets[s+1]) (order within a record
 * unspecified), rec_offsets device uint64[num_seqs + 1]; *num_distinct (host) =
 * rec_offsets[num_seqs].  If capacity < *num_distinct nothing is written except
 * rec_offsets and KMC_ERR_CAPACITY is returned (valid windows, <= data bytes,
 * always suffice).  data (any alignment, like the dense entry points) with
 * data[p] = byte p of the global offsets in `indices` (device int64[num_seqs + 1]).
 * Synchronous on `stream` (the distinct total is returned to the host).  The
 * workspace, about 20 bytes per window (no hash table lives in HBM), is
 * library-owned here (one per device, grown on demand, shared by the calls on that
 * device, which must not overlap); kmc_count_canonical_hash_ex takes the caller's
 * instead, of kmc_count_canonical_workspace_size() bytes (NULL: library-owned),
 * 256-byte aligned (KMC_ERR_ALIGNMENT otherwise; hipMalloc's pointers are).  The
 * size is that of a call on `device` (it depends on the device's CU count). */
#define KMC_CANON_MAX_K 31
#define KMC_CANON_SOFTMASK 1u
#define KMC_CANON_FORWARD 2u
KMC_API int kmc_count_canonical_hash(const char *data, const int64_t *indices, uint64_t num_seqs, int k, unsigned flags,
                             uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *rec_offsets,
                             uint64_t *num_distinct, hipStream_t stream);
/* Workspace bytes of a canonical call over records with these offsets (HOST
 * int64[num_seqs + 1], the same values as the call's device `indices`), on
 * `device`, valid for any alignment of `data`; 0 on bad arguments. */
KMC_API size_t kmc_count_canonical_workspace_size(const int64_t *host_indices, uint64_t num_seqs, int k, int device);
/* kmc_count_canonical_hash with a caller workspace (KMC_ERR_WORKSPACE when smaller
 * than the size above; NULL = the library-owned one).  Calls with their own
 * workspaces may run concurrently on different streams. */
KMC_API int kmc_count_canonical_hash_ex(const char *data, const int64_t *indices, uint64_t num_seqs, int k,
                                        unsigned flags, uint64_t *keys, uint32_t *counts, uint64_t capacity,
                                        uint64_t *rec_offsets, uint64_t *num_distinct, void *workspace,
                                        size_t workspace_bytes, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Pairwise distance from the sparse per-record lists of kmc_count_canonical_hash[_ex]
 * (step 2 for k <= 31, where no 4^k x num_seqs matrix exists): for every i < j
 *     d(i,j) = 1 - (float)S_ij / (float)(min(len_i, len_j) - k + 1)
 *     S_ij   = sum over the keys present in both records of min(count_i, count_j)
 * with len_s, the float expression and the packed upper triangle of
 * kmc_pair_distances; S_ij is summed exactly in 64-bit integers, so when the entries
 * are the non-zero bins of a dense matrix the result is kmc_pair_distances' bit for bit.
 *   keys, counts   device, num_entries elements: record s owns the entries
 *                  [rec_offsets[s], rec_offsets[s+1]), in any order, keys distinct
 *                  within the record (a repeated key: unspecified result, no stray
 *                  access); keys are opaque 64-bit values, counts taken as unsigned
 *   rec_offsets    device uint64[num_seqs + 1]; values are clamped to num_entries, so
 *                  keys/counts are never read at or beyond num_entries whatever it holds
 *   num_entries    the host value kmc_count_canonical_hash returned in *num_distinct
 *   indices        device int64[num_seqs + 1] record offsets (len_s only)
 *   out            device float[num_seqs*(num_seqs-1)/2]
 *   workspace      device scratch of kmc_pair_distances_sparse_workspace_size() bytes
 *                  (8 B per pair + 16 B per entry + the partition tables; it depends on
 *                  the device's CU count), or NULL for a library-owned buffer under the
 *                  rule of kmc_pair_distances' (NULL-workspace calls on a device must
 *                  not overlap); KMC_ERR_WORKSPACE when smaller than that size
 * Asynchronous on `stream`, no host read-back.  k in 1..KMC_CANON_MAX_K
 * (KMC_ERR_UNSUPPORTED_K); num_seqs < 2: KMC_OK, nothing written; num_seqs at most
 * KMC_SPARSE_MAX_SEQS (the record id is packed into 32 bits beside the count) and
 * num_entries at most 2^40, KMC_ERR_INVALID_ARG above, as for null rec_offsets,
 * indices or out, or null keys or counts with num_entries > 0.  The size query
 * returns 0 on bad arguments. */
#define KMC_SPARSE_MAX_SEQS 2147483648ull
KMC_API size_t kmc_pair_distances_sparse_workspace_size(uint64_t num_seqs, uint64_t num_entries, int device);
KMC_API int kmc_pair_distances_sparse(const uint64_t *keys, const uint32_t *counts, const uint64_t *rec_offsets,
                                      uint64_t num_entries, const int64_t *indices, uint64_t num_seqs, int k,
                                      float *out, void *workspace, size_t workspace_bytes, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* MinHash sketches and Mash distances (no reference counterpart): the distance
 * path for collections whose distinct k-mers do not fit, or whose n x n step over
 * every k-mer costs too much.  A record is reduced to its sketch_size smallest
 * distinct key hashes; distances come from those sorted lists alone, and sketches
 * made in separate calls (with one seed and sketch_size) may be concatenated.
 * The rows have three consumers: kmc_sketch_distances, all pairs of one row set;
 * the search of one row set (the queries) in another (the references):
 * kmc_sketch_distances_rect, every query against every reference, and
 * kmc_sketch_nearest, the best references of every query without that rectangle; and
 * kmc_sketch_cluster, the groups of one row set at a threshold without its pairs.
 * kmc_sketch_links[_rect] list the pairs of either shape that are within a threshold.
 *
 * kmc_sketch_from_counts: sketches of the per-record lists of
 * kmc_count_canonical_hash[_ex], with the list conventions of
 * kmc_pair_distances_sparse (record r owns [rec_offsets[r], rec_offsets[r+1]), any
 * order; offsets are clamped to num_entries and only compared against, nothing is
 * read at or beyond num_entries; keys are opaque 64-bit values, distinct within a
 * record: a repeated key gives an unspecified result and no stray access).
 *   min_count     an entry takes part iff counts[e] >= min_count; 0 and 1 both mean
 *                 every entry, and counts may then be NULL
 *   hash          h(key) = splitmix64 output 0 of the stream seeded with key ^ seed:
 *                     z = (key ^ seed) + 0x9E3779B97F4A7C15            (mod 2^64)
 *                     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *                     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *                     h = z ^ (z >> 31)
 *                 a bijection of the key, so distinct keys have distinct hashes
 *   sketch_sizes  device uint32[num_seqs]: min(sketch_size, participating entries of r)
 *   sketches      device uint64[num_seqs * sketch_size]: row r holds the sketch_sizes[r]
 *                 smallest hashes of record r, ascending, then UINT64_MAX to the end
 *                 of the row (a real hash may equal UINT64_MAX: sketch_sizes tells)
 *   workspace     device scratch of kmc_sketch_workspace_size() bytes (about 2 KB per
 *                 record), or NULL for a library-owned buffer under the rule of
 *                 kmc_pair_distances' (NULL-workspace calls on a device must not
 *                 overlap); KMC_ERR_WORKSPACE when smaller than that size
 * Exact for any content (a radix select over the 64 hash bits: no capacity, no
 * unlucky hash).  Asynchronous on `stream`, no host read-back; the work launched
 * depends on the host arguments only.  KMC_ERR_INVALID_ARG: sketch_size 0 or above
 * KMC_SKETCH_MAX_SIZE, num_entries above 2^40, null rec_offsets, sketches or
 * sketch_sizes, null keys with num_entries > 0, null counts with min_count > 1.
 * num_seqs == 0: KMC_OK.  The size query returns 0 on bad arguments.
 *
 * kmc_sketch_distances: for every i < j, with A and B the first sketch_sizes[i] and
 * sketch_sizes[j] values (sizes clamped to sketch_size) of rows i and j, assumed
 * ascending, U the min(sketch_size, |A u B|) smallest values of A u B, denom = |U|
 * and shared = |U n A n B| (Mash's merge rule):
 *     denom == 0       NaN
 *     shared == 0      1.0f
 *     shared == denom  +0.0f
 *     otherwise        J = shared / denom, d = -log(2J / (1 + J)) / k in double,
 *                      capped at 1.0, rounded to float
 * written to out[] in the packed upper triangle of kmc_pair_distances; shared and
 * denom (device uint32, same packing) receive the integer counts when non-NULL.
 * No workspace; asynchronous on `stream`.  k in 1..KMC_CANON_MAX_K
 * (KMC_ERR_UNSUPPORTED_K); num_seqs < 2: KMC_OK, nothing written; null sketches,
 * sketch_sizes or out, or a sketch_size outside 1..KMC_SKETCH_MAX_SIZE:
 * KMC_ERR_INVALID_ARG.
 *
 * kmc_sketch_from_sequences: the same rows and sizes straight from the record
 * buffer, without the canonical count: bit for bit what kmc_sketch_from_counts
 * (min_count <= 1) writes for the lists kmc_count_canonical_hash returns for the
 * same data, indices, k, flags, seed and sketch_size, so rows of both entry points
 * may be concatenated.  One pass over the bases; a workgroup keeps the sketch_size
 * smallest distinct hashes of the record it is in as a sorted set in LDS.  Exact
 * for any content (repeats, low complexity, fewer distinct k-mers than
 * sketch_size, records of no window): no capacity and no retry.  There is no
 * min_count: that filter needs the counts (kmc_sketch_accum_* below keeps them).
 *   data, indices, num_seqs, data_bytes  as kmc_count_dense: data a device pointer of
 *                 any alignment readable for [0, data_bytes), indices device
 *                 int64[num_seqs + 1] (offsets are clamped to [0, data_bytes])
 *   k, flags      windows, record rules, keys and flags of kmc_count_canonical_hash,
 *                 k in 1..KMC_CANON_MAX_K (KMC_ERR_UNSUPPORTED_K)
 *   workspace     device scratch of kmc_sketch_from_sequences_workspace_size() bytes,
 *                 8-byte aligned (KMC_ERR_ALIGNMENT), or NULL for a library-owned
 *                 buffer under kmc_pair_distances' rule; KMC_ERR_WORKSPACE when
 *                 smaller.  8 (num_seqs + 1) bytes of offsets and G (16 sketch_size
 *                 + 8) bytes of partial sets (each array rounded up to 256 bytes),
 *                 G = min(CUs, ceil((data_bytes / 16 + 3) / 1024)) walking
 *                 workgroups: it does not grow with the number of windows, and
 *                 grows with data_bytes only until G has reached the CU count.
 * Asynchronous on `stream`, no host read-back; the work launched depends on the
 * host arguments only.  KMC_ERR_INVALID_ARG: sketch_size 0 or above
 * KMC_SKETCH_MAX_SIZE, unknown flag bits, num_seqs above 2^40, null indices,
 * sketches or sketch_sizes, null data with data_bytes > 0.  num_seqs == 0: KMC_OK.
 * The size query returns 0 on bad arguments (and needs no device for those).
 *
 * kmc_sketch_from_sequences_grouped: one sketch per group of consecutive records (the
 * contigs of an assembly, the reads of a sample) instead of one per record.  Group g
 * owns the records [group_offsets[g], group_offsets[g+1]); row g holds the
 * sketch_size smallest distinct hashes over the valid windows of all of them,
 * ascending, then UINT64_MAX; sketch_sizes[g] the number kept.  Windows, validity,
 * keys, flags, k, seed and hash are kmc_sketch_from_sequences': no window spans two
 * records, so a group is the union of its records' k-mer sets, not their
 * concatenation.  With group_offsets = 0, 1, .., num_seqs the output is
 * kmc_sketch_from_sequences' bit for bit, and rows of separate calls concatenate.
 *   group_offsets device int64[num_groups + 1], ascending; values are clamped to
 *                 [0, num_seqs] on the device.  A descending pair makes an empty
 *                 group; otherwise offsets that do not ascend give an unspecified
 *                 result and no stray access.  Records outside
 *                 [group_offsets[0], group_offsets[num_groups]) are not sketched.
 *   sketches      device uint64[num_groups * sketch_size]
 *   sketch_sizes  device uint32[num_groups]; an empty group, or one whose records have
 *                 no valid window, gets size 0 and a row of UINT64_MAX
 *   workspace     as kmc_sketch_from_sequences, of
 *                 kmc_sketch_from_sequences_grouped_workspace_size() bytes: that
 *                 call's arrays and 8 (num_groups + 1) bytes of group offsets; it does
 *                 not grow with the number of windows
 * The LDS set of a walking workgroup lives as long as the group it is in, so a group
 * of many short records pays one threshold, one row and one merge per range, not one
 * per record.  Exact for any content; asynchronous on `stream`, no host read-back;
 * the work launched depends on the host arguments only; nothing a former call left
 * in the workspace is read.  Errors as kmc_sketch_from_sequences, and
 * KMC_ERR_INVALID_ARG for num_groups above 2^40 and for null group_offsets with
 * num_groups > 0.  num_groups == 0: KMC_OK.  num_seqs == 0: KMC_OK and nothing is
 * written (every group is empty; the caller knows it).
 *
 * kmc_sketch_merge_groups: row g of the output is the bottom-sketch_size of the union
 * of the input rows [group_offsets[g], group_offsets[g+1]) (offsets as above, clamped
 * to [0, num_rows]): the first sizes_in[r] values (clamped to sketch_size) of each,
 * assumed ascending and distinct within a row.  The bottom-s of a union is the
 * bottom-s of the union of the bottom-s sets, so merging the rows
 * kmc_sketch_from_sequences wrote gives what kmc_sketch_from_sequences_grouped
 * writes; it also groups the rows of kmc_sketch_from_counts (min_count per record)
 * and folds the rows of a collection sketched in several batches or on several
 * GPUs.  One workgroup per group; a row is left at its first run of values at or
 * above the current threshold.  No workspace; asynchronous on `stream`.  The output
 * must not overlap the input: KMC_ERR_INVALID_ARG when the byte ranges of
 * sketches_out and sketches_in, or of sizes_out and sizes_in, share a byte; also for
 * a sketch_size outside 1..KMC_SKETCH_MAX_SIZE, num_rows or num_groups above 2^40,
 * null group_offsets, sketches_out or sizes_out, null inputs with num_rows > 0.
 * num_groups == 0: KMC_OK.
 *
 * kmc_sketch_distances_rect: every query row against every reference row, by
 * kmc_sketch_distances' pair rule exactly (the same device function): shared, denom
 * and the float of query q and reference r go to out[q * num_refs + r], row-major,
 * and to shared[] and denom[] (device uint32, same indexing) when non-NULL.  Both row
 * sets share sketch_size; the pair is symmetric, and with both sets pointing at the
 * same rows out[i * n + j] is the triangle's entry (i, j) bit for bit, the diagonal
 * +0.0f for a non-empty row and NaN for an empty one.  No workspace; asynchronous
 * on `stream`; the work launched depends on the host arguments only.  k in
 * 1..KMC_CANON_MAX_K (KMC_ERR_UNSUPPORTED_K); num_queries == 0 or num_refs == 0:
 * KMC_OK, nothing written; otherwise KMC_ERR_INVALID_ARG for null rows, sizes or
 * out, a sketch_size outside 1..KMC_SKETCH_MAX_SIZE, or either count above
 * KMC_SPARSE_MAX_SEQS.
 *
 * kmc_sketch_nearest: for every query the `top` best references, without the
 * num_queries x num_refs matrix.
 *   participation reference r takes part for query q iff denom(q, r) > 0 and
 *                 shared(q, r) >= min_shared.  With min_shared = 0 unrelated
 *                 references (distance 1.0) take part, an empty reference among
 *                 them when the query is not empty (shared 0 of denom = the
 *                 query's size); a pair of two empty rows (NaN) never does.
 *   order         by the Jaccard estimate J = shared / denom, descending, the fractions
 *                 compared exactly (shared_a * denom_b against shared_b * denom_a);
 *                 equal J by ascending reference index.  The order is defined on the
 *                 integers, not on the float: it depends neither on the device's log
 *                 nor on the cap at 1.0.
 *   hit_counts    device uint32[num_queries]: min(top, participating references)
 *   hit_refs, hit_shared, hit_denom (device uint32), hit_dist (device float), each
 *                 [num_queries * top]: entry [q * top + i] is the i-th best of query q
 *                 for i < hit_counts[q]; the rest of each row holds UINT32_MAX, 0, 0
 *                 and NaN.  hit_shared, hit_denom and hit_dist may each be NULL;
 *                 hit_refs and hit_counts may not.  hit_dist is
 *                 kmc_sketch_distances_rect's float of that pair, bit for bit.
 *   limits        top in 1..KMC_NEAREST_MAX_TOP; num_refs <= 2^32 - 2 (the index is
 *                 32 bits and UINT32_MAX marks an empty slot); num_queries <=
 *                 KMC_SPARSE_MAX_SEQS
 *   workspace     device scratch of kmc_sketch_nearest_workspace_size() bytes, or NULL
 *                 for a library-owned buffer under kmc_pair_distances' rule
 *                 (NULL-workspace calls on a device must not overlap);
 *                 KMC_ERR_WORKSPACE when smaller.  The references are cut into S
 *                 slabs, each searched on its own and the survivors merged:
 *                     num_queries * S * top * 8  +  num_queries * S * 4  bytes
 *                 (each array rounded up to 256), S <= max(1, 2 CUs / T) with T the
 *                 number of query tiles (at most 32 queries each, fewer for a large
 *                 sketch_size or top) and never more than the reference chunks.  It
 *                 does not grow with num_refs beyond that.
 * Asynchronous on `stream`, no host read-back; the work launched depends on the
 * host arguments only; nothing a former call left in the workspace is read.
 * num_queries == 0: KMC_OK.  num_refs == 0: KMC_OK, every hit_counts[q] = 0 and the
 * rows filled as above (the sketch pointers may then be NULL).  k outside
 * 1..KMC_CANON_MAX_K: KMC_ERR_UNSUPPORTED_K.  KMC_ERR_INVALID_ARG for the limits, a
 * sketch_size outside 1..KMC_SKETCH_MAX_SIZE and, with num_queries > 0, null
 * hit_refs or hit_counts, or null rows or sizes with num_refs > 0.  The size query
 * returns 0 on bad arguments (and needs no device for those), and 0 when either
 * count is 0: no workspace is used then.
 *
 * kmc_sketch_cluster: the records of one row set grouped at a similarity threshold
 * (dereplication), without the triangle of their distances.
 *   link rule     records i < j are linked iff neither row is empty (so denom(i, j) > 0) and
 *                     (double)shared >= min_jaccard * (double)denom
 *                 with shared and denom exactly kmc_sketch_distances' (the same device
 *                 function; rows assumed ascending, sizes clamped to sketch_size).  One
 *                 IEEE double product and one compare of integers at most 16384: a host
 *                 that applies the rule to the triangle's counts gets the same links bit
 *                 for bit.  Like kmc_sketch_nearest's order the rule is defined on the
 *                 integers: it depends neither on the device's log nor on the cap at
 *                 1.0.  Two empty rows (denom 0) are never linked, and an empty row has
 *                 shared 0 of denom > 0 with a row that is not, which only min_jaccard
 *                 == 0 would accept: the rule leaves that pair out, so an empty row is
 *                 always a cluster of its own.  min_jaccard == 0 links every pair of
 *                 rows that are not empty; min_jaccard == 1 only pairs with shared ==
 *                 denom.
 *   clusters      the connected components of the link graph (single linkage)
 *   labels        device uint32[num_seqs]: the smallest record index of i's component,
 *                 the cluster's representative.  The input determines it, whatever
 *                 order the device links in.
 *   cluster_index device uint32[num_seqs], may be NULL: the rank of i's cluster among
 *                 all clusters ordered by representative, 0 .. C - 1
 *   num_clusters  device uint32, may be NULL: C
 *   workspace     device scratch of kmc_sketch_cluster_workspace_size() bytes, 8-byte
 *                 aligned (KMC_ERR_ALIGNMENT), or NULL for a library-owned buffer under
 *                 kmc_pair_distances' rule (NULL-workspace calls on a device must not
 *                 overlap); KMC_ERR_WORKSPACE when smaller.  The union-find parent of
 *                 every record, a representative flag per record, their exclusive scan
 *                 and the scan's partials:
 *                     4 n  +  4 n  +  8 (n + 1)  +  8 ceil(n / 4096)  bytes, n = num_seqs
 *                 (each array rounded up to 256).  The same for every call, whichever
 *                 optional output is asked for; it does not depend on the device.
 * Asynchronous on `stream`, no host read-back; the work launched depends on the host
 * arguments only; nothing a former call left in the workspace is read.  Errors, judged
 * before any device is touched: KMC_ERR_INVALID_ARG for a sketch_size outside
 * 1..KMC_SKETCH_MAX_SIZE, num_seqs above KMC_SPARSE_MAX_SEQS, a min_jaccard outside
 * [0, 1] or NaN, null labels, and null sketches or sketch_sizes with num_seqs > 0.
 * num_seqs == 0: KMC_OK, *num_clusters = 0 when it is given, nothing else is written.
 * num_seqs == 1: label 0, index 0, one cluster.  The size query returns 0 on bad
 * arguments and for num_seqs == 0, and needs no device.
 *
 * kmc_mash_jaccard_of_distance: the threshold of kmc_sketch_cluster for a Mash distance.
 * Host only, no device: e^(-k d) / (2 - e^(-k d)) in double, the J at which
 * -log(2J / (1 + J)) / k equals d, so a pair's distance is at most d exactly when its J
 * is at least this value.  NaN for d outside [0, 1] (or NaN) and for k outside
 * 1..KMC_CANON_MAX_K.
 *
 * kmc_sketch_links, kmc_sketch_links_rect: the pairs of rows within a distance, as a list
 * with their counts and distances (Mash's dist -d: the edge list of a collection), without
 * the triangle or the rectangle of all pairs.
 *   listed pairs  kmc_sketch_links: a pair (i, j) with i < j is listed iff kmc_sketch_cluster
 *                 links it at the same min_jaccard, exactly: neither row is empty and
 *                     (double)shared >= min_jaccard * (double)denom
 *                 with shared and denom kmc_sketch_distances' (the same device functions
 *                 for the counts and for the rule).  The components of the listed pairs are
 *                 kmc_sketch_cluster's clusters.  kmc_sketch_links_rect: every pair of a
 *                 query row q and a reference row r is judged by that rule, and an entry's
 *                 i is q, its j is r.  With both sets pointing at the same rows a row that
 *                 is not empty pairs with itself (shared == denom), and (a, b) and (b, a)
 *                 are both listed.
 *   links         device kmc_sketch_link[capacity], 16-byte aligned (KMC_ERR_ALIGNMENT):
 *                 entry e holds {i, j, shared, denom} of one listed pair
 *   dist          device float[capacity], may be NULL: dist[e] is the distance of entry e,
 *                 the float of kmc_sketch_distances[_rect] for that pair at this k, bit
 *                 for bit (the same device function)
 *   num_links     device uint64, required: after the call the number L of listed pairs,
 *                 whether or not they fit.  The call zeroes it itself, on `stream`.
 *   capacity      exactly min(L, capacity) entries are written, at positions 0 ..
 *                 min(L, capacity) - 1 of links and dist; they are distinct pairs of the
 *                 listed set; nothing is written at or beyond capacity.  capacity == 0
 *                 with links == NULL and dist == NULL is the count-only call.
 *   order         the input determines the set of entries.  Their order is unspecified
 *                 and may differ from call to call; when L > capacity, which entries are
 *                 kept is unspecified too.  A caller that needs all of them calls again
 *                 with capacity >= *num_links.
 * No workspace and no library-owned buffer: calls with different outputs may overlap.
 * Asynchronous on `stream`, no host read-back; the work launched depends on the host
 * arguments only.  Errors, judged before any device is touched and in this order: k outside
 * 1..KMC_CANON_MAX_K: KMC_ERR_UNSUPPORTED_K; KMC_ERR_INVALID_ARG for a sketch_size outside
 * 1..KMC_SKETCH_MAX_SIZE, a row count above KMC_SPARSE_MAX_SEQS, a min_jaccard outside
 * [0, 1] or NaN, a null num_links, null links with capacity > 0, and null rows or sizes
 * while there is a pair to judge; KMC_ERR_ALIGNMENT for links not 16-byte aligned.
 * num_seqs < 2, or num_queries == 0 or num_refs == 0: KMC_OK and *num_links = 0, nothing
 * else is written; the row pointers may then be NULL. */
#define KMC_SKETCH_MAX_SIZE 16384
#define KMC_NEAREST_MAX_TOP 1024
#define KMC_SKETCH_DEFAULT_SEED 42ull
KMC_API size_t kmc_sketch_workspace_size(uint64_t num_seqs, uint64_t num_entries, uint32_t sketch_size, int device);
KMC_API int kmc_sketch_from_counts(const uint64_t *keys, const uint32_t *counts, const uint64_t *rec_offsets,
                                   uint64_t num_entries, uint64_t num_seqs, uint32_t sketch_size, uint64_t seed,
                                   uint32_t min_count, uint64_t *sketches, uint32_t *sketch_sizes,
                                   void *workspace, size_t workspace_bytes, hipStream_t stream);
KMC_API int kmc_sketch_distances(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                                 uint32_t sketch_size, int k, float *out, uint32_t *shared, uint32_t *denom,
                                 hipStream_t stream);
KMC_API size_t kmc_sketch_from_sequences_workspace_size(uint64_t num_seqs, uint64_t data_bytes,
                                                        uint32_t sketch_size, int device);
KMC_API int kmc_sketch_from_sequences(const char *data, const int64_t *indices, uint64_t num_seqs,
                                      uint64_t data_bytes, int k, unsigned flags, uint32_t sketch_size,
                                      uint64_t seed, uint64_t *sketches, uint32_t *sketch_sizes,
                                      void *workspace, size_t workspace_bytes, hipStream_t stream);
KMC_API size_t kmc_sketch_from_sequences_grouped_workspace_size(uint64_t num_seqs, uint64_t num_groups,
                                                                uint64_t data_bytes, uint32_t sketch_size,
                                                                int device);
KMC_API int kmc_sketch_from_sequences_grouped(const char *data, const int64_t *indices, uint64_t num_seqs,
                                              uint64_t data_bytes, const int64_t *group_offsets,
                                              uint64_t num_groups, int k, unsigned flags, uint32_t sketch_size,
                                              uint64_t seed, uint64_t *sketches, uint32_t *sketch_sizes,
                                              void *workspace, size_t workspace_bytes, hipStream_t stream);
KMC_API int kmc_sketch_merge_groups(const uint64_t *sketches_in, const uint32_t *sizes_in, uint64_t num_rows,
                                    const int64_t *group_offsets, uint64_t num_groups, uint32_t sketch_size,
                                    uint64_t *sketches_out, uint32_t *sizes_out, hipStream_t stream);
KMC_API int kmc_sketch_distances_rect(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                                      const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                      uint32_t sketch_size, int k, float *out, uint32_t *shared, uint32_t *denom,
                                      hipStream_t stream);
KMC_API size_t kmc_sketch_nearest_workspace_size(uint64_t num_queries, uint64_t num_refs, uint32_t sketch_size,
                                                 uint32_t top, int device);
KMC_API int kmc_sketch_nearest(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                               const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                               uint32_t sketch_size, int k, uint32_t top, uint32_t min_shared,
                               uint32_t *hit_refs, uint32_t *hit_shared, uint32_t *hit_denom, float *hit_dist,
                               uint32_t *hit_counts, void *workspace, size_t workspace_bytes, hipStream_t stream);
KMC_API double kmc_mash_jaccard_of_distance(double max_dist, int k);
KMC_API size_t kmc_sketch_cluster_workspace_size(uint64_t num_seqs, int device);
KMC_API int kmc_sketch_cluster(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                               uint32_t sketch_size, double min_jaccard, uint32_t *labels, uint32_t *cluster_index,
                               uint32_t *num_clusters, void *workspace, size_t workspace_bytes, hipStream_t stream);
typedef struct kmc_sketch_link { uint32_t i, j, shared, denom; } kmc_sketch_link; /* 16 bytes */
KMC_API int kmc_sketch_links(const uint64_t *sketches, const uint32_t *sketch_sizes, uint64_t num_seqs,
                             uint32_t sketch_size, int k, double min_jaccard, kmc_sketch_link *links, float *dist,
                             uint64_t capacity, uint64_t *num_links, hipStream_t stream);
KMC_API int kmc_sketch_links_rect(const uint64_t *q_sketches, const uint32_t *q_sizes, uint64_t num_queries,
                                  const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                  uint32_t sketch_size, int k, double min_jaccard, kmc_sketch_link *links,
                                  float *dist, uint64_t capacity, uint64_t *num_links, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Screening a sequence set for the references it contains (containment; what Mash
 * calls a screen).  The entry points above compare sketches with sketches; a
 * bottom-s sketch of a mixture (a read set, a metagenome) holds only its most
 * abundant members, so a genome wholly contained in it still has a Jaccard estimate
 * near zero.  Here the values of every reference row are looked for among the hashes
 * of ALL valid windows of the mixture.  Four steps:
 *
 * kmc_sketch_screen_index_size: bytes of the index of num_refs rows of sketch_size
 * values, an opaque device blob the caller allocates (256-byte aligned; hipMalloc's
 * pointers are):
 *     256 + round256(4 C) + 8 C,   C = max(8, 4 num_refs sketch_size rounded up to a
 *                                  power of two)
 * a header, a uint32 multiplicity per slot and C 64-bit slots of an open-addressing
 * table, each array rounded up to 256 bytes.  It depends on the two numbers only and
 * needs no device; 0 on bad arguments (sketch_size outside 1..KMC_SKETCH_MAX_SIZE,
 * num_refs * sketch_size above KMC_SCREEN_MAX_VALUES).  num_refs == 0 gives the size
 * of the empty index (C = 8), so the size is monotone in both arguments.
 *
 * kmc_sketch_screen_build: fills the index with the distinct values among the first
 * min(r_sizes[r], sketch_size) values of every row (rows as the sketch entry points
 * write them; their order within a row does not matter here) and a zeroed
 * multiplicity per distinct value.  Values are opaque 64-bit numbers; UINT64_MAX
 * inside a row's size is a real value and is indexed like any other.  A value that
 * several rows hold is indexed once and shared by all of them.  Nothing a former use
 * left in the blob is read; building again zeroes the multiplicities.  index_bytes
 * below the size above: KMC_ERR_WORKSPACE.  num_refs == 0: KMC_OK; given an index
 * (checked as otherwise) it is made the empty index, and the row pointers may be NULL.
 *
 * kmc_sketch_screen_count: one pass over the records.  data, indices, num_seqs,
 * data_bytes, k, flags, the window rules and validity are kmc_sketch_from_sequences';
 * every valid window's hash (the hash above of its canonical key, with `seed`) that
 * is in the index adds 1 to that value's multiplicity.  It accumulates: several calls
 * on batches of a sample equal one call on their concatenation, so a read set larger
 * than device memory is screened batch by batch against one index (and shards
 * screened on several devices add up).  k, flags and seed must be those the
 * references were sketched with; that is the caller's business.  Multiplicities are
 * exact while fewer than 2^32 windows have been accumulated into an index; beyond
 * that they are modulo 2^32, with no stray access.  No workspace.  num_seqs == 0:
 * KMC_OK, the index is left as it is.
 *
 * kmc_sketch_screen_results: per row r of a row set (the one given to build, or any
 * other rows of any sketch_size: values not in the index count as absent; values are
 * assumed distinct within a row), with size = min(r_sizes[r], sketch_size):
 *   shared[r]       the number of the row's values with multiplicity > 0
 *   median_mult[r]  the lower median of the multiplicities of those found values
 *                   (ascending, element (shared - 1) / 2); 0 when shared == 0.  May
 *                   be NULL.
 *   identity[r]     Mash's containment identity.  May be NULL.
 *                     size == 0        NaN
 *                     shared == 0      +0.0f
 *                     shared == size   1.0f
 *                     otherwise        pow((double)shared / size, 1.0 / k), rounded to float
 * It does not modify the index: count, results, count, results is a valid sequence.
 * num_refs == 0: KMC_OK, nothing written.
 *
 * All three device calls are asynchronous on `stream`, with no host read-back; the
 * work launched depends on the host arguments only; no library-owned buffer is used,
 * so calls on different indexes may overlap (calls on one index are ordered by the
 * caller).  count and results learn the table's extent from the header build wrote
 * and check it against index_bytes on the device: on a blob that was never built the
 * result is unspecified, with no stray access.  On the host they refuse index_bytes
 * below the smallest index (kmc_sketch_screen_index_size(0, 1)) with
 * KMC_ERR_WORKSPACE.  Errors, judged before any device is touched: k outside
 * 1..KMC_CANON_MAX_K: KMC_ERR_UNSUPPORTED_K (count, results); KMC_ERR_INVALID_ARG
 * for a sketch_size outside 1..KMC_SKETCH_MAX_SIZE, num_refs * sketch_size above
 * KMC_SCREEN_MAX_VALUES, unknown flag bits, num_seqs above 2^40, a null index, null
 * rows or sizes with num_refs > 0, null shared, null indices, null data with
 * data_bytes > 0; then KMC_ERR_WORKSPACE; then KMC_ERR_ALIGNMENT for an index that
 * is not 256-byte aligned. */
#define KMC_SCREEN_MAX_VALUES 1073741824ull
KMC_API size_t kmc_sketch_screen_index_size(uint64_t num_refs, uint32_t sketch_size);
KMC_API int kmc_sketch_screen_build(const uint64_t *r_sketches, const uint32_t *r_sizes, uint64_t num_refs,
                                    uint32_t sketch_size, void *index, size_t index_bytes, hipStream_t stream);
KMC_API int kmc_sketch_screen_count(void *index, size_t index_bytes, const char *data, const int64_t *indices,
                                    uint64_t num_seqs, uint64_t data_bytes, int k, unsigned flags, uint64_t seed,
                                    hipStream_t stream);
KMC_API int kmc_sketch_screen_results(const void *index, size_t index_bytes, const uint64_t *r_sketches,
                                      const uint32_t *r_sizes, uint64_t num_refs, uint32_t sketch_size, int k,
                                      uint32_t *shared, uint32_t *median_mult, float *identity, hipStream_t stream);

/* Winner-takes-all results (Mash's screen -w), for a redundant reference collection.
 * In kmc_sketch_screen_results every row that holds a found value counts it as its own:
 * twenty strains of one species all report an identity near 1 when one is present.
 * Here every found value is credited to one row only, the best that holds it.
 *
 * kmc_sketch_screen_winners: the inputs of kmc_sketch_screen_results: a built and
 * counted index and a row set (the one given to build, or any other: values not in the
 * index are absent; values are assumed distinct within a row, a repeated value gives an
 * unspecified result and no stray access).  The rule is defined on integers only, like
 * kmc_sketch_nearest's order and kmc_sketch_cluster's links: it depends on no float and
 * no device pow.
 *   size[r]        min(r_sizes[r], sketch_size)
 *   all[r]         the number of the row's values with multiplicity > 0: exactly
 *                  kmc_sketch_screen_results' shared[r]
 *   ranking        row a ranks before row b iff all[a] * size[b] > all[b] * size[a], or
 *                  the products are equal and a < b (exact in 64 bits: both factors are
 *                  at most 16384).  A row with all == 0 holds no found value and never
 *                  competes.
 *   winner(v)      for every indexed value v with multiplicity > 0: the first row in
 *                  that ranking among the rows that hold v within their size.  One
 *                  round, from the first-pass counts, as Mash does it; not iterated.
 *   won[r]         the number of the row's values v with multiplicity > 0 and
 *                  winner(v) == r
 *   median_won[r]  the lower median of the multiplicities of those won values
 *                  (ascending, element (won - 1) / 2); 0 when won == 0.  May be NULL.
 *   identity_won[r] kmc_sketch_screen_results' formula on (won[r], size[r], k), by the
 *                  same device function: NaN for size 0, +0.0f for won == 0, 1.0f for
 *                  won == size, otherwise pow((double)won / size, 1.0 / k) rounded to
 *                  float.  May be NULL.
 *   shared_all[r]  all[r].  May be NULL.
 * UINT64_MAX within a row's size is a real value and takes part like any other.
 * Consequences: the sum of won over the rows is the number of distinct found values
 * that at least one row holds; won[r] <= all[r]; a row set with no value shared
 * between rows has won == all, and identity and median are then bit for bit those of
 * kmc_sketch_screen_results; the result does not depend on the order in which the
 * device processes rows.
 *   workspace      device scratch of kmc_sketch_screen_winners_workspace_size() bytes,
 *                  8-byte aligned (KMC_ERR_ALIGNMENT), or NULL for a library-owned buffer
 *                  under kmc_pair_distances' rule (NULL-workspace calls on a device must
 *                  not overlap); KMC_ERR_WORKSPACE when smaller.  One 64-bit owner word
 *                  for every slot an index of index_bytes can hold, one for UINT64_MAX,
 *                  and all[]:
 *                      8 (C' + 1)  +  4 num_refs  bytes (each array rounded up to 256),
 *                  C' the largest power of two in 8..2^32 with 256 + round256(4 C') +
 *                  8 C' <= index_bytes.  Host numbers only, no device; 0 on bad arguments
 *                  (index_bytes below the smallest index, num_refs above
 *                  KMC_SCREEN_MAX_VALUES) and for num_refs == 0; monotone in both.
 * It does not modify the index: count, winners, results, count, winners is a valid
 * sequence.  Asynchronous on `stream`, no host read-back; the work launched (one memset
 * of the owner words, the first pass, a claim and a recount) depends on the host
 * arguments only; nothing a former call left in the workspace is read.  The device
 * checks the slot count in the index's header against index_bytes and against the
 * owner words: on a blob that was never built the outputs are unspecified (they may
 * be left unwritten), with no stray access.  Errors, judged before any device is
 * touched, are those of kmc_sketch_screen_results in its order (null won for null
 * shared), then KMC_ERR_WORKSPACE and KMC_ERR_ALIGNMENT for the workspace.
 * num_refs == 0: KMC_OK, nothing written. */
KMC_API size_t kmc_sketch_screen_winners_workspace_size(size_t index_bytes, uint64_t num_refs);
KMC_API int kmc_sketch_screen_winners(const void *index, size_t index_bytes, const uint64_t *r_sketches,
                                      const uint32_t *r_sizes, uint64_t num_refs, uint32_t sketch_size, int k,
                                      uint32_t *won, uint32_t *median_won, float *identity_won,
                                      uint32_t *shared_all, void *workspace, size_t workspace_bytes,
                                      hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Sketching a sequence set of any size with a minimum k-mer abundance (Mash's -m).
 * In reads a large share of the distinct k-mers are sequencing errors seen once; they
 * fill the bottom of the hash range, so a bottom-s sketch of raw reads compares badly
 * with the assembly of the same organism.  kmc_sketch_from_sequences[_grouped] has no
 * counts, and kmc_count_canonical_hash counts per record, where every record is one
 * read.  The accumulator counts over ALL records of ALL batches, but only the k-mers
 * whose hash lies below a threshold, in a device hash table the handle owns:
 *
 * kmc_sketch_accum_create: a handle for sketches of sketch_size values with the
 * windows, validity, keys, flags, k, seed and hash of kmc_sketch_from_sequences.
 *   log2_slots  the table has C = 2^log2_slots slots of a key and a uint32 count,
 *               KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS .. KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS
 *               (16 slots .. 2^30); 0: the power of two at or above
 *               KMC_SKETCH_ACCUM_DEFAULT_SLOTS_PER_VALUE * sketch_size
 *   memory      kmc_sketch_accum_device_bytes(): 256 + 2 (8 C + 4 C) bytes and the
 *               workspace of kmc_sketch_from_counts for one record (each array rounded
 *               up to 256 bytes); host numbers only, 0 on bad arguments
 * The allocation is made and cleared on the current device before the call returns.
 *
 * kmc_sketch_accum_add: the valid windows of the records (data, indices, num_seqs,
 * data_bytes as kmc_sketch_from_sequences: any alignment, offsets clamped) join the
 * one multiset of canonical keys of all adds since create or reset.  With N the sum of
 * data_bytes so far, this call included (an upper bound of the windows), and j the
 * smallest integer with ceil(N / 2^j) <= C / 4, a window takes part iff its hash is
 * below 2^(64 - j); j never falls.  When a call raises j, the entries still below the
 * new bound first move, with their counts, to a second table of the same size.  A new
 * key is refused, and the smallest refused hash kept (`lost`), once C / 2 keys are
 * tracked or its probe chain is 256 slots long; nothing else happens then.  Counts
 * are exact while fewer than 2^32 windows have been added; beyond that they are
 * modulo 2^32, with no stray access.  num_seqs == 0: KMC_OK, N is unchanged.
 *
 * kmc_sketch_accum_finish: with limit = min(2^(64 - j), lost), unbounded when j = 0
 * and nothing was lost, every key with a hash below limit was tracked from its first
 * window on.  Among those, the keys with multiplicity >= min_count (0 and 1: every
 * key) are selected by kmc_sketch_from_counts itself, so the row is bit for bit what
 * the count -> sketch path gives for them.
 *   sketch_row       device uint64[sketch_size]: the smallest distinct hashes,
 *                    ascending, then UINT64_MAX
 *   sketch_size_out  device uint32: the number kept
 *   stats            device uint64[4], may be NULL:
 *                    [0] complete    1 iff *sketch_size_out == sketch_size or limit is
 *                                    unbounded: the row is the true bottom-s.  Else
 *                                    the row holds every qualifying hash below limit:
 *                                    an exact prefix of it, shorter than sketch_size
 *                                    (create the handle with more slots)
 *                    [1] limit       the exclusive bound; UINT64_MAX when unbounded
 *                    [2] tracked     keys tracked below limit
 *                    [3] qualifying  those of them with multiplicity >= min_count
 * It does not modify the accumulator: add, finish(1), finish(2), add, finish is a
 * valid sequence.  kmc_sketch_accum_reset: as after create, N = 0 and j = 0.
 * kmc_sketch_accum_free: releases everything (NULL: nothing).
 *
 * add, finish and reset are asynchronous on `stream`, with no host read-back; the
 * work launched depends on the host arguments and the handle's N and j only.  Calls
 * on one accumulator are ordered by the caller, on the device it was created on;
 * different accumulators may overlap (no library-owned buffer is used).  Errors,
 * judged before any device is touched: k outside 1..KMC_CANON_MAX_K:
 * KMC_ERR_UNSUPPORTED_K; KMC_ERR_INVALID_ARG for a sketch_size outside
 * 1..KMC_SKETCH_MAX_SIZE, unknown flag bits, log2_slots out of range, a null handle
 * or `out`, null sketch_row or sketch_size_out, num_seqs above 2^40, null indices,
 * null data with data_bytes > 0, an N that would reach 2^62.  KMC_ERR_NOMEM when
 * create cannot allocate. */
#define KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS 4
#define KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS 30
#define KMC_SKETCH_ACCUM_DEFAULT_SLOTS_PER_VALUE 4096
typedef struct kmc_sketch_accum kmc_sketch_accum;
KMC_API size_t kmc_sketch_accum_device_bytes(uint32_t sketch_size, uint32_t log2_slots);
KMC_API int kmc_sketch_accum_create(uint32_t sketch_size, int k, unsigned flags, uint64_t seed, uint32_t log2_slots,
                                    kmc_sketch_accum **out);
KMC_API int kmc_sketch_accum_add(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                 uint64_t data_bytes, hipStream_t stream);
KMC_API int kmc_sketch_accum_finish(kmc_sketch_accum *a, uint32_t min_count, uint64_t *sketch_row,
                                    uint32_t *sketch_size_out, uint64_t *stats, hipStream_t stream);
KMC_API int kmc_sketch_accum_reset(kmc_sketch_accum *a, hipStream_t stream);
KMC_API void kmc_sketch_accum_free(kmc_sketch_accum *a);

/* ------------------------------------------------------------------------ */
/* The abundance spectrum of everything added to an accumulator: how many distinct
 * k-mers were seen once, twice, ..., c times (jellyfish histo, kmc_tools histogram,
 * ntCard).  With limit and `all` exactly those of kmc_sketch_accum_finish (limit =
 * min(2^(64 - j), lost); all: j = 0 and nothing lost), every key with a hash below limit
 * was tracked from its first window on, so its count is exact; the hash is a bijection
 * of the key, so those keys are a uniform sample of the set's distinct k-mers at rate
 * limit / 2^64.  Their histogram times 2^64 / limit is an unbiased estimate of every bin
 * of the true spectrum, and with `all` it is the exact spectrum.
 *
 * kmc_spectrum_from_accum: an entry of the active table takes part iff it holds a key
 * and (all or its hash < limit).
 *   num_bins  2 .. KMC_SPECTRUM_MAX_BINS
 *   hist      device uint64[num_bins], overwritten: a participating entry with count c
 *             adds 1 to hist[min(c, num_bins - 1)]; the last bin saturates, and hist[0]
 *             is 0 unless a count wrapped at 2^32
 *   stats     device uint64[4], may be NULL:
 *             [0] exact    1 iff all
 *             [1] limit    the exclusive bound; UINT64_MAX when unbounded
 *             [2] entries  participating entries: finish's stats[2], the sum of hist
 *             [3] windows  the sum of their counts in 64 bits (the windows below limit),
 *                          not truncated by the last bin
 * It writes hist, stats and two scratch words of the handle only, neither the tables
 * nor what finish writes: add, spectrum, add, spectrum, finish, spectrum is a valid
 * sequence, and a spectrum after a finish equals the one before it.  Asynchronous on
 * `stream`, no host read-back; the launches depend on the table's size, num_bins and j
 * only; calls on one accumulator are ordered by the caller.  KMC_ERR_INVALID_ARG, judged
 * before any device is touched, for a null handle, a null hist, num_bins out of range.
 *
 * kmc_spectrum_summarize: host only, no device.  hist is a host copy of the histogram,
 * limit its stats[1]; B = num_bins.  Every double is one IEEE operation on the operands
 * stated beside its field.  The last bin is a tail and not a count: it is no rise and no
 * peak.  The valley is where the k-mers of sequencing errors end: the first bin that is
 * not above a NON-EMPTY next bin (the empty bins past the last count of an assembly's
 * spectrum are no valley: such a file gets min_abundance 1).  KMC_ERR_INVALID_ARG for a
 * null pointer, num_bins outside 2..KMC_SPECTRUM_MAX_BINS, limit == 0. */
#define KMC_SPECTRUM_MAX_BINS 8192
typedef struct kmc_spectrum_summary {
    double   scale;            /* limit == UINT64_MAX ? 1.0 : ldexp(1.0, 64) / (double)limit */
    uint64_t sampled_distinct; /* sum over c >= 1 of hist[c] */
    uint64_t sampled_total;    /* sum over c >= 1 of c * hist[c] (mod 2^64; the last bin at c = B - 1) */
    double   distinct;         /* scale * (double)sampled_distinct */
    double   total;            /* scale * (double)sampled_total */
    uint32_t valley;           /* smallest c in 1 .. B - 3 with hist[c] <= hist[c + 1] and hist[c + 1] > 0;
                                  0: none */
    uint32_t peak;             /* valley > 0: the c in valley + 1 .. B - 2 with the largest hist[c], the
                                  smallest such c on ties; else 0 */
    uint32_t min_abundance;    /* valley > 0 ? valley : 1 */
    uint32_t saturated;        /* hist[B - 1] > 0 */
    double   genome_size;      /* peak > 0 ? (scale * (double)(sum over c >= valley of c * hist[c], mod 2^64))
                                  / (double)peak : 0.0 */
} kmc_spectrum_summary;
KMC_API int kmc_spectrum_from_accum(kmc_sketch_accum *a, uint32_t num_bins, uint64_t *hist, uint64_t *stats,
                                    hipStream_t stream);
KMC_API int kmc_spectrum_summarize(const uint64_t *hist, uint32_t num_bins, uint64_t limit,
                                   kmc_spectrum_summary *out);

/* ------------------------------------------------------------------------ */
/* Matching records against everything added to an accumulator, per record: how many
 * of a read's k-mers are in the set (read recruitment, host or contaminant depletion,
 * reads made of k-mers seen once).  The accumulator is an exact counted k-mer set: it
 * holds every canonical key with a hash below limit with its exact count, so with
 * `all` the fraction hits / windows of a record is exact, and otherwise the table is a
 * uniform sample of the k-mers at rate limit / 2^64, the same sample for every
 * sequence hashed with the handle's seed: hits / sampled is an unbiased estimate of
 * the fraction of all the record's windows that are in the set.
 *
 * kmc_match_from_accum: data, indices, num_seqs, data_bytes as kmc_sketch_accum_add
 * (any alignment, offsets clamped); windows, validity, keys, flags, k, seed and hash are
 * the handle's; limit and `all` exactly those of kmc_sketch_accum_finish and
 * kmc_spectrum_from_accum (limit = min(2^(64 - j), lost); all: j = 0 and nothing lost).
 * A valid window is sampled iff all, or its hash < limit; a sampled window is a hit iff
 * its key is in the active table with count >= max(min_count, 1).
 *   windows  device uint32[num_seqs], may be NULL: the valid windows of record r
 *   sampled  device uint32[num_seqs], may be NULL: those of them that are sampled
 *   hits     device uint32[num_seqs]: those of them that are hits
 *            Every entry 0 .. num_seqs - 1 is overwritten (a record with no window:
 *            zeros); nothing a former call left there is read.  Exact while a record
 *            has fewer than 2^32 windows, modulo 2^32 beyond, with no stray access.
 *   stats    device uint64[4], may be NULL:
 *            [0] exact    1 iff all
 *            [1] limit    the exclusive bound; UINT64_MAX when unbounded
 *            [2] sampled  the sum of `sampled` over the records, in 64 bits
 *            [3] hits     the sum of `hits` over the records, in 64 bits
 * It only reads the accumulator and writes its outputs only: add, match, add, match,
 * finish, spectrum is a valid sequence, and finish and spectrum give the same bits with
 * and without a match in between.  Asynchronous on `stream`, no host read-back; the
 * launches depend on the host arguments and the handle's host state only; no workspace
 * and no library-owned buffer; calls on one accumulator are ordered by the caller.
 * KMC_ERR_INVALID_ARG, judged before any device is touched, for a null handle, a null
 * hits, a null indices, null data with data_bytes > 0, num_seqs above 2^40, data_bytes
 * of 2^62 or more.  num_seqs == 0: KMC_OK, nothing is written except stats when given,
 * with zeros in [2] and [3].
 * (The name follows kmc_spectrum_from_accum: the kmc_sketch_accum_* functions are the
 * handle's life cycle.) */
KMC_API int kmc_match_from_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                 uint64_t data_bytes, uint32_t min_count, uint32_t *windows, uint32_t *sampled,
                                 uint32_t *hits, uint64_t *stats, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Telling matched records apart by source: a label on the accumulator's k-mer set and
 * per-record votes (read binning, depletion with a host and a target, contamination
 * reports).  A source is one of up to KMC_CLASSIFY_MAX_SOURCES = 32 sequence sets,
 * numbered from 0.  A label is a uint32 bitmask per slot of the active table: bit g
 * means "source g holds this key".
 *
 * kmc_label_accum: data, indices, num_seqs, data_bytes as kmc_sketch_accum_add.
 * Every valid window that is sampled (all, or hash < limit; both exactly those of
 * kmc_sketch_accum_finish) is looked up in the active table by kmc_match_from_accum's
 * probe, and where its key is found the slot's label takes an atomic OR of
 * 1u << source.  A key below limit that was added is in the table, so the label of
 * every sampled window is exact.
 *   Read-only  counts, keys and the header are only read: finish, spectrum and match
 *              give the same bits with and without label calls in between, and
 *              labelling a source twice is labelling it once.
 *   Storage    4 C bytes in a second allocation that the handle owns, made by the first
 *              label call (that call allocates; everything after it is asynchronous on
 *              `stream`) and released by kmc_sketch_accum_free.
 *              kmc_sketch_accum_device_bytes is the size of a handle never labelled.
 *   Lifetime   the labels describe the table as it stands: a kmc_sketch_accum_add of at
 *              least one record and a kmc_sketch_accum_reset drop them (host state, no
 *              device work), and the first label call after that clears the array on
 *              its stream.  So the order is: all adds, then all labels, then classify.
 * KMC_ERR_INVALID_ARG, judged before any device is touched: a null handle, source >= 32,
 * num_seqs above 2^40, and with num_seqs > 0 null indices, null data with data_bytes >
 * 0, data_bytes of 2^62 or more.  KMC_ERR_NOMEM when the array cannot be allocated.
 * num_seqs == 0: KMC_OK, and the labels are established (allocated and cleared) all the
 * same.  (The name follows kmc_match_from_accum's note: the six kmc_sketch_accum_* functions
 * are the handle's life cycle.)
 *
 * kmc_classify_from_accum: kmc_match_from_accum with the votes.  windows, sampled, hits
 * and stats are bit for bit kmc_match_from_accum's for the same arguments (windows and
 * sampled may be NULL); a hit does not depend on the label.
 *   score(r, g)  for g < num_sources: the hit windows of record r whose label has bit g.
 *              Label bits at or above num_sources are ignored.
 *   best       device uint32[num_seqs]: the smallest g with the largest score when that
 *              score is above 0, else KMC_CLASSIFY_NONE
 *   best_hits  device uint32[num_seqs]: that score, or 0
 *   next_hits  device uint32[num_seqs]: the largest score among the other sources (0
 *              when num_sources == 1); next_hits == best_hits is a tie
 *   scores     may be NULL; else device uint32[num_seqs * num_sources], row r holding
 *              score(r, .).  best, best_hits and next_hits are the same bits with and
 *              without it.
 *              Every entry of every given output is overwritten; nothing a former call
 *              left in the outputs or the workspace is read.
 *   workspace  device scratch of kmc_classify_workspace_size() bytes, 8-byte aligned
 *              (KMC_ERR_WORKSPACE when smaller, then KMC_ERR_ALIGNMENT), or NULL for a
 *              library-owned buffer under kmc_pair_distances' rule (NULL-workspace calls
 *              on a device must not overlap).  It holds the partial score rows of the
 *              records cut between the launch's waves, two tagged rows of 32 words per
 *              wave: a few MB at most, growing with data_bytes up to the device's width
 *              and not at all with num_seqs * num_sources.  The query takes host numbers
 *              and the device's CU count only and returns 0 for arguments the call
 *              refuses.
 * Asynchronous on `stream`, no host read-back; the launches depend on the host arguments
 * and the handle's host state only; the result does not depend on where the launch cuts
 * the records.  It only reads the accumulator.  KMC_ERR_INVALID_ARG, judged before any
 * device is touched: the conditions of kmc_match_from_accum; a null best, best_hits or
 * next_hits; num_sources outside 1..32; a handle whose labels are not established (no
 * label call since create, the last add of records or the last reset).  num_seqs == 0:
 * KMC_OK, nothing is written except stats when given. */
#define KMC_CLASSIFY_MAX_SOURCES 32
#define KMC_CLASSIFY_NONE UINT32_MAX
KMC_API int kmc_label_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                   uint64_t data_bytes, uint32_t source, hipStream_t stream);
KMC_API size_t kmc_classify_workspace_size(uint64_t num_seqs, uint64_t data_bytes, uint32_t num_sources, int device);
KMC_API int kmc_classify_from_accum(kmc_sketch_accum *a, const char *data, const int64_t *indices, uint64_t num_seqs,
                                    uint64_t data_bytes, uint32_t num_sources, uint32_t min_count,
                                    uint32_t *windows, uint32_t *sampled, uint32_t *hits,
                                    uint32_t *best, uint32_t *best_hits, uint32_t *next_hits, uint32_t *scores,
                                    uint64_t *stats, void *workspace, size_t workspace_bytes, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* Tracing (the reference times step 1 with cudaEvents, main.cu:262-300): when set,
 * every following dense count call on this host thread records `before` right
 * before its histogram kernel and `after` right after it, on the call's stream,
 * so the caller can time the hot kernel alone.  NULL, NULL switches it off. */
#ifndef KMC_HIP_EVENT_T_DEFINED
#define KMC_HIP_EVENT_T_DEFINED
typedef struct ihipEvent_t *hipEvent_t; /* identical to HIP's own typedef */
#endif
KMC_API int kmc_trace_set_events(hipEvent_t before, hipEvent_t after);

/* ------------------------------------------------------------------------ */
/* Launch shaping for overlapped collectives (no reference counterpart): the k <= 8
 * dense kernel runs one 1024-thread workgroup per CU over static byte ranges, so a
 * CU that another kernel holds when a count starts (an RCCL all-reduce overlapping
 * the next step, bench.py at N > 1) delays the whole launch.  With n > 0 the
 * following dense calls issued from this host thread (like kmc_trace_set_events,
 * the setting is per thread: other threads' calls are unaffected) launch n
 * workgroups fewer, leaving n CUs to the concurrent kernel (0 <= n <= 64; 0 =
 * every CU, the default).  The workspace size depends on it: query
 * kmc_count_dense_ex_workspace_size after setting it, on the same thread. */
KMC_API int kmc_set_reserved_cus(int n);

/* ------------------------------------------------------------------------ */
/* Synthetic input generator (benchmark layout): num_records
 * records of record_len bases, each followed by one '\0'; base g (global index
 * first_base + r*record_len + i) is "ACGT"[(x_{g/32} >> 2*(g%32)) & 3] where x_n
 * is output n of splitmix64 seeded with `seed`.  Writes num_records*(record_len+1)
 * bytes.  kmc_synth_indices fills the matching int64 offsets on the host. */
KMC_API int kmc_synth_fill(char *data, uint64_t num_records, uint64_t record_len, uint64_t seed,
                   uint64_t first_base, hipStream_t stream);
KMC_API void kmc_synth_indices(int64_t *indices, uint64_t num_records, uint64_t record_len);
/* Bytes [lo, hi) of the same record stream with first_base = 0 (record r occupies
 * global bytes [r*(record_len+1), (r+1)*(record_len+1)), its last one '\0'),
 * written to data[0 .. hi-lo): what a rank of a strong-scaled job holds of the
 * one global buffer (its shard and halo) without generating whole records.
 * data 16-byte aligned; lo need not be. */
KMC_API int kmc_synth_fill_range(char *data, uint64_t lo, uint64_t hi, uint64_t record_len, uint64_t seed,
                         hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* FASTA loader (host), the successor of importSeqs / importSeqsNoNL
 * (main.cu:474-545 / 401-473) with identical record semantics, int64 offsets
 * and a streaming parser.
 *   dialect 0 = importSeqs: records end at a blank or '\r'-initial line (a '>'
 *               inside a record is sequence text);
 *   dialect 1 = importSeqsNoNL: records also end at a '>' header line.
 *   max_seqs  = the reference's MAX_SEQS cap (KMC_MAX_SEQS_REFERENCE keeps its
 *               behaviour, including the 101st record); <= 0 means unlimited.
 * The loaded buffer follows the reference convention ('|' bytes become '\0';
 * each record ends with '\0') and always carries num_seqs + 1 offsets. */
typedef struct kmc_fasta kmc_fasta;

KMC_API int kmc_fasta_load(const char *path, int dialect, int64_t max_seqs, kmc_fasta **out);
KMC_API uint64_t kmc_fasta_num_seqs(const kmc_fasta *f);
KMC_API const int64_t *kmc_fasta_indices(const kmc_fasta *f); /* num_seqs + 1 entries */
KMC_API const char *kmc_fasta_data(const kmc_fasta *f);
KMC_API uint64_t kmc_fasta_data_bytes(const kmc_fasta *f);
/* Number of entries the reference's indexes_aux would hold: num_seqs + 1, or
 * num_seqs when the input ends in a blank line (the reference then drops the end
 * sentinel and its kernel reads out of bounds). */
KMC_API uint64_t kmc_fasta_reference_num_indexes(const kmc_fasta *f);
KMC_API void kmc_fasta_free(kmc_fasta *f);

/* FASTA parsing on the GPU: the record rules of
 * kmc_fasta_load (importSeqs / importSeqsNoNL, main.cu:474-545 / 401-473) without
 * the MAX_SEQS cap, applied to raw FASTA bytes already in device memory, at HBM
 * speed instead of the reference's host getline loop.
 *   raw       device, 16-byte aligned, raw_bytes bytes of FASTA text
 *   data      device, 4-byte aligned, capacity data_cap >= raw_bytes + 1
 *   indices   device int64[indices_cap]; num_seqs + 1 entries are written
 * On return *num_seqs and *data_bytes describe the buffer exactly as
 * kmc_fasta_load would; KMC_ERR_CAPACITY (with *num_seqs set) when indices_cap <
 * *num_seqs + 1.  Synchronous on `stream`; library-owned scratch (~2 B per line). */
KMC_API int kmc_fasta_parse_device(const char *raw, uint64_t raw_bytes, int dialect, char *data, uint64_t data_cap,
                           int64_t *indices, uint64_t indices_cap, uint64_t *num_seqs, uint64_t *data_bytes,
                           hipStream_t stream);

/* File -> device record buffer: reads `path` through pinned staging buffers
 * into device memory (the read of one chunk overlapping the copy of the last) and
 * parses it there (kmc_fasta_parse_device).  With max_seqs > 0 and more records
 * than that, the reference's cap applies, which cuts mid-record; the file is then
 * loaded by kmc_fasta_load and copied instead.  *data (*data_bytes + 16 bytes) and
 * *indices (*num_seqs + 1 entries) are hipMalloc'ed; the caller hipFree's them.
 * Synchronous on `stream`. */
KMC_API int kmc_fasta_load_device(const char *path, int dialect, int64_t max_seqs, char **data, uint64_t *data_bytes,
                          int64_t **indices, uint64_t *num_seqs, hipStream_t stream);

/* ------------------------------------------------------------------------ */
/* FASTQ (no reference counterpart: read sets come off sequencers in this format).
 * Strict four-line FASTQ.  The input is split into lines on '\n'; one '\r' directly
 * before the '\n' is not part of the line, nor is a '\r' at the very end of a final
 * input that has no last '\n'.  Bytes after the last '\n' are a line when there are
 * any.  Record r is lines 4r .. 4r+3:
 *   4r    starts with '@' (the rest is ignored)
 *   4r+1  the sequence; may be empty
 *   4r+2  starts with '+' (the rest is ignored)
 *   4r+3  the quality, as long as the sequence
 * Multi-line FASTQ is refused, not guessed at: it breaks a rule above, or nobody can
 * tell it from four-line FASTQ.  Output follows the record convention above: record
 * r occupies data[indices[r] .. indices[r+1]), the sequence bytes verbatim, then one
 * '\0'.  No case folding and no '|' mapping (that is the reference's FASTA quirk): N
 * and lowercase bytes stay, and the counting rules and KMC_CANON_SOFTMASK decide
 * about them.  A record is complete when its fourth line is ended by '\n'; in a
 * final input also when that line runs to the end of the input.  In a final input
 * the lines after the last complete record must all be empty.
 *
 * kmc_fastq_parse_device: the complete records of raw[0, raw_bytes), on the GPU.
 *   raw       device, 16-byte aligned, raw_bytes < 2^33 bytes of FASTQ text
 *   final     non-zero: no more input follows raw (the last piece of a file)
 *   data      device, 4-byte aligned, capacity data_cap; data_cap >= raw_bytes / 2 + 1
 *             always suffices (a record's raw text is at least 2 len + 5 bytes) and a
 *             smaller one is refused: KMC_ERR_CAPACITY
 *   indices   device int64[indices_cap]; *num_seqs + 1 entries are written
 *   *consumed the raw offset just past the last complete record's last line;
 *             raw_bytes on success when final.  Without `final`, what follows the
 *             last complete record is left unconsumed and is not judged; no
 *             complete record (*consumed == 0, *num_seqs == 0) is a valid result.
 * KMC_ERR_CAPACITY, with *num_seqs set and nothing written, when indices_cap <
 * *num_seqs + 1.  raw_bytes == 0: KMC_OK, no record, indices[0] = 0.  Every complete
 * record is judged on the device before anything is written to data or indices, so
 * malformed input never overruns data_cap: KMC_ERR_FORMAT, *num_seqs the smallest
 * 0-based index of a record that breaks a rule, or the number of complete records
 * when only the leftover lines of a final input are at fault; nothing else is
 * promised about the outputs then.  KMC_ERR_INVALID_ARG (null pointers, raw_bytes
 * of 2^33 or more), KMC_ERR_ALIGNMENT and the data_cap refusal are returned before
 * any device is touched.  Synchronous on `stream`; library-owned scratch under
 * kmc_fasta_parse_device's rule (calls on a device must not overlap), 8 B per line
 * and 4 B per record. */
KMC_API int kmc_fastq_parse_device(const char *raw, uint64_t raw_bytes, int final, char *data, uint64_t data_cap,
                           int64_t *indices, uint64_t indices_cap, uint64_t *num_seqs, uint64_t *data_bytes,
                           uint64_t *consumed, hipStream_t stream);

/* File -> device record buffer, the whole-file twin of kmc_fasta_load_device on the
 * same staging code: one parse with final = 1.  *data (*data_bytes + 16 bytes) and
 * *indices (*num_seqs + 1 entries) are hipMalloc'ed; the caller hipFree's them.
 * max_seqs > 0 keeps the first max_seqs records, a plain truncation: *num_seqs =
 * max_seqs, *data_bytes = indices[max_seqs].  KMC_ERR_FORMAT: *num_seqs is the
 * record's index and no buffer is returned.  The raw bytes and the records are both
 * resident while it runs; files of 2^33 bytes and more (KMC_ERR_INVALID_ARG) and
 * pipes go through the reader below.  Synchronous on `stream`. */
KMC_API int kmc_fastq_load_device(const char *path, int64_t max_seqs, char **data, uint64_t *data_bytes,
                          int64_t **indices, uint64_t *num_seqs, hipStream_t stream);

/* Batch reader: a FASTQ file of any size as a sequence of record buffers, for
 * consumers that accumulate (kmc_sketch_screen_count).
 * kmc_fastq_open opens the file and touches no device (KMC_ERR_IO when it cannot).
 * batch_bytes == 0 means 256 MiB; any other value is rounded up to a multiple of 16
 * (2^32 and more: KMC_ERR_INVALID_ARG).  The reader only read()s until end of
 * file: it never seeks and never asks the size, so `path` may be a pipe
 * (/dev/stdin, a process substitution fed by zcat).
 * kmc_fastq_next reads up to batch_bytes new raw bytes behind the unconsumed tail of
 * the previous batch, copies them to the device through two pinned staging buffers
 * (the read of one chunk overlapping the copy of the last) and parses them
 * (kmc_fastq_parse_device, final exactly when end of file was reached).  It returns
 * device pointers the reader owns: *indices, *num_seqs + 1 offsets, and *data,
 * *data_bytes + 16 readable bytes.  A batch without a complete record before the
 * end of the file makes the raw buffer grow (doubling) and the read go on, so a
 * record longer than batch_bytes is handled; KMC_ERR_NOMEM when that fails.  After
 * the last batch every call returns KMC_OK with *num_seqs = 0, *data_bytes = 0 and
 * *data = NULL: the caller detects the end by *data == NULL.  KMC_ERR_FORMAT:
 * *num_seqs is the record's index within the whole file.  A reader that failed
 * returns the same code again.
 * Ordering: all device work of a call (copies, parse) is issued on `stream`, and the
 * returned buffers stay valid until the next call on the reader, whose writes are
 * stream-ordered behind whatever the caller enqueued on the same stream.  A caller
 * that counts each batch on that stream needs no synchronisation of its own, and
 * the host reads the next chunk while the GPU counts the last.  The call itself is
 * synchronous on `stream` (it returns sizes).  Device memory held: about 1.5 x
 * batch_bytes (the raw bytes and half as much for the records) plus the offsets,
 * unless a record forced growth; up to 128 MiB of pinned staging.
 * kmc_fastq_close frees everything (NULL: nothing). */
typedef struct kmc_fastq_reader kmc_fastq_reader;
KMC_API int kmc_fastq_open(const char *path, uint64_t batch_bytes, kmc_fastq_reader **out);
KMC_API int kmc_fastq_next(kmc_fastq_reader *rd, const char **data, uint64_t *data_bytes, const int64_t **indices,
                   uint64_t *num_seqs, hipStream_t stream);
KMC_API void kmc_fastq_close(kmc_fastq_reader *rd);

/* Where a record's raw text is.
 * kmc_fastq_parse_device_ex is kmc_fastq_parse_device with one more output:
 *   raw_indices  device int64[indices_cap], may be NULL (then it is
 *                kmc_fastq_parse_device, bit for bit).  raw_indices[r] is the raw
 *                offset of the '@' of record r; raw_indices[*num_seqs] is the offset
 *                just past the last complete record's fourth line: its '\n' included
 *                when there is one, raw_bytes when a final input ends without one.
 *                Records are contiguous in strict four-line FASTQ, so the full text
 *                of record r, line ends of either kind included, is
 *                raw[raw_indices[r], raw_indices[r+1]): (raw, raw_indices, num_seqs)
 *                is a record buffer for kmc_select_records.  *num_seqs + 1 entries
 *                are written; nothing when indices_cap is too small
 *                (KMC_ERR_CAPACITY); nothing is promised about them on KMC_ERR_FORMAT.
 * kmc_fastq_open_ex is kmc_fastq_open with flags; flags == 0 is kmc_fastq_open, any
 * bit but the ones below is KMC_ERR_INVALID_ARG.
 *   KMC_FASTQ_KEEP_RAW  the reader also keeps the raw offsets of every batch (8 more
 *                       bytes of device memory per record; nothing else changes)
 * kmc_fastq_raw returns the last batch's raw text and its num_seqs + 1 offsets: device
 * pointers the reader owns, valid exactly as long as that batch's data and indices
 * (until the next call on the reader, whose writes are stream-ordered behind the
 * caller's work); *raw_bytes = raw_indices[num_seqs] as a host value (the bytes
 * behind it, blank lines at the end of a file, belong to no record).
 * KMC_ERR_INVALID_ARG for a reader opened without KMC_FASTQ_KEEP_RAW, for null
 * arguments, and before the first kmc_fastq_next; a failed reader returns its code.
 * After the last batch (kmc_fastq_next returned *data == NULL): KMC_OK, *raw = NULL,
 * *raw_indices = NULL, *raw_bytes = 0.  No device is touched. */
#define KMC_FASTQ_KEEP_RAW 1u
KMC_API int kmc_fastq_parse_device_ex(const char *raw, uint64_t raw_bytes, int final, char *data, uint64_t data_cap,
                              int64_t *indices, uint64_t indices_cap, uint64_t *num_seqs, uint64_t *data_bytes,
                              uint64_t *consumed, int64_t *raw_indices, hipStream_t stream);
KMC_API int kmc_fastq_open_ex(const char *path, uint64_t batch_bytes, unsigned flags, kmc_fastq_reader **out);
KMC_API int kmc_fastq_raw(kmc_fastq_reader *rd, const char **raw, uint64_t *raw_bytes, const int64_t **raw_indices);

/* ------------------------------------------------------------------------ */
/* Selecting records (no reference counterpart): the reads that matched, or the reads
 * that did not, as one contiguous buffer in input order.
 *
 * kmc_select_records: stable compaction of byte records on the device.
 *   Records   record r is src[offsets[r], offsets[r+1]); offsets is a device
 *             int64[num_recs + 1], ascending, its values clamped to [0, src_bytes] on
 *             the device; offsets that do not ascend give an unspecified result and
 *             no stray access.  Records may be empty.  Bytes before offsets[0] and at
 *             or after offsets[num_recs] belong to no record and are dropped.  src may
 *             have any alignment (and so may dst).
 *   Selection keep is a device uint32[num_recs]; record r is selected iff
 *             (keep[r] != 0) != (invert != 0).  Any non-zero value counts, so the
 *             hits of kmc_match_from_accum are a valid keep.
 *   dst       receives the selected records' bytes concatenated in input order, bit
 *             for bit, nothing added or removed.
 *   dst_offsets  may be NULL; otherwise a device int64[num_recs + 1] of which the
 *             first kept + 1 entries are written: entry i is where the i-th selected
 *             record starts in dst, entry kept is the number of bytes kept.  So (dst,
 *             dst_offsets, kept) is again a record buffer under the convention above
 *             and can go straight into kmc_sketch_accum_add, kmc_match_from_accum and
 *             the rest.
 *   counts    required, device uint64[2]: the selected records and their bytes; both
 *             are written whether or not the bytes fit.
 *   Capacity  dst_cap >= src_bytes always suffices.  Nothing is ever written at or
 *             beyond dst + dst_cap; when counts[1] > dst_cap the content of dst is
 *             unspecified and the caller calls again.  dst may be NULL with dst_cap ==
 *             0: the count-only call (the pass over the source bytes is not launched).
 *   Overlap   dst must not overlap src: KMC_ERR_INVALID_ARG when [dst, dst + dst_cap)
 *             and [src, src + src_bytes) share a byte.
 *   workspace device scratch of kmc_select_records_workspace_size() bytes, 8-byte
 *             aligned (KMC_ERR_WORKSPACE when smaller, then KMC_ERR_ALIGNMENT), or NULL
 *             for a library-owned buffer under kmc_pair_distances' rule
 *             (NULL-workspace calls on a device must not overlap).  The size, with
 *             every array rounded up to 256 bytes: 4 n + 8 n + 8 (n + 1) + 8 (n + 1)
 *             + 8 (ceil(n / 4096) + 1) for n = num_recs; src_bytes does not enter.
 *             The query takes host numbers only and returns 0 for arguments the call
 *             refuses.
 * Asynchronous on `stream`, no host read-back; the launches depend on the host
 * arguments only; nothing a former call left in the workspace is read.
 * KMC_ERR_INVALID_ARG, judged before any device is touched: null offsets, keep or
 * counts; null src with src_bytes > 0; null dst with dst_cap > 0; num_recs above 2^40;
 * src_bytes of 2^62 or more.  num_recs == 0: KMC_OK, counts = {0, 0} and
 * dst_offsets[0] = 0 when given. */
KMC_API size_t kmc_select_records_workspace_size(uint64_t num_recs, uint64_t src_bytes);
KMC_API int kmc_select_records(const char *src, const int64_t *offsets, uint64_t num_recs, uint64_t src_bytes,
                       const uint32_t *keep, int invert, char *dst, uint64_t dst_cap, int64_t *dst_offsets,
                       uint64_t *counts, void *workspace, size_t workspace_bytes, hipStream_t stream);

/* kmc_match_select: the rule by which `kmc --recruit` lists a record, on the device:
 *   keep[r] = hits[r] >= min_hits && (double)hits[r] >= min_fraction * (double)sampled[r]
 * written as 1 or 0: one IEEE double product and one compare, so host and device
 * agree bit for bit.  sampled, hits (kmc_match_from_accum's) and keep are device
 * uint32[num_seqs]; sampled may be NULL when min_fraction == 0; num_kept is a device
 * uint64 (the number of ones) and may be NULL.  Match, select and kmc_select_records
 * chain on one stream without the host in between.  Asynchronous on `stream`, no
 * workspace.  KMC_ERR_INVALID_ARG, before any device is touched, for a min_fraction
 * outside [0, 1] or NaN, for null hits or keep with num_seqs > 0, for a null sampled
 * with num_seqs > 0 and min_fraction above 0, and for num_seqs above 2^40. */
KMC_API int kmc_match_select(const uint32_t *sampled, const uint32_t *hits, uint64_t num_seqs, uint32_t min_hits,
                     double min_fraction, uint32_t *keep, uint64_t *num_kept, hipStream_t stream);

/* kmc_classify_select: the rule by which `kmc --recruit --classify` assigns a record to
 * a source, on the device:
 *   keep[r] = listed[r] != 0 && best[r] == source && best_hits[r] - next_hits[r] >= min_margin
 * written as 1 or 0.  listed is kmc_match_select's keep and may be NULL, meaning all
 * ones; best, best_hits and next_hits are kmc_classify_from_accum's; keep may be the
 * same array as listed.  num_kept is a device uint64 (the number of ones) and may be
 * NULL.  min_margin 1 assigns a tie to nobody, 0 to the smaller index.  Asynchronous on
 * `stream`, no workspace.  KMC_ERR_INVALID_ARG, before any device is touched, for a
 * source >= 32, for a null best, best_hits, next_hits or keep with num_seqs > 0, and for
 * num_seqs above 2^40. */
KMC_API int kmc_classify_select(const uint32_t *listed, const uint32_t *best, const uint32_t *best_hits,
                                const uint32_t *next_hits, uint64_t num_seqs, uint32_t source, uint32_t min_margin,
                                uint32_t *keep, uint64_t *num_kept, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KMC_H */
