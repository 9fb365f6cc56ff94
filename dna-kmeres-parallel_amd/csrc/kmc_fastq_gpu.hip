// kmc_fastq_gpu.hip — FASTQ parsing on the GPU and the batch reader built on it
// (no reference counterpart: the reference reads FASTA only).
//
// Strict four-line FASTQ (include/kmc.h): the input is split into lines on '\n', one
// '\r' directly before the '\n' (or at the very end of a final input) is not part of
// the line, and record r is lines 4r .. 4r+3: '@' header, sequence, '+' line,
// quality of the sequence's length.  A line's role is its index mod 4, so unlike
// the FASTA parser no state has to be scanned over the lines.  Passes:
//   1. newlines per 16 KiB raw tile (fq_count_kernel) and their exclusive scan: the
//      line index of every tile's first byte, and the number of lines;
//   2. line starts: the thread that holds the j-th '\n' stores the offset after it
//      in lstart[j + 1] (fq_lstart_kernel), 8 bytes per line;
//   3. validation, one thread per complete record (fq_validate_kernel): its five
//      line starts give the four lines; len + 1 is stored per record and the
//      smallest index of a record that breaks a rule is kept with a 64-bit
//      atomicMin.  Nothing has been written to the caller's data and indices so
//      far; the first of the five line starts is the record's raw offset, stored
//      when the caller asked for them (kmc_fastq_parse_device_ex);
//   4. the exclusive scan of len + 1 over the records is `indices`;
//   5. write (fq_write_kernel), one pass over the raw tiles: byte p of line 4r + 1
//      goes to indices[r] + (p - lstart[4r + 1]), the byte that ends the sequence
//      (its '\n', or the '\r' before it) becomes the '\0'.  The bytes a tile keeps
//      are one contiguous output range, staged in LDS and stored as whole dwords.
// Threads whose 64 bytes hold no '\n' and lie in a header, '+' or quality line
// (more than half of a read file) leave pass 5 after their loads.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <new>

#include "kmc.h"
#include "kmc_scan.h"
#include "kmc_stage.h"
#include "kmc_text.h"
#include "kmc_workspace.h"

namespace kmc {
namespace {

constexpr int kFqVBlock = 256;  // records per block of the validation

struct QParams {
    const uint8_t *raw;
    int64_t n;            // raw bytes
    int final;
    int64_t ntiles;       // raw tiles
    uint32_t *tile_nl;    // [ntiles] newlines per tile
    uint64_t *tile_lb;    // [ntiles + 1] first line of each tile; [ntiles] = newlines
    uint64_t nl;          // newlines
    uint64_t nlines;      // lines: nl, + 1 when bytes follow the last '\n'
    uint64_t nrec;        // complete records
    uint64_t *lstart;     // [nl + 2] first byte of each line; [nl + 1] = n + 1 (as if raw[n] were '\n')
    uint32_t *reclen;     // [nrec] len + 1
    uint64_t *result;     // [2]: smallest bad record (UINT64_MAX: none), consumed
    uint8_t *out;
    uint64_t out_cap;
    const int64_t *idx;   // [nrec + 1], pass 5
    int64_t *rawidx;      // [nrec + 1] or null: where each record's raw text starts, and where the last one ends
};

// 1. newlines per tile
__global__ __launch_bounds__(kFpBlock) void fq_count_kernel(QParams p) {
    __shared__ uint32_t sh[kFpBlock / 64];
    uint32_t w[16];
    load64(p.raw, p.n, (int64_t)blockIdx.x * kFpTile + (int64_t)threadIdx.x * kFpPer, w);
    uint32_t total;
    block_excl_u32(count_nl(w), sh, total);
    if (threadIdx.x == 0) p.tile_nl[blockIdx.x] = total;
}

// 2. line starts
__global__ __launch_bounds__(kFpBlock) void fq_lstart_kernel(QParams p) {
    __shared__ uint32_t sh[kFpBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kFpTile + (int64_t)threadIdx.x * kFpPer;
    uint32_t w[16];
    load64(p.raw, p.n, q, w);
    uint32_t total;
    const uint32_t mine = count_nl(w);
    uint64_t j = p.tile_lb[blockIdx.x] + block_excl_u32(mine, sh, total);  // newlines before q
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.lstart[0] = 0;
        p.lstart[p.nl + 1] = (uint64_t)p.n + 1;
    }
    if (mine == 0) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uint32_t m = nl_bits(w[i]);
        while (m) {
            const int b = (__ffs((int)m) - 1) >> 3;
            m &= m - 1;
            if (++j <= p.nl) p.lstart[j] = (uint64_t)(q + 4 * i + b + 1);
        }
    }
}

// content of line l: [s, e), e before the '\n' (or the end of the input) and before one '\r' there
__device__ __forceinline__ void line_span(const QParams &p, uint64_t s, uint64_t next, uint64_t &e) {
    e = next - 1;
    if (e > s && p.raw[e - 1] == '\r') --e;
}

// 3. one thread per complete record; thread nrec judges what follows the records
__global__ __launch_bounds__(kFqVBlock) void fq_validate_kernel(QParams p) {
    const uint64_t r = (uint64_t)blockIdx.x * kFqVBlock + threadIdx.x;
    if (r < p.nrec) {
        uint64_t s[5], e[4];
#pragma unroll
        for (int i = 0; i < 5; ++i) s[i] = p.lstart[4 * r + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) line_span(p, s[i], s[i + 1], e[i]);
        const uint64_t len = e[1] - s[1];
        const bool ok = e[0] > s[0] && p.raw[s[0]] == '@' && e[2] > s[2] && p.raw[s[2]] == '+' && e[3] - s[3] == len;
        p.reclen[r] = (uint32_t)(len + 1);
        if (p.rawidx) p.rawidx[r] = (int64_t)s[0];
        if (!ok) atomicMin((unsigned long long *)&p.result[0], (unsigned long long)r);
    } else if (r == p.nrec) {
        // (lstart[nl + 1] = n + 1 stands for the '\n' a final input's last line lacks)
        if (p.rawidx) p.rawidx[r] = (int64_t)std::min<uint64_t>(p.lstart[4 * p.nrec], (uint64_t)p.n);
        if (p.final) {  // fewer than four lines are left over: all of them empty
            bool ok = true;
            for (uint64_t l = 4 * p.nrec; l < p.nlines; ++l) {
                uint64_t e;
                line_span(p, p.lstart[l], p.lstart[l + 1], e);
                ok = ok && e == p.lstart[l];
            }
            if (!ok) atomicMin((unsigned long long *)&p.result[0], (unsigned long long)p.nrec);
            p.result[1] = (uint64_t)p.n;
        } else {
            p.result[1] = p.lstart[4 * p.nrec];
        }
    }
}

// Output bytes written before raw position pos of line `line` (the kept bytes are a
// monotone compaction of the raw bytes: sequence content, then one terminator).
__device__ __forceinline__ uint64_t out_before(const QParams &p, uint64_t pos, uint64_t line) {
    if (line >= 4 * p.nrec) return (uint64_t)p.idx[p.nrec];
    const uint64_t r = line >> 2;
    const uint32_t role = (uint32_t)(line & 3);
    if (role == 0) return (uint64_t)p.idx[r];
    if (role != 1) return (uint64_t)p.idx[r + 1];
    const uint64_t a = (uint64_t)p.idx[r], kept = (uint64_t)p.idx[r + 1] - a;  // len + 1
    return a + std::min<uint64_t>(pos - p.lstart[line], kept);
}

// 5. write
__global__ __launch_bounds__(kFpBlock) void fq_write_kernel(QParams p) {
    __shared__ uint32_t sh[kFpBlock / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kFpTile + 8];
    const int64_t t0 = (int64_t)blockIdx.x * kFpTile, q = t0 + (int64_t)threadIdx.x * kFpPer;
    uint32_t w[16];
    load64(p.raw, p.n, q, w);
    uint32_t total;
    const uint32_t mine = count_nl(w);
    uint64_t line = p.tile_lb[blockIdx.x] + block_excl_u32(mine, sh, total);
    // the tile's output range (block-uniform)
    const int64_t t1 = std::min<int64_t>(t0 + kFpTile, p.n);
    const uint64_t ob = out_before(p, (uint64_t)t0, p.tile_lb[blockIdx.x]);
    const uint64_t oe = out_before(p, (uint64_t)t1, p.tile_lb[blockIdx.x + 1]);
    const uint32_t shift = (uint32_t)(ob & 3u);
    if (q < p.n && (mine != 0 || (line & 3) == 1)) {
        uint64_t cur = ~0ull, ls = 0, a = 0, kept = 0;  // of the current sequence line
        for (int i = 0; i < kFpPer; ++i) {
            if (q + i >= p.n) break;
            const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            if ((line & 3) == 1 && line < 4 * p.nrec) {
                if (line != cur) {
                    cur = line;
                    ls = p.lstart[line];
                    a = (uint64_t)p.idx[line >> 2];
                    kept = (uint64_t)p.idx[(line >> 2) + 1] - a;
                }
                const uint64_t o = (uint64_t)(q + i) - ls;
                if (o < kept) {
                    const uint64_t at = a + o - ob;  // < the tile's kept bytes
                    if (at < (uint64_t)kFpTile) stage[shift + at] = o + 1 == kept ? (uint8_t)0 : (uint8_t)b;
                }
            }
            line += b == '\n';
        }
    }
    __syncthreads();
    // (validated input: oe <= raw_bytes / 2 + 1 <= out_cap; the clamp costs nothing)
    const uint64_t end = std::min<uint64_t>(oe, p.out_cap);
    const uint32_t tk = end > ob ? (uint32_t)std::min<uint64_t>(end - ob, (uint64_t)kFpTile) : 0u;
    store_staged(p.out, stage, ob, tk);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
DeviceCache q_ws[2];  // [0]: per-tile arrays (sized from the raw bytes), [1]: per-line and per-record arrays

size_t q_tile_layout(void *base, QParams &p, uint64_t *&bsum) {
    Carver c(base);
    p.tile_nl = c.take<uint32_t>(p.ntiles);
    p.tile_lb = c.take<uint64_t>(p.ntiles + 1);
    bsum = c.take<uint64_t>(scan_tiles(p.ntiles) + 1);
    p.result = c.take<uint64_t>(2);
    return c.total();
}

size_t q_line_layout(void *base, QParams &p, uint64_t *&bsum) {
    Carver c(base);
    p.lstart = c.take<uint64_t>((size_t)p.nl + 2);
    p.reclen = c.take<uint32_t>((size_t)p.nrec);
    bsum = c.take<uint64_t>(scan_tiles((int64_t)p.nrec) + 1);
    return c.total();
}

// A record's length is scanned as a uint32: raw inputs of 2^33 bytes and more are
// parsed in pieces (the batch reader's business).
constexpr uint64_t kFqMaxRaw = 1ull << 33;

// Parses the complete records of raw[0, n); `get_idx(num_records)` supplies the
// offsets buffer (num_records + 1 entries) once the input is known to be well
// formed and the count is known, or returns null to stop with the count only.
// raw_idx(num_records) likewise supplies the buffer of the raw offsets, before the
// records are judged, or null for none.
template <class GetIdx, class GetRawIdx>
int fq_parse(const char *raw, uint64_t n, int final, char *out, uint64_t out_cap, GetIdx &&get_idx,
             GetRawIdx &&raw_idx, uint64_t *num_seqs, uint64_t *data_bytes, uint64_t *consumed, hipStream_t st) {
    *num_seqs = 0;
    *data_bytes = 0;
    *consumed = 0;
    hipError_t he;
    if (n == 0) {
        int64_t *idx = get_idx((uint64_t)0);
        if (!idx) return 0;
        const int64_t zero = 0;
        int64_t *ridx = raw_idx((uint64_t)0);
        if (ridx && (he = hipMemcpyAsync(ridx, &zero, 8, hipMemcpyHostToDevice, st))) return (int)he;
        if ((he = hipMemcpyAsync(idx, &zero, 8, hipMemcpyHostToDevice, st)) || (he = hipStreamSynchronize(st)))
            return (int)he;
        return 0;
    }
    QParams p{};
    p.raw = reinterpret_cast<const uint8_t *>(raw);
    p.n = (int64_t)n;
    p.final = final != 0;
    p.ntiles = (int64_t)((n + kFpTile - 1) / kFpTile);
    int device = 0;
    if ((he = hipGetDevice(&device))) return (int)he;
    void *ws = nullptr;
    uint64_t *bsum = nullptr;
    int e = q_ws[0].get(device, q_tile_layout(nullptr, p, bsum), &ws);
    if (e) return e;
    q_tile_layout(ws, p, bsum);
    // newlines -> lines and complete records
    hipLaunchKernelGGL(fq_count_kernel, dim3((unsigned)p.ntiles), dim3(kFpBlock), 0, st, p);
    excl_scan_u32(p.tile_nl, p.ntiles, bsum, p.tile_lb, st);
    uint8_t last = 0;
    const uint64_t none[2] = {~0ull, 0};
    if ((he = hipGetLastError()) || (he = hipMemcpyAsync(&p.nl, p.tile_lb + p.ntiles, 8, hipMemcpyDeviceToHost, st)) ||
        (he = hipMemcpyAsync(&last, raw + n - 1, 1, hipMemcpyDeviceToHost, st)) ||
        (he = hipMemcpyAsync(p.result, none, 16, hipMemcpyHostToDevice, st)) || (he = hipStreamSynchronize(st)))
        return (int)he;
    p.nlines = p.nl + (last != '\n');
    p.nrec = (p.final ? p.nlines : p.nl) / 4;
    if ((e = q_ws[1].get(device, q_line_layout(nullptr, p, bsum), &ws))) return e;
    q_line_layout(ws, p, bsum);
    p.rawidx = raw_idx(p.nrec);
    // line starts -> every record judged, before anything of the caller's is written
    hipLaunchKernelGGL(fq_lstart_kernel, dim3((unsigned)p.ntiles), dim3(kFpBlock), 0, st, p);
    hipLaunchKernelGGL(fq_validate_kernel, dim3((unsigned)(p.nrec / kFqVBlock + 1)), dim3(kFqVBlock), 0, st, p);
    uint64_t res[2];
    if ((he = hipGetLastError()) || (he = hipMemcpyAsync(res, p.result, 16, hipMemcpyDeviceToHost, st)) ||
        (he = hipStreamSynchronize(st)))
        return (int)he;
    if (res[0] != ~0ull) {
        *num_seqs = res[0];
        return KMC_ERR_FORMAT;
    }
    *num_seqs = p.nrec;
    *consumed = res[1];
    int64_t *idx = get_idx(p.nrec);
    if (!idx) return 0;  // count only
    p.idx = idx;
    p.out = reinterpret_cast<uint8_t *>(out);
    p.out_cap = out_cap;
    excl_scan_u32(p.reclen, (int64_t)p.nrec, bsum, reinterpret_cast<uint64_t *>(idx), st);
    if (p.nrec > 0) hipLaunchKernelGGL(fq_write_kernel, dim3((unsigned)p.ntiles), dim3(kFpBlock), 0, st, p);
    if ((he = hipGetLastError()) || (he = hipMemcpyAsync(data_bytes, idx + p.nrec, 8, hipMemcpyDeviceToHost, st)) ||
        (he = hipStreamSynchronize(st)))
        return (int)he;
    return 0;
}

// argument errors of a parse, judged before any device is touched
int fq_parse_args(const char *raw, uint64_t raw_bytes, const char *data, uint64_t data_cap, const int64_t *indices,
                  const uint64_t *num_seqs, const uint64_t *data_bytes, const uint64_t *consumed) {
    if (!num_seqs || !data_bytes || !consumed || !indices) return KMC_ERR_INVALID_ARG;
    if ((raw_bytes && (!raw || !data)) || raw_bytes >= kFqMaxRaw) return KMC_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(raw) & 15u) || (reinterpret_cast<uintptr_t>(data) & 3u)) return KMC_ERR_ALIGNMENT;
    if (raw_bytes && data_cap < raw_bytes / 2 + 1) return KMC_ERR_CAPACITY;
    return 0;
}

}  // namespace
}  // namespace kmc

using namespace kmc;

extern "C" int kmc_fastq_parse_device_ex(const char *raw, uint64_t raw_bytes, int final, char *data, uint64_t data_cap,
                                         int64_t *indices, uint64_t indices_cap, uint64_t *num_seqs,
                                         uint64_t *data_bytes, uint64_t *consumed, int64_t *raw_indices,
                                         hipStream_t stream) {
    if (int e = fq_parse_args(raw, raw_bytes, data, data_cap, indices, num_seqs, data_bytes, consumed)) return e;
    bool too_small = false;
    auto get_idx = [&](uint64_t nrec) -> int64_t * {
        if (indices_cap < nrec + 1) {
            too_small = true;
            return nullptr;
        }
        return indices;
    };
    auto raw_idx = [&](uint64_t nrec) -> int64_t * { return indices_cap < nrec + 1 ? nullptr : raw_indices; };
    const int rc = fq_parse(raw, raw_bytes, final, data, data_cap, get_idx, raw_idx, num_seqs, data_bytes, consumed,
                            stream);
    if (!rc && too_small) return KMC_ERR_CAPACITY;
    return rc;
}

extern "C" int kmc_fastq_parse_device(const char *raw, uint64_t raw_bytes, int final, char *data, uint64_t data_cap,
                                      int64_t *indices, uint64_t indices_cap, uint64_t *num_seqs,
                                      uint64_t *data_bytes, uint64_t *consumed, hipStream_t stream) {
    return kmc_fastq_parse_device_ex(raw, raw_bytes, final, data, data_cap, indices, indices_cap, num_seqs, data_bytes,
                                     consumed, nullptr, stream);
}

extern "C" int kmc_fastq_load_device(const char *path, int64_t max_seqs, char **data, uint64_t *data_bytes,
                                     int64_t **indices, uint64_t *num_seqs, hipStream_t stream) {
    if (!path || !data || !data_bytes || !indices || !num_seqs) return KMC_ERR_INVALID_ARG;
    *data = nullptr;
    *indices = nullptr;
    *data_bytes = 0;
    *num_seqs = 0;
    char *raw = nullptr;
    uint64_t n = 0, consumed = 0;
    int rc = stage_file(path, &raw, &n, stream);
    if (rc) return rc;
    if (n >= kFqMaxRaw) rc = KMC_ERR_INVALID_ARG;  // (a file this large goes through the batch reader)
    const uint64_t cap = n / 2 + 1;
    if (!rc && hipMalloc(data, cap + 16) != hipSuccess) rc = KMC_ERR_NOMEM;
    bool no_idx = false;
    auto get_idx = [&](uint64_t nrec) -> int64_t * {
        if (hipMalloc(indices, (nrec + 1) * 8) != hipSuccess) {
            *indices = nullptr;
            no_idx = true;
        }
        return *indices;
    };
    if (!rc) {
        rc = fq_parse(raw, n, 1, *data, cap, get_idx, [](uint64_t) -> int64_t * { return nullptr; }, num_seqs,
                      data_bytes, &consumed, stream);
        if (!rc && no_idx) rc = KMC_ERR_NOMEM;
    }
    (void)hipFree(raw);
    if (!rc && max_seqs > 0 && *num_seqs > (uint64_t)max_seqs) {  // the first max_seqs records
        *num_seqs = (uint64_t)max_seqs;
        rc = (int)hipMemcpy(data_bytes, *indices + max_seqs, 8, hipMemcpyDeviceToHost);
    }
    if (rc) {
        if (*data) (void)hipFree(*data);
        if (*indices) (void)hipFree(*indices);
        *data = nullptr;
        *indices = nullptr;
        if (rc != KMC_ERR_FORMAT) *num_seqs = 0;  // (KMC_ERR_FORMAT: the record's index)
        *data_bytes = 0;
    }
    return rc;
}

// ---------------------------------------------------------------------------
// the batch reader
// ---------------------------------------------------------------------------
struct kmc_fastq_reader {
    int fd = -1;
    uint64_t batch = 0;
    Stager stager;
    bool staged = false;       // the pinned buffers exist
    char *raw = nullptr;       // device: the unconsumed tail of the last batch, then the new bytes
    uint64_t raw_cap = 0, have = 0;
    uint64_t used = 0;         // raw[0, used) went into the last batch: dropped when the next call starts
    char *data = nullptr;      // device: the batch's records (data_cap + 16 bytes)
    uint64_t data_cap = 0;
    int64_t *idx = nullptr;    // device: their offsets
    uint64_t idx_cap = 0;
    bool keep_raw = false;     // KMC_FASTQ_KEEP_RAW
    int64_t *raw_idx = nullptr;  // device, idx_cap entries when keep_raw: the records' raw offsets
    uint64_t raw_end = 0;      // raw_idx[batch's records] on the host
    uint64_t batch_seqs = 0;   // records of the last batch
    int state = 0;             // 0: no batch yet, 1: a batch is held, 2: after the last batch
    uint64_t records = 0;      // records of the batches before this one
    bool eof = false, done = false;
    int failed = 0;            // a failed call's code: the reader stays failed
    uint64_t failed_at = 0;
};

namespace {

// at least `need` bytes at *buf (hipMalloc, + 16), the first `keep` bytes kept (copied on st)
int fq_grow(char **buf, uint64_t *cap, uint64_t need, uint64_t keep, hipStream_t st) {
    if (*cap >= need && *buf) return 0;
    char *nb = nullptr;
    const uint64_t ncap = (need + 15) & ~(uint64_t)15;
    if (hipMalloc(&nb, ncap + 16) != hipSuccess) return KMC_ERR_NOMEM;
    if (keep) {
        hipError_t he;
        if ((he = hipMemcpyAsync(nb, *buf, keep, hipMemcpyDeviceToDevice, st)) || (he = hipStreamSynchronize(st))) {
            (void)hipFree(nb);
            return (int)he;
        }
    }
    if (*buf) (void)hipFree(*buf);  // (waits for the work that still reads it)
    *buf = nb;
    *cap = ncap;
    return 0;
}

// raw[used, have) to raw[0, have - used) on st; the ranges may overlap
int fq_move_tail(kmc_fastq_reader *rd, hipStream_t st) {
    const uint64_t from = rd->used, tail = rd->have - from;
    rd->used = 0;
    hipError_t he = hipSuccess;
    if (from == 0 || tail == 0) {
    } else if (tail <= from) {
        he = hipMemcpyAsync(rd->raw, rd->raw + from, tail, hipMemcpyDeviceToDevice, st);
    } else {  // a short record before a long unfinished one: through a buffer of its own
        char *tmp = nullptr;
        if (hipMalloc(&tmp, tail) != hipSuccess) return KMC_ERR_NOMEM;
        if (!(he = hipMemcpyAsync(tmp, rd->raw + from, tail, hipMemcpyDeviceToDevice, st)) &&
            !(he = hipMemcpyAsync(rd->raw, tmp, tail, hipMemcpyDeviceToDevice, st)))
            he = hipStreamSynchronize(st);
        (void)hipFree(tmp);
    }
    rd->have = tail;
    return (int)he;
}

int fq_next(kmc_fastq_reader *rd, uint64_t *num_seqs, uint64_t *data_bytes, hipStream_t st) {
    if (!rd->staged) {
        if (int e = rd->stager.init((size_t)std::min<uint64_t>(rd->batch, kStageChunk))) return e;
        rd->staged = true;
    }
    if (int e = fq_move_tail(rd, st)) return e;
    uint64_t want = rd->batch;
    for (;;) {
        if (rd->have + want >= kFqMaxRaw) return KMC_ERR_NOMEM;
        if (int e = fq_grow(&rd->raw, &rd->raw_cap, rd->have + want, rd->have, st)) return e;
        uint64_t got = 0;
        if (!rd->eof)
            if (int e = rd->stager.feed(rd->fd, rd->raw + rd->have, want, &got, &rd->eof, st)) return e;
        rd->have += got;
        if (int e = fq_grow(&rd->data, &rd->data_cap, rd->have / 2 + 1, 0, st)) return e;
        uint64_t consumed = 0;
        for (;;) {  // (again with room for the offsets, when there are more records than ever before)
            if (!rd->idx) {
                rd->idx_cap = std::max<uint64_t>(rd->idx_cap, rd->have / 64 + 2);
                if (hipMalloc(&rd->idx, rd->idx_cap * 8) != hipSuccess) return KMC_ERR_NOMEM;
                if (rd->keep_raw && hipMalloc(&rd->raw_idx, rd->idx_cap * 8) != hipSuccess) return KMC_ERR_NOMEM;
            }
            const int rc = kmc_fastq_parse_device_ex(rd->raw, rd->have, rd->eof, rd->data, rd->data_cap, rd->idx,
                                                     rd->idx_cap, num_seqs, data_bytes, &consumed, rd->raw_idx, st);
            if (rc == KMC_ERR_CAPACITY && *num_seqs + 1 > rd->idx_cap) {
                (void)hipFree(rd->idx);
                rd->idx = nullptr;
                if (rd->raw_idx) (void)hipFree(rd->raw_idx);
                rd->raw_idx = nullptr;
                rd->idx_cap = *num_seqs + 1 + *num_seqs / 4;
                continue;
            }
            if (rc == KMC_ERR_FORMAT) *num_seqs += rd->records;
            if (rc) return rc;
            break;
        }
        if (*num_seqs > 0 || rd->eof) {
            rd->records += *num_seqs;
            rd->done = rd->eof;
            rd->used = rd->eof ? rd->have : consumed;
            rd->batch_seqs = *num_seqs;
            rd->raw_end = consumed;
            if (rd->keep_raw && rd->eof) {  // (blank lines may follow the last record of a file)
                int64_t end = 0;
                hipError_t he;
                if ((he = hipMemcpyAsync(&end, rd->raw_idx + *num_seqs, 8, hipMemcpyDeviceToHost, st)) ||
                    (he = hipStreamSynchronize(st)))
                    return (int)he;
                rd->raw_end = (uint64_t)end;
            }
            return 0;
        }
        want = std::max<uint64_t>(rd->have, rd->batch);  // no complete record yet: twice the bytes
    }
}

}  // namespace

extern "C" int kmc_fastq_open_ex(const char *path, uint64_t batch_bytes, unsigned flags, kmc_fastq_reader **out) {
    if (!path || !out) return KMC_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_bytes >= kFqMaxRaw / 2 || (flags & ~KMC_FASTQ_KEEP_RAW)) return KMC_ERR_INVALID_ARG;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return KMC_ERR_IO;
    kmc_fastq_reader *rd = new (std::nothrow) kmc_fastq_reader;
    if (!rd) {
        close(fd);
        return KMC_ERR_NOMEM;
    }
    rd->fd = fd;
    rd->batch = batch_bytes ? (batch_bytes + 15) & ~(uint64_t)15 : (256ull << 20);
    rd->keep_raw = (flags & KMC_FASTQ_KEEP_RAW) != 0;
    *out = rd;
    return 0;
}

extern "C" int kmc_fastq_open(const char *path, uint64_t batch_bytes, kmc_fastq_reader **out) {
    return kmc_fastq_open_ex(path, batch_bytes, 0u, out);
}

extern "C" int kmc_fastq_raw(kmc_fastq_reader *rd, const char **raw, uint64_t *raw_bytes, const int64_t **raw_indices) {
    if (!rd || !raw || !raw_bytes || !raw_indices) return KMC_ERR_INVALID_ARG;
    *raw = nullptr;
    *raw_indices = nullptr;
    *raw_bytes = 0;
    if (!rd->keep_raw) return KMC_ERR_INVALID_ARG;
    if (rd->failed) return rd->failed;
    if (rd->state == 0) return KMC_ERR_INVALID_ARG;
    if (rd->state == 2) return 0;
    *raw = rd->raw;
    *raw_indices = rd->raw_idx;
    *raw_bytes = rd->raw_end;
    return 0;
}

extern "C" int kmc_fastq_next(kmc_fastq_reader *rd, const char **data, uint64_t *data_bytes, const int64_t **indices,
                              uint64_t *num_seqs, hipStream_t stream) {
    if (!rd || !data || !data_bytes || !indices || !num_seqs) return KMC_ERR_INVALID_ARG;
    *data = nullptr;
    *indices = nullptr;
    *data_bytes = 0;
    *num_seqs = 0;
    if (rd->failed) {
        *num_seqs = rd->failed_at;
        return rd->failed;
    }
    if (rd->done) {
        rd->state = 2;
        return 0;
    }
    const int rc = fq_next(rd, num_seqs, data_bytes, stream);
    if (rc) {
        rd->failed = rc;
        rd->failed_at = rc == KMC_ERR_FORMAT ? *num_seqs : 0;
        *num_seqs = rd->failed_at;
        *data_bytes = 0;
        return rc;
    }
    rd->state = 1;
    *data = rd->data;
    *indices = rd->idx;
    return 0;
}

extern "C" void kmc_fastq_close(kmc_fastq_reader *rd) {
    if (!rd) return;
    rd->stager.release();
    if (rd->raw) (void)hipFree(rd->raw);
    if (rd->data) (void)hipFree(rd->data);
    if (rd->idx) (void)hipFree(rd->idx);
    if (rd->raw_idx) (void)hipFree(rd->raw_idx);
    if (rd->fd >= 0) close(rd->fd);
    delete rd;
}
