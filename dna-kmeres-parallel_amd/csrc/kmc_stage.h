// kmc_stage.h — file bytes -> device memory through two pinned staging buffers
// (host code only): the read() of chunk i + 1 overlaps the copy of chunk i.  Shared
// by the whole-file loaders (kmc_fasta_load_device, kmc_fastq_load_device) and the
// batch reader (kmc_fastq_next).  Only read() is used on the descriptor: no seek,
// no size, so it may be a pipe.
#pragma once

#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kmc.h"

namespace kmc {

constexpr size_t kStageChunk = 64u << 20;

class Stager {
public:
    Stager() = default;
    Stager(const Stager &) = delete;
    Stager &operator=(const Stager &) = delete;
    ~Stager() { release(); }

    // two pinned buffers of `chunk` bytes (called once, before feed)
    int init(size_t chunk) {
        chunk_ = std::max<size_t>(chunk, 16);
        for (int b = 0; b < 2; ++b) {
            if (hipHostMalloc(&pin_[b], chunk_, hipHostMallocDefault) != hipSuccess) return KMC_ERR_NOMEM;
            if (hipEventCreateWithFlags(&done_[b], hipEventDisableTiming) != hipSuccess) return KMC_ERR_NOMEM;
        }
        return 0;
    }

    // Reads up to `want` bytes of fd to dst[0, *got) (device), the copies issued on
    // st; *got < want only at end of file (*eof).  Returns without waiting for the
    // last copies: they are ordered on st, and a staging buffer is reused only
    // behind the event of its last copy, across calls too.
    int feed(int fd, char *dst, uint64_t want, uint64_t *got, bool *eof, hipStream_t st) {
        *got = 0;
        *eof = false;
        while (*got < want && !*eof) {
            const int b = (int)(turn_ & 1);
            if (turn_ >= 2)
                if (hipError_t he = hipEventSynchronize(done_[b])) return (int)he;
            const size_t room = (size_t)std::min<uint64_t>(chunk_, want - *got);
            size_t have = 0;
            while (have < room) {
                const ssize_t r = read(fd, pin_[b] + have, room - have);
                if (r < 0) return KMC_ERR_IO;
                if (r == 0) {
                    *eof = true;
                    break;
                }
                have += (size_t)r;
            }
            if (have == 0) break;
            if (hipError_t he = hipMemcpyAsync(dst + *got, pin_[b], have, hipMemcpyHostToDevice, st)) return (int)he;
            if (hipError_t he = hipEventRecord(done_[b], st)) return (int)he;
            ++turn_;
            *got += have;
        }
        return 0;
    }

    // waits for the copies in flight, then frees the buffers
    void release() {
        for (int b = 0; b < 2; ++b) {
            if (done_[b]) {
                if (turn_ > (uint64_t)b) (void)hipEventSynchronize(done_[b]);
                (void)hipEventDestroy(done_[b]);
            }
            if (pin_[b]) (void)hipHostFree(pin_[b]);
            done_[b] = nullptr;
            pin_[b] = nullptr;
        }
    }

private:
    char *pin_[2] = {nullptr, nullptr};
    hipEvent_t done_[2] = {nullptr, nullptr};
    size_t chunk_ = 0;
    uint64_t turn_ = 0;
};

// The twin of Stager, device memory -> file through two pinned buffers: the copy of
// chunk i + 1 overlaps the write() of chunk i.  Only write() is used on the
// descriptor, so it may be a pipe.
class Drainer {
public:
    Drainer() = default;
    Drainer(const Drainer &) = delete;
    Drainer &operator=(const Drainer &) = delete;
    ~Drainer() { release(); }

    // two pinned buffers of `chunk` bytes (called once, before drain)
    int init(size_t chunk) {
        chunk_ = std::max<size_t>(chunk, 16);
        for (int b = 0; b < 2; ++b) {
            if (hipHostMalloc(&pin_[b], chunk_, hipHostMallocDefault) != hipSuccess) return KMC_ERR_NOMEM;
            if (hipEventCreateWithFlags(&done_[b], hipEventDisableTiming) != hipSuccess) return KMC_ERR_NOMEM;
        }
        return 0;
    }

    // Writes src[0, bytes) (device; the copies issued on st, behind the work that fills
    // src) to fd.  Returns when every byte is written: KMC_ERR_IO for a failed or
    // short write.
    int drain(int fd, const char *src, uint64_t bytes, hipStream_t st) {
        uint64_t sent = 0;     // bytes whose copy is issued
        size_t len[2] = {0, 0};
        int pending = -1;      // the buffer whose copy is in flight
        while (sent < bytes || pending >= 0) {
            int issued = -1;
            if (sent < bytes) {
                issued = pending < 0 ? 0 : 1 - pending;
                len[issued] = (size_t)std::min<uint64_t>(chunk_, bytes - sent);
                if (hipError_t he = hipMemcpyAsync(pin_[issued], src + sent, len[issued], hipMemcpyDeviceToHost, st))
                    return (int)he;
                if (hipError_t he = hipEventRecord(done_[issued], st)) return (int)he;
                sent += len[issued];
            }
            if (pending >= 0) {  // the last chunk goes to the file while this one is copied
                if (hipError_t he = hipEventSynchronize(done_[pending])) return (int)he;
                size_t put = 0;
                while (put < len[pending]) {
                    const ssize_t w = write(fd, pin_[pending] + put, len[pending] - put);
                    if (w <= 0) return KMC_ERR_IO;
                    put += (size_t)w;
                }
            }
            pending = issued;
        }
        return 0;
    }

    void release() {
        for (int b = 0; b < 2; ++b) {
            if (done_[b]) {
                (void)hipEventSynchronize(done_[b]);  // (a copy a failed drain left in flight)
                (void)hipEventDestroy(done_[b]);
            }
            if (pin_[b]) (void)hipHostFree(pin_[b]);
            done_[b] = nullptr;
            pin_[b] = nullptr;
        }
    }

private:
    char *pin_[2] = {nullptr, nullptr};
    hipEvent_t done_[2] = {nullptr, nullptr};
    size_t chunk_ = 0;
};

// The whole of a regular file in device memory: *raw (hipMalloc, *n + 16 bytes; the
// caller frees it), the copies complete on return.
inline int stage_file(const char *path, char **raw, uint64_t *n, hipStream_t st) {
    *raw = nullptr;
    *n = 0;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return KMC_ERR_IO;
    const off_t size = lseek(fd, 0, SEEK_END);
    if (size < 0 || lseek(fd, 0, SEEK_SET) != 0) {
        close(fd);
        return KMC_ERR_IO;
    }
    int rc = 0;
    if (hipMalloc(raw, (uint64_t)size + 16) != hipSuccess) {
        *raw = nullptr;
        rc = KMC_ERR_NOMEM;
    }
    Stager stager;
    uint64_t got = 0;
    bool eof = false;
    if (!rc) rc = stager.init(kStageChunk);
    if (!rc && size > 0) rc = stager.feed(fd, *raw, (uint64_t)size, &got, &eof, st);
    close(fd);
    if (!rc && got != (uint64_t)size) rc = KMC_ERR_IO;  // the file shrank under the read
    if (!rc)
        if (hipError_t he = hipStreamSynchronize(st)) rc = (int)he;
    if (rc && *raw) {
        (void)hipFree(*raw);
        *raw = nullptr;
    }
    *n = rc ? 0 : (uint64_t)size;
    return rc;
}

}  // namespace kmc
