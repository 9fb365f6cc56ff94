// kmc_workspace.h — host-side workspace plumbing shared by the .hip translation
// units (no kernels, no device code): the 256-byte rounding of every layout, the
// carver that lays a workspace out, the per-device grow-only scratch buffer, the
// choice between it and a caller's workspace, the dispatch on k, the cached CU count of a device, and
// the two steps most entry points open with: the current device with its CU count,
// and a layout sized, bound and laid out (bind_layout).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>

#include "kmc.h"

namespace kmc {

inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// Lays a workspace out as consecutive arrays, each rounded up to 256 bytes.  A
// layout is written once, as a run of take() calls: over the workspace they bind
// the pointers, over no base (address 0: integer arithmetic, no pointer is formed
// from null and offset) the same calls give total(), the size to ask for.
class Carver {
public:
    explicit Carver(void *base = nullptr) : at_(reinterpret_cast<uintptr_t>(base)), base_(at_) {}
    template <class T>
    T *take(size_t count) {
        T *p = reinterpret_cast<T *>(at_);
        at_ += round256(count * sizeof(T));
        return p;
    }
    // an array only some modes have: no bytes and a null pointer in the others
    template <class T>
    T *take_if(bool on, size_t count) {
        return on ? take<T>(count) : nullptr;
    }
    size_t total() const { return at_ - base_; }

private:
    uintptr_t at_, base_;
};

// A library-owned scratch buffer per device that only grows: a larger request
// frees the buffer and allocates anew.  Every subsystem keeps its own instance
// (calls of different subsystems on different streams never share a buffer).  The
// lock covers the lookup and the growth, not the caller's launches.
class DeviceCache {
public:
    int get(int device, size_t need, void **out) {
        std::lock_guard<std::mutex> lk(mu_);
        if ((int)buf_.size() <= device) buf_.resize(device + 1);
        Buf &c = buf_[device];
        if (c.bytes < need) {
            if (c.ptr) {
                const hipError_t e = hipFree(c.ptr);
                if (e != hipSuccess) return (int)e;
                c.ptr = nullptr;
                c.bytes = 0;
            }
            if (hipMalloc(&c.ptr, need) != hipSuccess) return KMC_ERR_NOMEM;
            c.bytes = need;
        }
        *out = c.ptr;
        return 0;
    }

private:
    struct Buf {
        void *ptr = nullptr;
        size_t bytes = 0;
    };
    std::mutex mu_;
    std::vector<Buf> buf_;
};

// The workspace of one call, `need` bytes: the caller's when it gave one (size checked first,
// then `align`, a power of two, or 0 for any pointer), else `cache`'s buffer on `device`.
inline int bind_workspace(DeviceCache &cache, int device, size_t need, void *caller, size_t caller_bytes,
                          size_t align, void **out) {
    if (caller == nullptr) return cache.get(device, need, out);
    if (caller_bytes < need) return KMC_ERR_WORKSPACE;
    if (align && (reinterpret_cast<uintptr_t>(caller) & (align - 1))) return KMC_ERR_ALIGNMENT;
    *out = caller;
    return 0;
}

// f(std::integral_constant<int, k>{}) for LO <= k <= HI: the one runtime-to-template
// dispatch on k of a path; KMC_ERR_UNSUPPORTED_K outside.
template <int LO, int HI, class F>
inline int with_k(int k, F &&f) {
    if constexpr (LO > HI) return KMC_ERR_UNSUPPORTED_K;
    else return k == LO ? f(std::integral_constant<int, LO>{}) : with_k<LO + 1, HI>(k, f);
}

// Compute units of `device`, asked of the runtime once per device and process
// (one table for every translation unit: an inline function's statics are shared).
inline int device_cus(int device, int *cus) {
    static std::mutex mu;
    static std::vector<int> known;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)known.size() <= device) known.resize(device + 1, 0);
    if (known[device] == 0) {
        int v = 0;
        const hipError_t e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device);
        if (e != hipSuccess) return (int)e;
        known[device] = v;
    }
    *cus = known[device];
    return 0;
}

// The calling thread's current device and its compute units.
inline int current_device_cus(int *device, int *cus) {
    if (hipError_t he = hipGetDevice(device)) return (int)he;
    return device_cus(*device, cus);
}

// Sizes, binds and lays out the workspace of one call.  layout_of(base) is the one
// layout of the subsystem, a struct of pointers with the size in `bytes`: over null
// it gives the size to bind (bind_workspace), over the bound workspace *out.
template <class LayoutOf, class Layout>
inline int bind_layout(DeviceCache &cache, int device, void *caller, size_t caller_bytes, size_t align,
                       LayoutOf layout_of, Layout *out) {
    void *ws = nullptr;
    if (int e = bind_workspace(cache, device, layout_of(nullptr).bytes, caller, caller_bytes, align, &ws)) return e;
    *out = layout_of(ws);
    return 0;
}

}  // namespace kmc
