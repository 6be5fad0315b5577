// hm_host.h -- host-side HIP plumbing shared by the CNN engine (hm_engine.cpp) and the pileup engine (hm_pileup.hip):
// the error type behind HIP_TRY, the guard every C ABI entry point runs under, and move-only owners of device memory,
// pinned memory, streams and events.  Every hipFree / hipHostFree / hipStreamDestroy / hipEventDestroy of the library
// is in this file: a buffer, stream or event is released by the destructor of the member that holds it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>

namespace hm {

struct HipErr {
    hipError_t code;
    const char* what;
};

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) throw ::hm::HipErr{_e, #expr}; \
    } while (0)

inline std::string hip_error_text(const HipErr& h) { return std::string("HIP error: ") + hipGetErrorString(h.code) + " at " + h.what; }

// What an ABI entry point does around its device work: make `device` current, run `body`, and hand a HipErr thrown on
// the way to `fail` (which records hip_error_text for the engine and returns its error value).  Returns what body returns.
template <class Fail, class Body>
auto hip_guard(int device, Fail&& fail, Body&& body) -> decltype(body()) {
    try {
        HIP_TRY(hipSetDevice(device));
        return body();
    } catch (const HipErr& h) {
        return fail(h);
    }
}

// move-only owner of one HIP handle or pinned pointer (h == null: nothing held)
template <class T, auto Free>
struct Owned {
    T h{};
    Owned() = default;
    Owned(Owned&& o) noexcept : h(std::exchange(o.h, T{})) {}
    Owned& operator=(Owned&& o) noexcept {
        std::swap(h, o.h);
        return *this;
    }
    ~Owned() {
        if (h) (void)Free(h);
    }
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// N zeroed pinned elements: where an asynchronous D2H of a few counters lands
template <class T>
struct Pinned : Owned<T*, hipHostFree> {
    void alloc(size_t n = 1) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&this->h), n * sizeof(T), hipHostMallocDefault));
        memset(this->h, 0, n * sizeof(T));
    }
};

// grow-only device buffer.  How much head-room a growing reserve() adds is a property of the buffer, because memory
// footprints are behaviour: the CNN engine's group size (GROUP_BYTES_PER_BASE, "a quarter of free memory") counts on
// QUARTER, the pileup's per-batch buffers grow by HALF, its genome-sized planes are allocated once and EXACT.
struct DevBuf {
    enum Room { QUARTER, HALF, EXACT };
    void* p = nullptr;
    size_t cap = 0;
    Room room;
    explicit DevBuf(Room r = QUARTER) : room(r) {}
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), room(o.room) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        std::swap(room, o.room);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    // grow to at least `bytes`.  keep == 0: the old contents are discarded and the old allocation is freed BEFORE the new
    // one is made (a group's maps never exist twice); otherwise the first `keep` bytes are carried over on `st`
    void reserve(size_t bytes, size_t keep = 0, hipStream_t st = nullptr) {
        if (bytes <= cap) return;
        const size_t want = room == EXACT ? bytes : bytes + bytes / (room == HALF ? 2 : 4) + 256;
        if (!keep) *this = DevBuf(room);
        DevBuf grown(room);
        HIP_TRY(hipMalloc(&grown.p, want));
        grown.cap = want;
        if (keep) {
            HIP_TRY(hipMemcpyAsync(grown.p, p, keep, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        *this = std::move(grown);  // a swap: what was held until now goes with `grown`
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// grow-only pinned host array: what an asynchronous copy may read from / write to
template <class T>
struct PinnedArr {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    PinnedArr() = default;
    PinnedArr(PinnedArr&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)), cap(std::exchange(o.cap, 0)) {}
    PinnedArr& operator=(PinnedArr&& o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
        return *this;
    }
    ~PinnedArr() {
        if (p) (void)hipHostFree(p);
    }
    void reserve(size_t want) {
        if (want <= cap) return;
        want = std::max(want + want / 2, size_t(4096) / sizeof(T) + 1);
        T* q = nullptr;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&q), want * sizeof(T), hipHostMallocDefault));
        if (n) memcpy(q, p, n * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q;
        cap = want;
    }
    void push_back(const T& v) {
        if (n == cap) reserve(n + 1);
        p[n++] = v;
    }
};

}  // namespace hm
