// hip_owned.h -- host-only owners of HIP resources: device memory, pinned host memory, events, streams.  No kernels, no device code.
// Every owner is move-only and releases what it holds in its destructor; DeviceSpan is the one view type and releases nothing.
// Creation is explicit and returns hipError_t.  The owners count what is alive (live_resources): r3n_internal_live_resources
// exports the counters, tests/test_resources_gpu.py holds them to their baseline.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace hip_owned {

enum Ledger { kDevice = 0, kPinned = 1, kEvents = 2, kStreams = 3 };
inline std::atomic<uint64_t> live_resources[4];  // process-wide, indexed by Ledger

// A view into someone else's device block.
struct DeviceSpan {
    void *p = nullptr;
    size_t bytes = 0;
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// An owned block of device (kDevice: hipMalloc) or pinned host memory (kPinned: hipHostMalloc with `flags`).
template <Ledger L>
struct Block {
    void *p = nullptr;
    size_t bytes = 0;
    Block() = default;
    Block(Block &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Block &operator=(Block &&o) noexcept {
        if (this != &o) { (void)reset(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
        return *this;
    }
    ~Block() { (void)reset(); }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    // Replaces what is held by a new block of n bytes (contents undefined).
    hipError_t alloc(size_t n, unsigned flags = 0) {
        hipError_t e = reset();
        if (e == hipSuccess) e = L == kDevice ? hipMalloc(&p, n) : hipHostMalloc(&p, n, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = n;
        ++live_resources[L];
        return hipSuccess;
    }
    // Frees what is held (the free of a device block waits for the device) and reports.
    hipError_t reset() {
        if (!p) return hipSuccess;
        void *old = std::exchange(p, nullptr);
        bytes = 0;
        --live_resources[L];
        return L == kDevice ? hipFree(old) : hipHostFree(old);
    }
};
using DeviceBuffer = Block<kDevice>;
using PinnedHost = Block<kPinned>;

// An owned event or stream; converts to its raw handle.
template <class H, hipError_t (*Destroy)(H), Ledger L>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) { reset(); h = std::exchange(o.h, nullptr); }
        return *this;
    }
    ~Handle() { reset(); }
    operator H() const { return h; }
    void reset() {
        if (!h) return;
        --live_resources[L];
        (void)Destroy(std::exchange(h, nullptr));
    }

protected:
    hipError_t created(hipError_t e) {
        if (e == hipSuccess) ++live_resources[L];
        else h = nullptr;
        return e;
    }
};
struct Event : Handle<hipEvent_t, hipEventDestroy, kEvents> {
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return created(hipEventCreateWithFlags(&h, flags)); }
};
// The phase boundaries of one synchronous call: up to MAX events, all of them or none (arm(false): none), gone with the call.
// read() writes the time from event k to event k + 1 into ms[k]: 0 when unarmed, when the call failed (!ok) or where the query fails.
struct PhaseTaps {
    static constexpr int MAX = 5;
    Event ev[MAX];
    hipEvent_t handles[MAX] = {};  // the events as raw() hands them to a kernel unit that records them itself
    void arm(bool timing, int n = MAX) {
        for (int k = 0; k < n && timing; ++k) timing = ev[k].create() == hipSuccess;
        for (int k = 0; k < MAX; ++k) {
            if (!timing) ev[k].reset();
            handles[k] = ev[k];
        }
    }
    bool armed() const { return ev[0] != nullptr; }
    hipEvent_t *raw() { return armed() ? handles : nullptr; }
    hipError_t record(int k, hipStream_t stream) const { return armed() ? hipEventRecord(ev[k], stream) : hipSuccess; }
    void read(float *ms, int n_phases, bool ok) const {
        for (int k = 0; k < n_phases; ++k)
            if (!ok || !armed() || hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) ms[k] = 0.0f;
    }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy, kStreams> {
    hipError_t create(unsigned flags) { reset(); return created(hipStreamCreateWithFlags(&h, flags)); }
    hipError_t create(unsigned flags, int priority) { reset(); return created(hipStreamCreateWithPriority(&h, flags, priority)); }
};

}  // namespace hip_owned
