// Owners of device resources: every buffer, stream, event and graph exec of the library belongs to exactly one of these move-only types, whose
// destructor releases it.  Memory reaches the runtime only through wn_dev_alloc / wn_dev_free (defined once, in wn_api.hip; a stand-alone host
// program -- tests/host/devbuf_main.cpp -- defines a counting, failing pair instead).  Every error comes back as a hipError_t that the call site wraps
// in WN_HIP, so messages name the call site; nothing here knows wn_ctx.  Process-wide counters of live handles: wn_test_device_resources.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include <utility>

hipError_t wn_dev_alloc(void** p, size_t bytes, bool pinned);      // hipMalloc / hipHostMalloc; counts live buffers and allocations ever
void wn_dev_free(void* p, bool pinned);
struct WnDevCounts { std::atomic<int64_t> bufs{0}, streams{0}, events{0}, gexecs{0}, allocs{0}; };
inline WnDevCounts& wn_dev_counts() { static WnDevCounts c; return c; }

// A device (PINNED: pinned host) allocation and its capacity in elements.
template <class T, bool PINNED = false> class DevBuf {
    T* p_ = nullptr; size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p_) wn_dev_free(p_, PINNED); p_ = nullptr; cap_ = 0; }
    // at least n elements, contents NOT kept: the new block is allocated first and the old one freed only once that succeeded (a failed grow leaves
    // pointer and capacity as they were).  The caller synchronises whatever may still read the old block BEFORE it calls grow.
    hipError_t grow(size_t n) {
        if (n <= cap_) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = wn_dev_alloc(&q, n * sizeof(T), PINNED);
        if (e != hipSuccess) return e;
        reset(); p_ = (T*)q; cap_ = n;
        return hipSuccess;
    }
    // allocate if empty, no-op if n <= cap; never reallocates: a live buffer that is too small is the caller's mistake (a buffer that may grow takes grow)
    hipError_t reserve(size_t n) { return !p_ ? grow(n) : n <= cap_ ? hipSuccess : hipErrorInvalidValue; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
};
template <class T> using PinBuf = DevBuf<T, true>;

// Handle owners: created lazily by create*(), a no-op on a live handle.  H: the handle type, DESTROY: its release, COUNT: its live counter.
template <class H, hipError_t (*DESTROY)(H), std::atomic<int64_t> WnDevCounts::*COUNT> class DevHandle {
protected:
    H h_ = nullptr;
    template <class F> hipError_t make(F f) { if (h_) return hipSuccess; const hipError_t e = f(&h_); if (e == hipSuccess) ++(wn_dev_counts().*COUNT); else h_ = nullptr; return e; }
public:
    DevHandle() = default;
    DevHandle(const DevHandle&) = delete; DevHandle& operator=(const DevHandle&) = delete;
    DevHandle(DevHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    DevHandle& operator=(DevHandle&& o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); } return *this; }
    ~DevHandle() { reset(); }
    void reset() { if (h_) { (void)DESTROY(h_); --(wn_dev_counts().*COUNT); h_ = nullptr; } }
    H get() const { return h_; }
    operator H() const { return h_; }
};
inline hipError_t wn_stream_sync_destroy(hipStream_t s) { (void)hipStreamSynchronize(s); return hipStreamDestroy(s); }      // nothing of ours may still run on it
struct DevStream : DevHandle<hipStream_t, wn_stream_sync_destroy, &WnDevCounts::streams> {
    hipError_t create(unsigned flags) { return make([&](hipStream_t* s) { return hipStreamCreateWithFlags(s, flags); }); }
    hipError_t create_with_priority(unsigned flags, int prio) { return make([&](hipStream_t* s) { return hipStreamCreateWithPriority(s, flags, prio); }); }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy, &WnDevCounts::events> {
    hipError_t create(unsigned flags = hipEventDefault) { return make([&](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); }); }
};
struct DevGraphExec : DevHandle<hipGraphExec_t, hipGraphExecDestroy, &WnDevCounts::gexecs> {
    hipError_t instantiate(hipGraph_t g) { reset(); return make([&](hipGraphExec_t* x) { return hipGraphInstantiate(x, g, nullptr, nullptr, 0); }); }
};
struct DevGraphGuard {      // a captured hipGraph_t lives until the end of the scope that instantiates it
    hipGraph_t g = nullptr;
    DevGraphGuard() = default; DevGraphGuard(const DevGraphGuard&) = delete; DevGraphGuard& operator=(const DevGraphGuard&) = delete;
    ~DevGraphGuard() { if (g) (void)hipGraphDestroy(g); }
};
