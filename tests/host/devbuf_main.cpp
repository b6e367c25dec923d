// Stand-alone host check of the buffer owners of csrc/wn_dev.h (DevBuf / PinBuf), built with -fsanitize=address,undefined and run as an ordinary
// program by tests/test_host_cpu.py.  It supplies the allocator seam itself: wn_dev_alloc / wn_dev_free on malloc / free with a live count and a
// "fail the k-th allocation" switch, so a double free, a leak or a use after free is the sanitizer's to report and the counts are exact.
// Streams, events and graph execs cannot be created without a device: this program covers buffers only.
#include "wn_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <set>

static int64_t g_live = 0, g_allocs = 0, g_fail_at = 0;      // g_fail_at = k > 0: the k-th allocation from now fails
static std::set<void*> g_dev, g_pin;                         // which flavour every live block came from
hipError_t wn_dev_alloc(void** p, size_t bytes, bool pinned) {
    if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    (pinned ? g_pin : g_dev).insert(*p);
    ++g_live; ++g_allocs;
    return hipSuccess;
}
void wn_dev_free(void* p, bool pinned) {
    if ((pinned ? g_pin : g_dev).erase(p) != 1) { fprintf(stderr, "free of a block of the other flavour, or twice\n"); abort(); }
    free(p); --g_live;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

template <class Buf> static void basics() {
    CHECK(g_live == 0);
    {
        Buf a;
        CHECK(!a.get() && a.cap() == 0 && a.bytes() == 0);
        CHECK(a.reserve(10) == hipSuccess && g_live == 1 && a.cap() == 10 && a.bytes() == 10 * sizeof(*a.get()));
        a.get()[9] = 1;                                             // (the block really has 10 elements: ASAN watches)
        auto* p0 = a.get();
        CHECK(a.reserve(7) == hipSuccess && a.reserve(10) == hipSuccess && a.get() == p0 && a.cap() == 10 && g_live == 1);      // reserve: no-op when n <= cap
        CHECK(a.reserve(20) == hipErrorInvalidValue && a.get() == p0 && a.cap() == 10 && g_live == 1);      // ... and never reallocates: too small is an error
        CHECK(a.grow(5) == hipSuccess && a.get() == p0 && a.cap() == 10 && g_live == 1);      // grow: no-op when large enough
        CHECK(a.grow(40) == hipSuccess && a.cap() == 40 && g_live == 1);             // the old block is gone, one is live
        a.get()[39] = 2;
        // a failed growth leaves pointer, capacity and live count as they were
        auto* p1 = a.get(); const int64_t n1 = g_allocs;
        g_fail_at = 1;
        CHECK(a.grow(80) == hipErrorOutOfMemory && a.get() == p1 && a.cap() == 40 && g_live == 1 && g_allocs == n1);
        a.get()[39] = 3;                                            // still ours
        // moves
        Buf b(std::move(a));
        CHECK(!a.get() && a.cap() == 0 && b.get() == p1 && b.cap() == 40 && g_live == 1);
        Buf c;
        CHECK(c.reserve(3) == hipSuccess && g_live == 2);
        c = std::move(b);                                           // frees c's block, takes b's
        CHECK(g_live == 1 && c.get() == p1 && !b.get() && b.cap() == 0);
        { Buf& same = c; c = std::move(same); }                     // self-assignment keeps it
        CHECK(g_live == 1 && c.get() == p1 && c.cap() == 40);
        decltype(c.get()) raw = c;                                  // implicit conversion
        CHECK(raw == p1);
        Buf d;
        g_fail_at = 1;
        CHECK(d.reserve(7) == hipErrorOutOfMemory && !d.get() && d.cap() == 0 && g_live == 1);
        CHECK(d.reserve(7) == hipSuccess && g_live == 2);
        d.reset();
        CHECK(!d.get() && d.cap() == 0 && g_live == 1);
        d.reset();                                                  // twice is harmless
    }                                                               // the destructors free exactly once (after the failed growth too)
    CHECK(g_live == 0);
}

// a small scripted life of four buffers; returns whether every step succeeded
template <class Buf> static bool script() {
    Buf a, b[2], c;
    bool ok = a.reserve(4) == hipSuccess;
    for (size_t n : {8, 2, 16, 64}) { ok = ok && a.grow(n) == hipSuccess; for (auto& q : b) ok = ok && q.grow(n / 2) == hipSuccess; }
    ok = ok && c.reserve(1) == hipSuccess;
    c = std::move(b[1]);
    ok = ok && b[1].grow(5) == hipSuccess && c.grow(100) == hipSuccess;
    return ok;
}
template <class Buf> static void fail_every_allocation() {
    const int64_t n0 = g_allocs;
    g_fail_at = 0;
    CHECK(script<Buf>() && g_live == 0);
    const int64_t total = g_allocs - n0;
    CHECK(total >= 10);
    for (int64_t k = 1; k <= total; ++k) {                          // fail the k-th allocation of the same script
        g_fail_at = k;
        CHECK(!script<Buf>());
        CHECK(g_live == 0 && g_dev.empty() && g_pin.empty());
        g_fail_at = 0;
    }
}

int main() {
    basics<DevBuf<float>>();
    basics<PinBuf<int32_t>>();
    fail_every_allocation<DevBuf<double>>();
    fail_every_allocation<PinBuf<char>>();
    printf("devbuf ok: %lld allocations\n", (long long)g_allocs);
    return 0;
}
