// owned_driver.cpp — hip_owned.h without a HIP runtime (tests/test_hip_owned_cpu.py, under
// AddressSanitizer / UBSan / LeakSanitizer). The HIP entry points the header calls are counting
// fakes over malloc defined here: a live set per kind, the k-th creating call fails on request, a
// free of something not live aborts. A holder shaped like bt_engine runs a scripted sequence with
// every creating call failing in turn; whatever was made must be gone after the holder's scope.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "hip_owned.h"

namespace {

enum Kind { kDev, kPinned, kEvent, kStream, kKinds };
std::set<void*> g_live[kKinds];
int g_creates = 0, g_fail_at = 0, g_frees[kKinds] = {};

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::abort();                                                 \
        }                                                                 \
    } while (0)

hipError_t make(Kind k, void** out) {
    if (++g_creates == g_fail_at) return hipErrorOutOfMemory;
    *out = std::malloc(8);
    g_live[k].insert(*out);
    return hipSuccess;
}

hipError_t drop(Kind k, void* p) {
    REQUIRE(g_live[k].erase(p) == 1);  // live, and of this kind
    std::free(p);
    ++g_frees[k];
    return hipSuccess;
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t) { return make(kDev, p); }
hipError_t hipFree(void* p) { return drop(kDev, p); }
hipError_t hipHostMalloc(void** p, size_t, unsigned) { return make(kPinned, p); }
hipError_t hipHostFree(void* p) { return drop(kPinned, p); }
hipError_t hipEventCreate(hipEvent_t* e) { return make(kEvent, (void**)e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(kEvent, (void**)e); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(kEvent, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return make(kStream, (void**)s); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(kStream, s); }
const char* hipGetErrorString(hipError_t) { return "fake failure"; }
}

namespace {

using namespace bt;

char g_callers_stream;  // the borrowed stream's handle: in no live set, so destroying it aborts

struct Holder {
    Stream tstream, stream, borrowed;  // first, as in bt_engine: the last to go
    DevBuf<int32_t> d_axes[4];
    DevBuf<double> d_sum[2];
    PinnedBuf<int32_t> h_stage[3];
    PinnedBuf<char> h_top;
    Event ev[4];
    std::vector<std::pair<Event, Event>> pending, pool;
};

// One timed run as engine.cpp run_impl takes its pair: from the pool, else created.
void timed_run(Holder& h) {
    std::pair<Event, Event> ev;
    if (!h.pool.empty()) {
        ev = std::move(h.pool.back());
        h.pool.pop_back();
    }
    ev.first.ensure(0);
    ev.second.ensure(0);
    h.pending.push_back(std::move(ev));
}

void drain(Holder& h) {
    for (auto& ev : h.pending) h.pool.push_back(std::move(ev));
    h.pending.clear();
}

void script(Holder& h) {
    h.stream.create();
    h.borrowed.borrow((hipStream_t)&g_callers_stream);
    h.tstream.create();
    for (int i = 0; i < 4; ++i) h.ev[i].ensure(i & 1 ? hipEventDisableTiming : 0);
    for (int i = 0; i < 4; ++i) h.d_axes[i].ensure(3 + i);
    for (auto& b : h.d_sum) b.ensure(100);
    h.d_sum[0].ensure(200);  // growth
    for (auto& b : h.h_stage) b.ensure(64);
    h.h_stage[0].ensure(128);  // growth
    h.h_top.ensure(0);         // at least one element
    timed_run(h);
    timed_run(h);
    drain(h);
    timed_run(h);  // from the pool
    timed_run(h);
    timed_run(h);  // pool empty again: created
    drain(h);
}

bool all_gone() {
    for (const auto& s : g_live)
        if (!s.empty()) return false;
    return true;
}

// The script with the k-th creating call failing (k = 0: none); returns the creating calls made.
int run(int k) {
    g_creates = 0;
    g_fail_at = k;
    bool threw = false;
    {
        Holder h;
        try {
            script(h);
        } catch (const HipFail& f) {
            threw = true;
            REQUIRE(f.msg.find(": fake failure") != std::string::npos);
        }
        REQUIRE(!h.borrowed.owned && (k == 1 || h.borrowed.s == (hipStream_t)&g_callers_stream));
    }
    REQUIRE(all_gone());  // and no abort: the borrowed stream was never destroyed
    REQUIRE(threw == (k >= 1 && k <= g_creates));
    return g_creates;
}

void single_properties() {
    g_fail_at = 0;
    {
        DevBuf<int32_t> d;
        PinnedBuf<int32_t> p;
        d.ensure(0);
        REQUIRE(!d.p && g_live[kDev].empty());  // nothing asked for, nothing made
        d.ensure(10);
        p.ensure(10);
        const int calls = g_creates, dfree = g_frees[kDev], pfree = g_frees[kPinned];
        void *d0 = d.p, *p0 = p.p;
        d.ensure(10), d.ensure(1), p.ensure(10), p.ensure(0);
        REQUIRE(g_creates == calls && d.p == d0 && p.p == p0);  // want <= n: no call
        REQUIRE(g_frees[kDev] == dfree && g_frees[kPinned] == pfree);
        d.ensure(11), p.ensure(11);
        REQUIRE(g_creates == calls + 2 && d.n == 11 && p.n == 11);
        REQUIRE(g_frees[kDev] == dfree + 1 && g_frees[kPinned] == pfree + 1);  // the old block, once
        REQUIRE(g_live[kDev].size() == 1 && g_live[kPinned].size() == 1);
        d.release();
        REQUIRE(!d.p && d.n == 0 && g_live[kDev].empty());
        PinnedBuf<char> one;
        one.ensure(0);
        REQUIRE(one.p && one.n == 1);
    }
    {
        Event a;
        a.ensure(hipEventDisableTiming);
        const hipEvent_t raw = a;
        a.ensure(0);
        REQUIRE((hipEvent_t)a == raw);  // made once
        const int destroyed = g_frees[kEvent];
        {
            Event b(std::move(a));
            REQUIRE(!a.ev && (hipEvent_t)b == raw);
            Event c;
            c = std::move(b);
            REQUIRE(!b.ev && (hipEvent_t)c == raw);
            { Event gone(std::move(b)); }  // moved-from twice over: destroys nothing
            REQUIRE(g_frees[kEvent] == destroyed);
        }
        REQUIRE(g_frees[kEvent] == destroyed + 1);
    }
    REQUIRE(all_gone());
}

}  // namespace

int main() {
    single_properties();
    const int n = run(0);
    REQUIRE(n >= 20);
    for (int k = 1; k <= n + 1; ++k) run(k);  // k = n + 1: no call fails
    std::printf("ok %d creating calls\n", n);
    return 0;
}
