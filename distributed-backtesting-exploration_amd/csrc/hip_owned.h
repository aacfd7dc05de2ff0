// hip_owned.h — the host engine's HIP resources as types that free themselves, and the one error
// path of the C ABI (engine.cpp, comm.cpp). Runtime API only: a host compiler builds it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <exception>
#include <string>
#include <utility>

#include "host_common.h"

namespace bt {

struct HipFail { std::string msg; };

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess)                                                                  \
            throw bt::HipFail{std::string(#x) + ": " + hipGetErrorString(e_)};                 \
    } while (0)

// Body of a C ABI entry point: a failure becomes bt_last_error() and the return value `fail`.
#define ABI_GUARD(fail, ...)                                       \
    try {                                                          \
        __VA_ARGS__                                                \
    } catch (const bt::HipFail& f) {                               \
        bt::set_last_error(f.msg);                                 \
        return fail;                                               \
    } catch (const std::exception& x) {                            \
        bt::set_last_error(std::string("exception: ") + x.what()); \
        return fail;                                               \
    } catch (...) {                                                \
        bt::set_last_error("unknown exception");                   \
        return fail;                                               \
    }

// Device memory of at least n elements. Growth frees first: the old contents are gone.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void ensure(size_t want) {
        if (want <= n && p) return;
        release();
        if (want == 0) return;
        HIPCHK(hipMalloc((void**)&p, want * sizeof(T)));
        n = want;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, n = 0;
    }
};

// Pinned host memory of at least n elements, never fewer than one; growth as DevBuf.
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    void ensure(size_t want) {
        if (want <= n && p) return;
        T* old = p;
        p = nullptr, n = 0;
        if (old) HIPCHK(hipHostFree(old));
        want = std::max<size_t>(want, 1);
        HIPCHK(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
        n = want;
    }
};

// An event, created on first ensure(); flags 0 is a timing event.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { return std::swap(ev, o.ev), *this; }  // ours goes with `o`
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    void ensure(unsigned flags) {
        if (ev) return;
        if (flags)
            HIPCHK(hipEventCreateWithFlags(&ev, flags));
        else
            HIPCHK(hipEventCreate(&ev));
    }
    operator hipEvent_t() const { return ev; }
};

// A stream: the engine's own (non-blocking), or the caller's, which is never destroyed.
struct Stream {
    hipStream_t s = nullptr;
    bool owned = false;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (owned && s) (void)hipStreamDestroy(s); }
    void create() {
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        owned = true;
    }
    void borrow(hipStream_t caller) { s = caller; }
    operator hipStream_t() const { return s; }
};

}  // namespace bt
