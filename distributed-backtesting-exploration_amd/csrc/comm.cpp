// comm.cpp — the multi-GPU exchange step behind the C ABI: one RCCL
// all-gather over xGMI of every rank's top-k records and run counters, straight from the
// engine's device buffers, then the host merge with the engine's order.
//
// The reference's only parallelism is file-level job farming over gRPC
// (/root/reference/src/server/main.rs:131-143) with no collective at all. Here each GPU runs a
// contiguous block of symbols with no data-path collective; once per run the ranks exchange
// [header record | k records | bar-evals | trades] (k = 100: 2.4 KB per rank). That message is
// latency-bound, so it is a single ncclAllGather on the engine's top-k stream, enqueued behind
// the run's top-k chain without a host wait, and read back into one of BT_PIPE_SLOTS pinned slots so the
// next run overlaps it (the same pipelining as bt_topk_fetch_async / bt_topk_fetch_wait).
//
// RCCL is resolved with dlopen on the first communicator call, not linked: a single-GPU worker
// (configs 1-2) loads libbt.so on a box without librccl (the reference's worker build hook,
// /root/reference/build.rs:1-4, links nothing either). rccl.h is used for its types only. In a
// process that already holds an RCCL (PyTorch-ROCm's bundled librccl.so, SONAME librccl.so.1),
// dlopen by SONAME returns that copy, as the dynamic linker did when libbt.so linked it.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "hip_owned.h"
#include "internal.h"

using namespace bt;

struct bt_comm {
    ncclComm_t comm = nullptr;
    int32_t rank = 0, world = 1, device = 0, k = 0;
    size_t rec_bytes = 0;              // bytes one rank contributes
    DevBuf<unsigned char> d_send;                   // [rec_bytes]
    DevBuf<unsigned char> d_recv[BT_PIPE_SLOTS];    // [world * rec_bytes] per slot
    PinnedBuf<unsigned char> h_recv[BT_PIPE_SLOTS];
    PinnedBuf<int64_t> h_evals[BT_PIPE_SLOTS];      // this rank's bar-evals per slot
    Event done[BT_PIPE_SLOTS];
    bool armed[BT_PIPE_SLOTS] = {};
    ~bt_comm();
};

namespace {

// the RCCL entry points this file calls
struct Rccl {
    void* so = nullptr;
    std::string why;  // dlopen / dlsym failure
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t,
                              hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

const Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
            r.so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.so) break;
        }
        if (!r.so) {
            const char* e = dlerror();
            r.why = std::string("RCCL is not loadable (librccl.so.1): ") + (e ? e : "dlopen failed");
            return;
        }
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(r.so, name));
            if (!fn && r.why.empty()) r.why = std::string("RCCL lacks ") + name;
        };
        sym(r.GetUniqueId, "ncclGetUniqueId");
        sym(r.CommInitRank, "ncclCommInitRank");
        sym(r.CommDestroy, "ncclCommDestroy");
        sym(r.AllGather, "ncclAllGather");
        sym(r.GetErrorString, "ncclGetErrorString");
    });
    if (!r.why.empty()) throw HipFail{r.why};
    return r;
}

#define NCCLCHK(x)                                                                             \
    do {                                                                                       \
        ncclResult_t r_ = (x);                                                                 \
        if (r_ != ncclSuccess)                                                                 \
            throw HipFail{std::string(#x) + ": " + rccl().GetErrorString(r_)};                \
    } while (0)

// Per-rank message: header record (record count in its first int32), k records, then the two
// int64 counters (bar-evals, trades).
size_t message_bytes(int32_t k) { return ((size_t)k + 1) * sizeof(bt_topk_rec) + 2 * sizeof(int64_t); }

// The host half of bt_exchange_wait: merge `world` gathered messages of k_msg records each.
int32_t merge_block(const unsigned char* block, int32_t world, int32_t k_msg, bt_topk_rec* out,
                    int32_t k, int64_t* counters) {
    const size_t mb = message_bytes(k_msg);
    std::vector<bt_topk_rec> all;
    all.reserve((size_t)k_msg * world);
    int64_t evals = 0, trades = 0;
    for (int32_t r = 0; r < world; ++r) {
        const unsigned char* m = block + (size_t)r * mb;
        int32_t n = 0;
        memcpy(&n, m, sizeof n);
        // every rank's device selection is exact whatever the ties (k_topk.hip
        // topk_finish_ties), so a tie-heavy grid exchanges like any other
        if (n < 0) throw HipFail{"rank " + std::to_string(r) + ": bad top-k record count"};
        n = std::min(n, k_msg);
        const unsigned char* recs = m + sizeof(bt_topk_rec);
        for (int32_t i = 0; i < n; ++i) {  // memcpy: the block carries no alignment promise
            bt_topk_rec x;
            memcpy(&x, recs + (size_t)i * sizeof x, sizeof x);
            all.push_back(x);
        }
        int64_t x[2];
        memcpy(x, m + ((size_t)k_msg + 1) * sizeof(bt_topk_rec), sizeof x);
        evals += x[0];
        trades += x[1];
    }
    const size_t mm = std::min<size_t>(all.size(), (size_t)std::min(k, k_msg));
    std::partial_sort(all.begin(), all.begin() + mm, all.end(), topk_less);
    std::copy(all.begin(), all.begin() + mm, out);
    if (counters) {
        counters[0] = evals;
        counters[1] = trades;
    }
    return (int32_t)mm;
}

}  // namespace

// The read-backs still in flight finish, the communicator goes, then the members.
bt_comm::~bt_comm() {
    (void)hipSetDevice(device);
    for (Event& ev : done)
        if (ev) (void)hipEventSynchronize(ev);
    if (comm) (void)rccl().CommDestroy(comm);  // comm set: rccl() resolved
}

extern "C" {

int32_t bt_comm_unique_id(uint8_t* out) {
    ABI_GUARD(-1, {
        if (!out) throw HipFail{"null output"};
        ncclUniqueId id;
        NCCLCHK(rccl().GetUniqueId(&id));
        static_assert(sizeof(id) == BT_COMM_ID_BYTES, "RCCL unique id size");
        memcpy(out, &id, sizeof id);
        return 0;
    })
}

bt_comm* bt_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device,
                        int32_t k, char* err, size_t errlen) {
    auto failed = [&]() -> bt_comm* {  // bt_last_error() into the caller's buffer too
        if (err && errlen) snprintf(err, errlen, "%s", bt_last_error());
        return nullptr;
    };
    ABI_GUARD(failed(), {
        if (!id || world < 1 || rank < 0 || rank >= world || k < 1 || k > 1024)
            throw HipFail{"bad arguments"};
        auto c = std::make_unique<bt_comm>();  // a failure below frees what was made so far
        c->rank = rank;
        c->world = world;
        c->device = device;
        c->k = k;
        c->rec_bytes = message_bytes(k);
        const Rccl& nc = rccl();
        HIPCHK(hipSetDevice(device));
        ncclUniqueId uid;
        memcpy(&uid, id, sizeof uid);
        NCCLCHK(nc.CommInitRank(&c->comm, world, uid, rank));
        c->d_send.ensure(c->rec_bytes);
        for (int s = 0; s < BT_PIPE_SLOTS; ++s) {
            c->d_recv[s].ensure(c->rec_bytes * world);
            c->h_recv[s].ensure(c->rec_bytes * world);
            c->h_evals[s].ensure(1);
            c->done[s].ensure(hipEventDisableTiming);
        }
        return c.release();
    })
}

void bt_comm_destroy(bt_comm* c) { delete c; }

int32_t bt_exchange_async(bt_comm* c, bt_engine* e, int32_t slot) {
    ABI_GUARD(-1, {
        if (!c || !e || slot < 0 || slot >= BT_PIPE_SLOTS) throw HipFail{"bad arguments"};
        ExchangeView v{};
        std::string why;
        if (!engine_exchange_view(e, v, why)) throw HipFail{why};
        if (v.device != c->device) throw HipFail{"engine and communicator are on different devices"};
        if (v.topk < c->k) throw HipFail{"engine topk is smaller than the communicator's k"};
        HIPCHK(hipSetDevice(c->device));
        // the slot's previous read-back must be consumed before its pinned buffers are reused
        if (c->armed[slot]) HIPCHK(hipEventSynchronize(c->done[slot]));
        const size_t recs = ((size_t)c->k + 1) * sizeof(bt_topk_rec);
        unsigned char* cnt = c->d_send.p + recs;
        *c->h_evals[slot].p = v.bar_evals;
        // header + the first k records of the run's top-k, its trade counter, its bar-evals
        HIPCHK(hipMemcpyAsync(c->d_send.p, v.d_top, recs, hipMemcpyDeviceToDevice, v.tstream));
        HIPCHK(hipMemcpyAsync(cnt, c->h_evals[slot].p, sizeof(int64_t), hipMemcpyHostToDevice, v.tstream));
        HIPCHK(hipMemcpyAsync(cnt + sizeof(int64_t), v.d_ntr, sizeof(int64_t), hipMemcpyDeviceToDevice,
                              v.tstream));
        engine_exchange_enqueued(e);
        NCCLCHK(rccl().AllGather(c->d_send.p, c->d_recv[slot].p, c->rec_bytes, ncclChar, c->comm,
                                 v.tstream));
        HIPCHK(hipMemcpyAsync(c->h_recv[slot].p, c->d_recv[slot].p, c->rec_bytes * c->world,
                              hipMemcpyDeviceToHost, v.tstream));
        HIPCHK(hipEventRecord(c->done[slot], v.tstream));
        c->armed[slot] = true;
        return 0;
    })
}

int32_t bt_exchange_wait(bt_comm* c, int32_t slot, bt_topk_rec* out, int32_t k,
                         int64_t* counters) {
    ABI_GUARD(-1, {
        if (!c || slot < 0 || slot >= BT_PIPE_SLOTS || !out || k < 1) throw HipFail{"bad arguments"};
        if (!c->armed[slot]) throw HipFail{"no exchange pending on this slot"};
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipEventSynchronize(c->done[slot]));
        c->armed[slot] = false;
        return merge_block(c->h_recv[slot].p, c->world, c->k, out, k, counters);
    })
}

int64_t bt_exchange_message_bytes(int32_t k) { return k < 1 ? -1 : (int64_t)message_bytes(k); }

int32_t bt_exchange_merge(const uint8_t* block, size_t block_bytes, int32_t world, int32_t k_msg,
                          bt_topk_rec* out, int32_t k, int64_t* counters) {
    ABI_GUARD(-1, {
        if (!block || world < 1 || k_msg < 1 || !out || k < 1) throw HipFail{"bad arguments"};
        // a short or mismatched block (a truncated gather, a rank that sent another k) is
        // rejected, never read past its end
        if (block_bytes != (size_t)world * message_bytes(k_msg))
            throw HipFail{"block holds " + std::to_string(block_bytes) + " bytes, not world x " +
                           std::to_string(message_bytes(k_msg))};
        return merge_block(block, world, k_msg, out, k, counters);
    })
}

}  // extern "C"
