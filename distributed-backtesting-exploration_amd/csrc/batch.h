// batch.h — the host half of bt_run_batch (engine.cpp run_batch_impl holds the device half): parse
// the jobs, lay their rows out, decode into the caller's staging columns, format the
// CompleteRequest.data strings. No HIP: tests/asan/ingest_driver.cpp runs it under the sanitizers.
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "../../include/bt.h"
#include "csv.h"

namespace bt {

constexpr int64_t kStageAlign = 64;  // rows of a symbol start on this boundary (internal.h kRowAlign)
inline int64_t align_rows(int64_t bars) { return (bars + kStageAlign - 1) / kStageAlign * kStageAlign; }

// One CompleteRequest.data line per parameter (spec §6) into `out`, which holds P * kLineMax
// bytes; returns the bytes written (no terminator).
constexpr size_t kLineMax = 192;  // longest line: 10 + 11 + 20 x 3 + 24 + 16 + fixed text < 192
size_t fmt_job_into(const bt_summary* r, int32_t P, char* out);
void free_job_outs(bt_job_out* outs, size_t n);

struct StagedSym {
    int64_t row;   // first row in every staging column
    int32_t bars;
};

struct JobSlot {
    bool ok = false, binary = false;
    int32_t bars = 0;
    int64_t row = 0;
    size_t sym = 0;  // index into Batch::syms
    Bars parsed;     // CSV jobs only (binary payloads decode straight into the staging rows)
    std::string err;
};

// The JobsReply as one GPU batch (drop-in for process_incoming_job's loop,
// /root/reference/src/worker/process.rs:21-25), each step over the jobs on host threads:
//   parse():  1. binary payloads -> bar count from the header; CSV -> parsed;
//             2. rows of the good jobs laid out 64-aligned; returns the rows per column;
//   stage():  3. binary payloads validated and decoded straight into their rows in one pass
//                (decode_binary_into), CSV bars copied in; the jobs still good become `syms`;
//   (engine)  4. one async H2D per column, the strategy kernel, one D2H of every summary;
//   format(): 5. the CompleteRequest.data string of every job, from sum[sym * P + p].
struct Batch {
    Batch(size_t n, const bt_job_in* jobs, int32_t host_threads);
    int64_t parse();
    void stage(int32_t* c, int32_t* h, int32_t* l);  // h, l: nullptr for close alone
    void format(const bt_summary* sum, int32_t P, bt_job_out* outs);

    size_t n;
    const bt_job_in* jobs;
    int nt;
    std::vector<JobSlot> js;
    std::vector<StagedSym> syms;
    bt_batch_profile prof{};  // the host fields; the engine adds the three device timings
    std::chrono::steady_clock::time_point t_start;
};

}  // namespace bt
