// batch.cpp — the host half of bt_run_batch (batch.h): ingest of the jobs into staging rows and
// the CompleteRequest.data strings (/root/reference/proto/backtesting.proto:29-32).
#include "batch.h"

#include <algorithm>
#include <atomic>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

namespace bt {
namespace {

using clk = std::chrono::steady_clock;

double ms_between(clk::time_point a, clk::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// One CompleteRequest.data line (spec §6). std::to_chars gives printf's "%.17g" (general
// format, precision 17) and plain decimal integers without the locale and format-string work of
// snprintf; tests/test_abi_cpu.py checks the bytes against Python's "%.17g" / "%016x".
char* put_lit(char* q, const char* s) {
    while (*s) *q++ = *s++;
    return q;
}

char* fmt_line(char* q, int32_t p, const bt_summary& x) {
    static const char kHex[] = "0123456789abcdef";
    q = put_lit(q, "{\"param\":");
    q = std::to_chars(q, q + 16, p).ptr;
    q = put_lit(q, ",\"n\":");
    q = std::to_chars(q, q + 16, x.n_trades).ptr;
    q = put_lit(q, ",\"pnl\":");
    q = std::to_chars(q, q + 24, (long long)x.pnl).ptr;
    q = put_lit(q, ",\"mdd\":");
    q = std::to_chars(q, q + 24, (long long)x.mdd).ptr;
    q = put_lit(q, ",\"exp\":");
    q = std::to_chars(q, q + 24, (long long)x.exposure).ptr;
    q = put_lit(q, ",\"sharpe\":\"");
    q = std::to_chars(q, q + 32, x.sharpe, std::chars_format::general, 17).ptr;
    q = put_lit(q, "\",\"h\":\"");
    for (int i = 15; i >= 0; --i) *q++ = kHex[(x.hash >> (4 * i)) & 15];
    return put_lit(q, "\"}\n");
}

std::string json_escape(const std::string& in) {
    std::string o;
    for (char ch : in) {
        if (ch == '"' || ch == '\\') {
            o.push_back('\\');
            o.push_back(ch);
        } else if ((unsigned char)ch < 0x20) {
            o.push_back(' ');
        } else {
            o.push_back(ch);
        }
    }
    return o;
}

char* dup_string(const std::string& s) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) throw std::bad_alloc();
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    return p;
}

// f(i) for i in [0, n) on nt threads (f must not throw).
template <class F>
void parallel_for(int nt, size_t n, const F& f) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    if (nt <= 1 || n <= 1) {
        work();
        return;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)nt);
    for (int i = 0; i < nt; ++i) th.emplace_back(work);
    for (auto& t : th) t.join();
}

}  // namespace

size_t fmt_job_into(const bt_summary* r, int32_t P, char* out) {
    char* q = out;
    for (int32_t p = 0; p < P; ++p) q = fmt_line(q, p, r[p]);
    return (size_t)(q - out);
}

void free_job_outs(bt_job_out* outs, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        free(outs[i].data);
        outs[i].data = nullptr;
        outs[i].len = 0;
    }
}

// Host threads of the ingest: host_threads, else the machine's, at most 16 (the worker's share
// of a GPU box; /root/reference/src/worker/handlers.rs:35 reports num_cpus/2 as cores).
Batch::Batch(size_t n_, const bt_job_in* jobs_, int32_t host_threads)
    : n(n_), jobs(jobs_), js(n_), t_start(clk::now()) {
    const int want = host_threads > 0
                         ? host_threads
                         : (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
    nt = (int)std::min<size_t>((size_t)want, std::max<size_t>(1, n));
    prof.n_jobs = (int64_t)n;
}

int64_t Batch::parse() {
    for (size_t i = 0; i < n; ++i) prof.payload_bytes += (int64_t)jobs[i].len;
    parallel_for(nt, n, [&](size_t i) {
        JobSlot& j = js[i];
        try {
            const uint8_t* buf = jobs[i].file;
            const size_t len = jobs[i].len;
            if (!buf && len) {
                j.err = "null Job.File";
            } else if (buf && is_binary_payload(buf, len)) {
                j.binary = true;
                j.ok = binary_header(buf, len, j.bars, j.err);
            } else {
                j.ok = parse_csv(buf, len, j.parsed, j.err);
                j.bars = (int32_t)j.parsed.c.size();
            }
        } catch (...) {
            j.ok = false;
            j.err = "parse failure";
        }
    });
    int64_t rows = 0;
    for (size_t i = 0; i < n; ++i) {
        JobSlot& j = js[i];
        if (!j.ok) continue;
        // what ingest touches: a CSV is parsed whole; a binary payload's header and its four price
        // columns are validated, its volume column is never read
        prof.payload_bytes_read += j.binary ? (int64_t)binary_payload_size(j.bars, false) : (int64_t)jobs[i].len;
        j.row = rows;
        rows += align_rows(j.bars);
    }
    return rows;
}

void Batch::stage(int32_t* c0, int32_t* h0, int32_t* l0) {
    parallel_for(nt, n, [&](size_t i) {
        JobSlot& j = js[i];
        if (!j.ok) return;
        try {
            int32_t* c = c0 + j.row;
            int32_t* h = h0 ? h0 + j.row : nullptr;
            int32_t* l = l0 ? l0 + j.row : nullptr;
            if (j.binary) {
                j.ok = decode_binary_into(jobs[i].file, jobs[i].len, h, l, c, j.err);
            } else {
                memcpy(c, j.parsed.c.data(), (size_t)j.bars * 4);
                if (h) memcpy(h, j.parsed.h.data(), (size_t)j.bars * 4);
                if (l) memcpy(l, j.parsed.l.data(), (size_t)j.bars * 4);
                j.parsed = Bars();  // release early
            }
        } catch (...) {
            j.ok = false;
            j.err = "ingest failure";
        }
    });
    // a job that failed in step 3 leaves its rows unreferenced
    for (JobSlot& j : js) {
        if (!j.ok) {
            ++prof.n_failed;
            continue;
        }
        j.sym = syms.size();
        syms.push_back(StagedSym{j.row, j.bars});
        prof.bars += j.bars;
    }
    prof.host_ingest_ms = ms_between(t_start, clk::now());
}

void Batch::format(const bt_summary* sum, int32_t P, bt_job_out* outs) {
    const auto t_dev = clk::now();
    std::atomic<bool> alloc_fail{false};
    parallel_for(nt, n, [&](size_t i) {
        try {
            const JobSlot& j = js[i];
            if (j.ok) {
                char* buf = (char*)malloc((size_t)P * kLineMax + 1);
                if (!buf) throw std::bad_alloc();
                const size_t len = fmt_job_into(sum + j.sym * (size_t)P, P, buf);
                buf[len] = 0;
                char* fit = (char*)realloc(buf, len + 1);
                outs[i] = bt_job_out{fit ? fit : buf, len, 0, j.bars};
            } else {
                const std::string m = "{\"error\":\"" + json_escape(j.err) + "\"}\n";
                outs[i] = bt_job_out{dup_string(m), m.size(), -1, 0};
            }
        } catch (...) {
            alloc_fail = true;
        }
    });
    if (alloc_fail) throw std::bad_alloc();
    const auto t_end = clk::now();
    prof.format_ms = ms_between(t_dev, t_end);
    prof.total_ms = ms_between(t_start, t_end);
}

}  // namespace bt
