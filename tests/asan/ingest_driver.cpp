// ingest_driver.cpp — host-only harness of the Job.File ingest (csv.cpp, payload.cpp) and of the
// host half of bt_run_batch (batch.cpp) for the AddressSanitizer / UBSan CPU test
// (tests/test_ingest_asan_cpu.py). For every input file: the standalone parser, and the batch
// path's header + in-place decode for binary payloads. Then all the files as one batch on 4
// threads, into exact-size staging columns, checked against the standalone parser, and formatted
// from summaries whose fields sit at their widest.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "batch.h"
#include "csv.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::abort();                                                 \
        }                                                                 \
    } while (0)

namespace {

struct File {
    uint8_t* data = nullptr;  // an exact-size heap copy, so any read past the end is an ASan error
    size_t len = 0;
    bool ok = false;          // what the standalone parser says
    bt::Bars bars;
};

// All files as one batch: staged rows against parse_job's, then the strings.
void run_batch(const std::vector<File>& files, bool hl) {
    std::vector<bt_job_in> jobs;
    for (const File& f : files) jobs.push_back(bt_job_in{"job", f.data, f.len});
    bt::Batch bat(jobs.size(), jobs.data(), 4);
    REQUIRE(bat.nt == 4);
    const int64_t rows = bat.parse();
    int32_t* col[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < (hl ? 3 : 1); ++k) col[k] = new int32_t[(size_t)rows];
    bat.stage(col[0], col[1], col[2]);
    int64_t failed = 0, bars = 0, next_row = 0;
    for (size_t i = 0; i < files.size(); ++i) {
        const bt::JobSlot& j = bat.js[i];
        const File& f = files[i];
        REQUIRE(j.ok == f.ok);
        if (!j.ok) {
            REQUIRE(!j.err.empty());
            ++failed;
            continue;
        }
        const size_t n = f.bars.c.size();
        REQUIRE((size_t)j.bars == n && bat.syms[j.sym].row == j.row && bat.syms[j.sym].bars == j.bars);
        // rows in job order, each past the end of the one before, whole inside the columns
        REQUIRE(j.row >= next_row && j.row % bt::kStageAlign == 0 && j.row + (int64_t)n <= rows);
        next_row = j.row + (int64_t)n;
        REQUIRE(std::equal(f.bars.c.begin(), f.bars.c.end(), col[0] + j.row));
        if (hl) {
            REQUIRE(std::equal(f.bars.h.begin(), f.bars.h.end(), col[1] + j.row));
            REQUIRE(std::equal(f.bars.l.begin(), f.bars.l.end(), col[2] + j.row));
        }
        bars += (int64_t)n;
    }
    REQUIRE(bat.prof.n_failed == failed && bat.prof.n_jobs == (int64_t)files.size() && bat.prof.bars == bars);
    REQUIRE(bat.syms.size() == files.size() - (size_t)failed);
    for (int k = 0; k < 3; ++k) delete[] col[k];

    // an error message that needs every escape
    for (bt::JobSlot& j : bat.js)
        if (!j.ok) j.err = std::string("a\"b\\c\x01" "d\ne", 9);
    const double sharpes[3] = {-1.7976931348623157e308, 5e-324, -0.0};
    for (int32_t P : {1, 3}) {
        std::vector<bt_summary> sum(bat.syms.size() * (size_t)P);
        for (size_t i = 0; i < sum.size(); ++i) {
            sum[i].n_trades = std::numeric_limits<int32_t>::min();
            sum[i].status = 0;
            sum[i].pnl = sum[i].mdd = std::numeric_limits<int64_t>::min();
            sum[i].exposure = std::numeric_limits<int32_t>::min();
            sum[i].sharpe = sharpes[(i + (size_t)P) % 3];
            sum[i].hash = ~0ULL;
        }
        std::vector<bt_job_out> outs(files.size(), bt_job_out{nullptr, 0, 0, 0});
        bat.format(sum.data(), P, outs.data());
        size_t longest = 0;
        for (size_t i = 0; i < files.size(); ++i) {
            const bt_job_out& o = outs[i];
            REQUIRE(o.data && std::strlen(o.data) == o.len);
            const std::string s(o.data, o.len);
            if (!files[i].ok) {
                REQUIRE(o.status == -1 && o.n_bars == 0);
                REQUIRE(s == "{\"error\":\"a\\\"b\\\\c d e\"}\n");
                continue;
            }
            REQUIRE(o.status == 0 && o.n_bars == bat.js[i].bars);
            REQUIRE(o.len <= (size_t)P * bt::kLineMax);
            REQUIRE((int32_t)std::count(s.begin(), s.end(), '\n') == P && s.back() == '\n');
            size_t at = 0;
            for (int32_t p = 0; p < P; ++p) {
                const size_t end = s.find('\n', at);
                const std::string line = s.substr(at, end - at);
                longest = std::max(longest, line.size() + 1);
                const std::string head = "{\"param\":" + std::to_string(p) +
                                         ",\"n\":-2147483648,\"pnl\":-9223372036854775808,\"mdd\":-9223372036854775808"
                                         ",\"exp\":-2147483648,\"sharpe\":\"";
                REQUIRE(line.compare(0, head.size(), head) == 0);
                const std::string tail = "\",\"h\":\"ffffffffffffffff\"}";
                REQUIRE(line.size() > tail.size() && line.compare(line.size() - tail.size(), tail.size(), tail) == 0);
                at = end + 1;
            }
        }
        REQUIRE(longest <= bt::kLineMax);
        std::printf("P %d longest line %zu\n", P, longest);
        bt::free_job_outs(outs.data(), outs.size());
        for (const bt_job_out& o : outs) REQUIRE(!o.data && o.len == 0);
    }
}

}  // namespace

int main(int argc, char** argv) {
    int accepted = 0;
    std::vector<File> files((size_t)(argc - 1));
    for (int i = 1; i < argc; ++i) {
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<uint8_t> buf;
        uint8_t chunk[65536];
        size_t n;
        while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
        std::fclose(f);
        File& file = files[(size_t)i - 1];
        uint8_t* data = buf.empty() ? nullptr : new uint8_t[buf.size()];
        if (data) std::copy(buf.begin(), buf.end(), data);
        file.data = data;
        file.len = buf.size();
        std::string err;
        const bool ok = file.ok = bt::parse_job(data, buf.size(), file.bars, err);
        accepted += ok ? 1 : 0;
        int32_t bars = 0;
        if (data && bt::is_binary_payload(data, buf.size()) && bt::binary_header(data, buf.size(), bars, err)) {
            std::vector<int32_t> h(bars), l(bars), c(bars);
            bt::decode_binary_into(data, buf.size(), h.data(), l.data(), c.data(), err);
        }
    }
    std::printf("accepted %d of %d\n", accepted, argc - 1);
    run_batch(files, false);
    run_batch(files, true);
    for (File& f : files) delete[] f.data;
    return 0;
}
