// portfolio_driver — csrc/portfolio.cpp (bt_portfolio_host, bt_portfolio_merge, the argument rules
// and the resolution against a dataset) as a stand-alone host program, built with
// -fsanitize=address,undefined by test_portfolio_cpu.py.
//
//   portfolio_driver IN OUT
// IN:  int32 n, T, stride, parts; int64 annualization; n bt_pf_lane; n int32 n_bars;
//      n*stride int64 equity; n*stride int8 pos
// OUT: the portfolio of all entries (T int64 pnl, T int64 equity, T int32 n_long, T int32 n_short,
//      one bt_pf_summary), then the same from `parts` portfolios of entries i % parts == k merged
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "portfolio.h"

static std::string g_err;
void bt::set_last_error(const std::string& s) { g_err = s; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

// exactly sized rows: a write past bar T - 1 is a heap overflow
struct Rows {
    std::vector<int64_t> pnl, eq;
    std::vector<int32_t> nl, ns;
    bt_pf_summary sum;
    explicit Rows(size_t T) : pnl(T), eq(T), nl(T), ns(T) { memset(&sum, 0, sizeof sum); }
    bool write(FILE* f) const {
        return wr(f, pnl.data(), pnl.size()) && wr(f, eq.data(), eq.size()) && wr(f, nl.data(), nl.size()) &&
               wr(f, ns.data(), ns.size()) && wr(f, &sum, 1);
    }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    int64_t ann;
    if (!rd(f, hdr, 4) || !rd(f, &ann, 1)) return 2;
    const int32_t n = hdr[0], T = hdr[1], stride = hdr[2], parts = hdr[3];
    std::vector<bt_pf_lane> lanes((size_t)n);
    std::vector<int32_t> nb((size_t)n);
    std::vector<int64_t> eq((size_t)n * stride);
    std::vector<int8_t> ps((size_t)n * stride);
    if (!rd(f, lanes.data(), lanes.size()) || !rd(f, nb.data(), nb.size()) || !rd(f, eq.data(), eq.size()) ||
        !rd(f, ps.data(), ps.size()))
        return 2;
    fclose(f);

    Rows all((size_t)T);
    if (bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, ann, all.pnl.data(),
                          all.eq.data(), all.nl.data(), all.ns.data(), &all.sum) != 0)
        return 3;
    // the summary alone equals the summary of the full call
    bt_pf_summary alone;
    if (bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, ann, nullptr, nullptr, nullptr,
                          nullptr, &alone) != 0 ||
        memcmp(&alone, &all.sum, sizeof alone) != 0)
        return 5;

    // entries i % parts == k as portfolios of their own, merged
    std::vector<int64_t> m_pnl((size_t)parts * T);
    std::vector<int32_t> m_nl((size_t)parts * T), m_ns((size_t)parts * T);
    std::vector<bt_pf_summary> m_sum((size_t)parts);
    for (int32_t k = 0; k < parts; ++k) {
        std::vector<bt_pf_lane> l;
        std::vector<int32_t> b;
        std::vector<int64_t> e;
        std::vector<int8_t> p;
        for (int32_t i = k; i < n; i += parts) {
            l.push_back(lanes[i]);
            b.push_back(nb[i]);
            e.insert(e.end(), eq.begin() + (size_t)i * stride, eq.begin() + (size_t)(i + 1) * stride);
            p.insert(p.end(), ps.begin() + (size_t)i * stride, ps.begin() + (size_t)(i + 1) * stride);
        }
        if (bt_portfolio_host((int32_t)l.size(), e.data(), p.data(), b.data(), stride, l.data(), T, ann,
                              m_pnl.data() + (size_t)k * T, nullptr, m_nl.data() + (size_t)k * T,
                              m_ns.data() + (size_t)k * T, &m_sum[k]) != 0)
            return 3;
    }
    Rows merged((size_t)T);
    if (bt_portfolio_merge(parts, T, m_pnl.data(), m_nl.data(), m_ns.data(), m_sum.data(), ann, merged.pnl.data(),
                           merged.eq.data(), merged.nl.data(), merged.ns.data(), &merged.sum) != 0)
        return 3;

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!all.write(f) || !merged.write(f)) return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    bt_pf_summary s;
    const bt_pf_lane neg{0, 0, -3, 5}, back{0, 0, 7, 6};
    const int32_t one_bar = 1;
    const int64_t e1 = 0;
    const int8_t p1 = 0;
    refused(bt_portfolio_host(-1, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(BT_PORTFOLIO_MAX + 1, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), 0, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), (1 << 22) + 1, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, ann, nullptr, nullptr, nullptr, nullptr, nullptr));
    refused(bt_portfolio_host(n, eq.data(), ps.data(), nb.data(), stride, lanes.data(), T, 0, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(1, &e1, &p1, &one_bar, 1, &neg, T, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_host(1, &e1, &p1, &one_bar, 1, &back, T, ann, nullptr, nullptr, nullptr, nullptr, &s));
    refused(bt_portfolio_merge(0, T, m_pnl.data(), m_nl.data(), m_ns.data(), m_sum.data(), ann, nullptr, nullptr, nullptr, nullptr, &s));

    // the resolution against a dataset of three rows, ids 7, 9 and 7 again (the first row wins)
    const bt::SymDesc syms[3] = {{0, 100, 7}, {128, 40, 9}, {192, 5000, 7}};
    bt::PfResolved rs;
    const bt_pf_lane good[4] = {{7, 1, 0, 1000}, {9, 0, 10, 20}, {9, 2, 40, 90}, {7, 0, 99, 100}};
    const bt_pf_lane unknown[1] = {{8, 0, 0, 10}}, param[2] = {{7, 0, 0, 10}, {9, 3, 0, 10}};
    printf("rule: %s\n", bt::portfolio_resolve(syms, 3, 3, 4, good, 64, rs).c_str());
    printf("resolved: %d %d %d %lld %zu %d\n", rs.n_lanes, rs.lo, rs.hi, (long long)rs.window_bars, rs.req.size(),
           rs.req.empty() ? -1 : rs.req[0].bars);
    printf("rule: %s\n", bt::portfolio_resolve(syms, 3, 3, 1, unknown, 64, rs).c_str());
    printf("rule: %s\n", bt::portfolio_resolve(syms, 3, 3, 2, param, 64, rs).c_str());
    printf("rule: %s\n", bt::portfolio_refusal(false, 0, false, 10, true).c_str());
    // 2^20 entries of 1,025 bars: one bar too many in all
    std::vector<bt_pf_lane> many((size_t)BT_PORTFOLIO_MAX, bt_pf_lane{7, 0, 0, 1025});
    printf("rule: %s\n", bt::portfolio_resolve(syms + 2, 1, 3, BT_PORTFOLIO_MAX, many.data(), 1 << 22, rs).c_str());
    many.assign((size_t)BT_PORTFOLIO_MAX, bt_pf_lane{7, 0, 0, 1024});
    printf("rule: %s\n", bt::portfolio_resolve(syms + 2, 1, 3, BT_PORTFOLIO_MAX, many.data(), 1 << 22, rs).c_str());
    printf("ok %d %d %d\n", n, T, parts);
    return 0;
}
