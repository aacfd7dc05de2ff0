// boot_driver — csrc/bootstrap.cpp (bt_bootstrap_host and the argument rules) as a stand-alone host
// program, built with -fsanitize=address,undefined by test_bootstrap_cpu.py.
//
//   boot_driver IN OUT
// IN:  int32 n, G, stride, from, to, B, L, has_goff; uint64 seed; int32 goff[G + 1] (when has_goff);
//      int32 n_bars[n]; int64 equity[n][stride]
// OUT: G bt_boot_group; n bt_boot_lane; G * B int64 vmax; n * B int64 boot
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bootstrap.h"

static std::string g_err;
void bt::set_last_error(const std::string& s) { g_err = s; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[8];
    uint64_t seed;
    if (!rd(f, h, 8) || !rd(f, &seed, 1)) return 2;
    const int32_t n = h[0], G = h[1], stride = h[2], from = h[3], to = h[4], B = h[5], L = h[6];
    // exactly sized buffers: a read or write past a row, a group or a resample is a heap overflow
    std::vector<int32_t> goff(h[7] ? (size_t)G + 1 : 0), n_bars((size_t)n);
    std::vector<int64_t> equity((size_t)n * (size_t)stride);
    if (!rd(f, goff.data(), goff.size()) || !rd(f, n_bars.data(), n_bars.size()) || !rd(f, equity.data(), equity.size()))
        return 2;
    fclose(f);
    std::vector<bt_boot_group> groups((size_t)G);
    std::vector<bt_boot_lane> lanes((size_t)n);
    std::vector<int64_t> vmax((size_t)G * (size_t)B), boot((size_t)n * (size_t)B);
    const int32_t* go = h[7] ? goff.data() : nullptr;
    if (bt_bootstrap_host(n, equity.data(), n_bars.data(), stride, G, go, from, to, B, L, seed, groups.data(), lanes.data(),
                          vmax.data(), boot.data()) != 0) {
        fprintf(stderr, "%s\n", g_err.c_str());
        return 3;
    }
    // each output alone gives the same bytes
    std::vector<bt_boot_group> g2((size_t)G);
    if (bt_bootstrap_host(n, equity.data(), n_bars.data(), stride, G, go, from, to, B, L, seed, g2.data(), nullptr, nullptr,
                          nullptr) != 0)
        return 3;
    for (int32_t g = 0; g < G; ++g)
        if (g2[(size_t)g].n_ge != groups[(size_t)g].n_ge || g2[(size_t)g].best_lane != groups[(size_t)g].best_lane) return 5;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, groups.data(), groups.size()) || !wr(f, lanes.data(), lanes.size()) || !wr(f, vmax.data(), vmax.size()) ||
        !wr(f, boot.data(), boot.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    const int64_t eq[6] = {0, 5, -2, 1, 1, 4};
    const int32_t nb[2] = {3, 2}, two[3] = {0, 1, 2}, empty[3] = {0, 0, 2}, late[2] = {1, 2}, shortg[3] = {0, 1, 1};
    bt_boot_group gr[2];
    refused(bt_bootstrap_host(0, eq, nb, 3, 1, nullptr, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, nullptr, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 3, two, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, empty, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 1, late, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, shortg, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, -1, 2, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 2, 2, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, (1 << 22) + 1, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 0, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 65537, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 4, 0, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 4, (1 << 22) + 1, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 4, 2, 1, nullptr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, nullptr, nb, 3, 2, two, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    refused(bt_bootstrap_host(2, eq, nb, 2, 2, two, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr));
    const int32_t bad_d[4] = {1, 2, INT32_MIN, 3};
    int32_t Tw = 0;
    for (const std::string& why :
         {bt::boot_refusal(bt::BootCall{false, false, false, false, 0, 0, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, false, false, false, 0, 0, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, true, false, false, 3, 0, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, true, false, false, 0, 2, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, true, false, false, 0, 0, nullptr, 0, 0, 10, 5, true, true}),
          bt::boot_refusal(bt::BootCall{true, true, false, true, (int64_t)BT_BOOT_MAX + 1, 0, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, false, true, false, 2, 0, nullptr, 0, 3, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, true, false, false, 0, 0, nullptr, 0, 0, 10, 5, true, false}),
          bt::boot_refusal(bt::BootCall{true, true, false, true, 2, 2, two, 0, 0, 65536, 1 << 22, true, true}),
          bt::boot_window(0, 0, 0, Tw), bt::boot_window(5, 4, 100, Tw), bt::boot_window(0, 0, 2520, Tw),
          bt::boot_domain_refusal(2, 2, bad_d), bt::boot_budget_refusal(1000, 999), bt::boot_budget_refusal(1000, 1000),
          bt::boot_row_refusal(8128, 8129 * 8, 65024), bt::boot_row_refusal(8127, 8128 * 8, 65024)})
        printf("rule: %s\n", why.c_str());
    if (bt_bootstrap_host(2, eq, nb, 3, 2, two, 0, 0, 4, 2, 1, gr, nullptr, nullptr, nullptr) != 0 || gr[0].best_sum != -2 ||
        gr[1].best_sum != 1 || gr[0].n_lanes != 1)
        return 5;
    printf("ok %d %d\n", n, G);
    return 0;
}
