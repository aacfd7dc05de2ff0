// cscv_driver — csrc/cscv.cpp (bt_cscv_host, the refusal rules) as a stand-alone host program, built
// with -fsanitize=address,undefined by test_cscv_cpu.py (plan_cscv runs under the sanitizers through
// tests/plan/cscv_plan_driver.cpp).
//
//   cscv_driver IN OUT
// IN:  int32 G, P, K, has_ids; int64 annualization; G*P*K bt_fold ([G][P][K]); G int32 ids when has_ids
// OUT: G bt_cscv_group; G*(2P-1) uint32; G*C bt_cscv_pick
// stdout: one "refused: <message>" line per refusal tried.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cscv.h"

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
    int32_t hdr[4];
    int64_t ann;
    if (!rd(f, hdr, 4) || !rd(f, &ann, 1)) return 2;
    const int32_t G = hdr[0], P = hdr[1], K = hdr[2];
    std::vector<bt_fold> folds((size_t)G * P * K);
    std::vector<int32_t> ids(hdr[3] ? (size_t)G : 0);
    if (!rd(f, folds.data(), folds.size()) || !rd(f, ids.data(), ids.size())) return 2;
    fclose(f);
    const int32_t* idp = hdr[3] ? ids.data() : nullptr;

    // exactly sized buffers: a write past a group's histogram or picks is a heap overflow
    const size_t C = (size_t)bt::cscv_combos(K), H = 2 * (size_t)P - 1;
    std::vector<bt_cscv_group> groups((size_t)G), groups_alone((size_t)G);
    std::vector<uint32_t> hist((size_t)G * H, 0xAAAAAAAAu), hist_alone((size_t)G * H);
    std::vector<bt_cscv_pick> picks((size_t)G * C), picks_alone((size_t)G * C);
    if (bt_cscv_host(G, P, K, folds.data(), idp, ann, groups.data(), hist.data(), picks.data()) != 0) return 3;
    if (bt_cscv_host(G, P, K, folds.data(), idp, ann, groups_alone.data(), nullptr, nullptr) != 0) return 3;
    if (bt_cscv_host(G, P, K, folds.data(), idp, ann, nullptr, hist_alone.data(), nullptr) != 0) return 3;
    if (bt_cscv_host(G, P, K, folds.data(), idp, ann, nullptr, nullptr, picks_alone.data()) != 0) return 3;
    if (memcmp(groups.data(), groups_alone.data(), groups.size() * sizeof(bt_cscv_group)) != 0 || hist != hist_alone ||
        memcmp(picks.data(), picks_alone.data(), picks.size() * sizeof(bt_cscv_pick)) != 0)
        return 5;

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, groups.data(), groups.size()) || !wr(f, hist.data(), hist.size()) || !wr(f, picks.data(), picks.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    bt_cscv_group one;
    refused(bt_cscv_host(G, P, 3, folds.data(), idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(G, P, 0, folds.data(), idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(G, P, 22, folds.data(), idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(G, P, K, folds.data(), idp, ann, nullptr, nullptr, nullptr));
    refused(bt_cscv_host(G, 0, K, folds.data(), idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(-1, P, K, folds.data(), idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(1, P, K, nullptr, idp, ann, &one, nullptr, nullptr));
    refused(bt_cscv_host(G, P, K, folds.data(), idp, 0, groups.data(), nullptr, nullptr));
    refused(bt_cscv_host(1 << 20, 1, 4, folds.data(), idp, ann, nullptr, nullptr, picks.data()));
    if (G > 0) {    // one record spoilt at a time, in the last lane's last fold
        const size_t last = (size_t)P * K - 1;
        auto spoilt = [&](auto edit) {
            std::vector<bt_fold> bad(folds.begin(), folds.begin() + (size_t)P * K);
            edit(bad[last]);
            refused(bt_cscv_host(1, P, K, bad.data(), nullptr, ann, &one, nullptr, nullptr));
        };
        spoilt([](bt_fold& r) { r.s2_hi = -1; });
        spoilt([](bt_fold& r) { r.s2_hi = 1LL << 56; });
        spoilt([](bt_fold& r) { r.s1_hi = 1LL << 56; r.s1_lo = 0; });
        spoilt([](bt_fold& r) { r.s1_hi = -(1LL << 56); r.s1_lo = 0; });
        spoilt([](bt_fold& r) { r.n_bars = -1; });
        if (P > 1) spoilt([](bt_fold& r) { r.n_bars += 1; });
    }
    if (bt_cscv_host(0, P, K, nullptr, nullptr, ann, &one, nullptr, nullptr) != 0) return 3;   // writes nothing

    printf("ok %d %d %d\n", G, P, K);
    return 0;
}
