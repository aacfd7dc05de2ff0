// surface_driver — csrc/surface.cpp (bt_surface_host, bt_surface_merge, the refusal rules) as a
// stand-alone host program, built with -fsanitize=address,undefined by test_surface_cpu.py.
//
//   surface_driver IN OUT
// IN:  int32 S, P, n_parts; n_parts + 1 int32 row cuts (0 .. S, ascending); S*P bt_summary; S int32 ids
// OUT: P bt_param_agg of the whole matrix; S bt_topk_rec; P bt_param_agg merged from the parts
// stdout: one "refused: <message>" line per refusal tried.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "surface.h"

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
    int32_t hdr[3];
    if (!rd(f, hdr, 3)) return 2;
    const int32_t S = hdr[0], P = hdr[1], parts = hdr[2];
    std::vector<int32_t> cut((size_t)parts + 1), ids((size_t)S);
    std::vector<bt_summary> sum((size_t)S * P);
    if (!rd(f, cut.data(), cut.size()) || !rd(f, sum.data(), sum.size()) || !rd(f, ids.data(), ids.size())) return 2;
    fclose(f);

    std::vector<bt_param_agg> agg((size_t)P), merged((size_t)P), block((size_t)parts * P);
    std::vector<bt_topk_rec> best((size_t)S), part_best((size_t)S);
    if (bt_surface_host(S, P, sum.data(), ids.data(), agg.data(), best.data()) != 0) return 3;
    for (int32_t w = 0; w < parts; ++w) {
        const int32_t r0 = cut[w], n = cut[w + 1] - cut[w];
        if (bt_surface_host(n, P, sum.data() + (size_t)r0 * P, ids.data() + r0, block.data() + (size_t)w * P,
                            part_best.data() + r0) != 0)
            return 3;
    }
    if (bt_surface_merge(block.data(), parts, P, merged.data()) != 0) return 3;
    // either output alone
    std::vector<bt_param_agg> agg2((size_t)P);
    std::vector<bt_topk_rec> best2((size_t)S);
    if (bt_surface_host(S, P, sum.data(), ids.data(), agg2.data(), nullptr) != 0) return 3;
    bt_topk_rec none;  // an empty vector has no address to pass for "best wanted"
    if (bt_surface_host(S, P, sum.data(), ids.data(), nullptr, S ? best2.data() : &none) != 0) return 3;

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, agg.data(), agg.size()) || !wr(f, best.data(), best.size()) || !wr(f, merged.data(), merged.size()) ||
        !wr(f, part_best.data(), part_best.size()) || !wr(f, agg2.data(), agg2.size()) ||
        !wr(f, best2.data(), best2.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    refused(bt_surface_host(-1, P, sum.data(), ids.data(), agg.data(), nullptr));
    refused(bt_surface_host(S, 0, sum.data(), ids.data(), agg.data(), nullptr));
    refused(bt_surface_host(S, P, sum.data(), ids.data(), nullptr, nullptr));
    refused(bt_surface_merge(block.data(), 0, P, merged.data()));
    for (const std::string& why : {bt::surface_refusal(4096, 1025, true, true, 0),
                                   bt::surface_refusal(3, 2, true, false, 1ULL << 32),
                                   bt::surface_refusal(3, 2, true, false, (1ULL << 32) - 1),
                                   bt::surface_refusal(4096, 1024, true, true, 0)})
        printf("rule: %s\n", why.c_str());
    if (bt_surface_host(S, P, sum.data(), ids.data(), agg2.data(), nullptr) != 0) return 3;
    printf("ok %d %d %d\n", S, P, parts);
    return 0;
}
