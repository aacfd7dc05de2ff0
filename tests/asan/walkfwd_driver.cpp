// walkfwd_driver — csrc/walkfwd.cpp (bt_walk_forward_host, the totals, the refusal rules) as a
// stand-alone host program, built with -fsanitize=address,undefined by test_walkfwd_cpu.py.
//
//   walkfwd_driver IN OUT
// IN:  int32 S, P, K, train; int64 annualization; S*P*K bt_fold ([S][P][K]); S int32 ids
// OUT: S*n_steps bt_wf_step; S bt_fold totals; S bt_fold totals of a call without a steps buffer
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "walkfwd.h"

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
    const int32_t S = hdr[0], P = hdr[1], K = hdr[2], train = hdr[3];
    std::vector<bt_fold> folds((size_t)S * P * K);
    std::vector<int32_t> ids((size_t)S);
    if (!rd(f, folds.data(), folds.size()) || !rd(f, ids.data(), ids.size())) return 2;
    fclose(f);

    const int32_t n_steps = bt::walkfwd_steps(K, train);
    // exactly sized buffers: a write past a row's steps or past the totals is a heap overflow
    std::vector<bt_wf_step> steps((size_t)S * n_steps), steps_only((size_t)S * n_steps);
    std::vector<bt_fold> total((size_t)S), total_alone((size_t)S);
    bt_wf_step no_step;  // an empty vector has no address to pass for "steps wanted"
    bt_fold no_total;
    if (bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), ann, S ? steps.data() : &no_step,
                             S ? total.data() : &no_total) != 0)
        return 3;
    if (bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), ann, nullptr,
                             S ? total_alone.data() : &no_total) != 0)
        return 3;
    if (bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), ann, S ? steps_only.data() : &no_step,
                             nullptr) != 0)
        return 3;
    if (steps.size() && memcmp(steps.data(), steps_only.data(), steps.size() * sizeof(bt_wf_step)) != 0) return 5;

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, steps.data(), steps.size()) || !wr(f, total.data(), total.size()) ||
        !wr(f, total_alone.data(), total_alone.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    refused(bt_walk_forward_host(-1, P, K, train, folds.data(), ids.data(), ann, &no_step, nullptr));
    refused(bt_walk_forward_host(S, 0, K, train, folds.data(), ids.data(), ann, &no_step, nullptr));
    refused(bt_walk_forward_host(S, P, 1, 0, folds.data(), ids.data(), ann, &no_step, nullptr));
    refused(bt_walk_forward_host(S, P, K, K, folds.data(), ids.data(), ann, &no_step, nullptr));
    refused(bt_walk_forward_host(S, P, K, -1, folds.data(), ids.data(), ann, &no_step, nullptr));
    refused(bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), ann, nullptr, nullptr));
    refused(bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), 0, &no_step, nullptr));
    const int32_t up[3] = {0, 5, 5}, neg[2] = {-1, 5}, ok[3] = {0, 5, 9};
    for (const std::string& why : {bt::walkfwd_refusal(2, up, 0, true, false, false, 1, 1),
                                   bt::walkfwd_refusal(1, neg, 0, true, false, false, 1, 1),
                                   bt::walkfwd_refusal(2, ok, 1, true, true, true, 4096, 513),
                                   bt::walkfwd_refusal(2, ok, 1, true, true, true, 4096, 512),
                                   bt::walkfwd_refusal(2, ok, 1, false, true, true, 1 << 30, 1 << 20)})
        printf("rule: %s\n", why.c_str());
    if (bt_walk_forward_host(S, P, K, train, folds.data(), ids.data(), ann, S ? steps.data() : &no_step,
                             nullptr) != 0)
        return 3;
    printf("ok %d %d %d %d\n", S, P, K, train);
    return 0;
}
