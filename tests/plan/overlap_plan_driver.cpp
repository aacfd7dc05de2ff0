// overlap_plan_driver — prints whether the library would let a run overlap its neighbours
// (LaunchPlan::overlap of csrc/plan.cpp), with the segment count it follows from, without a GPU,
// as one JSON line.
//
//   overlap_plan_driver sma|ema_ols|boll a=1,2,3 b=4,5 [c=.. d=..] [band_bps=N] [k_den=N]
//                       sym=N bars=N cus=N [parity=1] [seg=N] [burn=N] [own=0|1] [on=0|1] [default=1]
//
// The grid and the shape are given as to plan_driver; own: the engine made its stream (0: the
// caller's), on: bt_set_run_overlap; both default to 1. default=1 leaves both to RunShape's own
// defaults instead. A refused grid prints {"error": "..."}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::map<std::string, std::string> kv;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        kv[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto num = [&](const char* k, int dflt) { return kv.count(k) ? atoi(kv[k].c_str()) : dflt; };
    std::vector<int32_t> ax[4];
    for (int i = 0; i < 4; ++i) {
        const std::string s = kv[std::string(1, (char)('a' + i))];
        for (const char* p = s.c_str(); *p;) {
            char* end;
            ax[i].push_back((int32_t)strtol(p, &end, 10));
            if (end == p) return 2;
            p = *end == ',' ? end + 1 : end;
        }
    }
    bt_config c{};
    const std::string strategy = argv[1];
    if (strategy == "sma") {
        c.strategy = BT_SMA_CROSS;
        c.fast = ax[0].data(), c.n_fast = (int32_t)ax[0].size();
        c.slow = ax[1].data(), c.n_slow = (int32_t)ax[1].size();
    } else if (strategy == "ema_ols") {
        c.strategy = BT_EMA_OLS;
        c.span = ax[0].data(), c.n_span = (int32_t)ax[0].size();
        c.ols = ax[1].data(), c.n_ols = (int32_t)ax[1].size();
        c.band_bps = num("band_bps", 0);
    } else if (strategy == "boll") {
        c.strategy = BT_BOLL;
        c.bwin = ax[0].data(), c.n_bwin = (int32_t)ax[0].size();
        c.k_num = ax[1].data(), c.n_k = (int32_t)ax[1].size();
        c.sl_bps = ax[2].data(), c.n_sl = (int32_t)ax[2].size();
        c.tp_bps = ax[3].data(), c.n_tp = (int32_t)ax[3].size();
        c.k_den = num("k_den", 0);
    } else {
        return 2;
    }
    Grid g{};
    const std::string err = plan_grid(c, g);
    if (!err.empty()) {
        printf("{\"error\": \"%s\"}\n", err.c_str());
        return 0;
    }
    RunShape r{num("sym", 0), num("bars", 0), num("parity", 0) != 0, num("seg", 0), num("burn", 0), num("cus", 0)};
    if (!num("default", 0)) {
        r.own_stream = num("own", 1) != 0;
        r.overlap_on = num("on", 1) != 0;
    }
    const LaunchPlan pl = plan_launch(g, ax[0].data(), r);
    printf("{\"G\": %d, \"overlap\": %d}\n", pl.G, (int)pl.overlap);
    return 0;
}
