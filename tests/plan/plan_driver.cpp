// plan_driver — prints what the library would launch for a shard, without a GPU: the grid's ring
// and the LaunchPlan of csrc/plan.cpp for a shape given on the command line, as one JSON line.
//
//   plan_driver sma|ema_ols|boll a=1,2,3 b=4,5 [c=.. d=..] [band_bps=N] [k_den=N]
//               sym=N bars=N cus=N [parity=1] [seg=N] [burn=N]
//
// a..d are the grid's axes in Grid order (SMA fast, slow; EMA+OLS span, ols; Bollinger bwin,
// k_num, sl_bps, tp_bps). A refused grid prints {"error": "..."}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "lds_layout.h"
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
    auto num = [&](const char* k) { return kv.count(k) ? atoi(kv[k].c_str()) : 0; };
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
        c.band_bps = num("band_bps");
    } else if (strategy == "boll") {
        c.strategy = BT_BOLL;
        c.bwin = ax[0].data(), c.n_bwin = (int32_t)ax[0].size();
        c.k_num = ax[1].data(), c.n_k = (int32_t)ax[1].size();
        c.sl_bps = ax[2].data(), c.n_sl = (int32_t)ax[2].size();
        c.tp_bps = ax[3].data(), c.n_tp = (int32_t)ax[3].size();
        c.k_den = num("k_den");
    } else {
        return 2;
    }
    Grid g{};
    const std::string err = plan_grid(c, g);
    if (!err.empty()) {
        printf("{\"error\": \"%s\"}\n", err.c_str());
        return 0;
    }
    const RunShape r{num("sym"), num("bars"), num("parity") != 0, num("seg"), num("burn"), num("cus")};
    const LaunchPlan pl = plan_launch(g, ax[0].data(), r);
    printf("{\"n_params\": %d, \"wmax\": %d, \"ring\": %d, \"kmin_idx\": %d, ", g.n_params, g.wmax, g.ring,
           g.kmin_idx);
    if (c.strategy == BT_EMA_OLS)  // the block's LDS at 64-bar and at 128-bar stages
        printf("\"ema_lds\": [%zu, %zu], ", tile_lds_layout(0, g.ring, g.na, g.nb, 0, 1).total,
               tile_lds_layout(0, g.ring, g.na, g.nb, 0, 2).total);
    printf("\"G\": %d, \"burn_tiles\": %d, \"grid_y\": %d, \"block\": %d, \"lds\": %zu, \"dedicated\": %d, "
           "\"one_trip\": %d, \"ts\": %d, \"xw\": %d, \"lpw\": %d, \"split_grp\": %d, \"wmap\": %u, "
           "\"seg_slots\": %zu, \"pos_off\": %zu, \"pos_bytes\": %zu, \"ema_doubles\": %zu, "
           "\"topk_lds_free\": %d}\n",
           pl.G, pl.burn_tiles, pl.grid_y, pl.block, pl.lds, pl.dedicated, pl.one_trip, pl.ts, pl.xw, pl.lpw,
           pl.split_grp, pl.wmap, pl.seg_slots, pl.pos_off, pl.pos_bytes, pl.ema_doubles,
           (int)pl.topk_lds_free);
    return 0;
}
