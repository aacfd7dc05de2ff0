// replay_plan_driver — what bt_replay decides on the host, without a GPU: the ReplayPlan of
// csrc/plan.cpp and the rules of csrc/replay.cpp, one JSON line per call.
//
//   replay_plan_driver plan n W trade_cap stride equity pos budget_req
//   replay_plan_driver refusal have_dataset n trade_cap have_trades have_lanes have_sum
//   replay_plan_driver resolve P curves stride [sym:param ...]
//
// `resolve` runs against a fixed dataset of three rows: 64, 65 and 1,000 bars with ids 907, 12 and
// 907 again (the first row of a repeated id wins), laid out 64-aligned as the engine does.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "plan.h"
#include "replay.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan") && argc == 9) {
        const int32_t n = atoi(argv[2]), W = atoi(argv[3]), cap = atoi(argv[4]);
        const ReplayPlan pl = plan_replay(n, W, cap, atoll(argv[5]), atoi(argv[6]) != 0, atoi(argv[7]) != 0,
                                          (size_t)atoll(argv[8]));
        printf("{\"dcap\": %lld, \"pitch\": %lld, \"lanes_per_chunk\": %d, \"chunks\": %d, \"o_lane\": %zu, "
               "\"o_sum\": %zu, \"o_trades\": %zu, \"o_equity\": %zu, \"o_pos\": %zu, \"staging_bytes\": %zu, "
               "\"budget\": %zu, \"lane_bytes\": %zu, \"summary_bytes\": %zu, \"trade_bytes\": %zu, \"lanes\": [",
               (long long)pl.dcap, (long long)pl.pitch, pl.lanes_per_chunk, pl.chunks, pl.o_lane, pl.o_sum,
               pl.o_trades, pl.o_equity, pl.o_pos, pl.staging_bytes, kReplayBudget, sizeof(ReplayLane),
               sizeof(bt_summary), sizeof(bt_trade));
        // the lanes of chunk c as analysis.cpp walks them (the first and last four chunks)
        for (int64_t c = 0, i0 = 0; c < pl.chunks; ++c, i0 += pl.lanes_per_chunk) {
            const int64_t i1 = i0 + pl.lanes_per_chunk < n ? i0 + pl.lanes_per_chunk : n;
            if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)i0, (long long)i1);
        }
        printf("]}\n");
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "refusal")) {
        printf("{\"why\": \"%s\"}\n", replay_refusal(atoi(argv[2]) != 0, atoll(argv[3]), atoll(argv[4]), atoi(argv[5]) != 0,
                                                     atoi(argv[6]) != 0, atoi(argv[7]) != 0).c_str());
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "resolve")) {
        const SymDesc syms[3] = {{0, 64, 907}, {64, 65, 12}, {192, 1000, 907}};
        std::vector<bt_lane> lanes;
        for (int i = 5; i < argc; ++i) {
            const char* colon = strchr(argv[i], ':');
            if (!colon) return 2;
            lanes.push_back(bt_lane{atoi(argv[i]), atoi(colon + 1)});
        }
        std::vector<ReplayLane> req;
        int32_t W = -1;
        const std::string why = replay_resolve(syms, 3, atoi(argv[2]), (int32_t)lanes.size(), lanes.data(),
                                               atoi(argv[3]) != 0, atoll(argv[4]), req, W);
        printf("{\"why\": \"%s\", \"W\": %d, \"lanes\": [", why.c_str(), W);
        if (why.empty())
            for (size_t i = 0; i < req.size(); ++i)
                printf("%s[%lld, %d, %d]", i ? ", " : "", (long long)req[i].off, req[i].bars, req[i].param);
        printf("]}\n");
        return 0;
    }
    return 2;
}
