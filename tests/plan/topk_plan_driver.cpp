// topk_plan_driver — what bt_topk_of and bt_load_ohlc decide on the host, without a GPU: the
// TopkOfPlan of csrc/plan.cpp and the rules of csrc/topk_rules.cpp, one JSON line per call.
//
//   topk_plan_driver plan S P
//   topk_plan_driver refusal S P k have_sum have_ids have_out [id ...]
//   topk_plan_driver ids [id ...]
//
// `refusal` passes the ids given (int32, zeros after them up to S), `ids` checks a dataset's int64
// ids.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plan.h"
#include "topk_rules.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "plan")) {
        const TopkOfPlan pl = plan_topk_of(atoi(argv[2]), atoi(argv[3]));
        printf("{\"o_key\": %zu, \"o_sum\": %zu, \"o_syms\": %zu, \"o_hist\": %zu, \"o_state\": %zu, \"o_counts\": %zu, "
               "\"o_above\": %zu, \"o_cand\": %zu, \"o_out\": %zu, \"staging_bytes\": %zu, \"summary_bytes\": %zu, "
               "\"sym_bytes\": %zu, \"rec_bytes\": %zu, \"cap\": %d, \"kmax\": %d}\n",
               pl.o_key, pl.o_sum, pl.o_syms, pl.o_hist, pl.o_state, pl.o_counts, pl.o_above, pl.o_cand, pl.o_out,
               pl.staging_bytes, sizeof(bt_summary), sizeof(SymDesc), sizeof(bt_topk_rec), kTopkCap, kTopkMax);
        return 0;
    }
    if (argc >= 8 && !strcmp(argv[1], "refusal")) {
        const int64_t S = atoll(argv[2]);
        std::vector<int32_t> ids;
        for (int i = 8; i < argc; ++i) ids.push_back((int32_t)atoll(argv[i]));
        const bool have_ids = atoi(argv[6]) != 0;
        if (S > 0 && S <= kTopkOfMax && (int64_t)ids.size() < S) ids.resize((size_t)S, 0);
        printf("{\"why\": \"%s\"}\n", topk_of_refusal(S, atoll(argv[3]), atoll(argv[4]), atoi(argv[5]) != 0,
                                                     have_ids ? ids.data() : nullptr, atoi(argv[7]) != 0).c_str());
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "ids")) {
        std::vector<int64_t> ids;
        for (int i = 2; i < argc; ++i) ids.push_back(atoll(argv[i]));
        printf("{\"why\": \"%s\"}\n", sym_id_refusal((int64_t)ids.size(), ids.data()).c_str());
        return 0;
    }
    return 2;
}
