// walkfwd_plan_driver — prints what bt_walk_forward would launch for S rows x P params x K folds,
// without a GPU: the WalkfwdPlan of csrc/plan.cpp as one JSON line, with every chunk's rows
// spelled out as analysis.cpp walks them.
//
//   walkfwd_plan_driver S P K max_bars cus budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int32_t S = atoi(argv[1]), P = atoi(argv[2]), K = atoi(argv[3]), bars = atoi(argv[4]), cus = atoi(argv[5]);
    const int64_t req = atoll(argv[6]);
    const WalkfwdPlan pl = plan_walkfwd(S, P, K, bars, cus, req);
    printf("{\"rows_per_chunk\": %d, \"chunks\": %d, \"sel_block\": %d, \"tiles\": %d, \"waves\": %lld, "
           "\"fill\": %.6f, \"bounds_bytes\": %zu, \"row_bytes\": %zu, \"staging_bytes\": %zu, \"budget\": %zu, "
           "\"fold_bytes\": %zu, \"step_bytes\": %zu, \"o_rec\": %zu, \"o_steps\": %zu, \"rows\": [",
           pl.rows_per_chunk, pl.chunks, pl.sel_block, pl.tiles, (long long)pl.waves, pl.fill, pl.bounds_bytes,
           pl.row_bytes, pl.staging_bytes, kWalkfwdBudget, sizeof(bt_fold), sizeof(bt_wf_step), pl.o_rec,
           pl.o_steps);
    for (int64_t c = 0, r0 = 0; c < pl.chunks; ++c, r0 += pl.rows_per_chunk) {
        const int64_t r1 = r0 + pl.rows_per_chunk < S ? r0 + pl.rows_per_chunk : S;
        if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)r0, (long long)r1);
    }
    printf("]}\n");
    return 0;
}
