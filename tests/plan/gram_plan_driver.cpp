// gram_plan_driver — prints what bt_covariance / bt_gram_of would launch for n lanes over T bars,
// without a GPU: the GramPlan of csrc/plan.cpp as one JSON line.
//
//   gram_plan_driver n T cus split_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int32_t n = atoi(argv[1]), T = atoi(argv[2]), cus = atoi(argv[3]), req = atoi(argv[4]);
    const GramPlan pl = plan_gram(n, T, cus, req);
    printf("{\"nt\": %d, \"tiles\": %d, \"chunks\": %d, \"chunk_bars\": %d, \"fold_block\": %d, \"pitch\": %lld, "
           "\"fill\": %.6f, \"o_lanes\": %zu, \"o_d\": %zu, \"o_partial\": %zu, \"o_gram\": %zu, \"o_sums\": %zu, "
           "\"d_bytes\": %zu, \"out_bytes\": %zu, \"staging_bytes\": %zu, \"lane_bytes\": %zu, \"wide_bytes\": %zu, "
           "\"staging_max\": %zu, \"partial_budget\": %zu, \"min_chunk_bars\": %d, \"waves_per_cu\": %d}\n",
           pl.nt, pl.tiles, pl.chunks, pl.chunk_bars, pl.fold_block, (long long)pl.pitch, pl.fill, pl.o_lanes, pl.o_d,
           pl.o_partial, pl.o_gram, pl.o_sums, pl.d_bytes, pl.out_bytes, pl.staging_bytes, sizeof(ReplayLane),
           sizeof(bt_wide), kGramStagingMax, kGramPartialBudget, kGramMinChunkBars, kGramWavesPerCu);
    return 0;
}
