// costs_plan_driver — prints what bt_costs would launch, without a GPU: the CostsPlan of
// csrc/plan.cpp as one JSON line, with the first and last chunks' units spelled out as
// analysis.cpp walks them.
//
//   costs_plan_driver units P C list cus budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int32_t units = atoi(argv[1]), P = atoi(argv[2]), C = atoi(argv[3]), list = atoi(argv[4]), cus = atoi(argv[5]);
    const int64_t req = atoll(argv[6]);
    const CostsPlan pl = plan_costs(units, P, C, list != 0, cus, req);
    printf("{\"list\": %d, \"C\": %d, \"per_chunk\": %d, \"chunks\": %d, \"waves\": %lld, \"fill\": %.6f, "
           "\"agg_block\": %d, \"agg_pblocks\": %d, \"agg_slices\": %d, \"unit_bytes\": %zu, \"o_agg\": %zu, "
           "\"o_lanes\": %zu, \"o_rec\": %zu, \"staging_bytes\": %zu, \"budget\": %zu, \"rec_bytes\": %zu, "
           "\"agg_bytes\": %zu, \"lane_bytes\": %zu, \"slice_rows\": %d, \"max_slices\": %d, \"units\": [",
           pl.list ? 1 : 0, pl.C, pl.per_chunk, pl.chunks, (long long)pl.waves, pl.fill, pl.agg_block, pl.agg_pblocks,
           pl.agg_slices, pl.unit_bytes, pl.o_agg, pl.o_lanes, pl.o_rec, pl.staging_bytes, kCostsBudget,
           sizeof(bt_cost_rec), sizeof(bt_cost_agg), sizeof(LaneRef), kCostsSliceRows, kCostsMaxSlices);
    for (int64_t c = 0, r0 = 0; c < pl.chunks; ++c, r0 += pl.per_chunk) {
        const int64_t r1 = r0 + pl.per_chunk < units ? r0 + pl.per_chunk : units;
        if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)r0, (long long)r1);
    }
    printf("]}\n");
    return 0;
}
