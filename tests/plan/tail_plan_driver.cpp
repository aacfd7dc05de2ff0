// tail_plan_driver — prints what bt_tail / bt_tail_of would launch, without a GPU: the TailPlan of
// csrc/plan.cpp as one JSON line, with the first and last chunks' units spelled out as analysis.cpp
// walks them.
//
//   tail_plan_driver units P Q list staged longest_n cus row_req budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int32_t units = atoi(argv[1]), P = atoi(argv[2]), Q = atoi(argv[3]), list = atoi(argv[4]), staged = atoi(argv[5]),
                  longest_n = atoi(argv[6]), cus = atoi(argv[7]), row_req = atoi(argv[8]);
    const int64_t req = atoll(argv[9]);
    const TailPlan pl = plan_tail(units, P, Q, list != 0, staged != 0, longest_n, cus, row_req, req);
    printf("{\"list\": %d, \"staged\": %d, \"Q\": %d, \"row_mode\": %d, \"row_refused\": %d, \"lds_row_cap\": %d, "
           "\"block\": %d, \"lds_bytes\": %zu, \"pitch\": %lld, \"per_chunk\": %d, \"chunks\": %d, \"unit_bytes\": %zu, "
           "\"need_bytes\": %zu, \"o_levels\": %zu, \"o_lanes\": %zu, \"o_rec\": %zu, \"o_q\": %zu, \"o_rows\": %zu, "
           "\"staging_bytes\": %zu, \"budget\": %zu, \"lds_cap_bytes\": %zu, \"fixed_bytes\": %zu, \"rec_bytes\": %zu, "
           "\"q_bytes\": %zu, \"lane_bytes\": %zu, \"units\": [",
           pl.list ? 1 : 0, pl.staged ? 1 : 0, pl.Q, pl.row_mode, pl.row_refused ? 1 : 0, pl.lds_row_cap, pl.block,
           pl.lds_bytes, (long long)pl.pitch, pl.per_chunk, pl.chunks, pl.unit_bytes, pl.need_bytes, pl.o_levels,
           pl.o_lanes, pl.o_rec, pl.o_q, pl.o_rows, pl.staging_bytes, kTailBudget, kTailLdsBytes, kTailFixedBytes,
           sizeof(bt_tail_rec), sizeof(bt_tail_q), sizeof(LaneRef));
    for (int64_t c = 0, r0 = 0; c < pl.chunks; ++c, r0 += pl.per_chunk) {
        const int64_t r1 = r0 + pl.per_chunk < units ? r0 + pl.per_chunk : units;
        if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)r0, (long long)r1);
    }
    printf("]}\n");
    return 0;
}
