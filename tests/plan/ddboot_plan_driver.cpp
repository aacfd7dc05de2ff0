// ddboot_plan_driver — prints what bt_drawdown_boot / bt_drawdown_boot_of would launch, without a
// GPU: the DdPlan of csrc/plan.cpp as one JSON line, with the first and last chunks' lanes spelled
// out as analysis.cpp walks them.
//
//   ddboot_plan_driver n T B L Q R list staged raw cus row_req budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 13) return 2;
    const int64_t n = atoll(argv[1]);
    const int32_t T = atoi(argv[2]), B = atoi(argv[3]), L = atoi(argv[4]), Q = atoi(argv[5]), R = atoi(argv[6]),
                  list = atoi(argv[7]), staged = atoi(argv[8]), raw = atoi(argv[9]), cus = atoi(argv[10]),
                  row_req = atoi(argv[11]);
    const int64_t req = atoll(argv[12]);
    const DdPlan pl = plan_ddboot(n, T, B, L, Q, R, list != 0, staged != 0, raw != 0, cus, row_req, req);
    printf("{\"T\": %d, \"Lp\": %d, \"K\": %d, \"last_len\": %d, \"two_tables\": %d, \"scan1\": %d, \"scan2\": %d, "
           "\"row_mode\": %d, \"row_refused\": %d, \"r_w1\": %zu, \"r_w2\": %zu, \"row_bytes\": %zu, "
           "\"block\": %d, \"lds_bytes\": %zu, \"l_vals\": %zu, \"pitch\": %lld, \"d_pitch\": %lld, \"v_pitch\": %lld, "
           "\"per_chunk\": %d, \"chunks\": %d, \"starts_block\": %d, \"starts_blocks\": %lld, ",
           pl.T, pl.Lp, pl.K, pl.last_len, pl.two_tables ? 1 : 0, pl.scan1 ? 1 : 0, pl.scan2 ? 1 : 0, pl.row_mode,
           pl.row_refused ? 1 : 0, pl.r_w1, pl.r_w2, pl.row_bytes, pl.block, pl.lds_bytes, pl.l_vals,
           (long long)pl.pitch, (long long)pl.d_pitch, (long long)pl.v_pitch, pl.per_chunk, pl.chunks, pl.starts_block,
           (long long)pl.starts_blocks);
    printf("\"o_starts\": %zu, \"o_levels\": %zu, \"o_limits\": %zu, \"o_lanes\": %zu, \"o_rec\": %zu, \"o_q\": %zu, "
           "\"o_reach\": %zu, \"o_raw\": %zu, \"o_rows\": %zu, \"o_vals\": %zu, \"o_d\": %zu, \"unit_bytes\": %zu, "
           "\"need_bytes\": %zu, \"staging_bytes\": %zu, \"budget\": %zu, \"lds_cap_bytes\": %zu, "
           "\"fixed_bytes\": %zu, \"entry_bytes\": %zu, \"rec_bytes\": %zu, \"lane_bytes\": %zu, \"lanes\": [",
           pl.o_starts, pl.o_levels, pl.o_limits, pl.o_lanes, pl.o_rec, pl.o_q, pl.o_reach, pl.o_raw, pl.o_rows, pl.o_vals,
           pl.o_d, pl.unit_bytes, pl.need_bytes, pl.staging_bytes, kDdBudget, kDdLdsBytes, kDdFixedBytes,
           kDdEntryBytes, sizeof(bt_dd_lane), sizeof(LaneRef));
    for (int64_t c = 0, r0 = 0; c < pl.chunks; ++c, r0 += pl.per_chunk) {
        const int64_t r1 = r0 + pl.per_chunk < n ? r0 + pl.per_chunk : n;
        if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)r0, (long long)r1);
    }
    printf("]}\n");
    return 0;
}
