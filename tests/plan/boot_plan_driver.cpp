// boot_plan_driver — prints what bt_bootstrap / bt_bootstrap_of would launch, without a GPU: the
// BootPlan of csrc/plan.cpp as one JSON line, with the first and last chunks' lanes spelled out as
// analysis.cpp walks them.
//
//   boot_plan_driver n G T B L list staged want_boot cus row_req budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 12) return 2;
    const int64_t n = atoll(argv[1]), G = atoll(argv[2]);
    const int32_t T = atoi(argv[3]), B = atoi(argv[4]), L = atoi(argv[5]);
    const bool list = atoi(argv[6]) != 0, staged = atoi(argv[7]) != 0, want_boot = atoi(argv[8]) != 0;
    const int cus = atoi(argv[9]);
    const int32_t row_req = atoi(argv[10]);
    const int64_t req = atoll(argv[11]);
    const BootPlan pl = plan_boot(n, G, T, B, L, list, staged, want_boot, cus, row_req, req);
    printf("{\"T\": %d, \"Lp\": %d, \"K\": %d, \"last_len\": %d, \"row_mode\": %d, \"row_refused\": %d, \"waves\": %d, "
           "\"block\": %d, \"lds_bytes\": %zu, \"pitch\": %lld, \"d_pitch\": %lld, \"per_chunk\": %d, \"chunks\": %d, "
           "\"starts_block\": %d, \"starts_blocks\": %lld, \"finish_block\": %d, \"o_starts\": %zu, \"o_goff\": %zu, "
           "\"o_vmax\": %zu, \"o_groups\": %zu, \"o_rec\": %zu, \"o_boot\": %zu, \"o_lanes\": %zu, \"o_gid\": %zu, "
           "\"o_rows\": %zu, \"o_d\": %zu, \"unit_bytes\": %zu, \"need_bytes\": %zu, \"staging_bytes\": %zu, "
           "\"budget\": %zu, \"lds_limit\": %zu, \"red_bytes\": %zu, \"max_waves\": %d, \"lane_rec\": %zu, "
           "\"group_rec\": %zu, \"lane_ref\": %zu, \"units\": [",
           pl.T, pl.Lp, pl.K, pl.last_len, pl.row_mode, pl.row_refused ? 1 : 0, pl.waves, pl.block, pl.lds_bytes,
           (long long)pl.pitch, (long long)pl.d_pitch, pl.per_chunk, pl.chunks, pl.starts_block,
           (long long)pl.starts_blocks, pl.finish_block, pl.o_starts, pl.o_goff, pl.o_vmax, pl.o_groups, pl.o_rec,
           pl.o_boot, pl.o_lanes, pl.o_gid, pl.o_rows, pl.o_d, pl.unit_bytes, pl.need_bytes, pl.staging_bytes,
           kBootBudget, kBootLdsBytes, kBootRedBytes, kBootMaxWaves, sizeof(bt_boot_lane), sizeof(bt_boot_group),
           sizeof(LaneRef));
    for (int64_t c = 0, r0 = 0; c < pl.chunks; ++c, r0 += pl.per_chunk) {
        const int64_t r1 = r0 + pl.per_chunk < n ? r0 + pl.per_chunk : n;
        if (c < 4 || c >= pl.chunks - 4) printf("%s[%lld, %lld]", c ? ", " : "", (long long)r0, (long long)r1);
    }
    printf("]}\n");
    return 0;
}
