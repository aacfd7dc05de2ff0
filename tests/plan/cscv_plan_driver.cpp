// cscv_plan_driver — prints what bt_cscv / bt_cscv_of would launch for G groups x P lanes x K folds,
// without a GPU: the CscvPlan of csrc/plan.cpp as one JSON line, with the regions of a full chunk
// in layout order, the launches of a full chunk as analysis.cpp issues them ([row0, rows, q0, q1],
// the first and the last four) and the mask table.
//
//   cscv_plan_driver G P K want_picks budget_req work_req
#include <cstdio>
#include <cstdlib>

#include "cscv.h"
#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int32_t G = atoi(argv[1]), P = atoi(argv[2]), K = atoi(argv[3]);
    const bool want = atoi(argv[4]) != 0;
    const int64_t budget = atoll(argv[5]), work = atoll(argv[6]);
    const CscvPlan pl = plan_cscv(G, P, K, want, budget, work);
    const size_t rows = (size_t)pl.rows_per_chunk;
    printf("{\"C\": %lld, \"pairs\": %lld, \"block\": %d, \"pack_block\": %d, \"rows_per_chunk\": %d, \"chunks\": %d, "
           "\"rows_per_launch\": %d, \"pairs_per_launch\": %lld, \"launches_per_row\": %d, \"row_bytes\": %zu, "
           "\"staging_bytes\": %zu, \"budget\": %zu, \"work\": %lld, ",
           (long long)pl.C, (long long)pl.pairs, pl.block, pl.pack_block, pl.rows_per_chunk, pl.chunks, pl.rows_per_launch,
           (long long)pl.pairs_per_launch, pl.launches_per_row, pl.row_bytes, pl.staging_bytes, kWalkfwdBudget,
           (long long)kCscvWork);
    printf("\"regions\": [[0, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu]], ",
           ((size_t)K + 1) * 4, pl.o_masks, (size_t)pl.pairs * 4, pl.o_rec, rows * (size_t)K * (size_t)P * sizeof(bt_fold),
           pl.o_sums, rows * (size_t)P * ((size_t)K + 1) * 32, pl.o_nret, rows * (size_t)K * 4, pl.o_groups,
           rows * sizeof(bt_cscv_group), pl.o_hist, rows * (2 * (size_t)P - 1) * 4, pl.o_picks,
           want ? rows * (size_t)pl.C * sizeof(bt_cscv_pick) : (size_t)0);
    // the launches of a full chunk
    int64_t n = 0, max_cells = 0;
    for (int64_t l0 = 0; l0 < pl.rows_per_chunk; l0 += pl.rows_per_launch)
        for (int64_t q0 = 0; q0 < pl.pairs; q0 += pl.pairs_per_launch) ++n;
    printf("\"launches\": %lld, \"launch_list\": [", (long long)n);
    int64_t i = 0;
    for (int64_t l0 = 0; l0 < pl.rows_per_chunk; l0 += pl.rows_per_launch)
        for (int64_t q0 = 0; q0 < pl.pairs; q0 += pl.pairs_per_launch, ++i) {
            const int64_t r = l0 + pl.rows_per_launch < pl.rows_per_chunk ? pl.rows_per_launch : pl.rows_per_chunk - l0;
            const int64_t q1 = q0 + pl.pairs_per_launch < pl.pairs ? q0 + pl.pairs_per_launch : pl.pairs;
            const int64_t cells = r * (q1 - q0) * P;
            if (cells > max_cells) max_cells = cells;
            if (i < 4 || i >= n - 4)
                printf("%s[%lld, %lld, %lld, %lld]", i ? ", " : "", (long long)l0, (long long)r, (long long)q0, (long long)q1);
        }
    printf("], \"max_cells\": %lld, \"masks\": [", (long long)max_cells);
    for (size_t q = 0; q < pl.masks.size(); ++q) printf("%s%u", q ? ", " : "", pl.masks[q]);
    printf("]}\n");
    return 0;
}
