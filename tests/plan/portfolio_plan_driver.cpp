// portfolio_plan_driver — prints what bt_portfolio would launch for n entries over T bars, without
// a GPU: the PortfolioPlan of csrc/plan.cpp as one JSON line.
//
//   portfolio_plan_driver n T cus replicas_req budget_req
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int32_t n = atoi(argv[1]), T = atoi(argv[2]), cus = atoi(argv[3]), req = atoi(argv[4]);
    const size_t budget = (size_t)atoll(argv[5]);
    const PortfolioPlan pl = plan_portfolio(n, T, cus, req, budget);
    printf("{\"R\": %d, \"finish_block\": %d, \"pitch\": %lld, \"tiles\": %d, \"fill\": %.6f, \"o_lanes\": %zu, "
           "\"o_acc_pnl\": %zu, \"o_acc_cnt\": %zu, \"o_pnl\": %zu, \"o_equity\": %zu, \"o_long\": %zu, "
           "\"o_short\": %zu, \"o_sum\": %zu, \"acc_bytes\": %zu, \"out_bytes\": %zu, \"staging_bytes\": %zu, "
           "\"lane_bytes\": %zu, \"summary_bytes\": %zu, \"acc_budget\": %zu, \"max_replicas\": %d}\n",
           pl.R, pl.finish_block, (long long)pl.pitch, pl.tiles, pl.fill, pl.o_lanes, pl.o_acc_pnl, pl.o_acc_cnt,
           pl.o_pnl, pl.o_equity, pl.o_long, pl.o_short, pl.o_sum, pl.acc_bytes, pl.out_bytes, pl.staging_bytes,
           sizeof(PfLane), sizeof(bt_pf_summary), kPortfolioAccBudget, kPortfolioMaxReplicas);
    return 0;
}
