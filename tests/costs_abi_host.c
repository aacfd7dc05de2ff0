/* costs_abi_host — the two records of bt_costs (include/bt.h) as a compiled C99 host sees them: sizes
 * and the offset of every field as one JSON line, under the names of the Python mirror (costs.py
 * COST_RECORDS), and the limits of the call. Built by tests/test_costs_cpu.py with -std=c99
 * -pedantic -Werror; needs no library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "bt.h"

#define OFF(T, f) printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define SZ(T) printf("\"%s\": %zu, ", #T, sizeof(T))

int main(void) {
    printf("{");
    SZ(bt_cost_rec); OFF(bt_cost_rec, n_trades); OFF(bt_cost_rec, n_win); OFF(bt_cost_rec, n_loss);
    OFF(bt_cost_rec, n_bars); OFF(bt_cost_rec, mdd_bar); OFF(bt_cost_rec, underwater_bars); OFF(bt_cost_rec, pnl);
    OFF(bt_cost_rec, fees); OFF(bt_cost_rec, turnover); OFF(bt_cost_rec, mdd); OFF(bt_cost_rec, win_sum);
    OFF(bt_cost_rec, loss_sum); OFF(bt_cost_rec, s2_lo); OFF(bt_cost_rec, s2_hi);
    SZ(bt_cost_agg); OFF(bt_cost_agg, n_sym); OFF(bt_cost_agg, n_traded); OFF(bt_cost_agg, n_profit);
    OFF(bt_cost_agg, pad); OFF(bt_cost_agg, trades); OFF(bt_cost_agg, pnl); OFF(bt_cost_agg, fees);
    OFF(bt_cost_agg, mdd_max);
    printf("\"costs_max\": %d, \"levels_max\": %d, \"fixed_max\": %d, \"bps_max\": %d, ", BT_COSTS_MAX,
           BT_COST_LEVELS_MAX, BT_COST_FIXED_MAX, BT_COST_BPS_MAX);
    printf("\"abi_version\": %d}\n", BT_ABI_VERSION);
    return 0;
}
