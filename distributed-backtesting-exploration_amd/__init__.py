"""MI355X-native backtest engine for the worker job path of
brendisurfs/Distributed-Backtesting-Exploration.

The reference worker's job function `process_incoming_job`
(/root/reference/src/worker/process.rs:13-29) sleeps 1 s per job. Here it is a batch call into
libbt.so (include/bt.h): CSV bytes -> HBM-resident columns -> hand-written HIP kernels
(gfx950) -> one CompleteRequest.data string per job. See DESIGN.md.

Import as `dbx_amd` (the directory name has hyphens; /root/repo/dbx_amd.py is the shim).
"""
from .engine import (ABI_VERSION, FOLD_DTYPE, PIPE_SLOTS, WALKFWD_FOLDS_MAX, WF_STEP_DTYPE, WalkForward, walk_forward_host, BT_BOLL, BT_DAILY, BT_EMA_OLS, BT_FLAG_PARITY, BT_FLAG_TIMING, BT_MINUTE,
                     BT_SMA_CROSS, LANE_DTYPE, PARAM_AGG_DTYPE, REPLAY_MAX, SUMMARY_DTYPE, SURFACE_OF_MAX,
                     TOPK_DTYPE, TOPK_OF_MAX, TRADE_DTYPE, BtError, Engine, Grid, Replay, Surface, as_lanes, build,
                     config2_grid, config3_grid, config4_grid, config5_grid, lib, merge_surfaces,
                     merge_topk, surface_host, PF_LANE_DTYPE, PF_SUMMARY_DTYPE, PORTFOLIO_MAX, Portfolio, as_pf_lanes,
                     merge_portfolios, portfolio_host, walk_forward_lanes, COV_MAX, WIDE_DTYPE, Covariance,
                     covariance_host, TSTATS_AGG_DTYPE, TSTATS_DTYPE, TSTATS_MAX, TradeStats, merge_trade_stats,
                     trade_stats_agg_host, trade_stats_host, BOOT_GROUP_DTYPE, BOOT_LANE_DTYPE, BOOT_MAX,
                     BOOT_MAX_RESAMPLES, RealityCheck, reality_check_host, CSCV_MAX_FOLDS, CSCV_PICKS_MAX)
from .overfit import CSCV_GROUP_DTYPE, CSCV_PICK_DTYPE, CSCV_RECORDS, Overfit, cscv_combos, cscv_host
from .costs import (COST_AGG_DTYPE, COST_BPS_MAX, COST_DTYPE, COST_FIXED_MAX, COST_LEVELS_MAX, COST_RECORDS, COSTS_MAX,
                    Costs, costs_agg_host, costs_host, merge_costs)
from .tail import (TAIL_ALL, TAIL_BARS_MAX, TAIL_DTYPE, TAIL_HELD, TAIL_LEVELS_MAX, TAIL_MAX, TAIL_PPM_MAX, TAIL_Q_DTYPE,
                   TAIL_RECORDS, TailRisk, tail_risk_host)
from .ddrisk import DD_LANE_DTYPE, DD_LEVELS_MAX, DD_LIMITS_MAX, DD_RECORDS, DrawdownRisk, drawdown_risk_host

__all__ = [
    "ABI_VERSION", "FOLD_DTYPE", "PIPE_SLOTS", "WALKFWD_FOLDS_MAX", "WF_STEP_DTYPE", "WalkForward", "walk_forward_host", "BT_BOLL", "BT_DAILY", "BT_EMA_OLS", "BT_FLAG_PARITY", "BT_FLAG_TIMING", "BT_MINUTE",
    "BT_SMA_CROSS", "LANE_DTYPE", "PARAM_AGG_DTYPE", "REPLAY_MAX", "SUMMARY_DTYPE", "SURFACE_OF_MAX",
    "TOPK_DTYPE", "TOPK_OF_MAX", "TRADE_DTYPE", "BtError", "Engine", "Grid", "Replay", "Surface", "as_lanes", "build",
    "config2_grid", "config3_grid", "config4_grid", "config5_grid", "lib", "merge_surfaces",
    "merge_topk", "surface_host", "PF_LANE_DTYPE", "PF_SUMMARY_DTYPE", "PORTFOLIO_MAX", "Portfolio", "as_pf_lanes",
    "merge_portfolios", "portfolio_host", "walk_forward_lanes", "COV_MAX", "WIDE_DTYPE", "Covariance",
    "covariance_host", "TSTATS_AGG_DTYPE", "TSTATS_DTYPE", "TSTATS_MAX", "TradeStats", "merge_trade_stats",
    "trade_stats_agg_host", "trade_stats_host", "BOOT_GROUP_DTYPE", "BOOT_LANE_DTYPE", "BOOT_MAX",
    "BOOT_MAX_RESAMPLES", "RealityCheck", "reality_check_host", "CSCV_GROUP_DTYPE", "CSCV_MAX_FOLDS",
    "CSCV_PICK_DTYPE", "CSCV_PICKS_MAX", "CSCV_RECORDS", "Overfit", "cscv_combos", "cscv_host",
    "COST_AGG_DTYPE", "COST_BPS_MAX", "COST_DTYPE", "COST_FIXED_MAX", "COST_LEVELS_MAX", "COST_RECORDS", "COSTS_MAX",
    "Costs", "costs_agg_host", "costs_host", "merge_costs",
    "TAIL_ALL", "TAIL_BARS_MAX", "TAIL_DTYPE", "TAIL_HELD", "TAIL_LEVELS_MAX", "TAIL_MAX", "TAIL_PPM_MAX", "TAIL_Q_DTYPE",
    "TAIL_RECORDS", "TailRisk", "tail_risk_host",
    "DD_LANE_DTYPE", "DD_LEVELS_MAX", "DD_LIMITS_MAX", "DD_RECORDS", "DrawdownRisk", "drawdown_risk_host",
]
