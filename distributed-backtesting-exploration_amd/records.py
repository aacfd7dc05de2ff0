"""The records and constants of include/bt.h as the binding mirrors them: numpy dtypes, one per C
struct the library reads or writes through a caller's array, and the header's limits. Pure data.
RECORDS maps every C struct name to its dtype; tests/test_abi_cpu.py checks each one's size and
every field's offset against a compiled C host of the header."""
import numpy as np

ABI_VERSION = 3  # BT_ABI_VERSION this wrapper is written against (build() checks the built library)
PIPE_SLOTS = 4  # BT_PIPE_SLOTS: pinned read-back / exchange slots

BT_SMA_CROSS, BT_EMA_OLS, BT_BOLL = 1, 2, 3
BT_FLAG_PARITY, BT_FLAG_TIMING = 1, 2
BT_DAILY, BT_MINUTE = 0, 1

REPLAY_MAX = 4096  # BT_REPLAY_MAX: lanes per Engine.replay call
SURFACE_OF_MAX = 1 << 22  # records Engine.surface_of stages (bt_surface_of)
TOPK_OF_MAX = 1 << 22  # records Engine.topk_of stages (bt_topk_of)
WALKFWD_FOLDS_MAX = 1 << 22  # fold records Engine.walk_forward(folds=True) returns
PORTFOLIO_MAX = 1 << 20  # BT_PORTFOLIO_MAX: entries per Engine.portfolio call
PF_WHOLE = 2**31 - 1  # to_bar of an entry without a window: every bar of its symbol
COV_MAX = 2048  # BT_COV_MAX: lanes per Engine.covariance call
TSTATS_MAX = 1 << 20  # BT_TSTATS_MAX: lanes per Engine.trade_stats call in list mode
BOOT_MAX = 1 << 20  # BT_BOOT_MAX: lanes per call with a lane list, and of bootstrap_of
BOOT_MAX_RESAMPLES = 65536  # BT_BOOT_MAX_RESAMPLES
CSCV_MAX_FOLDS = 20  # BT_CSCV_MAX_FOLDS: folds of Engine.cscv (even, at least 2)
CSCV_PICKS_MAX = 1 << 22  # pick records Engine.cscv(picks=True) returns

SUMMARY_DTYPE = np.dtype([
    ("n_trades", "<i4"), ("status", "<i4"), ("pnl", "<i8"), ("mdd", "<i8"),
    ("exposure", "<i8"), ("sharpe", "<f8"), ("hash", "<u8"),
])
SUMS_DTYPE = np.dtype([("s1_lo", "<u8"), ("s1_hi", "<i8"), ("s2_lo", "<u8"), ("s2_hi", "<i8")])
TRADE_DTYPE = np.dtype([
    ("entry_bar", "<i4"), ("exit_bar", "<i4"), ("side", "<i4"), ("pad", "<i4"),
    ("entry_px", "<i8"), ("exit_px", "<i8"),
])
TOPK_DTYPE = np.dtype([("sharpe", "<f8"), ("sym", "<i4"), ("param", "<i4"), ("pnl", "<i8")])
LANE_DTYPE = np.dtype([("sym", "<i4"), ("param", "<i4")])
# one parameter's aggregate over every symbol (docs/surface_spec.md)
PARAM_AGG_DTYPE = np.dtype([
    ("n_sym", "<i4"), ("n_traded", "<i4"), ("n_win", "<i4"), ("n_pos", "<i4"),
    ("trades", "<i8"), ("pnl", "<i8"), ("exposure", "<i8"), ("mdd_max", "<i8"),
    ("sharpe_max", "<f8"), ("sharpe_min", "<f8"), ("sym_max", "<i4"), ("sym_min", "<i4"),
    ("ss1_lo", "<u8"), ("ss1_hi", "<i8"), ("ss2_lo", "<u8"), ("ss2_hi", "<i8"),
])
# one lane's result over one bar fold, and one walk-forward step of one symbol
# (docs/walkforward_spec.md)
FOLD_DTYPE = np.dtype([
    ("first_bar", "<i4"), ("n_bars", "<i4"), ("n_trades", "<i4"), ("status", "<i4"),
    ("pnl", "<i8"), ("mdd", "<i8"), ("exposure", "<i8"), ("sharpe", "<f8"),
    ("s1_lo", "<u8"), ("s1_hi", "<i8"), ("s2_lo", "<u8"), ("s2_hi", "<i8"),
])
WF_STEP_DTYPE = np.dtype([
    ("sym", "<i4"), ("fold", "<i4"), ("param", "<i4"), ("pad", "<i4"), ("train_sharpe", "<f8"),
    ("oos", FOLD_DTYPE),
])
# one entry of a portfolio and the summary of its bars (docs/portfolio_spec.md)
PF_LANE_DTYPE = np.dtype([("sym", "<i4"), ("param", "<i4"), ("from_bar", "<i4"), ("to_bar", "<i4")])
PF_SUMMARY_DTYPE = np.dtype([
    ("n_lanes", "<i4"), ("first_bar", "<i4"), ("n_bars", "<i4"), ("max_gross", "<i4"),
    ("pnl", "<i8"), ("mdd", "<i8"), ("exposure", "<i8"), ("sharpe", "<f8"),
    ("s1_lo", "<u8"), ("s1_hi", "<i8"), ("s2_lo", "<u8"), ("s2_hi", "<i8"),
])
# an int128 as lo/hi words (docs/covariance_spec.md)
WIDE_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<i8")])
# one lane's trade statistics and drawdown timing, and one parameter's reduced over every dataset
# row (docs/tradestats_spec.md)
TSTATS_DTYPE = np.dtype([
    ("n_trades", "<i4"), ("n_win", "<i4"), ("n_loss", "<i4"), ("status", "<i4"),
    ("n_long", "<i4"), ("n_long_win", "<i4"), ("max_win_streak", "<i4"), ("max_loss_streak", "<i4"),
    ("hold_sum", "<i4"), ("hold_win", "<i4"), ("hold_max", "<i4"), ("n_bars", "<i4"),
    ("gross_win", "<i8"), ("gross_loss", "<i8"), ("max_win", "<i8"), ("max_loss", "<i8"),
    ("sq_lo", "<u8"), ("sq_hi", "<i8"), ("mdd", "<i8"), ("mdd_bar", "<i4"), ("peak_bar", "<i4"),
    ("underwater_bars", "<i4"), ("max_underwater", "<i4"), ("hash", "<u8"),
])
TSTATS_AGG_DTYPE = np.dtype([
    ("n_sym", "<i4"), ("n_traded", "<i4"), ("max_win_streak", "<i4"), ("max_loss_streak", "<i4"),
    ("hold_max", "<i4"), ("max_underwater", "<i4"),
    ("n_trades", "<i8"), ("n_win", "<i8"), ("n_loss", "<i8"), ("n_long", "<i8"), ("n_long_win", "<i8"),
    ("hold_sum", "<i8"), ("hold_win", "<i8"), ("gross_win", "<i8"), ("gross_loss", "<i8"),
    ("max_win", "<i8"), ("max_loss", "<i8"), ("mdd_max", "<i8"), ("sq_lo", "<u8"), ("sq_hi", "<i8"),
])
# one lane's and one group's result of the bootstrap reality check (docs/bootstrap_spec.md); the
# header's m1 and m2 (bt_wide) lie flat here as lo/hi words
BOOT_LANE_DTYPE = np.dtype([("sum", "<i8"), ("n_nonpos", "<i8"), ("m1_lo", "<u8"), ("m1_hi", "<i8"),
                            ("m2_lo", "<u8"), ("m2_hi", "<i8")])
BOOT_GROUP_DTYPE = np.dtype([("best_sum", "<i8"), ("best_lane", "<i4"), ("n_lanes", "<i4"), ("n_ge", "<i8")])

RECORDS = {
    "bt_summary": SUMMARY_DTYPE, "bt_sums": SUMS_DTYPE, "bt_trade": TRADE_DTYPE, "bt_topk_rec": TOPK_DTYPE,
    "bt_lane": LANE_DTYPE, "bt_param_agg": PARAM_AGG_DTYPE, "bt_fold": FOLD_DTYPE, "bt_wf_step": WF_STEP_DTYPE,
    "bt_pf_lane": PF_LANE_DTYPE, "bt_pf_summary": PF_SUMMARY_DTYPE, "bt_wide": WIDE_DTYPE,
    "bt_tstats": TSTATS_DTYPE, "bt_tstats_agg": TSTATS_AGG_DTYPE, "bt_boot_lane": BOOT_LANE_DTYPE,
    "bt_boot_group": BOOT_GROUP_DTYPE,
}
# the sizes the header's comments and the static_asserts under csrc/ state, checked on import
assert [d.itemsize for d in RECORDS.values()] == [48, 32, 32, 24, 8, 104, 80, 104, 16, 80, 16, 128, 136, 48, 24]
