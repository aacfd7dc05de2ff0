"""Reference for the replay tests (tests only): one lane of the C oracle, and the per-bar position
and equity curves of docs/oracle_spec.md §4 rebuilt in numpy from the oracle's trade list:

* pos_t is the side of the trade with entry_bar <= t < exit_bar (an SMA flip closes one trade and
  opens the next at the same bar: that bar belongs to the new trade);
* realized_t is the pnl of the trades with exit_bar <= t;
* E_t = realized_t + pos_t (c_t - entry_px).

test_replay_cpu.py pins this reconstruction to the oracle's own mdd, pnl and exposure."""
import numpy as np

import orc_ffi as F


def oracle_lane(strategy, grid, p, ohlc, cap=0):
    """(summary, trades) of the C oracle for param index p of `grid` on one symbol (h, l, c)."""
    h, lo, c = ohlc
    kw = grid.param(p)
    ann = grid.annualization
    if strategy == "sma":
        return F.sma(c, kw["f"], kw["s"], ann, cap)
    if strategy == "ema_ols":
        return F.ema_ols(c, kw["n"], kw["w"], kw["band_bps"], ann, cap)
    return F.boll(h, lo, c, kw["w"], kw["k_num"], kw["k_den"], kw["sl"], kw["tp"], ann, cap)


def curves_from_trades(c, trades):
    """(pos int8[B], equity int64[B]) from a complete trade list."""
    c = np.asarray(c, np.int64)
    B = len(c)
    pos = np.zeros(B, np.int8)
    entry = np.zeros(B, np.int64)
    realized = np.zeros(B, np.int64)
    for t in ([] if trades is None else trades):
        e, x, side = int(t["entry_bar"]), int(t["exit_bar"]), int(t["side"])
        pos[e:x] = side
        entry[e:x] = int(t["entry_px"])
        realized[x:] += side * (int(t["exit_px"]) - int(t["entry_px"]))
    return pos, realized + pos.astype(np.int64) * (c - entry)


def curves_from_trades_fast(c, trades):
    """curves_from_trades without a pass over the bars per trade, for series of millions of bars
    and hundreds of thousands of trades: a trade adds its side and entry price at entry_bar and
    takes them away at exit_bar, its pnl arrives at exit_bar, and prefix sums of those difference
    arrays are pos_t, the open trade's entry price and realized_t (the trades of a lane do not
    overlap; int64 throughout, as the loop). test_gpu_walk_limits.py pins it to the loop."""
    c = np.asarray(c, np.int64)
    B = len(c)
    if trades is None or len(trades) == 0:
        return np.zeros(B, np.int8), np.zeros(B, np.int64)
    e, x = trades["entry_bar"].astype(np.int64), trades["exit_bar"].astype(np.int64)
    side = trades["side"].astype(np.int64)
    epx, xpx = trades["entry_px"].astype(np.int64), trades["exit_px"].astype(np.int64)
    d = np.zeros((3, B + 1), np.int64)          # pos, entry price, realized
    np.add.at(d[0], e, side)
    np.add.at(d[0], x, -side)
    np.add.at(d[1], e, epx)
    np.add.at(d[1], x, -epx)
    np.add.at(d[2], x, side * (xpx - epx))
    pos, entry, realized = np.cumsum(d[:, :B], axis=1)
    return pos.astype(np.int8), realized + pos * (c - entry)


def gen_hlc(seed, sym, bars, freq=1):
    """Oracle-generated series of one symbol as (h, l, c)."""
    o, h, lo, c, v = F.gen(seed, sym, bars, freq)
    return h, lo, c
