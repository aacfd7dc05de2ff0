"""Inputs at the limits the kernels' exactness arguments assume (tests only), shared by
tests/test_gpu_exact_limits.py (the sweep kernels) and tests/test_gpu_walk_limits.py (the lane
kernels on walk_tile.h). Every series is valid by docs/oracle_spec.md (1 <= c < 2^31,
|c_t - c_(t-1)| <= c_(t-1)), seeded and built here; each case carries the C oracle's rows.

A. |ret| = 1 on almost every bar (doubling cycles 1, 2, ..., 2^30 with a crash back to 1).
B. Bollinger z tests that are exactly tied, D^2 k_den^2 = k_num^2 Q with D != 0, or one tick from
   tied, at operands up to 2^112.
C. One symbol of kMaxBars = 2^22 bars at prices within 2^21 of 2^31.
D. The longest windows bt_engine_create accepts (docs/oracle_spec.md §7), at ceiling prices.

The cases are built once per process and must not be modified by a test."""
import functools

import numpy as np

import dbx_amd as D
from helpers import oracle_row

PMAX = 2**31 - 1


def _i32(*cols):
    return tuple(np.ascontiguousarray(x, np.int32) for x in cols)


def _assert_valid(series):
    for c, h, lo in series:
        for x in (c, h, lo):
            x = x.astype(np.int64)
            assert x.min() >= 1 and x.max() < 2**31
        c = c.astype(np.int64)
        assert (np.abs(np.diff(c)) <= c[:-1]).all()


def _oracle(strategy, grid, series, cap):
    return [oracle_row(strategy, grid, (c, h, lo, c), grid.annualization, cap) for c, h, lo in series]


# ----------------------------------------------------------------------------------------- A
CAP_A = 2048
CYC31 = [1 << i for i in range(31)]          # 1, 2, ..., 2^30, then the crash back to 1
CYC32 = CYC31 + [PMAX]                       # ..., 2^30, 2^31 - 1, crash
SHIFTS = (0, 1, 33, 63)


def _cycle(cyc, n, shift):
    return np.asarray(cyc, np.int64)[(np.arange(n) - shift) % len(cyc)]


def _wicks(c):
    return np.minimum(c + c // 8, PMAX), np.maximum(c - c // 8, 1)


@functools.lru_cache(None)
def _a_closes(long_series=False):
    if long_series:  # the 1,560-bar window's series
        return (_cycle(CYC31, 4500, 0), _cycle(CYC32, 4500, 63), np.tile([10_000, 20_000], 2250))
    lens = (64 * 16 + 1, 128 * 8, 1000, 1100)
    out = [_cycle(CYC31, n, s) for n, s in zip(lens, SHIFTS)]
    out += [_cycle(CYC32, n, s) for n, s in zip(lens, SHIFTS)]
    out.append(np.tile([10_000, 20_000], 501)[:1001])
    return tuple(out)


A_CASES = {
    # name: (oracle strategy, grid, long series)
    "sma": ("sma", lambda: D.Grid.sma([1, 2, 3], [2, 7, 40]), False),
    "ema_ols": ("ema_ols", lambda: D.Grid.ema_ols([3, 10], [4, 16]), False),
    "ema_ols_128": ("ema_ols", lambda: D.Grid.ema_ols([3, 10, 40], [4, 16, 1560]), True),
    "boll": ("boll", lambda: D.Grid.boll([2, 5, 20], [1, 3], [50, 9999], [50, 9999], k_den=2), False),
}


@functools.lru_cache(None)
def _a_case(name):
    strategy, mk, long_series = A_CASES[name]
    grid = mk()
    if strategy == "boll":  # wicks of an eighth of the close, and bars with h = l = c
        series = [_i32(c, *_wicks(c)) for c in _a_closes()] + [_i32(c, c, c) for c in _a_closes()]
    else:
        series = [_i32(c, c, c) for c in _a_closes(long_series)]
    return strategy, grid, series, _oracle(strategy, grid, series, CAP_A)


# ----------------------------------------------------------------------------------------- B
CAP_B = 1024
M = 2**31 - 4
REPS = 96          # a third each: untouched (exact ties), one tick up, one tick down


def _extremal(w, d, reps=REPS):
    """[m] * (w + 2) + [m + d]: the outlier's window holds w - 1 equal closes and itself, so
    z^2 = w - 1 exactly whatever d is, the largest z^2 a window of w bars can have. A third of the
    repetitions move one in-window bar a tick up, a third a tick down: both fall below the tie."""
    out = np.full((reps, w + 3), M, np.int64)
    out[:, w + 2] += d
    out[1::3, w // 2 + 2] += 1
    out[2::3, w // 2 + 2] -= 1
    return out.reshape(-1)


PAT6 = np.array([0, 0, 1, 1, 1, 3])          # mean 1, variance 1: the last bar has z = 2 at w = 6
S6 = 2**16


def _nonextremal(sign, reps=REPS):
    """m - s (0,0,1,1,1,3) repeated (z = -2 at every sixth bar, not the largest z of the window)
    and its mirror m' + s (...) (z = +2); one-tick moves of the second bar land on either side."""
    base = M if sign < 0 else M - 3 * S6
    out = np.tile(base + sign * S6 * PAT6, (reps, 1))
    out[1::3, 1] += 1
    out[2::3, 1] -= 1
    return out.reshape(-1)


def _hl(c):
    return _i32(c, np.minimum(c + 1000, PMAX), c - 1000)


# name: (window, tied k, k_den, series)
B_TIES = {
    "w5": (5, 2, 2**19, lambda: [_extremal(5, -(M // 2)), _extremal(5, -2**18)]),
    "w10": (10, 3, 2**18, lambda: [_extremal(10, -(M // 2)), _extremal(10, -2**18)]),
    # w k_num = 3970 * 63 * 16644 = 4.163e9, the last tie of this family under 2^32; one tie per
    # 3,973 bars, so the 30 of each kind take 381,408 bars (6 ms of kernel, no more)
    "w3970": (3970, 63, 16644, lambda: [_extremal(3970, -(M // 2)), _extremal(3970, -2**18)]),
    "w6": (6, 2, 2**19, lambda: [_nonextremal(-1), _nonextremal(+1)]),
}


B_GRIDS = {
    # name: (tie, k_num offsets from the tied K k_den, sl, tp, k_den if not the tie's own).
    # k_num <= 2^20: at k_den = 2^19 the tied k_num = 2^20 is the axis' last value, so K + 1 runs
    # at k_den = 2^18
    "w5": ("w5", (-2, -1, 0), [9999], [9999], None),
    "w5_kd18": ("w5", (-1, 0, 1), [9999], [9999], 2**18),
    "w10": ("w10", (-1, 0, 1), [9999], [9999], None),
    "w3970": ("w3970", (-1, 0, 1), [9999], [9999], None),
    "w6": ("w6", (-2, -1, 0), [9999], [9999], None),
    "w6_kd18": ("w6", (-1, 0, 1), [9999], [9999], 2**18),
    "w5_stops": ("w5", (-2, -1, 0), [30, 9999], [30], None),
    # 12 thresholds: the tie and its neighbours are tested in the second pass of 8
    "w6_k12": ("w6", tuple(range(-11, 1)), [9999], [9999], None),
    "w10_k12": ("w10", tuple(range(-10, 2)), [9999], [9999], None),
}


@functools.lru_cache(None)
def _b_series(tie):
    return [_hl(c) for c in B_TIES[tie][3]()]


@functools.lru_cache(None)
def _b_case(name):
    tie, offs, sl, tp, kd = B_GRIDS[name]
    w, K, kd0, _ = B_TIES[tie]
    kd = kd or kd0
    grid = D.Grid.boll([w], [K * kd + j for j in offs], sl, tp, k_den=kd)
    series = _b_series(tie)
    return grid, series, _oracle("boll", grid, series, CAP_B)


# ----------------------------------------------------------------------------------------- C
MAXB = 2**22


def _reflected_walk(rng, bars, lo, hi, step, start):
    """A random walk kept inside [lo, hi] by reflection at the ends (a clipped walk, vectorised)."""
    span = hi - lo
    x = np.mod(start - lo + np.cumsum(rng.integers(-step, step + 1, bars)), 2 * span)
    return lo + np.where(x > span, 2 * span - x, x)


C_GRIDS = {
    "sma": lambda: D.Grid.sma([5, 100], [50, 1000, 4096], annualization=98280),
    # 20 bps of these prices is twice the walk's whole range: band 0
    "ema_ols": lambda: D.Grid.ema_ols([10, 390], [15, 1560], band_bps=0),
    # 1 bp = 214,748 ticks, inside the range; 50 bps levels lie outside it (TP above 2^31)
    "boll": lambda: D.Grid.boll([10, 240], [3], [1, 50], [1, 9999], k_den=2),
}


@functools.lru_cache(None)
def _c_case(strategy):
    rng = np.random.default_rng(20261019 + len(strategy))
    c = _reflected_walk(rng, MAXB, 2**31 - 2**21, PMAX, 4000, 2**31 - 2**20)
    h = np.minimum(c + rng.integers(0, 3000, MAXB), PMAX)
    lo = c - rng.integers(0, 3000, MAXB)
    grid = C_GRIDS[strategy]()
    series = [_i32(c, h, lo)]
    return grid, series, _oracle(strategy, grid, series, 0)


# ----------------------------------------------------------------------------------------- D
CAP_D = 1 << 15
# the longest window bt_engine_create accepts per grid (docs/oracle_spec.md §7): the prefix
# ring of wmax plus the tiles in flight must fit a CU's 160 KB of LDS beside the grid's tables
D_LIMITS = {
    "sma": (16192, "SMA", lambda w: D.Grid.sma([5], [w])),
    "ema_ols": (8512, "EMA", lambda w: D.Grid.ema_ols([10], [w], band_bps=0)),
    "ema_ols_2x2": (8384, "EMA", lambda w: D.Grid.ema_ols([10, 4000], [16, w], band_bps=0)),
    "boll": (4608, "Bollinger", lambda w: D.Grid.boll([w], [2], [50], [100], k_den=2)),
}
D_GRIDS = {
    "sma": ("sma", lambda: D.Grid.sma([5, 600], [20, 16192], annualization=98280)),
    "ema_ols": ("ema_ols", lambda: D.Grid.ema_ols([10], [8512], band_bps=0)),
    "ema_ols_2x2": ("ema_ols", lambda: D.Grid.ema_ols([10, 4000], [16, 8384], band_bps=0)),
    "boll": ("boll", lambda: D.Grid.boll([20, 4608], [2, 3], [1], [2], k_den=2)),
}


@functools.lru_cache(None)
def _d_case(name):
    strategy, mk = D_GRIDS[name]
    grid = mk()
    wmax = D_LIMITS[name][0]
    bars = 3 * wmax + 77
    rng = np.random.default_rng(1900 + len(name))
    flat = 2**31 - 2**20 - 1 - rng.integers(0, 4, bars)              # 0-3 ticks of noise
    walk = _reflected_walk(rng, bars, 2_000_000_000 - 3_000_000, 2_000_000_000 + 3_000_000, 20_000,
                           2_000_000_000)
    series = [_i32(c, np.minimum(c + rng.integers(0, 3, bars) * (c.max() - c.min()) // 64, PMAX),
                   c - rng.integers(0, 3, bars) * (c.max() - c.min()) // 64) for c in (flat, walk)]
    return strategy, grid, series, _oracle(strategy, grid, series, CAP_D)


# ------------------------------------------------ the engines of C and D as the lane tests load them
def _hlc(series):
    """This module keeps (c, h, l); the references and the engine loaders take (h, l, c)."""
    return [(h, lo, c) for c, h, lo in series]


# C_GRIDS as they are, and the longest EMA+OLS window on the EMA series: U = sum k c_k passes 2^64
C_ENGINES = {**{k: (k, v) for k, v in C_GRIDS.items()}, "ema_ols_8512": ("ema_ols", D_GRIDS["ema_ols"][1])}


@functools.lru_cache(None)
def _c_rows(name):
    """(strategy, grid, (h, l, c), oracle summaries per param) of one engine of family C."""
    strategy, mk = C_ENGINES[name]
    grid, series, oracle = _c_case(strategy)
    hlc = _hlc(series)[0]
    if name in C_GRIDS:
        return strategy, grid, hlc, oracle[0][0]
    grid = mk()
    return strategy, grid, hlc, oracle_row(strategy, grid, (hlc[2], hlc[0], hlc[1], hlc[2]), grid.annualization)[0]


@functools.lru_cache(2)
def _c_lane(name, p):
    """(summary, complete trade list) of one lane: up to 460,745 trades, so only two are kept."""
    from replay_ref import oracle_lane
    strategy, grid, hlc, rows = _c_rows(name)
    return oracle_lane(strategy, grid, p, hlc, cap=int(rows[p]["n_trades"]))


D_SMA_WIDE = "sma_wide"
D_ENGINES = list(D_GRIDS) + [D_SMA_WIDE]


@functools.lru_cache(None)
def _d_rows(name):
    """(strategy, grid, series (c, h, l), oracle rows) of one engine of family D."""
    if name != D_SMA_WIDE:
        return _d_case(name)
    _, _, series, _ = _d_case("sma")
    grid = D.Grid.sma([8096, 12144], [16192], annualization=98280)
    return "sma", grid, series, _oracle("sma", grid, series, CAP_D)
