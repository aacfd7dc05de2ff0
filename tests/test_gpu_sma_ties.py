"""The SMA kernel's compare stage and its equal-key pass (k_sma.hip stage 3), bit for bit against
the C oracle.

A lane compares its pair's two key rows over the tile; a tile in which some bar has equal floor
keys takes a second pass over the rows that collects the equality bits (eq_word), and the tied
bars are settled exactly. The cases put inputs where compare, equality pass and walk can go wrong:

* grids: one pair, one row, odd axes (3 x 5), config 2's 20 x 20 (a sparse seventh wave), at 63,
  65 and 200 bars (a partial tile, one bar into the second, several tiles), on a spec random walk
  and a two-price zig-zag;
* 40 x 40 (two y-blocks), 32 x 32 (the 16-wave block whose last wave also scans, the ONE_TRIP
  instantiation) and a run in three bar segments (the segment kernel shares the body);
* ties: a constant series (every key equal on every bar of every tile: no trades), a period-2
  series on which every floor key is equal while the exact means differ, so every decision bar
  goes through the exact settle, an odd grid on an ordinary series in the parity build (same
  trade lists as the oracle);
* warm-up bars max(fast, slow) - 1 in the middle of a 16-bar quarter of the tile, on its first and
  on its last bar, in the first tile and in the second: equality bits before the warm-up bar must
  not decide anything.

Every case compares all summary fields, in the parity instantiation the trade lists and the
128-bit sums as well.
"""
import functools

import numpy as np
import pytest

import dbx_amd as D
from helpers import launch_plan
from test_gpu_sma_trim import ANN, _floor_ties, _gpu_check, _no_trades_on_constant, _oracle, _walk, _zigzag

CAP = 704
BARS = (63, 65, 200)

# name: (fast, slow)
GRIDS = {
    "1x1": ([3], [11]),
    "1x3": ([4], [9, 20, 45]),
    "3x5": ([2, 5, 9], [12, 20, 31, 44, 60]),
    "20x20": (list(range(2, 22)), list(range(22, 62, 2))),
}


def _grid(fast, slow):
    return D.Grid.sma(list(fast), list(slow), annualization=ANN)


def _period2(bars):
    """1000, 1001, 1000, ...: every window's mean lies in [1000, 1001), so all floor keys are 1000,
    while an even window's mean is 1000.5 and an odd one's is not."""
    return np.ascontiguousarray(np.tile([1000, 1001], bars // 2 + 1)[:bars], np.int32)


def _const(bars):
    return np.full(bars, 4_321, np.int32)


@functools.lru_cache(None)
def _grid_case(name):
    grid = _grid(*GRIDS[name])
    series = [_walk(31 + i, n) for i, n in enumerate(BARS)] + [_zigzag(n) for n in BARS]
    return grid, series, _oracle(grid, series, CAP)


def test_grid_shapes():
    """The grids are what the cases are there for: one wave, and 6 1/4 waves in an 8-wave block."""
    for name, (fast, slow) in GRIDS.items():
        p = launch_plan(_grid(fast, slow))
        assert p["grid_y"] == 1 and p["block"] == (512 if name == "20x20" else 128), name
    # the walks and the zig-zag trade on the 200-bar series of every grid
    for name in GRIDS:
        _, _, oracle = _grid_case(name)
        assert max(int(o["n_trades"]) for o in oracle[2][0]) >= 1, name
        assert max(int(o["n_trades"]) for o in oracle[5][0]) >= 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids_gpu(name, mode):
    grid, series, oracle = _grid_case(name)
    _gpu_check(grid, series, oracle, mode, CAP, f"ties {name}")


# ------------------------------------------------------------- large grids, y-blocks, segments
@functools.lru_cache(None)
def _big_case(name):
    if name == "40x40":      # 1,600 pairs: two y-blocks of 13 parameter waves
        grid, bars = _grid(range(2, 42), range(42, 122, 2)), 300
    elif name == "32x32":    # 1,024 pairs: one 16-wave block, the last wave also scans
        grid, bars = _grid(range(2, 34), range(34, 98, 2)), 700
    else:                    # "seg": config 2's shape in three bar segments
        grid, bars = _grid(*GRIDS["20x20"]), 700
    series = [_walk(41, bars), _walk(42, bars - 37), _zigzag(bars), _const(bars)]
    return grid, series, _oracle(grid, series, CAP)


def test_big_grid_shapes():
    p40, p32 = launch_plan(_big_case("40x40")[0]), launch_plan(_big_case("32x32")[0])
    assert (p40["grid_y"], p40["block"], p40["dedicated"]) == (2, 14 * 64, 1)
    assert (p32["grid_y"], p32["block"], p32["dedicated"], p32["one_trip"]) == (1, 1024, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("40x40", "parity"), ("40x40", 1), ("32x32", "parity"), ("32x32", 1),
                                       ("seg", 3)])
def test_big_grids_gpu(name, mode):
    grid, series, oracle = _big_case(name)
    _gpu_check(grid, series, oracle, mode, CAP, f"ties {name}")


# ------------------------------------------------------------------------------------------ ties
@functools.lru_cache(None)
def _tie_case(name):
    grid = _grid(*GRIDS["3x5" if name == "odd" else "20x20"])
    if name == "const":
        series = [_const(n) for n in (63, 65, 200, 448)]
    elif name == "period2":
        series = [_period2(n) for n in (63, 65, 200, 449)]
    else:                    # the odd grid on ordinary series, for the parity build's trade lists
        series = [_walk(51 + i, n) for i, n in enumerate((63, 65, 200, 448))]
    return grid, series, _oracle(grid, series, CAP)


def test_tie_series_do_tie():
    _no_trades_on_constant(_tie_case("const")[2])
    grid, series, oracle = _tie_case("period2")
    c = series[3]
    # every decision bar of a pair of an even and an odd window is a floor tie with unequal means
    assert _floor_ties(c, 3, 22) == len(c) - 1 - 21
    assert _floor_ties(c, 2, 22) == 0           # two even windows: equal means, no decision
    assert max(int(o["n_trades"]) for o in oracle[3][0]) >= 1
    assert max(int(o["n_trades"]) for o in _tie_case("odd")[2][3][0]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("const", "parity"), ("const", 1), ("period2", "parity"), ("period2", 1),
                                       ("odd", "parity")])
def test_ties_gpu(name, mode):
    grid, series, oracle = _tie_case(name)
    _gpu_check(grid, series, oracle, mode, CAP, f"ties {name}")


# --------------------------------------------------------------------------------------- warm-up
WARM_FAST = [2, 3, 5, 8]
# warm-up bar max(fast, slow) - 1: 16 and 32 (first bar of a quarter), 31 and 47 (last), 39 (middle),
# and in the second tile 80 (first bar of its second quarter) and 89 (middle)
WARM_SLOW = [17, 32, 33, 40, 48, 81, 90]


@functools.lru_cache(None)
def _warm_case():
    grid = _grid(WARM_FAST, WARM_SLOW)
    series = [_walk(61, 200), _zigzag(200), _walk(62, 90), _zigzag(82)]
    return grid, series, _oracle(grid, series, CAP)


def test_warm_case_enters_at_the_warm_up_bar():
    grid, series, oracle = _warm_case()
    assert sorted({s - 1 for s in WARM_SLOW}) == [16, 31, 32, 39, 47, 80, 89]
    # on the zig-zag a pair of an odd and an even window decides at its first decision bar: the
    # first entry is at the warm-up bar itself
    orc, trades = oracle[1]
    for p in range(grid.n_params):
        kw = grid.param(p)
        if (kw["f"] + kw["s"]) % 2 == 1:
            assert int(orc[p]["n_trades"]) >= 1 and int(trades[p][0]["entry_bar"]) == kw["s"] - 1, kw


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1])
def test_warm_up_in_a_quarter_gpu(mode):
    grid, series, oracle = _warm_case()
    _gpu_check(grid, series, oracle, mode, CAP, "ties warm")
