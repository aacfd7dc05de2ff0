"""The SMA kernel's trimmed key tasks and skipped wave-tiles (k_sma.hip), against the C oracle.

Three things in the kernel rest on an argument rather than on arithmetic, and each group below
puts inputs where that argument is used:

* warm-up skip: a parameter wave runs no compare and no walk before the first tile in which one
  of its lanes has a decision bar (kfirst = min over the wave of max(fast, slow) - 1, >> 6).
* ring mirror: the prefix ring's first 64 entries are stored a second time past its end, so the
  key tasks read 64 consecutive entries from a scalar start without a wrap. The grids sit on
  both sides of the engine's ring sizing rule, ring = next_pow2(wmax + 3 * 64) (engine.cpp).
* sparse last parameter wave: pair counts that leave 1, 16, 32, 33 and 63 live lanes in a
  block's last wave, a 16-wave block whose last wave also scans, and a split grid whose last
  y-block ends in a 16-lane wave and a wave with no live lane.

Every group runs on a spec random walk, a constant series (every key ties: no trades) and a
two-price zig-zag (a flip on most bars); the sparse group adds a walk at prices near 1,000,
where floor keys tie while the exact means differ. Every case compares all summary fields with
the C oracle, in the parity instantiation also the trade lists and the 128-bit sums S1 and S2,
and in the release one with 1 segment and with more (the segment kernel shares the body).
"""
import functools

import numpy as np
import pytest

import dbx_amd as D
import orc_ffi as F
from helpers import compare_summary, compare_trades, launch_plan, oracle_row

SEED = 0x7121
ANN = 252


def _walk(sym, bars):
    return np.ascontiguousarray(F.gen(SEED, sym, bars, 0)[3], np.int32)


def _const(bars):
    return np.full(bars, 12_345, np.int32)


def _zigzag(bars):
    return np.ascontiguousarray(np.tile([10_000, 20_000], bars // 2 + 1)[:bars], np.int32)


def _low_walk(seed, bars):
    """A walk of one-tick steps reflected inside [1000, 1016]: the means of two windows differ by
    a fraction of a tick on most bars, so their floor keys are often equal."""
    rng = np.random.default_rng(seed)
    x = np.mod(8 + np.cumsum(rng.integers(-1, 2, bars)), 32)
    return np.ascontiguousarray(1000 + np.where(x > 16, 32 - x, x), np.int32)


def _oracle(grid, series, cap):
    return [oracle_row("sma", grid, (c, c, c, c), ANN, cap) for c in series]


def _gpu_check(grid, series, oracle, mode, cap, what):
    """One engine run of `series` against the rows of _oracle. mode: "parity" (trade lists and the
    128-bit sums as well) or n >= 1 (release library, n segments per symbol). Returns the
    summaries."""
    parity = mode == "parity"
    with D.Engine(grid, **(dict(parity=True, trade_cap=cap) if parity else {})) as e:
        if not parity:
            e.set_segments(mode)
        e.load_ohlc(series)
        e.run()
        if not parity:
            assert e.last_segments() == mode
        got = e.summaries()
        sums, tr = (e.sums(), e.trades()) if parity else (None, None)
    for s, (orc, otr) in enumerate(oracle):
        for p in range(grid.n_params):
            where = f"{what} mode {mode} series {s} ({len(series[s])} bars) {grid.param(p)}"
            if parity:
                for k in ("s1", "s2"):
                    g = F.i128(sums[s, p][k + "_lo"], sums[s, p][k + "_hi"])
                    o = F.i128(orc[p][k + "_lo"], orc[p][k + "_hi"])
                    assert g == o, f"{where}: {k} gpu={g} oracle={o}"
            compare_summary(got[s, p], orc[p], where)
            if parity:
                compare_trades(tr[s, p], otr[p], min(int(orc[p]["n_trades"]), cap), where)
    return got


def _no_trades_on_constant(oracle_rows):
    for orc, _ in oracle_rows:
        assert all(int(o["n_trades"]) == 0 and int(o["exposure"]) == 0 for o in orc)


# ------------------------------------------------------------------------------ warm-up skip
WARM_FAST = list(range(2, 18))
WARM_SLOW = [20, 70, 130, 200, 260, 330, 400, 460]
WARM_BARS = (40, 100, 259, 260, 261, 300, 461, 700)
WARM_KINDS = {
    "walk": lambda i, n: _walk(i, n),
    "const": lambda i, n: _const(n),
    "zigzag": lambda i, n: _zigzag(n),
}
CAP_WARM = 704


@functools.lru_cache(None)
def _warm_case(kind):
    grid = D.Grid.sma(WARM_FAST, WARM_SLOW, annualization=ANN)
    series = [WARM_KINDS[kind](i, n) for i, n in enumerate(WARM_BARS)]
    return grid, series, _oracle(grid, series, CAP_WARM)


def test_warm_grid_shape():
    """128 pairs in two waves, lanes fast-minor: the second wave holds slow 260..460, so its first
    decision bar is 259 and its tiles 0 to 3 are wholly before warm-up."""
    grid = D.Grid.sma(WARM_FAST, WARM_SLOW)
    nf = len(WARM_FAST)
    assert grid.n_params == 128
    second = [max(WARM_FAST[j % nf], WARM_SLOW[j // nf]) - 1 for j in range(64, 128)]
    first = [max(WARM_FAST[j % nf], WARM_SLOW[j // nf]) - 1 for j in range(64)]
    assert min(second) == 259 and min(second) >> 6 == 4 and min(first) >> 6 == 0
    _no_trades_on_constant(_warm_case("const")[2])
    # the other two series do trade, in both waves, once there are bars after warm-up
    for kind in ("walk", "zigzag"):
        orc = _warm_case(kind)[2][WARM_BARS.index(700)][0]
        n = np.array([int(o["n_trades"]) for o in orc]).reshape(nf, len(WARM_SLOW))
        assert (n[:, :4].max(axis=0) >= 1).all() and (n[:, 4:].max(axis=0) >= 1).all(), (kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1, 2])
@pytest.mark.parametrize("kind", list(WARM_KINDS))
def test_warm_up_skip_gpu(kind, mode):
    grid, series, oracle = _warm_case(kind)
    got = _gpu_check(grid, series, oracle, mode, CAP_WARM, f"warm {kind}")
    # at 100 bars the second wave (slow >= 260) never warms
    s100 = WARM_BARS.index(100)
    for p in range(grid.n_params):
        if grid.param(p)["s"] >= 260:
            assert int(got[s100, p]["n_trades"]) == 0 and int(got[s100, p]["exposure"]) == 0


# ------------------------------------------------------------------------------- ring mirror
def _planned_ring(wmax):
    """The SMA prefix ring of a grid whose longest window is wmax, from the library's planner
    (plan.cpp plan_grid through helpers.launch_plan)."""
    return launch_plan(_ring_grid(wmax))["ring"]


# the largest wmax of a 256-entry ring and of a 512-entry ring, and one more each
RING_WMAX = {"r256_w64": 64, "r512_w65": 65, "r512_w320": 320, "r1024_w321": 321}
CAP_RING = 3328


def _ring_grid(wmax):
    fast = [w for w in (3, 63, 64, 65) if w < wmax]
    return D.Grid.sma(fast, [wmax], annualization=ANN)


@functools.lru_cache(None)
def _ring_case(name):
    wmax = RING_WMAX[name]
    grid = _ring_grid(wmax)
    n = 3 * _planned_ring(wmax) + 77       # every ring position is overwritten at least 3 times
    series = [_walk(11, n), _const(n), _zigzag(n), _walk(12, n + 51)]   # n + 51: whole tiles
    return grid, series, _oracle(grid, series, CAP_RING)


def test_ring_grids_sit_on_the_sizing_rule():
    assert [_planned_ring(w) for w in (64, 65, 320, 321)] == [256, 512, 512, 1024]
    for name, wmax in RING_WMAX.items():
        grid, series, oracle = _ring_case(name)
        assert max(grid.axes[1]) == wmax and _planned_ring(wmax) == int(name[1:name.index("_")])
        windows = set(grid.axes[0]) | set(grid.axes[1])
        assert 3 in windows and {63, 64, 65} & windows and (wmax < 66 or {63, 64, 65} <= windows)
        assert all(3 * _planned_ring(wmax) <= len(c) <= 3500 for c in series)
        assert len(series[3]) % 64 == 0
        _no_trades_on_constant([oracle[1]])
        assert max(int(o["n_trades"]) for o in oracle[2][0]) <= CAP_RING
        assert min(int(o["n_trades"]) for o in oracle[0][0]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1, 3])
@pytest.mark.parametrize("name", list(RING_WMAX))
def test_ring_mirror_gpu(name, mode):
    grid, series, oracle = _ring_case(name)
    _gpu_check(grid, series, oracle, mode, CAP_RING, f"ring {name}")


# --------------------------------------------------------------------------------- sparse wave
# name: (fast, slow); live = lanes of the last parameter wave
SPARSE_GRIDS = {
    "p16": (range(2, 6), range(20, 60, 10)),                 # the only wave is the sparse one
    "live1": (range(2, 7), range(20, 46, 2)),                # P = 65
    "live16": (range(2, 10), range(20, 70, 5)),              # P = 80
    "live32": (range(2, 10), range(20, 80, 5)),              # P = 96
    "live33": ([5], range(10, 107)),                         # P = 97
    "live63": ([7], range(10, 137)),                         # P = 127
    "p976": (range(2, 18), range(18, 79)),                   # 16 waves, the last also scans
    "p1040": (range(2, 18), range(18, 83)),                  # two y-blocks of 9 parameter waves
}
SPARSE_LIVE = {"p16": 16, "live1": 1, "live16": 16, "live32": 32, "live33": 33, "live63": 63,
               "p976": 16, "p1040": 16}
SPARSE_BARS = (333, 448)
CAP_SPARSE = 448


def _sma_shape(grid):
    """Parameter waves per block and y-blocks per symbol, from the library's planner."""
    p = launch_plan(grid)
    return p["block"] // 64 - p["dedicated"], p["grid_y"]


def _sparse_pairs(fast, slow):
    """(fast, slow) of the lanes in the wave that holds the last pair (lanes are fast-minor)."""
    nf, P = len(fast), len(fast) * len(slow)
    return [(fast[j % nf], slow[j // nf]) for j in range((P - 1) // 64 * 64, P)]


def _floor_ties(c, f, s):
    """Decision bars where floor(SMA_f) == floor(SMA_s) while the exact means differ."""
    pre = np.concatenate([[0], np.cumsum(c.astype(np.int64))])
    t = np.arange(max(f, s) - 1, len(c) - 1)
    Fs, Ss = pre[t + 1] - pre[t + 1 - f], pre[t + 1] - pre[t + 1 - s]
    return int(((Fs // f == Ss // s) & (Fs * s != Ss * f)).sum())


@functools.lru_cache(None)
def _sparse_case(name):
    fast, slow = (list(x) for x in SPARSE_GRIDS[name])
    grid = D.Grid.sma(fast, slow, annualization=ANN)
    series = [_walk(21, SPARSE_BARS[0]), _walk(22, SPARSE_BARS[1]), _const(SPARSE_BARS[0]),
              _zigzag(SPARSE_BARS[1]), _low_walk(5, SPARSE_BARS[1])]
    return grid, series, _oracle(grid, series, CAP_SPARSE)


@pytest.mark.parametrize("name", list(SPARSE_GRIDS))
def test_sparse_grid_shapes(name):
    fast, slow = (list(x) for x in SPARSE_GRIDS[name])
    P = len(fast) * len(slow)
    pw, gy = _sma_shape(D.Grid.sma(fast, slow))
    pairs = _sparse_pairs(fast, slow)
    assert len(pairs) == SPARSE_LIVE[name] == (P - 1) % 64 + 1
    if name == "p16":
        assert (pw, gy) == (1, 1)
    if name == "p976":
        assert P == 976 and (pw, gy) == (16, 1)
    if name == "p1040":   # the last y-block: 7 full waves, a 16-lane wave, an empty wave
        assert P == 1040 and (pw, gy) == (9, 2) and P - 64 * pw == 7 * 64 + 16
    grid, series, oracle = _sparse_case(name)
    _no_trades_on_constant([oracle[2]])
    # the low-price walk has floor-key ties with unequal means on a pair of the sparse wave,
    # and that pair trades on it
    low = series[4]
    ties = {fs: _floor_ties(low, *fs) for fs in pairs}
    assert max(ties.values()) >= 10, ties
    f, s = max(ties, key=ties.get)
    p = fast.index(f) * len(slow) + slow.index(s)
    assert grid.param(p) == {"f": f, "s": s} and int(oracle[4][0][p]["n_trades"]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1, 2])
@pytest.mark.parametrize("name", list(SPARSE_GRIDS))
def test_sparse_wave_gpu(name, mode):
    grid, series, oracle = _sparse_case(name)
    _gpu_check(grid, series, oracle, mode, CAP_SPARSE, f"sparse {name}")
