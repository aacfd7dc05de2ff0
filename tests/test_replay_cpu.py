"""CPU side of the lane replay (bt_replay, Engine.replay): the numpy curve reconstruction the GPU
tests compare against is pinned to the C oracle's own fields, the entry point is declared and
bound, the Python surface exists, and every accepted form of `lanes` gives the same request."""
import os
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from replay_ref import curves_from_trades, gen_hlc, oracle_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = {
    "sma": D.Grid.sma([3, 10], [7, 40], annualization=98280),
    "ema_ols": D.Grid.ema_ols([5, 30], [4, 50], band_bps=5),
    "boll": D.Grid.boll([5, 40], [2, 3], [30], [60], k_den=2),
}


@pytest.mark.parametrize("strategy", list(GRIDS))
@pytest.mark.parametrize("bars", [1, 2, 3, 64, 65, 1000])
def test_curve_reconstruction_matches_the_oracle_fields(strategy, bars):
    grid = GRIDS[strategy]
    h, lo, c = gen_hlc(0xC0FFEE, 17 + bars, bars, 1)
    traded = 0
    for p in range(grid.n_params):
        s, tr = oracle_lane(strategy, grid, p, (h, lo, c), cap=4096)
        assert int(s["n_trades"]) <= 4096
        pos, eq = curves_from_trades(c, tr)
        peak = np.maximum.accumulate(np.maximum(eq, 0))
        assert int((peak - eq).max()) == int(s["mdd"])
        assert int(eq[-1]) == int(s["pnl"])
        assert int(np.count_nonzero(pos[:-1])) == int(s["exposure"])
        assert pos[-1] == 0
        traded += int(s["n_trades"])
    if bars == 1000:
        assert traded >= 10 * grid.n_params


def test_bt_replay_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "bt.h")).read()
    assert re.search(r"int32_t\s+bt_replay\s*\(\s*bt_engine\*", hdr)
    assert re.search(r"#define BT_REPLAY_MAX (\d+)", hdr).group(1) == str(D.REPLAY_MAX)
    assert re.search(r"typedef struct bt_lane \{\s*int32_t sym;[^}]*int32_t param;[^}]*\} bt_lane;", hdr)
    assert int(re.search(r"#define BT_ABI_VERSION (\d+)", hdr).group(1)) == 3
    assert E._LATE_SYMBOLS["bt_replay"][0] == 3
    f = E.sym("bt_replay")
    assert f is not None and len(f.argtypes) == 10
    # a null engine is refused, not dereferenced
    assert f(None, 0, None, 0, None, None, None, None, None, 0) == -1
    assert "null engine" in D.lib().bt_last_error().decode()


def test_python_surface():
    assert callable(D.Engine.replay)
    assert D.LANE_DTYPE.names == ("sym", "param") and D.LANE_DTYPE.itemsize == 8
    assert {"lanes", "summaries", "n_bars", "trades", "equity", "pos"} <= set(D.Replay.__dataclass_fields__)
    for name in ("Replay", "LANE_DTYPE", "REPLAY_MAX", "as_lanes"):
        assert name in D.__all__


def test_lane_forms_give_the_same_request():
    top = np.zeros(5, D.TOPK_DTYPE)
    top["sym"] = [907, 12, 500, 12, 2**31 - 1]
    top["param"] = [3, 0, 11, 0, 7]
    top["sharpe"] = [2.5, 1.0, 0.5, 0.25, -1.0]
    top["pnl"] = [10, 20, 30, 40, 50]
    want = D.as_lanes(top)
    assert want.dtype == D.LANE_DTYPE and want.flags["C_CONTIGUOUS"]
    assert want["sym"].tolist() == top["sym"].tolist() and want["param"].tolist() == top["param"].tolist()
    pairs = [(int(s), int(p)) for s, p in zip(top["sym"], top["param"])]
    for form in (np.array(pairs, np.int64), np.array(pairs, np.int32), pairs, [list(x) for x in pairs],
                 iter(pairs), want, top[["sym", "param"]]):
        got = D.as_lanes(form)
        assert got.dtype == D.LANE_DTYPE and got.tobytes() == want.tobytes()
    assert len(D.as_lanes([])) == 0 and D.as_lanes([]).dtype == D.LANE_DTYPE
    assert len(D.as_lanes(np.zeros((0, 2), np.int64))) == 0
    for bad in ([(1, 2, 3)], [1, 2], np.zeros((2, 2), np.float64), [(2**31, 0)]):
        with pytest.raises(ValueError):
            D.as_lanes(bad)
