"""The launch planner (csrc/plan.cpp) against a table of shards: what the library launches for a
grid and a dataset shape is a pure function of them and a CU count, so it is pinned here without
a GPU, through tests/plan/plan_driver.cpp (helpers.launch_plan).

EXPECTED was recorded at 256 CUs from the commit before the planner existed, not chosen by hand:
segment counts, burn-in, LDS bytes and the SMA block shape by a program linked against that
commit's libbt.so (its planning functions were exported and need no GPU), the tile kernels' block
shapes, wave maps and the segment buffer sizes by that commit's launcher and engine arithmetic
run unchanged in the same program. The GPU tests of test_gpu_segments.py tie the table to what
the engine launches (bt_last_segments equals the planner's G for the device's CU count)."""
import pytest

import dbx_amd as D
from helpers import assert_staging_layout, build_plan_driver, launch_plan, run_driver

EMA_960 = lambda: D.Grid.ema_ols(list(range(3, 3 + 2 * 29, 2)) + [3000], list(range(4, 4 + 5 * 32, 5)),
                                 band_bps=15)   # test_gpu_segments.test_ema_split_many_param_blocks
BOLL_1152 = lambda: D.Grid.boll([10, 20, 30, 45, 60, 90, 120, 240], [3, 4, 5, 6],
                                [25, 50, 75, 100, 150, 200], [50, 100, 150, 200, 300, 400], k_den=2)
FORCED = dict(seg=3, burn=1)

# name: (grid, symbols, bars of the longest, launch_plan keywords)
SHAPES = {
    "c2_5000": (D.config2_grid, 5000, 2520, {}),
    "c2_5000_forced": (D.config2_grid, 5000, 2520, FORCED),
    "c3_500": (D.config3_grid, 500, 98280, {}),
    "c3_250": (D.config3_grid, 250, 98280, {}),
    "c3_250_forced": (D.config3_grid, 250, 98280, FORCED),
    "c3_250_parity": (D.config3_grid, 250, 98280, dict(parity=True)),
    "c3_100": (D.config3_grid, 100, 98280, {}),
    "c4_500": (D.config4_grid, 500, 98280, {}),
    "c4_250": (D.config4_grid, 250, 98280, {}),
    "c4_250_forced": (D.config4_grid, 250, 98280, FORCED),
    "c4_250_parity": (D.config4_grid, 250, 98280, dict(parity=True)),
    "c4_64": (D.config4_grid, 64, 98280, {}),
    "c4_64_short": (D.config4_grid, 64, 20000, {}),   # the burn-in caps G below what the blocks allow
    "c5_1250": (D.config5_grid, 1250, 491400, {}),
    "c5_1250_parity": (D.config5_grid, 1250, 491400, dict(parity=True)),
    "c5_10000": (D.config5_grid, 10000, 491400, {}),
    "ema_960": (EMA_960, 3, 18000, {}),               # two y-blocks
    "boll_1152": (BOLL_1152, 100, 40000, {}),         # two y-blocks, hence no split walk
}

EXPECTED = {
    "c2_5000": {"n_params": 400, "wmax": 240, "ring": 512, "kmin_idx": 0, "G": 1, "burn_tiles": 2, "grid_y": 1, "block": 512, "lds": 42528, "dedicated": 1, "one_trip": 0, "ts": 0, "xw": 0, "lpw": 0, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c2_5000_forced": {"n_params": 400, "wmax": 240, "ring": 512, "kmin_idx": 0, "G": 3, "burn_tiles": 1, "grid_y": 1, "block": 512, "lds": 42528, "dedicated": 1, "one_trip": 0, "ts": 0, "xw": 0, "lpw": 0, "split_grp": -1, "wmap": 0, "seg_slots": 6093750, "pos_off": 768000000, "pos_bytes": 12000000, "ema_doubles": 0, "topk_lds_free": 0},
    "c3_500": {"n_params": 64, "wmax": 1560, "ring": 1856, "kmin_idx": 0, "ema_lds": [61120, 80208], "G": 1, "burn_tiles": 74, "grid_y": 1, "block": 512, "lds": 80208, "dedicated": 0, "one_trip": 0, "ts": 2, "xw": 5, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 1},
    "c3_250": {"n_params": 64, "wmax": 1560, "ring": 1856, "kmin_idx": 0, "ema_lds": [61120, 80208], "G": 2, "burn_tiles": 74, "grid_y": 1, "block": 512, "lds": 80208, "dedicated": 0, "one_trip": 0, "ts": 2, "xw": 5, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 32000, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 64000, "topk_lds_free": 1},
    "c3_250_forced": {"n_params": 64, "wmax": 1560, "ring": 1856, "kmin_idx": 0, "ema_lds": [61120, 80208], "G": 3, "burn_tiles": 1, "grid_y": 1, "block": 512, "lds": 80208, "dedicated": 0, "one_trip": 0, "ts": 2, "xw": 5, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 48000, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 96000, "topk_lds_free": 1},
    "c3_250_parity": {"n_params": 64, "wmax": 1560, "ring": 1856, "kmin_idx": 0, "ema_lds": [61120, 80208], "G": 1, "burn_tiles": 74, "grid_y": 1, "block": 512, "lds": 80208, "dedicated": 0, "one_trip": 0, "ts": 2, "xw": 5, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 1},
    "c3_100": {"n_params": 64, "wmax": 1560, "ring": 1856, "kmin_idx": 0, "ema_lds": [61120, 80208], "G": 4, "burn_tiles": 74, "grid_y": 1, "block": 512, "lds": 80208, "dedicated": 0, "one_trip": 0, "ts": 2, "xw": 5, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 25600, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 51200, "topk_lds_free": 1},
    "c4_500": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 1, "burn_tiles": 64, "grid_y": 1, "block": 512, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 2, "lpw": 64, "split_grp": 0, "wmap": 1165373968, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c4_250": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 2, "burn_tiles": 64, "grid_y": 1, "block": 512, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 2, "lpw": 64, "split_grp": 0, "wmap": 1165373968, "seg_slots": 128000, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c4_250_forced": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 3, "burn_tiles": 1, "grid_y": 1, "block": 512, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 2, "lpw": 64, "split_grp": 0, "wmap": 1165373968, "seg_slots": 192000, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c4_250_parity": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 1, "burn_tiles": 64, "grid_y": 1, "block": 640, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 4, "lpw": 64, "split_grp": 0, "wmap": 1985229328, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c4_64": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 4, "burn_tiles": 64, "grid_y": 1, "block": 640, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 4, "lpw": 64, "split_grp": 0, "wmap": 1985229328, "seg_slots": 65536, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c4_64_short": {"n_params": 256, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 2, "burn_tiles": 64, "grid_y": 1, "block": 640, "lds": 67168, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 4, "lpw": 64, "split_grp": 0, "wmap": 1985229328, "seg_slots": 32768, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c5_1250": {"n_params": 1024, "wmax": 6400, "ring": 8192, "kmin_idx": 0, "G": 6, "burn_tiles": 2, "grid_y": 1, "block": 1024, "lds": 117024, "dedicated": 0, "one_trip": 1, "ts": 0, "xw": 0, "lpw": 0, "split_grp": -1, "wmap": 0, "seg_slots": 7800000, "pos_off": 983040000, "pos_bytes": 15360000, "ema_doubles": 0, "topk_lds_free": 0},
    "c5_1250_parity": {"n_params": 1024, "wmax": 6400, "ring": 8192, "kmin_idx": 0, "G": 1, "burn_tiles": 2, "grid_y": 1, "block": 1024, "lds": 117024, "dedicated": 0, "one_trip": 1, "ts": 0, "xw": 0, "lpw": 0, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "c5_10000": {"n_params": 1024, "wmax": 6400, "ring": 8192, "kmin_idx": 0, "G": 1, "burn_tiles": 2, "grid_y": 1, "block": 1024, "lds": 117024, "dedicated": 0, "one_trip": 1, "ts": 0, "xw": 0, "lpw": 0, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "ema_960": {"n_params": 960, "wmax": 159, "ring": 448, "kmin_idx": 0, "ema_lds": [63744, 107888], "G": 1, "burn_tiles": 282, "grid_y": 2, "block": 1024, "lds": 63744, "dedicated": 0, "one_trip": 0, "ts": 1, "xw": 0, "lpw": 64, "split_grp": -1, "wmap": 0, "seg_slots": 0, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
    "boll_1152": {"n_params": 1152, "wmax": 240, "ring": 448, "kmin_idx": 0, "G": 2, "burn_tiles": 64, "grid_y": 2, "block": 1024, "lds": 78048, "dedicated": 0, "one_trip": 0, "ts": 0, "xw": 0, "lpw": 64, "split_grp": -1, "wmap": 1985229328, "seg_slots": 230400, "pos_off": 0, "pos_bytes": 0, "ema_doubles": 0, "topk_lds_free": 0},
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_matches_the_recorded_table(name):
    grid, n_sym, bars, kw = SHAPES[name]
    got = launch_plan(grid(), n_sym, bars, cus=256, **kw)
    assert got == EXPECTED[name], {k: (got[k], v) for k, v in EXPECTED[name].items() if got.get(k) != v}


def test_the_table_holds_the_shapes_it_is_there_for():
    assert set(EXPECTED) == set(SHAPES)
    G = {n: e["G"] for n, e in EXPECTED.items()}
    # on record from the strong-scaling runs: the 8-GPU shards of configs 3, 4 and 5
    assert (G["c3_250"], G["c4_250"], G["c5_1250"]) == (2, 2, 6)
    assert G["c2_5000"] == 1 and G["c5_10000"] == 1
    assert all(G[n] == 3 and EXPECTED[n]["burn_tiles"] == 1 for n in SHAPES if n.endswith("_forced"))
    assert all(G[n] == 1 and EXPECTED[n]["seg_slots"] == 0 for n in SHAPES if n.endswith("_parity"))
    assert G["c4_64_short"] < G["c4_64"]
    assert EXPECTED["ema_960"]["grid_y"] == 2
    assert EXPECTED["boll_1152"]["grid_y"] == 2 and EXPECTED["boll_1152"]["split_grp"] == -1
    assert EXPECTED["c4_500"]["split_grp"] >= 0


def test_a_refused_grid_reports_the_engines_error():
    assert launch_plan(D.Grid.boll([8000], [2], [50], [50])) == {
        "error": "Bollinger grid needs more LDS than a CU has (windows too long)"}


# ---- the staging of bt_topk_of (plan_topk_of, through tests/plan/topk_plan_driver.cpp)
TOPK_SOURCES = ("plan.cpp", "topk_rules.cpp")


def _check_topk_layout(pl, S, P):
    """The uploads (keys, summaries, one descriptor per row) and a whole TopkWork of the call's
    own: disjoint, 256-byte aligned, inside staging_bytes."""
    n = S * P
    assert (pl["summary_bytes"], pl["sym_bytes"], pl["rec_bytes"], pl["cap"], pl["kmax"]) == (48, 16, 24, 2048, 1024)
    assert_staging_layout([(pl["o_key"], n * 8), (pl["o_sum"], n * 48), (pl["o_syms"], S * 16),
                           (pl["o_hist"], 4096 * 4), (pl["o_state"], 4 * 8), (pl["o_counts"], 2 * 4),
                           (pl["o_above"], 2048 * 8), (pl["o_cand"], 2048 * 8), (pl["o_out"], 1025 * 24)],
                          pl["staging_bytes"], f"{S} x {P}")
    assert pl["o_key"] == 0


@pytest.mark.parametrize("S,P", [(1, 1), (2049, 1), (1, 2049), (3, 683), (1 << 22, 1), (1, 1 << 22), (2048, 2048),
                                 (33, 70_001)])
def test_plan_topk_of_lays_out_disjoint_aligned_regions(S, P):
    exe = build_plan_driver("topk_plan_driver", TOPK_SOURCES)
    pl = run_driver(exe, "plan", S, P)
    assert pl == run_driver(exe, "plan", S, P), "the plan is a function of its arguments"
    _check_topk_layout(pl, S, P)


def test_plan_topk_of_under_asan_and_ubsan():
    exe = build_plan_driver("topk_plan_driver", TOPK_SOURCES, sanitize=True)
    for S, P in ((1, 1), (2049, 1), (1 << 22, 1)):
        pl = run_driver(exe, "plan", S, P, sanitized=True)
        _check_topk_layout(pl, S, P)
        assert pl == run_driver(build_plan_driver("topk_plan_driver", TOPK_SOURCES), "plan", S, P)
