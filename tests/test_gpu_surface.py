"""Reductions of a run on the GPU (bt_surface / bt_surface_of, k_surface.hip; Engine.surface):
the per-parameter aggregates and the per-symbol best of the summaries a run left in HBM, byte for
byte against the plain-Python restatement of surface_ref.py over Engine.summaries() (which the
other GPU tests pin to the oracle), under every chunking, on grids wider than a tile, on tied
inputs, on the adversarial matrices of surface_cases.py, after a batch, and across shards."""
import functools
import re

import numpy as np
import pytest

import dbx_amd as D
import oracle_np as N
from replay_ref import gen_hlc
from surface_cases import SHAPES, adversarial, adversarial_ref, assert_same
from surface_ref import surface_ref

pytestmark = pytest.mark.gpu

STRATEGIES = ("sma", "ema_ols", "boll")


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]"""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc([s[2] for s in series], sym_ids=ids)


def _check(e, ids, where, chunks=(0,)):
    """surface() of the engine's last run against the reference over its summaries, under each
    chunk count; returns the reference."""
    ref_p, ref_b = surface_ref(e.summaries(), ids)
    for n in chunks:
        e.set_surface_chunks(n)
        s = e.surface()
        assert_same(s.params, ref_p, f"{where}, chunks {n}: params")
        assert_same(s.best, ref_b, f"{where}, chunks {n}: best")
    e.set_surface_chunks(0)
    return ref_p, ref_b


# ------------------------------------------------------------------------------ product path
# the 12-parameter edge grids and ragged series of test_gpu_replay.py: bars 1 .. 1000, ids shuffled
EDGE_BARS = (1, 2, 3, 63, 64, 65, 128, 129, 1000)
EDGE_IDS = (907, 12, 500, 3, 77, 2_000_000, 41, 8, 650)
EDGE_GRIDS = {
    "sma": lambda: D.Grid.sma([3, 70, 1200], [5, 100, 300, 2000], annualization=98280),
    "ema_ols": lambda: D.Grid.ema_ols([5, 80, 1500], [4, 64, 200, 1100], band_bps=5),
    "boll": lambda: D.Grid.boll([5, 64, 150, 1200], [2, 3, 4], [30], [60], k_den=2),
}


@functools.lru_cache(None)
def _edge_series():
    return [gen_hlc(0xED6E, i, b, 1) for i, b in zip(EDGE_IDS, EDGE_BARS)]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_surface_of_a_run_equals_the_reference_under_every_chunking(strategy):
    grid = EDGE_GRIDS[strategy]()
    assert grid.n_params == 12
    S = len(EDGE_IDS)
    with D.Engine(grid) as e:
        _load(e, strategy, _edge_series(), EDGE_IDS)
        e.run()
        ref_p, ref_b = _check(e, EDGE_IDS, strategy, chunks=(0, 1, 2, 3, S, S + 5))
        only = e.surface(best=False)
        assert only.best is None
        assert_same(only.params, ref_p, f"{strategy}: params alone")
    assert ref_b["sym"].tolist() == list(EDGE_IDS)
    # the inputs exercise what the reduction distinguishes (checked against the oracle when chosen)
    assert ((ref_p["n_win"] > 0) & (ref_p["n_win"] < ref_p["n_sym"])).any()
    assert (ref_p["n_traded"] < ref_p["n_sym"]).any() and (ref_p["n_sym"] == S).all()
    assert (ref_p["sym_max"] != ref_p["sym_min"]).any()
    assert int(ref_p["trades"].sum()) > 100
    assert len(set(ref_b["param"].tolist())) > 1


# ------------------------------------------------------------------- rows wider than a tile
WIDE_GRIDS = {
    ("sma", 65): lambda: D.Grid.sma(range(2, 7), range(10, 75, 5)),
    ("sma", 130): lambda: D.Grid.sma(range(2, 12), range(12, 77, 5)),
    ("ema_ols", 65): lambda: D.Grid.ema_ols(range(3, 18, 3), range(5, 70, 5), band_bps=10, annualization=252),
    ("ema_ols", 130): lambda: D.Grid.ema_ols(range(3, 33, 3), range(5, 70, 5), band_bps=10, annualization=252),
    ("boll", 65): lambda: D.Grid.boll(range(5, 70, 5), [2, 3, 4, 5, 6], [40], [80], annualization=252),
    ("boll", 130): lambda: D.Grid.boll(range(5, 70, 5), [2, 3, 4, 5, 6], [40, 90], [80], annualization=252),
}
WIDE_SYMS = (1, 2, 63, 64, 65, 257)


@pytest.mark.parametrize("strategy,P", list(WIDE_GRIDS))
def test_rows_that_span_tiles_with_a_ragged_tail(strategy, P):
    grid = WIDE_GRIDS[strategy, P]()
    assert grid.n_params == P
    best_params = set()
    with D.Engine(grid) as e:
        for S in WIDE_SYMS:
            e.load_synthetic(0x5AFE, 4000, S, 220, D.BT_DAILY)
            e.run()
            chunks = (0, 1, 3, S) if S in (65, 257) else (0,)
            _, ref_b = _check(e, range(4000, 4000 + S), f"{strategy} P {P} S {S}", chunks)
            best_params |= set(ref_b["param"].tolist())
    # winners on both sides of a tile boundary, so the cross-tile fold decides something (P = 65
    # has one lane in its last tile, which need not hold any row's best)
    assert P < 130 or min(best_params) < 64 <= max(best_params), sorted(best_params)


# ------------------------------------------------------------------------- ties on the device
def test_equal_sharpes_go_to_the_lowest_id_and_the_lowest_param():
    grid = D.Grid.sma([3, 5, 8], [20, 31, 50, 80])
    one = gen_hlc(0x71E5, 1, 300, 0)
    flat = tuple(np.full(300, 1000, np.int32) for _ in range(3))
    ids = (50, 7, 300, 9, 120, 4)
    with D.Engine(grid) as e:
        _load(e, "sma", [one, one, flat, one, one, flat], ids)
        e.run()
        summ = e.summaries()
        ref_p, ref_b = _check(e, ids, "ties", chunks=(0, 1, 2, 6))
        s = e.surface()
    assert summ[0].tobytes() == summ[1].tobytes() == summ[3].tobytes() == summ[4].tobytes()
    assert not summ[2]["sharpe"].any() and not summ[5]["sharpe"].any()
    # the four copies (lowest id 7) tie among themselves, the two flat rows (lowest id 4) at 0.0
    for a in s.params:
        assert int(a["sym_max"]) == (7 if a["sharpe_max"] != 0.0 else 4)
        assert int(a["sym_min"]) == (7 if a["sharpe_min"] != 0.0 else 4)
    assert (s.params["sharpe_max"] != 0.0).any() and (s.params["sharpe_min"] != 0.0).any()
    assert s.best["param"][2] == 0 and s.best["param"][5] == 0 and s.best["sharpe"][2] == 0.0
    assert s.best["sym"].tolist() == list(ids)


# -------------------------------------------------------------- values no run can produce
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_surface_of_adversarial_matrices_equals_host_and_reference(shape):
    S, P = shape
    m, ids = adversarial(S, P)
    ref_p, ref_b = adversarial_ref(S, P)
    host = D.surface_host(m, ids)
    with D.Engine(D.Grid.sma([3], [20])) as e:      # the matrix need not match the engine's grid
        for n in (0, 1, 3, S):
            e.set_surface_chunks(n)
            s = e.surface_of(m, ids)
            for got, want, what in ((s.params, ref_p, "params vs reference"), (s.best, ref_b, "best vs reference"),
                                    (s.params, host.params, "params vs host"), (s.best, host.best, "best vs host")):
                assert_same(got, want, f"{shape}, chunks {n}: {what}")
        assert_same(e.surface_of(m, ids, best=False).params, ref_p, f"{shape}: params alone")
    assert len(s.best) == S and len(s.params) == P


# -------------------------------------------------------------------------------- after a batch
def test_surface_after_run_batch():
    grid = D.Grid.sma([4, 10, 20], [50, 120], annualization=252)
    jobs = []
    for s, n in ((0, 300), (1, 451), (2, 64), (3, 777)):
        o, h, lo, c, v = N.gen(0xBA7C, [s], n, 0)
        jobs.append((f"job-{s}", N.csv_bytes(o[0], h[0], lo[0], c[0], v[0], 0)))
    with D.Engine(grid) as e:
        res = e.run_batch(jobs)
        assert [st for st, _ in res] == [0] * len(jobs)
        e.n_symbols = e.stats()["n_symbols"]          # summaries() of a batch: one row per good job
        assert e.n_symbols == len(jobs)
        ref_p, _ = _check(e, range(len(jobs)), "batch", chunks=(0, 2))
    assert int(ref_p["trades"].sum()) > 0 and (ref_p["n_sym"] == len(jobs)).all()


# ---------------------------------------------------------------------------- nothing disturbed
def test_surface_disturbs_nothing_and_refusals_leave_the_engine_usable():
    grid = D.config2_grid()
    m, ids = adversarial(65, 12)

    def state(e):
        return (e.summaries().tobytes(), e.read_topk().tobytes(), e.stats(), e.last_segments(with_refixed=True),
                e.kernel_timing()[1])

    with D.Engine(grid, topk=16, timing=True) as e:
        with pytest.raises(D.BtError, match="bt_surface: no results"):
            e.surface()
        e.load_synthetic(0xD1CE, 1000, 40, 600, D.BT_DAILY)
        with pytest.raises(D.BtError, match="bt_surface: no results"):
            e.surface()
        e.run()
        before = state(e)
        s1 = e.surface()
        e.surface_of(m, ids)
        assert state(e) == before
        # refused calls: the message names the value, the next call works
        f = D.engine.sym("bt_surface")
        assert f(e._h, None, None) == -1
        assert "agg and best are both NULL" in D.lib().bt_last_error().decode()
        for S, P, named in ((-2, 12, r"S = -2 "), (65, 0, r"P = 0 "), (4096, 1025, r"S\*P = 4096\*1025 exceeds 2\^22")):
            big = np.zeros((1, 1), D.SUMMARY_DTYPE)
            g = D.engine.sym("bt_surface_of")
            agg = np.zeros(2048, D.PARAM_AGG_DTYPE)
            assert g(e._h, S, P, big.ctypes.data, ids.ctypes.data, agg.ctypes.data, None) == -1
            assert re.search("bt_surface_of: " + named, D.lib().bt_last_error().decode())
        with pytest.raises(D.BtError, match="chunks = -1 "):
            e.set_surface_chunks(-1)
        s2 = e.surface()
        assert_same(s2.params, s1.params, "after refusals: params")
        assert_same(s2.best, s1.best, "after refusals: best")
        assert state(e) == before
        ref_p, ref_b = surface_ref(e.summaries(), range(1000, 1040))
        assert_same(s1.params, ref_p, "config-2 grid: params")
        assert_same(s1.best, ref_b, "config-2 grid: best")
        e.run()
        again = state(e)
        assert again[0] == before[0] and again[1] == before[1] and again[4] == before[4] + 1
        # the per-symbol records feed replay unchanged
        rp = e.replay(s1.best[:8])
        for i in range(8):
            assert rp.summaries[i].tobytes() == e.summaries()[i, s1.best["param"][i]].tobytes()


# ------------------------------------------------------------------------------ shard merge
def test_merge_of_two_shards_equals_the_single_engine():
    grid = D.config4_grid()
    S, bars, cut = 30, 1500, 10

    def run(begin, n):
        with D.Engine(grid) as e:
            e.load_synthetic(0x5AAD, begin, n, bars, D.BT_MINUTE)
            e.run()
            return e.surface()

    whole = run(0, S)
    merged = D.merge_surfaces([run(0, cut), run(cut, S - cut)])
    assert_same(merged.params, whole.params, "two shards merged: params")
    assert_same(merged.best, whole.best, "two shards concatenated: best")
    assert (whole.params["n_sym"] == S).all() and whole.best["sym"].tolist() == list(range(S))
    assert int(whole.params["trades"].sum()) > 100
