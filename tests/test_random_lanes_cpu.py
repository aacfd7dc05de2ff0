"""The random lane cases of random_cases.py, the parts that need no GPU: the host restatements
(bt_walk_forward_host, bt_portfolio_host, bt_covariance_host, bt_surface_host) against the cases'
references byte for byte, and the proof, from the references alone, that the default seeds reach the
shapes tests/test_gpu_random_lanes.py is there for: more folds than a wave has lanes with fold 64
empty on some rows only, 32 fold starts in one tile, stops and targets inside one bar, entry bars
that cross their own stop, exact SMA ties on the narrow paths; and that trade_stats and
reality_check, which that file puts among the drawn calls, take every place in the order."""
import numpy as np
import pytest

import dbx_amd as D
import gram_ref as G
import portfolio_ref as PR
import random_cases as RC
import walkfwd_ref as R
from helpers import build_plan_driver, run_driver
from surface_cases import assert_same

CASES = RC.CASES


@pytest.mark.parametrize("strategy,seed", CASES)
def test_a_case_is_a_pure_function_of_strategy_and_seed(strategy, seed):
    """Built again from nothing, the case is the same; and it has the shape the issue sets."""
    c = RC.lane_case(strategy, seed)
    d = RC.lane_case.__wrapped__(strategy, seed)
    assert c.grid.axes is not d.grid.axes and [list(a) for a in c.grid.axes] == [list(a) for a in d.grid.axes]
    assert c.entries.tobytes() == d.entries.tobytes() and c.bounds == d.bounds and c.order == d.order
    assert all(np.array_equal(x, y) for a, b in zip(c.series, d.series) for x, y in zip(a, b))
    assert (c.ids, c.cov_lanes, c.cov_window, c.replay_lanes) == (d.ids, d.cov_lanes, d.cov_window, d.replay_lanes)
    P, K = c.grid.n_params, len(c.bounds) - 1
    assert P <= 40 and len(c.series) == 6 and set(c.bars) <= set(RC.LENGTHS) and max(c.bars) >= 300
    assert len(set(c.ids)) == 6 and min(c.ids) >= 0 and max(c.ids) <= 2_000_000
    assert all(a < b for a, b in zip(c.bounds, c.bounds[1:])) and 0 <= c.bounds[0] < 70
    assert c.bounds[-1] == max(c.bars) + 300 and (K >= 65 or seed % 3)
    assert c.trains[:2] == (0, 1) and 2 <= c.trains[2] <= min(5, K - 1)
    assert len(c.entries) == 60 and len(np.unique(c.entries)) < 60
    n = len(c.cov_lanes)
    assert n in RC.COV_N and n <= 6 * P and len(set(c.cov_lanes)) == max(n - 1, 1)
    assert set(c.replay_lanes) == {(i, p) for i in c.ids for p in range(P)} and len(c.replay_lanes) > 6 * P
    assert sorted(c.order) == sorted(RC.STEPS)


@pytest.mark.parametrize("strategy,seed", CASES)
def test_host_restatements_equal_the_references(strategy, seed):
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    ann, where = c.grid.annualization, f"{strategy} seed {seed}"
    for train in c.trains:
        steps, total, _ = r.steps[train]
        got = D.walk_forward_host(r.folds, c.ids, train=train, annualization=ann)
        R.assert_same(got.steps, steps, f"{where}: steps, train {train}")
        R.assert_same(got.total, total, f"{where}: totals, train {train}")
    eq, ps, nb = PR.curve_arrays(r.pf_curves, max(c.bars))
    windows = np.stack([c.entries["from_bar"], c.entries["to_bar"]], 1)
    for T, want in r.portfolio.items():
        PR.assert_equal(D.portfolio_host(eq, ps, nb, windows=windows, T=T, annualization=ann), want,
                        f"{where}: portfolio, T {T}")
    eq, nb = G.curve_arrays(r.cov_curves, max(c.bars))
    G.assert_equal(D.covariance_host(eq, nb, c.cov_window), r.gram, f"{where}: covariance, window {c.cov_window}")
    host = D.surface_host(r.summaries, c.ids)
    assert_same(host.params, r.surface[0], f"{where}: surface params")
    assert_same(host.best, r.surface[1], f"{where}: surface best")


def test_the_walk_forward_budget_of_a_case_is_one_row_per_chunk_by_the_planner():
    """plan_walkfwd itself (csrc/plan.cpp through tests/plan/walkfwd_plan_driver.cpp) cuts every
    default case into one row per chunk under the case's budget, and has no row under a byte less."""
    exe = build_plan_driver("walkfwd_plan_driver")
    for st in RC.STRATEGIES:
        for seed in RC.DEFAULT_SEEDS:
            c = RC.lane_case(st, seed)
            P, K = c.grid.n_params, len(c.bounds) - 1
            pl = run_driver(exe, 6, P, K, max(c.bars), 256, c.wf_budget)
            assert (pl["rows_per_chunk"], pl["chunks"]) == (1, 6) and pl["staging_bytes"] == c.wf_budget, (st, seed, pl)
            assert run_driver(exe, 6, P, K, max(c.bars), 256, c.wf_budget - 1)["rows_per_chunk"] == 0, (st, seed)


# Totals over seeds 0..7 of each strategy, in the order of random_cases.COVERAGE. Conditions on the
# generator, not measurements of the code under test: every count comes from the C oracle's trade
# lists, the series and the bounds.
FLOORS = dict(k65_fold64_both=2, tile_32_starts=2, trades=100, picks=100, no_picks=50, traded=10, open_end=10,
              exit_last=10, entry_first=10, begins_inside=10, empty_windows=5)
ONLY = {"boll": dict(both_levels=20, entry_crosses_stop=20), "sma": dict(narrow_sma_ties=20)}
PINNED = {
    "sma": (5, 6, 2254, 3592, 6044, 1222, 9675, 158, 200, 96, 109, 0, 0, 56420),
    "ema_ols": (5, 4, 2010, 4496, 6514, 1060, 2884, 111, 149, 22, 99, 0, 0, 0),
    "boll": (3, 3, 28410, 3692, 5680, 8042, 14275, 3312, 3356, 31, 114, 17032, 18481, 0),
}


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_default_seeds_reach_the_shapes_they_are_there_for(strategy):
    total = dict.fromkeys(RC.COVERAGE, 0)
    for seed in RC.DEFAULT_SEEDS:
        for k, v in RC.coverage(strategy, seed).items():
            total[k] += int(v)
    for k, floor in {**FLOORS, **ONLY.get(strategy, {})}.items():
        assert total[k] >= floor, f"{strategy}: {k} = {total[k]}, floor {floor}"
    assert tuple(total[k] for k in RC.COVERAGE) == PINNED[strategy]


def test_default_seeds_use_every_knob_value_and_kind_of_window():
    cases = [RC.lane_case(st, s) for st in RC.STRATEGIES for s in RC.DEFAULT_SEEDS]
    assert len(cases) == 24
    for name, values in (("trade_cap", {1, 7, 64}), ("replicas", {0, 1, 3}), ("gram_split", {0, 1, 3}),
                         ("surface_chunks", {0, 1, 2, 5}), ("topk", {1, 10, 100})):
        assert {getattr(c, name) for c in cases} == values, name
    assert len({c.order for c in cases}) >= 12
    windows = [c.cov_window for c in cases]
    assert None in windows and any(w and w[0] == w[1] for w in windows) and any(w and w[0] < w[1] for w in windows)
    assert {len(c.cov_lanes) for c in cases} >= {1, 15, 16, 17, 33, 65}
    grams = [RC.lane_refs(c.strategy, c.seed).gram for c in cases]
    assert sum(T > 0 and any(int(x) for x in g.reshape(-1)) for g, _, T in grams) >= 12


def test_the_later_steps_take_every_place_among_the_drawn_ones():
    """test_gpu_random_lanes puts trade_stats and reality_check into a case's drawn order at places
    of their own drawing (random_cases.order_with_later_steps): over the default seeds each of them runs first, last, directly after
    every other kind of call, and the two come in both orders. The reference of the sub-case the
    reality-check step compares on every seed exists for the seeds past bootstrap_ref.WALK_SEEDS too,
    and the host code agrees with it."""
    import bootstrap_ref as BR
    after = {s: set() for s in RC.LATER_STEPS}
    first, last, both = set(), set(), set()
    for strategy, seed in RC.CASES:
        c = RC.lane_case(strategy, seed)
        order = RC.order_with_later_steps(c)
        assert order == RC.order_with_later_steps(RC.lane_case.__wrapped__(strategy, seed)), "a function of strategy and seed"
        assert tuple(s for s in order if s in RC.STEPS) == c.order and sorted(order) == sorted(RC.STEPS + RC.LATER_STEPS)
        first.add(order[0]), last.add(order[-1])
        both.add(order.index("trade_stats") < order.index("reality_check"))
        for s in RC.LATER_STEPS:
            if order.index(s):
                after[s].add(order[order.index(s) - 1])
    if not RC.NS:   # the default seeds
        assert set(RC.LATER_STEPS) <= first and set(RC.LATER_STEPS) <= last and both == {True, False}
        assert all(len(v) >= 6 for v in after.values()), after     # each of the six other kinds of call
    for strategy, seed in RC.CASES:
        if seed in BR.WALK_SEEDS:       # tests/test_bootstrap_cpu.py holds these
            continue
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        sub = BR.walk_case(strategy, seed)["inner"]
        eq = np.zeros((len(sub.lanes), max(c.bars)), np.int64)
        for i, (s, p) in enumerate(sub.lanes):
            eq[i, :c.bars[s]] = r.curves[s][p][1]
        got = D.reality_check_host(eq, [c.bars[s] for s, _ in sub.lanes], groups=sub.sizes, resamples=sub.B, block=sub.L,
                                   seed=sub.seed, window=sub.window, per_lane=True, vmax=True, boot=True)
        BR.assert_same(got, BR.walk_ref(strategy, seed, "inner"), f"{strategy} seed {seed} inner")
