"""Randomised differential suite for the analysis calls on top of a run: replay, walk_forward,
portfolio, covariance, trade_stats, reality_check, surface and read_topk on the seeded cases of
random_cases.py (random grids, ragged rows of the walk / narrow / plateau / spiky paths, shuffled
symbol ids, 15 to 115 folds with runs of one-bar folds, random portfolio and covariance windows),
every output byte for byte against
the references of random_cases.lane_refs: the C oracle's lanes and, from their complete trade lists,
replay_ref, walkfwd_ref, portfolio_ref, gram_ref, surface_ref and topk_ref, and against
tradestats_ref.random_refs and bootstrap_ref.walk_ref (the two calls share the device arena with the
others; their places in the drawn order come from a generator of their own).
tests/test_random_lanes_cpu.py holds the host restatements to the same references and proves that
the default seeds reach the shapes the cases are there for.

Then the Gram kernels at the capacity of a covariance call: bt_gram_of on random matrices of up to
2,048 rows (128 tile rows, 8,256 triangle tiles) against numpy's exact product mod 2^64 and
Python-int rows, and bt_covariance of 2,048 lanes against bt_covariance_host."""
import operator

import numpy as np
import pytest

import bootstrap_ref as BR
import dbx_amd as D
import gram_ref as G
import portfolio_ref as PR
import random_cases as RC
import tradestats_ref as TS
import walkfwd_ref as R
from helpers import compare_summary
from surface_cases import assert_same
from topk_ref import as_tuples

pytestmark = pytest.mark.gpu

WHOLE = 2**31 - 1
TRADE_FIELDS = ("entry_bar", "exit_bar", "side", "entry_px", "exit_px")


def _load(e, c):
    closes, highs, lows = [s[2] for s in c.series], [s[0] for s in c.series], [s[1] for s in c.series]
    if c.strategy == "boll":
        e.load_ohlc(closes, highs, lows, sym_ids=c.ids)
    else:
        e.load_ohlc(closes, sym_ids=c.ids)


def _i128(rec, name):
    return (int(rec[name + "_hi"]) << 64) | int(rec[name + "_lo"])


# --------------------------------------------------------------------------------- the steps
def _run_against_oracle(e, c, r, where):
    got = e.summaries()
    for s in range(len(c.series)):
        for p in range(c.grid.n_params):
            compare_summary(got[s, p], r.lanes[s][p][0], f"{where} row {s} ({c.bars[s]} bars) {c.grid.param(p)}")
    assert got.tobytes() == r.summaries.tobytes(), f"{where}: summaries() differ from the oracle's records"
    top = e.read_topk()
    assert top.dtype == D.TOPK_DTYPE and as_tuples(top) == as_tuples(r.topk), f"{where}: read_topk, k = {c.topk}"
    surf = e.surface()
    assert_same(surf.params, r.surface[0], f"{where}: surface params, chunks {c.surface_chunks}")
    assert_same(surf.best, r.surface[1], f"{where}: surface best, chunks {c.surface_chunks}")


def _replay(e, c, r, where):
    rp = e.replay(c.replay_lanes, trade_cap=c.trade_cap, curves=True)
    summ = e.summaries()
    row = {i: s for s, i in enumerate(c.ids)}
    n, stride = len(c.replay_lanes), max(c.bars)
    assert rp.trades.shape == (n, c.trade_cap) and rp.equity.shape == rp.pos.shape == (n, stride), where
    for i, (sym, p) in enumerate(c.replay_lanes):
        s = row[sym]
        at = f"{where} replay lane {i}: row {s} ({c.bars[s]} bars) {c.grid.param(p)}"
        orc, tr = r.lanes[s][p]
        compare_summary(rp.summaries[i], orc, at)
        assert rp.summaries[i].tobytes() == summ[s, p].tobytes(), f"{at}: not the bytes of summaries()"
        assert int(rp.n_bars[i]) == c.bars[s], at
        k = min(len(tr), c.trade_cap)
        got = rp.trades[i]
        for f in TRADE_FIELDS:
            assert got[f][:k].tolist() == tr[f][:k].tolist(), f"{at}: {f} of the first {k} trades"
        assert not got["pad"].any() and not got[k:].view(np.uint8).any(), f"{at}: trade row not zero past the trades"
        pos, eq = r.curves[s][p]
        B = c.bars[s]
        bad = np.nonzero(rp.pos[i, :B] != pos)[0]
        assert not len(bad), f"{at}: pos differs first at bar {bad[0]} ({len(bad)} bars)"
        bad = np.nonzero(rp.equity[i, :B] != eq)[0]
        assert not len(bad), f"{at}: equity differs first at bar {bad[0]}: {rp.equity[i, bad[0]]} vs {eq[bad[0]]}"
        assert not rp.pos[i, B:].any() and not rp.equity[i, B:].any(), f"{at}: curve rows not zero past the bars"


def _walk_forward(e, c, r, where):
    got = {}
    for train in c.trains:
        wf = got[train] = e.walk_forward(c.bounds, train=train, folds=True)
        steps, total, _ = r.steps[train]
        R.assert_same(wf.folds, r.folds, f"{where}: folds, train {train}")
        R.assert_same(wf.steps, steps, f"{where}: steps, train {train}")
        R.assert_same(wf.total, total, f"{where}: totals, train {train}")
    e.set_walkfwd_budget(c.wf_budget)          # one row per chunk
    try:
        one = {train: e.walk_forward(c.bounds, train=train, folds=True) for train in (0, c.trains[2])}
    finally:
        e.set_walkfwd_budget(0)
    for train, wf in one.items():
        for name in ("folds", "steps", "total"):
            assert getattr(wf, name).tobytes() == getattr(got[train], name).tobytes(), \
                f"{where}: {name}, train {train}, one row per chunk"


def _portfolio(e, c, r, where):
    PR.assert_equal(e.portfolio(c.entries), r.portfolio[max(c.bars)], f"{where}: portfolio, replicas {c.replicas}")
    PR.assert_equal(e.portfolio(c.entries, n_bars=c.pf_bars), r.portfolio[c.pf_bars],
                    f"{where}: portfolio over {c.pf_bars} bars, replicas {c.replicas}")


def _covariance(e, c, r, where):
    cv = e.covariance(c.cov_lanes, c.cov_window)
    G.assert_equal(cv, r.gram, f"{where}: covariance of {len(c.cov_lanes)} lanes, window {c.cov_window}, "
                               f"split {c.gram_split}")
    book = e.portfolio(c.cov_lanes, windows=c.cov_window or (0, WHOLE))
    assert cv.book_s2() == _i128(book.summary, "s2"), f"{where}: book_s2 against the portfolio of the same lanes"
    assert int(cv.sums.sum()) == _i128(book.summary, "s1"), f"{where}: sums against the portfolio's s1"


def _trade_stats(e, c, r, where):
    recs, agg = TS.random_refs(c.strategy, c.seed)
    ts = e.trade_stats(params=True)
    TS.assert_same(ts.lanes, recs, f"{where}: trade_stats, all-lanes records")
    TS.assert_same(ts.params, agg, f"{where}: trade_stats, aggregate")
    row = {i: s for s, i in enumerate(c.ids)}
    want = np.array([recs[row[sym], p] for sym, p in c.replay_lanes], D.TSTATS_DTYPE)
    TS.assert_same(e.trade_stats(c.replay_lanes).lanes, want, f"{where}: trade_stats, list mode")


def _reality_check(e, c, r, where):
    subs = BR.walk_case(c.strategy, c.seed)
    for name in ("inner",) + (("per_symbol",) if c.seed in BR.WALK_SEEDS else ()):
        sub = subs[name]
        got = e.reality_check(BR.sym_lanes(c, sub), groups=sub.sizes, resamples=sub.B, block=sub.L, seed=sub.seed,
                              window=sub.window, per_lane=True, vmax=True, boot=True)
        BR.assert_same(got, BR.walk_ref(c.strategy, c.seed, name), f"{where}: reality_check {name}")


STEP = {"run": _run_against_oracle, "replay": _replay, "walk_forward": _walk_forward, "portfolio": _portfolio,
        "covariance": _covariance, "trade_stats": _trade_stats, "reality_check": _reality_check}


@pytest.mark.parametrize("strategy,seed", RC.CASES)
def test_random_lanes(strategy, seed):
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    where = f"{strategy} seed {seed}"
    # trade_stats and reality_check at places drawn by a generator of their own, seeded by
    # strategy and seed: lane_case draws what it always drew
    order = RC.order_with_later_steps(c)
    assert sorted(order) == sorted(STEP) and tuple(s for s in order if s in RC.STEPS) == c.order
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, c)
        e.run()
        e.set_surface_chunks(c.surface_chunks)
        e.set_portfolio_replicas(c.replicas)
        e.set_gram_split(c.gram_split)
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        wrong = []      # every step runs: a failure names each call that differs, not the first alone
        for step in order:
            try:
                STEP[step](e, c, r, where)
            except AssertionError as err:
                wrong.append(f"{step}: {err}")
        assert not wrong, f"{where}, calls in the order {', '.join(order)}:\n" + "\n".join(wrong)
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"


# ------------------------------------------------------------------ covariance at its capacity
@pytest.fixture(scope="module")
def bare():
    """An engine without a dataset: gram_of needs none."""
    with D.Engine(D.Grid.sma([2], [5])) as e:
        yield e


PMAX = 2**31 - 1
# the rows whose entries are checked as whole int128 values: the first tile rows' edges, the
# middle, and the last tile row with the one before it; 64 rows at n >= 2047, every row below that
WIDE_ROWS = (0, 1, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1007, 1008, 1022, 1023, 1024, 1025) + tuple(range(2000, 2048))


@pytest.mark.parametrize("n,T", ((15, 65), (16, 64), (17, 64), (17, 65), (2047, 65), (2048, 64), (2048, 65)))
def test_gram_of_random_matrices_up_to_the_lane_limit(bare, n, T):
    """Random d over the whole domain |d| < 2^31 (bt_gram_of refuses -2^31), the ends included.
    Every entry's low word against u @ u.T in uint64, which is exact mod 2^64; the whole int128 in
    Python ints on WIDE_ROWS; sums exactly; symmetry. At n = 2048 the triangle has 8,256 tiles."""
    rng = np.random.default_rng([0x64A4, n, T])
    d = rng.integers(-PMAX, PMAX + 1, (n, T))
    d[rng.integers(0, n, 8), rng.integers(0, T, 8)] = (PMAX, -PMAX) * 4
    d = d.astype(np.int32)
    assert n <= D.COV_MAX == 2048
    got = bare.gram_of(d)
    assert got.n_bars == T and got.wide.shape == (n, n) and got.wide.dtype == D.WIDE_DTYPE
    assert np.array_equal(got.sums, d.astype(np.int64).sum(1)), "sums"
    u = d.astype(np.int64).astype(np.uint64)          # two's complement: products wrap mod 2^64
    low = u @ u.T
    bad = np.argwhere(got.wide["lo"] != low)
    assert not len(bad), f"low word of gram[{bad[0][0]}][{bad[0][1]}] ({len(bad)} entries differ)"
    rows = d.tolist()
    checked = [i for i in (WIDE_ROWS if n >= 2047 else range(n)) if i < n]
    assert len(checked) >= min(n, 64)
    for i in checked:
        want = [sum(map(operator.mul, rows[i], rj)) for rj in rows]
        lo, hi = got.wide["lo"][i].tolist(), got.wide["hi"][i].tolist()
        for j in range(n):
            assert (hi[j] << 64) | lo[j] == want[j], f"gram[{i}][{j}] = {(hi[j] << 64) | lo[j]}, want {want[j]}"
    assert np.array_equal(got.wide, got.wide.T), "symmetric"


def test_covariance_of_2048_lanes():
    """The most lanes a call takes: 2,048 distinct lanes of the config-2 grid on 6 symbols, window
    (37, 290), against bt_covariance_host fed from the replay of the same lanes
    (tests/test_random_lanes_cpu.py and tests/test_gram_cpu.py hold the host call to gram_ref)."""
    grid = D.config2_grid()
    rng = np.random.default_rng(0xC0F)
    flat = rng.choice(6 * grid.n_params, D.COV_MAX, replace=False)
    lanes = [(700 + int(k) // grid.n_params, int(k) % grid.n_params) for k in flat]
    window = (37, 290)
    with D.Engine(grid) as e:
        e.load_synthetic(0xC0FE, 700, 6, 300, D.BT_DAILY)
        cv = e.covariance(lanes, window)
        rp = e.replay(lanes, curves=True)
    assert len(set(lanes)) == 2048 and rp.equity.shape == (2048, 300) and (rp.n_bars == 300).all()
    host = D.covariance_host(rp.equity, rp.n_bars, window)
    assert cv.n_bars == host.n_bars == 253 and cv.wide.shape == (2048, 2048)
    assert np.array_equal(cv.sums, host.sums), "sums"
    bad = np.argwhere((cv.wide["lo"] != host.wide["lo"]) | (cv.wide["hi"] != host.wide["hi"]))
    assert not len(bad), f"gram[{bad[0][0]}][{bad[0][1]}] differs ({len(bad)} entries)"
    # the reference itself: every lane moves inside the window, and most of the curves differ
    assert (host.sums != 0).all() and len({row.tobytes() for row in host.wide["lo"]}) >= 1024
