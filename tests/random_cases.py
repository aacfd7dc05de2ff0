"""Seeded random inputs shared by the randomised suites (tests only).

_series, _ohlc and _windows are the price paths and window lists of tests/test_gpu_random.py (the
sweep kernels). lane_case(strategy, seed) builds on them one case for the analysis calls on top of
a run: replay, walk_forward, portfolio, covariance, surface and read_topk. A case is a pure function
of (strategy, seed): every draw is made here, in a fixed order, whatever a test later checks.
lane_refs(strategy, seed) holds the references of a case: the C oracle's lanes with complete trade
lists, the curves rebuilt from them (replay_ref), fold records and steps (walkfwd_ref), the
portfolio tuples (portfolio_ref), the Gram tuple (gram_ref), the surface (surface_ref) and the
top-k (topk_ref). coverage(strategy, seed) counts, from those references alone, how often the case
reaches the shapes tests/test_random_lanes_cpu.py sets floors for.

Cases and references are built once per process and must not be modified by a test."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import dbx_amd as D
import gram_ref as G
import portfolio_ref as PR
import walkfwd_ref as R
from replay_ref import curves_from_trades, oracle_lane
from surface_ref import surface_ref
from topk_ref import topk

KINDS = ("walk", "narrow", "plateau", "spiky")
STRATEGIES = ("sma", "ema_ols", "boll")
WHOLE = 2**31 - 1


def _series(rng, n, kind):
    if kind == "walk":          # ordinary tick walk around $100
        x = 1_000_000 + np.cumsum(rng.integers(-4000, 4001, n))
    elif kind == "narrow":      # a few ticks wide: floor keys and exact SMAs collide often
        x = 10_000 + np.cumsum(rng.integers(-1, 2, n))
        x = np.clip(x, 10_000, 10_004)
    elif kind == "plateau":     # long flat stretches with rare jumps
        x = 20_000 + 50 * np.cumsum(rng.random(n) < 0.03)
    else:                       # "spiky": near the int32 price ceiling with large moves
        x = 2_000_000_000 + np.cumsum(rng.integers(-3_000_000, 3_000_001, n))
    return np.clip(x, 10_000, 2**31 - 1).astype(np.int32)


def _ohlc(rng, c):
    hi = c + rng.integers(0, 3000, len(c)).astype(np.int64)
    lo = c - rng.integers(0, 3000, len(c)).astype(np.int64)
    return np.clip(hi, 1, 2**31 - 1).astype(np.int32), np.clip(lo, 1, 2**31 - 1).astype(np.int32)


def _windows(rng, k, top):
    return sorted(set(int(x) for x in rng.integers(1, top, k)))


# ------------------------------------------------------------------------------ the lane cases
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 300, 777, 1500)
TILE_EDGES = (63, 64, 65, 127, 128, 129, 192)
COV_N = (1, 15, 16, 17, 31, 33, 48, 65)
STEPS = ("run", "replay", "walk_forward", "portfolio", "covariance")
# seeds per strategy (BT_RANDOM_SEEDS widens the sweep for a one-off deep run, BT_RANDOM_SEED0
# moves its first seed, as in test_gpu_random.py)
NS = int(os.environ.get("BT_RANDOM_SEEDS", "0"))
S0 = int(os.environ.get("BT_RANDOM_SEED0", "0"))
DEFAULT_SEEDS = range(8)
CASES = [(st, s) for st in STRATEGIES for s in (range(S0, S0 + NS) if NS else DEFAULT_SEEDS)]


def _grid(strategy, rng):
    if strategy == "sma":
        return D.Grid.sma(_windows(rng, 5, 80), _windows(rng, 4, 300), annualization=252)
    if strategy == "ema_ols":
        return D.Grid.ema_ols(_windows(rng, 4, 200), _windows(rng, 4, 400), band_bps=int(rng.integers(0, 60)))
    return D.Grid.boll(_windows(rng, 3, 120), sorted(set(int(x) for x in rng.integers(1, 7, 3))),
                       [int(x) for x in rng.integers(10, 300, 2)], [int(x) for x in rng.integers(10, 500, 2)], k_den=2)


def _bounds(rng, seed, longest):
    """Strictly increasing fold bounds: a start inside the first 70 bars, a run of one-bar folds
    (70 of them on every third seed: more folds than a wave has lanes, and a tile that holds 32 or
    more fold starts), random cuts up to 200 bars past the longest row, three bounds at tile edges
    and one 300 bars past every row."""
    b0 = int(rng.integers(0, 70))
    run = 70 if seed % 3 == 0 else int(rng.integers(2, 70))
    # a long run starts inside the first tile it can: fold 64 then lies below bar 200
    r0 = b0 + int(rng.integers(0, 64 if run == 70 else max(longest - b0, 1)))
    cuts = set(range(r0, r0 + run + 1))
    cuts |= set(int(x) for x in rng.integers(b0 + 1, longest + 201, int(rng.integers(3, 41))))
    cuts |= set(int(x) for x in rng.choice(TILE_EDGES, 3, replace=False))
    cuts.add(longest + 300)
    return (b0,) + tuple(sorted(x for x in cuts if x > b0))


@functools.lru_cache(None)
def lane_case(strategy, seed):
    """One random case for the analysis calls; see the module's docstring. Fields: grid, series
    [(h, l, c)], ids, bars, bounds, trains, entries (PF_LANE_DTYPE), pf_bars (a T below the longest
    row), cov_lanes [(sym id, param)], cov_window (or None), replay_lanes [(sym id, param)], and the
    knobs trade_cap, replicas, gram_split, surface_chunks, topk, wf_budget and order."""
    rng = np.random.default_rng([0x1A4E5, STRATEGIES.index(strategy), seed])
    grid = _grid(strategy, rng)
    P = grid.n_params
    assert P <= 40
    S = 6
    bars = [int(n) for n in rng.choice(LENGTHS, S)]
    if max(bars) < 300:   # one row that outlasts the tile-edge bounds
        bars[int(rng.integers(0, S))] = int(rng.choice((300, 777, 1500)))
    series = []
    for i, n in enumerate(bars):
        c = _series(rng, n, KINDS[i % 4])
        h, lo = _ohlc(rng, c)
        series.append((h, lo, c))
    ids = [int(x) for x in rng.choice(2_000_001, S, replace=False)]
    longest = max(bars)
    bounds = _bounds(rng, seed, longest)
    trains = (0, 1, min(int(rng.integers(2, 6)), len(bounds) - 2))   # train <= K - 1

    # portfolio entries: (row, param, from, to), a fifth over the whole series, a tenth empty
    ent = []
    for _ in range(56):
        s, p = int(rng.integers(0, S)), int(rng.integers(0, P))
        frm = int(rng.integers(0, bars[s] + 11))
        to = int(rng.integers(frm, bars[s] + 101))
        u = rng.random()
        if u < 0.2:
            frm, to = 0, WHOLE
        elif u < 0.3:
            to = frm
        ent.append((ids[s], p, frm, to))
    for i in rng.integers(0, len(ent), 4):   # a few entries twice
        ent.append(ent[int(i)])
    entries = np.zeros(len(ent), D.PF_LANE_DTYPE)
    for i, r in enumerate(ent):
        entries[i] = r
    pf_bars = int(rng.integers(1, longest))

    # covariance: distinct lanes, a window on the longest of them (a quarter None, a tenth empty,
    # some beginning past the shorter lanes' ends); a window above 800 bars keeps 48 lanes
    n = int(rng.choice(COV_N))
    n = max(v for v in COV_N if v <= max(min(n, S * P), 1))   # a small grid: the next count below
    flat = [int(x) for x in rng.choice(S * P, max(n - 1, 1), replace=False)]
    top = max(bars[k // P] for k in flat)
    u = rng.random()
    frm = int(rng.integers(0, top))
    to = int(rng.integers(frm + 1, top + 101))
    cov_window = None if u < 0.25 else (frm, frm) if u < 0.35 else (frm, to)
    span = top if cov_window is None else min(cov_window[1], top) - cov_window[0]
    if span > 800 and n > 48:
        n, flat = 48, flat[:47]
    if n >= 2:            # one lane twice
        flat.insert(int(rng.integers(0, n)), flat[int(rng.integers(0, n - 1))])
    cov_lanes = [(ids[k // P], k % P) for k in flat]

    # replay: every lane, shuffled, about a tenth of them again
    order = [int(x) for x in rng.permutation(S * P)]
    again = [order[int(i)] for i in rng.integers(0, S * P, max(S * P // 10, 1))]
    mixed = order + again
    mixed = [mixed[int(i)] for i in rng.permutation(len(mixed))]
    replay_lanes = [(ids[k // P], k % P) for k in mixed]

    K = len(bounds) - 1
    # one row of walk-forward staging (plan_walkfwd): the bounds rounded to 256 bytes, two
    # roundings of the regions, K * P fold records and K - 1 steps; a second row does not fit
    wf_budget = ((K + 1) * 4 + 255) // 256 * 256 + 512 + K * P * D.FOLD_DTYPE.itemsize \
        + (K - 1) * D.WF_STEP_DTYPE.itemsize
    case = SimpleNamespace(
        strategy=strategy, seed=seed, grid=grid, series=series, ids=ids, bars=bars, bounds=bounds, trains=trains,
        entries=entries, pf_bars=pf_bars, cov_lanes=cov_lanes, cov_window=cov_window, replay_lanes=replay_lanes,
        trade_cap=int(rng.choice((1, 7, 64))), replicas=int(rng.choice((0, 1, 3))),
        gram_split=int(rng.choice((0, 1, 3))), surface_chunks=int(rng.choice((0, 1, 2, 5))),
        topk=int(rng.choice((1, 10, 100))), wf_budget=wf_budget,
        order=tuple(STEPS[int(i)] for i in rng.permutation(len(STEPS))))
    entries.setflags(write=False)
    for ohlc in series:
        for x in ohlc:
            x.setflags(write=False)
    return case


LATER_STEPS = ("trade_stats", "reality_check")   # analysis calls that came after STEPS


def order_with_later_steps(c):
    """c.order with LATER_STEPS put in at places drawn by a generator of their own, seeded by the
    case's strategy and seed: lane_case itself draws what it always drew."""
    rng = np.random.default_rng([0x0DE1, STRATEGIES.index(c.strategy), c.seed])
    order = list(c.order)
    for step in LATER_STEPS:
        order.insert(int(rng.integers(0, len(order) + 1)), step)
    return tuple(order)


# ------------------------------------------------------------------------------- references
def summary_matrix(lanes):
    """The oracle's summaries as the S x P matrix Engine.summaries() returns (the engine's record
    is the oracle's first seven fields)."""
    out = np.zeros((len(lanes), len(lanes[0])), D.SUMMARY_DTYPE)
    for s, row in enumerate(lanes):
        for p, (summ, _) in enumerate(row):
            for f in D.SUMMARY_DTYPE.names:
                out[s, p][f] = summ[f]
    return out


@functools.lru_cache(None)
def lane_refs(strategy, seed):
    """The references of lane_case(strategy, seed). Fields: lanes[s][p] = (oracle summary, complete
    trade list), curves[s][p] = (pos int8[B], equity int64[B]), summaries (S x P SUMMARY_DTYPE),
    folds (S x P x K), steps {train: (steps, total, tied)}, pf_curves / pf_trades (per portfolio
    entry), portfolio {T: tuple} for the default T and case.pf_bars, cov_curves, gram (gram, sums,
    T), surface (params, best) and topk."""
    c = lane_case(strategy, seed)
    P, S = c.grid.n_params, len(c.series)
    ann = c.grid.annualization
    folds, lanes = R.ref_folds(strategy, c.grid, c.series, c.bounds)
    curves = [[curves_from_trades(c.series[s][2], lanes[s][p][1]) for p in range(P)] for s in range(S)]
    steps = {t: R.ref_steps(folds, c.ids, t, ann) for t in c.trains}
    row = {i: s for s, i in enumerate(c.ids)}
    lists = {}

    def as_lists(s, p):
        if (s, p) not in lists:
            tr = lanes[s][p][1]
            lists[s, p] = (curves[s][p][0].tolist(), curves[s][p][1].tolist(),
                           [(int(t["entry_bar"]), int(t["exit_bar"])) for t in tr])
        return lists[s, p]

    pf = [as_lists(row[int(e["sym"])], int(e["param"])) for e in c.entries]
    pf_curves, pf_trades = [x[:2] for x in pf], [x[2] for x in pf]
    req = [(pos, eq, int(e["from_bar"]), int(e["to_bar"])) for (pos, eq), e in zip(pf_curves, c.entries)]
    portfolio = {T: PR.portfolio(req, T, ann) for T in (max(c.bars), c.pf_bars)}
    cov_curves = [as_lists(row[i], p)[1] for i, p in c.cov_lanes]
    gram = G.covariance(cov_curves, c.cov_window or (0, WHOLE))
    summaries = summary_matrix(lanes)
    summaries.setflags(write=False)
    folds.setflags(write=False)
    return SimpleNamespace(lanes=lanes, curves=curves, summaries=summaries, folds=folds, steps=steps,
                           pf_curves=pf_curves, pf_trades=pf_trades, portfolio=portfolio, cov_curves=cov_curves,
                           gram=gram, surface=surface_ref(summaries, c.ids), topk=topk(summaries, c.ids, c.topk))


# ---------------------------------------------------------------------------------- coverage
COVERAGE = ("k65_fold64_both", "tile_32_starts", "trades", "picks", "no_picks", "traded", "open_end", "exit_last",
            "entry_first", "begins_inside", "empty_windows", "both_levels", "entry_crosses_stop", "narrow_sma_ties")


def _levels(side, epx, sl, tp):
    """Stop and target of a Bollinger trade (docs/oracle_spec.md: entry * (10000 -+ bps) / 10000,
    truncated; prices are positive)."""
    if side > 0:
        return epx * (10000 - sl) // 10000, epx * (10000 + tp) // 10000
    return epx * (10000 + sl) // 10000, epx * (10000 - tp) // 10000


def _hit(side, h, lo, sl_lvl, tp_lvl):
    return (lo <= sl_lvl, h >= tp_lvl) if side > 0 else (h >= sl_lvl, lo <= tp_lvl)


@functools.lru_cache(None)
def coverage(strategy, seed):
    """The counts named in COVERAGE for one case, from the case and its references alone."""
    c, r = lane_case(strategy, seed), lane_refs(strategy, seed)
    P, K = c.grid.n_params, len(c.bounds) - 1
    n = dict.fromkeys(COVERAGE, 0)
    nonempty = [[min(c.bounds[k], B) < min(c.bounds[k + 1], B) for k in range(K)] for B in c.bars]
    if K >= 65:
        n["k65_fold64_both"] = int(any(row[64] for row in nonempty) and not all(row[64] for row in nonempty))
    for B, row in zip(c.bars, nonempty):
        starts = np.bincount([c.bounds[k] // 64 for k in range(K) if row[k]], minlength=1)
        n["tile_32_starts"] |= int(starts.max() >= 32)
    for t in c.trains:
        picked = r.steps[t][0]["param"] >= 0
        n["picks"] += int(picked.sum())
        n["no_picks"] += int((~picked).sum())
    for s, B in enumerate(c.bars):
        h, lo, cl = (x.tolist() for x in c.series[s])
        for p in range(P):
            tr = r.lanes[s][p][1]
            n["trades"] += len(tr)
            ex = [(int(t["entry_bar"]), int(t["exit_bar"])) for t in tr]
            for k in range(K):
                if not nonempty[s][k]:
                    continue
                ck, ck1 = min(c.bounds[k], B), min(c.bounds[k + 1], B)
                n["traded"] += any(ck <= x < ck1 for _, x in ex)
                n["open_end"] += any(e <= ck1 - 1 < x for e, x in ex)
                n["exit_last"] += any(x == ck1 - 1 and x != B - 1 for _, x in ex)
                n["entry_first"] += any(e == ck for e, _ in ex)
            if strategy == "boll":
                kw = c.grid.param(p)
                for t in tr:
                    e, x, side = int(t["entry_bar"]), int(t["exit_bar"]), int(t["side"])
                    sl_lvl, tp_lvl = _levels(side, int(t["entry_px"]), kw["sl"], kw["tp"])
                    n["both_levels"] += x > e and all(_hit(side, h[x], lo[x], sl_lvl, tp_lvl))
                    n["entry_crosses_stop"] += _hit(side, h[e], lo[e], sl_lvl, tp_lvl)[0]
        if strategy == "sma" and KINDS[s % 4] == "narrow":
            pre = [0]
            for x in cl:
                pre.append(pre[-1] + x)
            for p in range(P):
                f, sw = c.grid.param(p)["f"], c.grid.param(p)["s"]
                if f != sw:   # decision bars: both windows full, up to B - 2
                    n["narrow_sma_ties"] += sum((pre[t + 1] - pre[t + 1 - f]) * sw == (pre[t + 1] - pre[t + 1 - sw]) * f
                                                for t in range(max(f, sw) - 1, B - 1))
    entries = c.entries
    n["begins_inside"] = PR.begins_inside_a_trade(entries, r.pf_trades)
    n["empty_windows"] = sum(min(int(e["to_bar"]), len(eq)) <= int(e["from_bar"])
                             for e, (_, eq) in zip(entries, r.pf_curves))
    return n
