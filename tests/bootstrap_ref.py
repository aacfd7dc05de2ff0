"""Reference for the bootstrap reality check (tests only), from the text of docs/bootstrap_spec.md:
the resample plan drawn bar by bar in Python ints (block start, then +1 mod T), every lane's
resampled sum as the sum of its increments at the drawn bars, and the records that follow. It forms
no prefix row, so it shares nothing with k_boot.hip, and it is not bootstrap.cpp.

The sums over the drawn bars go through numpy int64 when max|d| * T < 2^62 (no partial sum can
leave int64, so the result is the Python-int one; test_bootstrap_cpu.py pins the two to each other)
and through Python ints otherwise. The ends of the range (constant increments of 2^31 - 1 over 2^22
bars, m1 past 2^63) have closed forms, stated where they are used.

Also here: the shared cases of the two test files, built once per process and not to be modified
by a test: the walked cases on random_cases.lane_case and limit_cases family A, and the staged
cases of bt_bootstrap_of."""
import functools
from types import SimpleNamespace

import numpy as np

import dbx_amd as D
import limit_cases as LC
import random_cases as RC
from replay_ref import curves_from_trades

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def draw(seed, b, k):
    """docs/oracle_spec.md §1 with b in the place of sym: draw k (0-based)."""
    s0 = (seed ^ (b * GOLDEN)) & M64
    z = (s0 + (k + 1) * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def blocks(T, L):
    """[length of block j]: L' = min(L, T), K = ceil(T / L'), the last one truncated."""
    lp = min(L, T)
    K = -(-T // lp)
    return [lp] * (K - 1) + [T - (K - 1) * lp]


def starts(T, B, L, seed):
    """[b][j]: the block starts."""
    K = len(blocks(T, L))
    return [[draw(seed, b, j) % T for j in range(K)] for b in range(B)]


def bar_plan(T, B, L, seed):
    """[b]: the T bars resample b draws, one by one."""
    lens = blocks(T, L)
    out = []
    for row in starts(T, B, L, seed):
        bars = []
        for s, ln in zip(row, lens):
            at = s
            for _ in range(ln):
                bars.append(at)
                at = at + 1 if at + 1 < T else 0
        assert len(bars) == T
        out.append(bars)
    return out


def increments(equity, n_bars, frm, T):
    """d_k = E_(from+k) - E_(from+k-1) below the row's bar count, 0 elsewhere (E_(-1) = 0)."""
    E = [int(x) for x in equity[:n_bars]]
    out = []
    for k in range(T):
        t = frm + k
        out.append(E[t] - (E[t - 1] if t > 0 else 0) if t < n_bars else 0)
    return out


def resampled_sums(d, plan, exact=False):
    """[lane][b] Python ints: the sum of the lane's increments at the bars of resample b."""
    n, T = len(d), len(d[0])
    top = max((abs(x) for row in d for x in row), default=0)
    if not exact and top * T < 2**62:
        m = np.array(d, np.int64).reshape(n, T)
        return np.stack([m[:, np.array(bars, np.int64)].sum(axis=1) for bars in plan], axis=1).tolist()
    return [[sum(map(row.__getitem__, bars)) for bars in plan] for row in d]


def wide(v):
    return v & M64, v >> 64


def records(sums, star, goff):
    """The outputs from S_i and S*_(i,b): SimpleNamespace(groups, lanes, vmax, boot) as the arrays
    the library returns."""
    n, B, G = len(sums), len(star[0]), len(goff) - 1
    lanes = np.zeros(n, D.BOOT_LANE_DTYPE)
    for i in range(n):
        m1, m2 = sum(star[i]), sum(x * x for x in star[i])
        (lanes[i]["m1_lo"], lanes[i]["m1_hi"]), (lanes[i]["m2_lo"], lanes[i]["m2_hi"]) = wide(m1), wide(m2)
        lanes[i]["sum"], lanes[i]["n_nonpos"] = sums[i], sum(x <= 0 for x in star[i])
    groups = np.zeros(G, D.BOOT_GROUP_DTYPE)
    vmax = np.zeros((G, B), np.int64)
    for g in range(G):
        idx = range(goff[g], goff[g + 1])
        best = max(sums[i] for i in idx)
        v = [max(star[i][b] - sums[i] for i in idx) for b in range(B)]
        vmax[g] = v
        groups[g] = (best, min(i for i in idx if sums[i] == best) - goff[g], len(idx), sum(x >= best for x in v))
    return SimpleNamespace(groups=groups, lanes=lanes, vmax=vmax, boot=np.array(star, np.int64).reshape(n, B))


def reality_check(d, goff, B, L, seed, exact=False):
    """The whole reference on increments d[n][T] (lists of Python ints)."""
    T = len(d[0])
    star = resampled_sums(d, bar_plan(T, B, L, seed), exact)
    return records([sum(row) for row in d], star, goff)


def goff_of(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def assert_same(got, want, where, boot=True):
    """A RealityCheck against records(): every output, the first difference named."""
    for name in ("groups", "lanes"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{where}: {name} {g.shape} vs {w.shape}"
        for f in w.dtype.names:
            bad = np.flatnonzero(g[f] != w[f])
            assert not len(bad), f"{where}: {name}.{f}[{bad[0]}] = {g[f][bad[0]]}, want {w[f][bad[0]]} ({len(bad)} differ)"
        assert g.tobytes() == w.tobytes(), f"{where}: {name}"
    bad = np.argwhere(got.vmax != want.vmax)
    assert not len(bad), f"{where}: vmax{bad[0].tolist()} = {got.vmax[tuple(bad[0])]}, want {want.vmax[tuple(bad[0])]}"
    if boot:
        bad = np.argwhere(got.boot != want.boot)
        assert not len(bad), f"{where}: boot{bad[0].tolist()} = {got.boot[tuple(bad[0])]}, want {want.boot[tuple(bad[0])]}"


def reduce_boot(boot, sums, goff):
    """Every other output from the raw resampled sums (boot[n][B]) and S_i."""
    return records([int(x) for x in sums], [[int(x) for x in row] for row in boot], goff)


# ------------------------------------------------------------------- staged cases (bt_bootstrap_of)
OF_T = (1, 2, 63, 64, 65, 129)
OF_B = (1, 63, 64, 65, 200)
OF_N = (1, 2, 63, 65)
OF_SEED = 0xB007


def of_L(T):
    return sorted({x for x in (1, 2, 7, 64, T - 1, T, T + 5) if x >= 1})


def of_splits(n):
    """Group sizes: one group, every lane its own, an uneven split."""
    out = [[n], [1] * n]
    if n >= 3:
        out.append([1, n // 3, n - 1 - n // 3])
    return out


@functools.lru_cache(None)
def of_cases(T):
    """The staged cases of one T: every L of of_L and B of OF_B (and 321, above the resample
    phase's 256 threads and no multiple of 64), with n and the group split cycling through OF_N x
    of_splits so that each appears several times. [SimpleNamespace(T, L, B, n, sizes, seed, d)]."""
    combos = [(n, tuple(sz)) for n in OF_N for sz in of_splits(n)]
    out, k = [], OF_T.index(T)
    for L in of_L(T):
        for B in OF_B + ((321,) if L == 7 else ()):
            n, sizes = combos[k % len(combos)]
            k += 1
            rng = np.random.default_rng([0xB0075, T, L, B])
            # small increments with a drift: resampled sums of both signs, ties in none
            d = rng.integers(-1000, 1100, (n, T)).astype(np.int32)
            d.setflags(write=False)
            out.append(SimpleNamespace(T=T, L=L, B=B, n=n, sizes=list(sizes), seed=OF_SEED + 7 * k, d=d))
    return out


@functools.lru_cache(None)
def of_ref(T, k):
    c = of_cases(T)[k]
    return reality_check(c.d.tolist(), goff_of(c.sizes), c.B, c.L, c.seed)


# ----------------------------------------------- staged cases with groups above 256 lanes
# boot_finish_kernel has 256 threads: thread t holds lanes t, t + 256, t + 512, .. of its group and
# keeps the first of equal sums; a tree over the threads then keeps the lower lane. The best row of
# a group is planted at two lanes (and zeroed where it stood), so that the best sum ties:
#   "same_thread": lanes 3 and 259, both thread 3's; "two_threads": lanes 5 and 70;
#   "ends": lane 0 and the group's last.
FINISH_THREADS = 256
BIG_T, BIG_B, BIG_L = 65, 64, 7
# (n, group sizes, the tie planted in each group or None)
BIG_CASES = (
    (257, (257,), ("ends",)),                                    # lanes 0 and 256: one thread after all
    (600, (600,), ("same_thread",)),
    (600, (300, 1, 299), ("same_thread", None, "two_threads")),
    (600, (300, 1, 299), ("two_threads", None, "ends")),
    (577, (256, 321), ("ends", "ends")),                         # a group boundary at lane 256
)


def _tie_lanes(kind, m):
    return {"same_thread": (3, 3 + FINISH_THREADS), "two_threads": (5, 70), "ends": (0, m - 1)}[kind]


@functools.lru_cache(None)
def big_case(k):
    """SimpleNamespace(n, sizes, ties [(group, first lane, second lane) within the group], d, seed)
    of BIG_CASES[k]."""
    n, sizes, kinds = BIG_CASES[k]
    rng = np.random.default_rng([0xB16, k])
    d = rng.integers(-1000, 1100, (n, BIG_T)).astype(np.int32)
    goff, ties = goff_of(sizes), []
    for g, kind in enumerate(kinds):
        if kind is None:
            continue
        i0, m = goff[g], sizes[g]
        best = i0 + int(np.argmax(d[i0:i0 + m].sum(axis=1)))
        row = d[best].copy()
        a, b = _tie_lanes(kind, m)
        assert 0 <= a < b < m
        d[best] = 0
        d[i0 + a] = d[i0 + b] = row
        ties.append((g, a, b))
    d.setflags(write=False)
    return SimpleNamespace(n=n, sizes=list(sizes), ties=ties, d=d, seed=0xB16 + k, T=BIG_T, B=BIG_B, L=BIG_L)


@functools.lru_cache(None)
def big_ref(k):
    c = big_case(k)
    return reality_check(c.d.tolist(), goff_of(c.sizes), c.B, c.L, c.seed)


def _up(x):
    return (x + 255) // 256 * 256


def arena_budget(n, G, T, B, L, lst, boot, per):
    """The staging budget under which plan_boot takes `per` lanes per chunk on the arena path of a
    walked call, from the text of plan.h: what is held for the whole call and `per` prefix rows of
    ceil((T + 1) / 32) lines of 256 bytes."""
    K = -(-T // min(L, T))
    fixed = (_up(K * B * 4) + _up((G + 1) * 4) + _up(G * B * 8) + _up(G * 24) + _up(n * 48) + _up(n * B * 8 if boot else 0)
             + _up(n * 16 if lst else 0) + _up(n * 4 if lst else 0))
    return fixed + per * ((T + 1 + 31) // 32 * 256)


# all-lanes mode in chunks that cut a symbol's group: (strategy, seed, sub-case)
CUT_CASES = (("sma", 0, "per_symbol"), ("ema_ols", 1, "inner"), ("boll", 2, "past_shortest"))


def cut_chunk(S, P):
    """Lanes per chunk for S rows of P lanes: a third of them, less one where that is a multiple
    of P, so that chunk boundaries fall inside groups."""
    per = S * P // 3
    return per - 1 if per % P == 0 else per


PMAX = 2**31 - 1


def constant_ref(c, T, B, n_lanes=1, sizes=None):
    """Closed form for rows of constant increments c[i]: every block of len bars sums to c * len
    wherever it starts and however it wraps, and the blocks of a resample hold T bars, so S* = c T
    = S_i for every resample: m1 = B c T, m2 = B (c T)^2, V* = 0."""
    sums = [ci * T for ci in c]
    return records(sums, [[s] * B for s in sums], goff_of(sizes or [len(c)]))


# ------------------------------------------------------------------------ walked cases
WALK_SEEDS = range(4)
WALK_B = 40


@functools.lru_cache(None)
def walk_case(strategy, seed):
    """The sub-cases of random_cases.lane_case(strategy, seed): name -> SimpleNamespace(lanes [(row,
    param)], sizes, window (from, to) or None, B, L, seed). per_symbol and one_group hold every lane
    in dataset order; duplicate holds one row's lanes and the row's best lane again (a tie);
    inner begins inside an open trade of some lane; past_shortest begins past the shortest rows'
    ends; beyond ends beyond every row (and L >= T: one block)."""
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    S, P = len(c.series), c.grid.n_params
    every = [(s, p) for s in range(S) for p in range(P)]
    longest = max(c.bars)
    s_long = c.bars.index(longest)
    sums = [int(r.curves[s_long][p][1][-1]) for p in range(P)]
    dup = [(s_long, p) for p in range(P)] + [(s_long, sums.index(max(sums)))]
    # a bar inside the longest open trade of the longest row
    tr = max((t for p in range(P) for t in ([] if r.lanes[s_long][p][1] is None else r.lanes[s_long][p][1])),
             key=lambda t: int(t["exit_bar"]) - int(t["entry_bar"]), default=None)
    inner_from = 1 if tr is None else (int(tr["entry_bar"]) + int(tr["exit_bar"]) + 1) // 2
    inner_from = max(min(inner_from, longest - 2), 1)
    second = sorted(c.bars)[-2]
    # the resampling seed: distinct per case for seeds below 16 (WALK_SEEDS are 0 to 3); a wider
    # sweep of case seeds (BT_RANDOM_SEEDS) reuses resampling seeds across strategies, on other data
    k = RC.STRATEGIES.index(strategy) * 16 + seed
    mk = lambda lanes, sizes, window, L, B=WALK_B: SimpleNamespace(lanes=lanes, sizes=sizes, window=window, B=B, L=L,
                                                                   seed=0x5EED0 + k)
    return {
        "per_symbol": mk(every, [P] * S, None, 10),
        "one_group": mk(every, [S * P], None, 64, 24),
        "duplicate": mk(dup, [P + 1], None, 7),
        "inner": mk(every, [P] * S, (inner_from, min(inner_from + 257, longest)), 10),
        "past_shortest": mk(every, [P] * S, (min(130, second - 1), min(130, second - 1) + 200), 33),
        "beyond": mk(every, [S * P], (max(longest - 50, 0), longest + 77), 10_000, 24),
    }


def window_of(c, sub):
    """(from, T) of a sub-case: the default window is [0, B_max) over the requested rows."""
    if sub.window is None:
        return 0, max(c.bars[s] for s, _ in sub.lanes)
    return sub.window[0], sub.window[1] - sub.window[0]


@functools.lru_cache(None)
def walk_ref(strategy, seed, name):
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    sub = walk_case(strategy, seed)[name]
    frm, T = window_of(c, sub)
    d = [increments(r.curves[s][p][1], c.bars[s], frm, T) for s, p in sub.lanes]
    return reality_check(d, goff_of(sub.sizes), sub.B, sub.L, sub.seed)


def sym_lanes(c, sub):
    """The sub-case's lanes as (symbol id, param) pairs."""
    return [(c.ids[s], p) for s, p in sub.lanes]


# ------------------------------------------------- window edges of the walked row (ragged rows)
EDGE_FROM = (0, 1, 63, 64, 65, 127, 128, 129)
EDGE_LEN = (1, 63, 64, 65, 129)
EDGE = SimpleNamespace(B=16, L=5, seed=0xED6E)


@functools.lru_cache(None)
def edge_case(strategy):
    """The ragged rows of tradestats_ref (1, 2, 64, 65, 130 and 700 bars) under the small grid of
    their strategy: SimpleNamespace(grid, series [(h, l, c)], bars, lanes [(row, param)], sizes (one
    group per row), curves [equity of lane i, from the oracle's complete trade list])."""
    import tradestats_ref as TS
    from replay_ref import oracle_lane
    grid, series = TS.RAGGED_GRIDS[strategy](), TS.ragged_series(strategy)
    P = grid.n_params
    lanes, curves = [], []
    for s, ohlc in enumerate(series):
        for p in range(P):
            summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=len(ohlc[2]))
            assert int(summ["n_trades"]) == (0 if tr is None else len(tr))
            lanes.append((s, p))
            curves.append(curves_from_trades(ohlc[2], tr)[1])
    return SimpleNamespace(grid=grid, series=series, bars=[len(s[2]) for s in series], lanes=lanes,
                           sizes=[P] * len(series), curves=curves)


@functools.lru_cache(None)
def edge_ref(strategy, frm, length):
    c = edge_case(strategy)
    d = [increments(eq, len(eq), frm, length) for eq in c.curves]
    return reality_check(d, goff_of(c.sizes), EDGE.B, EDGE.L, EDGE.seed + 1000 * frm + length)


# ---------------------------------------------------------- long rows (limit_cases B, C and D)
def increments_fast(equity, frm, T):
    """increments for an int64 curve of millions of bars: np.diff over the window's bars, zeros
    past the row's end."""
    E = np.asarray(equity, np.int64)
    t1 = min(frm + T, len(E))
    out = np.zeros(T, np.int64)
    if t1 > frm:
        seg = E[frm - 1:t1] if frm > 0 else np.concatenate([[0], E[:t1]])     # E_(-1) = 0
        out[:t1 - frm] = np.diff(seg)
    return out.tolist()


LIMITS = SimpleNamespace(B=16, L=100, seed=0x11A17)


FAMILY_A = SimpleNamespace(B=32, L=31, seed=0xFA)


@functools.lru_cache(None)
def family_a_ref(name):
    """(grid, series [(c, h, l)], reference) of limit_cases family A, the doubling cycles: every
    lane in one group over [0, B_max)."""
    strategy, grid, series, rows = LC._a_case(name)
    T = max(len(c) for c, _, _ in series)
    d = []
    for (c, _, _), (summ, trades) in zip(series, rows):
        for p in range(grid.n_params):
            assert int(summ[p]["n_trades"]) == len(trades[p]) <= LC.CAP_A, "family A keeps complete trade lists"
            d.append(increments(curves_from_trades(c, trades[p])[1], len(c), 0, T))
    return grid, series, reality_check(d, [0, len(d)], FAMILY_A.B, FAMILY_A.L, FAMILY_A.seed)
