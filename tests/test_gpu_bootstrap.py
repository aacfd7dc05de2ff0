"""Bootstrap reality check on the GPU (bt_bootstrap / bt_bootstrap_of, k_boot.hip;
docs/bootstrap_spec.md), every output field bit for bit against the Python-int reference of
bootstrap_ref.py: the resample path alone on staged increments (every T, L, B, n and group split of
the staged cases under both row modes, the ends of the range argument by closed form, groups of
257 to 600 lanes whose best sum ties at planted lanes), and the walked path on the random cases of
random_cases.py and the doubling cycles of limit_cases family A (list mode, all-lanes mode, one row
per chunk on the arena path, all-lanes mode in chunks that cut a row's group, two engines holding
half the rows each, the raw resampled sums reduced in Python, the refusals), and on ragged rows
under windows that begin and end at tile edges, at a row's end and one bar before it.
tests/test_bootstrap_cpu.py holds the host restatement to the same reference and proves that these
cases reach the plan shapes and outcomes the kernels can get wrong.
tests/test_gpu_tstats_boot_limits.py runs the limit families B, C and D; tests/test_gpu_random_lanes.py
runs the call among the other analysis calls on one engine."""
import re

import numpy as np
import pytest

import dbx_amd as D
import bootstrap_ref as R
import random_cases as RC

pytestmark = pytest.mark.gpu

OUTS = dict(per_lane=True, vmax=True, boot=True)
FIELDS = ("groups", "lanes", "vmax", "boot")


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]."""
    closes = [s[2] for s in series]
    if strategy == "boll":
        e.load_ohlc(closes, [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc(closes, sym_ids=ids)


def _bytes(rc, fields=FIELDS):
    return tuple(getattr(rc, f).tobytes() for f in fields)


def _one_row_budget(e, call):
    """The smallest budget the call runs in, as its refusal under a budget of one byte names it:
    everything held for the whole call and one prefix row."""
    e.set_boot_budget(1)
    try:
        with pytest.raises(D.BtError) as x:
            call()
    finally:
        e.set_boot_budget(0)
    m = re.search(r"the call needs (\d+) bytes of device staging, above the budget of 1 bytes", str(x.value))
    assert m, str(x.value)
    return int(m.group(1))


# ------------------------------------------------------- 1. the resample path alone, staged rows
@pytest.fixture(scope="module")
def bare():
    """An engine without a dataset: bt_bootstrap_of needs none."""
    with D.Engine(D.Grid.sma([2], [5])) as e:
        yield e


@pytest.mark.parametrize("T", R.OF_T)
def test_staged_cases_under_both_row_modes(bare, T):
    for k, c in enumerate(R.of_cases(T)):
        want = R.of_ref(T, k)
        where = f"T {T} L {c.L} B {c.B} n {c.n} groups {c.sizes}"
        for mode in (1, 2):
            bare.set_boot_row(mode)
            try:
                got = bare.bootstrap_of(c.d, groups=c.sizes, resamples=c.B, block=c.L, seed=c.seed, **OUTS)
            finally:
                bare.set_boot_row(0)
            R.assert_same(got, want, f"{where} row mode {mode}")


def test_range_ends_at_the_lds_size(bare):
    """|d| = 2^31 - 1, constant and alternating, over 4,096 bars: 32 KB of prefix row, which both
    row modes take; sums of 2^43."""
    T, B, L = 4096, 64, 101      # an odd block: an alternating row's block sums are +-(2^31 - 1), not 0
    alt = np.tile([R.PMAX, -R.PMAX], T // 2)
    d = np.stack([np.full(T, R.PMAX), np.full(T, -R.PMAX), alt, -alt]).astype(np.int32)
    want = R.reality_check(d.tolist(), [0, 2, 4], B, L, 0xE4D)
    const = R.constant_ref([R.PMAX, -R.PMAX], T, B, sizes=[2])
    assert want.lanes[:2].tobytes() == const.lanes.tobytes() and np.array_equal(want.boot[:2], const.boot)
    assert int(want.lanes["sum"][0]) == R.PMAX * T and len(set(want.boot[2].tolist())) > 1
    for mode in (0, 1, 2):
        bare.set_boot_row(mode)
        try:
            got = bare.bootstrap_of(d, groups=[2, 2], resamples=B, block=L, seed=0xE4D, **OUTS)
        finally:
            bare.set_boot_row(0)
        R.assert_same(got, want, f"range ends, row mode {mode}")


@pytest.mark.parametrize("T", (8127, 8128))
def test_the_lds_row_limit(bare, T):
    """The planner's threshold between the two row paths: T = 8,127 is the longest row that lives
    in LDS (512 + 8,128 * 8 = 64 KB of dynamic LDS, the most a launch asks for), 8,128 the first in
    the arena. The same reference on both sides, by the planner's choice and by request."""
    rng = np.random.default_rng([0x1D5, T])
    d = rng.integers(-5000, 5100, (3, T)).astype(np.int32)
    want = R.reality_check(d.tolist(), [0, 1, 3], 65, 100, 0x1D5)
    for mode in (0, 2) + ((1,) if T == 8127 else ()):
        bare.set_boot_row(mode)
        try:
            got = bare.bootstrap_of(d, groups=[1, 2], resamples=65, block=100, seed=0x1D5, **OUTS)
        finally:
            bare.set_boot_row(0)
        R.assert_same(got, want, f"T {T} row mode {mode}")
    if T == 8128:
        bare.set_boot_row(1)
        try:
            with pytest.raises(D.BtError, match=r"T \+ 1 = 8129 words \(65032 bytes\) does not fit the LDS row limit of 65024"):
                bare.bootstrap_of(d, resamples=65, block=100)
        finally:
            bare.set_boot_row(0)


def test_range_ends_at_the_longest_window(bare):
    """T = 2^22, constant +-(2^31 - 1): |S*| = (2^31 - 1) 2^22, just below 2^53, on the arena path
    (the row cannot live in LDS, and mode 1 says so). The reference is the closed form."""
    T, B = 1 << 22, 8
    d = np.empty((2, T), np.int32)
    d[0], d[1] = R.PMAX, -R.PMAX
    want = R.constant_ref([R.PMAX, -R.PMAX], T, B)
    assert abs(int(want.boot[1, 3])) == R.PMAX * T > 2**53 - 2**23
    got = bare.bootstrap_of(d, resamples=B, block=1 << 20, seed=1, **OUTS)
    R.assert_same(got, want, "T = 2^22")
    assert got.groups["best_lane"].tolist() == [0] and got.groups["n_ge"].tolist() == [0]
    bare.set_boot_row(1)
    try:
        with pytest.raises(D.BtError, match=r"a prefix row of T \+ 1 = 4194305 words \(33554440 bytes\) does not fit the "
                                            r"LDS row limit of 65024 bytes"):
            bare.bootstrap_of(d, resamples=B, block=1 << 20, seed=1)
    finally:
        bare.set_boot_row(0)


def test_m1_passes_int64(bare):
    """65,536 resamples of sums of (2^31 - 1) * 131,073: m1 = 2^64 and more."""
    T, B = 131073, 65536
    d = np.full((1, T), R.PMAX, np.int32)
    want = R.constant_ref([R.PMAX], T, B)
    assert int(want.lanes["m1_hi"][0]) >= 1
    got = bare.bootstrap_of(d, resamples=B, block=50_000, seed=2, **OUTS)
    R.assert_same(got, want, "m1 past 2^63")
    assert got.lane_se().tolist() == [0.0] and got.p_value().tolist() == [0.0]


@pytest.mark.parametrize("k", range(len(R.BIG_CASES)))
def test_staged_groups_above_256_lanes_with_planted_ties(bare, k):
    """257 to 600 lanes in groups of up to 600, so that a thread of boot_finish_kernel holds up to
    three lanes; the best row stands twice in a group: at two lanes of one thread, of two threads,
    at the group's first and last lane. The reference names the lower lane.
    Measured on an MI355X: below 0.07 s a case, its reference included."""
    c, want = R.big_case(k), R.big_ref(k)
    for mode in (1, 2):
        bare.set_boot_row(mode)
        try:
            got = bare.bootstrap_of(c.d, groups=c.sizes, resamples=c.B, block=c.L, seed=c.seed, **OUTS)
        finally:
            bare.set_boot_row(0)
        R.assert_same(got, want, f"n {c.n} groups {c.sizes} ties {c.ties} row mode {mode}")
    for g, a, _ in c.ties:
        assert int(got.groups["best_lane"][g]) == a


# ------------------------------------------------------------------------ 2. the walked path
@pytest.mark.parametrize("strategy,seed,name", R.CUT_CASES)
def test_all_lanes_mode_in_chunks_that_cut_a_group(strategy, seed, name):
    """All-lanes mode on the arena path under a budget of a third of the lanes a chunk, no multiple
    of P: rows' groups are cut by chunk boundaries, and a group's row of vmax is completed by two
    launches. The bytes of the unchunked call and of the reference.
    Measured on an MI355X: below 0.07 s a case."""
    c = RC.lane_case(strategy, seed)
    sub = R.walk_case(strategy, seed)[name]
    want = R.walk_ref(strategy, seed, name)
    S, P = len(c.series), c.grid.n_params
    frm, T = R.window_of(c, sub)
    per = R.cut_chunk(S, P)
    with D.Engine(c.grid) as e:
        _load(e, strategy, c.series, c.ids)
        call = lambda: e.reality_check(resamples=sub.B, block=sub.L, seed=sub.seed, window=sub.window, per_lane=True, vmax=True)
        whole = call()
        e.set_boot_row(2)
        e.set_boot_budget(R.arena_budget(S * P, S, T, sub.B, sub.L, False, False, per))
        try:
            cut = call()
        finally:
            e.set_boot_row(0)
            e.set_boot_budget(0)
    where = f"{strategy} seed {seed} {name}, {per} of {S * P} lanes a chunk"
    R.assert_same(cut, want, where, boot=False)
    assert _bytes(cut, FIELDS[:3]) == _bytes(whole, FIELDS[:3]), f"{where}: not the unchunked call's bytes"


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_window_edges_on_ragged_rows(strategy):
    """Rows of 1, 2, 64, 65, 130 and 700 bars under windows that begin at 0, 1, 63, 64, 65, 127,
    128 and 129 and hold 1, 63, 64, 65 and 129 bars: the tile of bar from - 1 is the window's first
    tile or the one before it, rows end at from, at from + 1 and inside the window, windows end on
    tile edges. Both row modes, list mode and all-lanes mode, 160 calls.
    Measured on an MI355X: below 0.07 s a strategy, the 40 references included."""
    c = R.edge_case(strategy)
    with D.Engine(c.grid) as e:
        _load(e, strategy, c.series)
        for frm in R.EDGE_FROM:
            for length in R.EDGE_LEN:
                want = R.edge_ref(strategy, frm, length)
                kw = dict(resamples=R.EDGE.B, block=R.EDGE.L, seed=R.EDGE.seed + 1000 * frm + length,
                          window=(frm, frm + length), per_lane=True, vmax=True)
                for mode in (1, 2):
                    where = f"{strategy} window [{frm}, {frm + length}) row mode {mode}"
                    e.set_boot_row(mode)
                    try:
                        got = e.reality_check(c.lanes, groups=c.sizes, boot=True, **kw)
                        every = e.reality_check(**kw)
                    finally:
                        e.set_boot_row(0)
                    R.assert_same(got, want, f"{where}, list mode")
                    R.assert_same(every, want, f"{where}, all-lanes mode", boot=False)


@pytest.mark.parametrize("strategy,seed", [(st, s) for st in RC.STRATEGIES for s in R.WALK_SEEDS])
def test_walked_cases(strategy, seed):
    c = RC.lane_case(strategy, seed)
    subs = R.walk_case(strategy, seed)
    where = f"{strategy} seed {seed}"
    S, P = len(c.series), c.grid.n_params
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, strategy, c.series, c.ids)
        e.run()
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        got = {}
        for name, sub in subs.items():
            call = lambda sub=sub, **kw: e.reality_check(R.sym_lanes(c, sub), groups=sub.sizes, resamples=sub.B,
                                                         block=sub.L, seed=sub.seed, window=sub.window, **{**OUTS, **kw})
            got[name] = call()
            want = R.walk_ref(strategy, seed, name)
            R.assert_same(got[name], want, f"{where} {name}")
            # boot reduces, in Python, to every other output
            frm, T = R.window_of(c, sub)
            R.assert_same(got[name], R.reduce_boot(got[name].boot, got[name].lanes["sum"], R.goff_of(sub.sizes)),
                          f"{where} {name}: boot reduced")
            # every output alone
            assert _bytes(call(per_lane=False, vmax=False, boot=False), ("groups",)) == _bytes(got[name], ("groups",))
            # the arena path, whole and with one row per chunk
            e.set_boot_row(2)
            try:
                assert _bytes(call()) == _bytes(got[name]), f"{where} {name}: arena path"
                if name in ("per_symbol", "past_shortest"):
                    e.set_boot_budget(_one_row_budget(e, call))
                    assert _bytes(call()) == _bytes(got[name]), f"{where} {name}: one row per chunk"
            finally:
                e.set_boot_row(0)
                e.set_boot_budget(0)
        # all-lanes mode: every row's P lanes one group, in dataset order
        for name in ("per_symbol", "inner", "past_shortest"):
            sub = subs[name]
            every = e.reality_check(resamples=sub.B, block=sub.L, seed=sub.seed, window=sub.window, per_lane=True, vmax=True)
            assert _bytes(every, FIELDS[:3]) == _bytes(got[name], FIELDS[:3]), f"{where} {name}: all-lanes mode"
            assert every.groups.shape == (S,) and every.lanes.shape == (S * P,) and every.vmax.shape == (S, sub.B)
        # a different seed changes vmax, the same seed repeats it
        sub = subs["per_symbol"]
        other = e.reality_check(resamples=sub.B, block=sub.L, seed=sub.seed + 1, vmax=True)
        again = e.reality_check(resamples=sub.B, block=sub.L, seed=sub.seed, vmax=True)
        assert np.array_equal(again.vmax, got["per_symbol"].vmax)
        if got["per_symbol"].vmax.any():   # a case without a trade has V* = 0 under every plan (counted in the CPU file)
            assert not np.array_equal(other.vmax, got["per_symbol"].vmax)
        assert np.array_equal(other.groups["best_sum"], again.groups["best_sum"])
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"
    # two engines with half the rows each and an explicit window: their results concatenate
    sub = subs["inner"]
    parts = []
    for rows in (slice(0, S // 2), slice(S // 2, S)):
        with D.Engine(c.grid) as e:
            _load(e, strategy, c.series[rows], c.ids[rows])
            parts.append(e.reality_check(resamples=sub.B, block=sub.L, seed=sub.seed, window=sub.window, per_lane=True,
                                         vmax=True))
    for f in FIELDS[:3]:
        assert np.concatenate([getattr(p, f) for p in parts]).tobytes() == getattr(got["inner"], f).tobytes(), \
            f"{where}: {f} of two shards"


@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_family_a_doubling_cycles(name):
    grid, series, want = R.family_a_ref(name)
    lanes = [(s, p) for s in range(len(series)) for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        got = e.reality_check(lanes, resamples=R.FAMILY_A.B, block=R.FAMILY_A.L, seed=R.FAMILY_A.seed, **OUTS)
    R.assert_same(got, want, f"family A {name}")


# ------------------------------------------------------------------------------- 3. refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    grid = D.Grid.sma([2, 4], [8, 16, 30])
    P = grid.n_params
    f = D.engine.sym("bt_bootstrap")
    grp = np.zeros(8, D.BOOT_GROUP_DTYPE)
    bt_ = np.zeros(8 * 16, np.int64)
    lanes = np.zeros(3, D.LANE_DTYPE)
    goff = np.array([0, 1, 3], np.int32)

    def last():
        return D.lib().bt_last_error().decode()

    with D.Engine(grid) as e:
        h, g, ln, go = e._h, grp.ctypes.data, lanes.ctypes.data, goff.ctypes.data
        assert f(h, 0, None, 0, None, 0, 0, 16, 5, 0, g, None, None, None) == -1 and "bt_bootstrap: no dataset loaded" in last()
        e.load_synthetic(0x5EED, 40, 4, 300, D.BT_DAILY)
        want = e.reality_check(resamples=16, block=5, seed=3, per_lane=True, vmax=True)
        assert want.groups["n_lanes"].tolist() == [P] * 4
        lanes["sym"], lanes["param"] = (40, 43, 41), (0, P - 1, 2)
        for args, named in (
            ((0, ln, 0, None, 0, 0, 16, 5, 0, g, None, None, None), "n = 0 outside [1, 1048576]"),
            (((1 << 20) + 1, ln, 0, None, 0, 0, 16, 5, 0, g, None, None, None), "n = 1048577 outside [1, 1048576]"),
            ((3, None, 0, None, 0, 0, 16, 5, 0, g, None, None, None), "n = 3 with lanes == NULL"),
            ((0, None, 2, go, 0, 0, 16, 5, 0, g, None, None, None), "G = 2 and goff given in all-lanes mode"),
            ((0, None, 0, None, 0, 0, 16, 5, 0, g, None, None, bt_.ctypes.data), "boot given in all-lanes mode"),
            ((3, ln, 3, None, 0, 0, 16, 5, 0, g, None, None, None), "G = 3 with goff == NULL"),
            ((3, ln, 4, go, 0, 0, 16, 5, 0, g, None, None, None), "G = 4 outside [1, n = 3]"),
            ((3, ln, 1, go, 0, 0, 16, 5, 0, g, None, None, None), "goff[1] = 1 is not n = 3"),
            ((3, ln, 2, go, -2, 0, 16, 5, 0, g, None, None, None), "from_bar = -2 is negative"),
            ((3, ln, 2, go, 7, 7, 16, 5, 0, g, None, None, None), "T = 0 bars of the window [7, 7)"),
            ((3, ln, 2, go, 9, 3, 16, 5, 0, g, None, None, None), "T = -6 bars of the window [9, 3)"),
            ((3, ln, 2, go, 1, (1 << 22) + 2, 16, 5, 0, g, None, None, None), "T = 4194305 bars"),
            ((3, ln, 2, go, 0, 0, 0, 5, 0, g, None, None, None), "B = 0 outside [1, 65536]"),
            ((3, ln, 2, go, 0, 0, 65537, 5, 0, g, None, None, None), "B = 65537 outside [1, 65536]"),
            ((3, ln, 2, go, 0, 0, 16, 0, 0, g, None, None, None), "L = 0 outside [1, 4194304]"),
            ((3, ln, 2, go, 0, 0, 16, (1 << 22) + 1, 0, g, None, None, None), "L = 4194305 outside [1, 4194304]"),
            ((3, ln, 2, go, 0, 0, 16, 5, 0, None, None, None, None), "groups, lanes, vmax and boot are all NULL"),
        ):
            assert f(h, *args) == -1
            assert last().startswith("bt_bootstrap: ") and named in last(), last()
        with pytest.raises(D.BtError, match=r"unknown symbol id 44 \(lane 1\)"):
            e.reality_check([(40, 0), (44, 0)])
        with pytest.raises(D.BtError, match=rf"param {P} outside \[0, {P}\) \(lane 2\)"):
            e.reality_check([(40, 0), (41, 1), (42, P)])
        with pytest.raises(ValueError, match="boot comes with lanes only"):
            e.reality_check(boot=True)
        with pytest.raises(ValueError, match="groups come with lanes"):
            e.reality_check(groups=[P] * 4)
        need = _one_row_budget(e, lambda: e.reality_check(resamples=16, block=5))
        e.set_boot_budget(need - 1)
        with pytest.raises(D.BtError, match=rf"the call needs {need} bytes of device staging, above the budget of {need - 1} bytes"):
            e.reality_check(resamples=16, block=5)
        e.set_boot_budget(need)
        assert e.reality_check(resamples=16, block=5, seed=3).groups.tobytes() == want.groups.tobytes()
        e.set_boot_budget(0)
        with pytest.raises(D.BtError, match="bytes = -5 is negative"):
            e.set_boot_budget(-5)
        with pytest.raises(D.BtError, match=r"mode = 3 outside \[0, 2\]"):
            e.set_boot_row(3)
        with pytest.raises(D.BtError, match=r"d\[1\]\[2\] = -2147483648 outside the domain"):
            e.bootstrap_of(np.array([[1, 2, 3], [4, 5, -2**31]]))
        with pytest.raises(D.BtError, match=r"bt_bootstrap_of: T = 0 bars"):
            e.bootstrap_of(np.zeros((2, 0), np.int32))
        assert f(None, 0, None, 0, None, 0, 0, 16, 5, 0, g, None, None, None) == -1 and "bt_bootstrap: null engine" in last()
        # the engine is usable afterwards, and says what it said before
        again = e.reality_check(resamples=16, block=5, seed=3, per_lane=True, vmax=True)
        assert _bytes(again, FIELDS[:3]) == _bytes(want, FIELDS[:3])
        pick = e.reality_check([(40, 0), (43, P - 1), (41, 2), (40, 0)], groups=[1, 3], resamples=16, block=5, seed=3,
                               per_lane=True)
        assert pick.lanes.tobytes() == want.lanes[[0, 3 * P + P - 1, P + 2, 0]].tobytes()
        assert pick.groups["n_lanes"].tolist() == [1, 3]
