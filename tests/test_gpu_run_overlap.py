"""Consecutive runs on two streams (bt_set_run_overlap, on by default): whatever is enqueued between
and behind pipelined runs, with no host wait of the test's own, every result equals byte for byte
what an engine with the overlap switched off gives for one run.

The shard is 1,600 symbols x 1,000 bars on config 2's grid: two rounds of the 768 resident blocks,
about 0.13 ms per kernel, long enough for the host to enqueue the next run while this one executes."""
import functools
import time

import numpy as np
import pytest

import dbx_amd as D
from helpers import gpu_cus

pytestmark = pytest.mark.gpu

S, BARS, TOPK = 1600, 1000, 100
SEED, SEED2 = 0x5EED, 0xBEEF
LANES = [(0, 1), (5, 7)]


def grid():
    return D.Grid.sma(range(4, 43, 2), range(50, 241, 10))


def engine(overlap, seed=SEED, **kw):
    e = D.Engine(grid(), device=0, topk=kw.pop("topk", TOPK), **kw)
    e.set_run_overlap(overlap)
    e.load_synthetic(seed, 0, S, BARS, D.BT_DAILY)
    return e


def _replay_bytes(rp):
    return b"".join(a.tobytes() for a in (rp.summaries, rp.n_bars, rp.trades, rp.equity, rp.pos) if a is not None)


def _surface_bytes(sf):
    return sf.params.tobytes() + sf.best.tobytes()


@functools.lru_cache(None)
def serial(seed):
    """One run of an engine that never overlaps, read after a sync(): computed once per seed."""
    with engine(0, seed) as e:
        e.run()
        e.topk_fetch_async(0)
        top, trades = e.topk_fetch_wait(0)
        e.sync()
        return {"top": top.tobytes(), "trades": trades, "summaries": e.summaries().tobytes(),
                "surface": _surface_bytes(e.surface()), "stats": e.stats(),
                "replay": _replay_bytes(e.replay(LANES, trade_cap=8, curves=True))}


def pipelined(e, n, before_run=None):
    """n runs, run r fetched into slot r % PIPE_SLOTS and consumed after run r + 1 is enqueued: two
    runs in flight, no sync(). Returns [(records, trades)] per run."""
    out = []

    def issue(r):
        if before_run:
            before_run(r)
        e.run()
        e.topk_fetch_async(r % D.PIPE_SLOTS)

    issue(0)
    for r in range(n):
        if r + 1 < n:
            issue(r + 1)
        top, trades = e.topk_fetch_wait(r % D.PIPE_SLOTS)
        out.append((top.tobytes(), trades))
    return out


def test_seventy_pipelined_runs_equal_one_serial_run():
    # 70 runs pass every slot of the 64-slot trade-counter ring and both of its zeroing points: a
    # lost zeroing or a double accumulation shows in the trade count
    want = serial(SEED)
    # the shard is several rounds of blocks (8-wave blocks: at most four to a CU), so the planner
    # lets these runs overlap: the tests of this file are about the two-stream path
    assert S > 4 * gpu_cus()
    with engine(1) as e:
        got = pipelined(e, 70)
        summaries = e.summaries().tobytes()
    assert len(want["top"]) == TOPK * D.TOPK_DTYPE.itemsize and want["trades"] > 0
    for r, (top, trades) in enumerate(got):
        assert trades == want["trades"], (r, trades, want["trades"])
        assert top == want["top"], r
    assert summaries == want["summaries"]


def test_loads_between_pipelined_runs():
    # a load is ordered behind the run before it and the run after it behind the load, whichever
    # stream either is on
    seeds = (SEED, SEED2)
    assert serial(SEED)["top"] != serial(SEED2)["top"]
    with engine(1) as e:
        got = pipelined(e, 8, before_run=lambda r: e.load_synthetic(seeds[r % 2], 0, S, BARS, D.BT_DAILY))
    for r, (top, trades) in enumerate(got):
        want = serial(seeds[r % 2])
        assert trades == want["trades"], (r, trades, want["trades"])
        assert top == want["top"], r


def test_split_and_unsplit_runs_alternate():
    # a split run keeps single-buffered segment records: it overlaps neither neighbour, and split
    # equals unsplit bit for bit
    want = serial(SEED)
    with engine(1) as e:
        out = []
        for r in range(8):  # run r + 1 is enqueued before run r is consumed
            asked = 2 if r % 2 == 0 else 1
            e.set_segments(asked)
            e.run()
            assert e.last_segments() == asked, r
            e.topk_fetch_async(r % D.PIPE_SLOTS)
            if r:
                out.append(e.topk_fetch_wait((r - 1) % D.PIPE_SLOTS))
        out.append(e.topk_fetch_wait(7 % D.PIPE_SLOTS))
        summaries = e.summaries().tobytes()
    for r, (top, trades) in enumerate(out):
        assert trades == want["trades"], (r, trades, want["trades"])
        assert top.tobytes() == want["top"], r
    assert summaries == want["summaries"]


def test_reads_and_analysis_calls_right_behind_three_runs():
    want = serial(SEED)
    for call in ("summaries", "surface", "replay", "stats"):
        with engine(1) as e:
            e.run()
            e.run()
            e.run()
            if call == "summaries":
                assert e.summaries().tobytes() == want["summaries"]
            elif call == "surface":
                assert _surface_bytes(e.surface()) == want["surface"]
            elif call == "replay":
                assert _replay_bytes(e.replay(LANES, trade_cap=8, curves=True)) == want["replay"]
            else:
                assert e.stats() == want["stats"]
    with engine(1) as e:  # and all four behind the same three runs
        e.run()
        e.run()
        e.run()
        assert e.summaries().tobytes() == want["summaries"]
        assert _surface_bytes(e.surface()) == want["surface"]
        assert _replay_bytes(e.replay(LANES, trade_cap=8, curves=True)) == want["replay"]
        assert e.stats() == want["stats"]


def test_parity_engine_stays_serial():
    # parity sums and trade lists are single-buffered: four pipelined runs give one run's bytes
    small = D.Grid.sma([3, 5], [20, 31])
    got = []
    for overlap, runs in ((0, 1), (1, 4)):
        with D.Engine(small, device=0, parity=True, trade_cap=8) as e:
            e.set_run_overlap(overlap)
            e.load_synthetic(SEED, 0, 3, 300, D.BT_DAILY)
            for _ in range(runs):
                e.run()
            got.append((e.trades().tobytes(), e.sums().tobytes(), e.summaries().tobytes()))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] and got[0][2] == got[1][2]
    assert np.frombuffer(got[0][0], D.TRADE_DTYPE)["exit_bar"].any()


def test_timing_stays_a_throughput_time():
    # overlapping runs are accounted end to end (a run counts from its start or from the end of
    # the run before it, whichever is later), so their sum cannot exceed the time they covered
    with engine(1, timing=True) as e:
        e.run()
        e.sync()
        e.reset_timing()
        t0 = time.perf_counter()
        pipelined(e, 12)
        e.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        total, launches, name = e.kernel_timing()
        print(f"12 pipelined runs: kernel time {total:.4f} ms, host wall {wall_ms:.4f} ms")
        assert launches == 12 and name == "bt::sma_kernel"
        assert 0.0 < total <= wall_ms, (total, wall_ms)
    with engine(0, timing=True) as e:
        e.run()
        e.sync()
        e.reset_timing()
        pipelined(e, 12)
        total, launches, _ = e.kernel_timing()
        assert launches == 12 and total > 0.0
        prev = total
        for r in range(4):  # every per-run figure
            e.run()
            total, launches, _ = e.kernel_timing()
            print(f"serial run {r}: {total - prev:.4f} ms")
            assert launches == 13 + r and total - prev > 0.0, (r, total, prev)
            prev = total
