"""Engine lifecycle on one GPU: everything an engine can own (device buffers of every entry point,
pinned read-back slots and staging, the timing event pool, both streams) is created, used and
freed three times over in one process and the third cycle gives the first one's bytes; a refused
call leaves the engine usable; a caller's stream outlives the engine that borrowed it; the
analysis calls, which share one staging arena, give in any order what each gives on a fresh engine."""
import numpy as np
import pytest

import dbx_amd as D
import oracle_np as N
from dbx_amd import payload as PL

pytestmark = pytest.mark.gpu

S, BARS = 3, 300
SMA = D.Grid.sma([3, 5], [20, 31])


def _jobs():
    jobs = []
    for s, kind in ((0, "csv"), (1, "csv"), (2, "bin")):
        o, h, lo, c, v = N.gen(0x5EED, [s], BARS - 7 * s, 0)
        blob = (N.csv_bytes(o[0], h[0], lo[0], c[0], v[0], 0) if kind == "csv"
                else PL.encode_columns(o[0], h[0], lo[0], c[0], v[0]))
        jobs.append((f"job-{s}", blob))
    jobs.append(("job-bad", jobs[0][1][:len(jobs[0][1]) // 2] + b"\nnot,a,row\n"))
    return jobs


JOBS = _jobs()


def _replay_bytes(rp):
    return b"".join(a.tobytes() for a in (rp.summaries, rp.n_bars, rp.trades, rp.equity, rp.pos) if a is not None)


def _walkfwd_bytes(wf):
    return wf.steps.tobytes() + wf.total.tobytes() + wf.folds.tobytes()


def _cycle():
    out = {}
    with D.Engine(SMA, topk=3, timing=True) as e:
        e.load_synthetic(0x5EED, 0, S, BARS, D.BT_DAILY)
        for r in range(3):  # the second and third run take their event pair from the pool
            e.run()
            assert e.kernel_timing()[1] == r + 1
        for slot in range(D.PIPE_SLOTS):
            e.topk_fetch_async(slot)
        for slot in range(D.PIPE_SLOTS):
            top, n_trades = e.topk_fetch_wait(slot)
            out[f"top{slot}"] = top.tobytes() + n_trades.to_bytes(8, "little")
        summ = e.summaries()
        out["sma"] = summ.tobytes()
        surf = e.surface()
        of = e.surface_of(summ, np.arange(S, dtype=np.int32))
        assert of.params.tobytes() == surf.params.tobytes() and of.best.tobytes() == surf.best.tobytes()
        out["surface"] = surf.params.tobytes() + surf.best.tobytes()
        rp = e.replay([(0, 1), (2, 3)], trade_cap=8, curves=True)
        assert rp.summaries.tobytes() == summ[[0, 2], [1, 3]].tobytes()
        out["replay"] = _replay_bytes(rp)
        out["walk_forward"] = _walkfwd_bytes(e.walk_forward([0, 100, 200, 300], train=1, folds=True))
    with D.Engine(SMA, parity=True, trade_cap=8) as e:
        e.load_synthetic(0x5EED, 0, S, BARS, D.BT_DAILY)
        e.run()
        assert e.summaries().tobytes() == out["sma"]
        out["parity"] = e.sums().tobytes() + e.trades().tobytes()
    with D.Engine(D.Grid.boll([10], [2], [50], [50])) as e:  # the high and low columns
        e.load_synthetic(0x5EED, 0, S, BARS, D.BT_MINUTE)
        e.run()
        out["boll"] = e.summaries().tobytes()
    with D.Engine(SMA) as e:
        res = e.run_batch(JOBS)
        assert [st for st, _ in res] == [0, 0, 0, -1] and res[3][1].startswith('{"error":"')
        assert all(data.count("\n") == SMA.n_params for _, data in res[:3])
        assert e.batch_profile()["n_failed"] == 1
        out["batch"] = "".join(data for _, data in res).encode()
    return out


def test_three_create_use_close_cycles_give_the_same_bytes():
    first = _cycle()
    _cycle()
    third = _cycle()
    assert first.keys() == third.keys()
    for name in first:
        assert first[name] == third[name], name
    assert len(set(first[f"top{slot}"] for slot in range(D.PIPE_SLOTS))) == 1


def test_a_refused_call_leaves_the_engine_usable():
    with D.Engine(SMA, topk=3) as e:
        e.load_synthetic(0x5EED, 0, S, BARS, D.BT_DAILY)
        e.run()
        before = e.summaries().tobytes(), e.read_topk().tobytes()
        with pytest.raises(D.BtError, match=r"param 4 outside \[0, 4\)"):
            e.replay([(0, SMA.n_params)])
        with pytest.raises(D.BtError, match="bad arguments"):
            e.set_segments(-1)
        e.run()
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before
        assert e.replay([(1, 2)]).summaries.tobytes() == e.summaries()[1, 2].tobytes()


def test_a_borrowed_stream_outlives_its_engine():
    import torch
    s = torch.cuda.Stream(device=0)
    with D.Engine(SMA, topk=3, stream=s.cuda_stream) as e:
        e.load_synthetic(0x5EED, 0, S, BARS, D.BT_DAILY)
        e.run()
        got = e.summaries().tobytes()
    with D.Engine(SMA) as own:
        own.load_synthetic(0x5EED, 0, S, BARS, D.BT_DAILY)
        own.run()
        assert own.summaries().tobytes() == got
    with torch.cuda.stream(s):
        t = torch.arange(1024, device="cuda:0", dtype=torch.int64) * 3 + 1
    s.synchronize()
    assert t.cpu().tolist() == [3 * i + 1 for i in range(1024)]


# ------------------------------------------------------------------------ the shared arena
WF_BOUNDS = [0, 100, 200, 300]
# one row of K = 3 folds x P = 4 params (80-byte records, K - 1 steps of 104 bytes) and no second one
# beside the padded bounds and the two region roundings
WF_ONE_ROW = 256 + 2 * 256 + (3 * 4 * 80 + 2 * 104) * 3 // 2


def _surface_bytes(sf):
    return sf.params.tobytes() + sf.best.tobytes()


def _analysis_calls(summ):
    """name -> (budget to set first, the call): the analysis calls of the arena sequence."""
    of_ids = np.array([7, 3, 5], np.int32)
    return {
        "surface": (0, lambda e: _surface_bytes(e.surface())),
        "replay_full": (0, lambda e: _replay_bytes(e.replay([(0, 1), (2, 3), (1, 0)], trade_cap=8, curves=True))),
        "walk_forward": (0, lambda e: _walkfwd_bytes(e.walk_forward(WF_BOUNDS, train=1, folds=True))),
        "surface_of": (0, lambda e: _surface_bytes(e.surface_of(summ[::-1], of_ids))),
        "replay": (0, lambda e: _replay_bytes(e.replay([(2, 2)]))),
        "walk_forward_chunked": (WF_ONE_ROW, lambda e: _walkfwd_bytes(e.walk_forward(WF_BOUNDS, train=0, folds=True))),
    }


ARENA_SEQUENCE = ("surface", "replay_full", "walk_forward", "surface", "surface_of", "replay", "walk_forward_chunked",
                  "surface")


@pytest.mark.parametrize("strategy", ("sma", "boll"))
def test_analysis_calls_share_one_arena_in_any_order(strategy):
    """The arena grows, is reused at a smaller size and after chunked use: every result equals,
    byte for byte, what the same call returns as the first analysis call on a fresh engine."""
    grid = SMA if strategy == "sma" else D.Grid.boll([10, 20], [2, 3], [50], [50])   # boll: three columns
    freq = D.BT_DAILY if strategy == "sma" else D.BT_MINUTE
    assert grid.n_params == 4

    def fresh():
        e = D.Engine(grid)
        e.load_synthetic(0x5EED, 0, S, BARS, freq)
        e.run()
        return e

    with fresh() as e:
        summ = e.summaries().copy()
    calls = _analysis_calls(summ)
    want = {}
    for name, (budget, call) in calls.items():
        with fresh() as e:
            e.set_walkfwd_budget(budget)
            want[name] = call(e)
    assert len(set(want.values())) == len(want), "the calls give different bytes"
    assert want["walk_forward"] != want["walk_forward_chunked"]
    with fresh() as e:
        for step, name in enumerate(ARENA_SEQUENCE):
            budget, call = calls[name]
            e.set_walkfwd_budget(budget)
            assert call(e) == want[name], f"{strategy} step {step + 1}: {name}"
        assert e.summaries().tobytes() == summ.tobytes()
