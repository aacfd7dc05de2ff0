"""The top-k chain (k_topk.hip) on crafted key sets, through bt_topk_of: every path of the radix
select against a plain sort (tests/topk_ref.py), in bytes. The cases and the path each one reaches
are tests/topk_cases.py; tests/test_topk_cases_cpu.py asserts without a GPU that they reach it.
All of it is exact integer work: no tolerance anywhere."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from dbx_amd import parallel as PAR

import topk_cases as T
import topk_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """A tiny grid, no dataset, top-k disabled: bt_topk_of brings its whole work set."""
    with D.Engine(D.Grid.sma([2], [3]), topk=0) as e:
        yield e


@functools.lru_cache(None)
def expected(name):
    c = T.case(name)
    exp = R.topk(c.summaries, c.ids, c.k)
    exp.setflags(write=False)
    return exp


def _assert_same(got, exp, where):
    assert len(got) == len(exp), f"{where}: {len(got)} records, expected {len(exp)}"
    if got.tobytes() != exp.tobytes():
        rows = lambda r: np.frombuffer(r.tobytes(), np.uint8).reshape(len(r), -1)
        bad = np.flatnonzero((rows(got) != rows(exp)).any(1))
        i = int(bad[0])
        raise AssertionError(f"{where}: {len(bad)} records differ, first at {i}: {got[i]} expected {exp[i]}")


def _run(e, name, lds_free=False):
    c = T.case(name)
    got = e.topk_of(c.summaries, c.ids, c.k, lds_free_hist=lds_free)
    _assert_same(got, expected(name), f"{name}{' (no-LDS histogram)' if lds_free else ''}")
    assert len(got) == min(c.k, c.n)


@pytest.mark.parametrize("name", list(T.BUILDERS))
def test_every_case_equals_the_sort(eng, name):
    _run(eng, name)


@pytest.mark.parametrize("name", T.SMALL)
def test_histogram_without_lds_gives_the_same_bytes(eng, name):
    _run(eng, name, lds_free=True)


def test_back_to_back_chains_on_one_engine(eng):
    """The finish block leaves the selection state for the next chain, whichever finish ran."""
    for name in ("tie_first", "sort_full", "low_bits_k1024", "short_1x7_k50", "tie_first"):
        _run(eng, name)


def test_topk_of_disturbs_nothing_a_run_left():
    grid = D.Grid.sma([2, 3, 5], [8, 13])
    with D.Engine(grid, topk=32) as e:
        e.load_synthetic(0x70C, 40, 9, 300)
        e.run()
        read = lambda: (e.read_topk().tobytes(), e.summaries().tobytes(), sorted(e.stats().items()))
        before = read()
        assert len(before[0]) == 32 * D.TOPK_DTYPE.itemsize
        _run(e, "low_bits_k1024")
        assert read() == before
        e.run()
        assert e.read_topk().tobytes() == before[0]
        _run(e, "sort_full")
        assert read() == before


@pytest.mark.parametrize("name", ["id_digits", "signs_k600", "signs_k1000", "low_bits_k1024"])
def test_shards_merged_on_the_host_agree_with_one_device_selection(eng, name):
    """Three contiguous row shards, each selected on the device, merged by bt_merge_topk, by the
    exchange's merge and by dbx_amd.parallel: the records one selection over all rows gives."""
    c = T.case(name)
    parts = [eng.topk_of(m, ids, c.k) for m, ids in T.shards(c)]
    for (m, ids), p in zip(T.shards(c), parts):
        _assert_same(p, R.topk(m, ids, c.k), f"{name} shard of {len(ids)} rows")
    whole = eng.topk_of(c.summaries, c.ids, c.k)
    exp = expected(name)
    _assert_same(whole, exp, name)
    _assert_same(D.merge_topk(np.concatenate(parts), c.k), exp, f"{name} bt_merge_topk")
    got, _ = E.exchange_merge(b"".join(E.exchange_message(p, c.k, 0, 0) for p in parts), 3, c.k, c.k)
    _assert_same(got, exp, f"{name} bt_exchange_merge")
    _assert_same(T.played(parts, lambda p, dist: PAR.gather_topk(p, c.k, dist)), exp, f"{name} gather_topk")
    got, _ = T.played(parts, lambda p, dist: PAR.exchange(p, c.k, [0, 0], dist))
    _assert_same(got, exp, f"{name} parallel.exchange")


def test_refusals_name_the_value_and_leave_the_engine_usable(eng):
    f = E.sym("bt_topk_of")
    c = T.case("short_1x7_k7")
    m = np.ascontiguousarray(c.summaries)
    ids = np.ascontiguousarray(c.ids)
    neg = np.array([3, -1, 4], np.int32)
    m3 = np.ascontiguousarray(np.concatenate([m, m, m]))
    out = np.zeros(1024, D.TOPK_DTYPE)
    sp, ip, op = m.ctypes.data, ids.ctypes.data, out.ctypes.data

    def good():
        out[:] = 0
        assert f(eng._h, 1, 7, sp, ip, 7, 0, op) == 7
        _assert_same(out[:7], expected("short_1x7_k7"), "after a refusal")

    good()
    for args, msg in (
        ((None, 1, 7, sp, ip, 7, 0, op), r"bt_topk_of: null engine"),
        ((eng._h, 0, 7, sp, ip, 7, 0, op), r"S = 0 is below 1"),
        ((eng._h, -2, 7, sp, ip, 7, 0, op), r"S = -2 is below 1"),
        ((eng._h, 1, 0, sp, ip, 7, 0, op), r"P = 0 is below 1"),
        ((eng._h, 2049, 2048, sp, ip, 7, 0, op), r"S\*P = 2049\*2048 exceeds 2\^22"),
        ((eng._h, 1, 7, sp, ip, 0, 0, op), r"k = 0 outside \[1, 1024\]"),
        ((eng._h, 1, 7, sp, ip, 1025, 0, op), r"k = 1025 outside \[1, 1024\]"),
        ((eng._h, 1, 7, None, ip, 7, 0, op), r"sum, sym_ids and out are required"),
        ((eng._h, 1, 7, sp, None, 7, 0, op), r"sum, sym_ids and out are required"),
        ((eng._h, 1, 7, sp, ip, 7, 0, None), r"sum, sym_ids and out are required"),
        ((eng._h, 3, 7, m3.ctypes.data, neg.ctypes.data, 7, 0, op), r"sym_ids\[1\] = -1 is negative"),
    ):
        assert f(*args) == -1, msg
        err = E.lib().bt_last_error().decode()
        assert err.startswith("bt_topk_of: ") and re.search(msg, err), (msg, err)
        good()
    with pytest.raises(D.BtError, match=r"sym_ids\[1\] = -1"):
        eng.topk_of(m3, neg, 7)
    with pytest.raises(D.BtError, match=r"k = 2000 "):
        eng.topk_of(m, ids, 2000)
    good()


def test_load_ohlc_refuses_an_id_outside_the_range_and_keeps_the_dataset():
    rng = np.random.default_rng(5)
    closes = [np.clip(1_000_000 + np.cumsum(rng.integers(-3000, 3100, n)), 10_000, 2**31 - 1).astype(np.int32)
              for n in (200, 333, 64)]
    with D.Engine(D.Grid.sma([2, 3, 5], [8, 13]), topk=5) as e:
        e.load_ohlc(closes, sym_ids=[2**31 - 1, 0, 77])
        e.run()
        first = (e.summaries().tobytes(), e.read_topk().tobytes(), sorted(e.stats().items()))
        bars = np.array([len(c) for c in closes], np.int32)
        offs = np.array([0, 200, 533], np.int64)
        cat = np.ascontiguousarray(np.concatenate(closes))
        for bad, msg in (([5, -1, 7], r"bt_load_ohlc: sym_ids\[1\] = -1 outside \[0, 2\^31\)"),
                         ([5, 6, 2**31], r"bt_load_ohlc: sym_ids\[2\] = 2147483648 outside \[0, 2\^31\)"),
                         ([2**32 + 1, 6, 7], r"bt_load_ohlc: sym_ids\[0\] = 4294967297 outside")):
            ids = np.array(bad, np.int64)
            rc = E.lib().bt_load_ohlc(e._h, 3, ids.ctypes.data, bars.ctypes.data, offs.ctypes.data, None, None,
                                      cat.ctypes.data)
            assert rc == -1
            assert re.search(msg, E.lib().bt_last_error().decode()), E.lib().bt_last_error()
            with pytest.raises(D.BtError, match=msg):
                e.load_ohlc(closes, sym_ids=bad)
            # the dataset loaded before is still the resident one
            assert (e.summaries().tobytes(), e.read_topk().tobytes(), sorted(e.stats().items())) == first
            e.run()
            assert (e.summaries().tobytes(), e.read_topk().tobytes(), sorted(e.stats().items())) == first
        assert set(e.read_topk()["sym"].tolist()) <= {2**31 - 1, 0, 77}
