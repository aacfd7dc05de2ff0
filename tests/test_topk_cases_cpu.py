"""The crafted top-k cases (tests/topk_cases.py) without a GPU: every case reaches the path of the
radix select it is there for, the reference (tests/topk_ref.py) is a plain sort, the host orders
(bt_merge_topk, bt_exchange_merge, dbx_amd.parallel) agree with it on the records where a signed
and an unsigned id order or a float and a bit-pattern compare could part, and the host rules of
bt_topk_of and bt_load_ohlc (csrc/topk_rules.cpp) through tests/plan/topk_plan_driver.cpp, once
more under AddressSanitizer and UBSan. The staging layout of bt_topk_of is checked with the other
plans in tests/test_launch_plan_cpu.py."""
import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from dbx_amd import parallel as PAR
from helpers import build_plan_driver, run_driver

import topk_cases as T
import topk_ref as R


# ------------------------------------------------------------------------- the cases' paths
@pytest.mark.parametrize("name", list(T.BUILDERS))
def test_case_reaches_its_path(name):
    c = T.case(name)
    got = T.path_counts(c.summaries, c.ids, c.k)
    for what, want in c.want.items():
        if isinstance(want, list):    # digits that must meet several bins / pass whole bins
            assert set(want) <= set(got[what]), (what, got["passes"])
        else:
            assert got[what] == want, (what, got[what], want)
    assert c.ids.min() >= 0 and len(c.summaries) == len(c.ids)
    assert not np.isnan(c.summaries["sharpe"]).any()


def test_the_cases_cover_the_paths_they_are_named_for():
    pc = {n: T.path_counts(T.case(n).summaries, T.case(n).ids, T.case(n).k) for n in T.BUILDERS}
    # the boundary of the sort and the tie finish, from both sides
    assert pc["sort_full"]["n_above"] + pc["sort_full"]["n_cand"] == T.CAP and not pc["sort_full"]["ties"]
    assert pc["tie_first"]["n_above"] + pc["tie_first"]["n_cand"] == T.CAP + 1 and pc["tie_first"]["ties"]
    # every pass of the tie finish meets several bins and subtracts a count in some case
    names = [f"key{s}" for s in (28, 16, 4, 0)] + [f"tb{s}" for s in (52, 40, 28, 16, 4, 0)]
    tie = [p for p in pc.values() if p["ties"]]
    for d in names:
        assert any(d in p["nontrivial"] for p in tie), d
        if d not in ("tb16",):   # param bits 27..16: at most two bins below 2^22 records, the cut in the upper
            assert any(d in p["above_nonzero"] for p in tie), d
    # all four low-bit passes in one case, with a count to subtract in each
    assert set(names[:4]) <= set(pc["low_bits_k1024"]["above_nonzero"]) & set(pc["low_bits_k100"]["above_nonzero"])
    # repeated ids: the cut inside records equal in key, id and param
    assert (pc["repeated_ids"]["need_equal"], pc["repeated_ids"]["n_equal"]) == (1, 3)
    # the second grid-stride iteration: past 256 blocks of 8,192 records; P past 2^16
    assert T.case("stride").n > 256 * 8192 and T.STRIDE_P > 1 << 16
    assert T.case("blocks").n > 2 * 8192
    assert all(T.case(n).n <= 1 << 18 for n in T.SMALL)
    # short: n < k, k == n, one record
    shapes = {(T.case(n).n, T.case(n).k) for n in T.BUILDERS if n.startswith("short")}
    assert {(1, 1), (1, 50), (7, 7), (7, 50), (7, 1)} <= shapes


def test_sign_cases_cut_where_they_say():
    def around(name):
        c = T.case(name)
        r = R.topk(c.summaries, c.ids, c.k + 1)["sharpe"]
        return r[c.k - 1], r[c.k]          # the last record taken and the first left
    neg_zero = lambda x: x == 0 and np.signbit(x)
    pos_zero = lambda x: x == 0 and not np.signbit(x)
    last, nxt = around("signs_k10")
    assert last > 0 and nxt > 0
    last, nxt = around("signs_k600")
    assert pos_zero(last) and neg_zero(nxt)
    last, nxt = around("signs_k1000")
    assert neg_zero(last) and neg_zero(nxt)
    last, nxt = around("signs_neg")
    assert last < 0 and nxt < 0 and np.isfinite(nxt)
    sh = T.case("signs_k10").summaries["sharpe"].reshape(-1)
    assert np.isposinf(sh).sum() == 2 and np.isneginf(sh).sum() == 2
    tiny = np.abs(sh[(sh != 0) & (np.abs(sh) < 2.3e-308)])
    assert len(tiny) == 6, "5e-324, 1e-310 and 2.5e-320 of both signs"
    assert (sh == 0).sum() == 2250 and np.signbit(sh[sh == 0]).sum() == 2100
    # the whole of a small case: the order crosses the sign bit and ends at -inf
    c = T.case("signs_neg")
    full = R.topk(c.summaries, c.ids, c.n)["sharpe"]
    assert np.isposinf(full[0]) and np.isneginf(full[-1]) and (full[1:] <= full[:-1]).all()
    z = np.flatnonzero(full == 0)
    assert not np.signbit(full[z[:50]]).any() and np.signbit(full[z[50:]]).all()


@pytest.mark.parametrize("name", T.SMALL)
def test_reference_is_a_plain_sort(name):
    c = T.case(name)
    got = R.topk(c.summaries, c.ids, c.k)
    assert len(got) == min(c.k, c.n)
    assert R.as_tuples(got) == R.topk_brute(c.summaries, c.ids, c.k)
    # the expected bytes are unique: records the order cannot tell apart are equal in every byte,
    # and only repeated ids give any
    every = R.as_tuples(R.topk(c.summaries, c.ids, c.n))
    assert len(set(every)) == len({t[:3] for t in every})
    assert (len(set(every)) < c.n) == (name == "repeated_ids")


def test_order_key_is_the_documented_map():
    x = np.array([np.inf, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf])
    k = R.order_key(x)
    assert (np.diff(k.astype(object)) < 0).all()
    assert int(k[3]) == 1 << 63 and int(k[4]) == (1 << 63) - 1
    assert (T.bits_of_key(k) == x.view(np.uint64)).all()


# ------------------------------------------------------------------- the host orders
def _records(summaries, ids):
    S, P = summaries.shape
    r = np.zeros(S * P, D.TOPK_DTYPE)
    r["sharpe"] = summaries["sharpe"].reshape(-1)
    r["pnl"] = summaries["pnl"].reshape(-1)
    r["sym"] = np.repeat(ids, P)
    r["param"] = np.tile(np.arange(P, dtype=np.int32), S)
    return r


@pytest.mark.parametrize("name", ["signs_k10", "signs_k600", "signs_k1000", "signs_neg", "id_digits", "repeated_ids"])
def test_host_orders_equal_the_reference(name):
    c = T.case(name)
    exp = R.topk(c.summaries, c.ids, c.k).tobytes()
    assert D.merge_topk(_records(c.summaries, c.ids), c.k).tobytes() == exp
    # three ranks, each with the sorted best k of its shard, as the exchange carries them
    parts = [R.topk(m, ids, c.k) for m, ids in T.shards(c)]
    assert sum(len(p) for p in parts) >= c.k and all(len(p) for p in parts)
    assert D.merge_topk(np.concatenate(parts), c.k).tobytes() == exp
    block = b"".join(E.exchange_message(p, c.k, 0, 0) for p in parts)
    got, _ = E.exchange_merge(block, 3, c.k, c.k)
    assert got.tobytes() == exp
    assert T.played(parts, lambda p, dist: PAR.gather_topk(p, c.k, dist)).tobytes() == exp
    got, cnt = T.played(parts, lambda p, dist: PAR.exchange(p, c.k, [len(p), 1], dist))
    assert got.tobytes() == exp and cnt == [sum(len(p) for p in parts), 3]


# ------------------------------------------------------------------------------ rules
SOURCES = ("plan.cpp", "topk_rules.cpp")


@pytest.fixture(scope="module")
def driver():
    exe = build_plan_driver("topk_plan_driver", SOURCES)
    return lambda *args: run_driver(exe, *args)


def _check_rules(run):
    #                                         S  P  k  sum ids out  ids...
    refusal = lambda *a: run("refusal", *a)["why"]
    assert refusal(1, 1, 1, 1, 1, 1, 0) == ""
    assert refusal(3, 2, 1024, 1, 1, 1, 0, 5, 2**31 - 1) == ""
    assert refusal(0, 2, 1, 1, 1, 1) == "S = 0 is below 1"
    assert refusal(-4, 0, 0, 0, 0, 0) == "S = -4 is below 1", "the first rule that fails speaks"
    assert refusal(2, 0, 1, 1, 1, 1, 0, 0) == "P = 0 is below 1"
    assert refusal(2, -1, 1, 1, 1, 1, 0, 0) == "P = -1 is below 1"
    assert refusal(1 << 22, 1, 1, 1, 1, 1) == "" and refusal(2048, 2048, 1024, 1, 1, 1) == ""
    assert refusal((1 << 22) + 1, 1, 1, 1, 1, 1) == "S*P = 4194305*1 exceeds 2^22 records"
    assert refusal(2049, 2048, 1, 1, 1, 1) == "S*P = 2049*2048 exceeds 2^22 records"
    assert refusal(2**31 - 1, 2**31 - 1, 1, 1, 1, 1) == "S*P = 2147483647*2147483647 exceeds 2^22 records"
    assert refusal(2, 2, 0, 1, 1, 1, 0, 0) == "k = 0 outside [1, 1024]"
    assert refusal(2, 2, 1025, 1, 1, 1, 0, 0) == "k = 1025 outside [1, 1024]"
    assert refusal(2, 2, -3, 1, 1, 1, 0, 0) == "k = -3 outside [1, 1024]"
    for have in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert refusal(2, 2, 5, *have, 0, 0) == "sum, sym_ids and out are required"
    assert refusal(4, 2, 5, 1, 1, 1, 0, 7, -7, -9) == "sym_ids[2] = -7 is negative"
    assert refusal(1, 2, 5, 1, 1, 1, -2**31) == "sym_ids[0] = -2147483648 is negative"
    assert refusal(2, 2, 0, 1, 1, 1, -1, -1) == "k = 0 outside [1, 1024]", "k before the ids"
    ids = lambda *a: run("ids", *a)["why"]
    assert ids() == "" and ids(0) == "" and ids(5, 0, 2**31 - 1, 7) == ""
    assert ids(1, 2, 3, -7, -8) == "sym_ids[3] = -7 outside [0, 2^31)"
    assert ids(2**31) == "sym_ids[0] = 2147483648 outside [0, 2^31)"
    assert ids(0, 2**32 + 5) == "sym_ids[1] = 4294967301 outside [0, 2^31)", "an id whose low 32 bits look valid"
    assert ids(0, -2**63) == "sym_ids[1] = -9223372036854775808 outside [0, 2^31)"


def test_refusal_and_id_rules_word_for_word(driver):
    _check_rules(driver)


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("topk_plan_driver", SOURCES, sanitize=True)
    run = lambda *args: run_driver(exe, *args, sanitized=True)
    _check_rules(run)
