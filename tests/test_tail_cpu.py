"""Tail risk, the parts that need no GPU (docs/tail_spec.md): bt_tail_host against the Python-int
reference of tail_ref.py on every lane of the random cases, the ragged rows and limit family A, in
both modes of counting, over the whole window and a cut one; proof from the references alone that the
cases reach what the selection can get wrong; every refusal; the record layouts
(tests/tail_abi_host.c); the chunk planner (plan_tail through tests/plan/tail_plan_driver.cpp);
planner and host code as a stand-alone program under AddressSanitizer and UBSan
(tests/asan/tail_driver.cpp); and the derived views of TailRisk against their restatement."""
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import random_cases as RC
import tail_ref as R
from helpers import CSRC, SANITIZE, SANITIZE_ENV, assert_staging_layout, build_plan_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(8)
LEVELS = R.LEVELS
Q = len(LEVELS)
MODES = [(held, cut) for held in (False, True) for cut in (False, True)]


def _host(curves, window, held, levels=LEVELS):
    eq, ps, nb = R.as_curve_arrays(curves)
    return D.tail_risk_host(eq, ps, nb, levels, window, held)


# ------------------------------------------------------------ (a) the host code to the reference
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_every_lane_of_the_random_cases(strategy):
    lanes = 0
    for seed in SEEDS:
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        S, P = len(c.series), c.grid.n_params
        curves = [r.curves[s][p] for s in range(S) for p in range(P)]
        for held, cut in MODES:
            recs, qs, window = R.random_refs(strategy, seed, held, cut)
            got = _host(curves, window, held)
            where = f"{strategy} seed {seed}, held={held}, window={window}"
            R.assert_same(got.lanes, recs.reshape(-1), f"{where}: records")
            R.assert_same(got.quantiles, qs.reshape(S * P, Q), f"{where}: quantiles")
        eq, _, nb = R.as_curve_arrays(curves)       # pos may be left out in all-bars mode
        recs, qs, _ = R.random_refs(strategy, seed)
        assert D.tail_risk_host(eq, None, nb, LEVELS).quantiles.tobytes() == qs.tobytes()
        lanes += S * P
    assert lanes == {"sma": 960, "ema_ols": 768, "boll": 1656}[strategy]


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_the_ragged_rows(strategy):
    grid, series, curves = R.ragged_curves(strategy)
    assert [len(s[2]) for s in series][:2] == [1, 2]
    for window in (None, (1, 64), (65, 1000), (700, 701)):
        for held in (False, True):
            recs, qs = R.lanes_tail(curves, window, held)
            got = _host(curves, window, held)
            R.assert_same(got.lanes, recs, f"{strategy} ragged rows, window {window}, held={held}: records")
            R.assert_same(got.quantiles, qs, f"{strategy} ragged rows, window {window}, held={held}: quantiles")
    # the 1-bar row: one counted bar with d = 0 in all-bars mode, none in held mode
    recs, qs = R.lanes_tail(curves[:grid.n_params], None, False)
    assert (recs["n"] == 1).all() and (qs["k"] == 1).all() and not qs["var"].any() and (recs["min_bar"] == 0).all()
    recs, qs = R.lanes_tail(curves[:grid.n_params], None, True)
    zero = np.zeros((), D.TAIL_DTYPE)
    zero["min_bar"] = zero["max_bar"] = -1
    zero["n_window"] = 1
    assert all(x.tobytes() == zero.tobytes() for x in recs) and not qs.tobytes().strip(b"\0")


@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_host_equals_the_reference_on_family_a(name):
    """Increments up to 2^30: the top key byte on real walks."""
    grid, series, curves = R.family_a_curves(name)
    for held in (False, True):
        for window in (None, (3, 40)):
            recs, qs = R.lanes_tail(curves, window, held)
            got = _host(curves, window, held)
            R.assert_same(got.lanes, recs, f"family A {name}, window {window}, held={held}: records")
            R.assert_same(got.quantiles, qs, f"family A {name}, window {window}, held={held}: quantiles")
    if name != "ema_ols":
        assert max(int(x) for x in recs["max_d"]) >= 2**29


# ------------------------------------------------- (b) the cases reach the shapes that matter
# counted on the default seeds for sma / ema_ols / boll: lanes; lanes without a held bar; lanes with
# at least 1,000 held bars; all-bars mode at 50,000 ppm: lanes with var != 0, lanes whose k has an
# equal value on both sides in the sorted row; held mode at 50,000 ppm: lanes with var != 0, lanes
# with var != 0 and a second bar at var
COUNTED = {"sma": (960, 506, 100, 229, 630, 293, 86), "ema_ols": (768, 633, 9, 110, 546, 130, 4),
           "boll": (1656, 648, 12, 724, 861, 1008, 420)}


def _floor(x):
    return x // 2 if x >= 10 else 1


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_cases_reach_what_the_selection_can_get_wrong(strategy):
    lanes = noheld = big = v0 = inside = hv0 = htie = 0
    top = 0
    for seed in SEEDS:
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        for s in range(len(c.series)):
            for p in range(c.grid.n_params):
                pos, eq = r.curves[s][p]
                every, held = R.counted(pos, eq)[0], R.counted(pos, eq, None, True)[0]
                lanes += 1
                noheld += not held
                big += len(held) >= 1000
                top = max(top, max(abs(d) for _, d in every))
                srt = sorted(d for _, d in every)
                k = -(-len(srt) * 50_000 // 10**6)
                v0 += srt[k - 1] != 0
                inside += 2 <= k < len(srt) and srt[k - 2] == srt[k - 1] == srt[k]
                if held:
                    srt = sorted(d for _, d in held)
                    var = srt[-(-len(srt) * 50_000 // 10**6) - 1]
                    hv0 += var != 0
                    htie += var != 0 and srt.count(var) >= 2
    got = (lanes, noheld, big, v0, inside, hv0, htie)
    print(strategy, got, top)
    assert lanes == COUNTED[strategy][0]
    assert all(g >= _floor(w) for g, w in zip(got[1:], COUNTED[strategy][1:])), (got, COUNTED[strategy])
    # the random cases never touch the top key byte: the crafted rows of the GPU file and family A do
    assert top < 2**22


# ----------------------------------------------------------------------------- (c) refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    eq = np.array([[0, 5, -2]], np.int64)
    ps = np.array([[1, 1, 0]], np.int8)
    nb = np.array([3], np.int32)
    lv = np.array([1, 500_000], np.int32)
    recs, qs = np.zeros(1, D.TAIL_DTYPE), np.zeros(2, D.TAIL_Q_DTYPE)
    host = E.sym("bt_tail_host")

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(1, eq.ctypes.data, ps.ctypes.data, nb.ctypes.data, 3, 0, 0, 0, 2, lv.ctypes.data, recs.ctypes.data,
                    qs.ctypes.data) == 0
        assert (int(recs[0]["n"]), int(recs[0]["s1"]), int(recs[0]["min_d"]), int(recs[0]["min_bar"])) == (3, -2, -7, 2)
        assert qs["var"].tolist() == [-7, 0] and qs["es_sum"].tolist() == [-7, -7] and qs["k"].tolist() == [1, 2]

    keep = []

    def levels(*v):
        keep.append(np.array(v, np.int32))
        return keep[-1].ctypes.data

    q, p, b, l2, r, o = eq.ctypes.data, ps.ctypes.data, nb.ctypes.data, lv.ctypes.data, recs.ctypes.data, qs.ctypes.data
    wild = np.array([[0, 1 << 31, 0]], np.int64)
    long_ = np.array([4], np.int32)
    for args, named in (
        ((-1, q, p, b, 3, 0, 0, 0, 2, l2, r, o), r"bt_tail_host: n = -1 is negative"),
        ((1, q, p, b, 3, 0, 0, 0, 0, l2, r, o), r"Q = 0 outside \[1, 8\]"),
        ((1, q, p, b, 3, 0, 0, 0, 9, l2, r, o), r"Q = 9 outside \[1, 8\]"),
        ((1, q, p, b, 3, 0, 0, 0, 2, None, r, o), r"alpha_ppm is NULL"),
        ((1, q, p, b, 3, 0, 0, 0, 2, levels(1, 0), r, o), r"level 1: alpha_ppm = 0 outside \[1, 1000000\]"),
        ((1, q, p, b, 3, 0, 0, 0, 2, levels(1_000_001, 5), r, o), r"level 0: alpha_ppm = 1000001 outside \[1, 1000000\]"),
        ((1, q, p, b, 3, 0, 0, 2, 2, l2, r, o), r"mode = 2 is neither BT_TAIL_ALL \(0\) nor BT_TAIL_HELD \(1\)"),
        ((1, q, p, b, 3, -1, 2, 0, 2, l2, r, o), r"window \[-1, 2\) is empty or negative"),
        ((1, q, p, b, 3, 2, 2, 0, 2, l2, r, o), r"window \[2, 2\) is empty or negative"),
        ((1, q, p, b, 3, 0, 0, 0, 2, l2, None, None), r"recs_out and q_out are both NULL"),
        ((1, None, p, b, 3, 0, 0, 0, 2, l2, r, o), r"equity and n_bars are required"),
        ((1, q, p, long_.ctypes.data, 3, 0, 0, 0, 2, l2, r, o), r"n_bars = 4 outside \[0, stride = 3\] \(lane 0\)"),
        ((1, q, None, b, 3, 0, 0, 1, 2, l2, r, o), r"pos is required with mode BT_TAIL_HELD"),
        ((1, wild.ctypes.data, p, b, 3, 0, 0, 0, 2, l2, r, o), r"increment 2147483648 at bar 1 of lane 0 outside the domain"),
    ):
        assert host(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    for name, args in (("bt_tail", (None, 0, None, 0, 0, 0, 2, l2, r, o)), ("bt_tail_of", (None, 1, 3, q, 2, l2, r, o)),
                       ("bt_set_tail_row", (None, 0)), ("bt_set_tail_budget", (None, 0)), ("bt_last_tail_row", (None,))):
        assert E.sym(name)(*args) == -1
        assert re.search(rf"{name}: null engine", last()), last()
    still_good()
    with pytest.raises(ValueError, match="fractions"):
        D.tail.as_levels_ppm(["a"])
    with pytest.raises(ValueError, match="int32"):
        D.tail.as_levels_ppm([1 << 40])
    assert D.tail.as_levels_ppm((0.01, 0.05, 50_000, 1.0, 0.0000014)).tolist() == [10_000, 50_000, 50_000, 1_000_000, 1]
    with pytest.raises(D.BtError, match=r"Q = 0 outside \[1, 8\]"):
        D.tail_risk_host(eq, ps, nb, ())


# the rules of the calls in the order they check them (tail_refusal, tail_of_refusal), and the two
# refusals of the plan, as the driver prints them
RULES = ("no dataset loaded", "n = 0 outside [1, 1048576]", "n = 1048577 outside [1, 1048576]",
         "n = 3 with lanes == NULL (all-lanes mode takes n = 0)", "Q = 0 outside [1, 8]", "alpha_ppm is NULL",
         "level 1: alpha_ppm = 0 outside [1, 1000000]", "mode = 7 is neither BT_TAIL_ALL (0) nor BT_TAIL_HELD (1)",
         "window [5, 3) is empty or negative (0, 0 is the whole row)", "recs_out and q_out are both NULL",
         "T = 4194305 bars of the longest row exceed 4194304", "", "",
         "n = 0 outside [1, 1048576]", "T = 0 outside [1, 4194304]", "T = 4194305 outside [1, 4194304]", "d is NULL",
         "Q = 9 outside [1, 8]", "recs_out and q_out are both NULL", "",
         "a row of 14081 counted bars (56324 bytes) does not fit the 56320 bytes of LDS a workgroup keeps for it",
         "the staging of one dataset row (6656 bytes) exceeds the budget of 2000 bytes",
         "the staging of one lane (1600 bytes) exceeds the budget of 100 bytes")
REFUSED = ("n = -1 ", "Q = 0 ", "Q = 9 ", "alpha_ppm is NULL", "level 1: alpha_ppm = 0", "level 0: alpha_ppm = 1000001",
           "mode = 2 ", "window [-1, 2)", "window [2, 2)", "both NULL", "equity and n_bars are required", "n_bars = 4 ",
           "pos is required", "increment 2147483648 at bar 1 of lane 0")


# ------------------------------------------------------------------------------------ layout
def test_record_layouts_match_the_c99_host(tmp_path):
    """The two records' mirror (tail.py TAIL_RECORDS) has the header's sizes and offsets, field by
    field, and every struct a bt_tail* entry point takes is one of them (or of the engine's)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "tail_abi_host")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "tail_abi_host.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("abi_version") == 3 == D.ABI_VERSION
    assert (got.pop("tail_max"), got.pop("levels_max"), got.pop("ppm_max"), got.pop("bars_max")) == \
        (D.TAIL_MAX, D.TAIL_LEVELS_MAX, D.TAIL_PPM_MAX, D.TAIL_BARS_MAX) == (1 << 20, 8, 10**6, 1 << 22)
    assert (got.pop("all"), got.pop("held")) == (D.TAIL_ALL, D.TAIL_HELD) == (0, 1)
    assert got.pop("s4_bytes") == 24 == D.TAIL_DTYPE["s4"].itemsize
    assert list(D.TAIL_RECORDS) == ["bt_tail_rec", "bt_tail_q"]
    assert D.TAIL_DTYPE.itemsize == 128 and D.TAIL_Q_DTYPE.itemsize == 24
    for cname, dt in D.TAIL_RECORDS.items():
        assert got.pop(cname) == dt.itemsize, cname
        for f in dt.names:
            assert got.pop(f"{cname}.{f}") == dt.fields[f][1], f"{cname}.{f}"
    assert not got, f"fields the mirror lacks: {sorted(got)}"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bt.h")).read(), flags=re.S)
    protos = re.findall(r"\b(bt_(?:set_|last_)?tail[a-z0-9_]*)\s*\(([^()]*)\)\s*;", hdr)
    names = ["bt_last_tail_row", "bt_set_tail_budget", "bt_set_tail_row", "bt_tail", "bt_tail_host", "bt_tail_of"]
    assert sorted(n for n, _ in protos) == names
    taken = {t for _, args in protos for t in re.findall(r"\b(bt_\w+)\s*\*", args)}
    assert taken - {"bt_engine", "bt_lane"} == set(D.TAIL_RECORDS)
    # engine.py names none of the entry points (tests/test_abi_cpu.py reads it for the calls it checks)
    binding = open(E.__file__).read()
    for name in names:
        assert not re.search(rf"\b{name}\b", binding), name
        assert E.sym(name) is not None


# ------------------------------------------------------------------------------ (d) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("tail_plan_driver")

    def run(units, P, Q_, list_mode=0, staged=0, longest=2520, cus=256, row=0, budget=0):
        return run_driver(exe, units, P, Q_, int(list_mode), int(staged), longest, cus, row, budget)
    return run


BUDGET = 256 << 20
# name: (units, P, Q, list mode, staged, longest_n, row_req, budget_req)
PLAN_SHAPES = {
    "config2": (5000, 400, 3, 0, 0, 2520, 0, 0), "config2_arena": (5000, 400, 3, 0, 0, 2520, 2, 0),
    "minute_list": (64, 400, 3, 1, 0, 491_400, 0, 0), "one": (1, 1, 1, 0, 0, 1, 0, 0),
    "empty_window": (3, 7, 8, 0, 0, 0, 2, 0), "longest_row_of": (1, 1, 8, 0, 1, 1 << 22, 0, 0),
    "longest_row_list": (2, 9, 8, 1, 0, 1 << 22, 0, 0), "staged_small": (300, 1, 2, 0, 1, 129, 0, 0),
    "one_row_chunks": (6, 36, 8, 0, 0, 1500, 0, R.rows_budget(36, 8, 0, 1)),
    "one_row_chunks_arena": (6, 36, 8, 0, 0, 1500, 2, R.rows_budget(36, 8, 1536, 1)),
    "list_small_budget": (1000, 7, 5, 1, 0, 700, 2, 40_000), "list_max": (1 << 20, 400, 2, 1, 0, 2520, 0, 0),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_tail_covers_every_unit_once_within_the_budget(plan, name):
    units, P, Q_, lst, staged, longest, row, req = PLAN_SHAPES[name]
    pl = plan(units, P, Q_, lst, staged, longest, 256, row, req)
    assert pl == plan(units, P, Q_, lst, staged, longest, 256, row, req), "the plan is a function of its arguments"
    assert (pl["budget"], pl["rec_bytes"], pl["q_bytes"], pl["lane_bytes"]) == (BUDGET, 128, 24, 16)
    assert (pl["list"], pl["staged"], pl["Q"], pl["block"]) == (lst, staged, Q_, 256)
    cap = pl["lds_row_cap"]
    assert cap == (pl["lds_cap_bytes"] - pl["fixed_bytes"]) // 4 and pl["lds_cap_bytes"] == 64 * 1024
    assert pl["fixed_bytes"] >= 8 * 256 * 4 and pl["fixed_bytes"] % 16 == 0
    home = 2 if row == 2 or longest > cap else 1
    assert pl["row_mode"] == home and not pl["row_refused"]
    assert pl["lds_bytes"] == pl["fixed_bytes"] + (4 * longest if home == 1 else 0) <= pl["lds_cap_bytes"]
    pitch = pl["pitch"]
    assert pitch == (max(-(-longest // 64) * 64, 64) if home == 2 or staged else 0) and pitch % 64 == 0
    lanes_per = 1 if lst or staged else P
    per = pl["per_chunk"]
    assert 1 <= per <= units and per * lanes_per <= 1 << 30
    lane = 128 + Q_ * 24 + pitch * 4
    assert pl["unit_bytes"] == lanes_per * lane + (16 if lst else 0)
    regions = [(pl["o_levels"], Q_ * 4), (pl["o_lanes"], per * 16 if lst else 0), (pl["o_rec"], per * lanes_per * 128),
               (pl["o_q"], per * lanes_per * Q_ * 24), (pl["o_rows"], per * lanes_per * pitch * 4)]
    assert_staging_layout(regions, pl["staging_bytes"], name)
    budget = req or BUDGET
    assert pl["staging_bytes"] <= budget and pl["need_bytes"] <= budget
    # as many units as fit: one more would pass the budget (or there is no more)
    assert per == units or pl["o_levels"] + 256 + 4 * 256 + (per + 1) * pl["unit_bytes"] > budget
    assert pl["chunks"] == -(-units // per)
    rows = pl["units"]
    assert rows[0][0] == 0 and rows[-1][1] == units
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:]) if pl["chunks"] <= 8), "chunks are contiguous"
    assert all(0 < r1 - r0 <= per for r0, r1 in rows)


def test_plan_tail_on_the_shapes_of_the_call(plan):
    c2 = plan(5000, 400, 3, longest=2520)          # the config-2 shard: rows in LDS, 400 MB of records in two chunks
    assert c2["row_mode"] == 1 and c2["pitch"] == 0 and c2["chunks"] == 2 and c2["lds_bytes"] == c2["fixed_bytes"] + 10080
    assert 2 * c2["lds_bytes"] <= 160 * 1024, "two workgroups per CU"
    m = plan(64, 400, 3, 1, 0, 491_400)            # minute rows: the arena
    assert m["row_mode"] == 2 and m["pitch"] == 491_456 and m["chunks"] == 1 and m["lds_bytes"] == m["fixed_bytes"]
    # one lane always fits the default budget at T = 2^22
    for lst, staged in ((1, 0), (0, 1)):
        big = plan(3, 1, 8, lst, staged, 1 << 22)
        assert big["row_mode"] == 2 and big["per_chunk"] == 3 and big["need_bytes"] < BUDGET // 8
    # the row's home flips exactly at the LDS capacity
    cap = c2["lds_row_cap"]
    assert cap >= 2520 and cap < 491_400
    for staged in (0, 1):
        assert plan(1, 1, 1, 0, staged, cap)["row_mode"] == 1 and plan(1, 1, 1, 0, staged, cap + 1)["row_mode"] == 2
        assert plan(1, 1, 1, 0, staged, cap)["lds_bytes"] == 64 * 1024
    # row_req is honoured or refused
    assert plan(1, 1, 1, longest=cap, row=2)["row_mode"] == 2 and plan(1, 1, 1, longest=cap, row=1)["row_mode"] == 1
    over = plan(1, 1, 1, longest=cap + 1, row=1)
    assert over["row_refused"] == 1 and over["row_mode"] == 2
    assert plan(1, 1, 1, longest=cap + 1, row=2)["row_refused"] == 0
    # exactly one unit per chunk under rows_budget, in both homes and in list mode
    assert plan(6, 36, 8, longest=1500, budget=R.rows_budget(36, 8, 0, 1))["chunks"] == 6
    assert plan(6, 36, 8, longest=1500, budget=R.rows_budget(36, 8, 0, 2))["chunks"] == 3
    assert plan(6, 36, 8, longest=1500, row=2, budget=R.rows_budget(36, 8, 1536, 1))["chunks"] == 6
    assert plan(50, 36, 8, 1, longest=1500, budget=R.rows_budget(1, 8, 0, 1, True))["chunks"] == 50
    assert plan(50, 36, 8, 1, longest=1500, row=2, budget=R.rows_budget(1, 8, 1536, 1, True))["chunks"] == 50
    # one unit that cannot fit: the plan says so with per_chunk 0 and the call is refused
    for args in ((3, 400, 8, 0, 0, 2520, 256, 0, 2000), (5, 7, 8, 1, 0, 1 << 22, 256, 0, 1 << 20)):
        pl = plan(*args)
        assert pl["per_chunk"] == 0 and pl["chunks"] == 0 and pl["staging_bytes"] == 0 and pl["need_bytes"] > args[-1]


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("tail_plan_driver", sanitize=True)
    for name in ("one_row_chunks_arena", "list_small_budget", "longest_row_of"):
        units, P, Q_, lst, staged, longest, row, req = PLAN_SHAPES[name]
        assert run_driver(exe, units, P, Q_, lst, staged, longest, 256, row, req, sanitized=True) == \
            run_driver(build_plan_driver("tail_plan_driver"), units, P, Q_, lst, staged, longest, 256, row, req)


# ---------------------------------------------------------------------- (e) under the sanitizers
def test_planner_and_host_code_under_asan_and_ubsan(tmp_path):
    """tests/asan/tail_driver.cpp with csrc/tail.cpp and csrc/plan.cpp: a program of its own, built
    with the sanitizers and run directly."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    exe = str(tmp_path / "tail_asan")
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *SANITIZE, "-x", "hip",
                        "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "tail_driver.cpp"), os.path.join(CSRC, "tail.cpp"),
                        os.path.join(CSRC, "plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lv = np.array(LEVELS, np.int32)
    for strategy, seed, held, cut in (("sma", 0, False, False), ("ema_ols", 1, True, True), ("boll", 2, True, False)):
        c, rf = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        recs, qs, window = R.random_refs(strategy, seed, held, cut)
        S, P = recs.shape
        eq, ps, nb = R.as_curve_arrays([rf.curves[s][p] for s in range(S) for p in range(P)])
        fin, fout = str(tmp_path / f"in_{strategy}"), str(tmp_path / f"out_{strategy}")
        frm, to = window or (0, 0)
        with open(fin, "wb") as f:
            f.write(np.array([S * P, eq.shape[1], frm, to, int(held), Q], np.int32).tobytes() + lv.tobytes() + nb.tobytes()
                    + eq.tobytes() + ps.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=SANITIZE_ENV, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        nr = S * P * 128
        assert len(raw) == nr + S * P * Q * 24
        R.assert_same(np.frombuffer(raw[:nr], D.TAIL_DTYPE).reshape(S, P), recs, f"{strategy}: records")
        R.assert_same(np.frombuffer(raw[nr:], D.TAIL_Q_DTYPE).reshape(S, P, Q), qs, f"{strategy}: quantiles")
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {S * P} {Q}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == len(REFUSED)
        for ln, named in zip(refused, REFUSED):
            assert named in ln, (ln, named)
        assert [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")] == list(RULES)
        assert [ln for ln in lines if ln.startswith("longest: ")] == ["longest: 700 10 690 0"]
        plans = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("plan: ")]
        assert [p[:3] for p in plans] == [(1, S * P, 1), (1, S * P, 1), (2, S * P, 1), (2, min(S * P, 15), -(-S * P // 15))]


# ------------------------------------------------------------------------- (f) derived views
def _risk(d, levels=(0.05,)):
    recs, qs = R.rows_tail(d, D.tail.as_levels_ppm(levels).tolist())
    return D.TailRisk(D.tail.as_levels_ppm(levels), recs, qs)


def test_derived_views_equal_their_restatement():
    rng = np.random.default_rng(0x7A13)
    d = [rng.integers(-3000, 3500, 400), rng.integers(-(2**31) + 1, 2**31, 400), np.arange(400) - 100,
         np.where(np.arange(400) % 7 == 0, -900, 35)]
    tr = _risk(np.array(d, np.int64), (0.01, 0.05, 1.0))
    want = [R.views(r, 252) for r in tr.lanes]
    assert tr.mean().tolist() == [w["mean"] for w in want] and tr.std().tolist() == [w["std"] for w in want]
    assert tr.skew().tolist() == [w["skew"] for w in want] and tr.kurtosis().tolist() == [w["kurtosis"] for w in want]
    assert tr.sharpe(252).tolist() == [w["sharpe"] for w in want]
    assert tr.sortino(252).tolist() == [w["sortino"] for w in want]
    assert tr.gain_to_pain().tolist() == [w["gain_to_pain"] for w in want]
    assert tr.sharpe().tolist() == [R.views(r)["sharpe"] for r in tr.lanes]
    assert all(type(x) is int for x in tr.s2.tolist() + tr.s3.tolist() + tr.s4.tolist() + tr.s2_neg.tolist())
    assert tr.s4.tolist() == [sum(int(x) ** 4 for x in row) for row in d] and tr.s3.tolist() == [sum(int(x) ** 3 for x in row) for row in d]
    # numpy's own moments agree to rounding on the small row
    x = np.array(d[0], np.float64)
    assert math.isclose(tr.std()[0], x.std(), rel_tol=1e-12) and math.isclose(tr.mean()[0], x.mean(), rel_tol=1e-12)
    m = x - x.mean()
    assert math.isclose(tr.skew()[0], (m**3).mean() / x.std()**3, rel_tol=1e-9)
    assert math.isclose(tr.kurtosis()[0], (m**4).mean() / x.std()**4, rel_tol=1e-9)
    for j in range(3):
        q = tr.quantiles[:, j]
        assert tr.var(j).tolist() == [-float(v) for v in q["var"]] and tr.es(j).tolist() == [-int(s) / int(k) for s, k in zip(q["es_sum"], q["k"])]
    assert tr.es(2).tolist() == [-w["mean"] for w in want]          # alpha = 1: the mean of every bar
    for got, rec in zip(tr.psr(0.01).tolist(), tr.lanes):
        assert math.isclose(got, R.psr(rec, 0.01), rel_tol=1e-12)
    V = 0.0004
    for got, rec in zip(tr.deflated_sharpe(n_trials=50, sr_var=V).tolist(), tr.lanes):
        assert math.isclose(got, R.psr(rec, R.dsr_threshold(V, 50)), rel_tol=1e-12)
    with pytest.raises(ValueError, match="required in list mode"):
        tr.deflated_sharpe()
    # all-lanes shape: the defaults are per symbol, N = P and V the variance of the row's Sharpes
    grid = D.TailRisk(tr.levels_ppm, tr.lanes.reshape(2, 2), tr.quantiles.reshape(2, 2, 3))
    sr = grid.sharpe(1)
    for s in range(2):
        V = sum((x - sum(sr[s]) / 2) ** 2 for x in sr[s].tolist()) / 2
        for p in range(2):
            assert math.isclose(grid.deflated_sharpe()[s, p], R.psr(grid.lanes[s, p], R.dsr_threshold(V, 2)), rel_tol=1e-12)


def test_psr_on_symmetric_rows_of_known_kurtosis():
    """-a, 0, a with weights 1 : 4 : 1 has skew 0 and kurtosis 3 around its mean; shifted by c the
    central moments stay. With skew 0 the radicand of psr is 1 + (kurtosis - 1) / 4 SR^2: at
    kurtosis 3 psr(0) is Phi(SR sqrt(n - 1) / sqrt(1 + SR^2 / 2)), the normal case, and on the
    two-point row -a, a (kurtosis 1) it is Phi(SR sqrt(n - 1)) itself."""
    row = np.array([-600] * 50 + [0] * 200 + [600] * 50, np.int64) + 7
    tr = _risk(row[None])
    assert tr.skew()[0] == 0.0 and tr.kurtosis()[0] == 3.0
    sr = float(tr.sharpe(1)[0])
    assert sr > 0
    assert math.isclose(tr.psr(0.0)[0], R.phi(sr * math.sqrt(len(row) - 1) / math.sqrt(1.0 + 0.5 * sr * sr)), rel_tol=1e-12)
    two = np.array([-600, 600] * 150, np.int64) + 7
    tr = _risk(two[None])
    assert tr.skew()[0] == 0.0 and tr.kurtosis()[0] == 1.0
    sr = float(tr.sharpe(1)[0])
    assert sr > 0 and math.isclose(tr.psr(0.0)[0], R.phi(sr * math.sqrt(len(two) - 1)), rel_tol=1e-12)
    assert math.isclose(tr.psr(sr)[0], 0.5, rel_tol=1e-12)


def test_derived_views_are_zero_where_the_denominator_is():
    for d in (np.zeros((1, 40), np.int64), np.array([[5]]), np.array([[0]])):
        tr = _risk(d)
        for v in (tr.std(), tr.skew(), tr.kurtosis(), tr.sharpe(252), tr.sortino(252), tr.gain_to_pain(), tr.psr(),
                  tr.deflated_sharpe(10, 0.01)):
            assert v.tolist() == [0.0]
    empty = D.TailRisk(np.array([50_000], np.int32), np.zeros(1, D.TAIL_DTYPE), np.zeros((1, 1), D.TAIL_Q_DTYPE))
    for v in (empty.mean(), empty.std(), empty.skew(), empty.kurtosis(), empty.sharpe(), empty.sortino(),
              empty.gain_to_pain(), empty.var(0), empty.es(0), empty.psr(), empty.deflated_sharpe(10, 0.01)):
        assert v.tolist() == [0.0]
    assert _risk(np.array([[5]])).mean().tolist() == [5.0]
