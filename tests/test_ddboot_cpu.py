"""The drawdown bootstrap, the parts that need no GPU (docs/drawdown_spec.md): bt_drawdown_boot_host
against the Python-int reference of ddboot_ref.py on every case the GPU tests use; proof from the
reference alone that the cases reach the shapes the kernel can get wrong; the record layout
(tests/ddboot_abi_host.c); the chunk planner (plan_ddboot through tests/plan/ddboot_plan_driver.cpp);
planner and host code as a stand-alone program under AddressSanitizer and UBSan
(tests/asan/ddboot_driver.cpp); and the derived views of DrawdownRisk against their restatement."""
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
import bootstrap_ref as BR
import ddboot_ref as R
import random_cases as RC
from helpers import CSRC, SANITIZE, SANITIZE_ENV, assert_staging_layout, build_plan_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS, LIMITS = R.LEVELS, R.LIMITS
Q, NR = len(LEVELS), len(LIMITS)
SOURCES = ("ddboot.cpp", "bootstrap.cpp", "plan.cpp")   # ddboot.cpp takes the window rule from bootstrap.cpp


def _host_rows(d, B, L, seed, levels=LEVELS, limits=LIMITS, window=None):
    """bt_drawdown_boot_host on rows of increments: their running sums are the equity rows."""
    d = np.asarray(d, np.int64)
    return D.drawdown_risk_host(np.cumsum(d, axis=1), [d.shape[1]] * len(d), B, L, seed, window, levels, limits, raw=True)


def _host_curves(curves, bars, B, L, seed, window):
    stride = max(bars)
    eq = np.zeros((len(curves), stride), np.int64)
    for i, c in enumerate(curves):
        eq[i, :len(c)] = c
    return D.drawdown_risk_host(eq, bars, B, L, seed, window, LEVELS, LIMITS, raw=True)


# ------------------------------------------------------------ (a) the host code to the reference
@pytest.mark.parametrize("T", R.OF_T)
def test_host_equals_the_reference_on_the_staged_shapes(T):
    for k, (L, B, n, seed) in enumerate(R.of_cases(T)):
        R.assert_same(_host_rows(R.of_rows(T, n), B, L, seed), R.of_ref(T, k), f"T = {T}, L = {L}, B = {B}, n = {n}")


def test_host_equals_the_reference_on_the_crafted_rows():
    for name, (rows, B, L, seed) in R.crafted().items():
        R.assert_same(_host_rows(rows, B, L, seed), R.drawdown_risk(rows.tolist(), B, L, seed), name)


def test_host_equals_the_reference_at_the_largest_increments():
    T, B, L = 4096, 64, 33
    alt = np.where(np.arange(T) % 2 == 0, -R.BIG, R.BIG)
    for rows in (np.stack([np.full(T, R.BIG), np.full(T, -R.BIG)]), np.stack([alt, -alt])):
        R.assert_same(_host_rows(rows, B, L, 0xB16), R.drawdown_risk(rows.tolist(), B, L, 0xB16), "T = 4096")


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_the_random_cases(strategy):
    for seed in range(8):
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        S, P = len(c.series), c.grid.n_params
        B, L, sd = R.walk_params(strategy, seed)
        curves = [r.curves[s][p][1] for s in range(S) for p in range(P)]
        bars = [c.bars[s] for s in range(S) for _ in range(P)]
        for cut in (False, True):
            want, window = R.walk_ref(strategy, seed, cut)
            R.assert_same(_host_curves(curves, bars, B, L, sd, window), want, f"{strategy} seed {seed}, window {window}")
        every, _ = R.walk_ref(strategy, seed)
        assert np.array_equal(every.lanes["mdd"], r.summaries["mdd"].reshape(-1)), "the observed drawdown is the run's"
        assert np.array_equal(every.lanes["sum"], r.summaries["pnl"].reshape(-1))


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_the_window_edges(strategy):
    c = BR.edge_case(strategy)
    for frm, to in R.EDGE_WINDOWS:
        got = _host_curves(c.curves, [len(x) for x in c.curves], R.EDGE.B, R.EDGE.L, R.EDGE.seed + 1000 * frm + to, (frm, to))
        R.assert_same(got, R.edge_ref(strategy, frm, to), f"{strategy}, window [{frm}, {to})")


def test_the_numpy_walk_is_the_python_int_walk():
    d = R.of_rows(65, 3).tolist()
    plan = BR.bar_plan(65, 20, 7, 5)
    assert R.resampled_mdd(d, plan) == R.resampled_mdd(d, plan, exact=True)
    assert R.mdd([3, -5, 2, -4, 6, 1, -7, 2]) == 7 and R.mdd([]) == 0 and R.mdd([5, 5]) == 0 and R.mdd([-1, -1]) == 2


# ------------------------------------------------- (b) the cases reach what the kernel can get wrong
def test_cases_reach_what_the_kernel_can_get_wrong():
    """Conditions on the reference alone: were one of them not met, the GPU tests would pass on a
    kernel that is wrong there."""
    seen = dict(cross=0, single=0, wrapping=0)
    shapes = set()
    for name, (rows, B, L, seed) in R.crafted().items():
        a = R.anatomy(rows.tolist(), min(B, 64), L, seed)
        for k in seen:
            seen[k] += a[k]
        shapes.add((a["K"] == 1, a["last_differs"]))
        if name in ("dip", "dip_31"):
            assert a["cross"] > 0 and a["single"] > 0, f"{name}: the dip is cut by a block edge in some resamples only"
    assert min(seen.values()) > 0, seen
    assert R.anatomy(R.crafted()["dip_31"][0].tolist(), 64, 31, 5)["wrapping"] > 0, "a wrapping block holds the whole dip"
    for T in R.OF_T:
        for L, B, n, seed in R.of_cases(T):
            lens = BR.blocks(T, L)
            shapes.add((len(lens) == 1, lens[-1] != lens[0]))
    assert shapes == {(True, False), (False, False), (False, True)}, "K = 1, last_len = L' and last_len != L'"
    # both ways of building a table
    plan = build_plan_driver("ddboot_plan_driver")
    built = {run_driver(plan, n, T, B, L, Q, NR, 0, 1, 1, 256, 0, 0)[k] for T in R.OF_T for L, B, n, _ in R.of_cases(T)
             for k in ("scan1", "scan2")}
    assert built == {0, 1}, "a thread per chunk and a wave per chunk"
    # ties at a level, and n_ge at both ends and between
    nge, tied = set(), False
    for T in R.OF_T:
        for k, (L, B, n, seed) in enumerate(R.of_cases(T)):
            ref = R.of_ref(T, k)
            nge |= {"none" if g == 0 else "all" if g == B else "some" for g in ref.lanes["n_ge"].tolist()}
            for i in range(n):
                s = sorted(ref.raw[i].tolist())
                for a in LEVELS:
                    kk = R.rank(B, a)
                    tied |= 1 < kk < B and s[kk - 2] == s[kk - 1] == s[kk]
    for name, (rows, B, L, seed) in R.crafted().items():
        ref = R.drawdown_risk(rows.tolist(), B, L, seed)
        nge |= {"none" if g == 0 else "all" if g == B else "some" for g in ref.lanes["n_ge"].tolist()}
    assert tied and nge == {"none", "all", "some"}, (tied, nge)


# ------------------------------------------------------------------------------------ layout
def test_record_layout_matches_the_c99_host(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "ddboot_abi_host")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "ddboot_abi_host.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("abi_version") == 3 == D.ABI_VERSION
    assert (got.pop("levels_max"), got.pop("limits_max")) == (D.DD_LEVELS_MAX, D.DD_LIMITS_MAX) == (8, 8)
    assert (got.pop("lanes_max"), got.pop("resamples_max")) == (E.BOOT_MAX, E.BOOT_MAX_RESAMPLES) == (1 << 20, 65536)
    assert list(D.DD_RECORDS) == ["bt_dd_lane"] and D.DD_LANE_DTYPE.itemsize == 72
    for cname, dt in D.DD_RECORDS.items():
        assert got.pop(cname) == dt.itemsize, cname
        for f in dt.names:
            assert got.pop(f"{cname}.{f}") == dt.fields[f][1], f"{cname}.{f}"
    assert not got, f"fields the mirror lacks: {sorted(got)}"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bt.h")).read(), flags=re.S)
    protos = re.findall(r"\b(bt_(?:drawdown_boot|set_ddboot|last_ddboot)[a-z0-9_]*)\s*\(([^()]*)\)\s*;", hdr)
    names = ["bt_drawdown_boot", "bt_drawdown_boot_host", "bt_drawdown_boot_of", "bt_last_ddboot_row", "bt_set_ddboot_budget",
             "bt_set_ddboot_row"]
    assert sorted(n for n, _ in protos) == names
    taken = {t for _, args in protos for t in re.findall(r"\b(bt_\w+)\s*\*", args)}
    assert taken - {"bt_engine", "bt_lane"} == set(D.DD_RECORDS)
    binding = open(E.__file__).read()
    for name in names:
        assert not re.search(rf"\b{name}\b", binding), name
        assert E.sym(name) is not None


# ------------------------------------------------------------------------------ (d) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("ddboot_plan_driver")

    def run(n, T, B, L, Q_=2, R_=0, lst=0, staged=0, raw=0, cus=256, row=0, budget=0):
        return run_driver(exe, n, T, B, L, Q_, R_, int(lst), int(staged), int(raw), cus, row, budget)
    return run


BUDGET = 256 << 20
# name: (n, T, B, L, Q, R, list mode, staged, raw, row_req, budget_req)
PLAN_SHAPES = {
    "config2": (2_000_000, 2520, 1000, 10, 2, 0, 0, 0, 0, 0, 0), "config2_lds": (2_000_000, 2520, 1000, 10, 2, 0, 0, 0, 0, 1, 0),
    "best_per_symbol": (5000, 2520, 1000, 10, 2, 3, 1, 0, 1, 0, 0), "one": (1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0),
    "two_tables": (300, 129, 257, 65, 8, 8, 0, 1, 1, 0, 0), "small_arena": (300, 129, 257, 65, 8, 8, 1, 0, 0, 2, 0),
    "longest_row": (2, 1 << 22, 64, 4096, 2, 2, 0, 1, 0, 0, 0), "most_resamples": (2, 8, 65_536, 3, 6, 4, 0, 1, 0, 0, 0),
    "one_lane_chunks": (7, 700, 40, 33, 4, 4, 1, 0, 1, 0, R.one_lane_budget(700, 40, 33, 4, 4, True, True, 1, False)),
    "one_lane_chunks_arena": (7, 700, 40, 33, 4, 4, 0, 0, 0, 2, R.one_lane_budget(700, 40, 33, 4, 4, False, False, 2, True)),
    "values_in_the_arena": (9, 1500, 60_000, 10, 1, 0, 0, 0, 0, 0, 0),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_ddboot_covers_every_lane_once_within_the_budget(plan, name):
    n, T, B, L, Q_, R_, lst, staged, raw, row, req = PLAN_SHAPES[name]
    pl = plan(n, T, B, L, Q_, R_, lst, staged, raw, 256, row, req)
    assert pl == plan(n, T, B, L, Q_, R_, lst, staged, raw, 256, row, req), "the plan is a function of its arguments"
    assert (pl["budget"], pl["rec_bytes"], pl["lane_bytes"], pl["entry_bytes"], pl["block"]) == (BUDGET, 72, 16, 24, 256)
    assert pl["lds_cap_bytes"] == 160 * 1024 and pl["fixed_bytes"] >= 8 * 256 * 4
    # the blocks are the reality check's
    lens = BR.blocks(T, L)
    assert (pl["T"], pl["Lp"], pl["K"], pl["last_len"]) == (T, lens[0] if len(lens) > 1 else T, len(lens), lens[-1])
    two = len(lens) > 1 and lens[-1] != lens[0]
    assert pl["two_tables"] == two
    row_bytes = (T + 1) * 8 + (2 if two else 1) * T * 24
    assert (pl["r_w1"], pl["r_w2"], pl["row_bytes"]) == ((T + 1) * 8, (T + 1) * 8 + (T * 24 if two else 0), row_bytes)
    limit = pl["lds_cap_bytes"]
    home = 2 if row == 2 or pl["fixed_bytes"] + row_bytes > limit else 1
    assert pl["row_mode"] == home and not pl["row_refused"]
    lds = pl["fixed_bytes"] + (row_bytes if home == 1 else 0)
    vals_lds = Q_ > 0 and not raw and lds + B * 8 <= limit
    assert pl["l_vals"] == (lds if vals_lds else 0) and pl["lds_bytes"] == lds + (B * 8 if vals_lds else 0) <= limit
    pitch, v_pitch = (-(-row_bytes // 256) * 256 if home == 2 else 0), (0 if raw or vals_lds or Q_ == 0 else -(-B // 32) * 32)
    d_pitch = -(-T // 64) * 64 if staged else 0
    assert (pl["pitch"], pl["v_pitch"], pl["d_pitch"]) == (pitch, v_pitch, d_pitch)
    unit = (16 if lst else 0) + 72 + Q_ * 8 + R_ * 8 + (B * 8 if raw else 0) + pitch + v_pitch * 8 + d_pitch * 4
    assert pl["unit_bytes"] == unit
    per = pl["per_chunk"]
    assert 1 <= per <= n and per <= 1 << 30
    regions = [(pl["o_starts"], len(lens) * B * 4), (pl["o_levels"], Q_ * 4), (pl["o_limits"], R_ * 8),
               (pl["o_lanes"], per * 16 if lst else 0), (pl["o_rec"], per * 72), (pl["o_q"], per * Q_ * 8),
               (pl["o_reach"], per * R_ * 8), (pl["o_raw"], per * B * 8 if raw else 0), (pl["o_rows"], per * pitch),
               (pl["o_vals"], per * v_pitch * 8), (pl["o_d"], per * d_pitch * 4)]
    assert_staging_layout(regions, pl["staging_bytes"], name)
    budget = req or BUDGET
    fixed = pl["o_lanes"] + 8 * 256
    assert pl["need_bytes"] == fixed + unit, "need_bytes is the staging of one lane per chunk"
    assert pl["staging_bytes"] <= budget and pl["need_bytes"] <= budget
    assert per == n or fixed + (per + 1) * unit > budget, "as many lanes as fit"
    assert pl["chunks"] == -(-n // per)
    rows = pl["lanes"]
    assert rows[0][0] == 0 and rows[-1][1] == n and all(0 < b - a <= per for a, b in rows)
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:]) if pl["chunks"] <= 8), "chunks are contiguous"
    assert pl["starts_block"] == 256 and pl["starts_blocks"] == -(-len(lens) * B // 256)


def test_plan_ddboot_on_the_shapes_of_the_call(plan):
    c2 = plan(2_000_000, 2520, 1000, 10)            # the config-2 shard: one table, 80 KB a row, in LDS with the values
    assert (c2["K"], c2["two_tables"], c2["row_bytes"], c2["scan1"]) == (252, 0, 2521 * 8 + 2520 * 24, 0)
    assert c2["row_mode"] == 1 and c2["l_vals"] == c2["fixed_bytes"] + c2["row_bytes"]
    assert 64 * 1024 < c2["lds_bytes"] == c2["l_vals"] + 8000 <= 160 * 1024
    arena = plan(2_000_000, 2520, 1000, 10, row=2)
    assert arena["row_mode"] == 2 and arena["l_vals"] == arena["fixed_bytes"] and arena["lds_bytes"] == arena["fixed_bytes"] + 8000
    # the row's home flips exactly where the constants say
    fixed, entry = c2["fixed_bytes"], c2["entry_bytes"]
    for L, tables in ((1, 1), (7, 2)):
        cap = (160 * 1024 - fixed - 8) // (8 + tables * entry)
        while tables == 2 and (cap % L == 0 or (cap + 1) % L == 0):    # both sizes keep a shorter last block
            cap -= 1
        if tables == 1:
            assert plan(1, cap, 4, L, 0)["row_mode"] == 1 and plan(1, cap + 1, 4, L, 0)["row_mode"] == 2
            assert plan(1, cap, 4, L, 0)["lds_bytes"] == fixed + 8 + cap * 32 <= 160 * 1024 < fixed + 8 + (cap + 1) * 32
        else:
            assert plan(1, cap, 4, L, 0)["two_tables"] == 1 and plan(1, cap, 4, L, 0)["row_mode"] == 1
            assert plan(1, 2 * cap, 4, L, 0)["row_mode"] == 2
    top = (160 * 1024 - fixed - 8) // 32
    assert plan(1, top, 4, 1, 0, row=1)["row_refused"] == 0 and plan(1, top, 4, 1, 0, row=1)["row_mode"] == 1
    over = plan(1, top + 1, 4, 1, 0, row=1)
    assert over["row_refused"] == 1 and over["row_mode"] == 2 and plan(1, top + 1, 4, 1, 0, row=2)["row_refused"] == 0
    # a long block is scanned by a wave, short blocks are walked by a thread each
    assert plan(1, 4096, 4, 4096)["scan2"] == 1 and plan(1, 4096, 4, 2048)["scan1"] == 1 and plan(1, 4096, 4, 16)["scan1"] == 0
    # one lane always fits the default budget at T = 2^22 with blocks of a tile or more
    big = plan(2, 1 << 22, 64, 4096, staged=1)
    assert big["row_mode"] == 2 and big["per_chunk"] == 1 and big["chunks"] == 2 and big["need_bytes"] < BUDGET
    # one lane that cannot fit: the plan says so with per_chunk 0 and the call is refused
    for args in (dict(n=3, T=2520, B=1000, L=10, budget=2000), dict(n=5, T=1 << 22, B=64, L=4096, budget=1 << 20)):
        pl = plan(**args)
        assert pl["per_chunk"] == 0 and pl["chunks"] == 0 and pl["staging_bytes"] == 0 and pl["need_bytes"] > args["budget"]


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("ddboot_plan_driver", sanitize=True)
    for name in ("one_lane_chunks_arena", "two_tables", "longest_row"):
        n, T, B, L, Q_, R_, lst, staged, raw, row, req = PLAN_SHAPES[name]
        assert run_driver(exe, n, T, B, L, Q_, R_, lst, staged, raw, 256, row, req, sanitized=True) == \
            run_driver(build_plan_driver("ddboot_plan_driver"), n, T, B, L, Q_, R_, lst, staged, raw, 256, row, req)


# ---------------------------------------------------------------------- (e) under the sanitizers
REFUSED = ("n = 0 outside", "from_bar = -1", "B = 0 outside", "B = 65537 outside", "L = 0 outside", "Q = 9 outside [0, 8]",
           "R = 9 outside [0, 8]", "alpha_ppm is NULL", "level 1: alpha_ppm = 0", "level 0: alpha_ppm = 1000001",
           "limits is NULL", "limit 1: -1 is negative", "are all NULL", "equity and n_bars are required", "n_bars = 4 ",
           "T = 0 bars of the window [2, 2)", "increment 2147483648 at bar 1 of lane 0")
RULES = ("null engine", "no dataset loaded", "n = 3 with lanes == NULL (all-lanes mode takes n = 0)",
         "n = 0 outside [1, 1048576]", "n = 1048577 outside [1, 1048576]", "d is required", "from_bar = -3 is negative",
         "lanes_out, q_out, reach_out and raw_out are all NULL", "lanes_out, q_out, reach_out and raw_out are all NULL",
         "raw_out given in all-lanes mode: it must be NULL", "",
         "the call needs 10496 bytes of device staging, above the budget of 2000 bytes", "", "",
         "the prefix row and block tables of T = 4832 bars (154632 bytes) do not fit the LDS row limit of 154624 bytes "
         "(bt_set_ddboot_row mode 1)")


def test_planner_and_host_code_under_asan_and_ubsan(tmp_path):
    """tests/asan/ddboot_driver.cpp with csrc/ddboot.cpp, the window rule of csrc/bootstrap.cpp and
    csrc/plan.cpp: a program of its own, built with the sanitizers and run directly."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    exe = str(tmp_path / "ddboot_asan")
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *SANITIZE, "-x", "hip",
                        "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "ddboot_driver.cpp"), *(os.path.join(CSRC, s) for s in SOURCES),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lv, lm = np.array(LEVELS, np.int32), np.array(LIMITS, np.int64)
    for strategy, seed, cut in (("sma", 0, False), ("ema_ols", 1, True), ("boll", 2, False)):
        c, rf = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        want, window = R.walk_ref(strategy, seed, cut)
        S, P = len(c.series), c.grid.n_params
        B, L, sd = R.walk_params(strategy, seed)
        n, stride = S * P, max(c.bars)
        eq = np.zeros((n, stride), np.int64)
        for s in range(S):
            for p in range(P):
                eq[s * P + p, :c.bars[s]] = rf.curves[s][p][1]
        nb = np.repeat(np.array(c.bars, np.int32), P)
        fin, fout = str(tmp_path / f"in_{strategy}"), str(tmp_path / f"out_{strategy}")
        frm, to = window or (0, 0)
        with open(fin, "wb") as f:
            f.write(np.array([n, stride, frm, to, B, L, Q, NR], np.int32).tobytes() + np.array([sd], np.uint64).tobytes()
                    + lv.tobytes() + lm.tobytes() + nb.tobytes() + eq.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=SANITIZE_ENV, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        cut_at = np.cumsum([n * 72, n * Q * 8, n * NR * 8, n * B * 8]).tolist()
        assert len(raw) == cut_at[-1]
        got = type(want)(lanes=np.frombuffer(raw[:cut_at[0]], D.DD_LANE_DTYPE),
                         quantiles=np.frombuffer(raw[cut_at[0]:cut_at[1]], np.int64).reshape(n, Q),
                         reach=np.frombuffer(raw[cut_at[1]:cut_at[2]], np.int64).reshape(n, NR),
                         raw=np.frombuffer(raw[cut_at[2]:], np.int64).reshape(n, B))
        R.assert_same(got, want, f"{strategy} under the sanitizers")
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {n} {B} {Q} {NR}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == len(REFUSED)
        for ln, named in zip(refused, REFUSED):
            assert named in ln, (ln, named)
        assert [ln[len("rule: "):] for ln in lines if ln.startswith("rule:")] == list(RULES)
        assert [ln for ln in lines if ln.startswith("rank: ")] == ["rank: 1 950 951 65536"]
        plans = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("plan: ")]
        assert [p[0] for p in plans] == [1, 1, 2, 2] and plans[0][1:3] == (n, 1)


# ------------------------------------------------------------------------- (f) derived views
def test_derived_views_equal_their_restatement():
    rows, B, L, seed = R.crafted()["dip_31"]
    ref = R.drawdown_risk(rows.tolist(), B, L, seed)
    dr = D.DrawdownRisk(np.array(LEVELS, np.int32), np.array(LIMITS, np.int64), B, ref.lanes, ref.quantiles, ref.reach, ref.raw)
    star = [[int(x) for x in r] for r in ref.raw]
    assert dr.m1.tolist() == [sum(s) for s in star] and dr.m2.tolist() == [sum(x * x for x in s) for s in star]
    assert dr.mean().tolist() == [sum(s) / B for s in star]
    assert dr.std().tolist() == [math.sqrt((B * sum(x * x for x in s) - sum(s) ** 2) / (B * B)) for s in star]
    assert np.allclose(dr.std(), np.std(ref.raw, axis=1), rtol=1e-12)
    assert dr.p_value().tolist() == [sum(x >= R.mdd(row) for x in s) / B for s, row in zip(star, rows.tolist())]
    for j, a in enumerate(LEVELS):
        assert dr.quantile(j).tolist() == [float(sorted(s)[R.rank(B, a) - 1]) for s in star]
        assert dr.pnl_to_dd(j).tolist() == [sum(row) / q if q else 0.0 for row, q in zip(rows.tolist(), dr.quantiles[:, j].tolist())]
    assert dr.prob_reach().tolist() == [[sum(x >= lim for x in s) / B for lim in LIMITS] for s in star]
    # a lane that never falls: every quantile is 0, and the ratio with it
    up = R.drawdown_risk([[1, 2, 3, 4]], 8, 2, 1)
    flat = D.DrawdownRisk(np.array(LEVELS, np.int32), np.array(LIMITS, np.int64), 8, up.lanes, up.quantiles, up.reach, None)
    assert flat.pnl_to_dd(1).tolist() == [0.0] and flat.std().tolist() == [0.0] and flat.p_value().tolist() == [1.0]
    assert flat.prob_reach().tolist() == [[1.0, 0.0, 0.0, 0.0]]
    assert D.ddrisk.as_limits((0, 5)).tolist() == [0, 5] and D.ddrisk.as_limits(np.array([7])).dtype == np.int64
    for bad in ((0.5,), (True,), (2**63,)):
        with pytest.raises(ValueError, match="limits"):
            D.ddrisk.as_limits(bad)


def test_host_refusals_name_the_value():
    eq, nb = np.array([[0, 5, -2]], np.int64), [3]
    for kw, named in ((dict(resamples=0), r"B = 0 outside"), (dict(block=0), r"L = 0 outside"),
                      (dict(levels=(1,) * 9), r"Q = 9 outside \[0, 8\]"), (dict(limits=(-1,)), r"limit 0: -1 is negative"),
                      (dict(window=(3, 3)), r"T = 0 bars"), (dict(levels=(0,)), r"level 0: alpha_ppm = 0")):
        with pytest.raises(D.BtError, match=named):
            D.drawdown_risk_host(eq, nb, **{"resamples": 4, "block": 3, **kw})
    got = D.drawdown_risk_host(eq, nb, 4, 3, 1, None, (1.0,), (0, 9), raw=True)
    assert got.raw.tolist() == [[7, 7, 7, 7]] and got.quantiles.tolist() == [[7]] and got.reach.tolist() == [[4, 0]]
