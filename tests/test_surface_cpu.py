"""Reductions of a run, the parts that need no GPU (docs/surface_spec.md): bt_surface_host and
bt_surface_merge against the plain-Python restatement of surface_ref.py on a literal case and on
adversarial matrices (surface_cases.py), the refusals, the record layout, the launch planner
(plan_surface through tests/plan/surface_plan_driver.cpp), Surface's derived figures, and the host
code as a stand-alone program under AddressSanitizer and UBSan (tests/asan/surface_driver.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from helpers import assert_staging_layout, build_plan_driver, run_driver
from surface_cases import SHAPES, adversarial, adversarial_ref, assert_same
from surface_ref import PARAM_AGG, SUMMARY, TOPK, qs, surface_ref, ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")


# ------------------------------------------------------------------------------ literal case
def _literal():
    m = np.zeros((3, 2), D.SUMMARY_DTYPE)
    #            n_trades status pnl   mdd exposure sharpe hash
    m[0, 0] = (4, 0, 100, 30, 50, 1.5, 11)
    m[1, 0] = (0, 0, 0, 0, 0, 0.0, 12)
    m[2, 0] = (7, 0, -40, 90, 20, -0.5, 13)
    m[0, 1] = (2, 0, 10, 5, 9, 2.0, 14)
    m[1, 1] = (3, 0, 20, 6, 8, 2.0, 15)
    m[2, 1] = (1, 0, -5, 7, 7, 0.25, 16)
    return m, [30, 10, 20]


def test_literal_matrix_gives_the_records_written_out_here():
    m, ids = _literal()
    s = D.surface_host(m, ids)
    want = np.zeros(2, D.PARAM_AGG_DTYPE)
    # ss1 = (1.5 + 0 - 0.5) 2^32 = 2^32; ss2 = (2.25 + 0.25) 2^64 = 2^65 + 2^63
    want[0] = (3, 2, 1, 1, 11, 60, 70, 90, 1.5, -0.5, 30, 20, 2**32, 0, 2**63, 2)
    # Sharpe 2.0 twice: the maximum goes to the lower id, 10
    # ss1 = 4.25 2^32; ss2 = (4 + 4 + 0.0625) 2^64 = 8 2^64 + 2^60
    want[1] = (3, 3, 2, 3, 6, 25, 24, 7, 2.0, 0.25, 10, 20, 17 * 2**30, 0, 2**60, 8)
    assert_same(s.params, want, "literal params")
    best = np.zeros(3, D.TOPK_DTYPE)
    best[0] = (2.0, 30, 1, 10)
    best[1] = (2.0, 10, 1, 20)
    best[2] = (0.25, 20, 1, -5)
    assert_same(s.best, best, "literal best")
    ref_p, ref_b = surface_ref(m, ids)
    assert_same(ref_p, want, "reference params")
    assert_same(ref_b, best, "reference best")


def test_fixed_point_sharpe_rounds_half_to_even_and_clamps():
    assert [qs(x) for x in (0.5 / 2**32, 1.5 / 2**32, 2.5 / 2**32, -0.5 / 2**32, -1.5 / 2**32)] == [0, 2, 2, 0, -2]
    assert qs(1e9) == qs(32768.0) == 2**47 and qs(-1e9) == -(2**47)
    assert qs(5e-324) == 0 and qs(-0.0) == 0 and qs(1.0) == 2**32
    m = np.zeros((5, 1), D.SUMMARY_DTYPE)
    m["sharpe"][:, 0] = (0.5 / 2**32, 1.5 / 2**32, 2.5 / 2**32, 1e9, -32768.0)
    a = D.surface_host(m, range(5)).params[0]
    assert (int(a["ss1_lo"]), int(a["ss1_hi"])) == (4, 0)             # 0 + 2 + 2 + 2^47 - 2^47
    assert (int(a["ss2_lo"]), int(a["ss2_hi"])) == (8, 2 * 2**30)     # 4 + 4 + 2 * 2^94


# ------------------------------------------------------------------- adversarial matrices
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_reference(shape):
    m, ids = adversarial(*shape)
    ref_p, ref_b = adversarial_ref(*shape)
    s = D.surface_host(m, ids)
    assert s.params.dtype == D.PARAM_AGG_DTYPE and s.best.dtype == D.TOPK_DTYPE
    assert_same(s.params, ref_p, f"params {shape}")
    assert_same(s.best, ref_b, f"best {shape}")
    assert_same(D.surface_host(m, ids, best=False).params, ref_p, f"params alone {shape}")
    if shape[0] == 0:
        assert len(s.best) == 0 and (s.params["n_sym"] == 0).all()
        assert (s.params["sym_max"] == -1).all() and (s.params["sym_min"] == -1).all()
        assert not s.params["sharpe_max"].any() and not s.params["mdd_max"].any()


def test_the_matrices_reach_the_limits_they_are_there_for():
    n_max = n_min = n_best = 0
    carried = negative = clamped = half = skipped = 0
    for shape in SHAPES:
        m, ids = adversarial(*shape)
        a, b, c = ties(m, ids)
        n_max, n_min, n_best = n_max + a, n_min + b, n_best + c
        ref_p, _ = adversarial_ref(*shape)
        carried += int((ref_p["ss2_hi"] != 0).sum())
        negative += int((ref_p["ss1_hi"] == -1).sum())
        clamped += int((np.abs(m["sharpe"]) > 32768).sum())
        half += int((np.abs(m["sharpe"] * 2.0**32 % 1.0) == 0.5).sum())
        skipped += int((m["status"] != 0).sum())
        if m.size > 16:   # a fifth of the records sit one tick inside +-2^52
            assert np.abs(m["pnl"]).max() >= 2**52 - 1
    assert n_max >= 1 and n_min >= 1 and n_best >= 1, (n_max, n_min, n_best)
    assert carried >= 1 and negative >= 1 and clamped >= 1 and half >= 1 and skipped >= 1


# ------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("parts", (1, 2, 3, 7))
def test_merge_of_row_splits_equals_the_whole(parts):
    m, ids = adversarial(300, 7)
    whole = D.surface_host(m, ids)
    # the tied maxima of some column land in different parts, and one part is empty
    col = next(p for p in range(7) if ties(m[:, p:p + 1], ids)[0])
    keys = m["sharpe"][:, col].copy()
    keys[m["status"][:, col] != 0] = -np.inf
    top = np.nonzero(keys == keys.max())[0]
    cuts = {0, 300}
    if parts > 1:
        cuts |= {int(top[0]) + 1}
        assert top[0] + 1 <= top[-1]
    rng = np.random.default_rng(parts)
    while len(cuts) < parts + (parts < 3):
        cuts.add(int(rng.integers(1, 300)))
    cuts = sorted(cuts)
    if parts > 2:
        cuts.insert(2, cuts[1])    # an empty part
    pieces = [D.surface_host(m[a:b], ids[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(pieces) == parts and (parts < 3 or len(pieces[1].best) == 0)
    got = D.merge_surfaces(pieces)
    assert_same(got.params, whole.params, f"merge of {parts}")
    assert_same(got.best, whole.best, f"concatenated best of {parts}")
    assert_same(D.merge_surfaces(pieces[::-1]).params, whole.params, f"merge of {parts}, reversed")


def test_merge_of_only_empty_parts_is_the_empty_aggregate():
    m, ids = adversarial(0, 3)
    e = D.surface_host(m, ids)
    assert_same(D.merge_surfaces([e, e]).params, adversarial_ref(0, 3)[0], "empty + empty")


# --------------------------------------------------------------------------------- refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    m, ids = _literal()
    ids = np.asarray(ids, np.int32)
    agg = np.zeros(2, D.PARAM_AGG_DTYPE)
    best = np.zeros(3, D.TOPK_DTYPE)
    host, merge = E.sym("bt_surface_host"), E.sym("bt_surface_merge")

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(3, 2, m.ctypes.data, ids.ctypes.data, agg.ctypes.data, best.ctypes.data) == 0
        assert_same(agg, surface_ref(m, ids)[0], "after a refusal")

    for args, named in (
        ((-1, 2, m.ctypes.data, ids.ctypes.data, agg.ctypes.data, None), r"bt_surface_host: S = -1 "),
        ((3, 0, m.ctypes.data, ids.ctypes.data, agg.ctypes.data, None), r"bt_surface_host: P = 0 "),
        ((3, -4, m.ctypes.data, ids.ctypes.data, agg.ctypes.data, None), r"P = -4 "),
        ((3, 2, m.ctypes.data, ids.ctypes.data, None, None), r"agg and best are both NULL"),
        ((3, 2, None, ids.ctypes.data, agg.ctypes.data, None), r"sum and sym_ids are required"),
    ):
        assert host(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    for world in (0, -3):
        assert merge(agg.ctypes.data, world, 2, agg.ctypes.data) == -1
        assert re.search(rf"bt_surface_merge: world = {world} ", last()), last()
        still_good()
    # the engine entry points refuse a null engine before anything else
    for name, args in (("bt_surface", (None, agg.ctypes.data, None)),
                       ("bt_surface_of", (None, 3, 2, m.ctypes.data, ids.ctypes.data, agg.ctypes.data, None)),
                       ("bt_set_surface_chunks", (None, 2))):
        assert E.sym(name)(*args) == -1
        assert re.search(rf"{name}: null engine", last()), last()
    still_good()
    with pytest.raises(D.BtError, match="P = 0 "):
        D.surface_host(np.zeros((2, 0), D.SUMMARY_DTYPE), [1, 2])
    with pytest.raises(D.BtError, match="world = 0 "):
        D.merge_surfaces([])
    with pytest.raises(ValueError, match="sym_ids"):
        D.surface_host(m, [1, 2])


# ----------------------------------------------------------------------------------- layout
def test_param_agg_layout(tmp_path):
    assert D.PARAM_AGG_DTYPE.itemsize == 104 == PARAM_AGG.itemsize
    assert D.PARAM_AGG_DTYPE == PARAM_AGG and D.SUMMARY_DTYPE == SUMMARY and D.TOPK_DTYPE == TOPK
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    fields = D.PARAM_AGG_DTYPE.names
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt.h"\nint main(void) {\n'
                   '    printf("{\\"size\\": %d", (int)sizeof(bt_param_agg));\n' +
                   "".join(f'    printf(", \\"{f}\\": %d", (int)offsetof(bt_param_agg, {f}));\n' for f in fields) +
                   '    printf("}\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("size") == 104
    assert got == {f: D.PARAM_AGG_DTYPE.fields[f][1] for f in fields}


# ---------------------------------------------------------------------------------- planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("surface_plan_driver")

    def run(S, P, cus=256, chunks=0, staged=0):
        return run_driver(exe, S, P, cus, chunks, staged)
    return run


PLAN_SHAPES = {
    "config2": (5000, 400, 0), "config3": (500, 64, 0), "config4": (500, 256, 0), "config5": (10000, 1024, 0),
    "one": (1, 1, 0), "wide": (3, 960, 0), "shard2": (5000, 400, 0), "shard3": (250, 64, 0),
    "forced_above_S": (7, 400, 12), "forced_3": (65, 130, 3), "no_rows": (0, 12, 0), "no_rows_forced": (0, 12, 5),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_surface_covers_every_row_once(plan, name):
    S, P, req = PLAN_SHAPES[name]
    pl = plan(S, P, 256, req)
    assert pl == plan(S, P, 256, req), "the plan is a function of its arguments"
    assert pl["agg_bytes"] == 104
    assert 1 <= pl["chunks"] <= max(S, 1)
    assert pl["block"] % 64 == 0 and 64 <= pl["block"] <= 256
    assert pl["p_blocks"] * pl["block"] >= P > (pl["p_blocks"] - 1) * pl["block"]
    assert pl["p_tiles"] == (P + 63) // 64
    assert pl["partial_bytes"] == pl["chunks"] * P * 104
    assert pl["best_partial_bytes"] == S * pl["p_tiles"] * 24
    # many chunks fold in two steps of about sqrt(chunks) partials each, few in one
    ways = pl["fold_ways"]
    assert pl["fold_bytes"] == ways * P * 104
    assert (ways == 0) if pl["chunks"] <= 16 else (1 < ways < pl["chunks"] <= ways * ways < pl["chunks"] + 2 * ways)
    rows = pl["rows"]
    assert len(rows) == pl["chunks"] and rows[0][0] == 0 and rows[-1][1] == S
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:])), "chunks are contiguous"
    assert S == 0 or all(r1 > r0 for r0, r1 in rows), "no empty chunk"
    assert max(r1 - r0 for r0, r1 in rows) - min(r1 - r0 for r0, r1 in rows) <= 1
    if req:
        assert pl["chunks"] == max(1, min(req, S))
    # the staging layout: the work regions, the two results next to each other (one copy brings
    # both back), and for bt_surface_of the matrix and the ids in the same layout
    for staged in (0, 1):
        st = plan(S, P, 256, req, staged)
        assert {k: v for k, v in st.items() if not k.startswith("o_") and k != "staging_bytes"} == \
            {k: v for k, v in pl.items() if not k.startswith("o_") and k != "staging_bytes"}
        assert_staging_layout([(st["o_partial"], st["partial_bytes"]), (st["o_fold"], st["fold_bytes"]),
                               (st["o_best_partial"], st["best_partial_bytes"]), (st["o_agg"], P * 104),
                               (st["o_best"], S * 24), (st["o_sum"], staged * S * P * 48), (st["o_ids"], staged * S * 4)],
                              st["staging_bytes"], f"{name} staged {staged}")
        assert st["o_best"] - (st["o_agg"] + P * 104) < 256
        assert st["staging_bytes"] < st["o_ids"] + staged * S * 4 + 512, "no more than the regions need"


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("surface_plan_driver", sanitize=True)
    assert run_driver(exe, 65, 130, 256, 3, 1, sanitized=True) == \
        run_driver(build_plan_driver("surface_plan_driver"), 65, 130, 256, 3, 1)


def test_plan_surface_fills_the_gpu_without_shredding_the_rows(plan):
    c2, c3 = plan(5000, 400), plan(250, 64)
    waves = lambda pl: pl["chunks"] * pl["p_blocks"] * pl["block"] // 64
    assert 256 * 4 <= waves(c2) <= 256 * 4 * 8          # one to a few waves per SIMD
    assert c2["rows_per_chunk"] >= 16 and c3["rows_per_chunk"] >= 16
    assert c3["chunks"] > 1                              # a one-tile grid still spreads over CUs
    assert plan(5000, 400, 64)["chunks"] < c2["chunks"]  # fewer CUs, fewer chunks
    assert plan(100000, 64, 256, 100000)["chunks"] == 65535  # the grid's y limit


# ------------------------------------------------------------------------- derived figures
def test_rank_and_mean_sharpe_on_a_literal_case():
    m = np.zeros((2, 4), D.SUMMARY_DTYPE)
    m["sharpe"] = [[1.0, 3.0, 2.0, 3.0], [2.0, 1.0, -2.0, 1.0]]
    m["pnl"] = [[5, -1, 0, 9], [-5, 1, 0, 9]]
    s = D.surface_host(m, [7, 8])
    assert s.mean_sharpe().tolist() == [1.5, 2.0, 0.0, 2.0]
    assert s.std_sharpe().tolist() == [0.5, 1.0, 2.0, 1.0]
    assert s.win_rate().tolist() == [0.5, 0.5, 0.0, 1.0]
    assert s.rank().tolist() == [1, 3, 0, 2]                 # ties to the lower index
    assert s.rank(2).tolist() == [1, 3]
    assert s.rank(1, by="win_rate").tolist() == [3]
    assert s.rank(by="pnl").tolist() == [3, 0, 1, 2]
    assert s.rank(by="std_sharpe").tolist() == [2, 1, 3, 0]
    with pytest.raises(ValueError, match="rank by"):
        s.rank(by="median")
    grid = D.Grid.sma([3, 5], [20, 31])
    assert grid.param(int(s.rank(1)[0])) == {"f": 3, "s": 31}
    empty = D.surface_host(m[:0], [])
    assert empty.mean_sharpe().tolist() == [0.0] * 4 and empty.rank().tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------- under the sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "surface_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
                        os.path.join(ROOT, "tests", "asan", "surface_driver.cpp"),
                        os.path.join(CSRC, "surface.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    for (S, P), parts in zip(SHAPES, (2, 1, 2, 3, 7)):
        m, ids = adversarial(S, P)
        cuts = np.linspace(0, S, parts + 1).astype(np.int32)
        if parts > 2:
            cuts[2] = cuts[1]   # an empty part
        fin, fout = str(tmp_path / f"in_{S}_{P}"), str(tmp_path / f"out_{S}_{P}")
        with open(fin, "wb") as f:
            f.write(np.array([S, P, parts], np.int32).tobytes() + cuts.tobytes() + m.tobytes() + ids.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        na, nb = P * 104, S * 24
        assert len(raw) == 3 * na + 3 * nb
        ref_p, ref_b = adversarial_ref(S, P)
        agg, best, merged, part_best, agg2, best2 = (
            np.frombuffer(raw[a:b], dt) for a, b, dt in (
                (0, na, PARAM_AGG), (na, na + nb, TOPK), (na + nb, 2 * na + nb, PARAM_AGG),
                (2 * na + nb, 2 * na + 2 * nb, TOPK), (2 * na + 2 * nb, 3 * na + 2 * nb, PARAM_AGG),
                (3 * na + 2 * nb, 3 * na + 3 * nb, TOPK)))
        for got, want, what in ((agg, ref_p, "params"), (merged, ref_p, "merged"), (agg2, ref_p, "params alone"),
                                (best, ref_b, "best"), (part_best, ref_b, "parts' best"), (best2, ref_b, "best alone")):
            assert_same(got, want, f"{what} {S}x{P}")
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {S} {P} {parts}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == 4
        assert "S = -1 " in refused[0] and "P = 0 " in refused[1] and "both NULL" in refused[2]
        assert "world = 0 " in refused[3]
        rules = [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")]
        assert re.search(r"S\*P = 4096\*1025 exceeds 2\^22", rules[0])
        assert rules[1] == "4294967296 rows: dataset too large for exact int64 sums"
        assert rules[2] == "" and rules[3] == ""
