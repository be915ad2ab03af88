"""The seeded slice of the randomised parity soak (tests/test_gpu_fuzz.py) without a GPU: its plans alone.  The list of seeds is chosen
so that every path the library can take meets every driver, every form of the state calls and of the metric, every `steps` and base
loop index; if an edit of the generator (tests/fuzz_support.py) thins that out, this fails here, before a GPU is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fuzz_support as fz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plans():
    return [fz.suite_plan(s) for s in fz.SUITE_SEEDS]


@pytest.fixture(scope="module")
def ba(plans):
    return [p for p in plans if p["kind"] == "ba"]


def test_kinds_and_size_classes(plans, ba):
    """about 120 seeds from one constant; every fourth SLAM, every eighth sharded; most graphs in the persistent kernel's range (below
    65 536 positions), a quarter between 65 536 and 131 072 positions, at least three of 2 048 tiles or more with SEG forced on, off and
    left to the library, those at most 20 iterations; nothing above 300 000 factors; long bursts only on graphs of at most 1 000 factors"""
    assert len(plans) == len(set(p["seed"] for p in plans)) == fz.SUITE_COUNT and 100 <= fz.SUITE_COUNT <= 140
    for p in plans:
        assert p["kind"] == fz.kind_of(p["seed"] - fz.SUITE_FIRST)
        assert p["bal"]["n_edges"] <= 300000
    assert sum(p["kind"] == "slam" for p in plans) == fz.SUITE_COUNT // 4 and sum(p["kind"] == "shard" for p in plans) == fz.SUITE_COUNT // 8
    small = [p for p in plans if p.get("positions", 0) < 65536]
    mid = [p for p in plans if 65536 <= p.get("positions", 0) < 131072]
    tiles = [p for p in ba if p["n_tiles"] >= 2048]
    print("size classes: %d below 65 536 positions, %d between, %d of >= 2 048 tiles" % (len(small), len(mid), len(tiles)))
    assert len(mid) * 4 >= fz.SUITE_COUNT - 16 and len(small) > fz.SUITE_COUNT // 2
    assert len(tiles) >= 3 and {p["seg"] for p in tiles} == {-1, 0, 1}
    for p in tiles:
        assert sum(b["n"] for b in p["bursts"]) <= 20 and p["tile_perm"] and p["row_placement"], fz.describe(p)
    for p in ba:
        assert p["persist"] == (p["path"] < 3)
        if p["persist"]:
            assert p["positions"] < 65536 + 4096, fz.describe(p)
        if any(b["n"] in fz.LONG_BURSTS for b in p["bursts"]):
            assert p["bal"]["n_edges"] <= fz.LONG_MAX_EDGES
            assert all(sum(b["n"] == n for b in p["bursts"]) <= 1 for n in fz.LONG_BURSTS)


def test_every_path_meets_every_driver_and_form(ba, plans):
    cells = {(pa, d): [] for pa in range(4) for d in range(4)}
    for p in ba:
        cells[(p["path"], p["drive"])].append(p["seed"])
    print("seeds per cell (predicted path of B x driver):")
    print("%-22s" % "" + "".join("%24s" % d for d in fz.DRIVERS))
    for pa in range(4):
        print("%-22s" % fz.PATH_NAMES[pa] + "".join("%24d" % len(cells[(pa, d)]) for d in range(4)))
    assert all(len(v) >= 2 for v in cells.values()), {k: v for k, v in cells.items() if len(v) < 2}
    for pa in range(4):
        on = [p for p in ba if p["path"] == pa]
        forms = {b["metric"] for p in on if p["drive"] in (1, 3) for b in p["bursts"]}
        assert forms == set(fz.METRIC_FORMS), (fz.PATH_NAMES[pa], forms)
        assert {p["upload"] for p in on} == set(fz.STATE_FORMS), fz.PATH_NAMES[pa]
        assert {b["eval"] for p in on for b in p["bursts"] if b["check"]} == {"host", "device"}
        assert {b["read"] for p in on for b in p["bursts"] if b["check"]} >= {"host", "device"}
        assert {b["sync"] for p in on for b in p["bursts"]} == {False, True}
    print("metric forms, upload forms, read forms, eval forms, sync / no sync: all on every path")
    assert {p["steps"] for p in ba} == {0, 1, 3, fz.CLI_STEPS}
    assert {(p["steps"], p["base"]) for p in ba} >= {(s, max(0, b)) for s in (0, 1, 3, fz.CLI_STEPS) for b in (0, 1, 2 * s - 2, 2 * s - 1)}
    lin = [p for p in ba if p["linearise_after"] >= 0]
    print("mid-run LINEARISE: %d seeds (%d persistent, %d hipGraph/direct)" % (len(lin), sum(p["persist"] for p in lin), sum(not p["persist"] for p in lin)))
    assert any(p["persist"] for p in lin) and any(not p["persist"] for p in lin)
    assert any(not p["bursts"][p["linearise_after"]]["sync"] for p in lin)          # ... with B's launches possibly still in flight
    for n in fz.LONG_BURSTS:
        assert any(b["n"] == n for p in ba for b in p["bursts"]), n
        assert any(b["n"] == n for p in ba if p["persist"] for b in p["bursts"]), n
    slam = [p for p in plans if p["kind"] == "slam"]
    assert {p["form"] for p in slam} == set(fz.STATE_FORMS) and {p["persist"] for p in slam} == {False, True}
    assert any(p["persist"] and p["form"] != "host" for p in slam) and any(p["persist"] and p["every"] == 1 for p in slam)


def test_the_graphs_are_what_the_docstring_promises(plans):
    """unsorted and sorted edge lists, duplicate edges, a landmark of degree > 15, factor-less landmarks, inactive factors"""
    free = [p for p in plans if p["kind"] != "slam"]
    for trait in ("sorted", "duplicates", "hub", "factorless"):
        assert sum(p["traits"][trait] for p in free) >= 5, trait
    assert sum(not p["traits"]["sorted"] for p in free) >= 5
    assert all((p["active_flag"] == 0).any() for p in free if p["bal"]["n_edges"] >= 200)
    assert all(p["traits"]["sorted"] for p in plans if p["kind"] == "slam")


def test_plans_are_a_pure_function_of_the_seed():
    for s in (fz.SUITE_FIRST, fz.SUITE_FIRST + 3, fz.SUITE_FIRST + 5, fz.SUITE_FIRST + 9):
        a, b = fz.suite_plan(s), fz.suite_plan(s)
        assert fz.describe(a) == fz.describe(b)
        for k in a["bal"]:
            assert np.array_equal(a["bal"][k], b["bal"][k])
        assert {k: v for k, v in a.items() if k not in ("bal", "active_flag")} == {k: v for k, v in b.items() if k not in ("bal", "active_flag")}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_oracle_alone_is_deterministic_and_weakens_where_passwalk_says(ba, tmp_path, oracle_mod):
    """three of the plans (small graphs; between them a base index in front of, on and behind the last weakening): the literal loop on the
    oracle, run twice, gives the same bits, and it weakens in front of exactly the loop indices PassWalk reports for (n, base, steps)"""
    exe = str(tmp_path / "loop_plan_walk")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "sanitize", "loop_plan_walk.cpp"), "-o", exe], cwd=ROOT)
    small = [p for p in ba if p["bal"]["n_edges"] <= 3000 and p["steps"] > 0]
    chosen = [next(p for p in small if p["base"] == 0), next(p for p in small if p["base"] == 2 * p["steps"] - 1), next(p for p in small if 0 < p["base"] < 2 * p["steps"] - 1)]
    n = 14
    oracle_mod.set_trig_mode(1)
    try:
        for p in chosen:
            s1, w1 = fz.oracle_walk(p, n)
            s2, w2 = fz.oracle_walk(p, n)
            assert w1 == w2 and all(np.array_equal(s1[k], s2[k], equal_nan=True) for k in s1), fz.describe(p)
            out = subprocess.run([exe, str(n), str(p["base"]), str(p["steps"])], stdout=subprocess.PIPE, text=True, timeout=60, check=True).stdout
            assert [int(x) for x in out.split()] == w1, (fz.describe(p), out, w1)
    finally:
        oracle_mod.set_trig_mode(0)
