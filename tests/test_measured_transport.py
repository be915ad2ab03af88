"""The measured transport of the sharded camera exchange (`gbp_comm_init(ctx, region, 5)`, `--transport measured`): the library times
every transport the ranks can form — host-staged, p2p, p2p-slices, RCCL in both schedules — on the camera side of the sharded iteration
and attaches the fastest, every rank deciding from the same gathered table.  What is claimed and checked: the ranks agree, the record
says what was measured, and whatever wins leaves the bits of the host-staged transport (2).  Which transport wins is a timing and is not
asserted anywhere.  The ranks are fresh processes (tests/rank_worker.py) started by the launcher the multi-process suites share
(tests/rank_group.py); nothing is run twice."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import seq_path
from tests.rank_group import GROUPS
from tests.test_cli import BA, LINE, ROOT, SLAM

STATE = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
HOST, MEASURED = 2, 5
ON_ONE_GPU = ("host-staged", "p2p", "p2p-slices")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


def run(cmd, timeout):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def _body(out):
    """the lines that carry the run's numbers: initial metric, weakenings, per-iteration metric"""
    return [l.strip() for l in out.splitlines() if l.strip().startswith(("Initial", "Weakening", "Iter "))]


# ---- CPU: the flag, the two pure functions -------------------------------------------------------------------------------------------

def test_transport_measured_is_parsed():
    """--transport measured (and its number, 5) gets past the parser of both CLIs: the run then stops at the missing input file."""
    for exe in (BA, SLAM):
        for value in ("measured", "5"):
            rc, _, err = run([exe, "--transport", value], 60)
            assert rc == 1 and "--bal_file" in err and "invalid option value" not in err, (exe, value, err)
            rc, _, err = run([exe, "--bal_file", "/nonexistent/file.txt", "--transport", value], 60)
            assert rc == 1 and "unable to open file" in err and "invalid option value" not in err, (exe, value, err)


def test_help_lists_measured_transport():
    for exe in (BA, SLAM):
        rc, out, _ = run([exe, "--help"], 60)
        assert rc == 0 and "| measured" in out and "auto | rccl | host | p2p" in out, exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_choice_and_eligibility_under_asan_ubsan(tmp_path):
    """eligible_candidates and choose_transport (csrc/gbp_transport.hpp) as a stand-alone program under ASan + UBSan
    (tests/sanitize/transport_choice_main.cpp): the baseline kept on a tie and when the gain is inside its own two-measurement spread, a
    clear winner taken, an ineligible candidate never winning, the MAX over the ranks deciding, the same table giving the same answer on
    every rank; RCCL out when ranks share a GPU or one lacks librccl, the peer transports out without mutual peer access."""
    exe = str(tmp_path / "transport_choice")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", os.path.join(ROOT, "tests", "sanitize", "transport_choice_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "transport_choice: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


# ---- GPU: real processes on the one GPU ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ranks_of(tmp_path_factory):
    """ranks_of(world, transport, scenario): the run, made once and shared by the tests that read it"""
    def get(world, transport, scenario):
        from gbp_poplar_amd import hostlib
        return GROUPS.ranks_of("tests.rank_worker", world, (transport, scenario), lambda: str(tmp_path_factory.mktemp("measured") / "run"),
                               lambda: int(hostlib.bal_read(seq_path("fr2robot2"))["n_cams"]), 150)[0]
    return get


def _assert_same_state(world, got, want):
    for r in range(world):
        for k in STATE:
            assert np.array_equal(got[r][0][k], want[r][0][k]), (r, k)
    for r in range(1, world):      # the replicated cameras agree across the ranks
        assert np.array_equal(got[r][0]["cam_beliefs_eta"], got[0][0]["cam_beliefs_eta"]), r
        assert np.array_equal(got[r][0]["cam_beliefs_lambda"], got[0][0]["cam_beliefs_lambda"]), r


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_every_rank_reports_the_same_choice_and_table(world, ranks_of):
    """gbp_comm_init(ctx, region, 5) on `world` real processes sharing the GPU: every rank names the same transport, one the ranks of one
    GPU can form; gbp_comm_describe says it was selected by measurement and lists host-staged, p2p and p2p-slices with finite positive
    figures that are equal on all ranks, RCCL as not eligible because ranks share a GPU; gbp_last_error holds the info line."""
    got = ranks_of(world, MEASURED, "loop")
    for r, (_, info) in enumerate(got):
        print("rank %d: init %.3f s; %s" % (r, info["init_s"], json.dumps(info["describe"])))
    chosen = got[0][1]["transport"]
    assert chosen in ON_ONE_GPU
    first = got[0][1]["describe"]["measured"]
    for r, (_, info) in enumerate(got):
        d = info["describe"]
        assert info["transport"] == chosen and d["transport"] == chosen and d["rank"] == r and d["world"] == world
        assert d["selected_by"] == "measurement" and d["two_streams"] is False
        for key in ("device", "pci_bus_id", "library", "library_version"):      # the present keys stay
            assert key in d
        by_name = {}
        for e in d["measured"]:
            by_name.setdefault(e["transport"], []).append(e)
        assert set(by_name) == {"rccl", "host-staged", "p2p", "p2p-slices"}
        for e in by_name["rccl"]:
            assert e["eligible"] is False and "share a GPU" in e["reason"] and "us_per_exchange" not in e
        for name in ON_ONE_GPU:
            e, = by_name[name]
            assert e["eligible"] is True and e["two_streams"] is False and e["reps"] >= 1
            assert math.isfinite(e["us_per_exchange"]) and e["us_per_exchange"] > 0
            assert 0 < e["us_this_rank"] <= e["us_per_exchange"] + 0.001      # (the MAX over the ranks; both printed to 0.001 us)
        base, = [e for e in d["measured"] if e.get("baseline")]
        assert base["transport"] == "host-staged" and base["us_per_exchange"] == min(base["us_first"], base["us_last"])
        assert [e for e in d["measured"] if e.get("chosen")][0]["transport"] == chosen
        # what every rank decided from: the same entries, this rank's own figure aside
        strip = lambda es: [{k: v for k, v in e.items() if k != "us_this_rank"} for e in es]
        assert strip(d["measured"]) == strip(first), r
        assert info["last_error"].count("info: gbp_comm_init: measured") == 1 and "chose " + chosen in info["last_error"]


@pytest.mark.gpu
def test_other_transports_say_who_chose_them(ranks_of):
    """transport 2: "selected_by" is "caller" and there is no "measured" key"""
    for _, info in ranks_of(2, HOST, "loop"):
        assert info["describe"]["selected_by"] == "caller" and "measured" not in info["describe"]
        assert info["transport"] == "host-staged"


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_loop_state_and_metric_bit_identical_to_host_staged(world, ranks_of):
    """LINEARISE and 30 passes of the loop body (the five weakenings, the relinearising sweeps) behind the measurement: every rank's
    beliefs, damping, damping counts and robust flags, the 12 per-pass metric records and gbp_eval_global are the host-staged
    transport's, bit for bit and field for field, and all ranks hold the same camera beliefs."""
    got, want = ranks_of(world, MEASURED, "loop"), ranks_of(world, HOST, "loop")
    _assert_same_state(world, got, want)
    assert np.any(got[0][0]["cam_beliefs_eta"] != 0)
    for r in range(world):
        assert len(got[r][1]["loop"]) == 12 and got[r][1]["loop"] == want[r][1]["loop"], r
        assert got[r][1]["eval"] == want[r][1]["eval"] and got[r][1]["eval"] == got[0][1]["eval"], r
    assert got[0][1]["eval"]["n_active"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_slam_flow_bit_identical_to_host_staged(world, ranks_of):
    """The SLAM flow behind the measurement: 23 sweeps, NEW_KEYFRAME in front of sweeps 8 and 16: state and trajectory are the
    host-staged transport's."""
    got, want = ranks_of(world, MEASURED, "slam"), ranks_of(world, HOST, "slam")
    assert got[0][1]["describe"]["selected_by"] == "measurement"
    _assert_same_state(world, got, want)
    for r in range(world):
        assert len(got[r][1]["traj"]) == 24 and got[r][1]["traj"] == want[r][1]["traj"], r


@pytest.mark.gpu
def test_upload_before_comm_init_gives_the_same_bits(ranks_of):
    """gbp_upload BEFORE gbp_comm_init(ctx, region, 5) — the measurement's launches run on the uploaded state and must leave it as it
    was — ends in the same bits and records as the upload after it, and as the host-staged transport."""
    got = ranks_of(2, MEASURED, "upload_first")
    assert all(info["describe"]["selected_by"] == "measurement" and len(info["describe"]["measured"]) == 5 for _, info in got)
    for want in (ranks_of(2, MEASURED, "loop"), ranks_of(2, HOST, "loop")):
        _assert_same_state(2, got, want)
        for r in range(2):
            assert got[r][1]["loop"] == want[r][1]["loop"] and got[r][1]["eval"] == want[r][1]["eval"], r


# ---- GPU: the executables ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_ba_ipus_2_measured_equals_host_staged():
    """`ba --ipus 2 --transport measured` through the five weakenings and the relinearising sweeps (17+): the host-staged run, line for
    line; the transport line names a real transport and the measurement's info line follows it."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "24", "--ipus", "2"]
    rc_h, out_h, err_h = run(base + ["--transport", "host"], 120)
    rc_m, out_m, err_m = run(base + ["--transport", "measured"], 120)
    assert rc_h == 0, err_h[-2000:]
    assert rc_m == 0, err_m[-2000:]
    assert any("Exchange between the 2 ranks: " + name in out_m for name in ON_ONE_GPU), out_m[:2000]
    assert "gbp_comm_init: measured" in out_m
    body = _body(out_m)
    assert len(LINE.findall(out_m)) == 24 and sum(l.startswith("Weakening") for l in body) == 5
    assert body == _body(out_h)


@pytest.mark.gpu
def test_measured_with_one_forked_rank_equals_plain_run(tmp_path):
    """--force_sharded 1 --transport measured: one rank, nothing to measure — transport 0's choice, "measured": [] in the --profile
    report's quote of gbp_comm_describe — and the plain ctx's lines."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "60", "--eval_every", "20"]
    rc1, out1, err1 = run(base, 120)
    env = dict(os.environ, GC_PROFILE_LOG_DIR=str(tmp_path))
    p = subprocess.run(base + ["--force_sharded", "1", "--transport", "measured", "--profile", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120, env=env)
    assert rc1 == 0 and p.returncode == 0, (err1[-500:], p.stderr[-1500:])
    assert "Exchange between the 1 ranks: " in p.stdout
    assert LINE.findall(out1) == LINE.findall(p.stdout) and len(LINE.findall(out1)) == 3
    with open(tmp_path / "gbp_profile.json") as f:
        comm = json.load(f)["comm"]
    assert comm["measured"] == [] and comm["world"] == 1 and comm["transport"] in ("rccl", "host-staged")
