"""The metric riding in the sharded iteration (gbp_ba_loop / gbp_iterate_eval_each with a host `out` on a ctx with a communicator): the
metric of iteration k is collected by the sweep of iteration k + 1, the belief update is two launches round the exchange, nothing of a burst
waits for the metric.  Whatever it runs must leave, byte for byte, the records and the state of the loop it replaces — gbp_iterate(1) +
gbp_eval per pass on the same kind of engine, calls this path does not touch — and the state of the N-shard oracle.  Every rank is a fresh
process (tests/metric_worker.py) started by the launcher the multi-process suites share (tests/rank_group.py), under a time limit;
nothing is run twice."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import seq_path
from tests.metric_worker import graph
from tests.rank_group import GROUPS
from tests.test_cli import BA, LINE, SLAM

STATE = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
HOST, P2P, SLICES = 2, 3, 4
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


@pytest.fixture(scope="module")
def ranks_of(tmp_path_factory):
    """ranks_of(world, transport, scenario, mode): the run, made once and shared by the tests that read it -> (per rank info, out_dir)"""
    def get(world, transport, scenario, mode):
        ranks, out_dir = GROUPS.ranks_of("tests.metric_worker", world, (transport, scenario, mode),
                                         lambda: str(tmp_path_factory.mktemp("metric") / "run"),
                                         lambda: None if scenario == "one_rank" else int(graph(scenario)["n_cams"]), 180)
        return [info for _, info in ranks], out_dir
    return get


def _state(out_dir, tag):
    return {k: np.load(os.path.join(out_dir, "%s_%s.npy" % (k, tag))) for k in STATE}


def _assert_same_state(a, b, what):
    for k in STATE:
        assert np.array_equal(a[k], b[k]), (what, k)


def _unpack(h):
    return struct.unpack("<dd5Q", bytes.fromhex(h))


def _rank_order_sum(recs):
    """gbp_eval_global's arithmetic over one pass's records in rank order -> the hex of the summed record"""
    acc = [0.0] * 7
    for h in recs:
        v = _unpack(h)
        for i in range(7):
            acc[i] = acc[i] + float(v[i])
    return struct.pack("<dd5Q", acc[0], acc[1], *(int(a + 0.5) for a in acc[2:])).hex()


def _assert_ranks_equal(world, got, want, what):
    (gi, gd), (wi, wd) = got, want
    for r in range(world):
        assert len(gi[r]["records"]) == len(wi[r]["records"]) > 0
        assert gi[r]["records"] == wi[r]["records"], (what, r)           # every field of every pass, as bytes
        _assert_same_state(_state(gd, "r%d" % r), _state(wd, "r%d" % r), (what, r))


# ---- 1, 5: one rank behind a communicator of every transport ---------------------------------------------------------------------------

def test_one_rank_rides_on_every_transport(ranks_of):
    """synth 5 x 70 x 3 (C no multiple of 4, L no multiple of 64 or 16, 210 factors), 12 passes with the five weakenings inside the burst,
    behind a 1-rank communicator of transports 2, 3 and 4: records and state are the plain ctx's riding ones and the per-pass loop's, and
    gbp_comm_describe says the metric rode for all 12 passes."""
    (info,), d = ranks_of(1, 0, "one_rank", "ride")
    assert info["n_factors"] == 210
    e = info["engines"]
    assert len(e["plain_ride"]["records"]) == 12 and _unpack(e["plain_ride"]["records"][-1])[2] == 210
    assert e["plain_ride"]["records"] == e["plain_perpass"]["records"] == e["t2_perpass"]["records"]
    for tag, name in (("t2", "host-staged"), ("t3", "p2p"), ("t4", "p2p-slices")):
        assert e[tag]["records"] == e["t2_perpass"]["records"], tag
        _assert_same_state(_state(d, tag), _state(d, "t2_perpass"), tag)
        _assert_same_state(_state(d, tag), _state(d, "plain_ride"), tag)
        m = e[tag]["describe"]["metric"]
        assert e[tag]["describe"]["transport"] == name
        assert m["path"] == "riding" and m["passes_riding"] == 12 and m["passes_per_pass"] == 0 and m["reason"] == "", (tag, m)
    m = e["t2_perpass"]["describe"]["metric"]      # no loop with the metric ran on that ctx
    assert m["path"] == "none" and m["passes_riding"] == 0 and m["passes_per_pass"] == 0


@pytest.mark.parametrize("schedule", ["one_stream", "two_streams"])
def test_one_rank_rides_over_rccl(schedule, ranks_of):
    """... and behind a 1-rank RCCL communicator in both schedules (gbp_comm_set_schedule): in the two-stream schedule the landmark half
    carries its share of the metric beside the all-gather and the combine behind the join counts the iteration."""
    (info,), d = ranks_of(1, 0, "one_rank", "ride")
    if not info["rccl"]:
        pytest.skip("librccl does not resolve here: " + info.get("rccl_error", ""))
    e = info["engines"]
    tag = "rccl_" + schedule
    assert e[tag]["describe"]["transport"] == "rccl" and e[tag]["describe"]["two_streams"] == (schedule == "two_streams")
    assert e[tag]["records"] == e["t2_perpass"]["records"]
    _assert_same_state(_state(d, tag), _state(d, "t2_perpass"), tag)
    m = e[tag]["describe"]["metric"]
    assert m["path"] == "riding" and m["passes_riding"] == 12, m


def test_burst_longer_than_the_ring(ranks_of):
    """gbp_iterate_eval_each(260) behind a 1-rank host-staged communicator: the ring of per-tile records holds at most 256 iterations, so
    the burst is two pieces — all 260 records and the state equal the per-pass loop's."""
    (info,), d = ranks_of(1, 0, "one_rank", "ride")
    e = info["engines"]
    assert len(e["each_ride"]["records"]) == 260
    assert e["each_ride"]["records"] == e["each_perpass"]["records"]
    _assert_same_state(_state(d, "each_ride"), _state(d, "each_perpass"), "each")
    assert e["each_ride"]["describe"]["metric"]["passes_riding"] == 260


# ---- 2, 3: two real ranks, fr2robot2 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transport", [HOST, P2P])
def test_two_ranks_ride(transport, ranks_of):
    """gbp_ba_loop(12, 0, steps) then (18, 12, steps) with the metric on two real ranks: each rank's records are its LOCAL sums — the
    per-pass loop's, byte for byte —, their rank-order sum is gbp_eval_global of the per-pass run, the state is the per-pass run's, and both
    ranks report the riding path."""
    got, want = ranks_of(2, transport, "loop", "ride"), ranks_of(2, HOST, "loop", "perpass")
    _assert_ranks_equal(2, got, want, transport)
    gi, wi = got[0], want[0]
    assert len(gi[0]["records"]) == 30
    for k in range(30):
        assert _rank_order_sum([gi[r]["records"][k] for r in range(2)]) == wi[0]["global"][k] == wi[1]["global"][k], k
    for r in range(2):
        m = gi[r]["describe"]["metric"]
        assert m["path"] == "riding" and m["passes_riding"] == 30 and m["passes_per_pass"] == 0, (r, m)
        assert _unpack(gi[r]["records"][0])[5:] == ((0, 0))      # healthy beliefs


def test_two_ranks_state_equals_sharded_oracle(ranks_of, oracle_mod):
    """... and the riding run's state is the oracle's in 2-shard summation order, device conventions: camera beliefs on every rank,
    landmark beliefs and factor state of its shard."""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], 2)
    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1, bounds)
        orc.upload(state)
        orc.linearise()
        means = []
        for it in range(30):
            if (it + 1) % 2 == 0 and it < 2 * opts.steps:
                orc.weaken_priors()
            orc.iterate(1)
            means.append(orc.eval())
        ro = orc.read()
    finally:
        oracle_mod.set_trig_mode(0)
    lmk = np.asarray(bal["lmk_id"])
    infos, d = ranks_of(2, HOST, "loop", "ride")
    for r in range(2):
        g = _state(d, "r%d" % r)
        assert np.array_equal(g["cam_beliefs_eta"], ro["cam_beliefs_eta"]), r
        assert np.array_equal(g["cam_beliefs_lambda"], ro["cam_beliefs_lambda"]), r
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        assert np.array_equal(g["lmk_beliefs_eta"][3 * lo:3 * hi], ro["lmk_beliefs_eta"][3 * lo:3 * hi]), r
        assert np.array_equal(g["lmk_beliefs_lambda"][9 * lo:9 * hi], ro["lmk_beliefs_lambda"][9 * lo:9 * hi]), r
        own = (lmk >= lo) & (lmk < hi)
        assert np.array_equal(g["damping_count"][own], ro["damping_count"][own]), r
        assert np.array_equal(g["robust_flag"][own], ro["robust_flag"][own]), r
    # the counters of every pass, summed over the ranks, are the oracle's (its sums are taken in another order: the counters are exact)
    for k in range(30):
        tot = _unpack(_rank_order_sum([infos[r]["records"][k] for r in range(2)]))
        assert tot[2:5] == (means[k]["n_active"], means[k]["n_relin"], means[k]["n_robust"]), k


def test_two_ranks_sliced_transport_stays_per_pass(ranks_of):
    """p2p-slices with two ranks: the same records and state, from the per-pass loop — its gathered cameras carry no metric records — and
    the reason names the transport."""
    got, want = ranks_of(2, SLICES, "loop", "ride"), ranks_of(2, HOST, "loop", "perpass")
    _assert_ranks_equal(2, got, want, "slices")
    for r in range(2):
        m = got[0][r]["describe"]["metric"]
        assert m["path"] == "per-pass" and m["passes_per_pass"] == 30 and m["passes_riding"] == 0 and "p2p-slices" in m["reason"], (r, m)


# ---- 4: more ranks than cameras, an empty landmark range ----------------------------------------------------------------------------

@pytest.mark.parametrize("scenario", ["synth:3:40", "synth:3:40:e"])
def test_four_ranks_three_cameras(scenario, ranks_of):
    """C = 3 < world = 4 on host-staged, 12 passes; `:e`: explicit bounds that leave rank 1 without a landmark (no landmark block, one
    tile of pads): records and state equal the per-pass loop's on every rank."""
    got, want = ranks_of(4, HOST, scenario, "ride"), ranks_of(4, HOST, scenario, "perpass")
    _assert_ranks_equal(4, got, want, scenario)
    b = got[0][0]["bounds"]
    assert (b[1] == b[2]) == scenario.endswith(":e")
    assert sum(_unpack(got[0][r]["records"][-1])[2] for r in range(4)) == 120
    if scenario.endswith(":e"):
        assert all(_unpack(h)[2] == 0 for h in got[0][1]["records"])
    for r in range(4):
        assert got[0][r]["describe"]["metric"]["path"] == "riding", r
        assert _rank_order_sum([got[0][q]["records"][11] for q in range(4)]) == want[0][r]["global"][11], r


# ---- 6: camera health is counted once ----------------------------------------------------------------------------------------------

def test_camera_health_is_counted_on_rank_0_only(ranks_of):
    """A camera and a landmark without information (zero prior, no active factor) on two ranks: per pass, the ranks' n_nonfinite and
    n_nonpd add up to the plain ctx's, and the camera is in rank 0's counts only (rank 1 reports the landmark, which it owns)."""
    infos, _ = ranks_of(2, HOST, "health", "ride")
    (one,), _ = ranks_of(1, 0, "one_rank", "ride")
    plain = [_unpack(h) for h in one["engines"]["health_plain"]["records"]]
    assert len(plain) == 6 and len(infos[0]["records"]) == 6
    r0 = [_unpack(h) for h in infos[0]["records"]]
    r1 = [_unpack(h) for h in infos[1]["records"]]
    for k in range(6):
        assert plain[k][5] + plain[k][6] >= 2, (k, plain[k])           # the two variables show in the plain ctx's health
        assert r0[k][5] + r1[k][5] == plain[k][5] and r0[k][6] + r1[k][6] == plain[k][6], (k, r0[k], r1[k], plain[k])
        assert r0[k][5] + r0[k][6] >= 1 and r1[k][5] + r1[k][6] >= 1, (k, r0[k], r1[k])      # the camera on rank 0, the landmark on rank 1
    assert infos[0]["describe"]["metric"]["path"] == "riding" and infos[1]["describe"]["metric"]["path"] == "riding"
    want, _ = ranks_of(2, HOST, "health", "perpass")
    for r in range(2):
        assert infos[r]["records"] == want[r]["records"], r


# ---- 7: the SLAM flow ----------------------------------------------------------------------------------------------------------------

def test_slam_flow_rides(ranks_of):
    """driver.run_slam on two ranks, transport 2: 23 sweeps, NEW_KEYFRAME before sweeps 8 and 16, the bursts between them through
    gbp_iterate_eval_each: trajectory and state equal the run that iterates and evaluates pass by pass."""
    got, want = ranks_of(2, HOST, "slam", "ride"), ranks_of(2, HOST, "slam", "perpass")
    for r in range(2):
        assert len(got[0][r]["traj"]) == 24 and got[0][r]["traj"] == want[0][r]["traj"], r
        _assert_same_state(_state(got[1], "r%d" % r), _state(want[1], "r%d" % r), ("slam", r))
        assert got[0][r]["describe"]["metric"]["path"] == "riding" and want[0][r]["describe"]["metric"]["path"] == "none"


# ---- 8: the executables --------------------------------------------------------------------------------------------------------------

def _cli(cmd, tmp_path, timeout=180):
    env = dict(os.environ, GC_PROFILE_LOG_DIR=str(tmp_path))
    p = subprocess.run(cmd + ["--profile", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(os.path.join(str(tmp_path), "gbp_profile.json")) as f:
        return p.stdout, json.load(f)


def _body(out, slam=False):
    keep = ("Initial", "Iters ", "Adding keyframe") if slam else ("Initial", "Weakening", "Iter ")
    return [l.strip() for l in out.splitlines() if l.strip().startswith(keep)]


_CLI = {}


def _cli_once(key, cmd, tmp_path):
    if key not in _CLI:
        try:
            _CLI[key] = _cli(cmd, tmp_path)
        except BaseException as e:
            _CLI[key] = e
    if isinstance(_CLI[key], BaseException):
        raise _CLI[key]
    return _CLI[key]


@pytest.mark.parametrize("transport", ["host-staged", "p2p"])
@pytest.mark.parametrize("world", [2, 4])
def test_ba_ipus_n_prints_the_same_run(world, transport, tmp_path_factory, oracle_mod, oracle_host):
    """`ba --ipus N` at the default --eval_every 1: bursts through gbp_ba_loop, the records summed over the ranks in the shared area.  The
    lines are those of the run whose library loop stays per pass (p2p-slices) — weakenings, iterations, relinearising sweeps (17+) —, the
    N-shard oracle's trajectory to print precision with exact counts, and --profile shows the riding path."""
    from tests.test_cli import _oracle_sharded_traj
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "24", "--ipus", str(world)]
    out, prof = _cli_once((world, transport), base + ["--transport", transport], tmp_path_factory.mktemp("cli"))
    ref, ref_prof = _cli_once((world, "p2p-slices"), base + ["--transport", "p2p-slices"], tmp_path_factory.mktemp("cli"))
    assert "Exchange between the %d ranks: %s" % (world, transport) in out
    assert _body(out) == _body(ref) and out.count("Weakening priors") == 5
    rows = [m.groups() for m in LINE.finditer(out)]
    assert len(rows) == 24 and sum(int(r[3]) for r in rows[17:]) > 0
    traj = _oracle_sharded_traj(oracle_mod, oracle_host, "fr2robot2", world, n_iters=24)
    for (it, m, c, nr, nb), (i, mean, cost, n_relin, n_robust) in zip(rows, traj[1:]):
        assert int(it) == i and abs(float(m) - mean) <= 2e-5 * mean, (i, m, mean)      # 6 printed digits
        assert int(nr) == n_relin and int(nb) == n_robust, (i, nr, n_relin, nb, n_robust)
    m = prof["comm"]["metric"]
    assert m["path"] == "riding" and m["passes_riding"] == 24 and m["passes_per_pass"] == 0, m
    assert ref_prof["comm"]["metric"]["path"] == "per-pass" and "p2p-slices" in ref_prof["comm"]["metric"]["reason"]


@pytest.mark.parametrize("transport", ["host-staged", "p2p"])
def test_slam_ipus_2_prints_the_same_run(transport, tmp_path_factory):
    """`slam --ipus 2`, a keyframe every 8 sweeps: within a keyframe interval the same bursts; keyframe and iteration lines equal those of
    the run whose library loop stays per pass, and --profile shows the riding path."""
    base = [SLAM, "--bal_file", seq_path("fr2robot2"), "--iters_between_kfs", "8", "--ipus", "2"]
    out, prof = _cli_once(("slam", transport), base + ["--transport", transport], tmp_path_factory.mktemp("cli"))
    ref, _ = _cli_once(("slam", "p2p-slices"), base + ["--transport", "p2p-slices"], tmp_path_factory.mktemp("cli"))
    assert len(_body(out, True)) == 1 + (19 * 8 - 1) + 18 and _body(out, True) == _body(ref, True)
    assert prof["comm"]["metric"]["path"] == "riding" and prof["comm"]["metric"]["passes_riding"] == 19 * 8 - 1
