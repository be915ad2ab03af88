"""The sliced peer-memory transport of the sharded camera exchange (`gbp_comm_init(ctx, region, 4)`, `--transport p2p-slices`): the cameras
are cut into `world` slices, rank s alone sums slice s out of its peers' partial sums (HIP IPC) and runs the camera chain behind the sum,
the other ranks gather the finished records — two host barriers per exchange.  Whatever it runs must leave the bits of the host-staged
transport (2) on the same shards: forked ranks on one GPU are separate processes, so IPC maps one process's buffers into another's
exactly as across peer GPUs.  The ranks are fresh processes (tests/rank_worker.py) started by the launcher the multi-process suites
share (tests/rank_group.py); nothing is run twice."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import seq_path
from tests.rank_group import GROUPS
from tests.rank_worker import graph
from tests.test_cli import BA, LINE, ROOT, SLAM

STATE = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
HOST, SLICES = 2, 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


def run(cmd, timeout):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def _body(out, slam=False):
    """the lines that carry the run's numbers: initial metric, weakenings, per-iteration metric (slam: keyframes)"""
    keep = ("Initial", "Iters ", "Adding keyframe") if slam else ("Initial", "Weakening", "Iter ")
    return [l.strip() for l in out.splitlines() if l.strip().startswith(keep)]


# ---- CPU: the slices, the flag -----------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_slice_bounds_under_asan_ubsan(tmp_path):
    """slice_bounds for C in {0, 1, 3, 5, 64, 8000} x world in {1, 2, 3, 4, 8}: contiguous, monotone, [0, C) covered exactly once — a
    stand-alone program under ASan + UBSan (tests/sanitize/slice_bounds_main.cpp)."""
    exe = str(tmp_path / "slice_bounds")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           os.path.join(ROOT, "tests", "sanitize", "slice_bounds_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "slice_bounds: ok (108 slices)" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


def test_help_lists_p2p_slices_transport():
    for exe in (BA, SLAM):
        rc, out, _ = run([exe, "--help"], 60)
        assert rc == 0 and "auto | rccl | host | p2p | p2p-slices" in out, exe


def test_transport_p2p_slices_is_parsed():
    """--transport p2p-slices (and its number, 4) gets past the parser: the run then stops at the missing input file, not at the value."""
    for value in ("p2p-slices", "4"):
        rc, _, err = run([BA, "--transport", value], 60)
        assert rc == 1 and "--bal_file" in err and "invalid option value" not in err, (value, err)
    rc, _, err = run([SLAM, "--bal_file", "/nonexistent/file.txt", "--transport", "p2p-slices"], 60)
    assert rc == 1 and "unable to open file" in err and "invalid option value" not in err


# ---- GPU: real processes, the whole state bit for bit --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ranks_of(tmp_path_factory):
    """ranks_of(world, transport, scenario): the run, made once and shared by the tests that read it"""
    def get(world, transport, scenario):
        return GROUPS.ranks_of("tests.rank_worker", world, (transport, scenario), lambda: str(tmp_path_factory.mktemp("slices") / "run"),
                               lambda: int(graph(scenario)["n_cams"]), 240)[0]
    return get


def _assert_same_state(world, got, want):
    for r in range(world):
        for k in STATE:
            assert np.array_equal(got[r][0][k], want[r][0][k]), (r, k)
    for r in range(1, world):      # the replicated cameras agree across the ranks
        assert np.array_equal(got[r][0]["cam_beliefs_eta"], got[0][0]["cam_beliefs_eta"]), r
        assert np.array_equal(got[r][0]["cam_beliefs_lambda"], got[0][0]["cam_beliefs_lambda"]), r


@pytest.mark.gpu
def test_transport_4_is_p2p_slices(ranks_of):
    """gbp_comm_init(ctx, region, 4) succeeds on two real ranks; gbp_comm_transport and gbp_comm_describe name the transport."""
    for r, (_, info) in enumerate(ranks_of(2, SLICES, "loop")):
        assert info["transport"] == "p2p-slices"
        d = info["describe"]
        assert d["transport"] == "p2p-slices" and d["rank"] == r and d["world"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_loop_state_bit_identical_to_host_staged(world, ranks_of):
    """LINEARISE and 30 passes of the loop body (the five weakenings inside) on `world` real processes: every rank's beliefs, damping,
    damping counts and robust flags are the host-staged transport's, bit for bit, and all ranks hold the same camera beliefs."""
    _assert_same_state(world, ranks_of(world, SLICES, "loop"), ranks_of(world, HOST, "loop"))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_loop_state_equals_sharded_oracle(world, ranks_of, oracle_mod):
    """... and the oracle's in `world`-shard summation order: camera beliefs on every rank, landmark beliefs and factor state of its shard."""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], world)
    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1, bounds)
        orc.upload(state)
        orc.linearise()
        for it in range(30):
            if (it + 1) % 2 == 0 and it < 2 * opts.steps:
                orc.weaken_priors()
            orc.iterate(1)
        ro = orc.read()
    finally:
        oracle_mod.set_trig_mode(0)
    lmk = np.asarray(bal["lmk_id"])
    for r, (g, _) in enumerate(ranks_of(world, SLICES, "loop")):
        assert np.array_equal(g["cam_beliefs_eta"], ro["cam_beliefs_eta"]), r
        assert np.array_equal(g["cam_beliefs_lambda"], ro["cam_beliefs_lambda"]), r
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        assert np.array_equal(g["lmk_beliefs_eta"][3 * lo:3 * hi], ro["lmk_beliefs_eta"][3 * lo:3 * hi]), r
        assert np.array_equal(g["lmk_beliefs_lambda"][9 * lo:9 * hi], ro["lmk_beliefs_lambda"][9 * lo:9 * hi]), r
        own = (lmk >= lo) & (lmk < hi)
        assert np.array_equal(g["damping_count"][own], ro["damping_count"][own]), r
        assert np.array_equal(g["robust_flag"][own], ro["robust_flag"][own]), r


@pytest.mark.gpu
def test_metric_records_equal_host_staged(ranks_of):
    """N = 2: the per-pass metric of gbp_ba_loop with a host `out` (12 passes, the weakenings between them) and gbp_eval_global after
    the 30th pass equal the host-staged transport's records field for field; gbp_eval_global gives every rank the same sums."""
    got, want = ranks_of(2, SLICES, "loop"), ranks_of(2, HOST, "loop")
    for r in range(2):
        assert len(got[r][1]["loop"]) == 12
        assert got[r][1]["loop"] == want[r][1]["loop"], r
        assert got[r][1]["eval"] == want[r][1]["eval"], r
    assert got[0][1]["eval"] == got[1][1]["eval"] and got[0][1]["eval"]["n_active"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cams,lmks,world", [(5, 40, 2), (3, 24, 4)])
def test_slice_edges_bit_identical_to_host_staged(cams, lmks, world, ranks_of):
    """The smallest shapes at which a slice bound can go wrong — C = 5 over 2 ranks (slices of 2 and 3 cameras), C = 3 over 4 ranks
    (rank 0's slice is empty: it reduces nothing and gathers everything) — 12 passes of the loop body on a synthetic graph."""
    scenario = "synth:%d:%d" % (cams, lmks)
    got = ranks_of(world, SLICES, scenario)
    assert all(info["transport"] == "p2p-slices" for _, info in got)
    assert np.any(got[0][0]["cam_beliefs_eta"] != 0)
    _assert_same_state(world, got, ranks_of(world, HOST, scenario))
    for r in range(world):
        assert got[r][1]["loop"] == ranks_of(world, HOST, scenario)[r][1]["loop"], r


@pytest.mark.gpu
def test_slam_flow_bit_identical_to_host_staged(ranks_of):
    """The SLAM flow on N = 2: 23 sweeps, NEW_KEYFRAME (read priors and beliefs, new priors, the refresh through the full peer gather)
    in front of sweeps 8 and 16, the sliced iteration between them: state and trajectory are the host-staged transport's."""
    got, want = ranks_of(2, SLICES, "slam"), ranks_of(2, HOST, "slam")
    _assert_same_state(2, got, want)
    for r in range(2):
        assert len(got[r][1]["traj"]) == 24 and got[r][1]["traj"] == want[r][1]["traj"], r


@pytest.mark.gpu
def test_one_rank_equals_plain_ctx_bit_for_bit(ranks_of):
    """A 1-rank transport-4 communicator (one slice, nothing to reduce from or gather: no peer kernel is launched) leaves the state and
    the metric records of the plain single-GPU ctx after the same 30 passes."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    (got, info), = ranks_of(1, SLICES, "loop")
    assert info["transport"] == "p2p-slices"
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    try:
        eng.upload(state)
        eng.linearise()
        loop = eng.ba_loop(12, 0, opts.steps)
        eng.ba_loop(18, 12, opts.steps, metrics=False)
        ev = eng.eval()
        want = eng.read()
    finally:
        eng.close()
    for k in STATE:
        assert np.array_equal(got[k], want[k]), k
    assert info["loop"] == json.loads(json.dumps(loop)) and info["eval"] == json.loads(json.dumps(ev))


# ---- GPU: the executables ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_ba_ipus_2_p2p_slices_equals_host_staged():
    """`ba --ipus 2 --transport p2p-slices` through the five weakenings and the relinearising sweeps (17+): the host-staged run, line for line."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "24", "--ipus", "2"]
    rc_h, out_h, err_h = run(base + ["--transport", "host"], 120)
    rc_s, out_s, err_s = run(base + ["--transport", "p2p-slices"], 120)
    assert rc_h == 0, err_h[-2000:]
    assert rc_s == 0, err_s[-2000:]
    assert "Exchange between the 2 ranks: p2p-slices" in out_s
    body = _body(out_s)
    assert len(LINE.findall(out_s)) == 24 and sum(l.startswith("Weakening") for l in body) == 5
    assert body == _body(out_h)


@pytest.mark.gpu
def test_ba_ipus_8_p2p_slices_equals_host_staged():
    """Eight ranks on the one GPU, 20 iterations (peer transports stall in ~10 ms quanta from four processes on: few iterations, a
    time limit sized for tens of milliseconds per exchange): the host-staged trajectory."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "20", "--ipus", "8"]
    rc_h, out_h, err_h = run(base + ["--transport", "host"], 180)
    rc_s, out_s, err_s = run(base + ["--transport", "p2p-slices"], 180)
    assert rc_h == 0, err_h[-2000:]
    assert rc_s == 0, err_s[-2000:]
    assert "Exchange between the 8 ranks: p2p-slices" in out_s
    assert len(LINE.findall(out_s)) == 20 and _body(out_s) == _body(out_h)


@pytest.mark.gpu
def test_slam_ipus_2_p2p_slices_equals_host_staged():
    """`slam --ipus 2 --transport p2p-slices`: NEW_KEYFRAME after every 8 sweeps; keyframe and iteration lines equal the host-staged run's."""
    base = [SLAM, "--bal_file", seq_path("fr2robot2"), "--iters_between_kfs", "8", "--ipus", "2"]
    rc_h, out_h, err_h = run(base + ["--transport", "host"], 180)
    rc_s, out_s, err_s = run(base + ["--transport", "p2p-slices"], 180)
    assert rc_h == 0, err_h[-2000:]
    assert rc_s == 0, err_s[-2000:]
    assert "Exchange between the 2 ranks: p2p-slices" in out_s
    body = _body(out_s, slam=True)
    assert sum("Adding keyframe" in l for l in body) == 18 and sum(l.startswith("Iters ") for l in body) > 0
    assert body == _body(out_h, slam=True)


@pytest.mark.gpu
def test_p2p_slices_with_one_forked_rank_equals_plain_run():
    """--force_sharded 1 --transport p2p-slices: a 1-rank communicator (one slice, nothing to gather, no peer kernel): the plain ctx's run."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "60", "--eval_every", "20"]
    rc1, out1, err1 = run(base, 120)
    rc2, out2, err2 = run(base + ["--force_sharded", "1", "--transport", "p2p-slices"], 120)
    assert rc1 == 0 and rc2 == 0, (err1[-500:], err2[-1500:])
    assert "Exchange between the 1 ranks: p2p-slices" in out2
    assert LINE.findall(out1) == LINE.findall(out2) and len(LINE.findall(out1)) == 3
