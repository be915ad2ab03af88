"""--out_file from multi-rank runs of `ba` / `slam` (csrc/cli_common.hpp: write_solution_ranks): the ranks read their beliefs into one
shared area, one barrier, rank 0 writes the file.  The file holds EVERY belief the run ends with (as means, printed with %.16e: doubles
exactly), so it is compared byte for byte: between the transports, and with the file written from the N-shard oracle's read() after the
same run — fr2robot2, 24 iterations, so that the relinearising sweeps from 17 on are inside."""
import os
import signal
import subprocess

import pytest

from tests.conftest import seq_path

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "gbp_poplar_amd", "bin", "ba")
SLAM = os.path.join(ROOT, "gbp_poplar_amd", "bin", "slam")
SEQ = "fr2robot2"
WRITTEN = "Refined problem written to"
FATAL = (124, 134, 137, 139)
_fatal = []      # the first run that ended on a signal or a time limit: nothing is started after it


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


def _cli(cmd, timeout=60):
    """(rc, stdout, stderr) of one run in a process group of its own.  A run that ends on a signal (its own or a rank's: 128 + signal
    from the supervisor), on 124 / 134 / 137 / 139 or at the time limit fails the test and every later run of this module."""
    if _fatal:
        pytest.fail("nothing more is started: " + _fatal[0])
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        _fatal.append("%s did not end within %d s" % (" ".join(cmd[:1] + cmd[3:]), timeout))
        pytest.fail(_fatal[0])
    rc = p.returncode
    if rc < 0 or rc in FATAL or 128 < rc < 255:
        _fatal.append("%s ended with status %d: %s" % (" ".join(cmd[:1] + cmd[3:]), rc, err[-1500:]))
        pytest.fail(_fatal[0])
    return rc, out, err


def _ba(out_file, *flags):
    return _cli([BA, "--bal_file", seq_path(SEQ), "--n_iters", "24", "--out_file", out_file] + list(flags))


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _oracle_file(oracle_mod, oracle_host, path, world, n_iters=None, slam_ibk=None):
    """The file of the reference-equivalent run in `world`-shard summation order, device conventions (tests/test_cli.py:
    _oracle_sharded_traj, with the oracle kept and read): hostlib.bal_write of hostlib.belief_means of its read()."""
    from gbp_poplar_amd import driver, hostlib
    bal = oracle_host.bal_read(seq_path(SEQ))
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, oracle_host, slam=slam_ibk is not None)
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], world)
    oracle_mod.set_trig_mode(1)
    try:
        o = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        o.set_sum_order(1, bounds)
        if slam_ibk is None:
            driver.run_ba(o, state, opts, n_iters=n_iters)
        else:
            driver.run_slam(o, oracle_host, bal, state, extra, opts, iters_between_kfs=slam_ibk)
        r = o.read()
    finally:
        oracle_mod.set_trig_mode(0)
    cams, pts = hostlib.belief_means(bal["n_cams"], bal["n_lmks"], r["cam_beliefs_eta"], r["cam_beliefs_lambda"],
                                     r["lmk_beliefs_eta"], r["lmk_beliefs_lambda"])
    hostlib.bal_write(path, dict(hostlib.bal_read(seq_path(SEQ)), cameras=cams, points=pts))
    return _bytes(path)


def _first_difference(a, b):
    la, lb = a.decode().splitlines(), b.decode().splitlines()
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d of %d / %d: %r != %r" % (i + 1, len(la), len(lb), x, y)
    return "%d lines != %d lines" % (len(la), len(lb))


@pytest.fixture(scope="module")
def two_rank_runs(tmp_path_factory):
    """`ba --ipus 2 --out_file` once per transport that ranks sharing a GPU can form: {transport: (rc, stdout, stderr, path)}"""
    d = tmp_path_factory.mktemp("ba2")
    runs = {}
    for t in ("host", "p2p", "p2p-slices"):
        path = str(d / (t + ".txt"))
        runs[t] = _ba(path, "--ipus", "2", "--transport", t) + (path,)
    return runs


def test_two_ranks_write_one_file_whatever_the_transport(two_rank_runs):
    files = {}
    for t, (rc, out, err, path) in two_rank_runs.items():
        assert rc == 0, (t, err[-2000:])
        assert out.count(WRITTEN) == 1 and WRITTEN + " " + path in out, (t, out[-500:])
        assert "Exchange between the 2 ranks: " + ("host-staged" if t == "host" else t) in out, t
        assert "is ignored" not in out
        files[t] = _bytes(path)
    assert files["p2p"] == files["host"], _first_difference(files["p2p"], files["host"])
    assert files["p2p-slices"] == files["host"], _first_difference(files["p2p-slices"], files["host"])


def test_two_rank_file_is_the_two_shard_oracles(two_rank_runs, oracle_mod, oracle_host, tmp_path):
    rc, _, err, path = two_rank_runs["host"]
    assert rc == 0, err[-2000:]
    got, want = _bytes(path), _oracle_file(oracle_mod, oracle_host, str(tmp_path / "oracle.txt"), 2, n_iters=24)
    assert got == want, _first_difference(got, want)
    # ... and it is a solution: read back in, it is the problem with other cameras and points
    from gbp_poplar_amd import hostlib
    import numpy as np
    a, b = hostlib.bal_read(seq_path(SEQ)), hostlib.bal_read(path)
    assert np.array_equal(a["lmk_id"], b["lmk_id"]) and np.array_equal(a["observations"], b["observations"])
    assert np.all(np.isfinite(b["points"])) and np.all(np.any(b["points"].reshape(-1, 3) != a["points"].reshape(-1, 3), axis=1))


def test_four_rank_file_is_the_four_shard_oracles(oracle_mod, oracle_host, tmp_path):
    path = str(tmp_path / "ba4.txt")
    rc, out, err = _ba(path, "--ipus", "4", "--transport", "host")
    assert rc == 0 and out.count(WRITTEN) == 1, err[-2000:]
    got, want = _bytes(path), _oracle_file(oracle_mod, oracle_host, str(tmp_path / "oracle.txt"), 4, n_iters=24)
    assert got == want, _first_difference(got, want)


def test_one_forked_rank_writes_the_single_process_file(tmp_path):
    """--force_sharded 1: fork, shard ctx, communicator, the shared result area — with one rank: the plain run's file."""
    plain, forked = str(tmp_path / "plain.txt"), str(tmp_path / "forked.txt")
    rc1, out1, err1 = _ba(plain)
    rc2, out2, err2 = _ba(forked, "--force_sharded", "1")
    assert rc1 == 0 and rc2 == 0, (err1[-500:], err2[-1500:])
    assert out1.count(WRITTEN) == 1 and out2.count(WRITTEN) == 1 and "Exchange between the 1 ranks" in out2
    assert _bytes(forked) == _bytes(plain), _first_difference(_bytes(forked), _bytes(plain))


def test_slam_two_rank_file_is_the_two_shard_oracles(oracle_mod, oracle_host, tmp_path):
    path = str(tmp_path / "slam2.txt")
    rc, out, err = _cli([SLAM, "--bal_file", seq_path(SEQ), "--iters_between_kfs", "8", "--ipus", "2", "--out_file", path])
    assert rc == 0 and out.count(WRITTEN) == 1 and out.count("Adding keyframe") == 18, err[-2000:]
    got, want = _bytes(path), _oracle_file(oracle_mod, oracle_host, str(tmp_path / "oracle.txt"), 2, slam_ibk=8)
    assert got == want, _first_difference(got, want)


def test_torchrun_example_writes_the_same_file(tmp_path, capsys):
    """examples/ba_torchrun.py --out_file on one GPU (no collective: the gathered read is the plain one): bin/ba's file."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ba_torchrun", os.path.join(ROOT, "examples", "ba_torchrun.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    mine, cli = str(tmp_path / "example.txt"), str(tmp_path / "cli.txt")
    assert example.main(["--bal_file", seq_path(SEQ), "--n_iters", "24", "--out_file", mine]) == 0
    assert capsys.readouterr().out.count(WRITTEN + " " + mine) == 1
    rc, _, err = _ba(cli)
    assert rc == 0, err[-1000:]
    assert _bytes(mine) == _bytes(cli), _first_difference(_bytes(mine), _bytes(cli))
    assert example.main(["--bal_file", seq_path(SEQ), "--n_iters", "2", "--out_file", "/nonexistent-dir/x.txt"]) == 1


class _ThreadGroup:
    """torch.distributed's all_gather_into_tensor between ShardedGbp objects of ONE process, one thread per rank (RCCL refuses ranks
    that share a GPU).  A rank that fails breaks the barrier for the others: nobody waits longer than the time limit."""

    def __init__(self, world):
        import threading
        self.slots, self.bar = [None] * world, threading.Barrier(world, timeout=30)

    def member(self, rank):
        import torch
        group = self

        class Member:
            def all_gather_into_tensor(self, recv, send):
                torch.cuda.current_stream().synchronize()
                group.slots[rank] = send
                group.bar.wait()
                recv.copy_(torch.cat(group.slots))
                torch.cuda.current_stream().synchronize()
                group.bar.wait()      # nobody replaces its slot before everyone has read it

        return Member()


def test_gathered_read_of_gpu_shards_is_the_sharded_oracles(oracle_mod):
    """ShardedGbp.read(gather=True) / read_priors(gather=True) over three GbpEngine shards on the GPU (their own streams; the middle
    rank's range empty; ownership taken from the engine): every rank gets the oracle's complete arrays in 3-shard order, bit for bit,
    after 20 passes of the loop body — all seven state members and the four priors."""
    import threading
    import numpy as np
    import torch
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    bal = hostlib.synth_generate(14, 260, 5, 5)
    C, L, world = bal["n_cams"], bal["n_lmks"], 3
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = [0, 101, 101, L]
    shards = [ShardedGbp(GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(r, world, bounds[r], bounds[r + 1])), C, r, world,
                         dist=None, device="cuda") for r in range(world)]

    def exchange():      # the all-gather of the camera partials, by device copies
        for sh in shards:
            sh.stream.synchronize()
        for dst in shards:
            for r, src in enumerate(shards):
                n = src.send.numel()
                dst.recv[r * n:(r + 1) * n].copy_(src.send)
        torch.cuda.synchronize()

    def everyone(*verbs):
        for sh in shards:
            for v in verbs:
                getattr(sh.e, v)()

    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], C, L, K)
        orc.set_sum_order(1, np.asarray(bounds, np.uint32))
        orc.upload(state)
        orc.linearise()
        for sh in shards:
            sh.e.upload(state)
        everyone("refresh_begin")
        exchange()
        everyone("refresh_end", "linearise_factors")
        for it in range(20):
            if (it + 1) % 2 == 0 and it < 2 * opts.steps:
                orc.weaken_priors()
                everyone("weaken_priors")
            orc.iterate(1)
            everyone("iterate_begin")
            exchange()
            everyone("iterate_end")
        want = orc.read()
        want.update(orc.read_priors())
    finally:
        oracle_mod.set_trig_mode(0)

    group = _ThreadGroup(world)
    got, errors = [None] * world, []

    def rank_reads(r):
        try:
            shards[r].dist = group.member(r)      # from here on the rank has a collective
            got[r] = dict(shards[r].read(gather=True), **shards[r].read_priors(gather=True))
        except Exception as exc:      # noqa: BLE001 - reported by the main thread
            errors.append((r, repr(exc)))
            group.bar.abort()

    threads = [threading.Thread(target=rank_reads, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(90)
    assert not errors and not any(t.is_alive() for t in threads), errors
    assert np.any(want["damping"] != 0) and np.any(want["lmk_beliefs_eta"] != 0)
    for r in range(world):
        for k, v in want.items():
            assert got[r][k].dtype == v.dtype and got[r][k].tobytes() == v.tobytes(), (r, k)


def test_a_file_that_cannot_be_written_is_status_1_on_every_rank():
    """The ranks all end (the call returns inside its time limit), the status is 1, nothing claims to have been written."""
    path = "/nonexistent-dir/x.txt"
    rc, out, err = _ba(path, "--ipus", "2")
    assert rc == 1, (rc, err[-1000:])
    assert "unable to write " + path in err and WRITTEN not in out and " Finished GBP." in out
    assert not os.path.exists(path)
