"""The policy of the rank-group launcher (tests/rank_group.py) on the CPU: real processes (tests/rank_selftest_worker.py) that meet in
the region's barriers through the host-only region calls, one of them misbehaving.  Every case has a harness instance of its own, so a
failure staged here bars nothing else."""
import glob
import os
import time

import pytest

from tests.rank_group import RankGroups

WORKER = "tests.rank_selftest_worker"
WORLD, N_CAMS, ROUNDS = 3, 10, 200


def _regions():
    return glob.glob("/dev/shm/gbp_test_%d_*" % os.getpid())


def test_well_behaved_ranks_return_their_info(tmp_path):
    g = RankGroups()
    ranks, out_dir = g.run_ranks(WORKER, WORLD, (ROUNDS, -1, "ok"), str(tmp_path / "run"), N_CAMS, 60)
    assert out_dir == str(tmp_path / "run")
    assert [info for _, info in ranks] == [{"rank": r, "rounds": ROUNDS} for r in range(WORLD)]
    assert [p.returncode for p in g.last_procs] == [0] * WORLD and g.stopped is None and g.n_runs == 1
    assert _regions() == []


def test_a_rank_that_fills_stderr_does_not_block(tmp_path):
    """1 MB on stderr, more than a pipe holds: it goes to a file, and the run succeeds"""
    g = RankGroups()
    ranks, out_dir = g.run_ranks(WORKER, WORLD, (ROUNDS, 1, "noisy"), str(tmp_path / "run"), N_CAMS, 60)
    assert len(ranks) == WORLD and g.stopped is None
    assert os.path.getsize(os.path.join(out_dir, "stderr_r1.txt")) == 1 << 20
    assert _regions() == []


def _assert_refuses_the_next_run(g, tmp_path, first):
    """after a failure: a further run raises at once, names the first failure and starts no process"""
    marker = str(tmp_path / "marker")
    n = g.n_runs
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as again:
        g.run_ranks(WORKER, WORLD, (ROUNDS, -1, "ok", marker), str(tmp_path / "next"), N_CAMS, 60)
    assert time.monotonic() - t0 < 1.0
    assert first in str(again.value) and g.n_runs == n and not os.path.exists(marker) and not os.path.exists(str(tmp_path / "next"))


def _assert_others_left_through_the_abort(g, bad):
    assert all(p.poll() is not None for p in g.last_procs)                                 # no child is left running
    assert all(p.returncode == 4 for r, p in enumerate(g.last_procs) if r != bad)         # by themselves, not by a signal
    assert _regions() == []


def test_first_failing_rank_aborts_the_region(tmp_path):
    """Rank 1 exits with 3 before its first barrier: ranks 0 and 2 wait for it there, and leave because the launcher aborts the region —
    well inside the 60 s deadline and the barrier's own 300 s."""
    g = RankGroups()
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        g.run_ranks(WORKER, WORLD, (ROUNDS, 1, "exit3"), str(tmp_path / "run"), N_CAMS, 60)
    assert time.monotonic() - t0 < 20.0
    text = str(e.value)
    assert "rank 1 of 3 exited with 3" in text and "rank 1 gives up before its first barrier" in text
    assert g.last_procs[1].returncode == 3
    _assert_others_left_through_the_abort(g, 1)
    _assert_refuses_the_next_run(g, tmp_path, "rank 1 of 3 exited with 3")


def test_deadline_aborts_the_region_and_ends_a_rank_that_never_arrives(tmp_path):
    """Rank 2 sleeps, deadline 3 s: the message says who was still running (all three: 0 and 1 wait for 2), ranks 0 and 1 leave through
    the abort, rank 2 is killed when the grace has passed (2 s here instead of the default 10: the path is the same)."""
    g = RankGroups(grace=2.0)
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        g.run_ranks(WORKER, WORLD, (ROUNDS, 2, "sleep"), str(tmp_path / "run"), N_CAMS, 3)
    assert time.monotonic() - t0 < 20.0
    assert "ranks [0, 1, 2] of 3 still running after 3 s" in str(e.value)
    assert g.last_procs[2].returncode < 0          # the one that had to be killed
    _assert_others_left_through_the_abort(g, 2)
    _assert_refuses_the_next_run(g, tmp_path, "ranks [0, 1, 2] of 3 still running after 3 s")


def test_one_run_per_key(tmp_path):
    g = RankGroups()
    dirs = iter([str(tmp_path / "a"), str(tmp_path / "b")])
    ask = lambda: g.ranks_of(WORKER, WORLD, (ROUNDS, -1, "ok"), lambda: next(dirs), lambda: N_CAMS, 60)
    first = ask()
    assert ask() is first and g.n_runs == 1 and first[1] == str(tmp_path / "a") and not os.path.exists(str(tmp_path / "b"))


def test_failed_attempt_is_raised_again_not_run_again(tmp_path):
    g = RankGroups()
    ask = lambda: g.ranks_of(WORKER, WORLD, (ROUNDS, 0, "exit3"), lambda: str(tmp_path / "run"), lambda: N_CAMS, 60)
    with pytest.raises(AssertionError) as first:
        ask()
    with pytest.raises(AssertionError) as second:
        ask()
    assert second.value is first.value and g.n_runs == 1 and "rank 0 of 3 exited with 3" in str(first.value)
