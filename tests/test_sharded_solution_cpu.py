"""ShardedGbp.read(gather=True) / read_priors(gather=True) on CPU: gloo ranks over the oracle-backed rank engine (as
tests/test_distributed_gloo.py).  Every rank gets COMPLETE arrays — cameras from its own copy, landmark entries from the rank that
owns them, per-factor entries from the rank that owns the factor's landmark — equal, bit for bit, to the single oracle's read in the
same shard order; entries are copied, so a -0.0 or a NaN keeps its bits; the default read() is what it was."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATE = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
PRIORS = ("cam_priors_eta", "cam_priors_lambda", "lmk_priors_eta", "lmk_priors_lambda")
NAN_BITS = 0x7FC12345            # a quiet NaN with a payload


def _graph(world):
    """(bal, bounds, n_iters): world 2 — the graph and partition of test_distributed_gloo.py; world 3 — the shape of
    test_empty_landmark_shard with the MIDDLE rank's range empty"""
    from gbp_poplar_amd import hostlib
    from gbp_poplar_amd.distributed import landmark_partition
    if world == 2:
        bal = hostlib.synth_generate(14, 260, 5, 5)
        return bal, landmark_partition(bal["lmk_id"], bal["n_lmks"], world), 22
    bal = hostlib.synth_generate(6, 40, 3, 9)
    return bal, np.asarray([0, 17, 17, bal["n_lmks"]], np.uint32), 6


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from tests.oracle_shard_engine import OracleShardEngine
    bal, bounds, n_iters = _graph(world)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])

    def engine():
        return OracleShardEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, (rank, world, lo, hi))

    run = ShardedGbp(engine(), bal["n_cams"], rank, world, dist=dist, device="cpu")
    driver.run_ba(run, state, opts, n_iters=n_iters, eval_every=1)
    out = {"bounds": bounds}
    out.update({"plain_" + k: v for k, v in run.read().items()})             # the default: the rank's own view ...
    out.update({"engine_" + k: v for k, v in run.e.read().items()})          # ... which is the engine's
    out.update({"g_" + k: v for k, v in run.read(gather=True).items()})
    out.update({"g_" + k: v for k, v in run.read_priors(gather=True).items()})
    out.update({"plainp_" + k: v for k, v in run.read_priors().items()})
    out.update({"enginep_" + k: v for k, v in run.e.read_priors().items()})
    if world == 2:
        # bits survive: rank 0 alone uploads a -0.0 and a NaN with a payload in the prior eta of its first landmark; ownership handed
        # in through the constructor this time
        st = dict(state)
        if rank == 0:
            eta = state["lmk_priors_eta"].copy()
            eta[3 * lo] = -0.0
            eta[3 * lo + 1:3 * lo + 2].view(np.uint32)[0] = NAN_BITS
            st["lmk_priors_eta"] = eta
        other = ShardedGbp(engine(), bal["n_cams"], rank, world, dist=dist, device="cpu", lmk_id=bal["lmk_id"], lmk_range=(lo, hi))
        other.upload(st)
        out["bits_lmk_priors_eta"] = other.read_priors(gather=True)["lmk_priors_eta"]
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, port):
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, port, d), nprocs=world, join=True)
        res = [np.load(os.path.join(d, "rank%d.npz" % r)) for r in range(world)]
        return [{k: x[k] for k in x.files} for x in res]


def _oracle(world):
    """read() and read_priors() of the single oracle in `world`-shard order after the same run"""
    from gbp_poplar_amd import driver, hostlib
    from oracle import oracle as orc
    bal, bounds, n_iters = _graph(world)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    ref = orc.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    ref.set_sum_order(1, bounds)
    driver.run_ba(ref, state, opts, n_iters=n_iters, eval_every=1)
    want = ref.read()
    want.update(ref.read_priors())
    return bal, want


@pytest.fixture(scope="module")
def two_ranks():
    return _spawn(2, 33500 + (os.getpid() % 2000)), _oracle(2)


@pytest.fixture(scope="module")
def three_ranks():
    return _spawn(3, 35500 + (os.getpid() % 2000)), _oracle(3)


def _assert_complete(res, want, bal):
    for k in STATE + PRIORS:
        for r in range(1, len(res)):
            assert res[r]["g_" + k].tobytes() == res[0]["g_" + k].tobytes(), (k, r)
        assert res[0]["g_" + k].dtype == want[k].dtype and res[0]["g_" + k].tobytes() == want[k].tobytes(), k
    assert np.any(want["lmk_beliefs_eta"] != 0) and np.any(want["damping_count"] != -15)      # (the run moved them)


def test_gathered_read_is_complete_and_equal_on_two_ranks(two_ranks):
    """World 2, 22 iterations of run_ba: read(gather=True) and read_priors(gather=True) are the same bytes on both ranks and the
    single oracle's in 2-shard order, all seven state members and all four priors."""
    res, (bal, want) = two_ranks
    bounds = res[0]["bounds"]
    assert 0 < bounds[1] < bal["n_lmks"]
    _assert_complete(res, want, bal)
    assert np.any(want["damping"] != 0)          # (the damped iterations from 15 on are inside the run)


def test_gathered_read_with_an_empty_range(three_ranks):
    """World 3, the middle rank owns no landmark and no factor: the gather still hands every rank the complete arrays."""
    res, (bal, want) = three_ranks
    assert list(res[0]["bounds"]) == [0, 17, 17, bal["n_lmks"]]
    _assert_complete(res, want, bal)


def test_default_read_is_the_local_view(two_ranks):
    """read() / read_priors() without arguments return what they returned before: the engine's own read, untouched."""
    res, (bal, want) = two_ranks
    bounds = res[0]["bounds"]
    for r in range(2):
        for k in STATE:
            assert res[r]["plain_" + k].tobytes() == res[r]["engine_" + k].tobytes(), (k, r)
        for k in PRIORS:
            assert res[r]["plainp_" + k].tobytes() == res[r]["enginep_" + k].tobytes(), (k, r)
        # ... and the local view is not the complete one: the other rank's landmark priors are not in it
        lo, hi = int(bounds[1 - r]), int(bounds[2 - r])
        assert not np.array_equal(res[r]["plainp_lmk_priors_lambda"][9 * lo:9 * hi], want["lmk_priors_lambda"][9 * lo:9 * hi])


def test_bits_survive_the_gather(two_ranks):
    """A -0.0 and a NaN with a payload that only rank 0 uploaded, in a landmark it owns, arrive on rank 1 with their bits."""
    res, _ = two_ranks
    for r in range(2):
        got = res[r]["bits_lmk_priors_eta"].view(np.uint32)
        assert got[0] == 0x80000000 and got[1] == NAN_BITS, (r, hex(got[0]), hex(got[1]))
        assert got[2] != 0x80000000


class _NoOwnership:
    """an engine that keeps neither the problem nor its shard"""

    def set_exchange_buffers(self, send, recv):
        pass

    def read(self):
        return {"lmk_beliefs_eta": np.zeros(6, np.float32)}

    def read_priors(self):
        return {"lmk_priors_eta": np.zeros(6, np.float32)}


def test_gather_without_ownership_information_raises():
    from gbp_poplar_amd.distributed import ShardedGbp
    not_used = object()      # the error comes before any collective
    run = ShardedGbp(_NoOwnership(), 1, 0, 2, dist=not_used, device="cpu")
    with pytest.raises(ValueError, match="lmk_id"):
        run.read(gather=True)
    with pytest.raises(ValueError, match="lmk_id"):
        run.read_priors(gather=True)
    only_range = ShardedGbp(_NoOwnership(), 1, 0, 2, dist=not_used, device="cpu", lmk_range=(0, 1))
    with pytest.raises(ValueError, match="lmk_id"):
        only_range.read(gather=True)
    assert run.read()["lmk_beliefs_eta"].shape == (6,)
    # one rank, or no collective at all: the gathered read is the plain one
    assert ShardedGbp(_NoOwnership(), 1, 0, 1, dist=not_used, device="cpu").read(gather=True)["lmk_beliefs_eta"].shape == (6,)
    assert ShardedGbp(_NoOwnership(), 1, 0, 2, dist=None, device="cpu").read_priors(gather=True)["lmk_priors_eta"].shape == (6,)
