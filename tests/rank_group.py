"""Rank groups for the multi-process transport tests: `world` fresh Python processes that share one rendezvous region in /dev/shm.

The launcher side (RankGroups.run_ranks, RankGroups.ranks_of) starts the ranks as

    python -m MODULE REGION RANK WORLD OUT_DIR ARGS...

(REGION "-": a run that needs no region), polls all of them, and on the first rank that fails, or at the deadline, aborts the region so
that the ranks waiting in a barrier leave by themselves, ends what is left and refuses every later run: after a rank has died nothing
further is started.  The worker side (rank_engine, write_rank) is the block every worker runs round its scenario: shard engine, mapped
region, communicator, the abort flag on an exception, the engine closed before the region is unmapped.

GROUPS is the instance the GPU suites share, with it the stop state and the cache of runs: a run that two suites ask for in one session
happens once, and nothing is run twice."""
import contextlib
import ctypes
import json
import mmap
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRACE_S = 10.0          # what the ranks get to leave by themselves once the region is aborted


@contextlib.contextmanager
def mapped_region(path):
    """the address of the region file `path`, mapped shared for the length of the block"""
    fd = os.open(path, os.O_RDWR)
    try:
        mm = mmap.mmap(fd, 0)
    finally:
        os.close(fd)
    buf = ctypes.c_char.from_buffer(mm)
    try:
        yield ctypes.addressof(buf)
    finally:
        del buf
        mm.close()


# ---- the launcher side ------------------------------------------------------------------------------------------------------------

def load_ranks(out_dir, world):
    """what the ranks wrote with write_rank: per rank ({array name: ndarray}, info)"""
    ranks = []
    for r in range(world):
        end = "_r%d.npy" % r
        arrays = {f[:-len(end)]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir) if f.endswith(end)}
        with open(os.path.join(out_dir, "info_r%d.json" % r)) as f:
            ranks.append((arrays, json.load(f)))
    return ranks


class RankGroups:
    def __init__(self, grace=GRACE_S):
        self.grace = grace
        self.stopped = None     # the first failure: a rank failed or hung once, nothing further is started
        self.n_runs = 0         # rank groups started
        self.last_procs = []    # the ranks of the last one, all of them ended
        self._runs = {}         # (module, world, args) -> (ranks, out_dir), or the exception of the one attempt

    def run_ranks(self, module, world, args, out_dir, n_cams, timeout):
        """Runs `world` ranks of `module` over a fresh region for `n_cams` cameras (None: no region) -> (load_ranks(...), out_dir)."""
        assert self.stopped is None, "an earlier run failed, nothing further is started: %s" % self.stopped
        from gbp_poplar_amd._lib import load
        lib = load()
        args = [str(a) for a in args]
        what = "%s %d %s" % (module, world, " ".join(args))
        os.makedirs(out_dir, exist_ok=True)
        self.n_runs += 1
        with contextlib.ExitStack() as stack:
            region, address = "-", None
            if n_cams is not None:
                size = int(lib.gbp_comm_region_bytes(n_cams, world))
                region = "/dev/shm/gbp_test_%d_%s" % (os.getpid(), what.replace(" ", "_").replace("/", "_"))
                with open(region, "wb") as f:
                    f.truncate(size)
                stack.callback(os.unlink, region)
                address = stack.enter_context(mapped_region(region))
                assert lib.gbp_comm_region_init(address, size, n_cams, world) == 0
            procs = self.last_procs = []
            stack.callback(self._end, procs, 0)         # whatever happens, no rank outlives the call
            for r in range(world):
                with open(os.path.join(out_dir, "stderr_r%d.txt" % r), "w") as log:
                    procs.append(subprocess.Popen([sys.executable, "-m", module, region, str(r), str(world), out_dir] + args, cwd=ROOT,
                                                  stdout=subprocess.DEVNULL, stderr=log))
            failure = self._wait(procs, timeout)
            if failure is not None:
                if address is not None:
                    lib.gbp_comm_region_abort(address)      # the abort flag lets a waiting rank leave by itself
                self._end(procs, self.grace)
                self.stopped = "%s (%s)" % (failure, what)
                tails = []
                for r in range(world):
                    with open(os.path.join(out_dir, "stderr_r%d.txt" % r), errors="replace") as f:
                        tails.append("rank %d: %s" % (r, f.read()[-1500:]))
                raise AssertionError(self.stopped + "\n" + "\n".join(tails))
        return load_ranks(out_dir, world), out_dir

    @staticmethod
    def _wait(procs, timeout):
        """polls every rank -> None once all have exited with 0, else what failed first"""
        world = len(procs)
        deadline = time.monotonic() + timeout
        left = set(range(world))
        while left:
            for r in sorted(left):
                rc = procs[r].poll()
                if rc is None:
                    continue
                left.discard(r)
                if rc != 0:
                    return "rank %d of %d exited with %d" % (r, world, rc)
            if left:
                if time.monotonic() > deadline:
                    return "ranks %s of %d still running after %d s" % (sorted(left), world, timeout)
                time.sleep(0.02)      # (waiting for processes, not for a time)
        return None

    @staticmethod
    def _end(procs, grace):
        end = time.monotonic() + grace
        for p in procs:
            try:
                p.wait(timeout=max(0.0, end - time.monotonic()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()

    def ranks_of(self, module, world, args, out_dir, n_cams, timeout):
        """run_ranks, made once per (module, world, args) and shared by everything that asks for it; a failed attempt is kept and raised
        again.  out_dir and n_cams are callables here, called only when the run is made."""
        key = (module, world, tuple(str(a) for a in args))
        if key not in self._runs:
            try:
                self._runs[key] = self.run_ranks(module, world, args, out_dir(), n_cams(), timeout)
            except BaseException as e:
                self._runs[key] = e
        if isinstance(self._runs[key], BaseException):
            raise self._runs[key]
        return self._runs[key]


GROUPS = RankGroups()


# ---- the worker side --------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def rank_engine(region_path, rank, world, transport, bal, K, bounds, before_init=None):
    """The shard engine of `rank` (landmarks bounds[rank] .. bounds[rank + 1] of the graph `bal`) with the library's communicator over
    `transport` attached through the region -> (engine, info).  before_init(engine) runs in front of gbp_comm_init.  info holds what
    gbp_comm_init took and left: init_s, last_error, describe, transport.  An exception raises the region's abort flag; the engine is
    always closed before the region is unmapped."""
    from gbp_poplar_amd._lib import load
    from gbp_poplar_amd.engine import GbpEngine
    lib = load()
    with mapped_region(region_path) as address:
        eng = None
        try:
            eng = GbpEngine(bal["cam_id"], bal["lmk_id"], int(bal["n_cams"]), int(bal["n_lmks"]), K,
                            shard=(rank, world, int(bounds[rank]), int(bounds[rank + 1])))
            if before_init is not None:
                before_init(eng)
            t0 = time.perf_counter()
            eng.comm_init(address, transport)
            yield eng, {"init_s": time.perf_counter() - t0, "last_error": eng.last_error(), "describe": eng.comm_describe(),
                        "transport": eng.comm_transport()}
        except BaseException:
            lib.gbp_comm_region_abort(address)     # wake the other ranks out of their barriers with an error
            raise
        finally:
            if eng is not None:
                eng.close()      # collective with a communicator: the peer transports meet the other ranks before they free their buffers


def write_rank(out_dir, rank, arrays, info):
    """OUT_DIR/<array>_r<RANK>.npy and OUT_DIR/info_r<RANK>.json, what load_ranks reads"""
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, "%s_r%d.npy" % (k, rank)), v)
    with open(os.path.join(out_dir, "info_r%d.json" % rank), "w") as f:
        json.dump(info, f)
