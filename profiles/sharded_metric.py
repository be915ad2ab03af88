"""What the loop with the metric costs on a ctx with a communicator, at config 5's shard shape (8 000 cameras x 125 000 landmarks x
1.25 M factors) on ONE GPU: profiles/sharded_metric.md.

    python profiles/sharded_metric.py [--configs host,rccl1,rccl2,p2p] [--passes 200] [--reps 3]      a 1-rank communicator per config
    python profiles/sharded_metric.py --world 2 [--passes 200]                                       two ranks on the one GPU, host-staged

Per config a fresh engine: upload, LINEARISE, 30 passes of warm-up, then `reps` times gbp_iterate(passes) + gbp_sync against
gbp_ba_loop(passes, ..., 0, out) with a host `out` (steps = 0: no weakening — the loop's body is iteration + metric), wall clock around
each.  Printed: us per pass of both, their ratio, and what gbp_comm_describe says about the metric's path (a build from before the
"metric" member prints "-").  GBP_LIB names another build of the library (the parent commit's, for the comparison: run the two
alternately).  Under `rocprofv3 --kernel-trace --stats -- python profiles/sharded_metric.py --reps 1` the per-kernel averages of the
belief kernels are the figures of the table's second half.  N = 2 shares one GPU between two processes: its lines show that the path runs,
they are no measurement of an exchange between GPUs."""
import argparse
import ctypes
import json
import mmap
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (8000, 125000, 10)      # cameras, landmarks, observations per landmark


def measure(eng, passes, reps):
    """[(us per pass of gbp_iterate, us per pass of gbp_ba_loop with the metric)] x reps"""
    eng.ba_loop(30, 100, 0)
    eng.iterate(30)
    eng.sync()
    rows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.iterate(passes)
        eng.sync()
        t1 = time.perf_counter()
        eng.ba_loop(passes, 100, 0)
        t2 = time.perf_counter()
        rows.append((1e6 * (t1 - t0) / passes, 1e6 * (t2 - t1) / passes))
    return rows


def report(name, eng, rows):
    try:
        m = eng.comm_describe().get("metric", {})
    except Exception:
        m = {}
    for it_us, loop_us in rows:
        print("%-22s iterate %8.2f us/pass   ba_loop+metric %8.2f us/pass   ratio %.3f   path %s" % (name, it_us, loop_us, loop_us / it_us, m.get("path", "-")), flush=True)


def inputs():
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.synth_generate(*SHAPE, 5)
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    return bal, K, state


def one_rank(configs, passes, reps):
    from gbp_poplar_amd.engine import GbpEngine
    bal, K, state = inputs()
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    for cfg in configs:
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=None if cfg == "plain" else (0, 1, 0, L))
        keep = None
        try:
            if cfg in ("rccl1", "rccl2"):
                eng.comm_init_rccl(eng.comm_unique_id())
                eng.comm_set_schedule(cfg == "rccl2")
            elif cfg != "plain":
                size = int(eng.lib.gbp_comm_region_bytes(C, 1))
                mm = mmap.mmap(-1, size)
                buf = (ctypes.c_char * size).from_buffer(mm)
                assert eng.lib.gbp_comm_region_init(ctypes.addressof(buf), size, C, 1) == 0
                keep = (mm, buf)
                eng.comm_init(ctypes.addressof(buf), {"host": 2, "p2p": 3}[cfg])
            eng.upload(state)
            eng.linearise()
            report("N=1 " + cfg, eng, measure(eng, passes, reps))
        finally:
            eng.close()
            del keep
    return 0


def rank_main(region_path, rank, world, passes):
    from gbp_poplar_amd import hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal, K, state = inputs()
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], C, L, world)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(rank, world, int(bounds[rank]), int(bounds[rank + 1])))
    size = int(eng.lib.gbp_comm_region_bytes(C, world))
    fd = os.open(region_path, os.O_RDWR)
    mm = mmap.mmap(fd, size)
    os.close(fd)
    buf = (ctypes.c_char * size).from_buffer(mm)
    try:
        eng.comm_init(ctypes.addressof(buf), 2)
        eng.upload(state)
        eng.linearise()
        rows = measure(eng, passes, 1)
        if rank == 0:
            report("N=%d host (one GPU)" % world, eng, rows)
    except BaseException:
        eng.lib.gbp_comm_region_abort(ctypes.addressof(buf))
        raise
    finally:
        eng.close()
        del buf
        mm.close()
    return 0


def many_ranks(world, passes, timeout=300):
    from gbp_poplar_amd._lib import load
    lib = load()
    C = SHAPE[0]
    size = int(lib.gbp_comm_region_bytes(C, world))
    region = "/dev/shm/gbp_sharded_metric_%d" % os.getpid()
    with open(region, "wb") as f:
        f.truncate(size)
    fd = os.open(region, os.O_RDWR)
    mm = mmap.mmap(fd, size)
    os.close(fd)
    buf = (ctypes.c_char * size).from_buffer(mm)
    procs = []
    try:
        assert lib.gbp_comm_region_init(ctypes.addressof(buf), size, C, world) == 0
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", region, str(r), str(world), str(passes)]) for r in range(world)]
        deadline = time.monotonic() + timeout
        for r, p in enumerate(procs):
            try:
                p.wait(timeout=max(1.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                pass
            if p.returncode != 0:
                lib.gbp_comm_region_abort(ctypes.addressof(buf))
                raise SystemExit("rank %d of %d failed: nothing further is run" % (r, world))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        del buf
        mm.close()
        os.unlink(region)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--rank":
        return rank_main(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="host,rccl1,rccl2")
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--world", type=int, default=1)
    a = ap.parse_args()
    print("library: %s" % (os.environ.get("GBP_LIB") or "in-tree"), flush=True)
    if a.world > 1:
        return many_ranks(a.world, a.passes)
    return one_rank(a.configs.split(","), a.passes, a.reps)


if __name__ == "__main__":
    sys.exit(main())
