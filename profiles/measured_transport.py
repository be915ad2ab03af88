"""What gbp_comm_init costs per transport, ranks as real processes on the visible GPU(s): profiles/measured_transport.md.

    python profiles/measured_transport.py [--worlds 2,4] [--transports 2,5] [--runs 3]

For every world size, transport and run: `world` fresh processes build their landmark shard of fr2robot2, meet at a barrier of the
region (gbp_comm_region_selftest: the ranks' start-up skew stays out of the figure), then time gbp_comm_init(ctx, region, transport).
Printed per run: the call's wall time on every rank, and for transport 5 the table gbp_comm_describe recorded.  GBP_LIB names another
build of the library (the parent commit's, for the comparison).  One rank failing ends the run: the region is aborted, nothing is
retried."""
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


def rank_main(region_path, rank, world, transport):
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], C, L, world)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(rank, world, int(bounds[rank]), int(bounds[rank + 1])))
    size = int(eng.lib.gbp_comm_region_bytes(C, world))
    fd = os.open(region_path, os.O_RDWR)
    mm = mmap.mmap(fd, size)
    os.close(fd)
    buf = (ctypes.c_char * size).from_buffer(mm)
    try:
        # (two rounds = an even number of region barriers: a build from before transport 5 starts its barrier sense from zero)
        assert eng.lib.gbp_comm_region_selftest(ctypes.addressof(buf), rank, world, 2) == 0
        t0 = time.perf_counter()
        eng._chk(eng.lib.gbp_comm_init(eng.h, ctypes.addressof(buf), transport), "gbp_comm_init")
        init_ms = 1e3 * (time.perf_counter() - t0)
        eng.upload(state)
        eng.linearise()
        eng.iterate(10)
        ev = eng.eval_global()
        print(json.dumps({"rank": rank, "init_ms": init_ms, "describe": eng.comm_describe(), "mean_reproj": ev["sum_norm"] / ev["n_active"]}), flush=True)
    except BaseException:
        eng.lib.gbp_comm_region_abort(ctypes.addressof(buf))
        raise
    finally:
        eng.close()
        del buf
        mm.close()
    return 0


def one_run(world, transport, timeout=120):
    from gbp_poplar_amd import hostlib
    from gbp_poplar_amd._lib import load
    lib = load()
    C = int(hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))["n_cams"])
    size = int(lib.gbp_comm_region_bytes(C, world))
    region = "/dev/shm/gbp_measured_profile_%d" % os.getpid()
    with open(region, "wb") as f:
        f.truncate(size)
    fd = os.open(region, os.O_RDWR)
    mm = mmap.mmap(fd, size)
    os.close(fd)
    buf = (ctypes.c_char * size).from_buffer(mm)
    procs = []
    try:
        assert lib.gbp_comm_region_init(ctypes.addressof(buf), size, C, world) == 0
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", region, str(r), str(world), str(transport)],
                                  stdout=subprocess.PIPE, text=True) for r in range(world)]
        deadline = time.monotonic() + timeout
        outs = []
        for r, p in enumerate(procs):
            try:
                out, _ = p.communicate(timeout=max(1.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                out = None
            if out is None or p.returncode != 0:
                lib.gbp_comm_region_abort(ctypes.addressof(buf))
                raise SystemExit("rank %d of %d (transport %d) failed: nothing further is run" % (r, world, transport))
            outs.append(json.loads(out.strip().splitlines()[-1]))
        return outs
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
        del buf
        mm.close()
        os.unlink(region)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--rank":
        return rank_main(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="2,4")
    ap.add_argument("--transports", default="2,5")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    print("library: %s" % (os.environ.get("GBP_LIB") or "in-tree"))
    for world in [int(w) for w in a.worlds.split(",")]:
        for run in range(a.runs):
            for transport in [int(t) for t in a.transports.split(",")]:      # alternated run by run
                outs = one_run(world, transport)
                d = outs[0]["describe"]
                print("N=%d transport=%d run=%d: gbp_comm_init %s ms per rank (max %.2f); attached %s; mean reproj after 10 it. %.6f"
                      % (world, transport, run, " ".join("%.2f" % o["init_ms"] for o in outs), max(o["init_ms"] for o in outs),
                         d["transport"], outs[0]["mean_reproj"]))
                for e in d.get("measured", []):
                    if e["eligible"]:
                        print("    %-11s %9.3f us per exchange (max over ranks), %d reps%s%s" % (
                            e["transport"], e["us_per_exchange"], e["reps"],
                            " — baseline: first %.3f, last %.3f" % (e["us_first"], e["us_last"]) if e.get("baseline") else "",
                            " — chosen" if e.get("chosen") else ""))
                    else:
                        print("    %-11s not eligible: %s" % (e["transport"], e["reason"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
