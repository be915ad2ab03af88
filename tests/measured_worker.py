"""One rank of the measured-transport comparisons in tests/test_measured_transport.py, run as a fresh process:

    python -m tests.measured_worker REGION RANK WORLD TRANSPORT OUT_DIR SCENARIO

REGION is a file (in /dev/shm) that the test created and initialised with gbp_comm_region_init for WORLD ranks of fr2robot2.  The rank
builds its landmark shard, attaches the library's communicator over TRANSPORT (GbpEngine.comm_init) and runs the scenario:

    loop           LINEARISE, passes 0 .. 11 of the loop body through gbp_ba_loop with the metric after every pass (the five
                   weakenings inside), passes 12 .. 29 without the metric (the relinearising sweeps), gbp_eval_global
    upload_first   the same, but gbp_upload comes BEFORE gbp_comm_init: the measurement runs on an uploaded ctx
    slam           the SLAM flow (driver.run_slam) for 23 sweeps, NEW_KEYFRAME before sweeps 8 and 16

and writes its whole gbp_read state as OUT_DIR/<array>_r<RANK>.npy, and gbp_comm_describe, gbp_comm_transport, the text gbp_comm_init
left in gbp_last_error, what the call took and the scenario's records as OUT_DIR/info_r<RANK>.json."""
import ctypes
import json
import mmap
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    region_path, rank, world, transport, out_dir, scenario = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4], argv[5]
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=scenario == "slam")
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], C, L, world)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(rank, world, int(bounds[rank]), int(bounds[rank + 1])))
    size = int(eng.lib.gbp_comm_region_bytes(C, world))
    fd = os.open(region_path, os.O_RDWR)
    mm = mmap.mmap(fd, size)
    os.close(fd)
    buf = (ctypes.c_char * size).from_buffer(mm)
    try:
        if scenario == "upload_first":
            eng.upload(state)
        t0 = time.perf_counter()
        eng.comm_init(ctypes.addressof(buf), transport)
        info = {"init_s": time.perf_counter() - t0, "last_error": eng.last_error(), "describe": eng.comm_describe(),
                "transport": eng.comm_transport()}
        if scenario == "slam":
            info["traj"] = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=8, max_iters=23)
        else:
            if scenario != "upload_first":
                eng.upload(state)
            eng.linearise()
            info["loop"] = eng.ba_loop(12, 0, opts.steps)
            eng.ba_loop(18, 12, opts.steps, metrics=False)
            info["eval"] = eng.eval_global()
        st = eng.read()
        for k, v in st.items():
            np.save(os.path.join(out_dir, "%s_r%d.npy" % (k, rank)), v)
        with open(os.path.join(out_dir, "info_r%d.json" % rank), "w") as f:
            json.dump(info, f)
    except BaseException:
        eng.lib.gbp_comm_region_abort(ctypes.addressof(buf))     # wake the other ranks out of their barriers with an error
        raise
    finally:
        eng.close()              # collective with a communicator: the peer transports meet the other ranks before they free their buffers
        del buf
        mm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
