"""One rank of the bit-level transport comparison in tests/test_p2p_transport.py, run as a fresh process:

    python -m tests.p2p_worker REGION RANK WORLD TRANSPORT OUT_DIR

REGION is a file (in /dev/shm) that the test created and initialised with gbp_comm_region_init for WORLD ranks.  The rank builds its
landmark shard of fr2robot2, attaches the library's communicator over TRANSPORT, uploads, linearises, runs 30 iterations, weakens the
priors, runs 5 more, then writes its whole gbp_read state as OUT_DIR/<array>_r<RANK>.npy and the global metric, gbp_comm_describe and
gbp_comm_probe as OUT_DIR/info_r<RANK>.json."""
import ctypes
import json
import mmap
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    region_path, rank, world, transport, out_dir = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4]
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
        eng._chk(eng.lib.gbp_comm_init(eng.h, ctypes.addressof(buf), transport), "gbp_comm_init")
        eng.upload(state)
        eng.linearise()
        eng.iterate(30)
        eng.weaken_priors()
        eng.iterate(5)
        ev = eng.eval_global()
        info = {"eval": ev, "describe": eng.comm_describe(), "probe_us": eng.comm_probe(reps=5)}
        st = eng.read()
        for k, v in st.items():
            np.save(os.path.join(out_dir, "%s_r%d.npy" % (k, rank)), v)
        with open(os.path.join(out_dir, "info_r%d.json" % rank), "w") as f:
            json.dump(info, f)
    except BaseException:
        eng.lib.gbp_comm_region_abort(ctypes.addressof(buf))     # wake the other ranks out of their barriers with an error
        raise
    finally:
        eng.close()              # collective with a communicator: the p2p transport meets the other ranks before it frees its buffer
        del buf
        mm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
