"""Wall time of upload + sync and read + sync with host arrays and with device tensors (profiles/device_io.md).
    python profiles/device_io.py [--host-only] [--reps N]        one process, one GPU; S1 (1 000 x 100 000 x 1 000 000) and fr2robot2
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/device_io.py --reps 5     kernel durations of the same calls"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gbp_poplar_amd import driver, hostlib                       # noqa: E402
from gbp_poplar_amd.engine import GbpEngine                      # noqa: E402


def timed(fn, eng, reps):
    ts = []
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 15
    host_only = "--host-only" in sys.argv
    for name in ("fr2robot2", "S1"):
        bal = hostlib.synth_generate(1000, 100000, 10, 20200303) if name == "S1" else hostlib.bal_read(os.path.join(ROOT, "data", "sequences", name + ".txt"))
        K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        eng.upload(state)
        eng.linearise()
        eng.iterate(5)
        eng.read()
        out = {"graph": name, "E": int(bal["n_edges"]), "reps": reps,
               "upload_host": timed(lambda: eng.upload(state), eng, reps), "read_host": timed(eng.read, eng, reps)}
        if not host_only:
            import torch
            dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in state.items()}
            bufs = eng.read(device=True)
            torch.cuda.synchronize()
            eng.upload(dev)
            out["upload_device"] = timed(lambda: eng.upload(dev), eng, reps)
            out["read_device"] = timed(lambda: eng.read(out=bufs), eng, reps)
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
