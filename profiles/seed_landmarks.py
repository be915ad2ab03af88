"""One gbp_seed_landmarks call at S1 shape (1 000 cameras, 100 000 landmarks, 1 000 000 observations), timed with an event bracket:

    python profiles/seed_landmarks.py

The graph: the product's synthetic generator, seeded at the file's (noisy) cameras with the default options.  Five warm-up calls, then
twenty timed ones, each in its own event bracket on the current stream; prints the median, the fastest and the slowest as one JSON line
(profiles/seed_landmarks.md quotes it) and the status counts — for the default two refinement steps, then for one and for none."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from gbp_poplar_amd import hostlib, seed

C_, L, OBS = 1000, 100000, 10


def main():
    bal = hostlib.synth_generate(C_, L, OBS, 1)
    assert bal["n_edges"] == 1000000
    start, edges = seed.index(bal["lmk_id"], L)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
    cam_id, start, edges = dev(bal["cam_id"]), dev(start), dev(edges)
    cams = torch.from_numpy(bal["cameras"].astype(np.float32)).cuda()
    z = torch.from_numpy(bal["observations"].astype(np.float32)).cuda()
    K = [bal["fx"], 0, bal["cx"], 0, bal["fy"], bal["cy"], 0, 0, 1]
    ws = torch.empty(seed.workspace_bytes(C_) // 4, dtype=torch.float32, device="cuda")
    for refine_iters in (2, 1, 0):      # the default first; the others show what a Gauss-Newton step (a jac_hfunc per observation) costs
        options = seed.default_options(refine_iters=refine_iters)
        out = None
        times = []
        for i in range(25):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = seed.landmarks(cam_id, start, edges, K, cams, z, options=options, out=out, workspace=ws)
            t1.record()
            t1.synchronize()
            if i >= 5:
                times.append(t0.elapsed_time(t1))
        st = out["status"].cpu().numpy()
        print(json.dumps({"shape": [C_, L, int(bal["n_edges"])], "refine_iters": refine_iters, "calls": len(times),
                          "median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)),
                          "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                          "max_views": int(out["n_views"].max())}), flush=True)


if __name__ == "__main__":
    main()
