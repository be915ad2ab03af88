"""The two kernels of the solution readout at S1 shape (1 000 cameras, 100 000 landmarks, 1 000 000 observations), for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/post_readout.py

Beliefs: random SPD blocks (the kernels' work does not depend on the values); the graph: the product's synthetic generator.  Three
launches of each kernel; profiles/post_readout.md quotes the trace."""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from gbp_poplar_amd import hostlib, post

C_, L, OBS = 1000, 100000, 10


def spd(n, w, rng):
    a = rng.normal(size=(n, w, w)).astype(np.float32)
    return (a @ a.transpose(0, 2, 1) + w * np.eye(w, dtype=np.float32)).astype(np.float32)


def main():
    rng = np.random.default_rng(1)
    bal = hostlib.synth_generate(C_, L, OBS, 1)
    assert bal["n_edges"] == 1000000
    b = {"cam_beliefs_eta": rng.normal(size=6 * C_), "cam_beliefs_lambda": spd(C_, 6, rng), "lmk_beliefs_eta": rng.normal(size=3 * L),
         "lmk_beliefs_lambda": spd(L, 3, rng)}
    b = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32).ravel()).cuda() for k, v in b.items()}
    ids = [torch.from_numpy(bal[k].view(np.int32).copy()).cuda() for k in ("cam_id", "lmk_id")]
    z = torch.from_numpy(bal["observations"].astype(np.float32)).cuda()
    K = [bal["fx"], 0, bal["cx"], 0, bal["fy"], bal["cy"], 0, 0, 1]
    for _ in range(3):
        m = post.moments(b)
        r = post.residuals(ids[0], ids[1], K, m, z, covs=m)
    torch.cuda.synchronize()
    print("status words set:", int((m["cam_status"] != 0).sum()), int((m["lmk_status"] != 0).sum()), "residual checksum", float(r["residual"].abs().sum()))


if __name__ == "__main__":
    main()
