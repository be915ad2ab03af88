"""What profiles/locate_cameras.md quotes, measured on one GPU:

    python profiles/locate_cameras.py [timing] [sequences]

timing     one gbp_locate_cameras call at S1 shape (1 000 cameras x 1 000 observations, 100 000 landmarks): the product's synthetic
           generator, the file's (noisy) observations against the file's points, default options, every output requested.  Five warm-up
           calls, then twenty timed ones, each in its own event bracket on the current stream; the median.  Then the same with
           rounds = 1, whose difference from the default's four rounds is three rounds of generating and scoring, and with the
           observations cut to 64 per camera (the register-resident path).  One JSON line each.
sequences  the three shipped sequences: bundle adjustment to its default end, then every camera with 20 views or more located with no
           guess against the solved points: the located share, the inlier share, the distance to the solved pose, the time of the call.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from gbp_poplar_amd import hostlib, locate, resect
from profiles.resect_cameras import solved_map


def timed(call, warm=5, reps=20):
    times = []
    for i in range(warm + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = call()
        t1.record()
        t1.synchronize()
        if i >= warm:
            times.append(t0.elapsed_time(t1))
    return res, times


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int32) if a.dtype == np.uint32 else a).copy()).cuda()


def timing():
    C_, L, OBS = 1000, 100000, 10
    bal = hostlib.synth_generate(C_, L, OBS, 1)
    assert bal["n_edges"] == 1000000
    start, edges = resect.index(bal["cam_id"], C_)
    lmk_id, pts, z = dev(bal["lmk_id"].astype(np.uint32)), dev(bal["points"].astype(np.float32)), dev(bal["observations"].astype(np.float32))
    K = [bal["fx"], 0, bal["cx"], 0, bal["fy"], bal["cy"], 0, 0, 1]
    short = np.minimum(start[:-1].astype(np.int64) + 64, start[1:])      # the first 64 entries of every camera: select by active_flag
    keep = np.zeros(bal["n_edges"], np.uint32)
    for c in range(C_):
        keep[edges[start[c]:short[c]]] = 1
    d_start, d_edges = dev(start), dev(edges)
    for label, rounds, active in (("default", 4, None), ("rounds_1", 1, None), ("64_views_active", 4, dev(keep))):
        options = locate.default_options(rounds=rounds)
        out = locate.cameras(lmk_id, d_start, d_edges, K, pts, z, active_flag=active, options=options)      # the outputs, allocated once
        res, times = timed(lambda: locate.cameras(lmk_id, d_start, d_edges, K, pts, z, active_flag=active, options=options, out=out))
        st, rep = res["status"].cpu().numpy(), res["report"].cpu().numpy().reshape(-1, 4)
        print(json.dumps({"what": "timing", "case": label, "shape": [C_, L, int(bal["n_edges"])], "rounds": rounds, "calls": len(times),
                          "median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)),
                          "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                          "candidates_scored_mean": float(rep[:, 2].mean()), "n_views_mean": float(res["n_views"].cpu().numpy().mean()),
                          "inlier_share_mean": float((res["n_inliers"].cpu().numpy() / np.maximum(res["n_views"].cpu().numpy(), 1)).mean())}), flush=True)


def sequences():
    for name in ("fr1xyz", "fr1desk", "fr2robot2"):
        bal, K, cams, pts, z = solved_map(name)
        n_c = bal["n_cams"]
        idx = resect.index(bal["cam_id"], n_c)
        n = np.bincount(bal["cam_id"], minlength=n_c)
        select = (n >= 20).astype(np.uint32)
        d = [dev(np.asarray(a, np.uint32)) for a in (bal["lmk_id"],) + tuple(idx)] + [dev(pts), dev(np.asarray(z, np.float32)), dev(select)]
        res, times = timed(lambda: locate.cameras(d[0], d[1], d[2], K, d[3], d[4], select=d[5]))
        r = {k: v.cpu().numpy() for k, v in res.items()}
        sel = select == 1
        located = sel & ((r["status"].view(np.uint32) & locate.NOT_LOCATED) == 0)
        x = r["cam_mean"].reshape(-1, 6)
        print(json.dumps({"what": "sequence", "sequence": name, "cameras": int(n_c), "with_20_views": int(sel.sum()), "located": int(located.sum()),
                          "views_min_median_max": [int(n[sel].min()), float(np.median(n[sel])), int(n[sel].max())],
                          "inlier_share_min_median": [float((r["n_inliers"][located] / r["n_views"][located]).min()),
                                                      float(np.median(r["n_inliers"][located] / r["n_views"][located]))],
                          "pose_distance_to_solved_max": float(np.abs(x[located] - cams[located]).max()),
                          "mean_squared_inlier_error_max": float(r["report"].reshape(-1, 4)[located, 3].max()),
                          "median_ms": float(np.median(times)), "min_ms": float(min(times))}), flush=True)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["timing", "sequences"]:
        {"timing": timing, "sequences": sequences}[w]()
