"""What profiles/resect_cameras.md quotes, measured on one GPU:

    python profiles/resect_cameras.py [timing] [passes] [slam]

timing  one gbp_resect_cameras call at S1 shape (1 000 cameras x 1 000 observations, 100 000 landmarks): the product's synthetic
        generator, every camera started at the file's (noisy) pose against the file's points, default options, every output requested.
        Five warm-up calls, then twenty timed ones, each in its own event bracket on the current stream (the start poses are copied
        back in front of the bracket: the call updates them in place).  One JSON line.
passes  the three shipped sequences: bundle adjustment to its default end, then every camera c >= 1 from camera c - 1's solved pose
        against the solved points, with max_passes = 1 .. 10 and 30 — a run with budget p is the first p passes of a longer one, so the
        cost after p passes is read off the report.  Per sequence: the passes until every camera's cost is within 1e-3 (relative) of its
        cost after 30, the statuses, the reprojection errors.
slam    fr2robot2, the default 700 iterations between keyframes: kf_init copy against resect, for both lmk_init settings: the final
        mean reprojection error, cost and health counters.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from gbp_poplar_amd import _cabi, driver, hostlib, resect
from gbp_poplar_amd.engine import GbpEngine

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def sequence(name):
    return os.path.join(ROOT, "data", "sequences", name + ".txt")


def engine(bal, K):
    return GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults())


def timing():
    C_, L, OBS = 1000, 100000, 10
    bal = hostlib.synth_generate(C_, L, OBS, 1)
    assert bal["n_edges"] == 1000000
    start, edges = resect.index(bal["cam_id"], C_)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
    lmk_id, start, edges = dev(bal["lmk_id"]), dev(start), dev(edges)
    cams0 = torch.from_numpy(bal["cameras"].astype(np.float32)).cuda()
    pts = torch.from_numpy(bal["points"].astype(np.float32)).cuda()
    z = torch.from_numpy(bal["observations"].astype(np.float32)).cuda()
    lam = torch.eye(6, device="cuda").repeat(C_, 1).reshape(-1).contiguous()
    K = [bal["fx"], 0, bal["cx"], 0, bal["fy"], bal["cy"], 0, 0, 1]
    cams, out, times = cams0.clone(), None, []
    for i in range(25):
        cams.copy_(cams0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = resect.cameras(lmk_id, start, edges, K, cams, pts, z, priors_lambda=lam, out=out)
        t1.record()
        t1.synchronize()
        out = {k: v for k, v in res.items() if k != "cam_mean"}
        if i >= 5:
            times.append(t0.elapsed_time(t1))
    st, rep = res["status"].cpu().numpy(), res["report"].cpu().numpy().reshape(-1, 4)
    print(json.dumps({"what": "timing", "shape": [C_, L, int(bal["n_edges"])], "calls": len(times), "median_ms": float(np.median(times)),
                      "min_ms": float(min(times)), "max_ms": float(max(times)),
                      "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                      "cost_start_sum": float(rep[:, 0].sum()), "cost_final_sum": float(rep[:, 1].sum())}), flush=True)


def solved_map(name):
    bal = hostlib.bal_read(sequence(name))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = engine(bal, K)
    eng.upload(state)
    eng.linearise()
    done = 0
    while done < opts.n_iters:
        n = min(500, opts.n_iters - done)
        eng.ba_loop(n, done, int(opts.steps), metrics=False)
        done += n
    b = eng.read()
    eng.close()
    cams, pts = hostlib.belief_means(bal["n_cams"], bal["n_lmks"], b["cam_beliefs_eta"], b["cam_beliefs_lambda"], b["lmk_beliefs_eta"],
                                     b["lmk_beliefs_lambda"])
    return bal, K, np.asarray(cams).reshape(-1, 6), np.asarray(pts).astype(np.float32), state["measurements"]


def passes():
    for name in ("fr1xyz", "fr1desk", "fr2robot2"):
        bal, K, cams, pts, z = solved_map(name)
        n_c = bal["n_cams"]
        start = np.concatenate([cams[:1], cams[:-1]]).astype(np.float32)
        select = (np.arange(n_c) >= 1).astype(np.uint32)
        idx = resect.index(bal["cam_id"], n_c)
        cost = {}
        for p in list(range(1, 11)) + [30]:
            r = resect.cameras(bal["lmk_id"], *idx, K, start, pts, z, select=select, options=resect.default_options(max_passes=p))
            cost[p] = r["report"].reshape(-1, 4)[:, 1].astype(np.float64)
            if p == 10:
                r10 = r
        seen = (select == 1) & (r10["n_views"] >= 6)
        need = np.array([min(p for p in range(1, 11) if cost[p][c] <= cost[30][c] * (1 + 1e-3)) if cost[10][c] <= cost[30][c] * (1 + 1e-3) else 11
                         for c in np.flatnonzero(seen)])
        rep = r10["report"].reshape(-1, 4)[seen]
        print(json.dumps({"what": "passes", "sequence": name, "cameras": int(seen.sum()), "views_min_median_max": [int(r10["n_views"][seen].min()),
                          float(np.median(r10["n_views"][seen])), int(r10["n_views"][seen].max())],
                          "passes_max": int(need.max()), "passes_median": float(np.median(need)),
                          "passes_hist": {str(k): int(v) for k, v in zip(*np.unique(need, return_counts=True))},
                          "status_counts": {str(k): int(v) for k, v in zip(*np.unique(r10["status"][seen], return_counts=True))},
                          "cost_start_sum": float(rep[:, 0].sum()), "cost_final_sum": float(rep[:, 1].sum()),
                          "pose_distance_to_solved_max": float(np.abs(r10["cam_mean"].reshape(-1, 6)[seen] - cams[seen]).max()),
                          "start_distance_to_solved_max": float(np.abs(start[seen] - cams[seen]).max())}), flush=True)


def slam():
    bal = hostlib.bal_read(sequence("fr2robot2"))
    opts = driver.Options()
    for lmk_init in ("file", "triangulate"):
        for kf_init in ("copy", "resect"):
            K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init=lmk_init)
            eng = engine(bal, K)
            log = []
            traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, lmk_init=lmk_init, kf_init=kf_init, eval_every=700, log=log.append)
            ev = eng.eval()
            eng.close()
            said = [l for l in log if l.startswith("Keyframe ")]
            print(json.dumps({"what": "slam", "sequence": "fr2robot2", "lmk_init": lmk_init, "kf_init": kf_init, "final_px": traj[-1][1],
                              "final_cost": traj[-1][2], "n_nonfinite": int(ev["n_nonfinite"]), "n_nonpd": int(ev["n_nonpd"]),
                              "resected": sum("resected" in l for l in said), "copied": sum("copied" in l for l in said)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["timing", "passes", "slam"]
    for w in what:
        {"timing": timing, "passes": passes, "slam": slam}[w]()
