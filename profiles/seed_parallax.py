"""What min_parallax does on the shipped sequences (the table of profiles/seed_landmarks.md behind the header's default):

    python profiles/seed_parallax.py

Per sequence and per min_parallax: how seed.landmarks classifies the landmarks from ALL observations at the file's cameras (triangulated,
placed, triangulated but behind a camera), and the initial metric of a bundle adjustment started there.  For fr2robot2 with its
`points` section zeroed: the keyframe-by-keyframe run of driver.run_slam(lmk_init="triangulate") at each min_parallax — final mean
reprojection error, the final metric's health counters, the largest metric on the way — beside the file-initialised run of the
unchanged file.  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np

from gbp_poplar_amd import driver, hostlib, seed
from gbp_poplar_amd.engine import GbpEngine

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SWEEP = (1e-4, 1e-3, 5e-3, 2e-2)


def with_min_parallax(value):
    driver._seed_options = lambda opts: seed.default_options(reproj_meas_var=opts.reproj_meas_var, min_parallax=value)


def classify(bal, value):
    K = driver.k_matrix(bal)
    cams = np.asarray(bal["cameras"], np.float64).astype(np.float32)
    z = np.asarray(bal["observations"], np.float64).astype(np.float32)
    s = seed.landmarks(bal["cam_id"], *seed.index(bal["lmk_id"], int(bal["n_lmks"])), K, cams, z, options=seed.default_options(min_parallax=value))
    st = s["status"]
    placed = (st & (seed.ONE_VIEW | seed.LOW_PARALLAX | seed.NONFINITE)) != 0
    none = (st & seed.NO_VIEW) != 0
    tri = ~placed & ~none
    return {"triangulated": int(tri.sum()), "placed": int(placed.sum()), "no_view": int(none.sum()),
            "triangulated_behind": int((tri & ((st & seed.BEHIND) != 0)).sum()), "nonfinite": int(((st & seed.NONFINITE) != 0).sum())}


def engine(bal, K):
    return GbpEngine(bal["cam_id"], bal["lmk_id"], int(bal["n_cams"]), int(bal["n_lmks"]), K)


def slam(bal, lmk_init):
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init=lmk_init)
    eng = engine(bal, K)
    traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, lmk_init=lmk_init, eval_every=100)
    ev = eng.eval()
    eng.close()
    m = np.array([t[1] for t in traj])
    return {"final_mean_reproj_px": float(driver.metric(ev)[0]), "final_cost": float(ev["sum_half_sq"]), "n_nonfinite": int(ev["n_nonfinite"]),
            "n_nonpd": int(ev["n_nonpd"]), "all_metrics_finite": bool(np.isfinite(m).all()),
            "largest_metric_px": float(np.nanmax(m)) if np.isfinite(m).any() else None}


def main():
    for name in ("fr1xyz", "fr1desk", "fr2robot2"):
        bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", name + ".txt"))
        for value in SWEEP:
            with_min_parallax(value)
            row = {"what": "classify", "sequence": name, "min_parallax": value, **classify(bal, value)}
            K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib, lmk_init="triangulate")
            eng = engine(bal, K)
            eng.upload(state)
            eng.linearise()
            row["ba_initial_mean_reproj_px"] = float(driver.metric(eng.eval())[0])
            last = eng.ba_loop(50, 0, 5)[-1]
            eng.close()
            row.update(ba_after_50_px=float(driver.metric(last)[0]), n_nonfinite=int(last["n_nonfinite"]), n_nonpd=int(last["n_nonpd"]))
            print(json.dumps(row), flush=True)
    bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))
    print(json.dumps({"what": "slam", "points": "file", "lmk_init": "file", **slam(bal, "file")}), flush=True)
    bal["points"] = np.zeros_like(bal["points"])
    for value in SWEEP:
        with_min_parallax(value)
        print(json.dumps({"what": "slam", "points": "zeroed", "lmk_init": "triangulate", "min_parallax": value, **slam(bal, "triangulate")}), flush=True)


if __name__ == "__main__":
    main()
