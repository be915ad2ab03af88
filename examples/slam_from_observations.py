"""SLAM from observations and rough camera poses alone: the file's `points` section is zeroed before use, every landmark prior comes
from seed.landmarks (triangulated where the views allow, placed on the ray of the first observation otherwise), every new keyframe's
prior from seed.keyframe — on device tensors, in place in what read_priors(device=True) returned, no host copy of the state.  The same
loop with host arrays runs beside it; the printed metrics are equal.  Then the driver's loop from the same start with
kf_init="locate": every new keyframe is first found with no pose guess among the landmarks mapped so far (locate.cameras), then resected
over the observations that agree.     python examples/slam_from_observations.py [sequence]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gbp_poplar_amd import driver, hostlib, post, seed           # noqa: E402
from gbp_poplar_amd.engine import GbpEngine                      # noqa: E402


def run(bal, device, keyframes=4, iters=25):
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init="triangulate")
    C, L, E = int(bal["n_cams"]), int(bal["n_lmks"]), int(bal["n_edges"])
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K)
    to = (lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()) if device else (lambda a: a)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)      # the ctx's work rides on torch's stream
    eng.upload({k: to(v) for k, v in state.items()})
    eng.linearise()
    active, cwf, lwf = state["active_flag"].copy(), state["cam_weaken_flag"].copy(), state["lmk_weaken_flag"].copy()
    laf = extra["lmk_active_flag"].copy()
    graph = [to(np.ascontiguousarray(a, np.uint32)) for a in (bal["cam_id"],) + tuple(extra["lmk_index"])]
    z, options = to(state["measurements"]), seed.default_options(reproj_meas_var=opts.reproj_meas_var)
    for kf in range(1, keyframes + 1):
        eng.iterate(iters)
        hostlib.slam_update_flags(bal["cam_id"], bal["lmk_id"], C, L, int(opts.steps), kf, active, lwf, cwf, laf)      # the graph is static: host flags
        bel, pri = eng.read(device=device), eng.read_priors(device=device)
        # the new keyframe's prior mean := the belief mean of the one before it, which is also its pose guess
        pri["cam_priors_eta"], guess = seed.keyframe(kf, kf + 1, bel["cam_beliefs_eta"], bel["cam_beliefs_lambda"], pri["cam_priors_lambda"],
                                                     pri["cam_priors_eta"])
        cam_mean = post.moments(bel)["cam_mean"]
        cam_mean[6 * (kf + 1):6 * (kf + 2)] = guess
        # the landmarks this keyframe brought in, from every observation that is active now; the other priors are not touched
        s = seed.landmarks(*graph, K, cam_mean, z, active_flag=to(active), select=to((lwf != 0).astype(np.uint32)), options=options,
                           out={"lmk_priors_eta": pri["lmk_priors_eta"], "lmk_priors_lambda": pri["lmk_priors_lambda"]})
        pri["lmk_priors_eta"], pri["lmk_priors_lambda"] = s["lmk_priors_eta"], s["lmk_priors_lambda"]
        cnt = torch.full((E,), -15, dtype=torch.int32, device="cuda") if device else np.full(E, -15, np.int32)
        eng.new_keyframe({"damping_count": cnt, **pri, "active_flag": to(active), "cam_weaken_flag": to(cwf), "lmk_weaken_flag": to(lwf)})
    eng.iterate(iters)
    ev = eng.eval()
    return ev["sum_norm"] / ev["n_active"], ev["sum_half_sq"]


if __name__ == "__main__":
    bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", (sys.argv[1] if len(sys.argv) > 1 else "fr2robot2") + ".txt"))
    bal["points"] = np.zeros_like(bal["points"])                 # nothing of a solved map is used
    dev, host = run(bal, True), run(bal, False)
    print("device loop: mean reprojection error %.9f cost %.6f" % dev)
    print("host loop:   mean reprojection error %.9f cost %.6f" % host)
    assert dev == host, "the device loop and the host-array loop differ"

    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init="triangulate")
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], int(bal["n_cams"]), int(bal["n_lmks"]), K)
    traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=25, max_iters=5 * 25, lmk_init="triangulate", kf_init="locate",
                           log=lambda line: print(line) if line.startswith("Keyframe ") else None)
    eng.close()
    print("driver, kf_init=locate: mean reprojection error %.9f cost %.6f" % (traj[-1][1], traj[-1][2]))
