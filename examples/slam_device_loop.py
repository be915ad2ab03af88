"""A SLAM-style loop whose state never leaves the GPU: read(device=True) -> tensor arithmetic -> new_keyframe, no host copy.
The same loop with host arrays runs beside it; the printed metrics are equal.     python examples/slam_device_loop.py [sequence]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gbp_poplar_amd import driver, hostlib                       # noqa: E402
from gbp_poplar_amd.engine import GbpEngine                      # noqa: E402


def run(bal, device, keyframes=4, iters=25):
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    C, E = int(bal["n_cams"]), int(bal["n_edges"])
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, bal["n_lmks"], K)
    to = (lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()) if device else (lambda a: a)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)      # the ctx's work rides on torch's stream
    eng.upload({k: to(v) for k, v in state.items()})
    eng.linearise()
    for kf in range(1, keyframes + 1):
        eng.iterate(iters)
        bel, pri = eng.read(device=device), eng.read_priors(device=device)
        # the new keyframe's prior mean := the belief of the one before it, at the prior's own strength (eta = Lambda_prior mu)
        lam_b, eta_b = bel["cam_beliefs_lambda"].reshape(C, 6, 6)[kf - 1], bel["cam_beliefs_eta"].reshape(C, 6)[kf - 1]
        lam_p = pri["cam_priors_lambda"].reshape(C, 6, 6)[kf]
        if device:
            mu = torch.linalg.solve(lam_b.double(), eta_b.double())
            pri["cam_priors_eta"].reshape(C, 6)[kf] = (lam_p.double() @ mu).float()
            cnt = torch.full((E,), -15, dtype=torch.int32, device="cuda")
        else:
            mu = torch.linalg.solve(torch.from_numpy(lam_b).cuda().double(), torch.from_numpy(eta_b).cuda().double())
            pri["cam_priors_eta"].reshape(C, 6)[kf] = (torch.from_numpy(lam_p).cuda().double() @ mu).float().cpu().numpy()
            cnt = np.full(E, -15, np.int32)
        eng.new_keyframe({"damping_count": cnt, **pri})
    eng.iterate(iters)
    ev = eng.eval()
    return ev["sum_norm"] / ev["n_active"], ev["sum_half_sq"]


if __name__ == "__main__":
    bal = hostlib.bal_read(os.path.join(ROOT, "data", "sequences", (sys.argv[1] if len(sys.argv) > 1 else "fr2robot2") + ".txt"))
    dev, host = run(bal, True), run(bal, False)
    print("device loop: mean reprojection error %.9f cost %.6f" % dev)
    print("host loop:   mean reprojection error %.9f cost %.6f" % host)
    assert dev == host, "the device loop and the host-array loop differ"
