"""Host-side driver logic of the reference's two programs, engine-agnostic.

Mirrors what `main()` does around the Poplar engine in the reference:
  ba/ba.cpp:479-604   load, K, measurements, prior means, priors, scalings, per-factor state
  ba/ba.cpp:979-1053  WRITE, LINEARISE, READ, eval, loop {WEAKEN_PRIORS?, GBP, READ, eval}
  ba/slam.cpp:589-595,1013-1103  the incremental (keyframe-by-keyframe) variant

`engine` is anything with the program-list verbs (upload, linearise, iterate, weaken_priors, read,
read_priors, new_keyframe, eval) — the product passes gbp_poplar_amd.engine.GbpEngine; `host`
supplies the CPU-side helper functions (the product passes gbp_poplar_amd.hostlib).  The C++ CLIs
(csrc/ba_main.cpp, csrc/slam_main.cpp) implement the same flow natively; this module exists so that
parity tests and bench.py can drive the C-ABI the way the reference's main() drives Poplar.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class Options:
    """CLI flags and defaults of ba.cpp:394-476 / slam.cpp:394-476."""
    n_iters: int = 1500
    iters_between_kfs: int = 700
    reproj_meas_var: float = 4.0
    prior_std_weaker_factor: float = 100.0
    first_cam_prior_std: float = 0.01
    steps: float = 5.0
    undamped_start: int = 15
    # initialisation options, ba.cpp:422-441 (+ --seed: the reference seeds its noise from the clock)
    tn: float = 0.0
    rn: float = 0.0
    ltn: float = 0.0
    avdepth_on: bool = False
    seed: int = 0


def k_matrix(bal):
    """ba.cpp:494-495"""
    return np.array([bal["fx"], 0.0, bal["cx"], 0.0, bal["fy"], bal["cy"], 0.0, 0.0, 1.0], dtype=np.float32)


LMK_INIT = ("file", "triangulate")


def _seed_options(opts):
    from . import seed
    return seed.default_options(reproj_meas_var=opts.reproj_meas_var)


def build_inputs(bal, opts, host, slam=False, lmk_init="file"):
    """Everything WRITE_PROG uploads, as a dict of numpy arrays (ba.cpp:494-604, slam.cpp:575-595).

    lmk_init = "triangulate": the landmarks' prior means and strengths come from the observations and the (possibly noised) camera
    prior means (seed.landmarks over ALL observations; runs on the GPU), not from the file's points, which are not used at all: the
    camera priors are computed as ever, their strengths taken at the seeded points.  extra["lmk_index"] then holds seed.index()."""
    if lmk_init not in LMK_INIT:
        raise ValueError("lmk_init: expected one of %s, got %r" % (LMK_INIT, lmk_init))
    if lmk_init == "triangulate" and getattr(opts, "avdepth_on", False):
        raise ValueError('lmk_init="triangulate" and avdepth_on both place the landmarks: choose one')
    C, L, E = int(bal["n_cams"]), int(bal["n_lmks"]), int(bal["n_edges"])
    K = k_matrix(bal)
    cam_file = np.asarray(bal["cameras"], dtype=np.float64).astype(np.float32)   # ba.cpp:523-528
    lmk_file = np.asarray(bal["points"], dtype=np.float64).astype(np.float32)    # ba.cpp:529-534
    cam_mean, lmk_mean = cam_file.copy(), lmk_file.copy()                       # no init noise by default
    if getattr(opts, "tn", 0) or getattr(opts, "rn", 0) or (getattr(opts, "ltn", 0) and not opts.avdepth_on):   # ba.cpp:536-545
        seed = opts.seed or int.from_bytes(__import__("os").urandom(8), "little")
        cam_mean, lmk_mean = host.init_add_noise(C, L, cam_mean, lmk_mean, opts.tn, opts.rn,
                                                 0.0 if opts.avdepth_on else opts.ltn, seed)
    if getattr(opts, "avdepth_on", False):                                       # ba.cpp:546-548
        lmk_mean = host.init_av_depth(bal["cam_id"], bal["lmk_id"], C, L, cam_mean, lmk_mean)
    measurements = np.asarray(bal["observations"], dtype=np.float64).astype(np.float32)
    extra = {}
    if lmk_init == "triangulate":
        from . import seed
        extra["lmk_index"] = seed.index(bal["lmk_id"], L)
        s = seed.landmarks(bal["cam_id"], *extra["lmk_index"], K, cam_mean, measurements, options=_seed_options(opts))
        lmk_mean = s["lmk_mean"]
        cpe, cpl, _, _ = host.set_prior_lambda(bal["cam_id"], bal["lmk_id"], C, L, K, opts.reproj_meas_var,
                                               cam_file, lmk_mean, cam_mean, lmk_mean)
        lpe, lpl = s["lmk_priors_eta"], s["lmk_priors_lambda"]
    else:
        cpe, cpl, lpe, lpl = host.set_prior_lambda(bal["cam_id"], bal["lmk_id"], C, L, K, opts.reproj_meas_var,
                                                   cam_file, lmk_file, cam_mean, lmk_mean)
    cs, ls = host.prior_scalings(C, L, cpl, opts.steps, opts.prior_std_weaker_factor, opts.first_cam_prior_std)
    steps = int(opts.steps)
    state = {
        "damping": np.zeros(E, np.float32),
        "damping_count": np.full(E, -opts.undamped_start, np.int32),        # ba.cpp:581
        # mu / oldmu are zero in the reference (ba.cpp:582-583): left out = NULL = zeros in the C-ABI
        "cam_scaling": cs, "lmk_scaling": ls,
        "cam_priors_eta": cpe, "cam_priors_lambda": cpl, "lmk_priors_eta": lpe, "lmk_priors_lambda": lpl,
        "measurements": measurements,
        "meas_variances": np.full(E, opts.reproj_meas_var, np.float32),
    }
    if not slam:                                                             # ba.cpp:588-590
        state["active_flag"] = np.ones(E, np.uint32)
        state["cam_weaken_flag"] = np.full(C, steps, np.uint32)
        state["lmk_weaken_flag"] = np.full(L, steps, np.uint32)
    else:                                                                    # slam.cpp:589-595
        active, cwf, lwf, laf = host.slam_create_flags(bal["cam_id"], bal["lmk_id"], C, L, steps)
        state["active_flag"], state["cam_weaken_flag"], state["lmk_weaken_flag"] = active, cwf, lwf
        extra["lmk_active_flag"] = laf
    return K, state, extra


def metric(ev):
    """(mean reprojection error, cost, rmse) from raw eval sums: util.cpp:143, SURVEY 8d."""
    n = max(int(ev["n_active"]), 1)
    return ev["sum_norm"] / n, ev["sum_half_sq"], float(np.sqrt(2.0 * ev["sum_half_sq"] / n))


def run_ba(engine, state, opts, n_iters=None, eval_every=1, log=None):
    """ba.cpp:979-1053.  Returns [(iter, mean_reproj, cost, n_relin, n_robust)], iter -1 = initial."""
    n_iters = opts.n_iters if n_iters is None else n_iters
    engine.upload(state)
    engine.linearise()
    traj = []
    ev = engine.eval()
    m = metric(ev)
    traj.append((-1, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
    if log:
        log("Initial Reprojection error: %.6f Cost %.6f" % (m[0], m[1]))
    it = 0
    while it < n_iters:
        if ((it + 1) % 2 == 0) and (it < opts.steps * 2):                   # ba.cpp:1003-1006
            if log:
                log("Weakening priors ")
            engine.weaken_priors()
        # up to the next host event (prior weakening, metric read-back, end) in ONE call, like csrc/ba_main.cpp: the
        # engine then runs the burst without leaving the device (hipGraph replay, or k_persist on small graphs)
        if eval_every == 1 and hasattr(engine, "iterate_eval_each"):
            # the reference's default, the metric after EVERY iteration: everything up to the next prior weakening in one call
            burst = 1
            while it + burst < n_iters and not (((it + burst + 1) % 2 == 0) and (it + burst < opts.steps * 2)):
                burst += 1
            for k, ev in enumerate(engine.iterate_eval_each(burst)):
                m = metric(ev)
                traj.append((it + k, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
                if log:
                    log("Iter %d // Reprojection error %.6f // Cost %.6f // n relins: %d // n robust edges %d"
                        % (it + k, m[0], m[1], ev["n_relin"], ev["n_robust"]))
            it += burst
            continue
        burst = 1
        while (it + burst < n_iters and not (eval_every and (it + burst) % eval_every == 0)
               and not (((it + burst + 1) % 2 == 0) and (it + burst < opts.steps * 2))):
            burst += 1
        engine.iterate(burst)
        it += burst - 1
        if eval_every and ((it + 1) % eval_every == 0 or it == n_iters - 1):
            ev = engine.eval()
            m = metric(ev)
            traj.append((it, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
            if log:
                log("Iter %d // Reprojection error %.6f // Cost %.6f // n relins: %d // n robust edges %d"
                    % (it, m[0], m[1], ev["n_relin"], ev["n_robust"]))
        it += 1
    return traj


def _resect_keyframe(host, bal, state, opts, extra, bel, pri, guess, active, laf, lwf, kf, log, locate_first=False):
    """kf_init = "resect": camera kf alone from the pose guess (the copy of its predecessor), against the belief means of the landmarks
    that were mapped before this keyframe, over the updated active_flag.  A resected pose replaces the prior eta of camera kf (prior
    Lambda . pose, the Lambda stays the file's) and is returned; otherwise the copy stands and the guess is returned.

    locate_first (kf_init = "locate"): before that, locate.cameras finds the camera with no guess over the same observations; if it does,
    the resection starts from the located pose over the active observations that agree with it, and its result is taken.  If the
    camera is not located, or that resection is NOT_RESECTED, everything above happens as without it."""
    from . import resect
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    if "cam_index" not in extra:
        extra["cam_index"] = resect.index(bal["cam_id"], C)
    with np.errstate(all="ignore"):      # (a landmark that was never active has a zero belief: its mean is not used)
        cam_mean, lmk_mean = host.belief_means(C, L, bel["cam_beliefs_eta"], bel["cam_beliefs_lambda"], bel["lmk_beliefs_eta"],
                                               bel["lmk_beliefs_lambda"])
    cam_mean, lmk_mean = cam_mean.astype(np.float32), lmk_mean.astype(np.float32)
    if guess is None:      # the copy: the belief mean of the camera before
        guess = cam_mean[6 * (kf - 1):6 * kf].copy()
    cam_mean[6 * kf:6 * kf + 6] = guess
    select = np.zeros(C, np.uint32)
    select[kf] = 1
    if locate_first:
        from . import locate
        lmk_use = ((laf != 0) & (lwf == 0)).astype(np.uint32)
        loc = locate.cameras(bal["lmk_id"], *extra["cam_index"], k_matrix(bal), lmk_mean, state["measurements"], active_flag=active, lmk_use=lmk_use,
                             select=select)
        if not int(loc["status"][kf]) & locate.NOT_LOCATED:
            start = cam_mean.copy()
            start[6 * kf:6 * kf + 6] = loc["cam_mean"][6 * kf:6 * kf + 6]
            agreeing = ((np.asarray(active) == 1) & (loc["inlier"] == 1)).astype(np.uint32)
            r = resect.cameras(bal["lmk_id"], *extra["cam_index"], k_matrix(bal), start, lmk_mean, state["measurements"], active_flag=agreeing,
                               lmk_use=lmk_use, select=select, options=resect.default_options(reproj_meas_var=opts.reproj_meas_var),
                               priors_lambda=pri["cam_priors_lambda"], out={"cam_priors_eta": pri["cam_priors_eta"]})
            st = int(r["status"][kf])
            if not st & resect.NOT_RESECTED:
                pri["cam_priors_eta"] = r["cam_priors_eta"]
                if log:
                    log("Keyframe %d: pose located from %d of %d views and resected, cost %.6f -> %.6f (status %d)"
                        % (kf + 1, loc["n_inliers"][kf], loc["n_views"][kf], r["report"][4 * kf], r["report"][4 * kf + 1], st))
                return r["cam_mean"][6 * kf:6 * kf + 6]
    r = resect.cameras(bal["lmk_id"], *extra["cam_index"], k_matrix(bal), cam_mean, lmk_mean, state["measurements"], active_flag=active,
                       lmk_use=((laf != 0) & (lwf == 0)).astype(np.uint32), select=select,
                       options=resect.default_options(reproj_meas_var=opts.reproj_meas_var), priors_lambda=pri["cam_priors_lambda"],
                       out={"cam_priors_eta": pri["cam_priors_eta"]})
    st, n = int(r["status"][kf]), int(r["n_views"][kf])
    if st & resect.NOT_RESECTED:
        if log:
            log("Keyframe %d: pose copied from keyframe %d (resection status %d, %d views)" % (kf + 1, kf, st, n))
        return guess
    pri["cam_priors_eta"] = r["cam_priors_eta"]
    if log:
        log("Keyframe %d: pose resected from %d views, cost %.6f -> %.6f (status %d)" % (kf + 1, n, r["report"][4 * kf], r["report"][4 * kf + 1], st))
    return r["cam_mean"][6 * kf:6 * kf + 6]


KF_INIT = ("copy", "resect", "locate")


def run_slam(engine, host, bal, state, extra, opts, iters_between_kfs=None, max_iters=None, eval_every=1, log=None, lmk_init="file",
             kf_init="copy"):
    """slam.cpp:1013-1103.

    lmk_init = "triangulate", at every keyframe: the new camera's prior eta comes from seed.keyframe (the bits of
    slam_initialise_new_kf), and the landmarks this keyframe activated are seeded from every now-active observation, at the belief
    means of the cameras so far and the new camera's pose guess; every other prior passes through.

    kf_init = "resect", at every keyframe: the new camera's pose guess — the copy of its predecessor — is refined against the landmarks
    mapped so far (resect.cameras: _resect_keyframe); its prior eta, and with lmk_init = "triangulate" the pose the new landmarks are
    seeded at, come from the resected pose.  Runs on the GPU, through host arrays.

    kf_init = "locate": the same, with locate.cameras in front — the new camera is first found with no guess at all among the landmarks
    mapped so far, wrong matches tolerated, and resected from there over the observations that agree; a keyframe where that fails
    takes the "resect" path unchanged."""
    if lmk_init not in LMK_INIT:
        raise ValueError("lmk_init: expected one of %s, got %r" % (LMK_INIT, lmk_init))
    if kf_init not in KF_INIT:
        raise ValueError("kf_init: expected one of %s, got %r" % (KF_INIT, kf_init))
    C, L, E = int(bal["n_cams"]), int(bal["n_lmks"]), int(bal["n_edges"])
    ibk = opts.iters_between_kfs if iters_between_kfs is None else iters_between_kfs
    steps = int(opts.steps)
    active = state["active_flag"].copy()
    cwf, lwf = state["cam_weaken_flag"].copy(), state["lmk_weaken_flag"].copy()
    laf = extra["lmk_active_flag"].copy()
    engine.upload(state)
    engine.linearise()
    traj = []
    ev = engine.eval()
    m = metric(ev)
    traj.append((-1, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
    if log:
        log("Initial Reprojection error: %.6f Cost %.6f" % (m[0], m[1]))
    niters = (C - 1) * ibk - 1                                              # slam.cpp:1013
    if max_iters is not None:
        niters = min(niters, max_iters)
    it, data_counter = 0, 0
    i = 0
    while i < niters:
        if (i + 1) % ibk == 0:                                              # slam.cpp:1020-1046
            it = 0
            data_counter += 1
            n_new = host.slam_update_flags(bal["cam_id"], bal["lmk_id"], C, L, steps, data_counter,
                                           active, lwf, cwf, laf)
            pri = engine.read_priors()
            bel = engine.read()
            if lmk_init == "triangulate":
                from . import seed
                pri["cam_priors_eta"], guess = seed.keyframe(data_counter, data_counter + 1, bel["cam_beliefs_eta"], bel["cam_beliefs_lambda"],
                                                             pri["cam_priors_lambda"], pri["cam_priors_eta"])
                cam_mean = host.belief_means(C, L, bel["cam_beliefs_eta"], bel["cam_beliefs_lambda"], bel["lmk_beliefs_eta"],
                                             bel["lmk_beliefs_lambda"])[0].astype(np.float32)
                if kf_init != "copy":
                    guess = _resect_keyframe(host, bal, state, opts, extra, bel, pri, guess, active, laf, lwf, data_counter + 1, log,
                                             kf_init == "locate")
                cam_mean[6 * (data_counter + 1):6 * (data_counter + 2)] = guess
                start, edges = extra["lmk_index"] if "lmk_index" in extra else seed.index(bal["lmk_id"], L)
                s = seed.landmarks(bal["cam_id"], start, edges, k_matrix(bal), cam_mean, state["measurements"], active_flag=active,
                                   select=(lwf != 0).astype(np.uint32), options=_seed_options(opts),
                                   out={"lmk_priors_eta": pri["lmk_priors_eta"], "lmk_priors_lambda": pri["lmk_priors_lambda"]})
                pri["lmk_priors_eta"], pri["lmk_priors_lambda"] = s["lmk_priors_eta"], s["lmk_priors_lambda"]
            else:
                host.slam_initialise_new_kf(data_counter, bel["cam_beliefs_eta"], bel["cam_beliefs_lambda"],
                                            pri["cam_priors_lambda"], pri["cam_priors_eta"])
                if kf_init != "copy":
                    _resect_keyframe(host, bal, state, opts, extra, bel, pri, None, active, laf, lwf, data_counter + 1, log, kf_init == "locate")
            engine.new_keyframe({"damping_count": np.full(E, -15, np.int32),   # literal -15, slam.cpp:1040
                                 "cam_priors_eta": pri["cam_priors_eta"], "cam_priors_lambda": pri["cam_priors_lambda"],
                                 "lmk_priors_eta": pri["lmk_priors_eta"], "lmk_priors_lambda": pri["lmk_priors_lambda"],
                                 "active_flag": active, "cam_weaken_flag": cwf, "lmk_weaken_flag": lwf})
            if log:
                log("Adding keyframe %d, %d new landmarks" % (data_counter + 1, n_new))
        if ((it + 1) % 2 == 0) and (it < opts.steps * 2):
            engine.weaken_priors()
        if eval_every == 1 and hasattr(engine, "iterate_eval_each"):
            burst = 1                   # the metric after EVERY iteration, up to the next keyframe / prior weakening in one call
            while (i + burst < niters and (i + burst + 1) % ibk != 0
                   and not (((it + burst + 1) % 2 == 0) and (it + burst < opts.steps * 2))):
                burst += 1
            for k, ev in enumerate(engine.iterate_eval_each(burst)):
                m = metric(ev)
                traj.append((i + k, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
                if log:
                    log("Iters %d (since last kf %d) // Reprojection error %.6f // Cost %.6f // n relins: %d // n robust edges %d"
                        % (ibk * data_counter + it + k, it + k, m[0], m[1], ev["n_relin"], ev["n_robust"]))
            i += burst
            it += burst
            continue
        burst = 1                       # up to the next keyframe / prior weakening / read-back in one call
        while (i + burst < niters and (i + burst + 1) % ibk != 0 and not (eval_every and (i + burst) % eval_every == 0)
               and not (((it + burst + 1) % 2 == 0) and (it + burst < opts.steps * 2))):
            burst += 1
        engine.iterate(burst)
        i += burst - 1
        it += burst - 1
        if eval_every and ((i + 1) % eval_every == 0 or i == niters - 1):
            ev = engine.eval()
            m = metric(ev)
            traj.append((i, m[0], m[1], int(ev["n_relin"]), int(ev["n_robust"])))
            if log:
                log("Iters %d (since last kf %d) // Reprojection error %.6f // Cost %.6f // n relins: %d // n robust edges %d"
                    % (ibk * data_counter + it, it, m[0], m[1], ev["n_relin"], ev["n_robust"]))
        it += 1
        i += 1
    return traj
