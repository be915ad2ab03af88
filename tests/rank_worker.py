"""One rank of the bit-level transport comparisons in tests/test_p2p_transport.py, tests/test_p2p_slices.py and
tests/test_measured_transport.py, run as a fresh process by tests/rank_group.py:

    python -m tests.rank_worker REGION RANK WORLD OUT_DIR TRANSPORT SCENARIO

REGION is a file (in /dev/shm) that the launcher created and initialised with gbp_comm_region_init for WORLD ranks and the scenario's
camera count.  The rank builds its landmark shard, attaches the library's communicator over TRANSPORT and runs the scenario:

    iterate        fr2robot2: LINEARISE, 30 iterations, WEAKEN_PRIORS, 5 more, gbp_eval_global, gbp_comm_probe(reps=5)
    loop           fr2robot2: LINEARISE, passes 0 .. 11 of the loop body through gbp_ba_loop with a host `out` (the five weakenings, the
                   metric after every pass), passes 12 .. 29 without the metric (the relinearising sweeps), gbp_eval_global
    upload_first   the same, but gbp_upload comes BEFORE gbp_comm_init: transport 5's measurement runs on an uploaded ctx
    slam           fr2robot2: the SLAM flow (driver.run_slam) for 23 sweeps, NEW_KEYFRAME before sweeps 8 and 16
    synth:C:L      a synthetic graph of C cameras and L landmarks, 3 observations each: LINEARISE, passes 0 .. 11 of the loop body,
                   gbp_eval_global

and writes its whole gbp_read state as OUT_DIR/<array>_r<RANK>.npy, and as OUT_DIR/info_r<RANK>.json what gbp_comm_init took and left
(init_s, last_error, describe, transport) with the scenario's records (probe_us, loop, eval, traj)."""
import os
import sys

from tests.rank_group import ROOT, rank_engine, write_rank


def graph(scenario):
    from gbp_poplar_amd import hostlib
    if scenario.startswith("synth:"):
        _, n_cams, n_lmks = scenario.split(":")
        return hostlib.synth_generate(int(n_cams), int(n_lmks), 3, 5)
    return hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))


def main(argv):
    region_path, rank, world, out_dir, transport, scenario = argv[0], int(argv[1]), int(argv[2]), argv[3], int(argv[4]), argv[5]
    from gbp_poplar_amd import driver, hostlib
    bal = graph(scenario)
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=scenario == "slam")
    bounds = hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], int(bal["n_cams"]), int(bal["n_lmks"]), world)
    upload_first = (lambda eng: eng.upload(state)) if scenario == "upload_first" else None
    with rank_engine(region_path, rank, world, transport, bal, K, bounds, before_init=upload_first) as (eng, info):
        if scenario == "slam":
            info["traj"] = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=8, max_iters=23)
        else:
            if scenario != "upload_first":
                eng.upload(state)
            eng.linearise()
            if scenario == "iterate":
                eng.iterate(30)
                eng.weaken_priors()
                eng.iterate(5)
            else:
                info["loop"] = eng.ba_loop(12, 0, opts.steps)
                if not scenario.startswith("synth:"):
                    eng.ba_loop(18, 12, opts.steps, metrics=False)
            info["eval"] = eng.eval_global()
            if scenario == "iterate":
                info["probe_us"] = eng.comm_probe(reps=5)
        write_rank(out_dir, rank, eng.read(), info)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
