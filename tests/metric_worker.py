"""One rank of the sharded-metric comparisons in tests/test_gpu_sharded_metric.py, run as a fresh process:

    python -m tests.metric_worker REGION RANK WORLD OUT_DIR TRANSPORT SCENARIO MODE

REGION is a file (in /dev/shm) that the test created and initialised with gbp_comm_region_init for WORLD ranks and the scenario's camera
count ("-": the scenario makes its own 1-rank regions).  MODE is `ride` — the loops with the metric as the library runs them
(gbp_ba_loop / gbp_iterate_eval_each with a host `out`) — or `perpass`: the loop they replace, spelled out with calls this change does not
touch (gbp_weaken_priors, gbp_iterate(1), gbp_eval, gbp_eval_global per pass).  Scenarios:

    loop           fr2robot2: LINEARISE, gbp_ba_loop(12, 0, steps) then (18, 12, steps), both with the metric
    synth:C:L      a synthetic graph of C cameras and L landmarks, 3 observations each: LINEARISE, passes 0 .. 11 of the loop body
    synth:C:L:e    the same with explicit landmark bounds that leave rank 1 an EMPTY range
    health         synth 5 x 70 with one camera and one landmark that carry no information (zero prior, no active factor): 6 passes
    slam           fr2robot2: the SLAM flow (driver.run_slam) for 23 sweeps, NEW_KEYFRAME before sweeps 8 and 16
    one_rank       WORLD = 1, its own regions: synth 5 x 70 x 3 on a plain ctx (riding and per pass) and behind a 1-rank communicator of
                   every transport (RCCL in both schedules where librccl resolves): 12 passes with the weakenings inside the burst; then
                   gbp_iterate_eval_each(260) over a ring piece on transport 2, and the `health` graph on a plain ctx per pass

Every metric record is written as the hex of its 56 bytes; the whole gbp_read state as OUT_DIR/<array>_r<RANK>.npy (one_rank: one set per
engine, <array>_<engine>.npy), everything else as OUT_DIR/info_r<RANK>.json."""
import ctypes
import mmap
import os
import struct
import sys

import numpy as np

from tests.rank_group import ROOT, rank_engine, write_rank

FIELDS = ("sum_norm", "sum_half_sq", "n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd")


def rec_hex(ev):
    """a gbp_eval_out as the hex of its bytes (two doubles, five 64-bit counters)"""
    return struct.pack("<dd5Q", *(ev[k] for k in FIELDS)).hex()


def graph(scenario):
    from gbp_poplar_amd import hostlib
    if scenario.startswith("synth:"):
        parts = scenario.split(":")
        return hostlib.synth_generate(int(parts[1]), int(parts[2]), 3, 5)
    if scenario in ("health", "one_rank"):
        return hostlib.synth_generate(5, 70, 3, 5)
    return hostlib.bal_read(os.path.join(ROOT, "data", "sequences", "fr2robot2.txt"))


def bounds_of(bal, scenario, world):
    from gbp_poplar_amd import hostlib
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    if scenario.startswith("synth:") and scenario.endswith(":e"):      # rank 1 owns nothing
        cut = [0, L // 3, L // 3] + [L // 3 + (L - L // 3) * k // (world - 2) for k in range(1, world - 1)]
        return np.asarray(cut, np.uint32)
    return hostlib.landmark_partition(bal["cam_id"], bal["lmk_id"], C, L, world)


def no_information(bal, state):
    """camera 1 and the last landmark: zero prior, none of their factors active"""
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    st = {k: np.array(v, copy=True) for k, v in state.items()}
    cam, lmk = np.asarray(bal["cam_id"]), np.asarray(bal["lmk_id"])
    st["active_flag"][(cam == 1) | (lmk == L - 1)] = 0
    st["cam_priors_eta"][6:12] = 0
    st["cam_priors_lambda"][36:72] = 0
    st["lmk_priors_eta"][3 * (L - 1):] = 0
    st["lmk_priors_lambda"][9 * (L - 1):] = 0
    return st


def weakens(it, steps):
    return (it + 1) % 2 == 0 and it < 2 * steps


def passes(eng, mode, n, it0, steps, with_global):
    """passes it0 .. it0 + n - 1 of the loop body with the metric -> (local records, global records or None)"""
    if mode == "ride":
        return [rec_hex(e) for e in eng.ba_loop(n, it0, steps)], None
    loc, glob = [], []
    for it in range(it0, it0 + n):
        if weakens(it, steps):
            eng.weaken_priors()
        eng.iterate(1)
        loc.append(rec_hex(eng.eval()))
        if with_global:
            glob.append(rec_hex(eng.eval_global()))
    return loc, glob if with_global else None


class PerPass:
    """an engine without the burst call: driver.run_slam then runs gbp_iterate + gbp_eval per pass"""
    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "iterate_eval_each":
            raise AttributeError(name)
        return getattr(self._eng, name)


def save_state(eng, out_dir, tag):
    for k, v in eng.read().items():
        np.save(os.path.join(out_dir, "%s_%s.npy" % (k, tag)), v)


def own_region(lib, C):
    size = int(lib.gbp_comm_region_bytes(C, 1))
    mm = mmap.mmap(-1, size)
    buf = (ctypes.c_char * size).from_buffer(mm)
    assert lib.gbp_comm_region_init(ctypes.addressof(buf), size, C, 1) == 0
    return mm, buf


def one_rank(out_dir):
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = graph("one_rank")
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    opts = driver.Options()
    steps = int(opts.steps)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    info = {"n_factors": int(bal["n_edges"]), "engines": {}}

    def run(tag, make, mode, st=state, n=12, each=0):
        eng, keep = make()
        try:
            eng.upload(st)
            eng.linearise()
            rec = {}
            if each:
                rec["records"] = [rec_hex(e) for e in eng.iterate_eval_each(each)] if mode == "ride" else passes(eng, mode, each, 0, 0, False)[0]
            else:
                rec["records"] = passes(eng, mode, n, 0, steps, False)[0]
            if keep is not None:
                rec["describe"] = eng.comm_describe()
            save_state(eng, out_dir, tag)
            info["engines"][tag] = rec
        finally:
            eng.close()
            del keep

    def plain():
        return GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K), None

    def behind(transport):
        def make():
            eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(0, 1, 0, L))
            mm, buf = own_region(eng.lib, C)
            eng.comm_init(ctypes.addressof(buf), transport)
            return eng, (mm, buf)
        return make

    def rccl(two_streams):
        def make():
            eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(0, 1, 0, L))
            eng.comm_init_rccl(eng.comm_unique_id())
            eng.comm_set_schedule(two_streams)
            return eng, ()
        return make

    run("plain_ride", plain, "ride")
    run("plain_perpass", plain, "perpass")
    for t in (2, 3, 4):
        run("t%d" % t, behind(t), "ride")
    run("t2_perpass", behind(2), "perpass")
    try:
        probe = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(0, 1, 0, L))
        try:
            probe.comm_unique_id()
        finally:
            probe.close()
        info["rccl"] = True
    except GbpError as e:
        info["rccl"] = False
        info["rccl_error"] = str(e)
    if info["rccl"]:
        run("rccl_one_stream", rccl(False), "ride")
        run("rccl_two_streams", rccl(True), "ride")
    run("each_ride", behind(2), "ride", each=260)
    run("each_perpass", behind(2), "perpass", each=260)
    run("health_plain", plain, "perpass", st=no_information(bal, state), n=6)
    write_rank(out_dir, 0, {}, info)
    return 0


def main(argv):
    region_path, rank, world, out_dir, transport, scenario, mode = argv[0], int(argv[1]), int(argv[2]), argv[3], int(argv[4]), argv[5], argv[6]
    if scenario == "one_rank":
        return one_rank(out_dir)
    from gbp_poplar_amd import driver, hostlib
    bal = graph(scenario)
    opts = driver.Options()
    steps = int(opts.steps)
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=scenario == "slam")
    if scenario == "health":
        state = no_information(bal, state)
    bounds = bounds_of(bal, scenario, world)
    with rank_engine(region_path, rank, world, transport, bal, K, bounds) as (eng, info):
        info["bounds"] = [int(b) for b in bounds]
        if scenario == "slam":
            info["traj"] = driver.run_slam(eng if mode == "ride" else PerPass(eng), hostlib, bal, state, extra, opts, iters_between_kfs=8, max_iters=23)
        else:
            eng.upload(state)
            eng.linearise()
            n = 6 if scenario == "health" else 12
            info["records"], info["global"] = passes(eng, mode, n, 0, steps, True)
            if scenario == "loop":
                more, more_glob = passes(eng, mode, 18, 12, steps, True)
                info["records"] += more
                if more_glob is not None:
                    info["global"] += more_glob
        info["describe"] = eng.comm_describe()      # after the loops: its "metric" member says how they ran
        write_rank(out_dir, rank, eng.read(), info)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
