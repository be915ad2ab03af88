"""Camera resection on the GPU (libgbp_mi355x_resect.so, gbp_poplar_amd/resect.py).

The kernel against the host twin (tests/sanitize/resect_math_main.cpp, the same header compiled as plain C++, run as a process): bit
for bit, NaNs equal NaNs, over 1, 3, 5 and 257 cameras whose degrees cycle through 0, 5, 6, 63, 64, 65, 127, 129 and 1 000 (the lane
stride and the tree's boundaries), with and without active_flag, lmk_use, select and cam_edges, each optional output left out in turn,
bases at and 4 bytes past a 16-byte boundary inside canary-filled buffers, one NaN landmark, two launches.  The numpy face against the
tensor face.  On the solved map of each shipped sequence every camera, started from its predecessor's solved pose, ends at a lower cost
(the figures: profiles/resect_cameras.md).  run_slam(kf_init="resect") stays healthy and bin/slam --kf_init resect prints its trajectory.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import resect_support as rs
from tests.conftest import seq_path
from tests.test_gpu_post import CANARY, _canaries_intact, _dev, _engine, _ptr, _stream
from tests.test_gpu_seed import _same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAM = os.path.join(ROOT, "gbp_poplar_amd", "bin", "slam")
SEQUENCES = ("fr1xyz", "fr1desk", "fr2robot2")
CYCLE = [0, 5, 6, 63, 64, 65, 127, 129, 1000]
INPUTS = ("lmk_id", "cam_start", "lmk_mean", "measurements")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return rs.compile_host(str(tmp_path_factory.mktemp("resect_host") / "resect_math"), sanitize=False)


def _scene(n_cams, with_edges, nan_landmark):
    g, _ = rs.degree_scene(np.resize(CYCLE, n_cams), seed=200 + n_cams, n_lmks=1000)
    if with_edges:      # the same edges in another file order: cam_edges is needed
        perm = np.random.default_rng(n_cams).permutation(g["lmk_id"].size)
        g = rs.graph_of(n_cams, 1000, g["cam_id"][perm], g["lmk_id"][perm], g["K"], g["cam_mean"], g["lmk_mean"],
                        g["measurements"].reshape(-1, 2)[perm])
    if nan_landmark:
        g["lmk_mean"] = g["lmk_mean"].copy()
        g["lmk_mean"][3 * 18 + 1] = np.nan
    return g


#        n_cams, active_flag, lmk_use, select, cam_edges, the output left out, 4-byte offset, NaN landmark
CASES = [pytest.param(1, False, False, False, False, None, False, False, id="C1"),
         pytest.param(3, True, True, False, True, "cam_priors_eta", True, False, id="C3-flags-use-edges-no_eta-offset4"),
         pytest.param(5, False, False, True, False, "cam_info", False, False, id="C5-select-no_info"),
         pytest.param(5, True, False, False, True, "report", True, False, id="C5-flags-edges-no_report-offset4"),
         pytest.param(257, True, True, True, True, "n_views", True, True, id="C257-flags-use-select-edges-no_n_views-offset4-nan_landmark"),
         pytest.param(257, False, False, False, False, None, False, False, id="C257")]


@pytest.mark.parametrize("n_cams,flags,use,sparse,with_edges,left_out,offset,nan_landmark", CASES)
def test_cameras_equal_the_host_program(n_cams, flags, use, sparse, with_edges, left_out, offset, nan_landmark, host_exe, tmp_path):
    import torch
    from gbp_poplar_amd import resect
    g = _scene(n_cams, with_edges, nan_landmark)
    rng = np.random.default_rng(n_cams)
    E = g["lmk_id"].size
    g["active_flag"] = (np.arange(E) % 3 != 1).astype(np.uint32) if flags else None
    g["lmk_use"] = (np.arange(1000) % 7 != 3).astype(np.uint32) if use else None
    select = (rng.uniform(size=n_cams) < 0.6).astype(np.uint32) if sparse else None
    lam = rng.normal(size=36 * n_cams).astype(np.float32)
    before = rs.initial_outputs(g["cam_mean"])
    want = rs.run_host(host_exe, tmp_path, g, select=select, before=before, priors_lambda=lam, trig="device")
    if n_cams > 8 and not sparse:
        assert want["n_views"].max() == 1000 and {0, 5, 6, 63, 64, 65, 127, 129} <= set(want["n_views"].tolist())
    ins = {k: _dev(g[k], offset) for k in INPUTS}
    opt = {k: _dev(a, offset) if a is not None else (None, None)
           for k, a in (("cam_edges", g["cam_edges"]), ("active_flag", g["active_flag"]), ("lmk_use", g["lmk_use"]), ("select", select))}
    d_lam = _dev(lam, offset)
    outs = {k: _dev(before[k], offset) for k, _, _ in rs.OUTPUTS}
    lib, opts = resect.load(), resect.default_options()
    K9 = (C.c_float * 9)(*[float(x) for x in g["K"]])
    results = []
    for _ in range(2):      # two launches from the same start: the same bits
        for k, _, _ in rs.OUTPUTS:
            outs[k][0].copy_(torch.from_numpy(before[k].view(np.int32) if before[k].dtype != np.float32 else before[k]))
        rc = lib.gbp_resect_cameras(_stream(), n_cams, 1000, E, _ptr(ins["lmk_id"][0]), _ptr(ins["cam_start"][0]), _ptr(opt["cam_edges"][0]), K9,
                                    _ptr(ins["lmk_mean"][0]), _ptr(ins["measurements"][0]), _ptr(opt["active_flag"][0]), _ptr(opt["lmk_use"][0]),
                                    _ptr(opt["select"][0]), C.byref(opts), _ptr(outs["cam_mean"][0]), _ptr(d_lam[0]),
                                    *[None if k == left_out else _ptr(outs[k][0]) for k, _, _ in rs.OUTPUTS[1:]])
        assert rc == 0, lib.gbp_resect_last_error()
        torch.cuda.synchronize()
        results.append({k: outs[k][0].cpu().numpy().view(dt) for k, _, dt in rs.OUTPUTS})
    got = results[0]
    for k, w, _ in rs.OUTPUTS:
        assert _canaries_intact(outs[k][1], w * n_cams, offset), k
        assert _same_bits(results[1][k], got[k]), k
        if k == left_out:
            assert _same_bits(got[k], before[k]), k
            continue
        assert _same_bits(got[k], want[k]), (k, np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))[:8])
        if select is not None:      # a camera that is not selected keeps every output
            assert _same_bits(got[k].reshape(-1, w)[select == 0], before[k].reshape(-1, w)[select == 0]), k
    for k in ins:
        assert _canaries_intact(ins[k][1], ins[k][0].numel(), offset), k
    assert _canaries_intact(d_lam[1], lam.size, offset)
    st = want["status"] if select is None else want["status"][select == 1]
    if nan_landmark:
        assert (st & rs.NONFINITE).any()
    if n_cams > 8:
        assert (st == 0).any() and (st & rs.NO_VIEW).any() and (st & rs.FEW_VIEWS).any()


def test_numpy_face_equals_the_tensor_face_and_out_writes_in_place():
    import torch
    from gbp_poplar_amd import resect
    g = _scene(9, True, False)
    lam = np.random.default_rng(1).normal(size=36 * 9).astype(np.float32)
    args = ("lmk_id", "cam_start", "cam_edges")
    host = resect.cameras(*[g[k] for k in args], g["K"], g["cam_mean"], g["lmk_mean"], g["measurements"], priors_lambda=lam)
    dev = lambda a, ints=False: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if ints else np.ascontiguousarray(a)).cuda()
    cam_mean, status = dev(g["cam_mean"]), torch.full((9,), 77, dtype=torch.int32, device="cuda")
    res = resect.cameras(*[dev(g[k], True) for k in args], g["K"], cam_mean, dev(g["lmk_mean"]), dev(g["measurements"]), priors_lambda=dev(lam),
                         out={"status": status})
    assert res["cam_mean"].data_ptr() == cam_mean.data_ptr() and res["status"].data_ptr() == status.data_ptr()      # in place
    assert set(host) == set(res) == {"cam_mean", "cam_priors_eta", "cam_info", "report", "status", "n_views"}
    for k in host:
        assert _same_bits(host[k], res[k].cpu().numpy().view(host[k].dtype)), k
    assert host["status"].dtype == np.uint32 and host["n_views"].tolist() == CYCLE
    assert not np.array_equal(host["cam_mean"], g["cam_mean"]) and (status.cpu().numpy() != 77).all()
    assert "cam_priors_eta" not in resect.cameras(*[g[k] for k in args], g["K"], g["cam_mean"], g["lmk_mean"], g["measurements"])


def _solved_map(name):
    """(bal, K, solved cameras [C, 6], solved points [3L]): bundle adjustment of the sequence to its default end, the belief means"""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path(name))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = _engine(bal, K)
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
    return bal, K, np.asarray(cams, np.float64).reshape(-1, 6), np.asarray(pts, np.float64).astype(np.float32), state["measurements"]


@pytest.mark.parametrize("name", SEQUENCES)
def test_every_camera_of_a_solved_map_is_resected_from_its_predecessors_pose(name):
    from gbp_poplar_amd import resect
    bal, K, cams, pts, z = _solved_map(name)
    n_c = bal["n_cams"]
    start = np.concatenate([cams[:1], cams[:-1]]).astype(np.float32)
    select = (np.arange(n_c) >= 1).astype(np.uint32)
    idx = resect.index(bal["cam_id"], n_c)
    r = resect.cameras(bal["lmk_id"], *idx, K, start, pts, z, select=select)
    g = {"n_cams": n_c, "cam_id": np.asarray(bal["cam_id"]), "lmk_id": np.asarray(bal["lmk_id"]), "lmk_mean": pts, "measurements": z, "K": K}
    seen = (select == 1) & (r["n_views"] >= resect.default_options().min_views)
    rep = r["report"].reshape(-1, 4)
    e0, e1, n = rs.mean_reprojection(start, g), rs.mean_reprojection(r["cam_mean"], g), np.bincount(bal["cam_id"], minlength=n_c)
    m0, m1 = np.sum((e0 * n)[seen]) / n[seen].sum(), np.sum((e1 * n)[seen]) / n[seen].sum()
    print("%s: %d of %d cameras with enough views; status bits seen %s; cost %.1f -> %.1f in total; mean reprojection error %.3f -> %.3f px "
          "(at the solved poses %.3f px)" % (name, seen.sum(), n_c - 1, sorted(set(r["status"][seen].tolist())), rep[seen, 0].sum(), rep[seen, 1].sum(),
                                              m0, m1, np.sum((rs.mean_reprojection(cams, g) * n)[seen]) / n[seen].sum()))
    assert seen.sum() >= 1 and not (r["status"][seen] & (resect.NONFINITE | resect.BAD_INDEX)).any()
    assert (rep[seen, 1] < rep[seen, 0]).all(), np.flatnonzero(seen & ~(rep[:, 1] < rep[:, 0]))
    assert m1 <= m0


@pytest.fixture(scope="module")
def slam_runs():
    """lmk_init -> (the driver's trajectory of run_slam(kf_init="resect") on fr2robot2 at 30 iterations between keyframes, its final
    metric, its log lines, the number of cameras)"""
    from gbp_poplar_amd import driver, hostlib
    runs = {}
    for lmk_init in ("file", "triangulate"):
        bal = hostlib.bal_read(seq_path("fr2robot2"))
        opts = driver.Options()
        K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init=lmk_init)
        eng = _engine(bal, K)
        log = []
        traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=30, lmk_init=lmk_init, kf_init="resect", log=log.append)
        runs[lmk_init] = (traj, eng.eval(), log, int(bal["n_cams"]))
        eng.close()
    return runs


@pytest.mark.parametrize("lmk_init", ["file", "triangulate"])
def test_run_slam_with_resected_keyframes_stays_healthy(lmk_init, slam_runs):
    traj, ev, log, n_cams = slam_runs[lmk_init]
    said = [l for l in log if l.startswith("Keyframe ")]
    print("%s: final mean reprojection error %.4f px; %d keyframes resected, %d copied"
          % (lmk_init, traj[-1][1], sum("resected" in l for l in said), sum("copied" in l for l in said)))
    assert len(said) == n_cams - 2 and any("resected" in l for l in said)      # one line per keyframe added
    assert ev["n_nonfinite"] == 0 and ev["n_nonpd"] == 0 and np.isfinite([t[1] for t in traj]).all()


@pytest.mark.parametrize("lmk_init", ["file", "triangulate"])
def test_slam_kf_init_resect_prints_the_drivers_trajectory(lmk_init, slam_runs):
    from tests.test_gpu_sharded_solution import _cli
    traj, _, log, n_cams = slam_runs[lmk_init]
    rc, out, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--iters_between_kfs", "30", "--kf_init", "resect", "--lmk_init", lmk_init], timeout=120)
    assert rc == 0 and " Finished GBP." in out, err[-2000:]
    init = re.search(r"Initial Reprojection error: (\S+) Cost (\S+)", out)
    rows = re.findall(r"Iters \d+ \(since last kf \d+\) // Reprojection error (\S+) // Cost (\S+)", out)
    printed = [(init.group(1), init.group(2))] + rows
    assert len(printed) == len(traj) == (n_cams - 1) * 30
    for (m, c), (_, mean, cost, _, _) in zip(printed, traj):      # six significant digits are printed
        assert abs(float(m) - mean) <= 1e-5 * mean and abs(float(c) - cost) <= 1e-5 * cost, (m, mean, c, cost)
    said = re.findall(r"^Keyframe \d+: pose (resected|copied)", out, flags=re.M)
    assert said == [re.match(r"Keyframe \d+: pose (resected|copied)", l).group(1) for l in log if l.startswith("Keyframe ")]


def test_slam_refuses_a_kf_init_it_cannot_run():
    from tests.test_gpu_sharded_solution import _cli
    rc, _, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--kf_init", "bogus"])
    assert rc == 2 and "--kf_init" in err
    rc, _, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--kf_init", "resect", "--ipus", "2"])
    assert rc == 2 and "one GPU" in err
