"""Camera location on the GPU (libgbp_mi355x_locate.so, gbp_poplar_amd/locate.py).

The kernel against the host twin (tests/sanitize/locate_math_main.cpp, the same header compiled as plain C++, run as a process): bit
for bit, NaNs equal NaNs, over 1, 3, 5 and 257 cameras whose degrees cycle through 0, 2, 3, 5, 6, 63, 64, 65, 127, 129 and 1 000 (the
register-resident limit, the lane stride and its neighbours), rounds 1 and 3, with and without active_flag, lmk_use, select and
cam_edges, each optional output left out in turn, bases at and 4 bytes past a 16-byte boundary inside canary-filled buffers, one NaN
landmark, two launches; unselected cameras and unused edges keep their bytes.  The numpy face against the tensor face.  On the solved
map of each shipped sequence every camera with 20 mapped views or more is located with no guess, and locate -> resect ends where resect
from the camera's own solved pose ends (the figures: profiles/locate_cameras.md).  The case resect cannot do: starts 2 scene units and
90 degrees off with 30 % wrong matches.  run_slam(kf_init="locate") stays healthy and bin/slam --kf_init locate prints its trajectory.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import locate_support as ls
from tests import resect_support as rs
from tests.conftest import seq_path
from tests.test_gpu_post import _canaries_intact, _dev, _engine, _ptr, _stream
from tests.test_gpu_seed import _same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAM = os.path.join(ROOT, "gbp_poplar_amd", "bin", "slam")
SEQUENCES = ("fr1xyz", "fr1desk", "fr2robot2")
FACTOR = 8.0
CYCLE = [0, 2, 3, 5, 6, 63, 64, 65, 127, 129, 1000]
INPUTS = ("lmk_id", "cam_start", "lmk_mean", "measurements")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ls.compile_host(str(tmp_path_factory.mktemp("locate_host") / "locate_math"), sanitize=False)


def _scene(n_cams, with_edges, nan_landmark):
    g, _, _ = ls.scene(np.resize(CYCLE, n_cams), seed=300 + n_cams, outlier_share=0.2, noise=0.5, n_lmks=1000)
    if with_edges:      # the same edges in another file order: cam_edges is needed
        perm = np.random.default_rng(n_cams).permutation(g["lmk_id"].size)
        g = rs.graph_of(n_cams, 1000, g["cam_id"][perm], g["lmk_id"][perm], g["K"], g["cam_mean"], g["lmk_mean"],
                        g["measurements"].reshape(-1, 2)[perm])
    if nan_landmark:
        g["lmk_mean"] = g["lmk_mean"].copy()
        g["lmk_mean"][3 * 18 + 1] = np.nan
    return g


#        n_cams, rounds, active_flag, lmk_use, select, cam_edges, the output left out, 4-byte offset, NaN landmark
CASES = [pytest.param(1, 1, False, False, False, False, None, False, False, id="C1-r1"),
         pytest.param(3, 3, True, True, False, True, "inlier", True, False, id="C3-r3-flags-use-edges-no_inlier-offset4"),
         pytest.param(5, 1, False, False, True, False, "report", False, False, id="C5-r1-select-no_report"),
         pytest.param(5, 3, True, False, False, True, "n_views", True, False, id="C5-r3-flags-edges-no_n_views-offset4"),
         pytest.param(257, 3, True, True, True, True, "n_inliers", True, True, id="C257-r3-flags-use-select-edges-no_n_inliers-offset4-nan_landmark"),
         pytest.param(257, 1, False, False, False, False, None, False, False, id="C257-r1")]


@pytest.mark.parametrize("n_cams,rounds,flags,use,sparse,with_edges,left_out,offset,nan_landmark", CASES)
def test_cameras_equal_the_host_program(n_cams, rounds, flags, use, sparse, with_edges, left_out, offset, nan_landmark, host_exe, tmp_path):
    import torch
    from gbp_poplar_amd import locate
    g = _scene(n_cams, with_edges, nan_landmark)
    rng = np.random.default_rng(n_cams)
    E = g["lmk_id"].size
    g["active_flag"] = (np.arange(E) % 3 != 1).astype(np.uint32) if flags else None
    g["lmk_use"] = (np.arange(1000) % 7 != 3).astype(np.uint32) if use else None
    select = (rng.uniform(size=n_cams) < 0.6).astype(np.uint32) if sparse else None
    before = ls.initial_outputs(g)
    want = ls.run_host(host_exe, tmp_path, g, opts={"rounds": rounds}, select=select, before=before, with_inlier=left_out != "inlier", trig="device")
    if n_cams > 11 and not sparse and not flags:
        assert set(CYCLE) <= set(want["n_views"].tolist())
    ins = {k: _dev(g[k], offset) for k in INPUTS}
    opt = {k: _dev(a, offset) if a is not None else (None, None)
           for k, a in (("cam_edges", g["cam_edges"]), ("active_flag", g["active_flag"]), ("lmk_use", g["lmk_use"]), ("select", select))}
    outs = {k: _dev(before[k], offset) for k, _, _ in ls.OUTPUTS}
    lib, opts = locate.load(), locate.default_options(rounds=rounds)
    K9 = (C.c_float * 9)(*[float(x) for x in g["K"]])
    results = []
    for _ in range(2):      # two launches: the same bits
        for k, _, _ in ls.OUTPUTS:
            outs[k][0].copy_(torch.from_numpy(before[k].view(np.int32) if before[k].dtype != np.float32 else before[k]))
        rc = lib.gbp_locate_cameras(_stream(), n_cams, 1000, E, _ptr(ins["lmk_id"][0]), _ptr(ins["cam_start"][0]), _ptr(opt["cam_edges"][0]), K9,
                                    _ptr(ins["lmk_mean"][0]), _ptr(ins["measurements"][0]), _ptr(opt["active_flag"][0]), _ptr(opt["lmk_use"][0]),
                                    _ptr(opt["select"][0]), C.byref(opts), _ptr(outs["cam_mean"][0]),
                                    *[None if k == left_out else _ptr(outs[k][0]) for k, _, _ in ls.OUTPUTS[1:]])
        assert rc == 0, lib.gbp_locate_last_error()
        torch.cuda.synchronize()
        results.append({k: outs[k][0].cpu().numpy().view(dt) for k, _, dt in ls.OUTPUTS})
    got = results[0]
    sizes = ls.sizes(g)
    for k, w, _ in ls.OUTPUTS:
        assert _canaries_intact(outs[k][1], sizes[k], offset), k
        assert _same_bits(results[1][k], got[k]), k
        if k == left_out:
            assert _same_bits(got[k], before[k]), k
            continue
        assert _same_bits(got[k], want[k]), (k, np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))[:8])
        if select is not None:      # a camera that is not selected keeps every output
            keep = (select == 0)[g["cam_id"]] if w is None else select == 0
            assert _same_bits(got[k].reshape(-1, w or 1)[keep], before[k].reshape(-1, w or 1)[keep]), k
    for k in ins:
        assert _canaries_intact(ins[k][1], ins[k][0].numel(), offset), k
    st = want["status"] if select is None else want["status"][select == 1]
    if n_cams > 11:
        assert (st == 0).any() and (st & ls.NO_VIEW).any() and (st & ls.FEW_VIEWS).any()
        if left_out != "inlier":      # unused edges and the edges of cameras that are not located keep their bytes; the others are 0 or 1
            written = want["inlier"] != before["inlier"]
            assert written.any() and not written.all() and set(want["inlier"][written].tolist()) <= {0, 1}


def test_numpy_face_equals_the_tensor_face_and_out_writes_in_place():
    import torch
    from gbp_poplar_amd import locate
    g = _scene(11, True, False)
    args = ("lmk_id", "cam_start", "cam_edges")
    host = locate.cameras(*[g[k] for k in args], g["K"], g["lmk_mean"], g["measurements"])
    dev = lambda a, ints=False: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if ints else np.ascontiguousarray(a)).cuda()
    status = torch.full((11,), 77, dtype=torch.int32, device="cuda")
    res = locate.cameras(*[dev(g[k], True) for k in args], g["K"], dev(g["lmk_mean"]), dev(g["measurements"]), out={"status": status})
    assert res["status"].data_ptr() == status.data_ptr()      # in place
    assert set(host) == set(res) == {"cam_mean", "inlier", "report", "status", "n_views", "n_inliers"}
    for k in host:
        assert _same_bits(host[k], res[k].cpu().numpy().view(host[k].dtype)), k
    assert host["status"].dtype == np.uint32 and host["n_views"].tolist() == CYCLE and (status.cpu().numpy() != 77).all()
    located = (host["status"] & locate.NOT_LOCATED) == 0
    assert located.sum() >= 5 and (host["cam_mean"].reshape(-1, 6)[located] != 0).all() and not host["cam_mean"].reshape(-1, 6)[~located].any()


def _costs(resect, g, K, start, active, select):
    r = resect.cameras(g["lmk_id"], g["cam_start"], g["cam_edges"], K, start, g["lmk_mean"], g["measurements"], active_flag=active, select=select)
    return r, r["report"].reshape(-1, 4)[:, 1]


@pytest.mark.parametrize("name", SEQUENCES)
def test_every_camera_of_a_solved_map_is_located_with_no_guess(name):
    """locate -> resect over the observations that agree, against resect over the same observations from the camera's own solved pose:
    both descend the same cost, so they may differ by what a run leaves undone — measured on the pair: what a restart of the second run
    from its own result still gains, or the rounding of a float32 sum of n_views terms if that is larger — times 8"""
    from gbp_poplar_amd import locate, resect
    from tests.test_gpu_resect import _solved_map
    bal, K, cams, pts, z = _solved_map(name)
    n_c = bal["n_cams"]
    idx = resect.index(bal["cam_id"], n_c)
    g = {"lmk_id": bal["lmk_id"], "cam_start": idx[0], "cam_edges": idx[1], "lmk_mean": pts, "measurements": z}
    n = np.bincount(bal["cam_id"], minlength=n_c)
    select = (n >= 20).astype(np.uint32)
    loc = locate.cameras(bal["lmk_id"], *idx, K, pts, z, select=select)
    sel = select == 1
    assert sel.sum() >= 2 and not (loc["status"][sel] & locate.NOT_LOCATED).any(), loc["status"][sel]
    a, cost_a = _costs(resect, g, K, loc["cam_mean"], loc["inlier"], select)
    b, cost_b = _costs(resect, g, K, cams.astype(np.float32).ravel(), loc["inlier"], select)
    _, cost_b2 = _costs(resect, g, K, b["cam_mean"], loc["inlier"], select)
    margin = FACTOR * np.maximum(np.abs(cost_b - cost_b2), 2.0 ** -24 * loc["n_views"] * cost_b)
    share = loc["n_inliers"][sel] / loc["n_views"][sel]
    print("%s: %d of %d cameras with 20 views or more, all located; inlier share %.3f .. %.3f; located pose %.3e from the solved pose (relative, "
          "worst); cost after locate -> resect %.4f, after resect from the solved pose %.4f (sums); worst excess %.3e (margin there %.3e)"
          % (name, sel.sum(), n_c, share.min(), share.max(), rs.pose_error(loc["cam_mean"].reshape(-1, 6)[sel], cams[sel]), cost_a[sel].sum(),
             cost_b[sel].sum(), (cost_a - cost_b)[sel].max(), margin[sel][np.argmax((cost_a - cost_b)[sel])]))
    assert not ((a["status"] | b["status"])[sel] & (resect.NO_VIEW | resect.FEW_VIEWS | resect.NONFINITE)).any()
    assert (cost_a[sel] <= cost_b[sel] + margin[sel]).all(), np.flatnonzero(sel & ~(cost_a <= cost_b + margin))


def test_starts_resect_cannot_use_are_located_among_wrong_matches():
    """every start 2 scene units and 90 degrees from the truth, 30 % of the pixels 80 px off, 0.5 px noise on the rest: resect alone leaves
    most cameras stalled or far away; locate -> resect ends where resect FROM THE TRUTH over the same observations ends, to 8 x what
    float32 costs a resection there (the numpy definition of the resection, float32 against float64)"""
    from gbp_poplar_amd import locate, resect
    g, gt, outlier = ls.scene([30, 64, 100, 200] * 6, seed=41, outlier_share=0.3, noise=0.5)      # (24 cameras: the share is stable over the draw of the starts)
    rng = np.random.default_rng(2)
    start = rs.perturbed(gt, rng, trans=2.0, rot_deg=90.0).ravel()
    args = (g["lmk_id"], g["cam_start"], g["cam_edges"], g["K"])
    alone = resect.cameras(*args, start, g["lmk_mean"], g["measurements"])
    far = np.max(np.abs(alone["cam_mean"].reshape(-1, 6) - gt), axis=1) > 0.1
    lost = far | ((alone["status"] & resect.NOT_RESECTED) != 0)
    assert lost.mean() > 0.5, (alone["status"], far)      # the test proves something
    loc = locate.cameras(*args, g["lmk_mean"], g["measurements"])
    assert not (loc["status"] & locate.NOT_LOCATED).any() and np.array_equal(loc["inlier"], (~outlier).astype(np.uint32))
    a = resect.cameras(*args, loc["cam_mean"], g["lmk_mean"], g["measurements"], active_flag=loc["inlier"])
    b = resect.cameras(*args, gt.astype(np.float32).ravel(), g["lmk_mean"], g["measurements"], active_flag=loc["inlier"])
    gm = dict(g, cam_mean=gt.astype(np.float32).ravel(), active_flag=loc["inlier"])
    r64, r32 = rs.resect_numpy(gm, np.float64), rs.resect_numpy(gm, np.float32)
    e, bound = rs.pose_error(a["cam_mean"], b["cam_mean"]), rs.pose_error(r32["cam_mean"], r64["cam_mean"])
    print("resect alone: %d of %d cameras stalled or more than 0.1 from the truth; locate -> resect against resect from the truth: %.3e "
          "(numpy float32 against float64 %.3e, bound %.3e); from the truth %.3e"
          % (lost.sum(), lost.size, e, bound, FACTOR * bound, rs.pose_error(a["cam_mean"], gt)))
    assert not ((a["status"] | b["status"]) & resect.NOT_RESECTED).any()
    assert e <= FACTOR * bound


@pytest.fixture(scope="module")
def slam_runs():
    """kf_init -> (the driver's trajectory of run_slam on fr2robot2 at 30 iterations between keyframes, its final metric, its log lines,
    the number of cameras)"""
    from gbp_poplar_amd import driver, hostlib
    runs = {}
    for kf_init in ("resect", "locate"):
        bal = hostlib.bal_read(seq_path("fr2robot2"))
        opts = driver.Options()
        K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True)
        eng = _engine(bal, K)
        log = []
        traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=30, kf_init=kf_init, log=log.append)
        runs[kf_init] = (traj, eng.eval(), log, int(bal["n_cams"]))
        eng.close()
    return runs


def test_run_slam_with_located_keyframes_stays_healthy_and_ends_no_worse_than_resect(slam_runs):
    traj, ev, log, n_cams = slam_runs["locate"]
    said = [l for l in log if l.startswith("Keyframe ")]
    print("final mean reprojection error %.4f px with kf_init=locate (%d keyframes located, %d resected from the copy, %d copied), %.4f px with "
          "kf_init=resect" % (traj[-1][1], sum("located" in l for l in said), sum("pose resected" in l for l in said), sum("copied" in l for l in said),
                              slam_runs["resect"][0][-1][1]))
    assert len(said) == n_cams - 2 and any("located" in l for l in said)      # one line per keyframe added
    assert ev["n_nonfinite"] == 0 and ev["n_nonpd"] == 0 and np.isfinite([t[1] for t in traj]).all()
    assert traj[-1][1] <= slam_runs["resect"][0][-1][1]


def test_slam_kf_init_locate_prints_the_drivers_trajectory(slam_runs):
    from tests.test_gpu_sharded_solution import _cli
    traj, _, log, n_cams = slam_runs["locate"]
    rc, out, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--iters_between_kfs", "30", "--kf_init", "locate"], timeout=120)
    assert rc == 0 and " Finished GBP." in out, err[-2000:]
    init = re.search(r"Initial Reprojection error: (\S+) Cost (\S+)", out)
    rows = re.findall(r"Iters \d+ \(since last kf \d+\) // Reprojection error (\S+) // Cost (\S+)", out)
    printed = [(init.group(1), init.group(2))] + rows
    assert len(printed) == len(traj) == (n_cams - 1) * 30
    for (m, c), (_, mean, cost, _, _) in zip(printed, traj):      # six significant digits are printed
        assert abs(float(m) - mean) <= 1e-5 * mean and abs(float(c) - cost) <= 1e-5 * cost, (m, mean, c, cost)
    said = re.findall(r"^Keyframe \d+: pose (located|resected|copied)", out, flags=re.M)
    assert said == [re.match(r"Keyframe \d+: pose (located|resected|copied)", l).group(1) for l in log if l.startswith("Keyframe ")]


def test_slam_refuses_locate_on_more_than_one_gpu():
    from tests.test_gpu_sharded_solution import _cli
    rc, _, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--kf_init", "locate", "--ipus", "2"])
    assert rc == 2 and "one GPU" in err
    rc, _, err = _cli([SLAM, "--bal_file", seq_path("fr2robot2"), "--kf_init", "bogus"])
    assert rc == 2 and "locate" in err
