"""Landmark and keyframe seeding on the GPU (libgbp_mi355x_seed.so, gbp_poplar_amd/seed.py).

The kernels against the host twin (tests/sanitize/seed_math_main.cpp, the same header compiled as plain C++, run as a process with the
GPU math library's sinf / cosf restated): bit for bit, NaNs equal NaNs, over landmark counts around the wave and workgroup sizes,
degrees 0, 1, 2, 15, 16, 17 and a hub of 320 views, one camera only, inactive observations, a sparse selection, each optional output
left out, bases at and 4 bytes past a 16-byte boundary inside canary-filled buffers.  gbp_seed_keyframe against
gbp_slam_initialise_new_kf of the core library.  End to end only orderings are asked, so no number is recorded here: the triangulated
start has a lower initial metric than --avdepth_on's on every shipped sequence and the default loop stays healthy from it, bin/ba prints
the driver's trajectory, bin/slam runs a file whose points are all zero to the end (its final error: profiles/seed_landmarks.md),
examples/slam_from_observations.py runs and its device and host loops print the same numbers.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import post_support as ps
from tests import seed_support as ss
from tests.conftest import seq_path
from tests.test_gpu_post import CANARY, _all_to_all, _canaries_intact, _dev, _engine, _inputs, _ptr, _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "gbp_poplar_amd", "bin", "ba")
SLAM = os.path.join(ROOT, "gbp_poplar_amd", "bin", "slam")
SEQUENCES = ("fr1xyz", "fr1desk", "fr2robot2")


def _same_bits(a, b):
    """the same bits, except that every NaN equals every NaN (the sign and payload of a NaN are not pinned by IEEE 754 operations)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ss.compile_host(str(tmp_path_factory.mktemp("seed_host") / "seed_math"), sanitize=False)


def _degrees(n_lmks):
    d = np.array([2, 0, 1, 15, 16, 17] * (n_lmks // 6 + 1))[:n_lmks]
    if n_lmks > 6:
        d[5] = 320
    return d


def _one_camera(n_lmks):
    """C = 1: every landmark has one view or none"""
    g, _ = ss.degree_graph(np.arange(n_lmks) % 3 != 0, seed=21, n_cams=2)
    return ss.graph_of(1, n_lmks, np.zeros_like(g["cam_id"]), g["lmk_id"], g["K"], g["cam_mean"][:6], g["measurements"])


#        n_lmks, one camera, a third inactive, sparse selection, the output left out, 4-byte offset, NaN camera
CASES = [pytest.param(1, False, False, False, None, False, False, id="L1"),
         pytest.param(63, False, True, True, "lmk_priors_eta", True, False, id="L63-flags-select-no_eta-offset4"),
         pytest.param(65, False, True, False, "lmk_priors_lambda", False, False, id="L65-flags-no_lambda"),
         pytest.param(257, False, False, True, "n_views", True, True, id="L257-select-no_n_views-offset4-nan_camera"),
         pytest.param(257, False, True, False, None, False, False, id="L257-flags"),
         pytest.param(65, True, False, False, None, True, False, id="L65-one_camera-offset4")]


@pytest.mark.parametrize("n_lmks,one_camera,flags,sparse,left_out,offset,nan_camera", CASES)
def test_landmarks_equal_the_host_program(n_lmks, one_camera, flags, sparse, left_out, offset, nan_camera, host_exe, tmp_path):
    import torch
    from gbp_poplar_amd import seed
    g = _one_camera(n_lmks) if one_camera else ss.degree_graph(_degrees(n_lmks), seed=100 + n_lmks, noise=0.5, n_cams=320)[0]
    rng = np.random.default_rng(n_lmks)
    E = g["cam_id"].size
    if nan_camera:
        g["cam_mean"] = g["cam_mean"].copy()
        g["cam_mean"][6 * 7 + 4] = np.nan
    g["active_flag"] = (np.arange(E) % 3 != 1).astype(np.uint32) if flags else None
    select = (rng.uniform(size=n_lmks) < 0.3).astype(np.uint32) if sparse else None
    before = ss.initial_outputs(n_lmks)
    want = ss.run_host(host_exe, tmp_path, g, select=select, before=before, trig="device")
    if not one_camera and not sparse:
        assert want["n_views"].max() >= (214 if flags else 320) or n_lmks < 7
    ins = {k: _dev(g[k], offset) for k in ("cam_id", "lmk_start", "lmk_edges", "cam_mean", "measurements")}
    act = _dev(g["active_flag"], offset) if flags else (None, None)
    sel = _dev(select, offset) if sparse else (None, None)
    outs = {k: _dev(before[k], offset) for k, _, _ in ss.OUTPUTS}
    ws = torch.full((seed.workspace_bytes(g["n_cams"]) // 4 + 8,), CANARY, dtype=torch.int32, device="cuda")
    lib, opts = seed.load(), seed.default_options()
    K9 = (C.c_float * 9)(*[float(x) for x in g["K"]])
    results = []
    for _ in range(2):      # two launches: the same bits
        for k, _, _ in ss.OUTPUTS:
            outs[k][0].copy_(torch.from_numpy(before[k].view(np.int32) if before[k].dtype != np.float32 else before[k]))
        rc = lib.gbp_seed_landmarks(_stream(), g["n_cams"], n_lmks, E, *[_ptr(ins[k][0]) for k in ("cam_id", "lmk_start", "lmk_edges")], K9,
                                    _ptr(ins["cam_mean"][0]), _ptr(ins["measurements"][0]), _ptr(act[0]), _ptr(sel[0]), C.byref(opts),
                                    C.c_void_p(ws.data_ptr()), *[None if k == left_out else _ptr(outs[k][0]) for k, _, _ in ss.OUTPUTS])
        assert rc == 0, lib.gbp_seed_last_error()
        torch.cuda.synchronize()
        results.append({k: outs[k][0].cpu().numpy().view(dt) for k, _, dt in ss.OUTPUTS})
    got = results[0]
    for k, w, _ in ss.OUTPUTS:
        assert _canaries_intact(outs[k][1], w * n_lmks, offset), k
        assert _same_bits(results[1][k], got[k]), k
        if k == left_out:
            assert _same_bits(got[k], before[k]), k
            continue
        assert _same_bits(got[k], want[k]), (k, np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))[:8])
        if select is not None:      # a landmark that is not selected keeps every output
            assert _same_bits(got[k].reshape(-1, w)[select == 0], before[k].reshape(-1, w)[select == 0]), k
    for k in ins:
        assert _canaries_intact(ins[k][1], ins[k][0].numel(), offset), k
    assert (ws[seed.workspace_bytes(g["n_cams"]) // 4:] == CANARY).all()
    st = want["status"] if select is None else want["status"][select == 1]
    if one_camera:
        assert set(st.tolist()) == {ss.NO_VIEW, ss.ONE_VIEW}
    if nan_camera:
        assert (st & ss.NONFINITE).any()


@pytest.fixture(scope="module")
def tiny_beliefs():
    """the beliefs and priors of _tiny_problem (6 cameras x 60 landmarks all to all) after 12 passes of the default loop"""
    bal = _all_to_all(6, 60)
    K, state, steps = _inputs(bal)
    eng = _engine(bal, K)
    eng.upload(state)
    eng.linearise()
    eng.ba_loop(12, 0, steps, metrics=False)
    b, pri = eng.read(), eng.read_priors()
    eng.close()
    return b, pri


def test_keyframe_equals_the_core_librarys_host_function(tiny_beliefs):
    """cameras 0-3: the hand-made blocks (a row swap, an indefinite block, the zero block — singular —, condition 1e6), 4-9: the tiny problem's"""
    import torch
    from gbp_poplar_amd import hostlib, seed
    b, pri = tiny_beliefs
    h = ps.hand_made_beliefs()
    cbe = np.concatenate([h["cam_beliefs_eta"], b["cam_beliefs_eta"]]).astype(np.float32)
    cbl = np.concatenate([h["cam_beliefs_lambda"], b["cam_beliefs_lambda"]]).astype(np.float32)
    n_c = cbe.size // 6
    cpl = np.resize(np.asarray(pri["cam_priors_lambda"], np.float32), 36 * n_c)
    cpl[36:72] = cbl[36 * 9:]      # one full (not diagonal) prior block
    cpe0 = np.random.default_rng(3).normal(size=6 * n_c).astype(np.float32)
    for src in range(n_c - 1):
        want = cpe0.copy()
        with np.errstate(all="ignore"):
            hostlib.slam_initialise_new_kf(src, cbe, cbl, cpl, want)
        d = [torch.from_numpy(a.copy()).cuda() for a in (cbe, cbl, cpl, cpe0)]
        eta, mean = seed.keyframe(src, src + 1, *d)
        assert eta.data_ptr() == d[3].data_ptr()      # in place
        eta, mean = eta.cpu().numpy(), mean.cpu().numpy()
        assert _same_bits(eta, want), src
        assert _same_bits(np.delete(eta.reshape(-1, 6), src + 1, axis=0), np.delete(cpe0.reshape(-1, 6), src + 1, axis=0))
        with np.errstate(all="ignore"):
            cams = hostlib.belief_means(n_c, 60, cbe, cbl, b["lmk_beliefs_eta"], b["lmk_beliefs_lambda"])[0].reshape(-1, 6)
        assert _same_bits(mean, cams[src].astype(np.float32)), src
        if src == 2:      # the zero block: nothing finite, no fault
            assert not np.isfinite(want.reshape(-1, 6)[3]).any() and not np.isfinite(mean).any()


# ---- end to end ----
def _initial_and_health(bal, opts, **how):
    from gbp_poplar_amd import driver, hostlib
    K, state, _ = driver.build_inputs(bal, opts, hostlib, **how)
    eng = _engine(bal, K)
    eng.upload(state)
    eng.linearise()
    m0 = driver.metric(eng.eval())[0]
    last = eng.ba_loop(50, 0, int(opts.steps))[-1]
    eng.close()
    return m0, last, state


@pytest.mark.parametrize("name", SEQUENCES)
def test_triangulated_start_is_below_the_average_depth_start_and_stays_healthy(name):
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path(name))
    tri, last, state = _initial_and_health(bal, driver.Options(), lmk_init="triangulate")
    av, _, _ = _initial_and_health(bal, driver.Options(avdepth_on=True))
    print("%s: initial mean reprojection error %.3f px triangulated, %.3f px at average depth; after 50 passes %.3f px"
          % (name, tri, av, driver.metric(last)[0]))
    assert np.isfinite(tri) and tri < av
    assert last["n_nonfinite"] == 0 and last["n_nonpd"] == 0 and np.isfinite(last["sum_norm"])
    assert np.isfinite(state["lmk_priors_lambda"]).all() and (state["lmk_priors_lambda"].reshape(-1, 9)[:, 0] > 0).all()


def test_ba_lmk_init_triangulate_prints_the_drivers_trajectory():
    from gbp_poplar_amd import driver, hostlib
    from tests.test_gpu_sharded_solution import _cli
    rc, out, err = _cli([BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "12", "--lmk_init", "triangulate"])
    assert rc == 0, err[-2000:]
    assert "Triangulating the landmarks from their observations" in out
    init = re.search(r"Initial Reprojection error: (\S+) Cost (\S+)", out)
    rows = re.findall(r"Iter (\d+) // Reprojection error (\S+) // Cost (\S+) // n relins: (\d+) // n robust edges (\d+)", out)
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib, lmk_init="triangulate")
    eng = _engine(bal, K)
    traj = driver.run_ba(eng, state, opts, n_iters=12)
    eng.close()
    assert init and len(rows) == 12 == len(traj) - 1
    printed = [(-1, init.group(1), init.group(2), traj[0][3], traj[0][4])] + rows
    for (it, m, c, nr, nb), (i, mean, cost, n_relin, n_robust) in zip(printed, traj):      # six significant digits are printed
        assert int(it) == i and abs(float(m) - mean) <= 1e-5 * mean and abs(float(c) - cost) <= 1e-5 * cost, (it, m, mean, c, cost)
        assert (int(nr), int(nb)) == (n_relin, n_robust)


def test_example_slam_from_observations_runs_and_its_two_loops_agree():
    """examples/slam_from_observations.py: the device-tensor loop and the host-array loop print the same two numbers (the example
    asserts it itself; a difference is a non-zero exit)"""
    import sys
    from tests.test_gpu_sharded_solution import _cli
    rc, out, err = _cli([sys.executable, os.path.join(ROOT, "examples", "slam_from_observations.py")], timeout=120)
    assert rc == 0, err[-2000:]
    rows = re.findall(r"^(device|host) loop:\s+mean reprojection error (\S+) cost (\S+)$", out, flags=re.M)
    assert [r[0] for r in rows] == ["device", "host"] and rows[0][1:] == rows[1][1:], out
    assert np.isfinite([float(v) for r in rows for v in r[1:]]).all()


def _zeroed_points(tmp_path):
    from gbp_poplar_amd import hostlib
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    bal["points"] = np.zeros_like(bal["points"])
    path = str(tmp_path / "fr2robot2_no_points.txt")
    hostlib.bal_write(path, bal)
    return path, bal


def test_slam_lmk_init_triangulate_runs_a_file_without_points(tmp_path, monkeypatch):
    """bin/slam on fr2robot2 with every point of the file zero: to the end, every printed metric finite, the last metric's non-finite
    count (what --profile reports) zero.  The driver's loop on the same file: both health counters of the final metric zero."""
    import json
    from gbp_poplar_amd import driver, hostlib
    from tests.test_gpu_sharded_solution import _cli
    path, _ = _zeroed_points(tmp_path)
    monkeypatch.setenv("GC_PROFILE_LOG_DIR", str(tmp_path))
    rc, out, err = _cli([SLAM, "--bal_file", path, "--lmk_init", "triangulate", "--profile", "1"], timeout=120)
    assert rc == 0 and " Finished GBP." in out, err[-2000:]
    rows = re.findall(r"Iters (\d+) \(since last kf (\d+)\) // Reprojection error (\S+) // Cost (\S+)", out)
    assert len(rows) == 19 * 700 - 1 and out.count("Adding keyframe") == 18
    vals = np.array([[float(m), float(c)] for _, _, m, c in rows])
    init = re.search(r"Initial Reprojection error: (\S+) Cost (\S+)", out)
    assert np.isfinite(vals).all() and np.isfinite([float(init.group(1)), float(init.group(2))]).all()
    with open(os.path.join(str(tmp_path), "gbp_profile.json")) as f:
        prof = json.load(f)
    assert prof["n_nonfinite"] == 0 and np.isfinite(prof["final_mean_reproj_px"])
    bal = hostlib.bal_read(path)
    assert not np.asarray(bal["points"]).any()
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True, lmk_init="triangulate")
    eng = _engine(bal, K)
    traj = driver.run_slam(eng, hostlib, bal, state, extra, opts, lmk_init="triangulate", eval_every=700)
    ev = eng.eval()
    eng.close()
    print("slam fr2robot2 without points: final mean reprojection error %.4f px (bin/slam), %.4f px (driver)"
          % (vals[-1, 0], traj[-1][1]))
    assert np.isfinite([t[1] for t in traj]).all() and ev["n_nonfinite"] == 0 and ev["n_nonpd"] == 0
