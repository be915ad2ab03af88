"""Camera resection without a GPU (gbp_poplar_amd/resect/, include/gbp_mi355x_resect.h).

1. The arithmetic — resect/resect_math.hpp, the header the kernel is built from — compiled for the host into a stand-alone program under
   ASan + UBSan (tests/sanitize/resect_math_main.cpp) and compared with the INDEPENDENT numpy implementation of the header's definition
   in tests/resect_support.py.  Per case family the program's largest pose difference from the numpy float64 run may be 8 x the numpy
   float32 run's largest difference from that same float64 run (computed here, on the family: no recorded number); the status word and
   the view count agree on every camera.  That the status is a property of the inputs is the generator's business: cameras with a
   landmark whose depth lies within 10 % of zero, or whose view count is exactly min_views, are deselected (at most half), and the test
   asserts that deselected cameras keep every output.  Families: a hand-made scene with 6, 63, 64, 65, 128 and 300 views per camera
   (0.5 px noise, every fifth camera with 10 % of its pixels 80 px off, starts 0.05 and 2 degrees from the truth), gbp_synth_generate
   graphs with exact and with the generator's noisy pixels.  On the cameras of the hand-made scene with 64 views or more the final cost
   is below the start cost and the result is closer to the true pose than the start.  The deliberate family (no view, every view
   inactive, 5 views, every landmark excluded, a zero rotation vector, a NaN landmark, a landmark behind the camera, duplicate edges, an
   index entry out of range) must give exactly the documented bit and touch nothing else.

2. gbp_resect_index against a numpy stable argsort; cam_edges = NULL against the identity index.

3. The C-ABI of libgbp_mi355x_resect.so: `nm -D` equals the header, every export goes through the guard macro, the argument checks
   answer GBP_ERR_INVALID and name the argument before anything touches HIP, the error text is the library's own.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import resect_support as rs
from tests import stateless_cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0      # tests/test_seed_cpu.py's
DEGREES = [6, 63, 64, 65, 128, 300]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return rs.compile_host(str(tmp_path_factory.mktemp("resect_host") / "resect_math"), sanitize=True)


def _synth(noisy):
    """the generator's graph at its true points, every camera started 0.05 and 2 degrees from its true pose; the index is resect.index's
    (cam_edges given, whatever the file order)"""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.synth_generate(12, 300, 6, 7, ground_truth=True)
    K = driver.k_matrix(bal)
    cams = np.asarray(bal["gt_cameras"], np.float64).astype(np.float32).astype(np.float64).reshape(-1, 6)
    pts = np.asarray(bal["gt_points"], np.float64).astype(np.float32)
    cam_id, lmk_id = bal["cam_id"].astype(np.int64), bal["lmk_id"].astype(np.int64)
    z = np.asarray(bal["observations"], np.float64).reshape(-1, 2) if noisy else rs.project64(cams, pts, cam_id, lmk_id, K)
    start = rs.perturbed(cams, np.random.default_rng(3))
    return rs.graph_of(bal["n_cams"], bal["n_lmks"], cam_id, lmk_id, K, start, pts, z), cams


FAMILIES = {"degrees": lambda: rs.degree_scene(DEGREES * 5, seed=11), "synth_exact": lambda: _synth(False), "synth_noisy": lambda: _synth(True)}
_cache = {}


def _family(name, host_exe, tmp):
    """(graph, true poses, select, numpy float64 run, numpy float32 run, prior Lambdas, outputs before, host program's outputs)"""
    if name not in _cache:
        g, gt = FAMILIES[name]()
        r64, r32 = rs.resect_numpy(g, np.float64), rs.resect_numpy(g, np.float32)
        select = (~rs.ambiguous(r64)).astype(np.uint32)
        before = rs.initial_outputs(g["cam_mean"])
        lam = np.random.default_rng(5).normal(size=36 * g["n_cams"]).astype(np.float32)
        _cache[name] = (g, gt, select, r64, r32, lam, before, rs.run_host(host_exe, tmp, g, select=select, before=before, priors_lambda=lam))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_host_program_against_the_numpy_definition(name, host_exe, tmp_path):
    g, _, select, r64, r32, lam, before, out = _family(name, host_exe, tmp_path)
    sel = select == 1
    assert sel.mean() >= 0.5, "the generator rejected most of the family"
    for k, w, _ in rs.OUTPUTS:      # deselected cameras: nothing is touched
        assert np.array_equal(out[k].reshape(-1, w)[~sel], before[k].reshape(-1, w)[~sel]), k
    # the status word and the view count: every selected camera, nothing excluded
    assert np.array_equal(out["status"][sel], r64["status"][sel]) and np.array_equal(out["n_views"][sel], r64["n_views"][sel])
    assert np.array_equal(r32["status"][sel], r64["status"][sel]), "the float32 run of the definition takes another branch"
    done = sel & ((r64["status"] & (rs.NO_VIEW | rs.FEW_VIEWS | rs.NONFINITE)) == 0)
    assert done.sum() >= 0.5 * sel.size
    if name == "degrees":
        assert (r64["status"][done] == 0).all() and r64["n_views"].max() == 300
    x = out["cam_mean"].reshape(-1, 6)
    e, b = rs.pose_error(x[done], r64["cam_mean"][done]), rs.pose_error(r32["cam_mean"][done], r64["cam_mean"][done])
    print("%s: %d of %d cameras selected, %d resected; pose error %.3e (numpy float32 %.3e, bound %.3e)"
          % (name, sel.sum(), sel.size, done.sum(), e, b, FACTOR * b))
    assert e <= FACTOR * b
    # what else is written: the information matrix is symmetric, H / var of the accepted pass; the report; the prior eta's row dots
    info, rep = out["cam_info"].reshape(-1, 6, 6)[done], out["report"].reshape(-1, 4)[done]
    assert np.array_equal(info, info.transpose(0, 2, 1)) and (info[:, np.arange(6), np.arange(6)] > 0).all()
    assert (rep[:, 1] < rep[:, 0]).all() and (rep[:, 2] > 0).all() and (rep[:, 3] >= np.float32(1e-9)).all()
    # (the start cost: a sum of at most 300 positive fp32 terms of residuals of several pixels, each good to 1e-4 or so)
    assert np.allclose(rep[:, 0], r64["report"][done][:, 0], rtol=1e-3)
    assert np.array_equal(out["cam_priors_eta"].reshape(-1, 6)[done], rs.eta_numpy(lam, x)[done])


def test_resection_moves_towards_the_true_pose_with_64_views_or_more(host_exe, tmp_path):
    g, gt, select, r64, _, _, _, out = _family("degrees", host_exe, tmp_path)
    many = (select == 1) & (r64["n_views"] >= 64)
    assert many.sum() == 20      # 64, 65, 128 and 300 views, five cameras each, every fifth camera with outliers
    rep = out["report"].reshape(-1, 4)[many]
    d0 = np.linalg.norm(g["cam_mean"].reshape(-1, 6).astype(np.float64) - gt, axis=1)[many]
    d1 = np.linalg.norm(out["cam_mean"].reshape(-1, 6).astype(np.float64) - gt, axis=1)[many]
    print("start %.4f from the truth at most, result %.4f at most" % (d0.max(), d1.max()))
    assert (rep[:, 1] < rep[:, 0]).all() and (d1 < d0).all()


def _deliberate():
    """one camera per case; cameras 3 and 5 see landmarks of their own (20-39 excluded by lmk_use, 40 is NaN), camera 6 also landmark 41,
    which lies behind it"""
    rng = np.random.default_rng(5)
    base, gt = rs.degree_scene([0, 20, 5, 20, 20, 20, 20, 10, 20, 20], seed=9, outliers=False, n_lmks=20)
    cam_id, lmk_id = base["cam_id"].astype(np.int64), base["lmk_id"].astype(np.int64)
    pts = np.concatenate([base["lmk_mean"].reshape(-1, 3), np.zeros((22, 3), np.float32)])
    pts[20:40] = np.concatenate([rng.uniform(-2, 2, (20, 2)), rng.uniform(4, 8, (20, 1))], axis=1)
    pts[40] = [0.3, -0.2, 5.0]
    pts[41] = [0.5, 0.5, -6.0]
    first3 = np.flatnonzero(cam_id == 3)[0]
    lmk_id[cam_id == 3] = np.arange(20, 40)
    lmk_id[np.flatnonzero(cam_id == 5)[7]] = 40
    lmk_id[np.flatnonzero(cam_id == 6)[3]] = 41
    dup = np.flatnonzero(cam_id == 7)                     # duplicate edges: every edge of camera 7 twice
    order = np.concatenate([np.arange(dup[-1] + 1), dup, np.arange(dup[-1] + 1, cam_id.size)])
    cam_id, lmk_id = cam_id[order], lmk_id[order]
    z = rs.project64(gt, pts, cam_id, lmk_id, rs.K_SYNTH) + 0.5 * rng.normal(size=(cam_id.size, 2))
    pts[40] = np.nan
    active = np.ones(cam_id.size, np.uint32)
    active[cam_id == 1] = 0
    use = np.ones(42, np.uint32)
    use[20:40] = 0
    start = base["cam_mean"].reshape(-1, 6).copy()
    start[4, 3:] = 0.0
    g = rs.graph_of(10, 42, cam_id, lmk_id, rs.K_SYNTH, start, pts, z, active_flag=active, lmk_use=use)
    g["cam_edges"] = g["cam_edges"].copy()
    g["cam_edges"][g["cam_start"][8] + 2] = 1000000      # an entry out of range
    assert first3 == g["cam_start"][3]
    return g


def test_deliberate_cases_give_the_documented_bit_and_touch_nothing_else(host_exe, tmp_path):
    g = _deliberate()
    before = rs.initial_outputs(g["cam_mean"])
    lam = np.random.default_rng(6).normal(size=360).astype(np.float32)
    out = rs.run_host(host_exe, tmp_path, g, before=before, priors_lambda=lam)
    r64 = rs.resect_numpy(g, np.float64)
    #        no view | all inactive | 5 views | all excluded | zero rotation | NaN landmark | one behind | duplicates | bad entry | ordinary
    want = [rs.NO_VIEW, rs.NO_VIEW, rs.FEW_VIEWS, rs.NO_VIEW, rs.NONFINITE, rs.NONFINITE, rs.BEHIND, 0, rs.BAD_INDEX, 0]
    assert out["status"].tolist() == r64["status"].tolist() == want
    assert out["n_views"].tolist() == r64["n_views"].tolist() == [0, 0, 5, 0, 20, 20, 20, 20, 19, 20]
    for k, w, _ in rs.OUTPUTS[:4]:      # cameras 0-5: only status and n_views are written
        assert np.array_equal(out[k][:6 * w], before[k][:6 * w]), k
    x, rep = out["cam_mean"].reshape(-1, 6)[6:], out["report"].reshape(-1, 4)[6:]
    assert np.isfinite(x).all() and np.isfinite(out["cam_info"][6 * 36:]).all() and (rep[:, 1] < rep[:, 0]).all()
    assert (x != before["cam_mean"].reshape(-1, 6)[6:]).any(axis=1).all()
    assert np.array_equal(out["cam_priors_eta"].reshape(-1, 6)[6:], rs.eta_numpy(lam, out["cam_mean"])[6:])
    r32 = rs.resect_numpy(g, np.float32)
    e, b = rs.pose_error(x, r64["cam_mean"][6:]), rs.pose_error(r32["cam_mean"][6:], r64["cam_mean"][6:])
    print("resected cameras of the deliberate family: pose error %.3e (numpy float32 %.3e)" % (e, b))
    assert e <= FACTOR * b


def test_a_camera_no_step_improves_is_stalled_and_keeps_its_start_bits(host_exe, tmp_path):
    """max_passes = 1: the first pass is the only one, so no step is accepted — the pose is the start pose's bits, the rest is written"""
    g, _ = rs.degree_scene([64, 65], seed=4)
    out = rs.run_host(host_exe, tmp_path, g, opts={"max_passes": 1})
    assert out["status"].tolist() == [rs.STALLED, rs.STALLED] and out["n_views"].tolist() == [64, 65]
    assert np.array_equal(out["cam_mean"].view(np.uint32), g["cam_mean"].view(np.uint32))
    rep = out["report"].reshape(-1, 4)
    assert np.array_equal(rep[:, 0], rep[:, 1]) and not rep[:, 2].any() and (rep[:, 3] == np.float32(1e-3)).all()


def test_a_reversed_or_overlong_range_is_clamped_and_flagged(host_exe, tmp_path):
    g, _ = rs.degree_scene([64, 64, 64], seed=3)
    good = rs.run_host(host_exe, tmp_path, g)
    g["cam_start"] = g["cam_start"].copy()
    g["cam_start"][3] = 500                      # camera 2: a range past the end
    out = rs.run_host(host_exe, tmp_path, g)
    assert out["status"].tolist() == [0, 0, rs.BAD_INDEX] and out["n_views"].tolist() == [64, 64, 64]
    assert np.array_equal(out["cam_mean"], good["cam_mean"])


def test_plain_least_squares_when_huber_is_not_positive(host_exe, tmp_path):
    """huber_px <= 0: every weight is 1 — the report's costs are half the summed squared residuals, and on a camera with outliers the
    result differs from the robust one"""
    g, _ = rs.degree_scene([128], seed=8)
    plain, robust = rs.run_host(host_exe, tmp_path, g, opts={"huber_px": 0.0}), rs.run_host(host_exe, tmp_path, g)
    r64 = rs.resect_numpy(g, np.float64, opts={"huber_px": 0.0})
    z = rs.project64(g["cam_mean"], g["lmk_mean"], g["cam_id"].astype(np.int64), g["lmk_id"].astype(np.int64), g["K"])
    half = 0.5 * np.sum((z - g["measurements"].reshape(-1, 2).astype(np.float64)) ** 2)
    assert abs(plain["report"][0] - half) <= 1e-4 * half and plain["report"][0] > robust["report"][0]
    assert plain["status"].tolist() == r64["status"].tolist() == [0]
    assert rs.pose_error(plain["cam_mean"], r64["cam_mean"]) < 1e-3 and not np.array_equal(plain["cam_mean"], robust["cam_mean"])


# ---- gbp_resect_index ----
@pytest.mark.parametrize("case", ["random", "sorted", "unobserved", "empty"])
def test_index_is_the_stable_argsort(case):
    from gbp_poplar_amd import resect
    rng = np.random.default_rng(17)
    n_cams = 40
    if case == "random":
        cam_id = rng.integers(0, n_cams, 500)
    elif case == "sorted":
        cam_id = np.sort(rng.integers(0, n_cams, 300))
    elif case == "unobserved":
        cam_id = rng.choice(np.arange(0, n_cams, 3), 200)
    else:
        cam_id = np.zeros(0, np.int64)
    start, edges = resect.index(cam_id, n_cams)
    want_start, want_edges = rs.index_numpy(cam_id, n_cams)
    assert start.dtype == edges.dtype == np.uint32 and np.array_equal(start, want_start) and np.array_equal(edges, want_edges)
    resect.check_index(start, edges)
    resect.check_index(start, None)
    if case == "sorted":
        assert np.array_equal(edges, np.arange(300))
    if case == "unobserved":
        assert (np.diff(start.astype(np.int64))[1::3] == 0).all()


def test_index_refuses_an_id_out_of_range():
    from gbp_poplar_amd import resect
    with pytest.raises(resect.ResectError, match=r"cam_id\[2\]"):
        resect.index([0, 1, 5, 2], 5)


def test_no_cam_edges_is_the_identity_index(host_exe, tmp_path):
    g, _ = rs.degree_scene(DEGREES, seed=2)
    assert g["cam_edges"] is None
    a = rs.run_host(host_exe, tmp_path, g)
    b = rs.run_host(host_exe, tmp_path, dict(g, cam_edges=np.arange(g["lmk_id"].size, dtype=np.uint32)))
    for k, _, _ in rs.OUTPUTS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- the C-ABI ----
EXPORTS = ["gbp_resect_abi_version", "gbp_resect_cameras", "gbp_resect_check_index", "gbp_resect_default_options", "gbp_resect_index",
           "gbp_resect_last_error"]


def test_library_exports_the_header_and_nothing_else():
    from gbp_poplar_amd import resect
    stateless_cabi.check_exports(resect, "gbp_mi355x_resect.h", EXPORTS, 1)


def test_every_export_is_defined_through_the_guard_macro():
    stateless_cabi.check_guard("resect", "gbp_mi355x_resect.h", EXPORTS)


def test_default_options_are_the_headers():
    from gbp_poplar_amd import resect
    o = resect.default_options()
    assert (o.max_passes, o.min_views, o.huber_px, o.lambda0, o.reproj_meas_var) == (10, 6, 5.0, np.float32(1e-3), 4.0)
    assert resect.load().gbp_resect_default_options(None) == -1 and b"opts" in resect.load().gbp_resect_last_error()
    with pytest.raises(TypeError, match="no field"):
        resect.default_options(min_parallax=1.0)


P = C.c_void_p(64)      # any non-NULL address: a call that fails its argument checks touches neither the array nor HIP


def _cameras_ok():
    from gbp_poplar_amd import resect
    return dict(n_cams=2, n_lmks=3, n_edges=4, lmk_id=P, cam_start=P, cam_edges=P, K=(C.c_float * 9)(), lmk_mean=P, measurements=P, active_flag=P,
                lmk_use=P, select=P, opts=C.pointer(resect.default_options()), cam_mean=P, cam_priors_lambda=P, cam_priors_eta=P, cam_info=P, report=P,
                status=P, n_views=P)


@pytest.mark.parametrize("change,named", [
    ({"lmk_id": None}, "lmk_id"), ({"cam_start": None}, "cam_start"), ({"K": None}, "K"), ({"lmk_mean": None}, "lmk_mean"),
    ({"measurements": None}, "measurements"), ({"cam_mean": None}, "cam_mean"), ({"status": None}, "status"), ({"n_lmks": 0}, "n_lmks"),
    ({"cam_priors_lambda": None}, "cam_priors_lambda"),
    ({"opts": "max_passes=0"}, "max_passes"), ({"opts": "min_views=2"}, "min_views"), ({"opts": "huber_px=nan"}, "huber_px"),
    ({"opts": "lambda0=0"}, "lambda0"), ({"opts": "lambda0=-1"}, "lambda0"), ({"opts": "lambda0=nan"}, "lambda0"),
    ({"opts": "reproj_meas_var=0"}, "reproj_meas_var"), ({"opts": "reproj_meas_var=-4"}, "reproj_meas_var"), ({"opts": "reproj_meas_var=nan"}, "reproj_meas_var"),
])
def test_bad_arguments_are_refused_by_name_before_any_hip_call(change, named):
    from gbp_poplar_amd import resect
    lib = resect.load()
    args = _cameras_ok()
    if isinstance(change.get("opts"), str):
        field, value = change["opts"].split("=")
        kind = dict(resect.Options._fields_)[field]
        change = {"opts": C.pointer(resect.default_options(**{field: int(value) if kind is C.c_uint32 else float(value)}))}
    args.update(change)
    rc = lib.gbp_resect_cameras(None, *args.values())
    text = lib.gbp_resect_last_error().decode()
    assert rc == -1 and text.startswith("gbp_resect_cameras:") and named in text, (rc, text)


@pytest.mark.parametrize("start,edges,named", [
    ([0, 2, 3, 3], [0, 1, 2, 3], "cam_start[n_cams]"),      # the last entry is not E
    ([1, 2, 3, 4], [0, 1, 2, 3], "cam_start[0]"), ([0, 3, 2, 4], [0, 1, 2, 3], "ascending"), ([0, 2, 3, 4], [0, 1, 2, 4], "cam_edges[3]"),
    ([0, 3, 2, 4], None, "ascending"),
])
def test_a_malformed_index_is_refused_by_name(start, edges, named):
    from gbp_poplar_amd import resect
    lib = resect.load()
    s = np.array(start, np.uint32)
    e = None if edges is None else np.array(edges, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.gbp_resect_check_index(3, 4, s.ctypes.data_as(u32p), None if e is None else e.ctypes.data_as(u32p)) == -1
    assert named in lib.gbp_resect_last_error().decode()
    with pytest.raises(resect.ResectError, match="gbp_resect_check_index"):      # the numpy face of cameras() asks before it stages anything
        resect.cameras(np.zeros(4, np.uint32), s, e, rs.K_SYNTH, np.zeros(18, np.float32), np.zeros(3, np.float32), np.zeros(8, np.float32))


def test_empty_problems_are_legal_without_a_device():
    """no camera: nothing to launch, so GBP_OK with every pointer NULL — on a machine without a GPU too"""
    from gbp_poplar_amd import resect
    lib = resect.load()
    assert lib.gbp_resect_cameras(None, 0, 0, 0, *[None] * 17) == 0
    assert lib.gbp_resect_last_error() == b""
    assert lib.gbp_resect_index(0, 0, None, np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0


def test_a_failure_here_leaves_the_other_libraries_texts_alone_and_the_reverse():
    from gbp_poplar_amd import post, resect, seed
    pl, sl, rl = post.load(), seed.load(), resect.load()
    assert pl.gbp_post_moments(None, 0, 0, *[None] * 10) == 0 and sl.gbp_seed_landmarks(None, 0, 0, 0, None, None, None, (C.c_float * 9)(), *[None] * 11) == 0
    assert rl.gbp_resect_cameras(None, 0, 0, 0, *[None] * 17) == 0
    assert rl.gbp_resect_cameras(None, *dict(_cameras_ok(), lmk_id=None).values()) == -1  # lmk_id is NULL
    text = rl.gbp_resect_last_error()
    assert text.startswith(b"gbp_resect_cameras:") and b"lmk_id" in text
    assert pl.gbp_post_last_error() == b"" and sl.gbp_seed_last_error() == b""
    assert sl.gbp_seed_keyframe(None, 3, 3, 2, P, P, P, P, P) == -1 and pl.gbp_post_moments(None, 2, 3, None, *[P] * 9) == -1
    assert rl.gbp_resect_last_error() == text                                           # their failures are not this library's
    assert rl.gbp_resect_cameras(None, 0, 0, 0, *[None] * 17) == 0 and rl.gbp_resect_last_error() == b""
    assert b"src" in sl.gbp_seed_last_error() and b"cam_eta" in pl.gbp_post_last_error()   # ... and a success here clears only its own


def test_host_twin_takes_its_trig_from_the_one_twin_header():
    """the include pattern of the post and seed mains: device_trig_twin.hpp in front of the arithmetic header, by the two defines"""
    src = re.sub(r"[ \t]*//[^\n]*", "", open(os.path.join(ROOT, "tests", "sanitize", "resect_math_main.cpp")).read())
    assert re.search(r'#include "device_trig_twin\.hpp"\n(?:#include [^\n]*\n)*#define sinf twin_sinf\n#define cosf twin_cosf\n'
                     r'#include "\.\./\.\./gbp_poplar_amd/resect/resect_math\.hpp"\n#undef sinf\n#undef cosf\n', src)
    for name in ("twin_sinf", "twin_cosf", "device_sincos_reduced"):
        assert not re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, src), name


def test_numpy_arrays_without_a_device_raise_a_resect_error(monkeypatch):
    """the numpy face stages through the GPU: where there is none the error is the resection's own"""
    import torch
    from gbp_poplar_amd import resect
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(resect.ResectError, match="the resection runs on the GPU"):
        resect.cameras(np.zeros(1, np.uint32), [0, 1], None, rs.K_SYNTH, np.zeros(6, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32))


def test_the_other_libraries_neither_export_nor_need_a_resect_symbol():
    """a library of its own: the core library, the readout and the seeding neither export nor need a gbp_resect_ symbol; of the
    sources under csrc/ only cli_common.hpp names one"""
    from gbp_poplar_amd import build
    for lib in (build.LIB, build.POST_LIB, build.SEED_LIB):
        out = subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert "gbp_resect_" not in out, lib
    for dirpath, _, files in os.walk(build.CSRC):
        for f in files:
            assert f == "cli_common.hpp" or "gbp_resect_" not in open(os.path.join(dirpath, f), errors="replace").read(), f


def test_run_slam_refuses_an_unknown_kf_init():
    from gbp_poplar_amd import driver
    with pytest.raises(ValueError, match="kf_init"):
        driver.run_slam(None, None, {"n_cams": 2, "n_lmks": 1, "n_edges": 1}, {}, {}, driver.Options(), kf_init="bogus")
