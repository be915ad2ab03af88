"""Landmark and keyframe seeding without a GPU (gbp_poplar_amd/seed/, include/gbp_mi355x_seed.h).

1. The arithmetic — seed/seed_math.hpp, the header the kernels are built from — compiled for the host into a stand-alone program under
   ASan + UBSan (tests/sanitize/seed_math_main.cpp) and compared with the INDEPENDENT numpy implementation of the header's definition in
   tests/seed_support.py.  Per case family the program's error against the numpy float64 run may be 8 x the error of the numpy float32
   run against the same float64 run (computed here, on the family: no recorded number), for the points and for the prior strengths; the
   status word and the view count agree on every landmark.  That the status is a property of the inputs is the generator's business:
   landmarks whose float64 parallax lies within a factor 2 of min_parallax, whose smallest depth is within 10 % of zero (of the point's distance) or (outside the
   non-finite family) whose float64 result is not finite are deselected, and the test asserts that deselected landmarks keep every
   output.  Families: gbp_synth_generate graphs with exact and with the generator's noisy pixels, the three shipped sequences at their
   file cameras, degrees 2, 3, 15, 16, 17 and a hub of 320 views.  The deliberate family (no view, every view inactive, one view, two
   edges of one camera, a point behind a camera, NaN in a camera mean) must give exactly the documented bit and placement.

2. gbp_seed_index against a numpy stable argsort.

3. The C-ABI of libgbp_mi355x_seed.so: `nm -D` equals the header, every export goes through the guard macro, the argument checks
   answer GBP_ERR_INVALID and name the argument before anything touches HIP.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import seed_support as ss
from tests import stateless_cabi
from tests.conftest import seq_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ss.compile_host(str(tmp_path_factory.mktemp("seed_host") / "seed_math"), sanitize=True)


def _synth(noisy):
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.synth_generate(12, 300, 6, 7, ground_truth=True)
    K = driver.k_matrix(bal)
    cams = np.asarray(bal["gt_cameras"], np.float64).astype(np.float32)
    z = None if noisy else ss.project64(cams, bal["gt_points"], bal["cam_id"].astype(np.int64), bal["lmk_id"].astype(np.int64), K)
    return ss.bal_graph(bal, K, cam_mean=cams, measurements=z), np.asarray(bal["gt_points"], np.float64).reshape(-1, 3)


def _sequence(name):
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path(name))
    return ss.bal_graph(bal, driver.k_matrix(bal)), None


def _degrees():
    return ss.degree_graph([2, 3, 15, 16, 17] * 6 + [320], seed=11, noise=0.5)


FAMILIES = {"synth_exact": lambda: _synth(False), "synth_noisy": lambda: _synth(True), "fr1xyz": lambda: _sequence("fr1xyz"),
            "fr1desk": lambda: _sequence("fr1desk"), "fr2robot2": lambda: _sequence("fr2robot2"), "degrees": _degrees}
_cache = {}


def _family(name, host_exe, tmp):
    """(graph, ground-truth points or None, select, numpy float64 run, numpy float32 run, outputs before, host program's outputs)"""
    if name not in _cache:
        g, gt = FAMILIES[name]()
        r64, r32 = ss.seed_numpy(g, np.float64, details=True), ss.seed_numpy(g, np.float32)
        select = (~ss.ambiguous(r64)).astype(np.uint32)
        before = ss.initial_outputs(g["n_lmks"])
        _cache[name] = (g, gt, select, r64, r32, before, ss.run_host(host_exe, tmp, g, select=select, before=before))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_host_program_against_the_numpy_definition(name, host_exe, tmp_path):
    g, _, select, r64, r32, before, out = _family(name, host_exe, tmp_path)
    sel = select == 1
    assert sel.mean() >= 0.5, "the generator rejected most of the family"
    # deselected landmarks: nothing is touched
    for k, w, _ in ss.OUTPUTS:
        assert np.array_equal(out[k].reshape(-1, w)[~sel], before[k].reshape(-1, w)[~sel]), k
    # the status word and the view count: every selected landmark, nothing excluded
    assert np.array_equal(out["status"][sel], r64["status"][sel]) and np.array_equal(out["n_views"][sel], r64["n_views"][sel])
    assert np.array_equal(r32["status"][sel], r64["status"][sel]), "the float32 run of the definition takes another branch"
    seen = sel & (r64["n_views"] > 0)
    if name == "degrees":
        assert (r64["status"][seen] == 0).all() and r64["n_views"].max() == 320
    lam = out["lmk_priors_lambda"].reshape(-1, 9)
    assert not lam[seen][:, [1, 2, 3, 5, 6, 7]].any() and (lam[seen, 0] == lam[seen, 4]).all() and (lam[seen, 0] == lam[seen, 8]).all()
    assert np.array_equal(out["lmk_priors_eta"].reshape(-1, 3)[seen], out["lmk_mean"].reshape(-1, 3)[seen] * lam[seen, :1])
    e_x, b_x = ss.point_error(out["lmk_mean"].reshape(-1, 3)[seen], r64["lmk_mean"][seen]), ss.point_error(r32["lmk_mean"][seen], r64["lmk_mean"][seen])
    e_l, b_l = ss.lam_error(lam[seen, 0], r64["lam"][seen]), ss.lam_error(r32["lam"][seen], r64["lam"][seen])
    print("%s: %d of %d landmarks selected; point error %.3e (numpy float32 %.3e, bound %.3e); lam error %.3e (numpy float32 %.3e, bound %.3e)"
          % (name, sel.sum(), sel.size, e_x, b_x, FACTOR * b_x, e_l, b_l, FACTOR * b_l))
    assert e_x <= FACTOR * b_x and e_l <= FACTOR * b_l


def test_exact_pixels_and_true_cameras_give_the_true_points(host_exe, tmp_path):
    _, gt, select, r64, r32, _, out = _family("synth_exact", host_exe, tmp_path)
    seen = (select == 1) & (r64["status"] == 0)
    assert seen.sum() >= 0.5 * seen.size
    e, b = ss.point_error(out["lmk_mean"].reshape(-1, 3)[seen], gt[seen]), ss.point_error(r32["lmk_mean"][seen], r64["lmk_mean"][seen])
    print("against gt_points: %.3e (bound %.3e) over %d landmarks" % (e, FACTOR * b, seen.sum()))
    assert e <= FACTOR * b


def _deliberate():
    """cameras 0-3 ordinary, 4 turned by pi about y at the origin (what lies in front of the others lies behind it), 5 with a NaN"""
    rng = np.random.default_rng(5)
    cams = np.concatenate([rng.uniform(-1, 1, (6, 3)), rng.uniform(-0.1, 0.1, (6, 3))], axis=1).astype(np.float32)
    cams[4] = [0.0, 0.0, 0.0, 0.0, np.pi, 0.0]
    pts = np.concatenate([rng.uniform(-1, 1, (7, 2)), rng.uniform(4, 8, (7, 1))], axis=1)
    #        no view | inactive | one view | same camera twice | behind camera 4 | NaN camera 5 | ordinary
    edges = [(1, 1), (2, 1), (0, 2), (3, 3), (3, 3), (0, 4), (1, 4), (4, 4), (0, 5), (5, 5), (2, 5), (0, 6), (1, 6), (3, 6)]
    cam_id, lmk_id = np.array([e[0] for e in edges]), np.array([e[1] for e in edges])
    z = ss.project64(cams, pts, cam_id, lmk_id, ss.K_SYNTH)
    cams[5, 1] = np.nan
    active = np.ones(len(edges), np.uint32)
    active[:2] = 0
    return ss.graph_of(6, 7, cam_id, lmk_id, ss.K_SYNTH, cams, z, active), pts


def test_deliberate_cases_give_the_documented_bit_and_placement(host_exe, tmp_path):
    g, pts = _deliberate()
    before = ss.initial_outputs(7)
    out = ss.run_host(host_exe, tmp_path, g, before=before)
    r64 = ss.seed_numpy(g, np.float64)
    assert out["status"].tolist() == r64["status"].tolist() == [ss.NO_VIEW, ss.NO_VIEW, ss.ONE_VIEW, ss.LOW_PARALLAX, ss.BEHIND, ss.NONFINITE, 0]
    assert out["n_views"].tolist() == [0, 0, 1, 2, 3, 3, 3]
    mean = out["lmk_mean"].reshape(-1, 3)
    for k in ("lmk_mean", "lmk_priors_eta", "lmk_priors_lambda"):      # no view: the mean and the prior keep what they held
        w = out[k].size // 7
        assert np.array_equal(out[k][:2 * w], before[k][:2 * w]), k
    assert np.isfinite(mean[2:]).all() and np.isfinite(out["lmk_priors_lambda"][18:]).all() and (out["lmk_priors_lambda"].reshape(-1, 9)[2:, 0] > 0).all()
    # the placements: depth fallback_depth (1) in the FIRST used view's camera, on the ray of its pixel
    # Every bound below is 8 x what the float32 run of the numpy definition misses by, on the same quantity of this same case.
    r32 = ss.seed_numpy(g, np.float32)
    assert r32["status"].tolist() == r64["status"].tolist()
    cams = g["cam_mean"].reshape(-1, 6).astype(np.float64)

    def placement_errors(points):
        """largest |camera-frame depth - 1| and largest pixel distance from the observation, over the three placed landmarks"""
        depth, pixel = 0.0, 0.0
        for l, e in ((2, 2), (3, 3), (5, 8)):
            c = g["cam_id"][e]
            p = ss._rotation(cams[c, 3:], np.float64) @ points[l].astype(np.float64) + cams[c, :3]
            pix = ss.project64(cams[c], points[l], np.array([0]), np.array([0]), ss.K_SYNTH)[0]
            depth, pixel = max(depth, abs(p[2] - 1.0)), max(pixel, float(np.abs(pix - g["measurements"].reshape(-1, 2)[e]).max()))
        return depth, pixel

    (e_d, e_p), (b_d, b_p) = placement_errors(mean), placement_errors(r32["lmk_mean"])
    # behind a camera: the lines still meet at the point, which is kept and flagged; the ordinary landmark is its point
    e_gt, b_gt = ss.point_error(mean[[4, 6]], pts[[4, 6]]), ss.point_error(r32["lmk_mean"][[4, 6]], pts[[4, 6]])
    e_x, b_x = ss.point_error(mean[2:], r64["lmk_mean"][2:]), ss.point_error(r32["lmk_mean"][2:], r64["lmk_mean"][2:])
    print("placement: depth error %.3e (numpy float32 %.3e), pixel error %.3e (%.3e); true points %.3e (%.3e); float64 run %.3e (%.3e)"
          % (e_d, b_d, e_p, b_p, e_gt, b_gt, e_x, b_x))
    assert e_d <= FACTOR * b_d and e_p <= FACTOR * b_p and e_gt <= FACTOR * b_gt and e_x <= FACTOR * b_x


def test_bad_index_entries_are_skipped_and_flagged(host_exe, tmp_path):
    g, _ = ss.degree_graph([3, 3, 3], seed=3)
    few = {"min_parallax": 1e-4}                  # (two of these views are enough)
    good = ss.run_host(host_exe, tmp_path, g, opts=few)
    g["lmk_edges"] = g["lmk_edges"].copy()
    g["lmk_edges"][4] = 1000                      # landmark 1: an edge that does not exist
    g["lmk_start"] = g["lmk_start"].copy()
    g["lmk_start"][3] = 12                        # landmark 2: a range past the end
    out = ss.run_host(host_exe, tmp_path, g, opts=few)
    assert out["status"].tolist() == [0, ss.BAD_INDEX, ss.BAD_INDEX] and out["n_views"].tolist() == [3, 2, 3]
    assert np.array_equal(out["lmk_mean"][:3], good["lmk_mean"][:3]) and np.array_equal(out["lmk_mean"][6:], good["lmk_mean"][6:])


def test_prior_strength_at_the_file_points_is_gbp_set_prior_lambdas(host_exe, tmp_path):
    """The prior is gbp_set_prior_lambda's rule at the seeded point, bit for bit: seed every landmark of a graph cut down to each
    landmark's first observation (so the used observations are all its observations), then ask gbp_set_prior_lambda for the landmark
    priors AT the seeded points."""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    K = driver.k_matrix(bal)
    first = np.unique(bal["lmk_id"], return_index=True)[1]
    cams = np.asarray(bal["cameras"], np.float64).astype(np.float32)
    z = np.asarray(bal["observations"], np.float64).astype(np.float32).reshape(-1, 2)[first]
    g = ss.graph_of(bal["n_cams"], bal["n_lmks"], bal["cam_id"][first], bal["lmk_id"][first], K, cams, z)
    out = ss.run_host(host_exe, tmp_path, g)
    assert (out["status"] == ss.ONE_VIEW).all()
    _, _, lpe, lpl = hostlib.set_prior_lambda(g["cam_id"], g["lmk_id"], bal["n_cams"], bal["n_lmks"], K, 4.0, cams, out["lmk_mean"], cams, out["lmk_mean"])
    assert np.array_equal(out["lmk_priors_lambda"], lpl) and np.array_equal(out["lmk_priors_eta"], lpe)


# ---- gbp_seed_index ----
@pytest.mark.parametrize("case", ["random", "duplicates", "unobserved", "empty"])
def test_index_is_the_stable_argsort(case):
    from gbp_poplar_amd import seed
    rng = np.random.default_rng(17)
    n_lmks = 40
    if case == "random":
        lmk_id = rng.integers(0, n_lmks, 500)
    elif case == "duplicates":
        lmk_id = np.repeat(rng.integers(0, n_lmks, 100), 3)[rng.permutation(300)]
    elif case == "unobserved":
        lmk_id = rng.choice(np.arange(0, n_lmks, 3), 200)
    else:
        lmk_id = np.zeros(0, np.int64)
    start, edges = seed.index(lmk_id, n_lmks)
    want_start, want_edges = ss.index_numpy(lmk_id, n_lmks)
    assert start.dtype == edges.dtype == np.uint32 and np.array_equal(start, want_start) and np.array_equal(edges, want_edges)
    seed.check_index(start, edges)
    if case == "unobserved":
        assert (np.diff(start.astype(np.int64))[1::3] == 0).all()


def test_index_refuses_an_id_out_of_range():
    from gbp_poplar_amd import seed
    with pytest.raises(seed.SeedError, match=r"lmk_id\[2\]"):
        seed.index([0, 1, 5, 2], 5)


# ---- the C-ABI ----
EXPORTS = ["gbp_seed_abi_version", "gbp_seed_check_index", "gbp_seed_default_options", "gbp_seed_index", "gbp_seed_keyframe", "gbp_seed_landmarks",
           "gbp_seed_last_error", "gbp_seed_workspace_bytes"]


def test_library_exports_the_header_and_nothing_else():
    from gbp_poplar_amd import seed
    stateless_cabi.check_exports(seed, "gbp_mi355x_seed.h", EXPORTS, 1)
    assert seed.workspace_bytes(1000) == 64000


def test_every_export_is_defined_through_the_guard_macro():
    stateless_cabi.check_guard("seed", "gbp_mi355x_seed.h", EXPORTS)


def test_default_options_are_the_headers():
    from gbp_poplar_amd import seed
    o = seed.default_options()
    assert (o.min_parallax, o.fallback_depth, o.refine_iters, o.reproj_meas_var) == (np.float32(5e-3), 1.0, 2, 4.0)
    assert seed.load().gbp_seed_default_options(None) == -1 and b"opts" in seed.load().gbp_seed_last_error()


P = C.c_void_p(64)      # any non-NULL address: a call that fails its argument checks touches neither the array nor HIP


def _landmarks_ok():
    from gbp_poplar_amd import seed
    return dict(n_cams=2, n_lmks=3, n_edges=4, cam_id=P, lmk_start=P, lmk_edges=P, K=(C.c_float * 9)(), cam_mean=P, measurements=P, active_flag=P,
                select=P, opts=C.pointer(seed.default_options()), workspace=P, lmk_mean=P, lmk_priors_eta=P, lmk_priors_lambda=P, status=P, n_views=P)


KEYFRAME_OK = dict(n_cams=3, src=1, dst=2, cam_beliefs_eta=P, cam_beliefs_lambda=P, cam_priors_lambda=P, cam_priors_eta=P, cam_mean_out=P)


@pytest.mark.parametrize("fn,change,named", [
    ("landmarks", {"cam_id": None}, "cam_id"), ("landmarks", {"lmk_start": None}, "lmk_start"), ("landmarks", {"lmk_edges": None}, "lmk_edges"),
    ("landmarks", {"K": None}, "K"), ("landmarks", {"cam_mean": None}, "cam_mean"), ("landmarks", {"measurements": None}, "measurements"),
    ("landmarks", {"workspace": None}, "workspace"), ("landmarks", {"workspace": C.c_void_p(68)}, "workspace"),
    ("landmarks", {"lmk_mean": None}, "lmk_mean"), ("landmarks", {"status": None}, "status"), ("landmarks", {"n_cams": 0}, "n_cams"),
    ("landmarks", {"opts": "reproj_meas_var=0"}, "reproj_meas_var"), ("landmarks", {"opts": "reproj_meas_var=-4"}, "reproj_meas_var"),
    ("landmarks", {"opts": "reproj_meas_var=nan"}, "reproj_meas_var"), ("landmarks", {"opts": "fallback_depth=0"}, "fallback_depth"),
    ("landmarks", {"opts": "min_parallax=nan"}, "min_parallax"),
    ("keyframe", {"src": 3}, "src"), ("keyframe", {"dst": 3}, "dst"), ("keyframe", {"n_cams": 0}, "src"),
    ("keyframe", {"cam_beliefs_eta": None}, "cam_beliefs_eta"), ("keyframe", {"cam_beliefs_lambda": None}, "cam_beliefs_lambda"),
    ("keyframe", {"cam_priors_lambda": None}, "cam_priors_lambda"), ("keyframe", {"cam_priors_eta": None}, "cam_priors_eta"),
])
def test_bad_arguments_are_refused_by_name_before_any_hip_call(fn, change, named):
    from gbp_poplar_amd import seed
    lib = seed.load()
    args = dict(_landmarks_ok() if fn == "landmarks" else KEYFRAME_OK)
    if isinstance(change.get("opts"), str):
        field, value = change["opts"].split("=")
        change = {"opts": C.pointer(seed.default_options(**{field: float(value)}))}
    args.update(change)
    rc = getattr(lib, "gbp_seed_" + fn)(None, *args.values())
    text = lib.gbp_seed_last_error().decode()
    assert rc == -1 and text.startswith("gbp_seed_" + fn + ":") and named in text, (rc, text)


@pytest.mark.parametrize("start,edges,named", [
    ([0, 2, 3, 3], [0, 1, 2, 3], "lmk_start[n_lmks]"),      # the last entry is not E
    ([1, 2, 3, 4], [0, 1, 2, 3], "lmk_start[0]"), ([0, 3, 2, 4], [0, 1, 2, 3], "ascending"), ([0, 2, 3, 4], [0, 1, 2, 4], "lmk_edges[3]"),
])
def test_a_malformed_index_is_refused_by_name(start, edges, named):
    from gbp_poplar_amd import seed
    lib = seed.load()
    s, e = np.array(start, np.uint32), np.array(edges, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.gbp_seed_check_index(3, 4, s.ctypes.data_as(u32p), e.ctypes.data_as(u32p)) == -1
    assert named in lib.gbp_seed_last_error().decode()
    with pytest.raises(seed.SeedError, match="gbp_seed_check_index"):      # the numpy face of landmarks() asks before it stages anything
        seed.landmarks(np.zeros(4, np.uint32), s, e, ss.K_SYNTH, np.zeros(12, np.float32), np.zeros(8, np.float32))


def test_empty_problems_are_legal_without_a_device():
    """no landmark: nothing to launch, so GBP_OK with every pointer NULL — on a machine without a GPU too"""
    from gbp_poplar_amd import seed
    lib = seed.load()
    assert lib.gbp_seed_landmarks(None, 0, 0, 0, None, None, None, (C.c_float * 9)(), *[None] * 11) == 0
    assert lib.gbp_seed_last_error() == b""
    assert lib.gbp_seed_index(0, 0, None, np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0


def test_both_host_twins_take_their_trig_from_the_one_twin_header():
    """tests/sanitize/device_trig_twin.hpp holds the only copy of the device's sinf / cosf: both mains include it, put it in front of
    their arithmetic header by the two defines, and define none of it themselves"""
    for main, math in (("post_math_main.cpp", "post/post_math.hpp"), ("seed_math_main.cpp", "seed/seed_math.hpp")):
        src = re.sub(r"[ \t]*//[^\n]*", "", open(os.path.join(ROOT, "tests", "sanitize", main)).read())
        assert re.search(r'#include "device_trig_twin\.hpp"\n(?:#include [^\n]*\n)*#define sinf twin_sinf\n#define cosf twin_cosf\n'
                         r'#include "\.\./\.\./gbp_poplar_amd/%s"\n#undef sinf\n#undef cosf\n' % re.escape(math), src), main
        for name in ("twin_sinf", "twin_cosf", "device_sincos_reduced"):
            assert not re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, src), (main, name)
    twin = open(os.path.join(ROOT, "tests", "sanitize", "device_trig_twin.hpp")).read()
    assert all(re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, twin) for name in ("twin_sinf", "twin_cosf", "device_sincos_reduced"))


def test_numpy_arrays_without_a_device_raise_a_seed_error(monkeypatch):
    """the numpy face stages through the GPU: where there is none the error is the seeding's own, not the readout's"""
    import torch
    from gbp_poplar_amd import seed
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(seed.SeedError, match="the seeding runs on the GPU"):
        seed.landmarks(np.zeros(1, np.uint32), [0, 1], [0], ss.K_SYNTH, np.zeros(6, np.float32), np.zeros(2, np.float32))
    with pytest.raises(seed.SeedError, match="the seeding runs on the GPU"):
        seed.keyframe(0, 1, np.zeros(12, np.float32), np.zeros(72, np.float32), np.zeros(72, np.float32), np.zeros(12, np.float32))


def test_product_libraries_are_not_linked_against_the_seed_library():
    """a library of its own: the core library and the readout neither export nor need a gbp_seed_ symbol"""
    from gbp_poplar_amd import build
    for lib in (build.LIB, build.POST_LIB):
        out = subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert "gbp_seed_" not in out, lib
