"""The solution readout without a GPU (gbp_poplar_amd/post/, include/gbp_mi355x_post.h).

1. The arithmetic — post/post_math.hpp, the header the kernels are built from — compiled for the host into a stand-alone program under
   ASan + UBSan (tests/sanitize/post_math_main.cpp) and run on the CPU oracle's beliefs of fr1xyz and fr2robot2 after 200 passes of the
   default loop (weakenings included) and on four hand-made blocks per width (a zero leading diagonal, an indefinite block, the zero
   block, an SPD block of condition 1e6).  Bit for bit (NaNs equal NaNs): the means are hostlib.belief_means, column j of a covariance
   is hostlib.belief_means of the same Lambda with eta = e_j — the host solve_pivot, which the parity suite ties to the device's —, the
   status words are numpy restatements of their two definitions.

   What the numbers MEAN is checked against float64, independently of any solve_pivot:
     covariance   max |cov - inv64(Lambda)| / max |inv64(Lambda)| <= 2^-21 per block of condition <= 1e6 (at most 1 % of the oracle's
                  blocks may be excluded by that limit).  Measured on these inputs: 2.07 x 2^-24 (a landmark of fr2robot2, condition
                  3.3e3; cameras: 1.99 x 2^-24 at condition 3.2e5); the largest condition present is 4.7e5, nothing is excluded.
                  2^-21 is about 4 x the measured worst; an error of meaning (a transposed block, another variable) shows at O(1).
     residual     max |r - r64| over the active edges, r64 = z - ref64.project at the SAME float32 means.  Measured: 1.82e-4 px
                  (fr2robot2; fr1xyz 1.15e-4 px) on projections of a few hundred pixels.  Bound: 4 x = 7.3e-4 px.
     reproj_cov   max over edges of max |S - S64| / max |S64|, S64 from ref64's complex-step Jacobian at the same float32 means
                  and covariances.  Measured: 4.77e-4 (fr1xyz; fr2robot2 3.99e-4).  Bound: 4 x = 1.9e-3.
   (4 x the measured error: the margin tests/test_exact_inference.py module D uses for the same projection.)  In float64, the
   rotation's transpose and the landmark index shifted by one land 0.9998 .. 1.6e6 away in these measures, at least 100 x the bound.

2. The C-ABI of libgbp_mi355x_post.so: `nm -D` equals the header, every export goes through the guard macro, the argument checks
   answer GBP_ERR_INVALID and name the argument before anything touches HIP.
"""
import ctypes as C

import numpy as np
import pytest

from tests import post_support as ps
from tests import stateless_cabi

COV_BOUND = 2.0 ** -21
COND_LIMIT = 1e6
MAX_EXCLUDED = 0.01
RESIDUAL_MEASURED, REPROJ_COV_MEASURED = 1.82e-4, 4.77e-4      # the host build against float64, on these inputs (module docstring)
RESIDUAL_BOUND, REPROJ_COV_BOUND = 4.0 * RESIDUAL_MEASURED, 4.0 * REPROJ_COV_MEASURED
SEQUENCES = ("fr1xyz", "fr2robot2")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ps.compile_host(str(tmp_path_factory.mktemp("post_host") / "post_math"), sanitize=True)


@pytest.fixture(scope="module")
def runs(host_exe, oracle_mod, tmp_path_factory):
    """name -> (bal, K, state, beliefs, outputs of the host program); "hand_made": the eight hand-made blocks, no edges"""
    tmp = tmp_path_factory.mktemp("post_runs")
    out = {}
    for name in SEQUENCES:
        bal, K, state, b = ps.oracle_sequence(oracle_mod, name)
        out[name] = (bal, K, state, b, ps.run_host(host_exe, tmp, b, bal["cam_id"], bal["lmk_id"], K, state["measurements"], state["active_flag"]))
    b = ps.hand_made_beliefs()
    out["hand_made"] = (None, None, None, b, ps.run_host(host_exe, tmp, b))
    return out


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("name", SEQUENCES + ("hand_made",))
def test_means_and_covariance_columns_are_the_host_pivot_solve(name, runs):
    from gbp_poplar_amd import hostlib
    b, out = runs[name][3], runs[name][4]
    n_c, n_l = b["cam_beliefs_eta"].size // 6, b["lmk_beliefs_eta"].size // 3
    with np.errstate(all="ignore"):
        cams, pts = hostlib.belief_means(n_c, n_l, *[b[k] for k in ps.BELIEFS])
        assert _same(out["cam_mean"], cams) and _same(out["lmk_mean"], pts)
        for j in range(6):
            e6, e3 = np.zeros((n_c, 6), np.float32), np.zeros((n_l, 3), np.float32)
            e6[:, j] = 1.0
            e3[:, j % 3] = 1.0
            cams, pts = hostlib.belief_means(n_c, n_l, e6.ravel(), b["cam_beliefs_lambda"], e3.ravel(), b["lmk_beliefs_lambda"])
            assert _same(out["cam_cov"].reshape(-1, 6, 6)[:, :, j], cams.reshape(-1, 6)), j
            assert _same(out["lmk_cov"].reshape(-1, 3, 3)[:, :, j % 3], pts.reshape(-1, 3)), j


@pytest.mark.parametrize("name", SEQUENCES + ("hand_made",))
def test_status_words_are_their_two_definitions(name, runs):
    b, out = runs[name][3], runs[name][4]
    for pre, w in (("cam", 6), ("lmk", 3)):
        want = ps.status_restated(b[pre + "_beliefs_lambda"], out[pre + "_mean"], out[pre + "_cov"], w)
        assert np.array_equal(out[pre + "_status"], want), pre
    if name == "hand_made":      # zero diagonal: swapped, finite, not PD; indefinite: finite, not PD; zero block: nothing finite; SPD 1e6: fine
        assert out["cam_status"].tolist() == [2, 2, 3, 0] and out["lmk_status"].tolist() == [2, 2, 3, 0]
        assert np.isfinite(out["cam_cov"].reshape(4, 36)[[0, 1, 3]]).all() and not np.isfinite(out["cam_cov"].reshape(4, 36)[2]).any()
    else:
        assert not out["cam_status"].any() and not out["lmk_status"].any()


def _inverse_errors(lam, cov, w):
    """(error per block, float64 2-norm condition per block); singular blocks: condition inf"""
    lam = np.asarray(lam, np.float32).reshape(-1, w, w).astype(np.float64)
    cov = np.asarray(cov, np.float64).reshape(-1, w, w)
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(lam)
    err = np.full(lam.shape[0], np.nan)
    ok = np.isfinite(cond) & (cond <= COND_LIMIT)
    inv = np.linalg.inv(lam[ok])
    err[ok] = np.max(np.abs(cov[ok] - inv), axis=(1, 2)) / np.max(np.abs(inv), axis=(1, 2))
    return err, cond, ok


def test_covariances_are_the_float64_inverse(runs):
    worst, n_oracle, n_excluded = 0.0, 0, 0
    for name in SEQUENCES + ("hand_made",):
        b, out = runs[name][3], runs[name][4]
        for pre, w in (("cam", 6), ("lmk", 3)):
            err, cond, ok = _inverse_errors(b[pre + "_beliefs_lambda"], out[pre + "_cov"], w)
            if name != "hand_made":
                n_oracle += ok.size
                n_excluded += int((~ok).sum())
            else:
                assert ok.tolist() == [True, True, False, cond[3] <= COND_LIMIT] and 5e5 < cond[3] < 2e6
            i = int(np.nanargmax(err))
            print("%s %s: worst %.3f x 2^-24 at condition %.3g; largest condition %.3g" % (name, pre, err[i] * 2.0 ** 24, cond[i], np.max(cond[np.isfinite(cond)])))
            worst = max(worst, float(np.nanmax(err)))
            assert np.nanmax(err) <= COV_BOUND, (name, pre, err[i], cond[i])
    print("worst %.3f x 2^-24, %d of %d oracle blocks excluded" % (worst * 2.0 ** 24, n_excluded, n_oracle))
    assert n_excluded <= MAX_EXCLUDED * n_oracle


@pytest.mark.parametrize("name", SEQUENCES)
def test_residuals_and_reprojection_covariances_against_float64(name, runs):
    bal, K, state, _, out = runs[name]
    act = np.asarray(state["active_flag"]) == 1
    z = state["measurements"]
    res, cov = out["residual"].reshape(-1, 2), out["reproj_cov"].reshape(-1, 3)
    assert not res[~act].any() and not cov[~act].any()
    r64, s64 = ps.edges64(bal, K, z, out)
    e_r, e_s = ps.residual_error(res[act], r64[act]), ps.reproj_cov_error(cov[act], s64[act])
    print("%s: residual error %.3e px (bound %.3e), reprojection covariance error %.3e (bound %.3e)" % (name, e_r, RESIDUAL_BOUND, e_s, REPROJ_COV_BOUND))
    assert e_r <= RESIDUAL_BOUND and e_s <= REPROJ_COV_BOUND
    # the bounds are not blind: in float64, the rotation's transpose and landmark l + 1 in place of l are at least 100 bounds away
    for wrong in ({"rotation_transposed": True}, {"lmk_shift": 1}):
        rw, sw = ps.edges64(bal, K, z, out, **wrong)
        assert ps.residual_error(r64[act], rw[act]) >= 100.0 * RESIDUAL_BOUND, wrong
        assert ps.reproj_cov_error(s64[act], sw[act]) >= 100.0 * REPROJ_COV_BOUND, wrong


@pytest.mark.parametrize("name", SEQUENCES)
def test_residuals_reproduce_the_metrics_per_factor_terms(name, runs):
    """sqrt(r0^2 + r1^2) and 0.5 (r0^2 + r1^2) of the residuals, in the metric's precisions, add up to gbp_eval_host's sums exactly"""
    from gbp_poplar_amd import hostlib
    bal, K, state, b, out = runs[name]
    sn, sh, na = hostlib.eval_host(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, state["active_flag"], state["measurements"],
                                   *[b[k] for k in ps.BELIEFS])
    r = out["residual"].reshape(-1, 2)[np.asarray(state["active_flag"]) == 1]
    sq = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]      # float32, as eval_residual forms it
    norm, half = np.sqrt(sq).astype(np.float64), (0.5 * sq.astype(np.float64)).astype(np.float32).astype(np.float64)
    a_n = a_h = 0.0
    for i in range(r.shape[0]):      # gbp_eval_host adds serially, in file order
        a_n, a_h = a_n + norm[i], a_h + half[i]
    assert na == r.shape[0] and a_n == sn and a_h == sh


# ---- the C-ABI ----
EXPORTS = ["gbp_post_abi_version", "gbp_post_last_error", "gbp_post_moments", "gbp_post_residuals"]


def test_library_exports_the_header_and_nothing_else():
    from gbp_poplar_amd import post
    stateless_cabi.check_exports(post, "gbp_mi355x_post.h", EXPORTS, 1)


def test_every_export_is_defined_through_the_guard_macro():
    stateless_cabi.check_guard("post", "gbp_mi355x_post.h", EXPORTS)


P = C.c_void_p(64)      # any non-NULL address: a call that fails its argument checks touches neither the array nor HIP
MOMENTS_OK = dict(n_cams=2, n_lmks=3, cam_eta=P, cam_lambda=P, lmk_eta=P, lmk_lambda=P, cam_mean=P, cam_cov=P, lmk_mean=P, lmk_cov=P,
                  cam_status=P, lmk_status=P)
RESIDUALS_OK = dict(n_cams=2, n_lmks=3, n_edges=4, cam_id=P, lmk_id=P, K=(C.c_float * 9)(), cam_mean=P, lmk_mean=P, measurements=P, active_flag=P,
                    cam_cov=P, lmk_cov=P, residual=P, reproj_cov=P)


@pytest.mark.parametrize("fn,change,named", [
    ("moments", {"cam_eta": None}, "cam_eta"), ("moments", {"cam_lambda": None}, "cam_lambda"),
    ("moments", {"lmk_eta": None}, "lmk_eta"), ("moments", {"lmk_lambda": None}, "lmk_lambda"),
    ("residuals", {"cam_id": None}, "cam_id"), ("residuals", {"lmk_id": None}, "lmk_id"), ("residuals", {"K": None}, "K"),
    ("residuals", {"cam_mean": None}, "cam_mean"), ("residuals", {"lmk_mean": None}, "lmk_mean"),
    ("residuals", {"measurements": None}, "measurements"), ("residuals", {"residual": None}, "residual"),
    ("residuals", {"cam_cov": None}, "cam_cov"), ("residuals", {"lmk_cov": None}, "lmk_cov"),
    ("residuals", {"cam_cov": None, "lmk_cov": None}, "reproj_cov"), ("residuals", {"n_cams": 0}, "n_cams"), ("residuals", {"n_lmks": 0}, "n_lmks"),
])
def test_bad_arguments_are_refused_by_name_before_any_hip_call(fn, change, named):
    from gbp_poplar_amd import post
    lib = post.load()
    args = dict(MOMENTS_OK if fn == "moments" else RESIDUALS_OK)
    args.update(change)
    rc = getattr(lib, "gbp_post_" + fn)(None, *args.values())
    text = lib.gbp_post_last_error().decode()
    assert rc == -1 and text.startswith("gbp_post_" + fn + ":") and named in text, (rc, text)


def test_empty_problems_are_legal_without_a_device():
    """no variable / no edge: nothing to launch, so GBP_OK with every pointer NULL — on a machine without a GPU too"""
    from gbp_poplar_amd import post
    lib = post.load()
    assert lib.gbp_post_moments(None, 0, 0, *[None] * 10) == 0
    assert lib.gbp_post_residuals(None, 0, 0, 0, None, None, (C.c_float * 9)(), *[None] * 8) == 0
    assert lib.gbp_post_last_error() == b""


def test_on_a_tree_the_oracles_covariances_are_the_exact_marginals(host_exe, oracle_mod, tmp_path):
    """What tests/test_gpu_post.py asks of the engine, asked of the CPU oracle first: the hub tree of tests/test_exact_inference.py,
    dmu_threshold = 0, diameter + 2 sweeps, the covariances of its beliefs (host program) against ref64.marginals within
    6 kappa_v A_BOUND[*_lambda] + 2^-21 per variable of kappa_v <= 1e3.  Measured: the worst variable uses 0.9 % of its bound (cameras,
    1.5e-6; landmarks 3.4e-7, 0.7 %), kappa <= 62, nothing is left unchecked; the covariance of variable v + 1 in place of v's is at
    least 500 bounds away."""
    from tests import test_exact_inference as tei
    bal, _ = tei.hub_tree()
    g = tei._Exact("A hub tree", bal, tei.diameter(bal) + tei.A_SWEEPS_OVER_DIAMETER, maxeta_damping=0.0)
    orc = tei._oracle_variant(oracle_mod, g, "restatement", 1)
    orc.upload(g.state)
    orc.linearise()
    ex = g.exact(*orc.factor_potentials())
    orc.iterate(g.sweeps)
    fig = ps.tree_covariance_check(ex, ps.run_host(host_exe, tmp_path, orc.read()), tei.A_BOUND, "oracle")
    assert fig["cam"]["unchecked"] == 0 and fig["lmk"]["unchecked"] == 0
