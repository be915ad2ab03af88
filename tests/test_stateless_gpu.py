"""The one call path of the ctx-less libraries' bindings (gbp_poplar_amd/_stateless.py: Binding.call) on the GPU, at C = 2, L = 3,
E = 4: seed.landmarks, resect.cameras, locate.cameras and post.residuals each refuse, with a TypeError that names the array and BEFORE
the library's function is called (it is replaced by one that fails the test, so no kernel is launched), a host array beside device
tensors, a wrong dtype, a tensor that is not contiguous, a wrong element count, an unknown `out` name and the Options of another
library; the correct call with every optional input None succeeds.  What the kernels compute is tests/test_gpu_{post,seed,resect,locate}.py's business."""
import numpy as np
import pytest

from tests.seed_support import K_SYNTH

pytestmark = pytest.mark.gpu

C_, L_, E_ = 2, 3, 4


def _arrays():
    """a file sorted by camera (cam_edges None is its index): camera 0 sees landmarks 0, 1, camera 1 sees 1, 2"""
    import torch
    from gbp_poplar_amd import seed
    cam_id, lmk_id = np.array([0, 0, 1, 1], np.uint32), np.array([0, 1, 1, 2], np.uint32)
    lmk_start, lmk_edges = seed.index(lmk_id, L_)
    host = {"cam_id": cam_id, "lmk_id": lmk_id, "lmk_start": lmk_start, "lmk_edges": lmk_edges, "cam_start": np.array([0, 2, 4], np.uint32),
            "cam_mean": np.array([0, 0, 0, 0.01, 0.02, 0.03, 0.1, 0, 0, 0.03, 0.01, 0.02], np.float32),
            "lmk_mean": np.array([-0.5, 0.2, 5, 0.1, -0.3, 6, 0.6, 0.4, 7], np.float32),
            "measurements": np.array([300, 250, 330, 220, 310, 215, 350, 270], np.float32)}
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to("cuda") for k, v in host.items()}


def _libraries():
    from gbp_poplar_amd import locate, post, resect, seed
    return {
        "seed": (seed, "gbp_seed_landmarks", lambda a, **kw: seed.landmarks(
            a["cam_id"], a["lmk_start"], a["lmk_edges"], K_SYNTH, a["cam_mean"], a["measurements"], **kw),
            ("lmk_mean", "lmk_priors_eta", "lmk_priors_lambda", "status", "n_views"), resect.Options),
        "resect": (resect, "gbp_resect_cameras", lambda a, **kw: resect.cameras(
            a["lmk_id"], a["cam_start"], None, K_SYNTH, a["cam_mean"], a["lmk_mean"], a["measurements"], **kw),
            ("cam_mean", "cam_info", "report", "status", "n_views"), locate.Options),
        "locate": (locate, "gbp_locate_cameras", lambda a, **kw: locate.cameras(
            a["lmk_id"], a["cam_start"], None, K_SYNTH, a["lmk_mean"], a["measurements"], **kw),
            ("cam_mean", "inlier", "report", "status", "n_views", "n_inliers"), seed.Options),
        "post": (post, "gbp_post_residuals", lambda a, **kw: post.residuals(a["cam_id"], a["lmk_id"], K_SYNTH, a, a["measurements"], **kw),
                 ("residual",), None),
    }


def _bad(case, a):
    """(the arrays with `measurements` [2E] spoilt, further arguments, what the TypeError says)"""
    import torch
    z = a["measurements"]
    if case == "host_array":
        return dict(a, measurements=z.cpu().numpy()), {}, "measurements: a host array beside device tensors"
    if case == "dtype":
        return dict(a, measurements=z.double()), {}, "measurements: dtype torch.float64"
    if case == "not_contiguous":
        return dict(a, measurements=torch.zeros(4 * E_, dtype=torch.float32, device="cuda")[::2]), {}, "measurements is not contiguous"
    if case == "count":
        return dict(a, measurements=torch.zeros(2 * E_ + 1, dtype=torch.float32, device="cuda")), {}, "measurements has 9 elements, expected 8"
    if case == "unknown_out":
        return a, {"out": {"bogus": z}}, r"out: unknown arrays \['bogus'\]"
    raise AssertionError(case)


# (post.residuals takes neither `out` nor options: nothing to refuse there)
REFUSALS = [(n, c) for n in ("seed", "resect", "locate", "post") for c in ("host_array", "dtype", "not_contiguous", "count", "unknown_out", "options")
            if not (n == "post" and c in ("unknown_out", "options"))]


@pytest.mark.parametrize("name,case", REFUSALS)
def test_a_bad_argument_is_a_type_error_naming_it_before_the_library_is_called(name, case, monkeypatch):
    module, fn, call, _, other_options = _libraries()[name]
    a = _arrays()
    if case == "options":
        arrays, more, text = a, {"options": other_options()}, r"options: expected a %s\.Options" % name
    else:
        arrays, more, text = _bad(case, a)

    def called(*args):
        raise AssertionError("%s was called" % fn)

    monkeypatch.setattr(module.load(), fn, called)
    with pytest.raises(TypeError, match=text):
        call(arrays, **more)


@pytest.mark.parametrize("name", ["seed", "resect", "locate", "post"])
def test_the_correct_call_with_every_optional_input_none_succeeds(name):
    import torch
    _, _, call, results, _ = _libraries()[name]
    a = _arrays()
    res = call(a)
    torch.cuda.synchronize()
    assert tuple(res) == results and all(v.is_cuda for v in res.values())
    per = {"seed": L_, "resect": C_, "locate": C_, "post": E_}[name]
    assert res[results[-1]].numel() == (2 * E_ if name == "post" else per)
    if name == "resect":
        assert res["cam_mean"] is a["cam_mean"]      # updated in place, and returned
