"""Seeding — Python face of libgbp_mi355x_seed.so (include/gbp_mi355x_seed.h): the landmark-major index of a graph (index, host), the
triangulated mean, prior and status word of every landmark from observations and camera poses (landmarks), and the prior eta of a new
keyframe from the previous camera's belief (keyframe).

landmarks and keyframe take torch tensors on the GPU — read in place, results in fresh tensors on the same GPU or written into the
tensors passed as `out`, nothing waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  Both
also take numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's and post.py's (the same _loader): it has no ctx.  There is no CPU path: the kernels are HIP."""
import ctypes as C

from . import _stateless as st
from ._stateless import F32P, U32P, VP

GBP_SEED_ABI_VERSION = 1
# status bits (GBP_SEED_* of the header)
NO_VIEW, ONE_VIEW, LOW_PARALLAX, BEHIND, NONFINITE, BAD_INDEX = 1, 2, 4, 8, 16, 32


class Options(C.Structure):
    """gbp_seed_options"""
    _fields_ = [("min_parallax", C.c_float), ("fallback_depth", C.c_float), ("refine_iters", C.c_uint32), ("reproj_meas_var", C.c_float)]


class SeedError(RuntimeError):
    pass


# every symbol include/gbp_mi355x_seed.h declares
_SIGS = {
    "gbp_seed_abi_version": (C.c_int, []),
    "gbp_seed_last_error": (C.c_char_p, []),
    "gbp_seed_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_seed_index": (C.c_int, [C.c_uint32, C.c_uint32, U32P, U32P, U32P]),
    "gbp_seed_check_index": (C.c_int, [C.c_uint32, C.c_uint32, U32P, U32P]),
    "gbp_seed_workspace_bytes": (C.c_size_t, [C.c_uint32]),
    "gbp_seed_landmarks": (C.c_int, [VP, C.c_uint32, C.c_uint32, C.c_uint32, VP, VP, VP, F32P] + [VP] * 4 + [C.POINTER(Options)] + [VP] * 6),
    "gbp_seed_keyframe": (C.c_int, [VP, C.c_uint32, C.c_uint32, C.c_uint32] + [VP] * 5),
}
BINDING = st.Binding("seed", _SIGS, GBP_SEED_ABI_VERSION, SeedError, "the seeding")
LIB_PATH, load, symbols = BINDING.LIB_PATH, BINDING.load, BINDING.symbols


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (min_parallax, fallback_depth, refine_iters, reproj_meas_var)"""
    return BINDING.default_options(Options, **changes)


def index(lmk_id, n_lmks):
    """HOST.  (lmk_start [L + 1], lmk_edges [E]) uint32: the edges of landmark l are lmk_edges[lmk_start[l]:lmk_start[l + 1]], in file order"""
    return BINDING.index(lmk_id, n_lmks)


def check_index(lmk_start, lmk_edges):
    """HOST.  Raises SeedError unless (lmk_start, lmk_edges) is a well-formed index of lmk_edges.size edges."""
    BINDING.check_index("lmk_start", lmk_start, lmk_edges)


def workspace_bytes(n_cams):
    return int(load().gbp_seed_workspace_bytes(int(n_cams)))


_LANDMARKS = st.Call(
    "gbp_seed_landmarks",
    inputs=(("cam_id", "u32", 1, "E"), ("lmk_start", "u32", 1, "L + 1"), ("lmk_edges", "u32", 1, "E"), ("cam_mean", "f32", 6, "C"),
            ("measurements", "f32", 2, "E"), ("active_flag", "u32", 1, "E", True), ("select", "u32", 1, "L", True)),
    outputs=(("lmk_mean", "f32", 3, "L"), ("lmk_priors_eta", "f32", 3, "L"), ("lmk_priors_lambda", "f32", 9, "L"), ("status", "u32", 1, "L"),
             ("n_views", "u32", 1, "L")),
    dims=lambda a: st.index_dims(a["cam_id"], a["lmk_start"], "L", "lmk_start", "n_lmks", C=a["cam_mean"].numel() // 6),
    args=("stream", "C", "L", "E", "cam_id", "lmk_start", "lmk_edges", "K", "cam_mean", "measurements", "active_flag", "select", "opts", "workspace",
          "lmk_mean", "lmk_priors_eta", "lmk_priors_lambda", "status", "n_views"),
    options=Options, workspace=("gbp_seed_workspace_bytes", "C"))
_KEYFRAME = st.Call(
    "gbp_seed_keyframe",
    inputs=(("cam_beliefs_eta", "f32", 6, "C"), ("cam_beliefs_lambda", "f32", 36, "C"), ("cam_priors_lambda", "f32", 36, "C"), ("cam_priors_eta", "f32", 6, "C")),
    outputs=(("cam_mean", "f32", 6, "one"),),
    dims=lambda a: {"C": a["cam_beliefs_eta"].numel() // 6, "one": 1},
    args=("stream", "C", "src", "dst", "cam_beliefs_eta", "cam_beliefs_lambda", "cam_priors_lambda", "cam_priors_eta", "cam_mean"),
    alloc="empty", returns=("cam_priors_eta",))


def landmarks(cam_id, lmk_start, lmk_edges, K, cam_mean, measurements, active_flag=None, select=None, options=None, out=None, workspace=None,
              stream=None):
    """cam_id [E], (lmk_start [L + 1], lmk_edges [E]) = index(), K: the nine pin-hole entries (host), cam_mean [6C], measurements [2E],
    active_flag [E] or None (= all active), select [L] or None (= every landmark), options: an Options (default_options()).
    Returns lmk_mean [3L], lmk_priors_eta [3L], lmk_priors_lambda [9L] (float32), status [L], n_views [L] (int32 on the device, uint32 as
    numpy; status: NO_VIEW | ONE_VIEW | LOW_PARALLAX | BEHIND | NONFINITE | BAD_INDEX).  `out`: a dict with any of the five — the call
    writes INTO those (a landmark that is not selected, or has no used view, keeps what they hold: the arrays of read_priors(device=True),
    say); the others are fresh, zero where nothing is written.  workspace: a device tensor of at least workspace_bytes(C) bytes
    (default: a fresh one).  Device tensors in: device tensors out, not blocking.  numpy in: numpy out, blocking, the index checked."""
    arrays = {"cam_id": cam_id, "lmk_start": lmk_start, "lmk_edges": lmk_edges, "cam_mean": cam_mean, "measurements": measurements,
              "active_flag": active_flag, "select": select}
    return BINDING.call(_LANDMARKS, arrays, K=K, options=options, out=out, stream=stream, workspace=workspace,
                        host_check=lambda: check_index(lmk_start, lmk_edges))


def keyframe(src, dst, cam_beliefs_eta, cam_beliefs_lambda, cam_priors_lambda, cam_priors_eta, stream=None):
    """The prior eta of camera dst from the belief of camera src (hostlib.slam_initialise_new_kf on the device, bit for bit, with
    dst = src + 1).  Device tensors: cam_priors_eta [6C] is updated IN PLACE and (cam_priors_eta, cam_mean [6]) is returned, not
    blocking; cam_mean is the mean of camera src, the pose guess of the new camera.  numpy: the same pair as fresh numpy arrays, blocking."""
    arrays = {"cam_beliefs_eta": cam_beliefs_eta, "cam_beliefs_lambda": cam_beliefs_lambda, "cam_priors_lambda": cam_priors_lambda,
              "cam_priors_eta": cam_priors_eta}
    res = BINDING.call(_KEYFRAME, arrays, stream=stream, values={"src": int(src), "dst": int(dst)})
    return res["cam_priors_eta"], res["cam_mean"]
