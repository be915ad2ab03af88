"""Resection — Python face of libgbp_mi355x_resect.so (include/gbp_mi355x_resect.h): the camera-major index of a graph (index, host) and
the pose of every selected camera from its observations of landmarks that are already mapped (cameras): pose-only Levenberg-Marquardt
against fixed landmarks, with the prior eta at the result, an information matrix, a report and a status word.

cameras takes torch tensors on the GPU — read and updated in place, further results in fresh tensors on the same GPU or written into
the tensors passed as `out`, nothing waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  It
also takes numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's, post.py's and seed.py's (the same _loader): it has no ctx.  There is no CPU path: the kernel is HIP."""
import ctypes as C

import numpy as np

from . import _stateless as st
from ._stateless import F32P, U32P, VP

GBP_RESECT_ABI_VERSION = 1
# status bits (GBP_RESECT_* of the header; the shared ones have seed's values)
NO_VIEW, BEHIND, NONFINITE, BAD_INDEX, FEW_VIEWS, STALLED = 1, 8, 16, 32, 64, 128
NOT_RESECTED = NO_VIEW | FEW_VIEWS | NONFINITE | STALLED      # the pose is the start pose


class Options(C.Structure):
    """gbp_resect_options"""
    _fields_ = [("max_passes", C.c_uint32), ("min_views", C.c_uint32), ("huber_px", C.c_float), ("lambda0", C.c_float),
                ("reproj_meas_var", C.c_float)]


class ResectError(RuntimeError):
    pass


# every symbol include/gbp_mi355x_resect.h declares
_SIGS = {
    "gbp_resect_abi_version": (C.c_int, []),
    "gbp_resect_last_error": (C.c_char_p, []),
    "gbp_resect_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_resect_index": (C.c_int, [C.c_uint32, C.c_uint32, U32P, U32P, U32P]),
    "gbp_resect_check_index": (C.c_int, [C.c_uint32, C.c_uint32, U32P, U32P]),
    "gbp_resect_cameras": (C.c_int, [VP, C.c_uint32, C.c_uint32, C.c_uint32, VP, VP, VP, F32P] + [VP] * 5 + [C.POINTER(Options)] + [VP] * 7),
}
BINDING = st.Binding("resect", _SIGS, GBP_RESECT_ABI_VERSION, ResectError, "the resection")
LIB_PATH, load, symbols = BINDING.LIB_PATH, BINDING.load, BINDING.symbols


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (max_passes, min_views, huber_px, lambda0, reproj_meas_var)"""
    return BINDING.default_options(Options, **changes)


def index(cam_id, n_cams):
    """HOST.  (cam_start [C + 1], cam_edges [E]) uint32: the edges of camera c are cam_edges[cam_start[c]:cam_start[c + 1]], in file order"""
    return BINDING.index(cam_id, n_cams)


def check_index(cam_start, cam_edges, n_edges=None):
    """HOST.  Raises ResectError unless (cam_start, cam_edges) is a well-formed index.  cam_edges None (entry k is edge k): cam_start
    alone is checked, against n_edges edges (default: its own last entry)."""
    BINDING.check_index("cam_start", cam_start, cam_edges, n_edges)


# the inputs of a camera-major call (locate.cameras takes the same) and how its dimensions follow from them
CAMERA_INPUTS = (("lmk_id", "u32", 1, "E"), ("cam_start", "u32", 1, "C + 1"), ("cam_edges", "u32", 1, "E", True), ("lmk_mean", "f32", 3, "L"),
                 ("measurements", "f32", 2, "E"), ("active_flag", "u32", 1, "E", True), ("lmk_use", "u32", 1, "L", True), ("select", "u32", 1, "C", True))


def camera_dims(a):
    return st.index_dims(a["lmk_id"], a["cam_start"], "C", "cam_start", "n_cams", L=a["lmk_mean"].numel() // 3)


_CAMERAS = st.Call(
    "gbp_resect_cameras",
    inputs=CAMERA_INPUTS[:3] + (("cam_mean", "f32", 6, "C"),) + CAMERA_INPUTS[3:] + (("priors_lambda", "f32", 36, "C", True),),
    outputs=(("cam_priors_eta", "f32", 6, "C", "priors_lambda"), ("cam_info", "f32", 36, "C"), ("report", "f32", 4, "C"), ("status", "u32", 1, "C"),
             ("n_views", "u32", 1, "C")),
    dims=camera_dims,
    args=("stream", "C", "L", "E", "lmk_id", "cam_start", "cam_edges", "K", "lmk_mean", "measurements", "active_flag", "lmk_use", "select", "opts",
          "cam_mean", "priors_lambda", "cam_priors_eta", "cam_info", "report", "status", "n_views"),
    options=Options, returns=("cam_mean",))


def cameras(lmk_id, cam_start, cam_edges, K, cam_mean, lmk_mean, measurements, active_flag=None, lmk_use=None, select=None, options=None,
            priors_lambda=None, out=None, stream=None):
    """lmk_id [E], (cam_start [C + 1], cam_edges [E]) = index() — cam_edges None: entry k is edge k (a file sorted by camera) —, K: the
    nine pin-hole entries (host), cam_mean [6C]: the START poses, lmk_mean [3L]: the map, measurements [2E], active_flag [E] or None
    (= all active), lmk_use [L] or None (= every landmark), select [C] or None (= every camera), options: an Options
    (default_options()), priors_lambda [36C] or None: the camera prior Lambdas, for cam_priors_eta.
    Returns a dict: cam_mean [6C], cam_info [36C], report [4C] (float32), status [C], n_views [C] (int32 on the device, uint32 as numpy;
    status: NO_VIEW | BEHIND | NONFINITE | BAD_INDEX | FEW_VIEWS | STALLED), and cam_priors_eta [6C] if priors_lambda is given.  `out`: a
    dict with any of cam_priors_eta, cam_info, report, status, n_views — the call writes INTO those (a camera that is not selected, or
    is not resected, keeps what they hold: the arrays of read_priors(device=True), say); the others are fresh, zero where nothing is
    written.  Device tensors in: cam_mean is updated IN PLACE (and returned), nothing blocks.  numpy in: numpy out (cam_mean a fresh
    array), blocking, the index checked first."""
    arrays = {"lmk_id": lmk_id, "cam_start": cam_start, "cam_edges": cam_edges, "lmk_mean": lmk_mean, "measurements": measurements,
              "active_flag": active_flag, "lmk_use": lmk_use, "select": select, "cam_mean": cam_mean, "priors_lambda": priors_lambda}
    return BINDING.call(_CAMERAS, arrays, K=K, options=options, out=out, stream=stream,
                        host_check=lambda: check_index(cam_start, cam_edges, np.asarray(lmk_id).size))
