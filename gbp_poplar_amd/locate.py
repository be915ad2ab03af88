"""Location — Python face of libgbp_mi355x_locate.so (include/gbp_mi355x_locate.h): the pose of every selected camera from its
observations of landmarks that are already mapped, with NO pose guess and with wrong matches among the observations (cameras): 64 x
rounds three-point hypotheses scored by the number of observations that agree, the winner's pose, the mask of the observations that
agree with it, a report and a status word.  The index is resect.index's.

cameras takes torch tensors on the GPU — results in fresh tensors on the same GPU or written into the tensors passed as `out`, nothing
waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  It also takes numpy arrays: those are
staged through device tensors and the call blocks until the numpy results are there.  The library is loaded beside _lib.py's, post.py's,
seed.py's and resect.py's (the same _loader): it has no ctx.  There is no CPU path: the kernel is HIP."""
import ctypes as C

import numpy as np

from . import _stateless as st
from . import resect
from ._stateless import F32P, VP

GBP_LOCATE_ABI_VERSION = 1
# status bits (GBP_LOCATE_* of the header; the shared ones have resect's values)
NO_VIEW, BAD_INDEX, FEW_VIEWS, FEW_INLIERS, NO_HYPOTHESIS = 1, 32, 64, 256, 512
NOT_LOCATED = NO_VIEW | FEW_VIEWS | FEW_INLIERS | NO_HYPOTHESIS      # neither a pose nor a mask is written


class Options(C.Structure):
    """gbp_locate_options"""
    _fields_ = [("rounds", C.c_uint32), ("inlier_px", C.c_float), ("min_inliers", C.c_uint32), ("seed", C.c_uint32)]


class LocateError(RuntimeError):
    pass


# every symbol include/gbp_mi355x_locate.h declares
_SIGS = {
    "gbp_locate_abi_version": (C.c_int, []),
    "gbp_locate_last_error": (C.c_char_p, []),
    "gbp_locate_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_locate_cameras": (C.c_int, [VP, C.c_uint32, C.c_uint32, C.c_uint32, VP, VP, VP, F32P] + [VP] * 5 + [C.POINTER(Options)] + [VP] * 6),
}
BINDING = st.Binding("locate", _SIGS, GBP_LOCATE_ABI_VERSION, LocateError, "the location")
LIB_PATH, load, symbols = BINDING.LIB_PATH, BINDING.load, BINDING.symbols


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (rounds, inlier_px, min_inliers, seed)"""
    return BINDING.default_options(Options, **changes)


_CAMERAS = st.Call(
    "gbp_locate_cameras",
    inputs=resect.CAMERA_INPUTS,
    outputs=(("cam_mean", "f32", 6, "C"), ("inlier", "u32", 1, "E"), ("report", "f32", 4, "C"), ("status", "u32", 1, "C"), ("n_views", "u32", 1, "C"),
             ("n_inliers", "u32", 1, "C")),
    dims=resect.camera_dims,
    args=("stream", "C", "L", "E", "lmk_id", "cam_start", "cam_edges", "K", "lmk_mean", "measurements", "active_flag", "lmk_use", "select", "opts",
          "cam_mean", "inlier", "report", "status", "n_views", "n_inliers"),
    options=Options)


def cameras(lmk_id, cam_start, cam_edges, K, lmk_mean, measurements, active_flag=None, lmk_use=None, select=None, options=None, out=None,
            stream=None):
    """lmk_id [E], (cam_start [C + 1], cam_edges [E]) = resect.index() — cam_edges None: entry k is edge k (a file sorted by camera) —, K:
    the nine pin-hole entries (host), lmk_mean [3L]: the map, measurements [2E], active_flag [E] or None (= all active), lmk_use [L] or
    None (= every landmark), select [C] or None (= every camera), options: an Options (default_options()).  No start pose.
    Returns a dict: cam_mean [6C], report [4C] (float32), inlier [E], status [C], n_views [C], n_inliers [C] (int32 on the device,
    uint32 as numpy; status: NO_VIEW | BAD_INDEX | FEW_VIEWS | FEW_INLIERS | NO_HYPOTHESIS; a camera with status & NOT_LOCATED has
    neither a pose nor a mask).  `out`: a dict with any of those six — the call writes INTO them (a camera that is not selected, or is
    not located, keeps what they hold, and so does every entry of inlier that is not a used observation of a located camera); the
    others are fresh, zero where nothing is written.  Device tensors in: nothing blocks.  numpy in: numpy out, blocking, the index
    checked first."""
    arrays = {"lmk_id": lmk_id, "cam_start": cam_start, "cam_edges": cam_edges, "lmk_mean": lmk_mean, "measurements": measurements,
              "active_flag": active_flag, "lmk_use": lmk_use, "select": select}
    return BINDING.call(_CAMERAS, arrays, K=K, options=options, out=out, stream=stream, host_check=lambda: resect.BINDING.check_index(
        "cam_start", cam_start, cam_edges, np.asarray(lmk_id).size, error=LocateError))      # (the index is the resection's)
