"""Location — Python face of libgbp_mi355x_locate.so (include/gbp_mi355x_locate.h): the pose of every selected camera from its
observations of landmarks that are already mapped, with NO pose guess and with wrong matches among the observations (cameras): 64 x
rounds three-point hypotheses scored by the number of observations that agree, the winner's pose, the mask of the observations that
agree with it, a report and a status word.  The index is resect.index's.

cameras takes torch tensors on the GPU — results in fresh tensors on the same GPU or written into the tensors passed as `out`, nothing
waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  It also takes numpy arrays: those are
staged through device tensors and the call blocks until the numpy results are there.  The library is loaded beside _lib.py's, post.py's,
seed.py's and resect.py's (the same _loader): it has no ctx.  There is no CPU path: the kernel is HIP."""
import ctypes as C
import os

import numpy as np

from . import _devarrays as arr
from ._devarrays import F32 as _F32, U32 as _U32, device_of as _device_of, ptr as _ptr, stream_handle as _stream_handle, tensor as _tensor
from ._loader import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgbp_mi355x_locate.so")
GBP_LOCATE_ABI_VERSION = 1
# status bits (GBP_LOCATE_* of the header; the shared ones have resect's values)
NO_VIEW, BAD_INDEX, FEW_VIEWS, FEW_INLIERS, NO_HYPOTHESIS = 1, 32, 64, 256, 512
NOT_LOCATED = NO_VIEW | FEW_VIEWS | FEW_INLIERS | NO_HYPOTHESIS      # neither a pose nor a mask is written
_lib = None

_vp = C.c_void_p


class Options(C.Structure):
    """gbp_locate_options"""
    _fields_ = [("rounds", C.c_uint32), ("inlier_px", C.c_float), ("min_inliers", C.c_uint32), ("seed", C.c_uint32)]


# every symbol include/gbp_mi355x_locate.h declares (device array pointers are passed as void*)
_SIGS = {
    "gbp_locate_abi_version": (C.c_int, []),
    "gbp_locate_last_error": (C.c_char_p, []),
    "gbp_locate_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_locate_cameras": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.POINTER(C.c_float)] + [_vp] * 5 +
                           [C.POINTER(Options)] + [_vp] * 6),
}


def symbols():
    return sorted(_SIGS)


def load():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, "gbp_locate_abi_version", GBP_LOCATE_ABI_VERSION, _SIGS)
    return _lib


class LocateError(RuntimeError):
    pass


def _chk(rc, what):
    arr.check(rc, what, load().gbp_locate_last_error, LocateError)


_WHAT = "the location"      # (what has no CPU path, in the error for numpy arrays without a GPU)


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (rounds, inlier_px, min_inliers, seed)"""
    o = Options()
    _chk(load().gbp_locate_default_options(C.byref(o)), "gbp_locate_default_options")
    for k, v in changes.items():
        if k not in dict(Options._fields_):
            raise TypeError("gbp_locate_options has no field %r" % k)
        setattr(o, k, v)
    return o


# (name, entries per camera — None: one per edge —, kind)
_OUT = (("cam_mean", 6, "float"), ("inlier", None, "int"), ("report", 4, "float"), ("status", 1, "int"), ("n_views", 1, "int"),
        ("n_inliers", 1, "int"))
_INTS = ("lmk_id", "cam_start", "cam_edges", "active_flag", "lmk_use", "select")
_UINTS = ("inlier", "status", "n_views", "n_inliers")      # the integer outputs: uint32 as numpy


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
    import torch
    arrays = {"lmk_id": lmk_id, "cam_start": cam_start, "cam_edges": cam_edges, "lmk_mean": lmk_mean, "measurements": measurements,
              "active_flag": active_flag, "lmk_use": lmk_use, "select": select}
    out = dict(out or {})
    unknown = set(out) - {k for k, _, _ in _OUT}
    if unknown:
        raise TypeError("out: unknown arrays %s" % sorted(unknown))
    if arr.on_host(dict(arrays, **out)):      # (the two sets of names are disjoint)
        from . import resect
        try:
            resect.check_index(cam_start, cam_edges, np.asarray(lmk_id).size)
        except resect.ResectError as e:
            raise LocateError(str(e)) from None
        return arr.round_trip(dict(arrays, **out), _INTS + _UINTS, lambda d: cameras(
            d["lmk_id"], d["cam_start"], d["cam_edges"], K, d["lmk_mean"], d["measurements"], d["active_flag"], d["lmk_use"], d["select"], options,
            {k: d[k] for k in out}, stream), _UINTS, LocateError, _WHAT)
    dev = _device_of([a for a in list(arrays.values()) + list(out.values()) if a is not None])
    n_e, n_c, n_l = arrays["lmk_id"].numel(), arrays["cam_start"].numel() - 1, arrays["lmk_mean"].numel() // 3
    if n_c < 0:
        raise TypeError("cam_start is empty: it has n_cams + 1 entries")
    counts = {"lmk_id": n_e, "cam_start": n_c + 1, "cam_edges": n_e, "lmk_mean": 3 * n_l, "measurements": 2 * n_e, "active_flag": n_e,
              "lmk_use": n_l, "select": n_c}
    t = {k: None if a is None else _tensor(k, a, _U32 if k in _INTS else _F32, counts[k], dev) for k, a in arrays.items()}
    res = {}
    for k, w, kind in _OUT:
        n = n_e if w is None else w * n_c
        if k in out:
            res[k] = _tensor(k, out[k], _U32 if kind == "int" else _F32, n, dev)
        else:
            res[k] = torch.zeros(n, dtype=torch.int32 if kind == "int" else torch.float32, device=dev)
    opts = options if options is not None else default_options()
    if not isinstance(opts, Options):
        raise TypeError("options: expected a locate.Options (locate.default_options(...))")
    with torch.cuda.device(dev):
        _chk(load().gbp_locate_cameras(_vp(_stream_handle(stream)), n_c, n_l, n_e, _ptr(t["lmk_id"]), _ptr(t["cam_start"]), _ptr(t["cam_edges"]),
                                       arr.k9(K), _ptr(t["lmk_mean"]), _ptr(t["measurements"]), _ptr(t["active_flag"]), _ptr(t["lmk_use"]),
                                       _ptr(t["select"]), C.byref(opts), *[_ptr(res[k]) for k, _, _ in _OUT]), "gbp_locate_cameras")
    return res
