"""Resection — Python face of libgbp_mi355x_resect.so (include/gbp_mi355x_resect.h): the camera-major index of a graph (index, host) and
the pose of every selected camera from its observations of landmarks that are already mapped (cameras): pose-only Levenberg-Marquardt
against fixed landmarks, with the prior eta at the result, an information matrix, a report and a status word.

cameras takes torch tensors on the GPU — read and updated in place, further results in fresh tensors on the same GPU or written into
the tensors passed as `out`, nothing waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  It
also takes numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's, post.py's and seed.py's (the same _loader): it has no ctx.  There is no CPU path: the kernel is HIP."""
import ctypes as C
import os

import numpy as np

from . import _devarrays as arr
from ._devarrays import F32 as _F32, U32 as _U32, device_of as _device_of, ptr as _ptr, stream_handle as _stream_handle, tensor as _tensor
from ._loader import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgbp_mi355x_resect.so")
GBP_RESECT_ABI_VERSION = 1
# status bits (GBP_RESECT_* of the header; the shared ones have seed's values)
NO_VIEW, BEHIND, NONFINITE, BAD_INDEX, FEW_VIEWS, STALLED = 1, 8, 16, 32, 64, 128
NOT_RESECTED = NO_VIEW | FEW_VIEWS | NONFINITE | STALLED      # the pose is the start pose
_lib = None

_vp = C.c_void_p
_u32p = C.POINTER(C.c_uint32)


class Options(C.Structure):
    """gbp_resect_options"""
    _fields_ = [("max_passes", C.c_uint32), ("min_views", C.c_uint32), ("huber_px", C.c_float), ("lambda0", C.c_float),
                ("reproj_meas_var", C.c_float)]


# every symbol include/gbp_mi355x_resect.h declares (device array pointers are passed as void*)
_SIGS = {
    "gbp_resect_abi_version": (C.c_int, []),
    "gbp_resect_last_error": (C.c_char_p, []),
    "gbp_resect_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_resect_index": (C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]),
    "gbp_resect_check_index": (C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p]),
    "gbp_resect_cameras": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.POINTER(C.c_float)] + [_vp] * 5 +
                           [C.POINTER(Options)] + [_vp] * 7),
}


def symbols():
    return sorted(_SIGS)


def load():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, "gbp_resect_abi_version", GBP_RESECT_ABI_VERSION, _SIGS)
    return _lib


class ResectError(RuntimeError):
    pass


def _chk(rc, what):
    arr.check(rc, what, load().gbp_resect_last_error, ResectError)


_WHAT = "the resection"      # (what has no CPU path, in the error for numpy arrays without a GPU)


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (max_passes, min_views, huber_px, lambda0, reproj_meas_var)"""
    o = Options()
    _chk(load().gbp_resect_default_options(C.byref(o)), "gbp_resect_default_options")
    for k, v in changes.items():
        if k not in dict(Options._fields_):
            raise TypeError("gbp_resect_options has no field %r" % k)
        setattr(o, k, v)
    return o


def _host_u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return a, a.ctypes.data_as(_u32p)


def index(cam_id, n_cams):
    """HOST.  (cam_start [C + 1], cam_edges [E]) uint32: the edges of camera c are cam_edges[cam_start[c]:cam_start[c + 1]], in file order"""
    ids, p_ids = _host_u32(cam_id)
    start, edges = np.zeros(int(n_cams) + 1, np.uint32), np.zeros(ids.size, np.uint32)
    _chk(load().gbp_resect_index(int(n_cams), ids.size, p_ids, start.ctypes.data_as(_u32p), edges.ctypes.data_as(_u32p)), "gbp_resect_index")
    return start, edges


def check_index(cam_start, cam_edges, n_edges=None):
    """HOST.  Raises ResectError unless (cam_start, cam_edges) is a well-formed index.  cam_edges None (entry k is edge k): cam_start
    alone is checked, against n_edges edges (default: its own last entry)."""
    start, p_start = _host_u32(cam_start)
    if start.size == 0:
        raise ResectError("gbp_resect_check_index: cam_start is empty")
    if cam_edges is None:
        n_edges, p_edges = int(start[-1]) if n_edges is None else int(n_edges), None
    else:
        edges, p_edges = _host_u32(cam_edges)
        n_edges = edges.size
    _chk(load().gbp_resect_check_index(start.size - 1, n_edges, p_start, p_edges), "gbp_resect_check_index")


_OUT = (("cam_priors_eta", 6, "float"), ("cam_info", 36, "float"), ("report", 4, "float"), ("status", 1, "int"), ("n_views", 1, "int"))
_INTS = ("lmk_id", "cam_start", "cam_edges", "active_flag", "lmk_use", "select")
_UINTS = ("status", "n_views")      # the integer outputs: uint32 as numpy


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
    import torch
    arrays = {"lmk_id": lmk_id, "cam_start": cam_start, "cam_edges": cam_edges, "cam_mean": cam_mean, "lmk_mean": lmk_mean, "measurements": measurements,
              "active_flag": active_flag, "lmk_use": lmk_use, "select": select, "priors_lambda": priors_lambda}
    out = dict(out or {})
    unknown = set(out) - {k for k, _, _ in _OUT}
    if unknown:
        raise TypeError("out: unknown arrays %s" % sorted(unknown))
    if "cam_priors_eta" in out and priors_lambda is None:
        raise TypeError("out: cam_priors_eta needs priors_lambda")
    if arr.on_host(dict(arrays, **out)):      # (the two sets of names are disjoint)
        check_index(cam_start, cam_edges, np.asarray(lmk_id).size)
        return arr.round_trip(dict(arrays, **out), _INTS + _UINTS, lambda d: cameras(
            d["lmk_id"], d["cam_start"], d["cam_edges"], K, d["cam_mean"], d["lmk_mean"], d["measurements"], d["active_flag"], d["lmk_use"],
            d["select"], options, d["priors_lambda"], {k: d[k] for k in out}, stream), _UINTS, ResectError, _WHAT)
    dev = _device_of([a for a in list(arrays.values()) + list(out.values()) if a is not None])
    n_e, n_c, n_l = arrays["lmk_id"].numel(), arrays["cam_start"].numel() - 1, arrays["lmk_mean"].numel() // 3
    if n_c < 0:
        raise TypeError("cam_start is empty: it has n_cams + 1 entries")
    counts = {"lmk_id": n_e, "cam_start": n_c + 1, "cam_edges": n_e, "cam_mean": 6 * n_c, "lmk_mean": 3 * n_l, "measurements": 2 * n_e,
              "active_flag": n_e, "lmk_use": n_l, "select": n_c, "priors_lambda": 36 * n_c}
    t = {k: None if a is None else _tensor(k, a, _U32 if k in _INTS else _F32, counts[k], dev) for k, a in arrays.items()}
    res = {"cam_mean": t["cam_mean"]}
    for k, w, kind in _OUT:
        if k in out:
            res[k] = _tensor(k, out[k], _U32 if kind == "int" else _F32, w * n_c, dev)
        elif k != "cam_priors_eta" or priors_lambda is not None:
            res[k] = torch.zeros(w * n_c, dtype=torch.int32 if kind == "int" else torch.float32, device=dev)
    opts = options if options is not None else default_options()
    if not isinstance(opts, Options):
        raise TypeError("options: expected a resect.Options (resect.default_options(...))")
    with torch.cuda.device(dev):
        _chk(load().gbp_resect_cameras(_vp(_stream_handle(stream)), n_c, n_l, n_e, _ptr(t["lmk_id"]), _ptr(t["cam_start"]), _ptr(t["cam_edges"]),
                                       arr.k9(K), _ptr(t["lmk_mean"]), _ptr(t["measurements"]), _ptr(t["active_flag"]), _ptr(t["lmk_use"]),
                                       _ptr(t["select"]), C.byref(opts), _ptr(t["cam_mean"]), _ptr(t["priors_lambda"]),
                                       _ptr(res.get("cam_priors_eta")), *[_ptr(res[k]) for k, _, _ in _OUT[1:]]), "gbp_resect_cameras")
    return res
