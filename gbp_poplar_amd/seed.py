"""Seeding — Python face of libgbp_mi355x_seed.so (include/gbp_mi355x_seed.h): the landmark-major index of a graph (index, host), the
triangulated mean, prior and status word of every landmark from observations and camera poses (landmarks), and the prior eta of a new
keyframe from the previous camera's belief (keyframe).

landmarks and keyframe take torch tensors on the GPU — read in place, results in fresh tensors on the same GPU or written into the
tensors passed as `out`, nothing waits: the work is queued on `stream` (a raw stream handle; default: torch's current stream).  Both
also take numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's and post.py's (the same _loader): it has no ctx.  There is no CPU path: the kernels are HIP."""
import ctypes as C
import os

import numpy as np

from . import _cabi as cabi
from . import _devarrays as arr
from ._devarrays import F32 as _F32, U32 as _U32, device_of as _device_of, ptr as _ptr, stream_handle as _stream_handle, tensor as _tensor
from ._loader import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgbp_mi355x_seed.so")
GBP_SEED_ABI_VERSION = 1
# status bits (GBP_SEED_* of the header)
NO_VIEW, ONE_VIEW, LOW_PARALLAX, BEHIND, NONFINITE, BAD_INDEX = 1, 2, 4, 8, 16, 32
_lib = None

_vp = C.c_void_p
_u32p = C.POINTER(C.c_uint32)


class Options(C.Structure):
    """gbp_seed_options"""
    _fields_ = [("min_parallax", C.c_float), ("fallback_depth", C.c_float), ("refine_iters", C.c_uint32), ("reproj_meas_var", C.c_float)]


# every symbol include/gbp_mi355x_seed.h declares (device array pointers are passed as void*)
_SIGS = {
    "gbp_seed_abi_version": (C.c_int, []),
    "gbp_seed_last_error": (C.c_char_p, []),
    "gbp_seed_default_options": (C.c_int, [C.POINTER(Options)]),
    "gbp_seed_index": (C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]),
    "gbp_seed_check_index": (C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p]),
    "gbp_seed_workspace_bytes": (C.c_size_t, [C.c_uint32]),
    "gbp_seed_landmarks": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.POINTER(C.c_float)] + [_vp] * 4 +
                           [C.POINTER(Options)] + [_vp] * 6),
    "gbp_seed_keyframe": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32] + [_vp] * 5),
}


def symbols():
    return sorted(_SIGS)


def load():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, "gbp_seed_abi_version", GBP_SEED_ABI_VERSION, _SIGS)
    return _lib


class SeedError(RuntimeError):
    pass


def _chk(rc, what):
    arr.check(rc, what, load().gbp_seed_last_error, SeedError)


_WHAT = "the seeding"      # (what has no CPU path, in the error for numpy arrays without a GPU)


def default_options(**changes):
    """the library's defaults as an Options, with `changes` applied (min_parallax, fallback_depth, refine_iters, reproj_meas_var)"""
    o = Options()
    _chk(load().gbp_seed_default_options(C.byref(o)), "gbp_seed_default_options")
    for k, v in changes.items():
        if k not in dict(Options._fields_):
            raise TypeError("gbp_seed_options has no field %r" % k)
        setattr(o, k, v)
    return o


def _host_u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return a, a.ctypes.data_as(_u32p)


def index(lmk_id, n_lmks):
    """HOST.  (lmk_start [L + 1], lmk_edges [E]) uint32: the edges of landmark l are lmk_edges[lmk_start[l]:lmk_start[l + 1]], in file order"""
    ids, p_ids = _host_u32(lmk_id)
    start, edges = np.zeros(int(n_lmks) + 1, np.uint32), np.zeros(ids.size, np.uint32)
    _chk(load().gbp_seed_index(int(n_lmks), ids.size, p_ids, start.ctypes.data_as(_u32p), edges.ctypes.data_as(_u32p)), "gbp_seed_index")
    return start, edges


def check_index(lmk_start, lmk_edges):
    """HOST.  Raises SeedError unless (lmk_start, lmk_edges) is a well-formed index of lmk_edges.size edges."""
    start, p_start = _host_u32(lmk_start)
    edges, p_edges = _host_u32(lmk_edges)
    if start.size == 0:
        raise SeedError("gbp_seed_check_index: lmk_start is empty")
    _chk(load().gbp_seed_check_index(start.size - 1, edges.size, p_start, p_edges), "gbp_seed_check_index")


def workspace_bytes(n_cams):
    return int(load().gbp_seed_workspace_bytes(int(n_cams)))


_OUT = (("lmk_mean", 3, "float"), ("lmk_priors_eta", 3, "float"), ("lmk_priors_lambda", 9, "float"), ("status", 1, "int"), ("n_views", 1, "int"))
_INTS = ("cam_id", "lmk_start", "lmk_edges", "active_flag", "select")
_UINTS = ("status", "n_views")      # the integer outputs: uint32 as numpy


def landmarks(cam_id, lmk_start, lmk_edges, K, cam_mean, measurements, active_flag=None, select=None, options=None, out=None, workspace=None,
              stream=None):
    """cam_id [E], (lmk_start [L + 1], lmk_edges [E]) = index(), K: the nine pin-hole entries (host), cam_mean [6C], measurements [2E],
    active_flag [E] or None (= all active), select [L] or None (= every landmark), options: an Options (default_options()).
    Returns lmk_mean [3L], lmk_priors_eta [3L], lmk_priors_lambda [9L] (float32), status [L], n_views [L] (int32 on the device, uint32 as
    numpy; status: NO_VIEW | ONE_VIEW | LOW_PARALLAX | BEHIND | NONFINITE | BAD_INDEX).  `out`: a dict with any of the five — the call
    writes INTO those (a landmark that is not selected, or has no used view, keeps what they hold: the arrays of read_priors(device=True),
    say); the others are fresh, zero where nothing is written.  workspace: a device tensor of at least workspace_bytes(C) bytes
    (default: a fresh one).  Device tensors in: device tensors out, not blocking.  numpy in: numpy out, blocking, the index checked."""
    import torch
    arrays = {"cam_id": cam_id, "lmk_start": lmk_start, "lmk_edges": lmk_edges, "cam_mean": cam_mean, "measurements": measurements,
              "active_flag": active_flag, "select": select}
    out = dict(out or {})
    unknown = set(out) - {k for k, _, _ in _OUT}
    if unknown:
        raise TypeError("out: unknown arrays %s" % sorted(unknown))
    if arr.on_host(dict(arrays, **out)):      # (the two sets of names are disjoint)
        check_index(lmk_start, lmk_edges)
        return arr.round_trip(dict(arrays, **out), _INTS + _UINTS, lambda d: landmarks(
            d["cam_id"], d["lmk_start"], d["lmk_edges"], K, d["cam_mean"], d["measurements"], d["active_flag"], d["select"], options,
            {k: d[k] for k in out}, None, stream), _UINTS, SeedError, _WHAT)
    dev = _device_of([a for a in list(arrays.values()) + list(out.values()) if a is not None])
    n_e, n_l, n_c = arrays["cam_id"].numel(), arrays["lmk_start"].numel() - 1, arrays["cam_mean"].numel() // 6
    if n_l < 0:
        raise TypeError("lmk_start is empty: it has n_lmks + 1 entries")
    counts = {"cam_id": n_e, "lmk_start": n_l + 1, "lmk_edges": n_e, "cam_mean": 6 * n_c, "measurements": 2 * n_e, "active_flag": n_e, "select": n_l}
    t = {k: None if a is None else _tensor(k, a, _U32 if k in _INTS else _F32, counts[k], dev) for k, a in arrays.items()}
    res = {}
    for k, w, kind in _OUT:
        if k in out:
            res[k] = _tensor(k, out[k], _U32 if kind == "int" else _F32, w * n_l, dev)
        else:
            res[k] = torch.zeros(w * n_l, dtype=torch.int32 if kind == "int" else torch.float32, device=dev)
    need = workspace_bytes(n_c)
    if workspace is None:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    elif not cabi.is_device_tensor(workspace) or workspace.device != dev or workspace.numel() * workspace.element_size() < need:
        raise TypeError("workspace: expected a tensor of at least %d bytes on %s" % (need, dev))
    opts = options if options is not None else default_options()
    if not isinstance(opts, Options):
        raise TypeError("options: expected a seed.Options (seed.default_options(...))")
    with torch.cuda.device(dev):
        _chk(load().gbp_seed_landmarks(_vp(_stream_handle(stream)), n_c, n_l, n_e, _ptr(t["cam_id"]), _ptr(t["lmk_start"]), _ptr(t["lmk_edges"]), arr.k9(K),
                                       _ptr(t["cam_mean"]), _ptr(t["measurements"]), _ptr(t["active_flag"]), _ptr(t["select"]), C.byref(opts),
                                       _ptr(workspace), *[_ptr(res[k]) for k, _, _ in _OUT]), "gbp_seed_landmarks")
    return res


def keyframe(src, dst, cam_beliefs_eta, cam_beliefs_lambda, cam_priors_lambda, cam_priors_eta, stream=None):
    """The prior eta of camera dst from the belief of camera src (hostlib.slam_initialise_new_kf on the device, bit for bit, with
    dst = src + 1).  Device tensors: cam_priors_eta [6C] is updated IN PLACE and (cam_priors_eta, cam_mean [6]) is returned, not
    blocking; cam_mean is the mean of camera src, the pose guess of the new camera.  numpy: the same pair as fresh numpy arrays, blocking."""
    import torch
    arrays = {"cam_beliefs_eta": cam_beliefs_eta, "cam_beliefs_lambda": cam_beliefs_lambda, "cam_priors_lambda": cam_priors_lambda,
              "cam_priors_eta": cam_priors_eta}
    if arr.on_host(arrays):
        return arr.round_trip(arrays, (), lambda d: keyframe(src, dst, d["cam_beliefs_eta"], d["cam_beliefs_lambda"], d["cam_priors_lambda"],
                                                             d["cam_priors_eta"], stream), (), SeedError, _WHAT)
    dev = _device_of(arrays.values())
    n_c = arrays["cam_beliefs_eta"].numel() // 6
    t = {k: _tensor(k, a, _F32, (36 if k.endswith("lambda") else 6) * n_c, dev) for k, a in arrays.items()}
    mean = torch.empty(6, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _chk(load().gbp_seed_keyframe(_vp(_stream_handle(stream)), n_c, int(src), int(dst), _ptr(t["cam_beliefs_eta"]), _ptr(t["cam_beliefs_lambda"]),
                                      _ptr(t["cam_priors_lambda"]), _ptr(t["cam_priors_eta"]), _ptr(mean)), "gbp_seed_keyframe")
    return t["cam_priors_eta"], mean
