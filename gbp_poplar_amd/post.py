"""Solution readout — Python face of libgbp_mi355x_post.so (include/gbp_mi355x_post.h): means, marginal covariances and a status word
per variable from the beliefs gbp_read returns (moments), reprojection residuals and their covariance per observation (residuals).

Both take torch tensors on the GPU — read in place, results in fresh tensors on the same GPU, nothing waits: the work is queued on
`stream` (a raw stream handle; default: torch's current stream) and the results are valid for what is queued behind it there.  Both
also take numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's (the same _loader): it has no ctx and is not part of the program list.  There is no CPU path: the kernels are HIP."""
import ctypes as C
import os

from . import _devarrays as arr
from ._loader import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgbp_mi355x_post.so")
GBP_POST_ABI_VERSION = 1
STATUS_NONFINITE, STATUS_NONPD = 1, 2      # status bits: an output of the variable is not finite / Lambda fails the LDL^T pivot test
_lib = None

_vp = C.c_void_p
# every symbol include/gbp_mi355x_post.h declares (array pointers are device addresses: passed as void*)
_SIGS = {
    "gbp_post_abi_version": (C.c_int, []),
    "gbp_post_last_error": (C.c_char_p, []),
    "gbp_post_moments": (C.c_int, [_vp, C.c_uint32, C.c_uint32] + [_vp] * 10),
    "gbp_post_residuals": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, C.POINTER(C.c_float)] + [_vp] * 8),
}


def symbols():
    return sorted(_SIGS)


def load():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, "gbp_post_abi_version", GBP_POST_ABI_VERSION, _SIGS)
    return _lib


class PostError(RuntimeError):
    pass


def _chk(rc, what):
    arr.check(rc, what, load().gbp_post_last_error, PostError)


_BELIEFS = (("cam_beliefs_eta", 6), ("cam_beliefs_lambda", 36), ("lmk_beliefs_eta", 3), ("lmk_beliefs_lambda", 9))
_F32, _U32 = arr.F32, arr.U32
_device_of, _tensor, _ptr, _stream_handle = arr.device_of, arr.tensor, arr.ptr, arr.stream_handle
_STATUS = ("cam_status", "lmk_status")      # as numpy: uint32
_WHAT = "the solution readout"              # (what has no CPU path, in the error for numpy arrays without a GPU)


def moments(beliefs, stream=None):
    """beliefs: the four belief arrays of read() (cam_beliefs_eta [6C], cam_beliefs_lambda [36C], lmk_beliefs_eta [3L],
    lmk_beliefs_lambda [9L]; other members are ignored).  Returns cam_mean [6C], cam_cov [36C], lmk_mean [3L], lmk_cov [9L] (float32; the
    covariances row-major, the general inverse: not symmetrised), cam_status [C], lmk_status [L] (int32; STATUS_NONFINITE | STATUS_NONPD).
    Device tensors in: device tensors out, not blocking.  numpy in: numpy out, blocking."""
    import torch
    b = {k: beliefs[k] for k, _ in _BELIEFS}
    if arr.on_host(b):
        return arr.round_trip(b, (), lambda d: moments(d, stream), _STATUS, PostError, _WHAT)
    dev = _device_of(b.values())
    n_c, n_l = b["cam_beliefs_eta"].numel() // 6, b["lmk_beliefs_eta"].numel() // 3
    t = {k: _tensor(k, b[k], _F32, w * (n_c if k.startswith("cam") else n_l), dev) for k, w in _BELIEFS}
    out = {"cam_mean": torch.empty(6 * n_c, dtype=torch.float32, device=dev), "cam_cov": torch.empty(36 * n_c, dtype=torch.float32, device=dev),
           "lmk_mean": torch.empty(3 * n_l, dtype=torch.float32, device=dev), "lmk_cov": torch.empty(9 * n_l, dtype=torch.float32, device=dev),
           "cam_status": torch.empty(n_c, dtype=torch.int32, device=dev), "lmk_status": torch.empty(n_l, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        _chk(load().gbp_post_moments(_vp(_stream_handle(stream)), n_c, n_l, *[_ptr(t[k]) for k, _ in _BELIEFS],
                                     *[_ptr(out[k]) for k in ("cam_mean", "cam_cov", "lmk_mean", "lmk_cov", "cam_status", "lmk_status")]),
             "gbp_post_moments")
    return out


def residuals(cam_id, lmk_id, K, means, measurements, active_flag=None, covs=None, stream=None):
    """One result per edge, in file order.  cam_id, lmk_id [E] (int32 / uint32), K: the nine pin-hole entries (host), means: cam_mean
    [6C] and lmk_mean [3L], measurements [2E], active_flag [E] or None (= all active), covs: cam_cov [36C] and lmk_cov [9L] or None.
    Returns residual [2E] = z - pi(mean) and, with covs, reproj_cov [3E] = (S00, S01, S11) of J_c cov_c J_c^T + J_l cov_l J_l^T (the
    camera-landmark cross term is neglected); inactive edges hold zeros.  Device tensors in: device tensors out, not blocking.  numpy
    in: numpy out, blocking."""
    import torch
    arrays = {"cam_id": cam_id, "lmk_id": lmk_id, "cam_mean": means["cam_mean"], "lmk_mean": means["lmk_mean"], "measurements": measurements,
              "active_flag": active_flag, "cam_cov": None if covs is None else covs["cam_cov"], "lmk_cov": None if covs is None else covs["lmk_cov"]}
    ints = ("cam_id", "lmk_id", "active_flag")
    if arr.on_host(arrays):
        return arr.round_trip(arrays, ints, lambda d: residuals(d["cam_id"], d["lmk_id"], K, d, d["measurements"], d["active_flag"],
                                                                None if covs is None else d, stream), _STATUS, PostError, _WHAT)
    present = [a for a in arrays.values() if a is not None]
    dev = _device_of(present)
    n_e = arrays["cam_id"].numel()
    n_c, n_l = arrays["cam_mean"].numel() // 6, arrays["lmk_mean"].numel() // 3
    counts = {"cam_id": n_e, "lmk_id": n_e, "cam_mean": 6 * n_c, "lmk_mean": 3 * n_l, "measurements": 2 * n_e, "active_flag": n_e,
              "cam_cov": 36 * n_c, "lmk_cov": 9 * n_l}
    t = {k: None if a is None else _tensor(k, a, _U32 if k in ints else _F32, counts[k], dev) for k, a in arrays.items()}
    out = {"residual": torch.empty(2 * n_e, dtype=torch.float32, device=dev)}
    if covs is not None:
        out["reproj_cov"] = torch.empty(3 * n_e, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _chk(load().gbp_post_residuals(_vp(_stream_handle(stream)), n_c, n_l, n_e, _ptr(t["cam_id"]), _ptr(t["lmk_id"]), arr.k9(K), _ptr(t["cam_mean"]),
                                       _ptr(t["lmk_mean"]), _ptr(t["measurements"]), _ptr(t["active_flag"]), _ptr(t["cam_cov"]), _ptr(t["lmk_cov"]),
                                       _ptr(out["residual"]), _ptr(out.get("reproj_cov"))), "gbp_post_residuals")
    return out
