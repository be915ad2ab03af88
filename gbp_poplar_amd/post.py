"""Solution readout — Python face of libgbp_mi355x_post.so (include/gbp_mi355x_post.h): means, marginal covariances and a status word
per variable from the beliefs gbp_read returns (moments), reprojection residuals and their covariance per observation (residuals).

Both take torch tensors on the GPU — read in place, results in fresh tensors on the same GPU, nothing waits: the work is queued on
`stream` (a raw stream handle; default: torch's current stream) and the results are valid for what is queued behind it there.  Both
also take numpy arrays: those are staged through device tensors and the call blocks until the numpy results are there.  The library is
loaded beside _lib.py's (the same _loader): it has no ctx and is not part of the program list.  There is no CPU path: the kernels are HIP."""
import ctypes as C

from . import _stateless as st
from ._stateless import F32P, VP

GBP_POST_ABI_VERSION = 1
STATUS_NONFINITE, STATUS_NONPD = 1, 2      # status bits: an output of the variable is not finite / Lambda fails the LDL^T pivot test


class PostError(RuntimeError):
    pass


# every symbol include/gbp_mi355x_post.h declares
_SIGS = {
    "gbp_post_abi_version": (C.c_int, []),
    "gbp_post_last_error": (C.c_char_p, []),
    "gbp_post_moments": (C.c_int, [VP, C.c_uint32, C.c_uint32] + [VP] * 10),
    "gbp_post_residuals": (C.c_int, [VP, C.c_uint32, C.c_uint32, C.c_uint32, VP, VP, F32P] + [VP] * 8),
}
BINDING = st.Binding("post", _SIGS, GBP_POST_ABI_VERSION, PostError, "the solution readout")
LIB_PATH, load, symbols = BINDING.LIB_PATH, BINDING.load, BINDING.symbols

# (the outputs are made with torch.empty: both calls write every entry)
_MOMENTS = st.Call(
    "gbp_post_moments",
    inputs=(("cam_beliefs_eta", "f32", 6, "C"), ("cam_beliefs_lambda", "f32", 36, "C"), ("lmk_beliefs_eta", "f32", 3, "L"), ("lmk_beliefs_lambda", "f32", 9, "L")),
    outputs=(("cam_mean", "f32", 6, "C"), ("cam_cov", "f32", 36, "C"), ("lmk_mean", "f32", 3, "L"), ("lmk_cov", "f32", 9, "L"),
             ("cam_status", "u32", 1, "C"), ("lmk_status", "u32", 1, "L")),
    dims=lambda a: {"C": a["cam_beliefs_eta"].numel() // 6, "L": a["lmk_beliefs_eta"].numel() // 3},
    args=("stream", "C", "L", "cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "cam_mean", "cam_cov", "lmk_mean",
          "lmk_cov", "cam_status", "lmk_status"),
    alloc="empty")
_RESIDUALS = st.Call(
    "gbp_post_residuals",
    inputs=(("cam_id", "u32", 1, "E"), ("lmk_id", "u32", 1, "E"), ("cam_mean", "f32", 6, "C"), ("lmk_mean", "f32", 3, "L"), ("measurements", "f32", 2, "E"),
            ("active_flag", "u32", 1, "E", True), ("cam_cov", "f32", 36, "C", True), ("lmk_cov", "f32", 9, "L", True)),
    outputs=(("residual", "f32", 2, "E"), ("reproj_cov", "f32", 3, "E", "cam_cov")),
    dims=lambda a: {"E": a["cam_id"].numel(), "C": a["cam_mean"].numel() // 6, "L": a["lmk_mean"].numel() // 3},
    args=("stream", "C", "L", "E", "cam_id", "lmk_id", "K", "cam_mean", "lmk_mean", "measurements", "active_flag", "cam_cov", "lmk_cov", "residual",
          "reproj_cov"),
    alloc="empty")


def moments(beliefs, stream=None):
    """beliefs: the four belief arrays of read() (cam_beliefs_eta [6C], cam_beliefs_lambda [36C], lmk_beliefs_eta [3L],
    lmk_beliefs_lambda [9L]; other members are ignored).  Returns cam_mean [6C], cam_cov [36C], lmk_mean [3L], lmk_cov [9L] (float32; the
    covariances row-major, the general inverse: not symmetrised), cam_status [C], lmk_status [L] (int32; STATUS_NONFINITE | STATUS_NONPD).
    Device tensors in: device tensors out, not blocking.  numpy in: numpy out, blocking."""
    return BINDING.call(_MOMENTS, {s[0]: beliefs[s[0]] for s in _MOMENTS.inputs}, stream=stream)


def residuals(cam_id, lmk_id, K, means, measurements, active_flag=None, covs=None, stream=None):
    """One result per edge, in file order.  cam_id, lmk_id [E] (int32 / uint32), K: the nine pin-hole entries (host), means: cam_mean
    [6C] and lmk_mean [3L], measurements [2E], active_flag [E] or None (= all active), covs: cam_cov [36C] and lmk_cov [9L] or None.
    Returns residual [2E] = z - pi(mean) and, with covs, reproj_cov [3E] = (S00, S01, S11) of J_c cov_c J_c^T + J_l cov_l J_l^T (the
    camera-landmark cross term is neglected); inactive edges hold zeros.  Device tensors in: device tensors out, not blocking.  numpy
    in: numpy out, blocking."""
    arrays = {"cam_id": cam_id, "lmk_id": lmk_id, "cam_mean": means["cam_mean"], "lmk_mean": means["lmk_mean"], "measurements": measurements,
              "active_flag": active_flag, "cam_cov": None if covs is None else covs["cam_cov"], "lmk_cov": None if covs is None else covs["lmk_cov"]}
    return BINDING.call(_RESIDUALS, arrays, K=K, stream=stream)
