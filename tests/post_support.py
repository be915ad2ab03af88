"""What tests/test_post_cpu.py and tests/test_gpu_post.py share: the host twin of the solution readout (tests/sanitize/post_math_main.cpp,
a stand-alone program: compiled here, run as a process, never loaded into python), its file format, the hand-made belief blocks, the
oracle's beliefs of a sequence, and the float64 side of the residual / reprojection-covariance checks."""
import os

import numpy as np

from tests import host_twin, ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "sanitize", "post_math_main.cpp")
BELIEFS = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda")
OUTPUTS = (("cam_mean", 6, np.float32), ("cam_cov", 36, np.float32), ("lmk_mean", 3, np.float32), ("lmk_cov", 9, np.float32),
           ("cam_status", 1, np.uint32), ("lmk_status", 1, np.uint32))


def compile_host(exe, sanitize):
    return host_twin.compile_host(MAIN, exe, sanitize)


def run_host(exe, tmp, beliefs, cam_id=(), lmk_id=(), K=None, measurements=(), active_flag=None, want_cov=True, trig="libm"):
    """-> dict of the eight outputs of the program (flat arrays) for the beliefs (dict of the four arrays) and the edges.
    trig: "libm" (the host's sinf / cosf in the residual's rotation: what gbp_eval_host calls) or "device" (the GPU math library's
    algorithm, bit for bit: the twin of the kernels; see tests/sanitize/device_trig_twin.hpp)"""
    b = [np.ascontiguousarray(beliefs[k], np.float32).ravel() for k in BELIEFS]
    C, L = b[0].size // 6, b[2].size // 3
    cam_id, lmk_id = np.ascontiguousarray(cam_id, np.uint32), np.ascontiguousarray(lmk_id, np.uint32)
    E = cam_id.size
    act = np.ones(E, np.uint32) if active_flag is None else np.ascontiguousarray(active_flag, np.uint32)
    K = np.zeros(9, np.float32) if K is None else np.ascontiguousarray(K, np.float32).ravel()
    parts = [np.array([C, L, E, int(want_cov)], np.uint32)] + b + [cam_id, lmk_id, K, np.ascontiguousarray(measurements, np.float32).ravel(), act]
    outputs = [(name, dt, w * (C if name.startswith("cam") else L)) for name, w, dt in OUTPUTS] + \
              [("residual", np.float32, 2 * E), ("reproj_cov", np.float32, 3 * E)]
    return host_twin.run(exe, tmp, "post", parts, outputs, trig)


def hand_made(width):
    """(eta [4, w], Lambda [4, w, w]) float32: a leading zero diagonal that needs a row swap; an indefinite block (finite inverse);
    the all-zero block; an SPD block with a 2-norm condition of about 1e6"""
    rng = np.random.default_rng(100 + width)
    swap = np.eye(width)
    swap[:2, :2] = [[0.0, 2.0], [2.0, 0.0]]
    swap[2:, 2:] *= 3.0
    swap[0, width - 1] = swap[width - 1, 0] = 0.5
    indef = np.diag([(-1.0) ** i * (i + 1.5) for i in range(width)]) + 0.25 * (np.ones((width, width)) - np.eye(width))
    q, _ = np.linalg.qr(rng.normal(size=(width, width)))
    spd = q @ np.diag(np.logspace(0, 6, width)) @ q.T
    lam = np.stack([swap, indef, np.zeros((width, width)), 0.5 * (spd + spd.T)]).astype(np.float32)
    return rng.normal(size=(4, width)).astype(np.float32), lam


def hand_made_beliefs():
    ce, cl = hand_made(6)
    le, ll = hand_made(3)
    return {"cam_beliefs_eta": ce.ravel(), "cam_beliefs_lambda": cl.ravel(), "lmk_beliefs_eta": le.ravel(), "lmk_beliefs_lambda": ll.ravel()}


def ldl_pivots_positive(lam, width):
    """numpy restatement of ldl_pivots_positive<N> (csrc/kernels/gbp_metric_math.hpp): the un-pivoted LDL^T of the LOWER triangle in
    float64, ok while every pivot is > 0 -> bool per block"""
    A = np.asarray(lam, np.float32).reshape(-1, width, width).astype(np.float64)
    n = A.shape[0]
    Lo, D, ok = np.zeros((n, width, width)), np.zeros((n, width)), np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(width):
            d = A[:, j, j].copy()
            for k in range(j):
                d = d - Lo[:, j, k] * Lo[:, j, k] * D[:, k]
            D[:, j] = d
            ok &= d > 0.0
            for i in range(j + 1, width):
                v = A[:, i, j].copy()
                for k in range(j):
                    v = v - Lo[:, i, k] * Lo[:, j, k] * D[:, k]
                Lo[:, i, j] = v / d
    return ok


def status_restated(lam, mean, cov, width):
    """the two definitions of the status word from the outputs and Lambda"""
    finite = np.isfinite(np.asarray(mean).reshape(-1, width)).all(axis=1) & np.isfinite(np.asarray(cov).reshape(-1, width * width)).all(axis=1)
    return (~finite).astype(np.uint32) | ((~ldl_pivots_positive(lam, width)).astype(np.uint32) << 1)


def oracle_sequence(oracle_mod, name, n=200):
    """(bal, K, state, beliefs): the CPU oracle's beliefs of a shipped sequence after n passes of the default loop, weakenings included"""
    from gbp_poplar_amd import driver, hostlib
    from tests.conftest import seq_path
    bal = hostlib.bal_read(seq_path(name))
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    orc.upload(state)
    orc.linearise()
    for i in range(n):
        if (i + 1) % 2 == 0 and i < 2 * int(opts.steps):
            orc.weaken_priors()
        orc.iterate(1)
    return bal, K, state, orc.read()


# ---- float64: residual and reprojection covariance at given (float32) means and covariances ----
def _jacobian(x0, K, rotation_transposed):
    """ref64.jacobian's complex step, with the switch of ref64.project that computes something wrong on purpose"""
    J = np.empty((x0.shape[0], 2, 9))
    for k in range(9):
        xc = x0.astype(np.complex128)
        xc[:, k] += 1e-30j
        J[:, :, k] = np.imag(ref64.project(xc, K, rotation_transposed=rotation_transposed)) / 1e-30
    return J


def edges64(bal, K, measurements, out, rotation_transposed=False, lmk_shift=0):
    """(residual [E, 2], S [E, 3]) in float64 from the float32 means / covariances of `out`: ref64.project and the complex-step
    Jacobian at the means, S = J_c cov_c J_c^T + J_l cov_l J_l^T as (S00, S01, S11)"""
    L = int(bal["n_lmks"])
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), (np.asarray(bal["lmk_id"], np.int64) + lmk_shift) % L
    x0 = ref64.factor_points(out["cam_mean"], out["lmk_mean"], bal, lmk_shift)
    r = np.asarray(measurements, np.float64).reshape(-1, 2) - ref64.project(x0, K, rotation_transposed=rotation_transposed)
    J = ref64.jacobian(x0, K) if not rotation_transposed else _jacobian(x0, K, True)
    cc = np.asarray(out["cam_cov"], np.float64).reshape(-1, 6, 6)[cam_id]
    lc = np.asarray(out["lmk_cov"], np.float64).reshape(-1, 3, 3)[lmk_id]
    S = np.einsum("eik,ekl,ejl->eij", J[:, :, :6], cc, J[:, :, :6]) + np.einsum("eik,ekl,ejl->eij", J[:, :, 6:], lc, J[:, :, 6:])
    return r, np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 1, 1]], axis=1)


def residual_error(res, r64):
    """max |r - r64| in pixels"""
    return float(np.max(np.abs(np.asarray(res, np.float64).reshape(-1, 2) - r64)))


def reproj_cov_error(s, s64):
    """max over edges of max |S - S64| / max |S64| of the edge"""
    s = np.asarray(s, np.float64).reshape(-1, 3)
    return float(np.max(np.max(np.abs(s - s64), axis=1) / np.max(np.abs(s64), axis=1)))


# ---- covariances on a tree: the exact marginals ----
KAPPA_LIMIT = 1e3          # variables whose exact marginal precision has a 2-norm condition above this are not checked ...
MAX_UNCHECKED = 0.10       # ... and at most this share of the variables may be left out that way


def tree_covariance_check(ex, out, a_bound, what):
    """The covariances `out` (cam_cov, lmk_cov) of beliefs that have converged on a tree against the exact marginals `ex` (ref64.marginals).
    Per variable v:  max |cov_v - S_v| / max |S_v| <= 6 kappa_v a_bound[*_lambda] + 2^-21  —  the first-order perturbation of an inverse
    (|d inv(P)| <= kappa |dP| / |P| in the 2-norm, 6 between the 2-norm and the max-norm of a 6 x 6 block) under the precision bound
    the exact-inference suite measured, plus the inverse's own rounding (tests/test_post_cpu.py).  Also asserted, in float64: variable v
    given the covariance of variable v + 1 breaks the bound for every checked v, so a wrong order cannot pass.  Returns the figures."""
    fig = {}
    for pre, w in (("cam", 6), ("lmk", 3)):
        P = ex[pre + "_lambda"]
        S = np.linalg.inv(P)
        kappa = np.linalg.cond(P)
        cov = np.asarray(out[pre + "_cov"], np.float64).reshape(-1, w, w)
        scale = np.max(np.abs(S), axis=(1, 2))
        err = np.max(np.abs(cov - S), axis=(1, 2)) / scale
        bound = 6.0 * kappa * a_bound[pre + "_lambda"] + 2.0 ** -21
        ok = kappa <= KAPPA_LIMIT
        wrong = np.max(np.abs(np.roll(S, -1, axis=0) - S), axis=(1, 2)) / scale
        fig[pre] = {"worst_over_bound": float(np.max(err[ok] / bound[ok])), "worst": float(np.max(err[ok])), "unchecked": int((~ok).sum()),
                    "of": int(ok.size), "kappa_max": float(kappa.max()), "wrong_order_over_bound": float(np.min(wrong[ok] / bound[ok]))}
        print("%s %s: %s" % (what, pre, fig[pre]))
        assert (~ok).sum() <= MAX_UNCHECKED * ok.size, fig[pre]
        assert np.all(err[ok] <= bound[ok]), fig[pre]
        assert np.all(wrong[ok] > bound[ok]), fig[pre]
    return fig
