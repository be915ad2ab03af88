"""Exact Gaussian inference and the reprojection metric in float64 numpy: the independent reference of
tests/test_exact_inference.py.  It calls no engine and no oracle and shares no code with either; everything it knows about
the problem is the layout of the tensors that cross the C-ABI.

Variables are ordered cameras first (6 unknowns each: translation 3, rotation vector 3), then landmarks (3 each).
"""
import numpy as np


def _f64(a, *shape):
    return np.asarray(a, np.float64).reshape(*shape)


def var_slices(n_cams, n_lmks):
    """index ranges of every variable in the joint: cameras, then landmarks"""
    cams = [slice(6 * c, 6 * c + 6) for c in range(n_cams)]
    off = 6 * n_cams
    lmks = [slice(off + 3 * l, off + 3 * l + 3) for l in range(n_lmks)]
    return cams, lmks


def factor_block(fac_lambda_e):
    """The 9x9 information matrix of one factor from its 81 floats.  They are four blocks in a row — cc 6x6, cl 6x3, lc 3x6,
    ll 3x3 — not a flat 9x9."""
    f = _f64(fac_lambda_e, 81)
    blk = np.empty((9, 9))
    blk[:6, :6] = f[:36].reshape(6, 6)
    blk[:6, 6:] = f[36:54].reshape(6, 3)
    blk[6:, :6] = f[54:72].reshape(3, 6)
    blk[6:, 6:] = f[72:].reshape(3, 3)
    return blk


def joint(bal, state, fac_eta, fac_lambda, skip=None):
    """Information form (Lambda, eta) of the whole problem: the priors of `state` plus the potential of every active factor
    (`skip`: one factor index left out)."""
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), np.asarray(bal["lmk_id"], np.int64)
    E = cam_id.size
    n = 6 * C + 3 * L
    Lam, eta = np.zeros((n, n)), np.zeros(n)
    cams, lmks = var_slices(C, L)
    cpe, cpl = _f64(state["cam_priors_eta"], C, 6), _f64(state["cam_priors_lambda"], C, 6, 6)
    lpe, lpl = _f64(state["lmk_priors_eta"], L, 3), _f64(state["lmk_priors_lambda"], L, 3, 3)
    for c in range(C):
        Lam[cams[c], cams[c]] += cpl[c]
        eta[cams[c]] += cpe[c]
    for l in range(L):
        Lam[lmks[l], lmks[l]] += lpl[l]
        eta[lmks[l]] += lpe[l]
    active = np.asarray(state["active_flag"]) if "active_flag" in state else np.ones(E, np.uint32)
    fe, fl = _f64(fac_eta, E, 9), _f64(fac_lambda, E, 81)
    for e in range(E):
        if active[e] != 1 or e == skip:
            continue
        blk = factor_block(fl[e])
        sc, sl = cams[cam_id[e]], lmks[lmk_id[e]]
        Lam[sc, sc] += blk[:6, :6]
        Lam[sc, sl] += blk[:6, 6:]
        Lam[sl, sc] += blk[6:, :6]
        Lam[sl, sl] += blk[6:, 6:]
        eta[sc] += fe[e, :6]
        eta[sl] += fe[e, 6:]
    asym = np.max(np.abs(Lam - Lam.T))
    assert asym <= 1e-6 * np.max(np.abs(Lam)), "joint information matrix is not symmetric: %.3e" % asym
    return Lam, eta


def marginals_from_cov(Sigma, mean, n_cams, n_lmks):
    """per variable: mean, marginal precision inv(Sigma_vv), marginal eta = precision @ mean"""
    C, L = int(n_cams), int(n_lmks)
    off = 6 * C
    cm, lm = mean[:off].reshape(C, 6), mean[off:].reshape(L, 3)
    ci = np.arange(off).reshape(C, 6)
    li = off + np.arange(3 * L).reshape(L, 3)
    cS = Sigma[ci[:, :, None], ci[:, None, :]]
    lS = Sigma[li[:, :, None], li[:, None, :]]
    cP, lP = np.linalg.inv(cS), np.linalg.inv(lS)
    return {"cam_mean": cm, "cam_lambda": cP, "cam_eta": np.einsum("vij,vj->vi", cP, cm),
            "lmk_mean": lm, "lmk_lambda": lP, "lmk_eta": np.einsum("vij,vj->vi", lP, lm)}


def marginals(Lambda, eta, n_cams, n_lmks):
    """Dense inverse of the joint; for every variable the exact mean, the exact marginal precision and the marginal eta
    (and the joint's covariance and mean vector, for without_factor)."""
    Sigma = np.linalg.inv(np.asarray(Lambda, np.float64))
    Sigma = 0.5 * (Sigma + Sigma.T)
    mean = Sigma @ np.asarray(eta, np.float64)
    out = marginals_from_cov(Sigma, mean, n_cams, n_lmks)
    out["Sigma"], out["mean"] = Sigma, mean
    return out


def without_factor(Sigma, mean, idx, blk, f_eta):
    """Covariance columns and mean of the joint with one factor taken out, from the full joint's (Sigma, mean) by the Woodbury
    identity: the factor adds U blk U^T to Lambda and U f_eta to eta, U selecting its nine unknowns `idx`.
    Returns (D, mean2) with Sigma2 = Sigma + D[0] @ D[1] (n x 9 times 9 x n)."""
    S_cols = Sigma[:, idx]                       # n x 9
    S_ss = S_cols[idx]                           # 9 x 9
    M = np.linalg.solve(np.eye(9) - blk @ S_ss, blk)       # Sigma2 = Sigma + S_cols M S_cols^T
    mean2 = mean - S_cols @ f_eta + S_cols @ (M @ (mean[idx] - S_ss @ f_eta))
    return (S_cols @ M, S_cols.T), mean2


def belief_means(eta, lam, width):
    """means of float32 beliefs, promoted to float64 and solved there"""
    e = _f64(eta, -1, width)
    lm = _f64(lam, -1, width, width)
    return np.linalg.solve(lm, e[:, :, None])[:, :, 0]


def rodrigues(w):
    """rotation matrix of a rotation vector; the identity below 1e-6"""
    w = np.asarray(w, np.float64)
    th = np.sqrt(w @ w)
    if th < 1e-6:
        return np.eye(3)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * W + ((1.0 - np.cos(th)) / (th * th)) * (W @ W)


def metric_terms(beliefs, bal, K, measurements, active, rotation_transposed=False, lmk_shift=0):
    """Per factor: the norm of the reprojection residual and half its square, 0 for inactive factors.  Means by solve() of the
    float32 beliefs promoted to float64, p = R(w) y + t, prediction = (K p)[:2] / p_z, residual = measurement - prediction.
    rotation_transposed / lmk_shift deliberately compute something wrong (the rotation's transpose; landmark l + shift in place
    of l): what the test's tolerance must be able to tell from the right answer."""
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), np.asarray(bal["lmk_id"], np.int64)
    cm = belief_means(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6)
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = belief_means(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3) if L else np.zeros((0, 3))
    Km = _f64(K, 3, 3)
    z = _f64(measurements, -1, 2)
    act = np.asarray(active)
    norm, half = np.zeros(cam_id.size), np.zeros(cam_id.size)
    R = {}
    for e in np.nonzero(act == 1)[0]:
        c, l = cam_id[e], (lmk_id[e] + lmk_shift) % L
        if c not in R:
            R[c] = rodrigues(cm[c, 3:])
        Rc = R[c].T if rotation_transposed else R[c]
        p = Rc @ lm[l] + cm[c, :3]
        pr = (Km @ p) / p[2]
        r = z[e] - pr[:2]
        norm[e] = np.sqrt(r @ r)
        half[e] = 0.5 * (r @ r)
    return norm, half
