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
    """Rotation matrices of rotation vectors (..., 3) -> (..., 3, 3); the identity below 1e-6.  The angle is sqrt(w . w) without a
    conjugate, so a complex w is carried analytically (the complex step of linearise_factor)."""
    w = np.asarray(w)
    w = w if np.iscomplexobj(w) else w.astype(np.float64)
    th2 = w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2]
    small = np.real(th2) < 1e-12
    th = np.sqrt(np.where(small, 1.0, th2))
    W = np.zeros(w.shape[:-1] + (3, 3), w.dtype)
    W[..., 0, 1], W[..., 0, 2] = -w[..., 2], w[..., 1]
    W[..., 1, 0], W[..., 1, 2] = w[..., 2], -w[..., 0]
    W[..., 2, 0], W[..., 2, 1] = -w[..., 1], w[..., 0]
    a = np.where(small, 0.0, np.sin(th) / th)[..., None, None]
    b = np.where(small, 0.0, (1.0 - np.cos(th)) / (th * th))[..., None, None]
    return np.eye(3) + a * W + b * (W @ W)


def project(x9, K, rotation_transposed=False):
    """pi(K (R(w) y + t)) of factors' nine unknowns (..., 9) = [t 3, w 3, y 3] -> (..., 2); real or complex"""
    x9 = np.asarray(x9)
    Km = _f64(K, 3, 3)
    R = rodrigues(x9[..., 3:6])
    if rotation_transposed:
        R = np.swapaxes(R, -1, -2)
    p = np.einsum("...ij,...j->...i", R, x9[..., 6:9]) + x9[..., 0:3]
    q = np.einsum("ij,...j->...i", Km, p)
    return q[..., :2] / p[..., 2:3]


def jacobian(x0, K, method="complex", h=None):
    """d project / d x at x0 (N, 9) -> (N, 2, 9), numerically: by complex step (h = 1e-30: no subtraction, exact to round-off) or by
    central differences (h = 1e-6 by default).  Not a restatement of any closed form."""
    x0 = _f64(x0, -1, 9)
    J = np.empty((x0.shape[0], 2, 9))
    for k in range(9):
        if method == "complex":
            d = 1e-30 if h is None else h
            xc = x0.astype(np.complex128)
            xc[:, k] += 1j * d
            J[:, :, k] = np.imag(project(xc, K)) / d
        else:
            d = 1e-6 if h is None else h
            xp, xm = x0.copy(), x0.copy()
            xp[:, k] += d
            xm[:, k] -= d
            J[:, :, k] = (project(xp, K) - project(xm, K)) / (2 * d)
    return J


def _hat(y):
    H = np.zeros(y.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2] = -y[..., 2], y[..., 1]
    H[..., 1, 0], H[..., 1, 2] = y[..., 2], -y[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -y[..., 1], y[..., 0]
    return H


def huber_mvar(err, var, nstds, no_huber=False):
    """(robust decision err > nstds sqrt(var), the variance the factor is scaled by)"""
    err, var = np.asarray(err, np.float64), np.asarray(var, np.float64)
    s = nstds * np.sqrt(var)
    robust = err > s
    with np.errstate(divide="ignore", invalid="ignore"):
        mv = var * err * err / (2.0 * (s * err - 0.5 * nstds * nstds * var))
    mvar = np.where(robust & (not no_huber), mv, var)
    return robust, mvar


def linearise_factor(x0, K, z, var, nstds, first_order_rotation=False, no_huber=False, flip_residual=False):
    """The linearisation of N reprojection factors at x0 (N, 9), measurements z (N, 2), variances var (N): a dict of
      eta     J^T (J x0 + z - h(x0)), unscaled (N, 9)
      lam     J^T J, unscaled (N, 9, 9)
      err     ||h - z||
      robust  err > nstds sqrt(var)
      mvar    var err^2 / (2 (nstds sqrt(var) err - nstds^2 var / 2)) when robust, else var
      J, h    the Jacobian (complex step) and the prediction.
    The switches deliberately compute something wrong, for the blindness tests: the rotation block taken as the first-order
    -R [y]x (through the landmark block, d pi / d y = (d pi / d p) R); no Huber rescale; the sign of z - h flipped.  (The fourth wrong
    variant, landmark l + 1 in place of l, is the caller's choice of x0.)"""
    x0, z = _f64(x0, -1, 9), _f64(z, -1, 2)
    var = np.broadcast_to(np.asarray(var, np.float64), (x0.shape[0],))
    J = jacobian(x0, K)
    if first_order_rotation:
        J = J.copy()
        J[:, :, 3:6] = -np.einsum("nij,njk->nik", J[:, :, 6:9], _hat(x0[:, 6:9]))
    h = project(x0, K)
    r = h - z if flip_residual else z - h
    rhs = np.einsum("nij,nj->ni", J, x0) + r
    eta = np.einsum("nij,ni->nj", J, rhs)
    lam = np.einsum("nij,nik->njk", J, J)
    err = np.sqrt(np.sum((h - z) ** 2, axis=1))
    robust, mvar = huber_mvar(err, var, nstds, no_huber)
    return {"eta": eta, "lam": lam, "err": err, "robust": robust, "mvar": mvar, "J": J, "h": h}


def factor_points(cam_mean, lmk_mean, bal, lmk_shift=0):
    """x0 (E, 9) of every factor from per-variable means (C, 6), (L, 3); lmk_shift: landmark l + shift in place of l (wrong on purpose)"""
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), np.asarray(bal["lmk_id"], np.int64)
    L = int(bal["n_lmks"])
    return np.concatenate([_f64(cam_mean, -1, 6)[cam_id], _f64(lmk_mean, -1, 3)[(lmk_id + lmk_shift) % L]], axis=1)


def blocks_of(lam81):
    """(E, 9, 9) from the four blocks in a row of the C-ABI (E, 81): factor_block for every factor"""
    f = _f64(lam81, -1, 81)
    out = np.empty((f.shape[0], 9, 9))
    out[:, :6, :6] = f[:, :36].reshape(-1, 6, 6)
    out[:, :6, 6:] = f[:, 36:54].reshape(-1, 6, 3)
    out[:, 6:, :6] = f[:, 54:72].reshape(-1, 3, 6)
    out[:, 6:, 6:] = f[:, 72:].reshape(-1, 3, 3)
    return out


def cost_gradient(means, bal, K, state, nstds=2.5, lmk_shift=0, **wrong):
    """Gradient of  1/2 x^T Lp x - ep^T x + sum over active factors of rho_Huber(||h - z||)  at means = (cam (C, 6), lmk (L, 3)):
    the prior's Lp x - ep, and per factor J^T (h - z) / mvar(err) (rho' / err = 1 / mvar on both sides of the Huber threshold).
    Returns (gradient, scale): per unknown, the sum of the terms and the sum of their absolute values (the prior's products taken one
    by one), the scale of a relative measure.  lmk_shift and the switches of linearise_factor compute something wrong on purpose."""
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), np.asarray(bal["lmk_id"], np.int64)
    cm, lm = _f64(means[0], C, 6), _f64(means[1], L, 3)
    g, s = np.zeros(6 * C + 3 * L), np.zeros(6 * C + 3 * L)
    cpl, cpe = _f64(state["cam_priors_lambda"], C, 6, 6), _f64(state["cam_priors_eta"], C, 6)
    lpl, lpe = _f64(state["lmk_priors_lambda"], L, 3, 3), _f64(state["lmk_priors_eta"], L, 3)
    g[:6 * C] = (np.einsum("vij,vj->vi", cpl, cm) - cpe).ravel()
    s[:6 * C] = (np.einsum("vij,vj->vi", np.abs(cpl), np.abs(cm)) + np.abs(cpe)).ravel()
    g[6 * C:] = (np.einsum("vij,vj->vi", lpl, lm) - lpe).ravel()
    s[6 * C:] = (np.einsum("vij,vj->vi", np.abs(lpl), np.abs(lm)) + np.abs(lpe)).ravel()
    lin = linearise_factor(factor_points(cm, lm, bal, lmk_shift), K, state["measurements"], state["meas_variances"], nstds, **wrong)
    res = (lin["h"] - _f64(state["measurements"], -1, 2)) * (-1.0 if wrong.get("flip_residual") else 1.0)
    t = np.einsum("nij,ni->nj", lin["J"], res) / lin["mvar"][:, None]
    act = np.asarray(state["active_flag"]) == 1 if "active_flag" in state else np.ones(cam_id.size, bool)
    ci = (6 * cam_id[:, None] + np.arange(6))[act]
    li = (6 * C + 3 * lmk_id[:, None] + np.arange(3))[act]
    np.add.at(g, ci, t[act, :6])
    np.add.at(g, li, t[act, 6:])
    np.add.at(s, ci, np.abs(t[act, :6]))
    np.add.at(s, li, np.abs(t[act, 6:]))
    return g, s


def metric_terms(beliefs, bal, K, measurements, active, rotation_transposed=False, lmk_shift=0):
    """Per factor: the norm of the reprojection residual and half its square, 0 for inactive factors.  Means by solve() of the
    float32 beliefs promoted to float64, prediction = project(), residual = measurement - prediction.
    rotation_transposed / lmk_shift deliberately compute something wrong (the rotation's transpose; landmark l + shift in place
    of l): what the test's tolerance must be able to tell from the right answer."""
    L = int(bal["n_lmks"])
    cm = belief_means(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6)
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = belief_means(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3) if L else np.zeros((0, 3))
    z = _f64(measurements, -1, 2)
    act = np.asarray(active) == 1
    norm, half = np.zeros(z.shape[0]), np.zeros(z.shape[0])
    if act.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            r = z[act] - project(factor_points(cm, lm, bal, lmk_shift)[act], K, rotation_transposed=rotation_transposed)
        sq = np.sum(r * r, axis=1)
        norm[act], half[act] = np.sqrt(sq), 0.5 * sq
    return norm, half


# ---- the variable side: beliefs as sums, the health predicates (tests/test_wide_state_cpu.py, tests/test_gpu_wide_state.py) ------
def lower_mirrored(lam, width):
    """(N, width, width) float64 matrices from their LOWER triangles alone, mirrored: how inv6x6 reads a camera's Lambda (the upper
    triangle of a camera message is not stored by the engines, and that of a camera belief is not read by the sweeps)"""
    A = _f64(lam, -1, width, width)
    return np.tril(A) + np.swapaxes(np.tril(A, -1), 1, 2)


def belief_sums(bal, priors, messages, active):
    """Every variable's belief as the plain float64 sum of its prior and the messages of its ACTIVE factors, and beside each sum the sum
    of the absolute values of the same terms (the scale a relative error is measured on).  priors: the four *_priors_* tensors as
    read_priors() returns them; messages: cam_eta [6E], cam_lambda [36E], lmk_eta [3E], lmk_lambda [9E] in file order.  Of a camera's
    Lambdas (prior and messages) only the lower triangle is read and mirrored (lower_mirrored): compare the sum with the lower triangle
    of a camera belief.
    Returns {"cam_eta": (sum (C, 6), scale (C, 6)), "cam_lambda": ((C, 36), (C, 36)), "lmk_eta": ..., "lmk_lambda": ...}."""
    C, L = int(bal["n_cams"]), int(bal["n_lmks"])
    cam_id, lmk_id = np.asarray(bal["cam_id"], np.int64), np.asarray(bal["lmk_id"], np.int64)
    E = cam_id.size
    act = np.asarray(active).reshape(-1) == 1
    cl = lower_mirrored(messages["cam_lambda"], 6)
    terms = {"cam_eta": (cam_id, C, _f64(priors["cam_priors_eta"], C, 6), _f64(messages["cam_eta"], E, 6)),
             "cam_lambda": (cam_id, C, lower_mirrored(priors["cam_priors_lambda"], 6).reshape(C, 36), cl.reshape(E, 36)),
             "lmk_eta": (lmk_id, L, _f64(priors["lmk_priors_eta"], L, 3), _f64(messages["lmk_eta"], E, 3)),
             "lmk_lambda": (lmk_id, L, _f64(priors["lmk_priors_lambda"], L, 9), _f64(messages["lmk_lambda"], E, 9))}
    out = {}
    for k, (ids, n, prior, msg) in terms.items():
        s, a = prior.copy(), np.abs(prior)
        np.add.at(s, ids[act], msg[act])
        np.add.at(a, ids[act], np.abs(msg[act]))
        out[k] = (s, a)
    return out


def sum_error(got, want, scale):
    """per variable: max |got - want| / max scale (0 where a variable has no term at all and got is 0 too)"""
    want, scale = np.asarray(want, np.float64), np.asarray(scale, np.float64)
    d = np.max(np.abs(_f64(got, *want.shape) - want), axis=1)
    den = np.max(scale, axis=1)
    return np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d == 0, 0.0, np.inf))


def ldl_pivots(lambda_f32, width):
    """The un-pivoted LDL^T pivots of float32 matrices (N x width x width, any shape that holds them), computed in float64 from the
    LOWER triangle alone, as inv6x6 reads it (D(j,j) = A(j,j) - sum_k L(j,k)^2 D(k,k); L(i,j) = (A(i,j) - sum_k L(i,k) L(j,k) D(k,k)) /
    D(j,j), i > j).  Returns (pivots (N, width), scales (N, width)): a scale is |A(j,j)| + sum_k |L(j,k)^2 D(k,k)|, what a pivot's
    distance from zero is relative to."""
    A = _f64(lambda_f32, -1, width, width)
    N = A.shape[0]
    Lm, D, S = np.zeros((N, width, width)), np.zeros((N, width)), np.zeros((N, width))
    with np.errstate(all="ignore"):
        for j in range(width):
            d, s = A[:, j, j].copy(), np.abs(A[:, j, j])
            for k in range(j):
                t = Lm[:, j, k] * Lm[:, j, k] * D[:, k]
                d -= t
                s += np.abs(t)
            D[:, j], S[:, j] = d, s
            for i in range(j + 1, width):
                v = A[:, i, j].copy()
                for k in range(j):
                    v -= Lm[:, i, k] * Lm[:, j, k] * D[:, k]
                Lm[:, i, j] = v / d
    return D, S


def positive_definite(lambda_f32, width):
    """per matrix: every LDL^T pivot > 0 (a NaN pivot is not)"""
    with np.errstate(invalid="ignore"):
        return np.all(ldl_pivots(lambda_f32, width)[0] > 0.0, axis=1)


def pivot_solve(A, b):
    """x of A x = b by Gaussian elimination with partial pivoting in float64, written out (numpy's solve() refuses a singular matrix and
    leaves open what it does with a non-finite one): the pivot of column k is the first row of the largest |entry| among rows k.. (a NaN
    never compares larger), then plain elimination and back substitution.  Whatever is non-finite stays in the arithmetic."""
    M = np.concatenate([np.array(A, np.float64), np.array(b, np.float64)[:, None]], axis=1)
    n = M.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n):
            piv, best = k, abs(M[k, k])
            for i in range(k + 1, n):
                if abs(M[i, k]) > best:
                    piv, best = i, abs(M[i, k])
            if piv != k:
                M[[k, piv]] = M[[piv, k]]
            for i in range(k + 1, n):
                f = M[i, k] / M[k, k]
                M[i, k:] -= f * M[k, k:]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = (M[i, n] - M[i, i + 1:n] @ x[i + 1:]) / M[i, i]
    return x


def nonfinite_means(eta, lam, width):
    """per variable: is the mean of the float32 belief, solved in float64 (pivot_solve) and rounded to float32, non-finite?"""
    e, lm = _f64(eta, -1, width), _f64(lam, -1, width, width)
    with np.errstate(all="ignore"):
        return np.array([not np.all(np.isfinite(pivot_solve(lm[v], e[v]).astype(np.float32))) for v in range(e.shape[0])], bool)
