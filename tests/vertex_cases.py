"""Deterministic generator of VERTEX CASES and the CPU driver that runs them (shared by tests/test_oracle_vertices.py,
tests/test_gpu_vertices.py, tests/test_gpu_device_math.py and tests/golden/make_golden.py).

A case is one factor's complete vertex input under the reference's tensor names (ba/gbp_codelets.cpp): beliefs of its camera and
landmark, previous messages, factor potential, measurement, K, variance, oldmu, damping, damping_count, active flag, the robust
flag it enters with and the hyper-parameters.  Cases are rows of ONE float32 array in the layout of the device hook
gbp_debug_vertex (include/gbp_mi355x_debug.h; integers as their bit patterns), outputs rows of the hook's output layout, so the
same arrays go to the reference's vertices (rv_*), to the restatement (orc_vertex_*) and to the GPU.

Groups (GROUPS): harvested (restatement-oracle runs of the three sequences, three parameter sets), boundaries (count, dmu, err,
inactive, relin_reset), conditioning, geometry, nonfinite.  Potentials are kept in the form the program produces and the device
stores: Lambda_cc / Lambda_ll bit-symmetric, Lambda_lc = Lambda_cl^T.

Nothing here reads the reference: the generator uses the restatement's dense-math layer (pinned bit for bit to the reference's,
tests/test_oracle_math.py) to place the boundaries; that each boundary is really hit is asserted against the reference's
vertices in tests/test_oracle_vertices.py.
"""
import ctypes as C
import functools
import os

import numpy as np

from gbp_poplar_amd import _cabi as cabi
from gbp_poplar_amd import driver
from oracle import oracle as orc
from tests.oracle_host import OracleHost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- record layouts (== hooks/gbp_debug_vertex.hip) ------------------------------------------------------------------------
IN_FIELDS = (("K", 9), ("z", 2), ("var", 1), ("cbe", 6), ("cbl", 36), ("lbe", 3), ("lbl", 9), ("fe", 9), ("fl", 81), ("pce", 6),
             ("pcl", 36), ("ple", 3), ("pll", 9), ("oldmu", 9), ("damping", 1), ("count", 1), ("active", 1), ("robust", 1),
             ("maxeta", 1), ("nund", 1), ("thr", 1), ("minlin", 1), ("nstds", 1), ("relin_mode", 1))
OUT_FIELDS = (("fe", 9), ("fl", 81), ("mce", 6), ("mcl", 36), ("mle", 3), ("mll", 9), ("mu", 9), ("dmu", 1), ("damping", 1),
              ("count", 1), ("robust", 1))
INT_FIELDS = {"count": np.int32, "active": np.uint32, "robust": np.uint32, "nund": np.int32, "minlin": np.int32, "relin_mode": np.int32}


def _offsets(fields):
    off, o = {}, 0
    for k, w in fields:
        off[k] = (o, w)
        o += w
    return off, o


IN_OFF, W_IN = _offsets(IN_FIELDS)
OUT_OFF, W_OUT = _offsets(OUT_FIELDS)
assert (W_IN, W_OUT) == (229, 157)
OP0_FIELDS = ("fe", "fl", "robust")       # what RelineariseFactorVertex (op 0) writes

GROUPS = ("harvested", "count", "dmu", "err", "inactive", "relin_reset", "conditioning", "geometry", "nonfinite")
GID = {g: i for i, g in enumerate(GROUPS)}

# parameter sets (maxeta_damping, num_undamped_iters, dmu_threshold, min_linear_iters, nstds): the reference's and two others
PARAMS = ((0.4, 8, 3e-3, 10, 2.5), (0.7, 4, 1e-2, 6, 1.5), (0.1, 12, 1e-3, 14, 4.0))
SEQUENCES = ("fr2robot2", "fr1xyz", "fr1desk")
HARVEST_SWEEPS = (0, 1, 2, 17, 18, 19, 100)
HARVEST_PER_SNAPSHOT = 256


def field(A, name, out=False):
    """View of one field of an input (or output) array; integer fields as integers."""
    o, w = (OUT_OFF if out else IN_OFF)[name]
    v = A[:, o:o + w]
    return v.view(INT_FIELDS[name]) if name in INT_FIELDS else v


def blank(n):
    X = np.zeros((n, W_IN), np.float32)
    set_params(X, PARAMS[0])
    return X


def set_params(X, prm, rows=slice(None)):
    field(X, "maxeta")[rows] = prm[0]
    field(X, "nund")[rows] = prm[1]
    field(X, "thr")[rows] = prm[2]
    field(X, "minlin")[rows] = prm[3]
    field(X, "nstds")[rows] = prm[4]


# ---- the CPU driver: one set of calls for rv_* and orc_vertex_* --------------------------------------------------------------

def run_cpu(api, X, op):
    """Run every case of X through the vertex classes of `api` (oracle.vertex_api): op 0 RelineariseFactorVertex, op 1
    PrepMessageVertex followed by the four message vertices (program order of ba.cpp:895-905).  Returns the outputs in the hook's
    layout (mu starts as oldmu, dmu as 0: what the program holds between sweeps)."""
    X = np.ascontiguousarray(X, np.float32)
    n = X.shape[0]
    Y = np.zeros((n, W_OUT), np.float32)
    if op != 0:
        field(Y, "fe", True)[:] = field(X, "fe")
        field(Y, "fl", True)[:] = field(X, "fl")
        field(Y, "mu", True)[:] = field(X, "oldmu")
        field(Y, "damping", True)[:] = field(X, "damping")
        field(Y, "count", True)[:] = field(X, "count")
    field(Y, "robust", True)[:] = field(X, "robust")
    xb, yb = X.ctypes.data, Y.ctypes.data
    xi = {k: o * 4 for k, (o, _) in IN_OFF.items()}
    yo = {k: o * 4 for k, (o, _) in OUT_OFF.items()}
    var, active = field(X, "var")[:, 0], field(X, "active")[:, 0]
    hyper = np.concatenate([field(X, k).astype(np.float64) for k in ("maxeta", "nund", "thr", "minlin", "nstds")], axis=1)
    thr32, maxeta32, nstds32 = field(X, "thr")[:, 0], field(X, "maxeta")[:, 0], field(X, "nstds")[:, 0]
    relin_mode = field(X, "relin_mode")[:, 0]
    damp_out = field(Y, "damping", True)[:, 0]
    last = None
    for i in range(n):
        x, y = xb + i * W_IN * 4, yb + i * W_OUT * 4
        key = (hyper[i].tobytes(), int(relin_mode[i]))
        if key != last:
            api.set_hyper(float(maxeta32[i]), int(hyper[i, 1]), float(thr32[i]), int(hyper[i, 3]), float(nstds32[i]))
            if api.set_relin_mode is not None:
                api.set_relin_mode(int(relin_mode[i]))
            elif relin_mode[i] != 0:
                raise ValueError("the reference has no relin_mode 1")
            last = key
        fe, cc = y + yo["fe"], y + yo["fl"]
        cl, lc, ll = cc + 36 * 4, cc + 54 * 4, cc + 72 * 4
        bel = (x + xi["cbe"], x + xi["cbl"], x + xi["lbe"], x + xi["lbl"])
        if op == 0:
            api.relinearise_factor(x + xi["z"], float(var[i]), x + xi["K"], *bel, fe, cc, ll, cl, lc, y + yo["robust"])
            continue
        a = int(active[i])
        api.prep_message(y + yo["damping"], y + yo["count"], a, y + yo["robust"], x + xi["z"], x + xi["K"], float(var[i]), *bel,
                         x + xi["oldmu"], y + yo["mu"], y + yo["dmu"], fe, cc, ll, cl, lc)
        d = float(damp_out[i])
        pce, pcl, ple, pll = x + xi["pce"], x + xi["pcl"], x + xi["ple"], x + xi["pll"]
        api.cam_message_eta(d, a, fe, fe + 24, ll, cl, bel[2], bel[3], ple, pll, pce, y + yo["mce"])
        api.lmk_message_eta(d, a, fe + 24, fe, cc, lc, bel[0], bel[1], pce, pcl, ple, y + yo["mle"])
        api.cam_message_lambda(a, cc, ll, cl, lc, bel[3], pll, y + yo["mcl"])
        api.lmk_message_lambda(a, ll, cc, lc, cl, bel[1], pcl, y + yo["mll"])
    return Y


def relinearised(X, Y):
    """The cases whose PrepMessageVertex relinearised: count was reset to -num_undamped_iters.  (A count that merely steps onto
    that value, count + 1 == -num_undamped_iters < 0, is no reset — and cannot be one: the test needs count + 1 > min_linear_iters -
    num_undamped_iters, which is positive in every parameter set here.)"""
    cin, cout, nund = field(X, "count")[:, 0], field(Y, "count", True)[:, 0], field(X, "nund")[:, 0]
    return (cout == -nund) & (cin + 1 != -nund) & (field(X, "active")[:, 0] == 1)


def finite_rows(Y):
    return np.isfinite(Y[:, :OUT_OFF["count"][0]]).all(axis=1)


# ---- helpers over the restatement's math layer ------------------------------------------------------------------------------

def _lib():
    return orc.load("restatement")


def means(X):
    """Belief means of every case (inf2mean6x6 / inf2mean3x3 of the restatement's math layer: trig-free)."""
    lib, P = _lib(), lambda a: cabi.ptr(a, cabi.c_f32p)
    n = X.shape[0]
    m = np.zeros((n, 9), np.float32)
    for i in range(n):
        c, l = np.zeros(6, np.float32), np.zeros(3, np.float32)
        lib.om_inf2mean6x6(P(np.ascontiguousarray(field(X, "cbe")[i])), P(np.ascontiguousarray(field(X, "cbl")[i])), P(c))
        lib.om_inf2mean3x3(P(np.ascontiguousarray(field(X, "lbe")[i])), P(np.ascontiguousarray(field(X, "lbl")[i])), P(l))
        m[i, :6], m[i, 6:] = c, l
    return m


def dmu_of(oldmu, mu):
    """dmu as PrepMessageVertex accumulates it (gbp_codelets.cpp:268-277): fp32, element by element."""
    d = np.zeros(oldmu.shape[0], np.float32)
    for k in range(9):
        t = (oldmu[:, k] - mu[:, k]).astype(np.float32)
        d = (d + (t * t).astype(np.float32)).astype(np.float32)
    return np.sqrt(d).astype(np.float32)


def err_of(X, mu, trig):
    """The Huber residual norm of gbp_codelets.cpp:135 at the linearisation point mu, in trig mode `trig`."""
    lib, P = _lib(), lambda a: cabi.ptr(a, cabi.c_f32p)
    n = X.shape[0]
    hx = np.zeros((n, 2), np.float32)
    orc.set_trig_mode(trig)
    try:
        for i in range(n):
            lib.om_hfunc(P(np.ascontiguousarray(mu[i, :6])), P(np.ascontiguousarray(mu[i, 6:])), P(np.ascontiguousarray(field(X, "K")[i])), P(hx[i]))
    finally:
        orc.set_trig_mode(0)
    z = field(X, "z")
    with np.errstate(all="ignore"):
        a, b = (hx[:, 0] - z[:, 0]).astype(np.float32), (hx[:, 1] - z[:, 1]).astype(np.float32)
        return np.sqrt(((a * a).astype(np.float32) + (b * b).astype(np.float32)).astype(np.float32)).astype(np.float32)


def schur_pivots(X):
    """fp64 un-pivoted LDL^T pivots of the two Schur blocks (Lambda_f + Lambda_belief - Lambda_prev_msg, formed in fp32 as the
    vertices form them): (n, 3) for the camera messages' 3x3 block, (n, 6) for the landmark messages' 6x6 block."""
    fl = field(X, "fl")
    with np.errstate(all="ignore"):
        B3 = ((fl[:, 72:81] + field(X, "lbl")).astype(np.float32) - field(X, "pll")).astype(np.float32).reshape(-1, 3, 3)
        B6 = ((fl[:, :36] + field(X, "cbl")).astype(np.float32) - field(X, "pcl")).astype(np.float32).reshape(-1, 6, 6)

    def piv(A):
        n = A.shape[1]
        out = np.zeros((A.shape[0], n))
        for c in range(A.shape[0]):
            M = np.tril(A[c].astype(np.float64))
            M = M + np.tril(M, -1).T
            Lm, D = np.eye(n), np.zeros(n)
            with np.errstate(all="ignore"):
                for j in range(n):
                    D[j] = M[j, j] - np.sum(Lm[j, :j] ** 2 * D[:j])
                    for i in range(j + 1, n):
                        Lm[i, j] = (M[i, j] - np.sum(Lm[i, :j] * Lm[j, :j] * D[:j])) / D[j]
            out[c] = D
        return out
    return piv(B3), piv(B6)


# ---- harvested -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def harvested():
    """Per-factor inputs of real sweeps: the restatement oracle (correctly rounded trig, so the inputs do not depend on the
    host's libm) on the three sequences under the three parameter sets, the state in front of sweeps HARVEST_SWEEPS."""
    host = OracleHost("restatement")
    rows = []
    orc.set_trig_mode(1)
    try:
        for si, name in enumerate(SEQUENCES):
            bal = host.bal_read(os.path.join(ROOT, "data", "sequences", name + ".txt"))
            K, state, _ = driver.build_inputs(bal, driver.Options(), host)
            cam, lmk, E = np.asarray(bal["cam_id"]), np.asarray(bal["lmk_id"]), int(bal["n_edges"])
            for pi, prm in enumerate(PARAMS):
                params = cabi.GbpParams.defaults(maxeta_damping=prm[0], num_undamped_iters=prm[1], dmu_threshold=prm[2],
                                                 min_linear_iters=prm[3], nstds=prm[4])
                o = orc.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=params)
                o.upload(state)
                o.linearise()
                rng = np.random.default_rng(1000 + 10 * si + pi)
                for it in range(max(HARVEST_SWEEPS) + 1):
                    if (it + 1) % 2 == 0 and it < 10:
                        o.weaken_priors()
                    if it in HARVEST_SWEEPS:
                        ids = np.sort(rng.choice(E, HARVEST_PER_SNAPSHOT, replace=False))
                        r, m = o.read(), o.messages()
                        fe, fl = o.factor_potentials()
                        mu, _ = o.mu()
                        X = blank(len(ids))
                        set_params(X, prm)
                        field(X, "K")[:] = np.asarray(K, np.float32)
                        field(X, "z")[:] = state["measurements"].reshape(-1, 2)[ids]
                        field(X, "var")[:, 0] = state["meas_variances"][ids]
                        field(X, "cbe")[:] = r["cam_beliefs_eta"].reshape(-1, 6)[cam[ids]]
                        field(X, "cbl")[:] = r["cam_beliefs_lambda"].reshape(-1, 36)[cam[ids]]
                        field(X, "lbe")[:] = r["lmk_beliefs_eta"].reshape(-1, 3)[lmk[ids]]
                        field(X, "lbl")[:] = r["lmk_beliefs_lambda"].reshape(-1, 9)[lmk[ids]]
                        field(X, "fe")[:] = fe.reshape(-1, 9)[ids]
                        field(X, "fl")[:] = fl.reshape(-1, 81)[ids]
                        field(X, "pce")[:] = m["cam_eta"].reshape(-1, 6)[ids]
                        field(X, "pcl")[:] = m["cam_lambda"].reshape(-1, 36)[ids]
                        field(X, "ple")[:] = m["lmk_eta"].reshape(-1, 3)[ids]
                        field(X, "pll")[:] = m["lmk_lambda"].reshape(-1, 9)[ids]
                        field(X, "oldmu")[:] = mu.reshape(-1, 9)[ids]
                        field(X, "damping")[:, 0] = r["damping"][ids]
                        field(X, "count")[:, 0] = r["damping_count"][ids]
                        field(X, "active")[:, 0] = state["active_flag"][ids]
                        field(X, "robust")[:, 0] = r["robust_flag"][ids]
                        rows.append(X)
                    o.iterate(1)
                o.close()
    finally:
        orc.set_trig_mode(0)
    X = np.concatenate(rows)
    X.setflags(write=False)
    return X


def _late(H):
    """harvested cases with a history (non-zero previous messages and oldmu): sweeps >= 17"""
    return H[(np.abs(field(H, "pll")).sum(axis=1) > 0) & (np.abs(field(H, "oldmu")).sum(axis=1) > 0)]


# ---- boundaries ----------------------------------------------------------------------------------------------------------

def _boundary_count(H, rng):
    """damping_count in {-1, 0, m - 2 .. m + 1}, m = min_linear_iters - num_undamped_iters (the test is count + 1 > m), once
    with dmu = 0 (oldmu = the belief means: only the count decides) and once with the harvested, larger dmu."""
    rows = []
    for prm in PARAMS:
        m = prm[3] - prm[1]
        base = _late(H)[rng.choice(len(_late(H)), 12, replace=False)].copy()
        set_params(base, prm)
        mu = means(base)
        for cnt in (-1, 0, m - 2, m - 1, m, m + 1):
            for still in (True, False):
                X = base.copy()
                field(X, "count")[:] = cnt
                field(X, "damping")[:] = 0.25
                if still:
                    field(X, "oldmu")[:] = mu
                else:
                    field(X, "oldmu")[:] = mu + np.float32(0.5)
                rows.append(X)
    return np.concatenate(rows)


def _boundary_dmu(H, rng):
    """dmu_threshold one ulp below / equal to / one ulp above the dmu the case produces (count large: only dmu decides)."""
    rows = []
    base = _late(H)[rng.choice(len(_late(H)), 60, replace=False)].copy()
    field(base, "count")[:] = 50
    d = dmu_of(field(base, "oldmu"), means(base))
    keep = np.isfinite(d) & (d > 0)
    base, d = base[keep], d[keep]
    for thr in (np.nextafter(d, np.float32(0)), d, np.nextafter(d, np.float32(np.inf))):
        X = base.copy()
        field(X, "thr")[:, 0] = thr
        rows.append(X)
    return np.concatenate(rows)


def _boundary_err(H, rng):
    """Nstds * sqrt(var) one ulp below / equal to / one ulp above the residual norm of a relinearising case.  var is 1 or 4, so
    sqrt(var) and the product are exact and Nstds places the threshold; cases whose residual differs between the two trig
    conventions (libm / correctly rounded) are left out, so that the boundary is the same one for the reference and the device."""
    rows = []
    base = H[rng.choice(len(H), 160, replace=False)].copy()
    mu = means(base)
    field(base, "oldmu")[:] = mu
    field(base, "count")[:] = 50
    e0, e1 = err_of(base, mu, 0), err_of(base, mu, 1)
    keep = (e0 == e1) & np.isfinite(e0) & (e0 > 0)
    base, err = base[keep][:96], e0[keep][:96]
    for var, s in ((1.0, 1.0), (4.0, 2.0)):
        for nst in (np.nextafter(err, np.float32(0)), err, np.nextafter(err, np.float32(np.inf))):
            X = base.copy()
            field(X, "var")[:] = var
            field(X, "nstds")[:, 0] = (nst / np.float32(s)).astype(np.float32)
            rows.append(X)
    return np.concatenate(rows)


def _inactive(H, rng):
    """inactive factors with non-zero old messages, potentials and damping state: everything but the messages must stay"""
    X = _late(H)[rng.choice(len(_late(H)), 48, replace=False)].copy()
    field(X, "active")[:] = 0
    field(X, "count")[:, 0] = np.resize(np.array([-1, 0, 1, 3, 50], np.int32), len(X))
    return X


def _relin_reset(H, rng):
    """relin_mode 1 (ours: zero the potential before relinearising) on cases that relinearise and cases that do not"""
    X = _late(H)[rng.choice(len(_late(H)), 64, replace=False)].copy()
    field(X, "relin_mode")[:] = 1
    field(X, "count")[:] = 50
    mu = means(X)
    half = len(X) // 2
    field(X, "oldmu")[:half] = mu[:half]
    return X


# ---- conditioning --------------------------------------------------------------------------------------------------------

def _sym_with_spectrum(rng, d):
    q, _ = np.linalg.qr(rng.standard_normal((len(d), len(d))))
    return q @ np.diag(d) @ q.T


def _conditioning(H, rng):
    """Schur blocks Lambda_f + Lambda_belief - Lambda_prev_msg with chosen spectra (indefinite, negative definite, one tiny
    pivot, positive), beliefs rescaled so that their largest Lambda entry spans 1e-6 .. 1e8 (the cofactor determinant of inv3x3 is
    a cubic in the entries: fp32 overflows beyond ~7e12), large and out-of-range damping.  The previous messages carry the
    construction (they enter nothing but the Schur blocks and the eta sums), so the belief means stay those of a real sweep."""
    late = _late(H)
    n = 400
    X = late[rng.choice(len(late), n, replace=True)].copy()
    field(X, "count")[:] = 3                      # non-zero, and dmu (harvested oldmu + noise below) is far above the threshold
    field(X, "oldmu")[:] += rng.standard_normal((n, 9)).astype(np.float32)
    field(X, "damping")[:, 0] = np.resize(np.array([0.0, 0.4, 0.9, 0.999, 1.0, 2.0, -0.5], np.float32), n)
    spectra3 = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (1, 1, 1e-6), (1, 0.5, 0.25), (1, -1e-5, 1))
    spectra6 = ((1, 1, 1, 1, 1, -1), (1, -1, 1, -1, 1, -1), (-1,) * 6, (1, 1, 1, 1, 1, 1e-6), (1, .8, .6, .4, .2, .1), (1, 1, -1e-5, 1, 1, 1))
    for i in range(n):
        sc, sl = 10.0 ** rng.uniform(-6, 8), 10.0 ** rng.uniform(-6, 8)
        for eta, lam, s in (("cbe", "cbl", sc), ("lbe", "lbl", sl)):
            f = np.float32(s / np.max(np.abs(field(X, lam)[i])))
            field(X, eta)[i] *= f
            field(X, lam)[i] *= f
        fl = field(X, "fl")[i].astype(np.float64)
        lbl, cbl = field(X, "lbl")[i].astype(np.float64).reshape(3, 3), field(X, "cbl")[i].astype(np.float64).reshape(6, 6)
        ll, cc = fl[72:81].reshape(3, 3), fl[:36].reshape(6, 6)
        m3 = max(np.max(np.abs(ll)), np.max(np.abs(lbl)))
        m6 = max(np.max(np.abs(cc)), np.max(np.abs(cbl)))
        T3 = _sym_with_spectrum(rng, m3 * np.array(spectra3[i % 6]) * rng.uniform(0.5, 2.0, 3))
        T6 = _sym_with_spectrum(rng, m6 * np.array(spectra6[(i // 6) % 6]) * rng.uniform(0.5, 2.0, 6))
        p3, p6 = ll + lbl - T3, cc + cbl - T6
        field(X, "pll")[i] = (0.5 * (p3 + p3.T)).astype(np.float32).ravel()
        field(X, "pcl")[i] = (0.5 * (p6 + p6.T)).astype(np.float32).ravel()
    return X


# ---- geometry --------------------------------------------------------------------------------------------------------------

def _rodrigues(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th <= 1e-6:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def _posed(base, rng, w, lmk, depth, view, K, z_off, lam_c=4.0, lam_l=2.0):
    """One relinearising case whose linearisation point is EXACTLY (t, w | lmk): the beliefs are (power of two) x identity, so
    inf2mean returns eta / lambda without rounding.  t puts the point at camera-frame depth `depth` and at `view` x depth
    sideways; the measurement sits z_off pixels from the projection."""
    X = base.copy()
    w, lmk = np.asarray(w, np.float32), np.asarray(lmk, np.float32)
    Rl = _rodrigues(w.astype(np.float64)) @ lmk.astype(np.float64)
    t = np.array([view[0] * depth - Rl[0], view[1] * depth - Rl[1], depth - Rl[2]]).astype(np.float32)
    x = np.concatenate([t, w]).astype(np.float32)
    field(X, "K")[0] = K
    field(X, "cbl")[0] = (np.float32(lam_c) * np.eye(6, dtype=np.float32)).ravel()
    field(X, "cbe")[0] = x * np.float32(lam_c)
    field(X, "lbl")[0] = (np.float32(lam_l) * np.eye(3, dtype=np.float32)).ravel()
    field(X, "lbe")[0] = lmk * np.float32(lam_l)
    field(X, "oldmu")[0] = np.concatenate([x, lmk])
    field(X, "count")[0] = 50
    field(X, "active")[0] = 1
    with np.errstate(all="ignore"):
        yc = Rl + t.astype(np.float64)
        hx = np.array([K[0] * yc[0] / yc[2] + K[2], K[4] * yc[1] / yc[2] + K[5]])
        field(X, "z")[0] = np.nan_to_num(hx, nan=100.0, posinf=1e6, neginf=-1e6) + np.asarray(z_off)
    return X


K_SQUARE = np.array([520.9, 0, 325.1, 0, 521.0, 249.7, 0, 0, 1], np.float32)
K_WIDE = np.array([731.25, 0, 401.5, 0, 260.5, 133.0, 0, 0, 1], np.float32)
K_SHORT = np.array([32.0, 0, 20.5, 0, 24.0, 15.25, 0, 0, 1], np.float32)


def _geometry(H, rng):
    """|w| from 2e-6 (just above the identity branch of so3exp) to 6 rad, camera-frame depth from 1e-3 to 1e3 and negative
    (behind the camera), points far off the optical axis, measurements far from the projection (large err), non-square K.
    At |depth| = 1e-3 the focal length is short (K_SHORT): the potential's entries are of order (f / depth)^2 / var and the
    cofactor determinant of the message vertices' 3x3 block is a cubic in them — with f = 521 that is 1e36 and more, past
    fp32, whatever the implementation; with f = 32 the same depth stays in range."""
    late = _late(H)
    rows = []
    mags = (2e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.7, 1.5, 3.0, 3.1415925, 3.1415927, 4.5, 6.0)
    depths = (1e-3, 1e-2, 0.1, 1.0, 4.0, 30.0, 1e3, -1e-3, -0.1, -4.0, -1e3)
    for mag in mags:
        for depth in depths:
            for rep in range(3):
                base = late[rng.integers(len(late))][None, :].copy()
                d = rng.standard_normal(3)
                w = d / np.linalg.norm(d) * mag
                view = rng.uniform(-1, 1, 2) * (1.0 if rep < 2 else 8.0)
                z_off = rng.choice([-1.0, 1.0], 2) * (0.3, 3.0, 1e3)[rep] * rng.uniform(0.5, 1.5, 2)
                rows.append(_posed(base, rng, w, rng.standard_normal(3) * 2.0, depth, view,
                                   K_SHORT if abs(depth) < 5e-3 else K_WIDE if rep == 1 else K_SQUARE, z_off))
    return np.concatenate(rows)


def _nonfinite(H, rng):
    """Non-finite BY CONSTRUCTION (a short, counted list): w = 0 (the Jacobian divides by |w|^2 = 0), camera-frame depth exactly
    0 (identity branch of so3exp, so the depth is exact), the all-zero belief of a camera without prior or factors (1 / 0 in its
    mean), an exactly singular 3x3 Schur block."""
    late = _late(H)
    rows = []
    for rep in range(4):
        base = late[rng.integers(len(late))][None, :].copy()
        lmk = rng.standard_normal(3) * 2.0
        rows.append(_posed(base, rng, (0.0, 0.0, 0.0), lmk, 4.0, (0.2, -0.1), K_SQUARE, (1.0, 1.0)))
        X = _posed(base, rng, (5e-7, 0.0, 0.0), (lmk[0], lmk[1], 1.0), 1.0, (0.0, 0.0), K_SQUARE, (1.0, 1.0))
        field(X, "cbe")[0, 2] = np.float32(-1.0) * field(X, "cbl")[0, 0]      # t_z = -1, l_z = 1, R = I: depth exactly 0
        field(X, "oldmu")[0, 2] = -1.0
        rows.append(X)
        X = base.copy()
        field(X, "cbe")[:] = 0
        field(X, "cbl")[:] = 0
        rows.append(X)
        X = base.copy()
        field(X, "count")[:] = 3
        field(X, "oldmu")[:] += np.float32(1.0)
        field(X, "fl")[0, 72:81] = 4.0
        field(X, "lbl")[:] = 0
        field(X, "pll")[:] = 0
        rows.append(X)
    return np.concatenate(rows)


# ---- the whole set --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_cases():
    """(X [n][229] float32, group [n] uint8): every group, in a fixed order."""
    H = harvested()
    rng = np.random.default_rng(20240611)
    parts = [("harvested", np.array(H)), ("count", _boundary_count(H, rng)), ("dmu", _boundary_dmu(H, rng)),
             ("err", _boundary_err(H, rng)), ("inactive", _inactive(H, rng)), ("relin_reset", _relin_reset(H, rng)),
             ("conditioning", _conditioning(H, rng)), ("geometry", _geometry(H, rng)), ("nonfinite", _nonfinite(H, rng))]
    X = np.ascontiguousarray(np.concatenate([p for _, p in parts]), np.float32)
    g = np.concatenate([np.full(len(p), GID[k], np.uint8) for k, p in parts])
    X.setflags(write=False)
    g.setflags(write=False)
    return X, g


def golden_subset(group, per_group=16):
    """Indices of the committed sub-sample: evenly spaced cases of every group (that takes every third of the dmu and err
    groups: below, on and above the boundary).  The count group is laid out [parameter set][count][dmu = 0, large][12 bases]; its
    share is, for every parameter set, the two counts next to the test (count + 1 == m and m + 1, dmu = 0) twice and count 0,
    plus one case with a large dmu."""
    idx = []
    for gi in range(len(GROUPS)):
        w = np.nonzero(group == gi)[0]
        if GROUPS[gi] == "count":
            at = lambda p, c, s, b: ((p * 6 + c) * 2 + s) * 12 + b
            pick = [at(p, c, 0, b) for p in range(len(PARAMS)) for c in (3, 4) for b in (0, 1)]
            pick += [at(p, 1, 0, 0) for p in range(len(PARAMS))] + [at(0, 4, 1, 0)]
            idx.append(w[np.sort(np.array(pick))])
            continue
        idx.append(w[np.unique(np.linspace(0, len(w) - 1, min(per_group, len(w))).astype(int))])
    return np.concatenate(idx)


def weaken_cases():
    """WeakenPriorVertex: weaken_flag 0 .. 7 and a huge one, several scalings, camera- and landmark-sized priors."""
    rng = np.random.default_rng(99)
    flags = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0xffffffff], np.uint32)
    scal = np.array([0.5, 0.9440609, 1.0, 1e-3, 0.0, 1.25], np.float32)
    f, s = np.meshgrid(flags, scal, indexing="ij")
    n = f.size
    return {"flag": f.ravel().copy(), "scaling": s.ravel().copy(), "eta": rng.standard_normal((n, 6)).astype(np.float32),
            "lam": (rng.standard_normal((n, 36)) * 100).astype(np.float32)}


def run_weaken(api, W):
    out = {k: v.copy() for k, v in W.items()}
    for i in range(len(W["flag"])):
        ne, nl = (6, 36) if i % 2 == 0 else (3, 9)
        api.weaken_prior(float(W["scaling"][i]), out["flag"][i:].ctypes.data, out["eta"][i].ctypes.data, ne, out["lam"][i].ctypes.data, nl)
    return out


def wide_math_inputs():
    """Inputs of the device math ops (gbp_debug_math) from the conditioning / geometry groups: 3x3 and 6x6 Schur blocks (ops 0, 1),
    linearisation points (op 3), beliefs (ops 7, 8)."""
    X, g = all_cases()
    sel = X[(g == GID["conditioning"]) | (g == GID["geometry"])]
    fl = field(sel, "fl")
    with np.errstate(all="ignore"):
        B3 = ((fl[:, 72:81] + field(sel, "lbl")).astype(np.float32) - field(sel, "pll")).astype(np.float32)
        B6 = ((fl[:, :36] + field(sel, "cbl")).astype(np.float32) - field(sel, "pcl")).astype(np.float32)
    geo = X[g == GID["geometry"]]
    lin = np.concatenate([field(geo, "oldmu"), field(geo, "K")], axis=1)
    return {"inv3": np.ascontiguousarray(B3), "inv6": np.ascontiguousarray(B6), "lin": np.ascontiguousarray(lin),
            "mean6": np.ascontiguousarray(np.concatenate([field(sel, "cbe"), field(sel, "cbl")], axis=1)),
            "mean3": np.ascontiguousarray(np.concatenate([field(sel, "lbe"), field(sel, "lbl")], axis=1))}
