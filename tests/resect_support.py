"""What tests/test_resect_cpu.py and tests/test_gpu_resect.py share: the host twin of the resection arithmetic
(tests/sanitize/resect_math_main.cpp, a stand-alone program: compiled here, run as a process, never loaded into python), its file format,
an INDEPENDENT numpy implementation of the definition in include/gbp_mi355x_resect.h, parametrised by dtype, and the graphs the case
families are made of.

The numpy implementation follows the header's text, not the C++: matrices, einsum and closed-form derivatives in place of unrolled loops,
np.sum over each partial's entries, np.linalg.solve for the step.  Its float32 run against its float64 run measures what float32 costs on
a family; the tests allow the code under test 8 x that (the project's convention):
    pose     max over cameras of max |x - x64| / max |x64|
"""
import os

import numpy as np

from tests import host_twin
from tests.seed_support import K_SYNTH, _hat, _rotation, project64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "sanitize", "resect_math_main.cpp")
NO_VIEW, BEHIND, NONFINITE, BAD_INDEX, FEW_VIEWS, STALLED = 1, 8, 16, 32, 64, 128
DEFAULTS = {"max_passes": 10, "min_views": 6, "huber_px": 5.0, "lambda0": 1e-3, "reproj_meas_var": 4.0}
OUTPUTS = (("cam_mean", 6, np.float32), ("cam_priors_eta", 6, np.float32), ("cam_info", 36, np.float32), ("report", 4, np.float32),
           ("status", 1, np.uint32), ("n_views", 1, np.uint32))


def compile_host(exe, sanitize):
    return host_twin.compile_host(MAIN, exe, sanitize)


def index_numpy(cam_id, n_cams):
    """the camera-major index by a stable argsort"""
    cam_id = np.asarray(cam_id, np.int64)
    start = np.zeros(n_cams + 1, np.uint32)
    start[1:] = np.cumsum(np.bincount(cam_id, minlength=n_cams))
    return start, np.argsort(cam_id, kind="stable").astype(np.uint32)


def initial_outputs(start_poses, seed=7):
    """what the output arrays hold before a call: the start poses in cam_mean, recognisable values elsewhere ('not touched' can be seen)"""
    rng = np.random.default_rng(seed)
    C = np.asarray(start_poses).size // 6
    out = {k: (rng.integers(1 << 20, 1 << 21, w * C).astype(np.uint32) if dt is np.uint32 else
               rng.uniform(1000.0, 2000.0, w * C).astype(np.float32)) for k, w, dt in OUTPUTS}
    out["cam_mean"] = np.ascontiguousarray(start_poses, np.float32).ravel().copy()
    return out


def graph_of(n_cams, n_lmks, cam_id, lmk_id, K, cam_mean, lmk_mean, measurements, active_flag=None, lmk_use=None, identity=False):
    """cam_mean: the START poses.  identity: the edges are sorted by camera and cam_edges is None (entry k is edge k)."""
    start, edges = index_numpy(cam_id, n_cams)
    if identity:
        assert np.array_equal(edges, np.arange(edges.size))
    return {"n_cams": int(n_cams), "n_lmks": int(n_lmks), "cam_id": np.asarray(cam_id, np.uint32), "lmk_id": np.asarray(lmk_id, np.uint32),
            "cam_start": start, "cam_edges": None if identity else edges, "K": np.asarray(K, np.float32),
            "cam_mean": np.asarray(cam_mean, np.float32).ravel(), "lmk_mean": np.asarray(lmk_mean, np.float32).ravel(),
            "measurements": np.asarray(measurements, np.float32).ravel(), "active_flag": active_flag, "lmk_use": lmk_use}


def run_host(exe, tmp, graph, opts=None, select=None, before=None, priors_lambda=None, trig="libm"):
    """-> dict of the six output arrays after the host program's run of `graph`.  before: what the outputs hold before (default
    initial_outputs of the graph's start poses).  priors_lambda None: no cam_priors_eta is written."""
    o = dict(DEFAULTS, **(opts or {}))
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    lmk_id = np.ascontiguousarray(graph["lmk_id"], np.uint32)
    E = lmk_id.size

    def opt(a, n):
        return np.zeros(n, np.uint32) if a is None else np.ascontiguousarray(a, np.uint32)

    has = (int(select is not None) | 2 * int(graph.get("cam_edges") is not None) | 4 * int(graph.get("active_flag") is not None) |
           8 * int(graph.get("lmk_use") is not None) | 16 * int(priors_lambda is not None))
    before = initial_outputs(graph["cam_mean"]) if before is None else before
    lam = np.zeros(36 * C, np.float32) if priors_lambda is None else np.ascontiguousarray(priors_lambda, np.float32).ravel()
    parts = [np.array([C, L, E, has], np.uint32), np.array([o["max_passes"], o["min_views"]], np.uint32),
             np.array([o["huber_px"], o["lambda0"], o["reproj_meas_var"]], np.float32), lmk_id, np.ascontiguousarray(graph["cam_start"], np.uint32),
             opt(graph.get("cam_edges"), E), np.ascontiguousarray(graph["K"], np.float32).ravel(), np.ascontiguousarray(graph["lmk_mean"], np.float32).ravel(),
             np.ascontiguousarray(graph["measurements"], np.float32).ravel(), opt(graph.get("active_flag"), E), opt(graph.get("lmk_use"), L),
             opt(select, C), lam] + [before[k] for k, _, _ in OUTPUTS]
    return host_twin.run(exe, tmp, "resect", parts, [(name, dt, w * C) for name, w, dt in OUTPUTS], trig, timeout=300)


# ---- the definition, in numpy, in one dtype ----
def _pass(x, lm, z, K, huber, T):
    """pass(x) over the used observations (lm [n, 3], z [n, 2]) -> cost, H [6, 6], g [6], behind, smallest |depth| / distance"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    w, n = x[3:], len(lm)
    th2 = np.sum(w * w, dtype=T)
    R = _rotation(w, T) if np.sqrt(th2) > 1e-6 else np.eye(3, dtype=T)
    N = ((R.T - np.eye(3, dtype=T)) @ _hat(w, T) + np.outer(w, w)).astype(T)
    yc = (lm @ R.T + x[:3]).astype(T)
    zc = yc[:, 2]
    hx = np.stack([fx * yc[:, 0] / zc + cx, fy * yc[:, 1] / zc + cy], axis=1).astype(T)
    Jp = np.zeros((n, 2, 3), T)
    Jp[:, 0, 0], Jp[:, 0, 2] = fx / zc, -fx * yc[:, 0] / (zc * zc)
    Jp[:, 1, 1], Jp[:, 1, 2] = fy / zc, -fy * yc[:, 1] / (zc * zc)
    Y = np.stack([_hat(v, T) for v in lm]) if n else np.zeros((0, 3, 3), T)
    dR = (-(np.einsum("ij,njk,kl->nil", R, Y, N).astype(T)) / th2).astype(T)
    J = np.concatenate([Jp, np.einsum("nij,njk->nik", Jp, dR).astype(T)], axis=2)
    r = (z - hx).astype(T)
    err = np.sqrt(np.sum(r * r, axis=1, dtype=T))
    plain = (err <= huber) if huber > 0 else np.ones(n, bool)
    wt = np.where(plain, T(1), T(huber) / err).astype(T)
    rho = np.where(plain, T(0.5) * err * err, T(huber) * (err - T(0.5) * T(huber))).astype(T)
    terms = np.concatenate([rho[:, None], (wt[:, None, None] * np.einsum("nki,nkj->nij", J, J)).reshape(n, 36),
                            wt[:, None] * np.einsum("nki,nk->ni", J, r)], axis=1).astype(T)
    # the sum order: partial j takes the entries j, j + 64, ...; the halving tree combines the 64 partials
    pad = (-n) % 64
    part = np.concatenate([terms, np.zeros((pad, 43), T)]).reshape(-1, 64, 43).sum(axis=0, dtype=T)
    while len(part) > 1:
        h = len(part) // 2
        part = (part[:h] + part[h:]).astype(T)
    s = part[0]
    ratio = np.min(np.abs(zc) / np.sqrt(np.sum(yc * yc, axis=1))) if n else np.nan
    return s[0], s[1:37].reshape(6, 6), s[37:], bool((zc <= 0).any()), ratio


def resect_numpy(graph, dtype, opts=None, select=None):
    """The definition of gbp_resect_cameras in `dtype` arithmetic -> dict cam_mean [C, 6] (the start pose where nothing is written),
    cam_info [C, 36], report [C, 4] (NaN where nothing is written), status [C], n_views [C], depth_ratio [C]: the smallest
    |depth| / distance of a used landmark at the accepted pose."""
    T = np.dtype(dtype).type
    o = dict(DEFAULTS, **(opts or {}))
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    K = np.asarray(graph["K"], np.float32).astype(T).reshape(3, 3)
    pts = np.asarray(graph["lmk_mean"], np.float32).astype(T).reshape(L, 3)
    zs = np.asarray(graph["measurements"], np.float32).astype(T).reshape(-1, 2)
    E = len(zs)
    lmk_id, start = np.asarray(graph["lmk_id"], np.int64), np.asarray(graph["cam_start"], np.int64)
    edges = np.arange(E) if graph.get("cam_edges") is None else np.asarray(graph["cam_edges"], np.int64)
    act = None if graph.get("active_flag") is None else np.asarray(graph["active_flag"])
    use = None if graph.get("lmk_use") is None else np.asarray(graph["lmk_use"])
    mean = np.asarray(graph["cam_mean"], np.float32).astype(T).reshape(C, 6).copy()
    info, report = np.full((C, 36), np.nan, T), np.full((C, 4), np.nan, T)
    status, n_views, ratio = np.zeros(C, np.uint32), np.zeros(C, np.uint32), np.full(C, np.nan)
    huber, var = float(np.float32(o["huber_px"])), T(o["reproj_meas_var"])
    with np.errstate(all="ignore"):
        for c in range(C):
            if select is not None and select[c] == 0:
                continue
            st = 0
            k0, k1 = start[c], start[c + 1]
            if k1 > E:
                k1, st = E, BAD_INDEX
            if k0 > k1:
                k0, st = k1, BAD_INDEX
            e = edges[k0:k1]
            if (e >= E).any():
                st, e = BAD_INDEX, e[e < E]
            if act is not None:
                e = e[act[e] == 1]
            if (lmk_id[e] >= L).any():
                st, e = BAD_INDEX, e[lmk_id[e] < L]
            if use is not None:
                e = e[use[lmk_id[e]] != 0]
            n = n_views[c] = e.size
            if n == 0 or n < o["min_views"]:
                status[c] = st | (NO_VIEW if n == 0 else FEW_VIEWS)
                continue
            lm, z = pts[lmk_id[e]], zs[e]
            x = mean[c].copy()
            cost, H, g, behind, rat = _pass(x, lm, z, K, huber, T)
            if not (np.isfinite(cost) and np.isfinite(H).all() and np.isfinite(g).all()):
                status[c] = st | NONFINITE
                continue
            cost0, passes, lam, last, accepted = cost, 1, T(np.float32(o["lambda0"])), T(0), False
            while passes < o["max_passes"] and lam <= 1e8:
                A = H.copy()
                A[np.diag_indices(6)] = np.diag(H) * (T(1) + lam)
                try:
                    dx = np.linalg.solve(A.astype(np.float64), g.astype(np.float64)).astype(T)
                except np.linalg.LinAlgError:
                    dx = np.full(6, np.nan, T)
                if not np.isfinite(dx).all():
                    lam = T(lam * T(10))
                    continue
                xt = (x + dx).astype(T)
                ct, Ht, gt, bt, rt = _pass(xt, lm, z, K, huber, T)
                passes += 1
                if np.isfinite(xt).all() and np.isfinite(ct) and np.isfinite(Ht).all() and np.isfinite(gt).all() and ct < cost:
                    x, cost, H, g, behind, rat, last, accepted = xt, ct, Ht, gt, bt, rt, np.max(np.abs(dx)), True
                    lam = max(T(lam / T(10)), T(1e-9))
                else:
                    lam = T(lam * T(10))
            mean[c], info[c], report[c], ratio[c] = x, (H / var).ravel(), [cost0, cost, last, lam], rat
            status[c] = st | (BEHIND if behind else 0) | (0 if accepted else STALLED)
    return {"cam_mean": mean, "cam_info": info, "report": report, "status": status, "n_views": n_views, "depth_ratio": ratio}


def ambiguous(ref64, opts=None):
    """[C] bool: the cameras whose status is not a property of the inputs, decided on the float64 run: a depth within 10 % of zero
    (|depth| below a tenth of the landmark's distance) or a view count AT min_views"""
    o = dict(DEFAULTS, **(opts or {}))
    with np.errstate(all="ignore"):
        return (ref64["depth_ratio"] < 0.1) | (ref64["n_views"] == o["min_views"])


def pose_error(x, x64):
    x, x64 = np.asarray(x, np.float64).reshape(-1, 6), np.asarray(x64, np.float64).reshape(-1, 6)
    return float(np.max(np.max(np.abs(x - x64), axis=1) / np.max(np.abs(x64), axis=1))) if x.size else 0.0


def eta_numpy(priors_lambda, cam_mean):
    """the row dots of the prior Lambda with the pose, fp32, k ascending"""
    lam, x = np.asarray(priors_lambda, np.float32).reshape(-1, 6, 6), np.asarray(cam_mean, np.float32).reshape(-1, 6)
    s = np.zeros((len(x), 6), np.float32)
    for k in range(6):
        s = (s + lam[:, :, k] * x[:, k:k + 1]).astype(np.float32)
    return s


# ---- graphs ----
def perturbed(cams, rng, trans=0.05, rot_deg=2.0):
    """every pose `trans` and `rot_deg` degrees away from `cams` [C, 6], in random directions"""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    d = rng.normal(size=(len(cams), 6))
    d[:, :3] *= trans / np.linalg.norm(d[:, :3], axis=1, keepdims=True)
    d[:, 3:] *= np.deg2rad(rot_deg) / np.linalg.norm(d[:, 3:], axis=1, keepdims=True)
    return (cams + d).astype(np.float32)


def degree_scene(degrees, seed=11, noise=0.5, outliers=True, n_lmks=None):
    """A hand-made scene: camera c looks down +z with a rotation vector of about 0.1 rad and sees degrees[c] distinct landmarks (chosen at
    random) that lie 4 to 8 in front; pixel noise `noise`; every fifth camera has 10 % of its pixels displaced by 80 px; every camera
    starts 0.05 and 2 degrees from the truth.  Edges in file order (sorted by camera): cam_edges is None.
    -> (graph, true poses [C, 6] float64)"""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    C, L = degrees.size, int(n_lmks or max(1, degrees.max(initial=0)))
    w = rng.normal(size=(C, 3))
    w *= rng.uniform(0.05, 0.15, (C, 1)) / np.linalg.norm(w, axis=1, keepdims=True)
    cams = np.concatenate([rng.uniform(-1, 1, (C, 2)), rng.uniform(-0.3, 0.3, (C, 1)), w], axis=1).astype(np.float32).astype(np.float64)
    pts = np.concatenate([rng.uniform(-2, 2, (L, 2)), rng.uniform(4, 8, (L, 1))], axis=1).astype(np.float32)
    cam_id = np.repeat(np.arange(C), degrees)
    lmk_id = np.concatenate([np.sort(rng.choice(L, k, replace=False)) for k in degrees] + [np.zeros(0, np.int64)]).astype(np.int64)
    z = project64(cams, pts, cam_id, lmk_id, K_SYNTH) + noise * rng.normal(size=(cam_id.size, 2))
    if outliers:
        for c in range(0, C, 5):
            e = np.flatnonzero(cam_id == c)
            hit = e[rng.uniform(size=e.size) < 0.1]
            a = rng.uniform(0, 2 * np.pi, hit.size)
            z[hit] += 80.0 * np.stack([np.cos(a), np.sin(a)], axis=1)
    return graph_of(C, L, cam_id, lmk_id, K_SYNTH, perturbed(cams, rng), pts, z, identity=True), cams


def mean_reprojection(cam_mean, graph, cams_mask=None):
    """float64 mean reprojection error per camera [C] (NaN: no edge) of poses cam_mean against the graph's landmarks, over all edges"""
    z = project64(cam_mean, graph["lmk_mean"], graph["cam_id"].astype(np.int64), graph["lmk_id"].astype(np.int64), graph["K"])
    err = np.linalg.norm(z - np.asarray(graph["measurements"], np.float64).reshape(-1, 2), axis=1)
    n = np.bincount(graph["cam_id"], minlength=graph["n_cams"])
    with np.errstate(all="ignore"):
        return np.bincount(graph["cam_id"], weights=err, minlength=graph["n_cams"]) / n
