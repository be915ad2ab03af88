"""What tests/test_seed_cpu.py and tests/test_gpu_seed.py share: the host twin of the seeding arithmetic
(tests/sanitize/seed_math_main.cpp, a stand-alone program: compiled here, run as a process, never loaded into python), its file format,
an INDEPENDENT numpy implementation of the definition in include/gbp_mi355x_seed.h, parametrised by dtype, and the graphs the case
families are made of.

The numpy implementation follows the header's text, not the C++: matrices and np.linalg.solve in place of unrolled loops, np.sum in place
of serial sums, closed-form pin-hole derivatives.  Its float32 run against its float64 run measures what float32 costs on a family; the
tests allow the code under test 8 x that (the project's convention), per measure:
    point    max over landmarks of max |x - x64| / max |x64|
    lam      max over landmarks of |lam - lam64| / lam64
"""
import os

import numpy as np

from tests import host_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "sanitize", "seed_math_main.cpp")
NO_VIEW, ONE_VIEW, LOW_PARALLAX, BEHIND, NONFINITE, BAD_INDEX = 1, 2, 4, 8, 16, 32
DEFAULTS = {"min_parallax": 5e-3, "fallback_depth": 1.0, "refine_iters": 2, "reproj_meas_var": 4.0}
K_SYNTH = np.array([500.0, 0.0, 320.0, 0.0, 500.0, 240.0, 0.0, 0.0, 1.0], np.float32)
OUTPUTS = (("lmk_mean", 3, np.float32), ("lmk_priors_eta", 3, np.float32), ("lmk_priors_lambda", 9, np.float32), ("status", 1, np.uint32),
           ("n_views", 1, np.uint32))


def compile_host(exe, sanitize):
    return host_twin.compile_host(MAIN, exe, sanitize)


def index_numpy(lmk_id, n_lmks):
    """the landmark-major index by a stable argsort"""
    lmk_id = np.asarray(lmk_id, np.int64)
    start = np.zeros(n_lmks + 1, np.uint32)
    start[1:] = np.cumsum(np.bincount(lmk_id, minlength=n_lmks))
    return start, np.argsort(lmk_id, kind="stable").astype(np.uint32)


def initial_outputs(n_lmks, seed=7):
    """what the output arrays hold before a call: recognisable values, so that 'not touched' can be seen"""
    rng = np.random.default_rng(seed)
    return {k: (rng.integers(1 << 20, 1 << 21, w * n_lmks).astype(np.uint32) if dt is np.uint32 else
                rng.uniform(1000.0, 2000.0, w * n_lmks).astype(np.float32)) for k, w, dt in OUTPUTS}


def run_host(exe, tmp, graph, opts=None, select=None, before=None, trig="libm"):
    """-> dict of the five output arrays after the host program's run of `graph` (a dict: n_cams, n_lmks, cam_id, lmk_start, lmk_edges, K,
    cam_mean, measurements, active_flag or None).  before: what the outputs hold before (default initial_outputs)."""
    o = dict(DEFAULTS, **(opts or {}))
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    cam_id = np.ascontiguousarray(graph["cam_id"], np.uint32)
    E = cam_id.size
    act = np.ones(E, np.uint32) if graph.get("active_flag") is None else np.ascontiguousarray(graph["active_flag"], np.uint32)
    sel = np.ones(L, np.uint32) if select is None else np.ascontiguousarray(select, np.uint32)
    before = initial_outputs(L) if before is None else before
    parts = [np.array([C, L, E, int(select is not None)], np.uint32),
             np.array([o["min_parallax"], o["fallback_depth"], o["reproj_meas_var"]], np.float32), np.array([o["refine_iters"]], np.uint32),
             np.ascontiguousarray(graph["cam_mean"], np.float32).ravel(), cam_id, np.ascontiguousarray(graph["lmk_start"], np.uint32),
             np.ascontiguousarray(graph["lmk_edges"], np.uint32), np.ascontiguousarray(graph["K"], np.float32).ravel(),
             np.ascontiguousarray(graph["measurements"], np.float32).ravel(), act, sel] + [before[k] for k, _, _ in OUTPUTS]
    return host_twin.run(exe, tmp, "seed", parts, [(name, dt, w * L) for name, w, dt in OUTPUTS], trig, timeout=300)


# ---- the definition, in numpy, in one dtype ----
def _hat(v, T):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], T)


def _rotation(w, T):
    th = np.sqrt(np.sum(w * w, dtype=T))
    if not th >= 1e-6:
        return np.eye(3, dtype=T) if th == th else np.full((3, 3), np.nan, T)
    W = _hat(w, T)
    return (np.eye(3, dtype=T) + (np.sin(th) / th) * W + ((T(1) - np.cos(th)) / (th * th)) * (W @ W)).astype(T)


def _solve(A, b, T):
    try:
        with np.errstate(all="ignore"):
            return np.linalg.solve(A, b).astype(T)
    except np.linalg.LinAlgError:
        return np.full(3, np.nan, T)


def seed_numpy(graph, dtype, opts=None, details=False):
    """The definition of gbp_seed_landmarks in `dtype` arithmetic -> dict lmk_mean [L, 3], lam [L], status [L], n_views [L] (a landmark
    without a used view: NaN mean and lam); with details also parallax [L] and depth_ratio [L]: the smallest |depth| / distance of the
    point that is written over its used views (the sine of its elevation over a camera's plane z = 0)."""
    T = np.dtype(dtype).type
    o = dict(DEFAULTS, **(opts or {}))
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    K = np.asarray(graph["K"], np.float32).astype(T).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    cams = np.asarray(graph["cam_mean"], np.float32).astype(T).reshape(C, 6)
    z = np.asarray(graph["measurements"], np.float32).astype(T).reshape(-1, 2)
    cam_id, start, edges = np.asarray(graph["cam_id"]), np.asarray(graph["lmk_start"], np.int64), np.asarray(graph["lmk_edges"], np.int64)
    act = None if graph.get("active_flag") is None else np.asarray(graph["active_flag"])
    with np.errstate(all="ignore"):
        R = np.stack([_rotation(c[3:], T) for c in cams]) if C else np.zeros((0, 3, 3), T)
        t = cams[:, :3]
        centre = -np.einsum("cji,cj->ci", R, t).astype(T)
    mean, lam = np.full((L, 3), np.nan, T), np.full(L, np.nan, T)
    status, n_views = np.zeros(L, np.uint32), np.zeros(L, np.uint32)
    parallax, ratio = np.full(L, np.nan), np.full(L, np.nan)
    var = T(o["reproj_meas_var"])

    def project(x, c):      # (camera-frame points [n, 3], pin-hole Jacobians [n, 2, 3])
        p = np.einsum("nij,j->ni", R[c], x).astype(T) + t[c]
        J = np.zeros((len(c), 2, 3), T)
        J[:, 0, 0], J[:, 0, 2] = fx / p[:, 2], -fx * p[:, 0] / (p[:, 2] * p[:, 2])
        J[:, 1, 1], J[:, 1, 2] = fy / p[:, 2], -fy * p[:, 1] / (p[:, 2] * p[:, 2])
        return p, J

    with np.errstate(all="ignore"):
        for l in range(L):
            e = edges[start[l]:start[l + 1]]
            if act is not None:
                e = e[act[e] == 1]
            n = n_views[l] = e.size
            if n == 0:
                status[l] = NO_VIEW
                continue
            c = cam_id[e]
            pix = np.stack([(z[e, 0] - cx) / fx, (z[e, 1] - cy) / fy, np.ones(n, T)], axis=1).astype(T)
            w = np.einsum("nji,nj->ni", R[c], pix).astype(T)
            d = (w / np.sqrt(np.sum(w * w, axis=1, dtype=T))[:, None]).astype(T)
            place = (centre[c[0]] + T(o["fallback_depth"]) * w[0]).astype(T)
            st, x = 0, None
            if n == 1:
                st = ONE_VIEW
            else:
                m = np.sum(d, axis=0, dtype=T) / T(n)
                parallax[l] = par = T(1) - np.sum(m * m, dtype=T)
                if par < T(o["min_parallax"]):
                    st = LOW_PARALLAX
                else:
                    P = (np.eye(3, dtype=T)[None] - d[:, :, None] * d[:, None, :]).astype(T)
                    x = _solve(np.sum(P, axis=0, dtype=T), np.sum(np.einsum("nij,nj->ni", P, centre[c]).astype(T), axis=0, dtype=T), T)
                    for _ in range(int(o["refine_iters"])):
                        p, Jp = project(x, c)
                        r = (z[e] - np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], axis=1)).astype(T)
                        J = np.einsum("nij,njk->nik", Jp, R[c]).astype(T)
                        xn = x + _solve(np.einsum("nki,nkj->ij", J, J).astype(T), np.einsum("nki,nk->i", J, r).astype(T), T)
                        if not np.isfinite(xn).all():
                            break
                        x = xn.astype(T)
                    if not np.isfinite(x).all():
                        st, x = NONFINITE, None
            placed = x is None
            x = place if placed else x
            while True:
                p, Jp = project(x, c)
                Rx = np.einsum("nij,j->ni", R[c], x).astype(T)
                full = np.concatenate([Jp, -np.einsum("nij,njk->nik", Jp, np.stack([_hat(v, T) for v in Rx])),
                                       np.einsum("nij,njk->nik", Jp, R[c])], axis=2)
                a = np.abs(full)
                peak = T(np.max(a[np.isfinite(a)], initial=0.0)) if not np.isinf(a).any() else T(np.inf)
                lm = T((np.float64(peak) * np.float64(peak)) / np.float64(var))
                behind = bool((p[:, 2] <= 0).any())
                if (np.isfinite(x).all() and np.isfinite(lm) and np.isfinite(x * lm).all()) or placed:
                    break
                placed, x, st = True, place, st | NONFINITE
            if not (np.isfinite(x).all() and np.isfinite(lm) and np.isfinite(x * lm).all()):
                st |= NONFINITE
            mean[l], lam[l], status[l] = x, lm, st | (BEHIND if behind else 0)
            ratio[l] = np.min(np.abs(p[:, 2]) / np.sqrt(np.sum(p * p, axis=1)))
    out = {"lmk_mean": mean, "lam": lam, "status": status, "n_views": n_views}
    if details:
        out.update(parallax=parallax, depth_ratio=ratio)
    return out


def ambiguous(ref64, opts=None, nonfinite_family=False):
    """[L] bool: the landmarks whose status is not a property of the inputs, decided in float64 on the reference's run with details:
    a parallax measure within a factor 2 of min_parallax, a smallest depth within 10 % of zero (|depth| below a tenth of the point's
    distance from that camera), or anything not finite (outside the non-finite family)."""
    o = dict(DEFAULTS, **(opts or {}))
    par = ref64["parallax"]
    with np.errstate(all="ignore"):
        bad = (par > 0.5 * o["min_parallax"]) & (par < 2.0 * o["min_parallax"])
        bad |= ref64["depth_ratio"] < 0.1
    if not nonfinite_family:
        seen = ref64["n_views"] > 0
        bad |= seen & ~(np.isfinite(ref64["lmk_mean"]).all(axis=1) & np.isfinite(ref64["lam"]))
        bad |= (ref64["n_views"] > 1) & ~np.isfinite(par)
    return bad


def point_error(x, x64):
    x, x64 = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(x64, np.float64).reshape(-1, 3)
    return float(np.max(np.max(np.abs(x - x64), axis=1) / np.max(np.abs(x64), axis=1))) if x.size else 0.0


def lam_error(lam, lam64):
    lam, lam64 = np.asarray(lam, np.float64).ravel(), np.asarray(lam64, np.float64).ravel()
    return float(np.max(np.abs(lam - lam64) / lam64)) if lam.size else 0.0


# ---- graphs ----
def graph_of(n_cams, n_lmks, cam_id, lmk_id, K, cam_mean, measurements, active_flag=None):
    start, edges = index_numpy(lmk_id, n_lmks)
    return {"n_cams": int(n_cams), "n_lmks": int(n_lmks), "cam_id": np.asarray(cam_id, np.uint32), "lmk_id": np.asarray(lmk_id, np.uint32),
            "lmk_start": start, "lmk_edges": edges, "K": np.asarray(K, np.float32), "cam_mean": np.asarray(cam_mean, np.float32).ravel(),
            "measurements": np.asarray(measurements, np.float32).ravel(), "active_flag": active_flag}


def project64(cam_mean, points, cam_id, lmk_id, K):
    """float64 pixels of the observations (cam_id, lmk_id)"""
    cams = np.asarray(cam_mean, np.float64).reshape(-1, 6)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    Km = np.asarray(K, np.float64).reshape(3, 3)
    R = np.stack([_rotation(c[3:], np.float64) for c in cams])
    p = np.einsum("eij,ej->ei", R[cam_id], pts[lmk_id]) + cams[cam_id, :3]
    return np.stack([Km[0, 0] * p[:, 0] / p[:, 2] + Km[0, 2], Km[1, 1] * p[:, 1] / p[:, 2] + Km[1, 2]], axis=1)


def degree_graph(degrees, seed=11, noise=0.0, n_cams=None):
    """A hand-made scene: cameras spread over a 4 x 4 x 0.6 slab looking down +z with rotations up to 0.2 rad, points 4 to 8 in front of
    them; landmark l is seen by degrees[l] distinct cameras (chosen at random), edges sorted by (camera, landmark) as a file's are.
    -> (graph, points [L, 3] float64)"""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    C = int(n_cams or max(2, degrees.max(initial=0)))
    cams = np.concatenate([rng.uniform(-2, 2, (C, 2)), rng.uniform(-0.3, 0.3, (C, 1)), rng.uniform(-0.2, 0.2, (C, 3))], axis=1).astype(np.float32)
    pts = np.concatenate([rng.uniform(-2, 2, (degrees.size, 2)), rng.uniform(4, 8, (degrees.size, 1))], axis=1)
    lmk_id = np.repeat(np.arange(degrees.size), degrees)
    cam_id = np.concatenate([rng.choice(C, k, replace=False) for k in degrees] + [np.zeros(0, np.int64)]).astype(np.int64)
    order = np.lexsort((lmk_id, cam_id))
    cam_id, lmk_id = cam_id[order], lmk_id[order]
    z = project64(cams, pts, cam_id, lmk_id, K_SYNTH) + noise * rng.normal(size=(cam_id.size, 2))
    return graph_of(C, degrees.size, cam_id, lmk_id, K_SYNTH, cams, z), pts


def bal_graph(bal, K, cam_mean=None, measurements=None):
    """the graph of a loaded file at its file cameras"""
    cams = np.asarray(bal["cameras"], np.float64).astype(np.float32) if cam_mean is None else cam_mean
    z = np.asarray(bal["observations"], np.float64).astype(np.float32) if measurements is None else measurements
    return graph_of(bal["n_cams"], bal["n_lmks"], bal["cam_id"], bal["lmk_id"], K, cams, z)
