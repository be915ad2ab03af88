"""What tests/test_locate_cpu.py and tests/test_gpu_locate.py share: the host twin of the location arithmetic
(tests/sanitize/locate_math_main.cpp, a stand-alone program: compiled here, run as a process, never loaded into python), its file
formats, an INDEPENDENT numpy implementation of the definition in include/gbp_mi355x_locate.h, and the scenes the case families are
made of.

The numpy implementation follows the header's text where the header fixes the outcome (the hash, the sampling, the counting, the tie
rule, what is written) and is its own where the header only fixes the mathematics: its three-point solver is Grunert's — the two
depth ratios, the resultant of the two quadratics in one of them as a quartic in the other through numpy's polynomial arithmetic, the
roots of the companion matrix, each polished by Newton on the two quadratics themselves, the pose of each root by the SVD
alignment of the three points — and its rotation vector comes from
numpy's arctan2.  The solver runs in a dtype: its float32 run against its float64 run measures what float32 costs on a family, and the
tests allow the code under test 8 x that (the project's convention).
"""
import os

import numpy as np

from tests import host_twin
from tests import resect_support as rs
from tests.seed_support import K_SYNTH, _rotation, project64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "sanitize", "locate_math_main.cpp")
NO_VIEW, BAD_INDEX, FEW_VIEWS, FEW_INLIERS, NO_HYPOTHESIS = 1, 32, 64, 256, 512
NOT_LOCATED = NO_VIEW | FEW_VIEWS | FEW_INLIERS | NO_HYPOTHESIS
DEFAULTS = {"rounds": 4, "inlier_px": 5.0, "min_inliers": 6, "seed": 0}
HAIR = 1e-4
# per camera (width, dtype), but `inlier`, which is per edge
OUTPUTS = (("cam_mean", 6, np.float32), ("inlier", None, np.uint32), ("report", 4, np.float32), ("status", 1, np.uint32),
           ("n_views", 1, np.uint32), ("n_inliers", 1, np.uint32))


def compile_host(exe, sanitize):
    return host_twin.compile_host(MAIN, exe, sanitize)


def sizes(graph):
    C, E = int(graph["n_cams"]), int(np.asarray(graph["lmk_id"]).size)
    return {k: (E if w is None else w * C) for k, w, _ in OUTPUTS}


def initial_outputs(graph, seed=7):
    """what the output arrays hold before a call: recognisable values, so that 'not touched' can be seen"""
    rng = np.random.default_rng(seed)
    n = sizes(graph)
    return {k: (rng.integers(1 << 20, 1 << 21, n[k]).astype(np.uint32) if dt is np.uint32 else rng.uniform(1000.0, 2000.0, n[k]).astype(np.float32))
            for k, _, dt in OUTPUTS}


def _parts(graph, opts, select, before, with_inlier, mode=0):
    o = dict(DEFAULTS, **(opts or {}))
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    lmk_id = np.ascontiguousarray(graph["lmk_id"], np.uint32)
    E = lmk_id.size

    def opt(a, n):
        return np.zeros(n, np.uint32) if a is None else np.ascontiguousarray(a, np.uint32)

    has = (int(select is not None) | 2 * int(graph.get("cam_edges") is not None) | 4 * int(graph.get("active_flag") is not None) |
           8 * int(graph.get("lmk_use") is not None) | 16 * int(with_inlier) | mode)
    before = initial_outputs(graph) if before is None else before
    return [np.array([C, L, E, has], np.uint32), np.array([o["rounds"], o["min_inliers"], o["seed"]], np.uint32),
            np.array([o["inlier_px"]], np.float32), lmk_id, np.ascontiguousarray(graph["cam_start"], np.uint32), opt(graph.get("cam_edges"), E),
            np.ascontiguousarray(graph["K"], np.float32).ravel(), np.ascontiguousarray(graph["lmk_mean"], np.float32).ravel(),
            np.ascontiguousarray(graph["measurements"], np.float32).ravel(), opt(graph.get("active_flag"), E), opt(graph.get("lmk_use"), L),
            opt(select, C)] + [before[k] for k, _, _ in OUTPUTS]


def run_host(exe, tmp, graph, opts=None, select=None, before=None, with_inlier=True, trig="libm"):
    """-> dict of the six output arrays after the host program's run of `graph`.  before: what the outputs hold before (default
    initial_outputs).  with_inlier False: the inlier array is not passed (NULL)."""
    n = sizes(graph)
    return host_twin.run(exe, tmp, "locate", _parts(graph, opts, select, before, with_inlier), [(k, dt, n[k]) for k, _, dt in OUTPUTS], trig,
                         timeout=300)


def run_solver(exe, tmp, K, pixels, points):
    """the three-point solver alone on N triples: pixels [N, 3, 2], points [N, 3, 3] (float32) -> (n [N], R [N, 4, 3, 3], t [N, 4, 3])"""
    px, pts = np.ascontiguousarray(pixels, np.float32), np.ascontiguousarray(points, np.float32)
    N = px.shape[0]
    out = host_twin.run(exe, tmp, "locate", [np.array([N, 0, 0, 256], np.uint32), np.ascontiguousarray(K, np.float32).ravel(), px.ravel(), pts.ravel()],
                        [("n", np.uint32, N), ("R", np.uint32, 72 * N), ("t", np.uint32, 24 * N)], timeout=300)
    return out["n"], out["R"].view(np.float64).reshape(N, 4, 3, 3), out["t"].view(np.float64).reshape(N, 4, 3)


def run_sampling(exe, tmp, graph, queries):
    """queries [Q, 4] = (seed, c, r, j) -> [Q, 4] = (1 if the hypothesis is not void, the three offsets)"""
    q = np.ascontiguousarray(queries, np.uint32)
    parts = _parts(graph, None, None, None, True, mode=512) + [np.array([len(q)], np.uint32), q.ravel()]
    return host_twin.run(exe, tmp, "locate", parts, [("res", np.uint32, 4 * len(q))], timeout=300)["res"].reshape(-1, 4)


# ---- the header's hash and sampling, restated ----
def mix(x):
    x = np.uint32(x)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x = np.uint32(x * np.uint32(0x7feb352d))
        x ^= x >> np.uint32(15); x = np.uint32(x * np.uint32(0x846ca68b))
        x ^= x >> np.uint32(16)
    return x


def sample(seed, c, r, j, deg, used, lmk):
    """used [deg] bool, lmk [deg]: the index range of camera c -> the three offsets, or None (void)"""
    with np.errstate(over="ignore"):
        h = mix(mix(np.uint32(seed) + np.uint32(c)) + np.uint32(64 * r + j))
        taken = []
        for s in range(3):
            for t in range(8):
                d = (int(mix(h + np.uint32(8 * s + t))) * int(deg)) >> 32
                if used[d] and all(lmk[d] != lmk[k] for k in taken):
                    taken.append(d)
                    break
            else:
                return None
    return taken


# ---- an independent three-point solver (Grunert), in one dtype ----
def _roots(coeffs, T):
    """the roots of a polynomial (highest power first) as the eigenvalues of its companion matrix, in dtype T"""
    c = np.asarray(coeffs, T)
    n = len(c) - 1
    M = np.zeros((n, n), T)
    M[0] = -c[1:] / c[0]
    M[np.arange(1, n), np.arange(n - 1)] = 1
    return np.linalg.eigvals(M)


def bearings(K, pixels, T):
    K = np.asarray(K, T).reshape(3, 3)
    px = np.asarray(pixels, T).reshape(-1, 2)
    y = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(px), T)], axis=1).astype(T)
    return (y / np.sqrt(np.sum(y * y, axis=1, dtype=T))[:, None]).astype(T)


def p3p_numpy(K, pixels, X, dtype, details=False):
    """-> list of (R [3, 3], t [3]) with R X_i + t = depth_i bearing_i, depth_i > 0.  details: also the smallest separation of the quartic's
    roots relative to their size, and the largest |imaginary part| of the roots taken as real."""
    T = np.dtype(dtype).type
    X = np.asarray(X, T).reshape(3, 3)
    y = bearings(K, pixels, T)
    none = ([], np.inf, 0.0) if details else []
    with np.errstate(all="ignore"):
        a2, b2, c2 = [np.sum((X[i] - X[j]) ** 2, dtype=T) for i, j in ((1, 2), (0, 2), (0, 1))]
        n3 = np.cross(X[1] - X[0], X[2] - X[0])
        if not np.sum(n3 * n3) > 1e-10 * (c2 * b2):      # the header's 3.a: repeated or collinear points have no solution
            return none
        ca, cb, cg = [np.sum(y[i] * y[j], dtype=T) for i, j in ((1, 2), (0, 2), (0, 1))]
        # depths s1, u s1, v s1; polynomials in v, highest power first
        f = np.array([1, -2 * cb, 1], T)                      # 1 + v^2 - 2 v cos(beta)
        p1, p0 = np.array([-2 * b2 * cg], T), np.polysub(np.array([b2], T), c2 * f).astype(T)
        q1, q0 = np.array([-2 * b2 * ca, 0], T), np.polysub(np.array([b2, 0, 0], T), a2 * f).astype(T)
        p2 = np.array([b2], T)
        d20 = np.polysub(np.polymul(p2, q0), np.polymul(p0, p2))
        quartic = np.polysub(np.polymul(d20, d20), np.polymul(np.polysub(np.polymul(p2, q1), np.polymul(p1, p2)),
                                                              np.polysub(np.polymul(p1, q0), np.polymul(p0, q1)))).astype(T)
        if not np.isfinite(quartic).all() or len(quartic) != 5 or quartic[0] == 0:
            return none
        roots = _roots(quartic, T)
        sols, imag = [], 0.0
        for v in roots:
            if abs(v.imag) > 1e-4 * (1 + abs(v.real)) * (1 if T is np.float64 else 100):
                continue
            imag = max(imag, abs(v.imag))
            v = T(v.real)
            den = np.polyval(p1, v) - np.polyval(q1, v)
            u = T(-(np.polyval(p0, v) - np.polyval(q0, v)) / den)
            s1sq = b2 / (1 + v * v - 2 * v * cb)
            if not (v > 0 and u > 0 and s1sq > 0 and np.isfinite(u)):
                continue
            # The quartic's coefficients are differences of products of the data: in float32 its roots are rough.  Polish (u, v) on
            # the two quadratics themselves, whose coefficients are the data's, by Newton in T (eight steps; a root on which it has not settled is dropped).
            step, rough = np.inf, (u, v)
            for _ in range(8):
                g = T(1) + v * v - T(2) * v * cb
                P = b2 * (T(1) + u * u - T(2) * u * cg) - c2 * g
                Q = b2 * (u * u + v * v - T(2) * u * v * ca) - a2 * g
                Pu, Pv = b2 * (T(2) * u - T(2) * cg), -c2 * (T(2) * v - T(2) * cb)
                Qu, Qv = b2 * (T(2) * u - T(2) * v * ca), b2 * (T(2) * v - T(2) * u * ca) - a2 * (T(2) * v - T(2) * cb)
                det = Pu * Qv - Pv * Qu
                if not (det != 0 and np.isfinite(det)):
                    break
                du, dv = (P * Qv - Pv * Q) / det, (Pu * Q - P * Qu) / det
                u, v, step = T(u - du), T(v - dv), max(abs(du), abs(dv))
            if not step <= 1e3 * np.finfo(T).eps * (1 + abs(u) + abs(v)):      # Newton did not settle (a nearly double root)
                if T is not np.float64:
                    continue               # a float32 run has lost the root
                u, v = rough               # float64: the quartic's own root is good to 1e-9 there, and stays
            s1sq = b2 / (T(1) + v * v - T(2) * v * cb)
            if not (v > 0 and u > 0 and s1sq > 0 and np.isfinite(u) and np.isfinite(v)):
                continue
            s1 = np.sqrt(s1sq)
            Y = (np.array([s1, u * s1, v * s1], T)[:, None] * y).astype(T)
            mx, my = X.mean(axis=0), Y.mean(axis=0)
            U, _, Vt = np.linalg.svd(((Y - my).T @ (X - mx)).astype(T))
            D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))]).astype(T)
            R = (U @ D @ Vt).astype(T)
            sols.append((R, (my - R @ mx).astype(T)))
        if not details:
            return sols
        sep = min([abs(r1 - r2) / (1 + abs(r1)) for i, r1 in enumerate(roots) for r2 in roots[i + 1:]], default=np.inf)
        return sols, float(sep), float(imag)


def rotvec(R):
    """float64 rotation vector of a rotation matrix, through the quaternion and numpy's arctan2; below HAIR: length HAIR"""
    R = np.asarray(R, np.float64)
    q = np.empty(4)
    tr = np.trace(R)
    i = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if i == 0:
        q[:] = [1 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    else:
        a, b, c = i - 1, i % 3, (i + 1) % 3
        q[0] = R[c, b] - R[b, c]
        q[1 + a], q[1 + b], q[1 + c] = 1 + R[a, a] - R[b, b] - R[c, c], R[a, b] + R[b, a], R[a, c] + R[c, a]
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vn = np.linalg.norm(q[1:])
    th = 2 * np.arctan2(vn, q[0])
    if th >= HAIR:
        return q[1:] * th / vn
    return q[1:] * HAIR / vn if vn > 0 else np.array([HAIR, 0.0, 0.0])


def pose_of(R, t):
    return np.concatenate([np.asarray(t, np.float64), rotvec(R)])


def solution_distance(R, t, R2, t2):
    return max(np.max(np.abs(R - R2)), np.max(np.abs(t - t2)) / max(1.0, np.max(np.abs(t2))))


def match(sols, refs):
    """one to one: for each (R, t) of refs the index of its nearest of sols, or None if sols has another count, two refs share a
    nearest one, or one of sols is nearer to another ref than to the one it is given to (a run that lost, gained or merged a root)"""
    if len(sols) != len(refs):
        return None
    d = np.array([[solution_distance(np.asarray(a, np.float64), np.asarray(b, np.float64), R2, t2) for a, b in sols] for R2, t2 in refs]).reshape(len(refs), len(sols))
    idx = [int(i) for i in np.argmin(d, axis=1)]
    if len(set(idx)) != len(idx) or any(int(np.argmin(d[:, i])) != k for k, i in enumerate(idx)):
        return None
    return idx


# ---- the definition, in numpy float64 ----
def _project(R, t, X, K):
    yc = X @ R.T + t
    with np.errstate(all="ignore"):
        px = np.stack([K[0, 0] * yc[:, 0] / yc[:, 2] + K[0, 2], K[1, 1] * yc[:, 1] / yc[:, 2] + K[1, 2]], axis=1)
    return px, yc[:, 2], np.linalg.norm(yc, axis=1)


def camera_entries(graph, c):
    """(status bits of the index, the in-range index entries' edges [n], used [n] bool, landmark [n]) of camera c, in index order; an
    entry with a bad edge or landmark is kept as unused with landmark -1"""
    E, L = int(np.asarray(graph["lmk_id"]).size), int(graph["n_lmks"])
    lmk_id, start = np.asarray(graph["lmk_id"], np.int64), np.asarray(graph["cam_start"], np.int64)
    edges = np.arange(E) if graph.get("cam_edges") is None else np.asarray(graph["cam_edges"], np.int64)
    st, k0, k1 = 0, start[c], start[c + 1]
    if k1 > E:
        k1, st = E, BAD_INDEX
    if k0 > k1:
        k0, st = k1, BAD_INDEX
    e = edges[k0:k1].copy()
    bad = e >= E
    e[bad] = 0
    used = ~bad
    if graph.get("active_flag") is not None:
        used &= np.asarray(graph["active_flag"])[e] == 1
    l = lmk_id[e]
    bad_l = used & (l >= L)
    bad |= bad_l
    used &= ~bad_l
    l = np.where(l < L, l, 0)
    if graph.get("lmk_use") is not None:
        used &= np.asarray(graph["lmk_use"])[l] != 0
    return (st | (BAD_INDEX if bad.any() else 0)), e, used, np.where(used, l, -1)


def locate_numpy(graph, opts=None, select=None, rounds_list=None):
    """The definition of gbp_locate_cameras, float64 -> {rounds: dict} for every rounds of rounds_list (default: the options' alone;
    a smaller count is a prefix of a larger one's hypotheses).  Each dict: cam_mean [C, 6] (NaN where nothing is written), status,
    n_views, n_inliers [C], win [C] (64 r + j, -1: none), mask {c: (edges, 0/1)}, ambiguous [C] bool, triple {c: (pixels, points)} of the
    winner, sol {c: (R, t)}."""
    o = dict(DEFAULTS, **(opts or {}))
    rounds_list = sorted(rounds_list or [o["rounds"]])
    C, L = int(graph["n_cams"]), int(graph["n_lmks"])
    K = np.asarray(graph["K"], np.float64).reshape(3, 3)
    pts = np.asarray(graph["lmk_mean"], np.float32).astype(np.float64).reshape(L, 3)
    zs = np.asarray(graph["measurements"], np.float32).astype(np.float64).reshape(-1, 2)
    thr = float(np.float32(o["inlier_px"]))
    res = {r: {"cam_mean": np.full((C, 6), np.nan), "status": np.zeros(C, np.uint32), "n_views": np.zeros(C, np.uint32),
               "n_inliers": np.zeros(C, np.uint32), "win": np.full(C, -1, np.int64), "mask": {}, "ambiguous": np.zeros(C, bool), "triple": {},
               "sol": {}} for r in rounds_list}
    for c in range(C):
        if select is not None and select[c] == 0:
            continue
        st, e, used, lmk = camera_entries(graph, c)
        n = int(used.sum())
        for r in rounds_list:
            res[r]["n_views"][c] = n
            res[r]["status"][c] = st | (NO_VIEW if n == 0 else FEW_VIEWS if n < o["min_inliers"] else 0)
        if n < o["min_inliers"]:
            continue
        X, z = pts[np.where(lmk >= 0, lmk, 0)], zs[e]
        cands = []      # (hypothesis, R, t, count, agreeing set, margin trouble, (pixels, points))
        for hyp in range(64 * rounds_list[-1]):
            tri = sample(o["seed"], c, hyp // 64, hyp % 64, len(e), used, lmk)
            if tri is None:
                continue
            px3, X3 = z[tri].astype(np.float32), X[tri].astype(np.float32)
            for R, t in p3p_numpy(K, px3, X3, np.float64):
                if not (np.isfinite(R).all() and np.isfinite(t).all()):
                    continue
                px, depth, dist = _project(R, t, X, K)
                with np.errstate(all="ignore"):
                    err = np.linalg.norm(px - z, axis=1)
                    agree = used & (depth > 0) & (err <= thr)
                    shaky = used & (np.abs(depth) < 0.1 * dist)
                    near_in = agree & ((err > 0.9 * thr) | shaky)
                    near_out = used & ~agree & (((err < 1.1 * thr) & (depth > 0)) | shaky)
                cands.append((hyp, R, t, int(agree.sum()), agree, bool(near_in.any()), (px3, X3), int(near_out.sum()), px))
        for r in rounds_list:
            out = res[r]
            mine = [cd for cd in cands if cd[0] < 64 * r]
            if not mine:
                out["status"][c] |= NO_HYPOTHESIS
                continue
            best = max(cd[3] for cd in mine)
            win = next(cd for cd in mine if cd[3] == best)
            at = next(i for i, cd in enumerate(mine) if cd is win)
            amb = win[5]
            for i, cd in enumerate(mine):
                if cd is win:
                    continue
                # a candidate that observations within 10 % of the threshold (or depths within 10 % of zero) could lift over the winner
                amb = amb or (cd[3] + cd[7] >= best if i < at else cd[3] + cd[7] > best)
                # a runner-up within one count from a DIFFERENT pose: one that cannot agree with the winner's own observations — it predicts
                # one of them more than two thresholds away from the winner's prediction (two poses that both agree with an
                # observation lie within two thresholds of each other there)
                if cd[3] >= best - 1:
                    with np.errstate(all="ignore"):
                        amb = amb or not (np.linalg.norm(cd[8] - win[8], axis=1)[win[4]] <= 2 * thr).all()
            x = pose_of(win[1], win[2])
            # the final pass at the pose (float64, numpy's own rotation)
            px, depth, dist = _project(_rotation(x[3:], np.float64), x[:3], X, K)
            with np.errstate(all="ignore"):
                err = np.linalg.norm(px - z, axis=1)
                inl = used & (depth > 0) & (err <= thr)
                amb = amb or bool((used & (((err > 0.9 * thr) & (err < 1.1 * thr)) | (np.abs(depth) < 0.1 * dist))).any())
            out["n_inliers"][c], out["win"][c], out["ambiguous"][c] = int(inl.sum()), win[0], amb or int(inl.sum()) == o["min_inliers"]
            out["triple"][c], out["sol"][c] = win[6], (win[1], win[2])
            if inl.sum() < o["min_inliers"]:
                out["status"][c] |= FEW_INLIERS
                continue
            out["cam_mean"][c] = x
            out["mask"][c] = (e[used], inl[used].astype(np.uint32))
    return res


def float32_cost(ref, K):
    """What float32 costs on the winners of a float64 run -> (the largest pose difference (rs.pose_error) between the float64 winner and
    ITS solution of the numpy solver's float32 run on the winner's own triple, the cameras counted, the cameras left out).  The two
    runs' solutions are matched one to one; a camera on whose triple the float32 run lost, gained or merged a root is left out: the
    distance to some other pose is not a cost of float32."""
    worst, counted, left_out = 0.0, 0, 0
    for c, (px3, X3) in ref["triple"].items():
        if not np.isfinite(ref["cam_mean"][c]).all():
            continue
        s64 = p3p_numpy(K, px3, X3, np.float64)
        s32 = p3p_numpy(K, px3, X3, np.float32)
        idx = match(s32, s64)
        R64, t64 = ref["sol"][c]
        mine = [i for i, (R2, t2) in enumerate(s64) if solution_distance(R2, t2, R64, t64) == 0.0]
        if idx is None or len(mine) != 1:
            left_out += 1
            continue
        R, t = s32[idx[mine[0]]]
        worst, counted = max(worst, rs.pose_error(pose_of(R.astype(np.float64), t.astype(np.float64)), ref["cam_mean"][c])), counted + 1
    return worst, counted, left_out


# ---- scenes ----
def scene(degrees, seed=11, outlier_share=0.0, noise=0.0, n_lmks=None, rot=0.3, spread=2.0, depth=(4.0, 8.0)):
    """A hand-made scene: camera c looks down +z with a rotation vector of up to `rot` rad and sees degrees[c] distinct landmarks (chosen
    at random) that lie `depth` in front and up to `spread` to the sides; pixel noise uniform in +-noise; per camera the share `outlier_share` of its pixels (rounded
    down) is displaced by 80 px.  Edges in file order (sorted by camera): cam_edges is None.  cam_mean holds recognisable junk: no
    start pose is needed.  -> (graph, true poses [C, 6] float64, outlier [E] bool)"""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    C, L = degrees.size, int(n_lmks or max(1, degrees.max(initial=0)))
    w = rng.normal(size=(C, 3))
    w *= rng.uniform(0.05, rot, (C, 1)) / np.linalg.norm(w, axis=1, keepdims=True)
    cams = np.concatenate([rng.uniform(-1, 1, (C, 2)), rng.uniform(-0.3, 0.3, (C, 1)), w], axis=1).astype(np.float32).astype(np.float64)
    pts = np.concatenate([rng.uniform(-spread, spread, (L, 2)), rng.uniform(depth[0], depth[1], (L, 1))], axis=1).astype(np.float32)
    cam_id = np.repeat(np.arange(C), degrees)
    lmk_id = np.concatenate([np.sort(rng.choice(L, k, replace=False)) for k in degrees] + [np.zeros(0, np.int64)]).astype(np.int64)
    z = project64(cams, pts, cam_id, lmk_id, K_SYNTH) + noise * rng.uniform(-1, 1, (cam_id.size, 2))
    outlier = np.zeros(cam_id.size, bool)
    for c in range(C):
        e = np.flatnonzero(cam_id == c)
        hit = rng.choice(e, int(outlier_share * e.size), replace=False)
        a = rng.uniform(0, 2 * np.pi, hit.size)
        z[hit] += 80.0 * np.stack([np.cos(a), np.sin(a)], axis=1)
        outlier[hit] = True
    junk = rng.uniform(50.0, 60.0, 6 * C).astype(np.float32)
    return rs.graph_of(C, L, cam_id, lmk_id, K_SYNTH, junk, pts, z, identity=True), cams, outlier
