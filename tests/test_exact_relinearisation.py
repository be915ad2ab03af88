"""LINEARISE, the relinearising sweeps, prior weakening, inactive factors and NEW_KEYFRAME against float64 (tests/ref64.py).

tests/test_exact_inference.py holds the potentials fixed and builds its joint from what the engine linearised: nothing there checks the
linearisation itself, the relinearising branch of the sweep (the hoisted means and the per-camera record of the belief kernel, the
persistent kernel's camera owners, the sharded camera combines, and the per_factor_mu twin), WeakenPriorVertex inside the belief
kernel, or the zero messages of inactive factors and their activation.  Here the reference is a float64 linearisation whose Jacobian
is the complex-step derivative of ref64.project, the float64 Huber cost, and the joint of float64-scaled priors.

  E  LINEARISE: every factor's eta (9) and Lambda (9 x 9) against ref64.linearise_factor at solve() of the float32 beliefs; the
     robust flags exactly; again under live messages; on the tree the new potentials' exact marginals
  F  relinearising sweeps: WHICH factors relinearise from the counts alone; those against float64 at the pre-sweep means, all
     others bit-identical
  G  converged relinearising GBP (relin_mode = 1) is a stationary point of the float64 Huber cost
  H  prior weakening on the tree, inactive factors and their activation on the loopy graph, under exact inference

HOW THE BOUNDS WERE SET.  As in test_exact_inference: the CPU oracle (restatement, device summation order) ran the final graphs; its
error against ref64 is *_ORACLE below and every engine has to meet 8 x that, the same margin for the same reason (float32 additions in
another order; an error of meaning shows at 1e-3 and more).  The measure of E and F is per factor, ||a - b||_inf / ||b||_inf over the
nine / eighty-one entries; G's is max |g| / sum |terms| of ref64.cost_gradient; H's is that of A and B.  That the bounds are not blind
is asserted in float64 on the CPU (the tests named *not_blind*).  profiles/exact_inference.md has the same figures and the device's.

WHERE THE INPUTS ARE NOT THE PLAIN GRAPHS, so that the blindness and margin conditions can hold (reasons at _f_graph, _g_graph and
_huber_clear): F's row graph carries added measurement noise, G's B carries outliers on every seventh measurement, and the variant
without the Huber rescale is counted on the robust factors at least 10 % over the threshold.

The weaken flags cannot be read back through the C-ABI.  What is asserted of them is their effect, which determines them: after k
calls the priors are the uploaded ones times scaling^min(flag, k) for k = 1 .. 6, past every uploaded flag.
"""
import numpy as np
import pytest

from tests import ref64
from tests.conftest import per_var_rel
from tests.test_exact_inference import (A_BOUND, EXACT_PATHS, TENSORS, _Exact, _gpu_path, _inputs, _moved_by_leaving_out, _oracle,
                                        _sorted_by_camera, all_to_all, graph_a, graph_b, rounded_trig, row_graph)      # noqa: F401 (fixtures)

gpu = pytest.mark.gpu

NSTDS = 2.5                       # GbpParams.defaults: the reference's globals
MIN_LINEAR, UNDAMPED = 10, 8
MARGIN = 8.0
ROBUST_MARGIN = 1e-4              # every factor's |err / (nstds sigma) - 1| is at least this, asserted in float64: the flags are then decided

# ---- measured on the CPU oracle (restatement, sum order 1) against ref64 ---------------------------------------------------------------
# E: per graph, (eta, Lambda), the larger of the first LINEARISE and the one under live messages.  The geometry graph per |w| class:
# the rotation block divides (R^T - I) [w]x + w w^T by |w|^2, which cancels in float32 like eps / |w|.
GEOMETRY_W = (1e-3, 1e-2, 0.07, 0.5, 1.5, 3.0)
E_ORACLE = {"A": (1.913e-5, 2.738e-6), "B": (2.499e-5, 1.145e-6),
            "G": {0: (1.834e-5, 2.080e-5), 1: (1.606e-5, 2.021e-6), 2: (3.050e-5, 2.154e-6), 3: (7.617e-6, 4.628e-6), 4: (7.439e-6, 1.806e-6),
                  5: (5.072e-6, 5.351e-6)}}
# F: per graph and relin_mode, over the 14 sweeps of both legs (all factors active; a third inactive)
F_ORACLE = {("B", 0): (1.380e-5, 6.942e-7), ("B", 1): (2.009e-5, 1.030e-6), ("rows", 0): (6.569e-5, 3.140e-6), ("rows", 1): (1.225e-4, 3.931e-6)}
F_SWEEPS = 14
# G: max |g| / sum |terms| after 200 sweeps, relin_mode = 1
G_SWEEPS = 200
G_ORACLE = {"all": 2.183e-6, "inactive": 1.698e-6}
G_ACCUMULATING_STAYS_ABOVE = 1e-2      # relin_mode = 0 accumulates onto the old potential (the reference's behaviour): not a stationary point
# H: per weakening count, the tensors of A; the loopy graph with 16 factors inactive, and after their activation
H_WEAKEN_ORACLE = {1: {"cam_mean": 1.965e-6, "lmk_mean": 1.049e-5, "cam_lambda": 1.742e-7, "lmk_lambda": 1.676e-7},
                   2: {"cam_mean": 1.945e-6, "lmk_mean": 8.710e-6, "cam_lambda": 1.429e-7, "lmk_lambda": 1.896e-7},
                   3: {"cam_mean": 1.822e-6, "lmk_mean": 1.694e-5, "cam_lambda": 1.106e-7, "lmk_lambda": 1.936e-7}}
B_INACTIVE_ORACLE = {"cam_mean": 5.302e-8, "lmk_mean": 2.097e-7}
B_ACTIVATED_ORACLE = {"cam_mean": 5.081e-8, "lmk_mean": 2.466e-7}
H_COND_LIMIT = 16000.0            # of A's joint after the third weakening: float32 eps x condition stays below 1e-3
H_SWEEPS = 160


def _bound(pair):
    return tuple(MARGIN * v for v in pair)


# ---- the geometry graph ----------------------------------------------------------------------------------------------------------------
GEOMETRY_CLASS = (0, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5)      # |w| class of each of the 16 cameras


def geometry_graph(seed=3):
    """16 cameras of 17 factors (two rows each, so every camera crosses a row boundary) on 68 shared landmarks in a cloud of radius
    1.1; rotation vectors of the lengths GEOMETRY_W in random directions; depths from 0.5 to 50; the measurement of a factor is the
    float64 projection at the initial means (the noisy file values the priors are centred on) shifted by 1 .. 4 px (even factors) or
    6.5 .. 30 px (odd factors): against the Huber threshold of 2.5 x 2 px about half the factors are robust, none near it."""
    rng = np.random.default_rng(seed)
    C, L, per = 16, 68, 17
    cam_id = np.repeat(np.arange(C), per)
    lmk_id = np.concatenate([(4 * c + 3 * np.arange(per)) % L for c in range(C)])
    cam_id, lmk_id = _sorted_by_camera(cam_id, lmk_id)
    depth = np.geomspace(1.2, 50.0, C)[rng.permutation(C)]
    cams = np.zeros((C, 6))
    for c in range(C):
        d = rng.normal(size=3)
        cams[c, 3:] = GEOMETRY_W[GEOMETRY_CLASS[c]] * d / np.linalg.norm(d)
        cams[c, :3] = [0.1 * depth[c] * rng.uniform(-1, 1), 0.1 * depth[c] * rng.uniform(-1, 1), depth[c]]
    pts = rng.normal(size=(L, 3))
    pts = 1.1 * pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (L, 1))
    bal = {"n_cams": C, "n_lmks": L, "n_edges": len(cam_id), "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0,
           "cam_id": np.asarray(cam_id, np.uint32), "lmk_id": np.asarray(lmk_id, np.uint32),
           "cameras": (cams * (1.0 + rng.normal(0, 0.003, cams.shape))).ravel(), "points": (pts + rng.normal(0, 0.005, pts.shape)).ravel()}
    K = [bal["fx"], 0.0, bal["cx"], 0.0, bal["fy"], bal["cy"], 0.0, 0.0, 1.0]
    x0 = ref64.factor_points(np.float32(bal["cameras"]).reshape(C, 6), np.float32(bal["points"]).reshape(L, 3), bal)
    E = len(cam_id)
    size = np.where(np.arange(E) % 2 == 0, rng.uniform(1.0, 4.0, E), rng.uniform(6.5, 30.0, E))
    ang = rng.uniform(0, 2 * np.pi, E)
    bal["observations"] = (ref64.project(x0, K) + size[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).ravel()
    return bal


@pytest.fixture(scope="module")
def graph_g():
    g = _Exact("G geometry", geometry_graph(), 0, cond_limit=np.inf, maxeta_damping=0.4)
    g.classes = np.asarray(GEOMETRY_CLASS)[np.asarray(g.bal["cam_id"], np.int64)]
    return g


def test_geometry_graph_has_the_shapes_it_is_for(graph_g):
    from gbp_poplar_amd import hostlib
    bal = graph_g.bal
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    assert np.diff(lay["cam_row_ptr"]).tolist() == [2] * 16 and np.all(np.bincount(bal["cam_id"]) == 17)
    cams = np.asarray(bal["cameras"]).reshape(16, 6)
    w = np.linalg.norm(cams[:, 3:], axis=1)
    assert set(GEOMETRY_CLASS) == set(range(6)) and np.all(np.abs(w / np.asarray(GEOMETRY_W)[list(GEOMETRY_CLASS)] - 1) < 0.02)
    p = ref64.factor_points(cams, np.asarray(bal["points"]).reshape(-1, 3), bal)
    depth = np.einsum("nj,nj->n", ref64.rodrigues(p[:, 3:6])[:, 2, :], p[:, 6:9]) + p[:, 2]
    assert depth.min() < 0.75 and depth.min() > 0.4 and depth.max() > 49 and depth.max() < 52, (depth.min(), depth.max())


# ---- what every part needs ---------------------------------------------------------------------------------------------------------------
def _means_of(eta, lam, width):
    """belief means in float64; NaN for a variable no factor sees (a zero prior and a zero belief: it is in no factor's x0)"""
    lam = np.asarray(lam).reshape(-1, width * width)
    seen = np.any(lam != 0, axis=1)
    out = np.full((seen.size, width), np.nan)
    out[seen] = ref64.belief_means(np.asarray(eta).reshape(-1, width)[seen], lam[seen], width)
    return out


def _means(beliefs):
    return (_means_of(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6),
            _means_of(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3))


def _per_factor_rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(b), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    return np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)


def _lin64(g, beliefs, lmk_shift=0, **wrong):
    cm, lm = _means(beliefs)
    return ref64.linearise_factor(ref64.factor_points(cm, lm, g.bal, lmk_shift), g.K, g.state["measurements"], g.state["meas_variances"],
                                  NSTDS, **wrong)


def _scaled(lin, old=None):
    """(eta, Lambda) of a float64 linearisation as the engine holds it: over mvar; `old`: accumulated onto that potential first"""
    eta, lam = lin["eta"], lin["lam"]
    if old is not None:
        eta, lam = eta + old[0], lam + old[1]
    return eta / lin["mvar"][:, None], lam / lin["mvar"][:, None, None]


def _robust_margin(lin, var):
    return np.abs(lin["err"] / (NSTDS * np.sqrt(np.asarray(var, np.float64))) - 1.0)


def _linearise_errors(x, g, what):
    """the potentials x holds against the float64 linearisation at the means of the beliefs x holds; the robust flags exactly"""
    b = x.read()
    fe, fl = x.factor_potentials()
    lin = _lin64(g, b)
    margin = _robust_margin(lin, g.state["meas_variances"]).min()
    assert margin >= ROBUST_MARGIN, margin
    assert np.array_equal(b["robust_flag"] == 1, lin["robust"]), np.nonzero((b["robust_flag"] == 1) != lin["robust"])[0]
    eta, lam = _scaled(lin)
    ee, el = _per_factor_rel(np.asarray(fe).reshape(-1, 9), eta), _per_factor_rel(ref64.blocks_of(fl), lam)
    print("E %s %s: eta %.3e  Lambda %.3e;  %d of %d robust, nearest to the threshold %.1e" % (g.name, what, ee.max(), el.max(), lin["robust"].sum(), ee.size, margin))
    return ee, el


def _worst_per_class(g, ee, el):
    if g.name[0] != "G":
        return {g.name[0]: (ee.max(), el.max())}
    return {k: (ee[g.classes == k].max(), el[g.classes == k].max()) for k in range(len(GEOMETRY_W))}


def _e_bounds(g):
    return {g.name[0]: E_ORACLE[g.name[0]]} if g.name[0] != "G" else E_ORACLE["G"]


def _run_linearise(x, g, what):
    """E's procedure: per class the larger of the two LINEARISEs' errors against its bound; on the tree, the relinearised joint"""
    x.upload(g.state)
    x.linearise()
    first = _worst_per_class(g, *_linearise_errors(x, g, what + ", first LINEARISE"))
    x.iterate(3)
    x.linearise()
    second = _worst_per_class(g, *_linearise_errors(x, g, what + ", LINEARISE under live messages"))
    worst = {k: tuple(max(a, b) for a, b in zip(first[k], second[k])) for k in first}
    print("E %s %s: %s" % (g.name, what, "  ".join("%s eta %.3e Lambda %.3e" % (k, v[0], v[1]) for k, v in worst.items())))
    _assert_linearise(worst, g, what)
    if g.name[0] == "A":                      # a tree forgets its old messages: the literal records LINEARISE left must carry the new joint
        fe, fl = x.factor_potentials()
        ex = g.exact(fe, fl)
        x.iterate(g.sweeps)
        err = g.errors(x.read(), ex)
        print("E %s %s: exact marginals of the relinearised joint: %s" % (g.name, what, "  ".join("%s %.3e" % kv for kv in err.items())))
        for k in TENSORS:
            assert err[k] <= A_BOUND[k], (what, k, err[k], A_BOUND[k])
    return worst


def _assert_linearise(worst, g, what):
    for k, (be, bl) in _e_bounds(g).items():
        assert worst[k][0] <= MARGIN * be and worst[k][1] <= MARGIN * bl, (what, g.name, k, worst[k], (MARGIN * be, MARGIN * bl))


def _graph(which, graph_a, graph_b, graph_g):
    return {"A": graph_a, "B": graph_b, "G": graph_g}[which]


# ---- E: LINEARISE --------------------------------------------------------------------------------------------------------------------------
def test_complex_step_jacobian_agrees_with_central_differences(graph_a, graph_b, graph_g):
    for g in (graph_a, graph_b, graph_g):
        x0 = ref64.factor_points(np.float32(g.bal["cameras"]).reshape(-1, 6), np.float32(g.bal["points"]).reshape(-1, 3), g.bal)
        Jc, Jd = ref64.jacobian(x0, g.K), ref64.jacobian(x0, g.K, "central")
        rel = np.max(np.abs(Jc - Jd), axis=(1, 2)) / np.max(np.abs(Jc), axis=(1, 2))
        print("%s: complex step against central differences %.2e" % (g.name, rel.max()))
        assert rel.max() <= 1e-7


@pytest.mark.parametrize("which", ["A", "B", "G"])
def test_oracle_linearise_against_float64(which, graph_a, graph_b, graph_g, oracle_mod):
    g = _graph(which, graph_a, graph_b, graph_g)
    _run_linearise(_oracle(oracle_mod, g.bal, g.K, **g.params), g, "oracle")


# (B's four cameras are one row each: nothing for row placement to move, as in test_exact_inference)
E_CASES = [(w, p) for w in ("A", "B", "G") for p in EXACT_PATHS if (w, p) != ("B", "rows_placed")]


@gpu
@pytest.mark.parametrize("which, path", E_CASES, ids=["%s-%s" % wp for wp in E_CASES])
def test_linearise_against_float64_on_the_gpu(which, path, graph_a, graph_b, graph_g, rounded_trig):
    g = _graph(which, graph_a, graph_b, graph_g)
    _run_linearise(_gpu_path(path, g.bal, g.K, **g.params), g, path)


WRONG = {"first_order_rotation": dict(first_order_rotation=True), "no_huber": dict(no_huber=True), "flip_residual": dict(flip_residual=True),
         "lmk_shift": dict(lmk_shift=1)}


HUBER_CLEAR = 1.1


def _huber_clear(lin, var):
    """the factors no_huber is wrong on by a visible amount: robust, and at least 10 % over the threshold.  Huber's rescale
    var / mvar = (2 u - 1) / u^2, u = err / (nstds sigma), is continuous at the threshold: at u = 1.1 it is 0.83 % off 1, and as u -> 1
    no bound tells it from none"""
    return lin["robust"] & (lin["err"] >= HUBER_CLEAR * NSTDS * np.sqrt(np.asarray(var, np.float64)))


def _wrong_ratio(right, wrong, bound):
    """per factor: how far the wrong linearisation lies from the right one, in the tests' measure over the bound, on its best tensor"""
    (re, rl), (we, wl) = right, wrong
    return np.maximum(_per_factor_rel(we, re) / bound[0], _per_factor_rel(wl, rl) / bound[1])


@pytest.mark.parametrize("which", ["A", "B", "G"])
def test_linearise_bounds_are_not_blind(which, graph_a, graph_b, graph_g, oracle_mod):
    """In float64 alone, at the means the oracle holds at both LINEARISEs of E: each wrong variant of linearise_factor lies at least
    100 x the bound away, on its best tensor, on at least 90 % of the factors it concerns (no Huber rescale is wrong on the robust
    factors at least 10 % over the threshold, _huber_clear, and is counted among those).  The 10 % are a cap, not a measurement: they
    cover the camera with |w| = 1e-3, whose first-order rotation block is off by |w| / 2 only, landmarks near the rotation axis, where
    the second order of the rotation vanishes, and residuals that are small beside J x0 (measured: at least 91.6 % everywhere)."""
    g = _graph(which, graph_a, graph_b, graph_g)
    orc = _oracle(oracle_mod, g.bal, g.K, **g.params)
    orc.upload(g.state)
    orc.linearise()
    for stage in ("first", "live"):
        if stage == "live":
            orc.iterate(3)
            orc.linearise()
        b = orc.read()
        lin = _lin64(g, b)
        right = _scaled(lin)
        if which == "G":
            bound = (MARGIN * np.asarray([E_ORACLE["G"][k][0] for k in g.classes]), MARGIN * np.asarray([E_ORACLE["G"][k][1] for k in g.classes]))
        else:
            bound = _bound(E_ORACLE[which])
        for name, kw in WRONG.items():
            ratio = _wrong_ratio(right, _scaled(_lin64(g, b, **kw)), bound)
            if name == "no_huber":
                ratio = ratio[_huber_clear(lin, g.state["meas_variances"])]
            if not ratio.size:                # (B under live messages has no robust factor)
                continue
            frac = float(np.mean(ratio >= 100.0))
            print("E %s %s %-20s: %5.1f %% of %d factors at least 100 x the bound away (median ratio %.0f, smallest %.1f)"
                  % (g.name, stage, name, 100 * frac, ratio.size, np.median(ratio), ratio.min()))
            assert frac >= 0.9, (which, stage, name, frac)


# ---- F: relinearising sweeps -----------------------------------------------------------------------------------------------------------
ROWS_SEED = 38     # of the measurement noise added to the row graph: see _f_graph


def _f_graph(which):
    """B, or the row graph of C with measurement noise added: 0 .. 2 px on even factors, 8 .. 16 px on odd ones.  As it stands one of
    the row graph's 1 058 factors comes within 2e-5 of the Huber threshold in a relinearising sweep, where float32 may decide the
    robust flag either way, and its residuals of about 2 px beside J x0 of about 30 px leave a flipped residual less than 100 x the
    bound away on most factors.  With 5 relinearising sweeps of up to 1 058 factors on four legs, a factor within 1e-4 of the threshold
    is the rule, not the exception: of the seeds 0 .. 39 this one keeps every relinearising factor at least 1.9e-4 away on all legs
    (asserted in run())."""
    bal = all_to_all(4, 12) if which == "B" else row_graph()
    K, state = _inputs(bal)
    E = bal["n_edges"]
    if which == "rows":
        rng = np.random.default_rng(ROWS_SEED)
        size = np.where(np.arange(E) % 2 == 0, rng.uniform(0.0, 2.0, E), rng.uniform(8.0, 16.0, E))
        ang = rng.uniform(0, 2 * np.pi, E)
        state = dict(state, measurements=(state["measurements"].reshape(E, 2) + np.float32(size[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))).ravel())
    state = dict(state, damping_count=np.asarray([2, 1, -3], np.int32)[np.arange(E) % 3])
    return bal, K, state


def _third_inactive(E):
    return np.where(np.isin(np.arange(E) % 9, (0, 4, 8)), 0, 1).astype(np.uint32)      # one of each residue of e % 3 in every nine


class _Relin:
    """the state F carries from sweep to sweep: one graph, one relin_mode, one leg"""

    def __init__(self, which, mode, inactive):
        self.which, self.mode = which, mode
        self.bal, self.K, self.state = _f_graph(which)
        if inactive:
            self.state = dict(self.state, active_flag=_third_inactive(self.bal["n_edges"]))
        self.params = dict(dmu_threshold=1e30, relin_mode=mode)
        self.active = np.asarray(self.state["active_flag"]) == 1
        self.name = "%s relin_mode %d%s" % (which, mode, ", a third inactive" if inactive else "")

    def predict(self, count):
        """from integers alone: (the factors that relinearise in the next sweep, the counts after it)"""
        bumped = count + 1
        relin = self.active & (bumped > MIN_LINEAR - UNDAMPED)
        return relin, np.where(relin, -UNDAMPED, np.where(self.active, bumped, count)).astype(np.int32)

    def run(self, x, what):
        """14 single sweeps; returns the largest (eta, Lambda) error of a relinearised factor and the end state"""
        x.upload(self.state)
        x.linearise()
        worst, sets, self.margin = np.zeros(2), [], np.inf
        seen = np.zeros(self.bal["n_edges"], bool)
        for sweep in range(1, F_SWEEPS + 1):
            b = x.read()
            fe, fl = x.factor_potentials()
            old = (np.asarray(fe, np.float64).reshape(-1, 9), ref64.blocks_of(fl))
            relin, count = self.predict(b["damping_count"])
            x.iterate(1)
            after = x.read()
            ge, gl = x.factor_potentials()
            assert np.array_equal(after["damping_count"], count), (what, sweep)
            assert x.eval()["n_relin"] == int(relin.sum()), (what, sweep, x.eval()["n_relin"], int(relin.sum()))
            keep = ~relin
            assert np.array_equal(np.asarray(ge).reshape(-1, 9)[keep], np.asarray(fe).reshape(-1, 9)[keep]), (what, sweep)
            assert np.array_equal(np.asarray(gl).reshape(-1, 81)[keep], np.asarray(fl).reshape(-1, 81)[keep]), (what, sweep)
            sets.append(int(relin.sum()))
            if not relin.any():
                continue
            seen |= relin
            lin = ref64.linearise_factor(ref64.factor_points(*_means(b), self.bal)[relin], self.K,
                                         np.asarray(self.state["measurements"]).reshape(-1, 2)[relin],
                                         np.asarray(self.state["meas_variances"])[relin], NSTDS)
            margin = _robust_margin(lin, np.asarray(self.state["meas_variances"])[relin]).min()
            self.margin = min(self.margin, margin)
            assert margin >= ROBUST_MARGIN, (what, sweep, margin)
            eta, lam = _scaled(lin, None if self.mode == 1 else (old[0][relin], old[1][relin]))
            err = (_per_factor_rel(np.asarray(ge).reshape(-1, 9)[relin], eta).max(), _per_factor_rel(ref64.blocks_of(gl)[relin], lam).max())
            print("F %s %s sweep %2d: %3d factors relinearise, eta %.3e  Lambda %.3e" % (self.name, what, sweep, relin.sum(), err[0], err[1]))
            assert np.array_equal(after["robust_flag"][relin] == 1, lin["robust"]), (what, sweep)
            worst = np.maximum(worst, err)
        assert np.array_equal(seen, self.active) and sum(n > 0 for n in sets) >= 5, sets      # every active factor, in five different sweeps
        return worst, (x.read(), x.factor_potentials())


F_CASES = [pytest.param(m, i, id="relin_mode_%d%s" % (m, "_inactive" if i else "")) for m in (0, 1) for i in (False, True)]


@pytest.mark.parametrize("mode, inactive", F_CASES)
@pytest.mark.parametrize("which", ["B", "rows"])
def test_oracle_relinearising_sweeps_against_float64(which, mode, inactive, oracle_mod):
    r = _Relin(which, mode, inactive)
    worst, _ = r.run(_oracle(oracle_mod, r.bal, r.K, **r.params), "oracle")
    print("F %s oracle: eta %.3e  Lambda %.3e" % (r.name, worst[0], worst[1]))
    be, bl = _bound(F_ORACLE[which, mode])
    assert worst[0] <= be and worst[1] <= bl, (worst, be, bl)


F_PATHS = [("B", p) for p in ("two_kernels", "library_choice", "per_factor_mu", "seg_skip", "shards_2", "shards_3")] + [("rows", "rows_placed")]


def _same_state(a, b):
    (ra, (ea, la)), (rb, (eb, lb)) = a, b
    for k in ra:
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    assert np.array_equal(ea, eb) and np.array_equal(la, lb)


@gpu
@pytest.mark.parametrize("mode, inactive", F_CASES)
@pytest.mark.parametrize("which, path", F_PATHS, ids=["%s-%s" % wp for wp in F_PATHS])
def test_relinearising_sweeps_against_float64_on_the_gpu(which, path, mode, inactive, rounded_trig):
    r = _Relin(which, mode, inactive)
    worst, end = r.run(_gpu_path(path, r.bal, r.K, **r.params), path)
    print("F %s %s: eta %.3e  Lambda %.3e" % (r.name, path, worst[0], worst[1]))
    be, bl = _bound(F_ORACLE[which, mode])
    assert worst[0] <= be and worst[1] <= bl, (path, worst, be, bl)
    if path == "library_choice":              # the same 14 sweeps in one burst: the persistent kernel relinearises inside one launch
        x = _gpu_path(path, r.bal, r.K, **r.params)
        x.upload(r.state)
        x.linearise()
        x.iterate(F_SWEEPS)
        _same_state((x.read(), x.factor_potentials()), end)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["B", "rows"])
def test_relinearising_bounds_are_not_blind(which, mode, oracle_mod):
    """float64 alone, at the oracle's pre-sweep means of every sweep that relinearises: as for E, on the factors that relinearise"""
    r = _Relin(which, mode, False)
    orc = _oracle(oracle_mod, r.bal, r.K, **r.params)
    orc.upload(r.state)
    orc.linearise()
    bound = _bound(F_ORACLE[which, mode])
    fewest = {k: 1.0 for k in WRONG}
    for sweep in range(1, F_SWEEPS + 1):
        b = orc.read()
        relin, _ = r.predict(b["damping_count"])
        if relin.any():
            fe, fl = orc.factor_potentials()
            old = None if mode == 1 else (np.asarray(fe, np.float64).reshape(-1, 9), ref64.blocks_of(fl))
            lin = _lin64(r, b)
            right = _scaled(lin, old)
            for name, kw in WRONG.items():
                ratio = _wrong_ratio(right, _scaled(_lin64(r, b, **kw), old), bound)
                ratio = ratio[relin & _huber_clear(lin, r.state["meas_variances"])] if name == "no_huber" else ratio[relin]
                if ratio.size:
                    fewest[name] = min(fewest[name], float(np.mean(ratio >= 100.0)))
        orc.iterate(1)
    print("F %s relin_mode %d: smallest share of relinearising factors at least 100 x the bound away: %s"
          % (which, mode, "  ".join("%s %.1f %%" % (k, 100 * v) for k, v in fewest.items())))
    for name, frac in fewest.items():
        assert frac >= 0.9, (name, frac)


# ---- G: converged relinearising GBP is a stationary point -------------------------------------------------------------------------------
def _b_inactive_flags(bal):
    """16 of B's 48 factors inactive: all four factors of landmark 5 and twelve others, no other landmark left with fewer than two"""
    E = bal["n_edges"]
    lmk, cam = np.asarray(bal["lmk_id"], np.int64), np.asarray(bal["cam_id"], np.int64)
    off = (lmk == 5) | ((lmk != 5) & ((lmk + cam) % 4 == 0)) | ((lmk == 0) & (cam == 1))
    flags = np.where(off, 0, 1).astype(np.uint32)
    assert flags.size == E and int(np.sum(flags == 0)) == 16, int(np.sum(flags == 0))
    return flags


G_OUTLIER_PX = 20.0      # added to both coordinates of every seventh measurement of G's graph: see _g_graph


def _g_graph(config, mode=1):
    """B (config "inactive": with 16 factors inactive) with outliers among its measurements.  As it stands B has no robust factor at
    the converged means: the Huber rescale is then not in the cost at all (the gradient without it is the same number), and the
    first-order rotation reaches only 49 x the bound.  With the outliers 9 (16) factors stay robust and every wrong variant lies more
    than 100 x the bound away (test_stationarity_bound_is_not_blind)."""
    bal = all_to_all(4, 12)
    K, state = _inputs(bal)
    z = np.array(state["measurements"]).reshape(-1, 2)
    z[np.arange(len(z)) % 7 == 3] += np.float32(G_OUTLIER_PX)
    state = dict(state, measurements=z.ravel())
    if config == "inactive":
        state = dict(state, active_flag=_b_inactive_flags(bal))
    return bal, K, state, dict(dmu_threshold=1e30, relin_mode=mode)


def _stationarity(x, bal, K, state, **wrong):
    g, s = ref64.cost_gradient(_means(x.read()), bal, K, state, NSTDS, **wrong)
    return float(np.max(np.abs(g) / s))


def _run_stationarity(x, bal, K, state, what):
    x.upload(state)
    x.linearise()
    start = _stationarity(x, bal, K, state)
    x.iterate(G_SWEEPS)
    end = _stationarity(x, bal, K, state)
    print("G %s: relative gradient of the float64 Huber cost %.3e at the start, %.3e after %d sweeps" % (what, start, end, G_SWEEPS))
    return start, end


@pytest.mark.parametrize("config", ["all", "inactive"])
def test_oracle_converges_to_a_stationary_point(config, oracle_mod):
    bal, K, state, params = _g_graph(config)
    start, end = _run_stationarity(_oracle(oracle_mod, bal, K, **params), bal, K, state, "oracle, %s" % config)
    assert end <= MARGIN * G_ORACLE[config], (end, MARGIN * G_ORACLE[config])
    assert start >= 1e4 * MARGIN * G_ORACLE[config], start
    bal, K, state, params = _g_graph(config, mode=0)
    _, acc = _run_stationarity(_oracle(oracle_mod, bal, K, **params), bal, K, state, "oracle, %s, relin_mode 0" % config)
    assert acc > G_ACCUMULATING_STAYS_ABOVE, acc


@pytest.mark.parametrize("config", ["all", "inactive"])
def test_stationarity_bound_is_not_blind(config, oracle_mod):
    """the float64 gradient with each wrong variant, at the oracle's converged means, is at least 100 x the bound"""
    bal, K, state, params = _g_graph(config)
    orc = _oracle(oracle_mod, bal, K, **params)
    orc.upload(state)
    orc.linearise()
    orc.iterate(G_SWEEPS)
    for name, kw in WRONG.items():
        v = _stationarity(orc, bal, K, state, **kw)
        print("G %s %-20s: relative gradient %.3e = %.0f x the bound" % (config, name, v, v / (MARGIN * G_ORACLE[config])))
        assert v >= 100.0 * MARGIN * G_ORACLE[config], (name, v)


@gpu
@pytest.mark.parametrize("path", EXACT_PATHS[:-1])
@pytest.mark.parametrize("config", ["all", "inactive"])
def test_converges_to_a_stationary_point_on_the_gpu(config, path, rounded_trig):
    bal, K, state, params = _g_graph(config)
    start, end = _run_stationarity(_gpu_path(path, bal, K, **params), bal, K, state, "%s, %s" % (path, config))
    assert end <= MARGIN * G_ORACLE[config], (path, end, MARGIN * G_ORACLE[config])
    assert start >= 1e4 * MARGIN * G_ORACLE[config], start


# ---- H: prior weakening on the tree --------------------------------------------------------------------------------------------------------
def _frac(n, mult):
    return np.modf(np.arange(n) * mult)[0]


@pytest.fixture(scope="module")
def graph_w(graph_a):
    """A with milder scalings than the default 0.158, which multiplies the joint's condition by 6.3 per weakening: per variable in
    [0.6, 0.9], the cameras' and the landmarks' different, and weaken flags spread over 0 .. 5"""
    bal = graph_a.bal
    C, L = bal["n_cams"], bal["n_lmks"]
    state = dict(cam_scaling=np.float32(0.6 + 0.3 * _frac(C, 0.6180339887)), lmk_scaling=np.float32(0.62 + 0.27 * _frac(L, 0.7548776662)),
                 cam_weaken_flag=((np.arange(C) * 5 + 1) % 6).astype(np.uint32), lmk_weaken_flag=((np.arange(L) * 5 + 4) % 6).astype(np.uint32))
    g = _Exact("A hub tree, weakened", bal, graph_a.sweeps, state=state, cond_limit=H_COND_LIMIT, maxeta_damping=0.0)
    assert set(state["cam_weaken_flag"].tolist()) == set(range(6)) == set(state["lmk_weaken_flag"].tolist())
    assert not set(np.round(state["cam_scaling"], 6).tolist()) & set(np.round(state["lmk_scaling"], 6).tolist())
    return g


PRIORS = (("cam_priors_eta", "cam", 6), ("cam_priors_lambda", "cam", 36), ("lmk_priors_eta", "lmk", 3), ("lmk_priors_lambda", "lmk", 9))


def _weakened64(state, k):
    """the uploaded priors times scaling^min(flag, k), in float64"""
    out = dict(state)
    for name, var, width in PRIORS:
        s = np.asarray(state[var + "_scaling"], np.float64) ** np.minimum(np.asarray(state[var + "_weaken_flag"], np.int64), k)
        out[name] = (np.asarray(state[name], np.float64).reshape(-1, width) * s[:, None]).ravel()
    return out


def _check_priors(x, state, k, what):
    got, want = x.read_priors(), _weakened64(state, k)
    for name, var, width in PRIORS:
        w32 = np.float32(want[name])
        ulps = np.abs(np.asarray(got[name], np.float64) - want[name]) / np.spacing(np.abs(w32)).astype(np.float64)
        assert np.nanmax(np.where(w32 == 0, 0.0, ulps)) <= 4.0 and np.all(got[name][w32 == 0] == 0), (what, k, name, np.nanmax(ulps))
        still = np.repeat(np.asarray(state[var + "_weaken_flag"]) == 0, width)
        assert still.any() and np.array_equal(got[name][still], np.asarray(state[name])[still]), (what, k, name)


def _run_weakening(x, g, what, weaken=None):
    """upload, LINEARISE; three times: weaken, diameter + 2 sweeps, priors and exact marginals; then weakenings 4 .. 6 for the priors
    alone (the flags are spent one by one, the last at the fifth call)"""
    x.upload(g.state)
    x.linearise()
    fe, fl = x.factor_potentials()
    errs = {}
    for k in (1, 2, 3):
        if weaken is None:
            x.weaken_priors()
            x.iterate(g.sweeps)
        else:
            weaken(x, g.sweeps)
        _check_priors(x, g.state, k, what)
        ex = g.exact(fe, fl, state=_weakened64(g.state, k), key=k)
        errs[k] = g.errors(x.read(), ex)
        print("H %s %s after %d weakenings (condition %.0f): %s" % (g.name, what, k, ex["cond"], "  ".join("%s %.3e" % kv for kv in errs[k].items())))
    for k in (4, 5, 6):
        x.weaken_priors()
        _check_priors(x, g.state, k, what)
    return errs


def _assert_weakening(errs, what):
    for k, err in errs.items():
        for t in TENSORS:
            assert err[t] <= MARGIN * H_WEAKEN_ORACLE[k][t], (what, k, t, err[t], MARGIN * H_WEAKEN_ORACLE[k][t])


def test_oracle_prior_weakening_is_exact(graph_w, oracle_mod):
    _assert_weakening(_run_weakening(_oracle(oracle_mod, graph_w.bal, graph_w.K, **graph_w.params), graph_w, "oracle"), "oracle")


def _weaken_in_the_loop(x, sweeps):
    """passes 0 .. sweeps of the reference's loop with steps = 1 in ONE call without the metric: pass 0 does not weaken, pass 1 does, no
    later one.  A weakening in front of a call's first pass is a launch of its own; this one lies inside the launch, where on a graph
    this small the persistent kernel weakens in registers.  (The sweep in front of it changes nothing: the tree is exact `sweeps`
    sweeps after the weakening whatever its messages were.)"""
    x.ba_loop(sweeps + 1, 0, 1, metrics=False)


@gpu
@pytest.mark.parametrize("path", ["two_kernels", "library_choice", "library_choice_ba_loop", "shards_2"])
def test_prior_weakening_is_exact_on_the_gpu(path, graph_w, rounded_trig):
    x = _gpu_path(path.replace("_ba_loop", ""), graph_w.bal, graph_w.K, **graph_w.params)
    _assert_weakening(_run_weakening(x, graph_w, path, _weaken_in_the_loop if path.endswith("ba_loop") else None), path)


def test_weakening_bounds_are_not_blind(graph_w, oracle_mod):
    """float64 alone: a prior scaled one time too few, on ANY one variable that the k-th call weakens, moves that variable's exact
    marginal by at least 100 x the bound, on its best tensor (by the Woodbury identity on the variable's own block)"""
    g = graph_w
    orc = _oracle(oracle_mod, g.bal, g.K, **g.params)
    orc.upload(g.state)
    orc.linearise()
    fe, fl = orc.factor_potentials()
    C = g.bal["n_cams"]
    for k in (1, 2, 3):
        st = _weakened64(g.state, k)
        ex = g.exact(fe, fl, state=st, key=k)
        bound = {t: MARGIN * H_WEAKEN_ORACLE[k][t] for t in TENSORS}
        least = np.inf
        for var, width, off in (("cam", 6, 0), ("lmk", 3, 6 * C)):
            flag, s = np.asarray(g.state[var + "_weaken_flag"], np.int64), np.asarray(g.state[var + "_scaling"], np.float64)
            for v in np.nonzero(flag >= k)[0]:
                idx = slice(off + width * v, off + width * v + width)
                dL = st[var + "_priors_lambda"].reshape(-1, width, width)[v] * (1.0 / s[v] - 1.0)      # one scaling too few
                de = st[var + "_priors_eta"].reshape(-1, width)[v] * (1.0 / s[v] - 1.0)
                Svv, mv = ex["Sigma"][idx, idx], ex["mean"][idx]
                S2 = Svv - Svv @ np.linalg.solve(np.eye(width) + dL @ Svv, dL) @ Svv
                m2 = mv - (Svv - S2) @ np.linalg.solve(Svv, mv) + S2 @ de
                moved = max(per_var_rel(m2, mv, width) / bound[var + "_mean"],
                            per_var_rel(np.linalg.inv(S2), np.linalg.inv(Svv), width * width) / bound[var + "_lambda"])
                least = min(least, moved)
        print("H weakening %d: one scaling too few moves the variable's marginal by at least %.0f x the bound" % (k, least))
        assert least >= 100.0, (k, least)


# ---- H: inactive factors and their activation --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_i():
    bal = all_to_all(4, 12)
    return _Exact("B loopy 4x12, 16 inactive", bal, H_SWEEPS, state=dict(active_flag=_b_inactive_flags(bal)), maxeta_damping=0.4)


def _run_inactive(x, g, what):
    bal, state = g.bal, g.state
    off = np.asarray(state["active_flag"]) == 0
    assert np.all(off[np.asarray(bal["lmk_id"]) == 5]) and off.sum() == 16
    x.upload(state)
    x.linearise()
    fe, fl = x.factor_potentials()
    x.iterate(g.sweeps)
    b = x.read()
    first = g.errors(b, g.exact(fe, fl))
    assert np.array_equal(b["lmk_beliefs_eta"][15:18], state["lmk_priors_eta"][15:18])                 # no active factor: the prior, untouched
    assert np.array_equal(b["lmk_beliefs_lambda"][45:54], state["lmk_priors_lambda"][45:54])
    for k, m in x.messages().items():
        assert not np.any(m.reshape(off.size, -1)[off]), (what, k)
    x.new_keyframe({"active_flag": np.ones(off.size, np.uint32)})
    x.iterate(g.sweeps)
    second = g.errors(x.read(), g.exact(fe, fl, state=dict(state, active_flag=np.ones(off.size, np.uint32)), key="activated"))
    print("H %s %s: 16 inactive: %s;  after their activation: %s" % (g.name, what, "  ".join("%s %.3e" % (k, first[k]) for k in B_INACTIVE_ORACLE),
                                                                      "  ".join("%s %.3e" % (k, second[k]) for k in B_ACTIVATED_ORACLE)))
    return first, second


def _assert_inactive(first, second, what):
    for k in B_INACTIVE_ORACLE:
        assert first[k] <= MARGIN * B_INACTIVE_ORACLE[k], (what, k, first[k])
        assert second[k] <= MARGIN * B_ACTIVATED_ORACLE[k], (what, k, second[k])


def test_oracle_inactive_factors_and_their_activation(graph_i, oracle_mod):
    _assert_inactive(*_run_inactive(_oracle(oracle_mod, graph_i.bal, graph_i.K, **graph_i.params), graph_i, "oracle"), "oracle")


@gpu
@pytest.mark.parametrize("path", ["two_kernels", "library_choice", "shards_2"])
def test_inactive_factors_and_their_activation_on_the_gpu(path, graph_i, rounded_trig):
    _assert_inactive(*_run_inactive(_gpu_path(path, graph_i.bal, graph_i.K, **graph_i.params), graph_i, path), path)


def test_inactive_bounds_are_not_blind(graph_i, oracle_mod):
    """float64 alone: leaving any one active factor out of the joint with 16 inactive, and any one factor out of the full joint the
    activation leads to, moves the exact means by at least 100 x the bound (an activated factor left inactive is such a factor)"""
    g = graph_i
    orc = _oracle(oracle_mod, g.bal, g.K, **g.params)
    orc.upload(g.state)
    orc.linearise()
    fe, fl = orc.factor_potentials()
    E = g.bal["n_edges"]
    for name, state, oracle_err in ((None, g.state, B_INACTIVE_ORACLE), ("activated", dict(g.state, active_flag=np.ones(E, np.uint32)), B_ACTIVATED_ORACLE)):
        ex = g.exact(fe, fl, state=state, key=name)
        least = np.inf
        for e in np.nonzero(np.asarray(state["active_flag"]) == 1)[0]:
            moved = _moved_by_leaving_out(g, ex, fe, fl, int(e))
            least = min(least, max(moved[k] / (MARGIN * oracle_err[k]) for k in oracle_err))
        print("H %s: one missing factor moves the exact means by at least %.0f x the bound" % (name or "inactive", least))
        assert least >= 100.0, (name, least)
