"""Sweeps, beliefs and the metric against float64 exact inference (tests/ref64.py), and the data-dependent edges of the belief
kernel bit for bit against the oracle.

The other GPU tests compare the kernels with oracle/, a restatement of the same vertices: an error of meaning made in both passes them
all.  Gaussian belief propagation has an answer that needs neither.  With the potentials held fixed (dmu_threshold = 0: no factor ever
relinearises) it computes, on a tree, the exact marginals of the joint Gaussian after as many sweeps as the tree's diameter; on a loopy
graph its means — not its precisions — converge to the exact means.  The joint is built from the potentials the engine under test holds
after LINEARISE, so trig conventions do not enter.

  A  hub tree: exact means and precisions on every variable, through every gather / row / rank edge of k_beliefs
  B  loopy 4 x 12: exact means after 160 damped sweeps; the precisions must NOT be exact
  C  gather and row boundaries on loopy graphs, bit for bit against the oracle (a tree cannot take every shape)
  D  the metric per factor and as a sum against float64

HOW THE BOUNDS WERE SET.  The CPU oracle (restatement, device summation order) ran the final graphs at the final sweep counts; its
error against ref64 is *_ORACLE below, per tensor, in the per-variable inf-norm of conftest.per_var_rel (D: absolute pixels).  The
bound every engine has to meet is 8 x that (A, B) and 4 x that (D): the margin covers paths whose float32 additions are ordered
differently from the oracle's (rank order of sharded sums, the literal mu path), a few ulps; an error
of meaning shows at 1e-3 and more.  That the bounds are not blind is itself asserted, in float64 on the CPU: taking ANY single factor
out of the joint moves the exact marginals by at least 100 x the bound (A, B), and the metric with the rotation transposed or the
landmark index shifted by one lies at least 100 x the bound away (D).  profiles/exact_inference.md has the same figures and the
device's.
"""
import numpy as np
import pytest

from oracle import oracle as orc_build
from tests import ref64
from tests.conftest import per_var_rel
from tests.test_gpu_parity import _FakeDist, _assert_state_equal, _tiny_problem

gpu = pytest.mark.gpu

TENSORS = ("cam_mean", "lmk_mean", "cam_lambda", "lmk_lambda")

# ---- measured on the CPU oracle (restatement, sum order 1) against ref64; see the module docstring ------------------------------
A_SWEEPS_OVER_DIAMETER = 2
A_ORACLE = {"cam_mean": 1.420e-6, "lmk_mean": 7.039e-6, "cam_lambda": 8.574e-8, "lmk_lambda": 1.554e-7}      # after 16 + 2 sweeps
B_SWEEPS = 160
B_ORACLE = {"cam_mean": 5.153e-8, "lmk_mean": 3.384e-7}      # (its Lambdas are 24 % and 21 % off the marginal precisions, as they should be)
D_ORACLE = {"term_norm": 2.715e-5, "term_half_sq": 5.899e-5, "mean_norm": 6.593e-7, "mean_half_sq": 2.300e-6}      # on terms of 1 .. 6 px
A_BOUND = {k: 8.0 * v for k, v in A_ORACLE.items()}
B_BOUND = {k: 8.0 * v for k, v in B_ORACLE.items()}
D_BOUND = {k: 4.0 * v for k, v in D_ORACLE.items()}      # pixels (norm) and pixels^2 (half square): per factor / per factor of the sum
# 2-norm condition of the joints, measured: A 2516, B 26.7 (the cameras of _tiny_problem recede with their index, from depth 5 to depth 30
# on A's 126, and an observation's information falls with the square of the depth).  The limits keep float32 eps x condition — the most
# round-off can be amplified by, 6e-8 x 4000 = 2.4e-4 — below the 1e-3 at which an error of meaning shows; the bounds themselves are far
# tighter, and what they can see is asserted directly (test_bounds_are_not_blind_to_a_missing_factor).
COND_LIMIT = {"A": 4000.0, "B": 100.0}
B_LAMBDA_GAP = 0.01         # loopy GBP's precisions are not the marginal precisions: they must differ by more than this


# ---- the graphs ---------------------------------------------------------------------------------------------------------------
HUB_DEGREES = (2, 10, 11, 15, 16, 23, 24, 32)
CAM_COUNTS = (16, 17, 256, 257, 272, 273)      # factor counts of the cameras that carry leaves (+ cameras of 1 and 2 factors)


def _sorted_by_camera(cam_id, lmk_id):
    order = np.lexsort((lmk_id, cam_id))
    return np.asarray(cam_id)[order].tolist(), np.asarray(lmk_id)[order].tolist()


def hub_tree():
    """Eight hub landmarks of the degrees at which the landmark gather of k_beliefs changes path (ten loads; five more where any lane of
    the wave has more than 10; rounds of eight through lmk_fpos beyond slot 15), chained so that consecutive hubs share exactly one
    camera; leaf landmarks of degree 1 bring chosen cameras to the factor counts at which the camera row loop changes path (rows of 16
    in batches of 16 with a clamped tail).  A tree: 126 cameras, a diameter of 16 factor hops.
    Landmark ids: hub i sits among the leaves of the i-th group of 16 (a wave with one long and many short gathers), the groups
    behind hold leaves only (the wave that skips the second batch), and there are far more than the 64 landmarks of one workgroup."""
    hub_cams, n_cams = [], 0
    for i, d in enumerate(HUB_DEGREES):
        first = n_cams - 1 if i else 0          # the previous hub's last camera is shared
        hub_cams.append(list(range(first, first + d)))
        n_cams = first + d
    hub_id = [16 * i + (2 * i + 1) % 16 for i in range(len(HUB_DEGREES))]
    shared = {cams[-1] for cams in hub_cams[:-1]}
    # one camera with one hub factor in each of hubs 1..6 takes the leaves that bring it to the wanted count; the camera shared by
    # hubs 6 and 7 (two hub factors) gets 14 leaves: 16 factors, one full row, on the tree's spine
    leaves_of = {hub_cams[i + 1][1]: CAM_COUNTS[i] - 1 for i in range(len(CAM_COUNTS))}
    leaves_of[hub_cams[6][-1]] = 14
    assert not (set(leaves_of) - {hub_cams[6][-1]}) & shared
    cam_id, lmk_id = [], []
    for h, cams in zip(hub_id, hub_cams):
        cam_id += cams
        lmk_id += [h] * len(cams)
    nxt = 0
    for c, n in sorted(leaves_of.items()):
        for _ in range(n):
            while nxt in hub_id:
                nxt += 1
            cam_id.append(c)
            lmk_id.append(nxt)
            nxt += 1
    n_lmks = nxt
    cam_id, lmk_id = _sorted_by_camera(cam_id, lmk_id)
    return _tiny_problem(cam_id, lmk_id, n_cams, n_lmks), hub_id


def diameter(bal):
    """largest variable-to-variable distance in factor hops (breadth-first from every hub end is enough on a tree: twice from anywhere)"""
    C = bal["n_cams"]
    nbr = [[] for _ in range(C + bal["n_lmks"])]
    for c, l in zip(bal["cam_id"].tolist(), bal["lmk_id"].tolist()):
        nbr[c].append(C + l)
        nbr[C + l].append(c)

    def far(src):
        dist = {src: 0}
        todo = [src]
        for v in todo:
            for w in nbr[v]:
                if w not in dist:
                    dist[w] = dist[v] + 1
                    todo.append(w)
        assert len(dist) == len(nbr), "the graph is not connected"
        v = max(dist, key=dist.get)
        return v, dist[v]
    return far(far(0)[0])[1]


def all_to_all(n_cams, n_lmks):
    cam_id = np.repeat(np.arange(n_cams), n_lmks)
    lmk_id = np.tile(np.arange(n_lmks), n_cams)
    return _tiny_problem(cam_id.tolist(), lmk_id.tolist(), n_cams, n_lmks)


GATHER_KINDS = (0, 1, 2, 9, 10, 11, 14, 15, 16, 17, 22, 23, 24, 31, 32, 40)


def gather_graph():
    """80 landmarks whose degree goes by l % 16 through every gather boundary, then 16 of degree <= 10 (a group that skips the second
    batch); 40 cameras, a landmark's observations start at a camera that rotates with l so that the cameras' rows stay ragged"""
    n_cams = 40
    deg = [GATHER_KINDS[l % 16] for l in range(80)] + [(3 * l) % 11 for l in range(16)]
    cam_id, lmk_id = [], []
    for l, d in enumerate(deg):
        cam_id += [(7 * l + j) % n_cams for j in range(d)]
        lmk_id += [l] * d
    cam_id, lmk_id = _sorted_by_camera(cam_id, lmk_id)
    bal = _tiny_problem(cam_id, lmk_id, n_cams, len(deg))
    assert np.array_equal(np.bincount(bal["lmk_id"], minlength=len(deg)), deg) and np.all(np.bincount(bal["cam_id"], minlength=n_cams) > 0)
    return bal


ROW_COUNTS = (0, 1, 16, 17, 256, 257, 272, 273, 512, 513, 528, 529)


def row_graph():
    """cameras of 0, 1, 1, 2, 16, 17, 17, 18, 32, 33, 33 and 34 rows: a camera with n factors sees landmarks 0 .. n - 1"""
    cam_id = sum(([c] * n for c, n in enumerate(ROW_COUNTS)), [])
    lmk_id = sum((list(range(n)) for n in ROW_COUNTS), [])
    return _tiny_problem(cam_id, lmk_id, len(ROW_COUNTS), max(ROW_COUNTS))


# ---- the paths: everything that can run the program list ------------------------------------------------------------------------
def _inputs(bal):
    from gbp_poplar_amd import driver, hostlib
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    return K, state


def _params(**kw):
    from gbp_poplar_amd import _cabi
    return _cabi.GbpParams.defaults(**kw)


def _oracle(oracle_mod, bal, K, bounds=None, **kw):
    orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_params(**kw))
    orc.set_sum_order(1, bounds)
    return orc


class _Shards:
    """`world` landmark-shard contexts on one GPU, the exchange done by device copies (the _FakeDist pattern), under the verbs of an
    engine; read() and factor_potentials() put every shard's own landmarks / factors together"""

    def __init__(self, bal, K, world, **kw):
        from gbp_poplar_amd.distributed import ShardedGbp, landmark_partition
        from gbp_poplar_amd.engine import GbpEngine
        self.bal, self.world, self.hooks, self.E = bal, world, True, len(bal["cam_id"])
        self.bounds = landmark_partition(bal["lmk_id"], bal["n_lmks"], world)
        self.fake = _FakeDist()
        self.shards = []
        for r in range(world):
            eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_params(**kw), hooks=True,
                            shard=(r, world, int(self.bounds[r]), int(self.bounds[r + 1])))
            sh = ShardedGbp(eng, bal["n_cams"], r, world, dist=None, device="cuda")
            sh._exchange = lambda: None          # the exchange is performed for all shards at once
            self.fake.members.append(sh)
            self.shards.append(sh)

    def _all(self, verb, *a):
        for sh in self.shards:
            getattr(sh.e, verb)(*a)

    def upload(self, state):
        self._all("upload", state)

    def linearise(self):
        self._all("refresh_begin")
        self.fake.gather_all()
        self._all("refresh_end")
        self._all("linearise_factors")

    def iterate(self, n=1):
        for it in range(n):
            self._all("iterate_begin")
            if it % 2:
                self._all("iterate_local")       # the landmark half first (what overlaps the exchange on several GPUs)
            self.fake.gather_all()
            self._all("iterate_end")

    def weaken_priors(self):
        for sh in self.shards:
            sh.weaken_priors()                   # priors are replicated / local: the partials of the last exchange still hold

    def new_keyframe(self, upd):
        for sh in self.shards:
            sh.new_keyframe(upd)

    def eval(self):
        """the shards' local sums added in rank order, as ShardedGbp.eval does over a process group"""
        evs = [sh.eval() for sh in self.shards]
        return {k: sum(ev[k] for ev in evs) for k in evs[0]}

    def read_priors(self):
        out = self.shards[0].read_priors()
        for r, sh in enumerate(self.shards):
            g = sh.read_priors()
            assert np.array_equal(g["cam_priors_eta"], out["cam_priors_eta"]) and np.array_equal(g["cam_priors_lambda"], out["cam_priors_lambda"])
            lo, hi, _ = self._own(r)
            out["lmk_priors_eta"][3 * lo:3 * hi] = g["lmk_priors_eta"][3 * lo:3 * hi]
            out["lmk_priors_lambda"][9 * lo:9 * hi] = g["lmk_priors_lambda"][9 * lo:9 * hi]
        return out

    def _own(self, r):
        lo, hi = int(self.bounds[r]), int(self.bounds[r + 1])
        lmk = np.asarray(self.bal["lmk_id"])
        return lo, hi, (lmk >= lo) & (lmk < hi)

    def read(self):
        out = self.shards[0].read()
        for r, sh in enumerate(self.shards):
            g = sh.read()
            assert np.array_equal(g["cam_beliefs_eta"], out["cam_beliefs_eta"], equal_nan=True)       # replicated, identical on every shard
            assert np.array_equal(g["cam_beliefs_lambda"], out["cam_beliefs_lambda"], equal_nan=True)
            lo, hi, own = self._own(r)
            out["lmk_beliefs_eta"][3 * lo:3 * hi] = g["lmk_beliefs_eta"][3 * lo:3 * hi]
            out["lmk_beliefs_lambda"][9 * lo:9 * hi] = g["lmk_beliefs_lambda"][9 * lo:9 * hi]
            for k in ("damping", "damping_count", "robust_flag"):
                out[k][own] = g[k][own]
        return out

    def factor_potentials(self):
        E = len(self.bal["cam_id"])
        eta, lam = np.zeros((E, 9), np.float32), np.zeros((E, 81), np.float32)
        for r, sh in enumerate(self.shards):
            e, l = sh.e.factor_potentials()      # factors of other shards are left at zero
            own = self._own(r)[2]
            eta[own], lam[own] = e.reshape(E, 9)[own], l.reshape(E, 81)[own]
        return eta.ravel(), lam.ravel()

    def messages(self):
        out = {}
        for r, sh in enumerate(self.shards):
            own = self._own(r)[2]
            for k, v in sh.e.messages().items():      # factors of other shards are left at zero
                out.setdefault(k, np.zeros_like(v)).reshape(self.E, -1)[own] = v.reshape(self.E, -1)[own]
        return out


def _engine(bal, K, **kw):
    from gbp_poplar_amd.engine import GbpEngine
    return GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_params(**kw), hooks=True)


def _placement_options(bal):
    """layout options under which a graph this small gets its rows placed by landmark class (and its tiles permuted)"""
    from gbp_poplar_amd import hostlib
    opt = hostlib.layout_options(tile_min_tiles=1, row_window=min(32, bal["n_cams"] // 2))
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], options=opt)
    return opt, lay


def _gpu_path(path, bal, K, **kw):
    """an object with the engine's verbs for one of the ways the library can run the program list"""
    from gbp_poplar_amd import _lib
    lib = _lib.load(hooks=True)
    if path == "two_kernels":
        eng = _engine(bal, K, persistent=-1, **kw)
        assert eng.graph_state() != 2 and eng.sweep_variant() == (1, False)      # camera messages loaded cached: the choice for every small graph
    elif path == "library_choice":
        eng = _engine(bal, K, **kw)
        assert eng.graph_state() == 2, eng.last_error()      # graphs this small run their bursts inside the persistent kernel
    elif path == "per_factor_mu":
        eng = _engine(bal, K, per_factor_mu=1, **kw)
    elif path == "seg_skip":
        # the segment-skipping sweep exists for cache policy 0 only, and graphs this small get policy 1 by shape: both are forced
        assert lib.gbp_debug_force_sweep_policy(0) == 0 and lib.gbp_debug_force_seg_skip(1) == 0
        try:
            eng = _engine(bal, K, persistent=-1, **kw)
        finally:
            lib.gbp_debug_force_seg_skip(-1)
            lib.gbp_debug_force_sweep_policy(-1)
        assert eng.graph_state() != 2 and eng.sweep_variant() == (0, True)
    elif path == "rows_placed":
        opt, lay = _placement_options(bal)
        assert lay["row_slot"].size and not np.array_equal(lay["row_slot"], np.arange(lay["row_slot"].size)), "rows were not placed"
        assert lib.gbp_debug_layout_options(opt) == 0
        try:
            eng = _engine(bal, K, **kw)
        finally:
            lib.gbp_debug_layout_options(None)
        assert eng.graph_state() != 2                       # placed rows never run in the persistent kernel
    elif path in ("shards_2", "shards_3"):
        eng = _Shards(bal, K, int(path[-1]), **kw)
    else:
        raise ValueError(path)
    return eng


EXACT_PATHS = ["two_kernels", "library_choice", "per_factor_mu", "seg_skip", "shards_2", "shards_3", "rows_placed"]
BIT_PATHS = ["two_kernels", "library_choice", "per_factor_mu", "seg_skip", "shards_2"]


@pytest.fixture
def rounded_trig(oracle_mod):
    """the oracle's sin / cos correctly rounded, as the kernels compute them"""
    oracle_mod.set_trig_mode(1)
    yield
    oracle_mod.set_trig_mode(0)


# ---- A and B: exact inference ----------------------------------------------------------------------------------------------------
class _Exact:
    """One graph of A / B: its inputs and, per set of potentials, the joint's exact marginals.  The dense inverse is computed once and
    kept: every path holds the same potentials bit for bit, which run() checks before it uses them."""

    def __init__(self, name, bal, sweeps, state=None, cond_limit=None, **params):
        """state: what the run uploads and the joint takes its priors and active flags from (default: the inputs of _inputs, every
        factor active, the priors as uploaded); members given replace those of _inputs"""
        self.name, self.bal, self.sweeps = name, bal, sweeps
        self.params = {"dmu_threshold": 0.0, **params}             # by default relin = dmu < 0 never fires
        self.K, self.state = _inputs(bal)
        if state is not None:
            self.state = dict(self.state, **state)
        self.cond_limit = COND_LIMIT[name[0]] if cond_limit is None else cond_limit
        self._kept = {}

    def exact(self, fac_eta, fac_lambda, state=None, key=None):
        """the exact marginals of the joint of `state`'s priors (default: the uploaded state's) and its active factors' potentials.  The
        last joint of each `key` (a name the caller gives a state) is kept and used again for the same potentials"""
        kept = self._kept.get(key)
        if kept is None or not (np.array_equal(kept[0], fac_eta) and np.array_equal(kept[1], fac_lambda)):
            Lam, eta = ref64.joint(self.bal, self.state if state is None else state, fac_eta, fac_lambda)
            w = np.linalg.eigvalsh(Lam)
            cond = float(w[-1] / w[0])
            print("%s: joint of %d unknowns, condition %.1f" % (self.name, eta.size, cond))
            assert w[0] > 0 and cond <= self.cond_limit, cond
            ex = ref64.marginals(Lam, eta, self.bal["n_cams"], self.bal["n_lmks"])
            ex["cond"] = cond
            kept = self._kept[key] = (np.array(fac_eta), np.array(fac_lambda), ex)
        return kept[2]

    def errors(self, beliefs, ex):
        cm = ref64.belief_means(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6)
        lm = ref64.belief_means(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3)
        return {"cam_mean": per_var_rel(cm, ex["cam_mean"], 6), "lmk_mean": per_var_rel(lm, ex["lmk_mean"], 3),
                "cam_lambda": per_var_rel(beliefs["cam_beliefs_lambda"], ex["cam_lambda"], 36),
                "lmk_lambda": per_var_rel(beliefs["lmk_beliefs_lambda"], ex["lmk_lambda"], 9)}

    def run(self, x, what):
        """the program on engine / oracle / shard group x: upload, LINEARISE, read the potentials back, sweep; errors against the joint
        of those potentials"""
        x.upload(self.state)
        x.linearise()
        fe, fl = x.factor_potentials()
        ex = self.exact(fe, fl)
        x.iterate(self.sweeps)
        err = self.errors(x.read(), ex)
        print("%s %s after %d sweeps: %s" % (self.name, what, self.sweeps, "  ".join("%s %.3e" % kv for kv in err.items())))
        return err


@pytest.fixture(scope="module")
def graph_a():
    bal, hub_id = hub_tree()
    d = diameter(bal)
    g = _Exact("A hub tree", bal, d + A_SWEEPS_OVER_DIAMETER, maxeta_damping=0.0)
    g.hub_id, g.diameter = hub_id, d
    return g


@pytest.fixture(scope="module")
def graph_b():
    return _Exact("B loopy 4x12", all_to_all(4, 12), B_SWEEPS, maxeta_damping=0.4)


def test_hub_tree_has_the_shapes_it_is_for(graph_a):
    bal = graph_a.bal
    ldeg = np.bincount(bal["lmk_id"], minlength=bal["n_lmks"])
    cdeg = np.bincount(bal["cam_id"], minlength=bal["n_cams"])
    assert bal["n_edges"] == bal["n_cams"] + bal["n_lmks"] - 1 and graph_a.diameter == 16      # a tree (connected: diameter())
    assert bal["n_cams"] == 126 and bal["n_lmks"] > 64
    assert sorted(ldeg[graph_a.hub_id]) == sorted(HUB_DEGREES) and np.all(np.delete(ldeg, graph_a.hub_id) == 1)
    assert {1, 16, 17, 256, 257, 272, 273} <= set(cdeg.tolist())
    assert [-(-n // 16) for n in (1, 16, 17, 256, 257, 272, 273)] == [1, 1, 2, 16, 17, 17, 18]
    assert np.array_equal(bal["cam_id"], np.sort(bal["cam_id"]))
    hubs = np.asarray(graph_a.hub_id)
    assert np.array_equal(hubs // 16, np.arange(8))                   # one hub in each of the first eight groups of 16
    assert bal["n_lmks"] // 16 - 8 >= 2                               # whole groups of leaves only behind them
    for a, b in zip(graph_a.hub_id[:-1], graph_a.hub_id[1:]):         # consecutive hubs share exactly one camera
        assert len(set(bal["cam_id"][bal["lmk_id"] == a]) & set(bal["cam_id"][bal["lmk_id"] == b])) == 1
    leafless = [c for c in range(bal["n_cams"]) if np.all(np.isin(bal["lmk_id"][bal["cam_id"] == c], hubs))]
    assert len(leafless) >= 1


ORACLES = [pytest.param("restatement", 1, id="device_order"), pytest.param("restatement", 0, id="slot_order"),
           pytest.param("ref", 0, id="reference_math", marks=pytest.mark.skipif(
               not orc_build.have("ref"), reason="reference-math build absent (make -C oracle ref)"))]


def _oracle_variant(oracle_mod, g, variant, order):
    orc = oracle_mod.Oracle(g.bal["cam_id"], g.bal["lmk_id"], g.bal["n_cams"], g.bal["n_lmks"], g.K, params=_params(**g.params), variant=variant)
    orc.set_sum_order(order)
    return orc


@pytest.mark.parametrize("variant, order", ORACLES)
def test_oracle_on_the_hub_tree_is_exact(variant, order, graph_a, oracle_mod):
    orc = _oracle_variant(oracle_mod, graph_a, variant, order)
    err = graph_a.run(orc, "oracle(%s, sum order %d)" % (variant, order))
    for k in TENSORS:
        assert err[k] <= A_BOUND[k], (k, err[k], A_BOUND[k])


@pytest.mark.parametrize("variant, order", ORACLES)
def test_oracle_on_the_loopy_graph_has_exact_means(variant, order, graph_b, oracle_mod):
    orc = _oracle_variant(oracle_mod, graph_b, variant, order)
    err = graph_b.run(orc, "oracle(%s, sum order %d)" % (variant, order))
    for k in B_BOUND:
        assert err[k] <= B_BOUND[k], (k, err[k], B_BOUND[k])
    assert err["cam_lambda"] > B_LAMBDA_GAP and err["lmk_lambda"] > B_LAMBDA_GAP      # converged LOOPY GBP, not something else
    assert np.all(orc.read()["damping"] == np.float32(0.4))                            # the eta damping was on and left the fixed point alone


def _moved_by_leaving_out(g, ex, fe, fl, e):
    """per tensor: how far the exact marginals move, in the tests' error measure, when factor e is taken out of the joint"""
    bal = g.bal
    C, L = bal["n_cams"], bal["n_lmks"]
    c, l = int(bal["cam_id"][e]), int(bal["lmk_id"][e])
    idx = np.r_[6 * c:6 * c + 6, 6 * C + 3 * l:6 * C + 3 * l + 3]
    (P, Q), mean2 = ref64.without_factor(ex["Sigma"], ex["mean"], idx, ref64.factor_block(fl.reshape(-1, 81)[e]),
                                         np.asarray(fe, np.float64).reshape(-1, 9)[e])
    ci = np.arange(6 * C).reshape(C, 6)
    li = 6 * C + np.arange(3 * L).reshape(L, 3)
    cS = np.linalg.inv(ex["cam_lambda"]) + np.einsum("vik,vkj->vij", P[ci], Q[:, ci].transpose(1, 0, 2))
    lS = np.linalg.inv(ex["lmk_lambda"]) + np.einsum("vik,vkj->vij", P[li], Q[:, li].transpose(1, 0, 2))
    return {"cam_mean": per_var_rel(mean2[:6 * C], ex["cam_mean"], 6), "lmk_mean": per_var_rel(mean2[6 * C:], ex["lmk_mean"], 3),
            "cam_lambda": per_var_rel(np.linalg.inv(cS), ex["cam_lambda"], 36), "lmk_lambda": per_var_rel(np.linalg.inv(lS), ex["lmk_lambda"], 9)}


def _potentials_of_oracle(g, oracle_mod):
    orc = _oracle(oracle_mod, g.bal, g.K, **g.params)
    orc.upload(g.state)
    orc.linearise()
    return orc.factor_potentials()


def test_woodbury_removal_equals_rebuilding_the_joint(graph_b, oracle_mod):
    """the low-rank form the blindness test of A relies on, against the plain way: build the joint without the factor and invert it"""
    fe, fl = _potentials_of_oracle(graph_b, oracle_mod)
    ex = graph_b.exact(fe, fl)
    bal = graph_b.bal
    for e in (0, 17, 47):
        ex2 = ref64.marginals(*ref64.joint(bal, graph_b.state, fe, fl, skip=e), bal["n_cams"], bal["n_lmks"])
        want = {k: per_var_rel(ex2[k], ex[k], w) for k, w in zip(TENSORS, (6, 3, 36, 9))}
        got = _moved_by_leaving_out(graph_b, ex, fe, fl, e)
        for k in TENSORS:
            assert abs(got[k] - want[k]) <= 1e-6 * want[k], (e, k, got[k], want[k])


@pytest.mark.parametrize("which", ["A", "B"])
def test_bounds_are_not_blind_to_a_missing_factor(which, graph_a, graph_b, oracle_mod):
    """In float64 alone: for EVERY factor, the exact marginals of the joint without it lie at least 100 x the bound away from the full
    joint's, in the error measure and on the tensors the tests compare: a belief that misses any one factor fails by two orders of
    magnitude.  On A the precisions carry that for every factor (measured: at least 4 221 x the bound on the cameras, 19 462 x on the
    landmarks); its means alone would not — a factor that agrees with the rest of the graph hardly moves them — which is why A
    compares both.  On B only the means are exact, and they do (113 x and 148 x).
    (So on A "the marginals move" is asked of mean and precision TOGETHER — each factor's best tensor, and both precision tensors for
    every factor — not of the means by themselves: no tree of these observations makes every leaf factor disagree with its prior.)"""
    g, bound = (graph_a, A_BOUND) if which == "A" else (graph_b, B_BOUND)
    fe, fl = _potentials_of_oracle(g, oracle_mod)
    ex = g.exact(fe, fl)
    least = {k: np.inf for k in bound}
    least_of_factor = np.inf
    for e in range(g.bal["n_edges"]):
        moved = _moved_by_leaving_out(g, ex, fe, fl, e)
        ratio = {k: moved[k] / bound[k] for k in bound}
        least = {k: min(least[k], ratio[k]) for k in bound}
        least_of_factor = min(least_of_factor, max(ratio.values()))
    print("%s: smallest (marginals moved by one missing factor) / bound: %s;  of a factor's best tensor %.0f"
          % (g.name, "  ".join("%s %.0f" % kv for kv in least.items()), least_of_factor))
    assert least_of_factor >= 100.0, least_of_factor
    if which == "A":
        assert least["cam_lambda"] >= 100.0 and least["lmk_lambda"] >= 100.0, least
    else:
        assert least["cam_mean"] >= 100.0 and least["lmk_mean"] >= 100.0, least


@gpu
@pytest.mark.parametrize("path", EXACT_PATHS)
def test_hub_tree_is_exact_on_the_gpu(path, graph_a, rounded_trig):
    err = graph_a.run(_gpu_path(path, graph_a.bal, graph_a.K, **graph_a.params), path)
    for k in TENSORS:
        assert err[k] <= A_BOUND[k], (path, k, err[k], A_BOUND[k])


@gpu
@pytest.mark.parametrize("path", EXACT_PATHS[:-1])      # (four cameras of one row each: nothing for row placement to move, that leg is A's)
def test_loopy_means_are_exact_on_the_gpu(path, graph_b, rounded_trig):
    x = _gpu_path(path, graph_b.bal, graph_b.K, **graph_b.params)
    err = graph_b.run(x, path)
    for k in B_BOUND:
        assert err[k] <= B_BOUND[k], (path, k, err[k], B_BOUND[k])
    assert err["cam_lambda"] > B_LAMBDA_GAP and err["lmk_lambda"] > B_LAMBDA_GAP
    assert np.all(x.read()["damping"] == np.float32(0.4))


# ---- C: gather and row boundaries, bit for bit ---------------------------------------------------------------------------------
def _equal(eng, orc):
    """beliefs, both message sets, damping state and robust flags (a shard group: every shard's own landmarks and factors put together)"""
    _assert_state_equal(eng, orc)
    assert np.array_equal(eng.read()["robust_flag"], orc.read()["robust_flag"])


def test_boundary_graphs_have_the_shapes_they_are_for():
    from gbp_poplar_amd import hostlib
    bal = gather_graph()
    ldeg = np.bincount(bal["lmk_id"], minlength=bal["n_lmks"])
    assert bal["n_cams"] == 40 and bal["n_lmks"] == 96 and set(ldeg[:80].tolist()) == set(GATHER_KINDS) and ldeg[80:].max() <= 10
    assert len(set(np.bincount(bal["cam_id"]).tolist())) > 4                               # ragged cameras
    bal = row_graph()
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    assert np.diff(lay["cam_row_ptr"]).tolist() == [0, 1, 1, 2, 16, 17, 17, 18, 32, 33, 33, 34]


@gpu
@pytest.mark.parametrize("path", BIT_PATHS)
@pytest.mark.parametrize("graph", ["gather", "rows"])
def test_gather_and_row_boundaries_bit_for_bit(graph, path, oracle_mod, rounded_trig):
    bal = gather_graph() if graph == "gather" else row_graph()
    K, state = _inputs(bal)
    eng = _gpu_path(path, bal, K)
    orc = _oracle(oracle_mod, bal, K, bounds=eng.bounds if isinstance(eng, _Shards) else None)

    def both(verb, *a):
        getattr(eng, verb)(*a)
        getattr(orc, verb)(*a)

    both("upload", state)
    both("linearise")
    fe, fl = eng.factor_potentials()
    oe, ol = orc.factor_potentials()
    assert np.array_equal(fe, oe) and np.array_equal(fl, ol)
    _equal(eng, orc)
    for n in (1, 1, 1, 3):                       # sweeps 1, 2, 3 from the upload's zero messages, then a burst
        both("iterate", n)
        _equal(eng, orc)
    both("linearise")                            # under live messages
    _equal(eng, orc)
    both("iterate", 2)
    _equal(eng, orc)
    if path == "two_kernels":                    # k_beliefs_ev and the sweep the metric rides in, on the same shapes
        evs = eng.iterate_eval_each(3)
        # n_nonfinite is the one counter the two define differently: the oracle counts variables whose belief eta / Lambda hold a
        # non-finite number, the library (include/gbp_mi355x.h) those whose belief MEAN is not finite.  A variable no factor sees has
        # a zero prior and a zero belief here: finite for the oracle (0), a 0 / 0 mean for the library.  So: the oracle's count
        # plus the unseen variables.
        unseen = int(np.sum(np.bincount(bal["cam_id"], minlength=bal["n_cams"]) == 0) + np.sum(np.bincount(bal["lmk_id"], minlength=bal["n_lmks"]) == 0))
        assert unseen == (7 if graph == "gather" else 1)
        for ev in evs:
            orc.iterate(1)
            o = orc.eval()
            for k in ("n_active", "n_relin", "n_robust", "n_nonpd"):
                assert ev[k] == o[k], (k, ev[k], o[k])
            assert o["n_nonfinite"] == 0 and ev["n_nonfinite"] == o["n_nonfinite"] + unseen
            assert abs(ev["sum_norm"] - o["sum_norm"]) <= 1e-6 * o["sum_norm"]
        _equal(eng, orc)


# ---- D: the metric, per factor ---------------------------------------------------------------------------------------------------
def metric_graph():
    return all_to_all(6, 40)


def metric_cases(bal):
    """factors 0, 15, 16, 63, 64, 239, the last factor in front of a pad and the first factor of the last tile that holds one"""
    from gbp_poplar_amd import hostlib
    pos_edge = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])["pos_edge"]
    pad = pos_edge == 0xFFFFFFFF
    before_pad = int(pos_edge[np.nonzero(~pad[:-1] & pad[1:])[0][0]])
    last_tile = np.nonzero(np.any(~pad.reshape(-1, 64), axis=1))[0][-1]
    first_of_last_tile = int(pos_edge[64 * last_tile:64 * last_tile + 64][~pad[64 * last_tile:64 * last_tile + 64]][0])
    assert last_tile >= 3 and pad.any()
    return sorted({0, 15, 16, 63, 64, 239, before_pad, first_of_last_tile})


def _one_hot(E, e):
    a = np.zeros(E, np.uint32)
    a[e] = 1
    return a


def _check_term(ev, x, bal, K, state, e, what):
    """one evaluation record with a single active factor e against the float64 term from the beliefs read back"""
    norm, half = ref64.metric_terms(x.read(), bal, K, state["measurements"], state["active_flag"])
    d_norm, d_half = abs(ev["sum_norm"] - norm[e]), abs(ev["sum_half_sq"] - half[e])
    print("D factor %3d %-22s norm %.6f px (float64 %.6f, off by %.2e)  half square off by %.2e" % (e, what, ev["sum_norm"], norm[e], d_norm, d_half))
    assert ev["n_active"] == 1 and norm[e] > 0 and np.count_nonzero(norm) == 1
    return d_norm, d_half


def _single_factor_terms(x, bal, K, state, e, calls):
    """upload with factor e alone active, LINEARISE, two sweeps; every metric call in `calls` against ref64; returns the largest errors"""
    st = dict(state, active_flag=_one_hot(bal["n_edges"], e))
    x.upload(st)
    x.linearise()
    x.iterate(2)
    worst = np.zeros(2)
    for call in calls:
        if call == "eval":
            ev = x.eval()
        elif call == "iterate_eval_each":
            ev = x.iterate_eval_each(2)[-1]
        elif call == "ba_loop":
            ev = x.ba_loop(2, 20, 5)[-1]         # passes 20, 21 of the loop: behind the prior weakening of its first ten
        worst = np.maximum(worst, _check_term(ev, x, bal, K, st, e, call))
    return worst


def _whole_graph_sums(x, bal, K, state, device_calls):
    """all factors active, after 0, 3 and 30 sweeps: the sums against float64, per factor; returns the largest errors"""
    E = bal["n_edges"]
    x.upload(state)
    x.linearise()
    worst, done = np.zeros(2), 0
    for sweeps in (0, 3, 30):
        evs = [x.eval()] if sweeps == done else None
        if evs is None and device_calls:
            evs = [x.iterate_eval_each(sweeps - done)[-1], x.eval()]
        elif evs is None:
            x.iterate(sweeps - done)
            evs = [x.eval()]
        done = sweeps
        norm, half = ref64.metric_terms(x.read(), bal, K, state["measurements"], state["active_flag"])
        for ev in evs:
            d = np.array([abs(ev["sum_norm"] - norm.sum()), abs(ev["sum_half_sq"] - half.sum())]) / E
            print("D whole graph after %2d sweeps: mean norm %.6f px, off by %.2e px per factor; half square off by %.2e" % (sweeps, ev["sum_norm"] / E, d[0], d[1]))
            assert ev["n_active"] == E
            worst = np.maximum(worst, d)
    return worst


def test_oracle_metric_per_factor_and_as_a_sum(oracle_mod):
    bal = metric_graph()
    K, state = _inputs(bal)
    orc = _oracle(oracle_mod, bal, K)
    worst = np.zeros(2)
    for e in metric_cases(bal):
        worst = np.maximum(worst, _single_factor_terms(orc, bal, K, state, e, ["eval"]))
    mean = _whole_graph_sums(orc, bal, K, state, device_calls=False)
    print("D oracle: per factor %.3e px, %.3e px^2;  sums per factor %.3e px, %.3e px^2" % (worst[0], worst[1], mean[0], mean[1]))
    assert worst[0] <= D_BOUND["term_norm"] and worst[1] <= D_BOUND["term_half_sq"]
    assert mean[0] <= D_BOUND["mean_norm"] and mean[1] <= D_BOUND["mean_half_sq"]


def test_metric_bounds_are_not_blind(oracle_mod):
    """the same terms with the rotation transposed, or with the landmark index shifted by one, lie at least 100 x the bound away in
    every case: the single factors after two sweeps and the sums after 0, 3 and 30"""
    bal = metric_graph()
    K, state = _inputs(bal)
    E = bal["n_edges"]
    orc = _oracle(oracle_mod, bal, K)
    wrongs = (dict(rotation_transposed=True), dict(lmk_shift=1))
    for e in metric_cases(bal):
        st = dict(state, active_flag=_one_hot(E, e))
        orc.upload(st)
        orc.linearise()
        orc.iterate(2)
        b = orc.read()
        norm, half = ref64.metric_terms(b, bal, K, st["measurements"], st["active_flag"])
        for kw in wrongs:
            n2, h2 = ref64.metric_terms(b, bal, K, st["measurements"], st["active_flag"], **kw)
            assert abs(n2[e] - norm[e]) >= 100 * D_BOUND["term_norm"] and abs(h2[e] - half[e]) >= 100 * D_BOUND["term_half_sq"], (e, kw)
    orc.upload(state)
    orc.linearise()
    for n in (0, 3, 27):
        orc.iterate(n)
        b = orc.read()
        norm, half = ref64.metric_terms(b, bal, K, state["measurements"], state["active_flag"])
        for kw in wrongs:
            n2, h2 = ref64.metric_terms(b, bal, K, state["measurements"], state["active_flag"], **kw)
            assert abs(n2.sum() - norm.sum()) / E >= 100 * D_BOUND["mean_norm"] and abs(h2.sum() - half.sum()) / E >= 100 * D_BOUND["mean_half_sq"], (n, kw)


@gpu
@pytest.mark.parametrize("path", ["two_kernels", "library_choice"])
def test_metric_of_single_factors_on_the_gpu(path):
    """eval(), iterate_eval_each and ba_loop with metrics; under library_choice the loops' metric is the persistent kernel's"""
    bal = metric_graph()
    K, state = _inputs(bal)
    eng = _gpu_path(path, bal, K)
    worst = np.zeros(2)
    for e in metric_cases(bal):
        worst = np.maximum(worst, _single_factor_terms(eng, bal, K, state, e, ["eval", "iterate_eval_each", "ba_loop"]))
    print("D %s: per factor %.3e px, %.3e px^2" % (path, worst[0], worst[1]))
    assert worst[0] <= D_BOUND["term_norm"] and worst[1] <= D_BOUND["term_half_sq"]


@gpu
@pytest.mark.parametrize("path", ["two_kernels", "library_choice"])
def test_metric_of_the_whole_graph_on_the_gpu(path):
    bal = metric_graph()
    K, state = _inputs(bal)
    mean = _whole_graph_sums(_gpu_path(path, bal, K), bal, K, state, device_calls=True)
    print("D %s: sums per factor %.3e px, %.3e px^2" % (path, mean[0], mean[1]))
    assert mean[0] <= D_BOUND["mean_norm"] and mean[1] <= D_BOUND["mean_half_sq"]
