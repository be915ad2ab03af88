"""Whole-graph inputs in which no stream is uniform and the variable side sees wide numbers: the generator, the graphs, the chosen
(graph, seed, ranges) and the program of tests/test_wide_state_cpu.py and tests/test_gpu_wide_state.py.  No GPU.

driver.build_inputs hands every other whole-graph test one measurement variance, one prior block, one scaling, one weaken flag, zero
damping and one damping count: reading any of them from the wrong factor or variable changes nothing there.  wide_state() draws all of
them per factor / per variable:

  "placement"  benign magnitudes, every value exact in float32 (so the weakened priors are exact too): what the upload's permutation
               from file order into device order, and the per-variable records, are checked with, bit for bit
  "wide"       every prior a full SPD block Q diag(s geomspace(1, 1 / cond)) Q^T with s over decades per variable, the measurement
               variance over decades per factor, the scalings over four decades: beliefs that are not positive definite, message
               Lambdas of 1e7
  "nonfinite"  s over 12 decades, cond up to 1e6: the first sweep leaves non-finite beliefs

The draws are a pure function of (graph, seed, profile, ranges).  WIDE_CASES, METRIC_CASES, RELIN_CASES and NONFINITE_CASES hold
what the tests run; the conditions the GPU tests rest
on (finite where promised, how many beliefs are non-PD, decided health predicates) are asserted on the CPU oracle, per case, in
tests/test_wide_state_cpu.py."""
import numpy as np

FY = 437.5          # K of every state: fx = 500 != fy (the graphs' generators use one focal length)
PLACEMENT_VARIANCES = (1.0, 2.25, 4.0, 9.0)
PLACEMENT_DAMPING = (0.0, 0.1, 0.4)
PLACEMENT_SCALINGS = (0.25, 0.5, 2.0, 4.0)
INACTIVE_SHARE = 0.15
# log10 ranges of the "wide" profile as the CPU probe drew them: s per variable, cond <= 10^cond, variance per factor, scaling per variable
WIDE = {"s": (-3.0, 5.0), "cond": 2.0, "var": (-3.0, 3.0), "scaling": (-2.0, 2.0)}
RELIN = {"s": (-1.0, 3.0), "cond": 2.0, "var": (-1.0, 1.0), "scaling": (-2.0, 2.0)}
NONFINITE = {"s": (-6.0, 6.0), "cond": 6.0, "var": (-3.0, 3.0), "scaling": (-2.0, 2.0)}
RELIN_PARAMS = dict(min_linear_iters=2, num_undamped_iters=1, dmu_threshold=0.05)
RELIN_COUNT = -1
RELIN_SWEEPS = 6


def narrowed(ranges, decades):
    """every range `decades` narrower: half a range's share taken off at either end, cond's off its top"""
    h = 0.5 * decades
    return {"s": (ranges["s"][0] + h, ranges["s"][1] - h), "cond": max(ranges["cond"] - h, 0.0),
            "var": (ranges["var"][0] + h, ranges["var"][1] - h), "scaling": ranges["scaling"]}


# ---- the graphs ------------------------------------------------------------------------------------------------------------------
def probe_graph():
    """6 cameras x 40 landmarks, about half of the factors kept (every camera and landmark keeps one)"""
    from tests.test_gpu_parity import _tiny_problem
    rng = np.random.default_rng(640)
    cam_id, lmk_id = np.repeat(np.arange(6), 40), np.tile(np.arange(40), 6)
    keep = rng.random(240) < 0.5
    keep[40 * (np.arange(40) % 6) + np.arange(40)] = True      # factor (camera l % 6, landmark l)
    assert np.unique(cam_id[keep]).size == 6 and np.unique(lmk_id[keep]).size == 40
    return _tiny_problem(cam_id[keep].tolist(), lmk_id[keep].tolist(), 6, 40)


def fuzz_graph():
    """a graph of the randomised soak's smallest class whose edge list is NOT sorted by camera and holds duplicate (camera, landmark)
    factors and a hub landmark: the device order differs from the file order in every stream.  (Of at least 600 factors: the smaller
    ones of the class have no seed among the first 200 that relinearises ten times in six sweeps.)"""
    from tests import fuzz_support
    for seed in range(64):
        bal = fuzz_support.random_problem(np.random.default_rng(52000 + seed), size="tiny")
        t = fuzz_support.graph_traits(bal)
        if not t["sorted"] and t["duplicates"] and t["hub"] and 600 <= bal["n_edges"] <= 1000 and bal["n_cams"] >= 8:
            return bal
    raise AssertionError("no unsorted tiny graph with duplicates among 64 seeds")


def graph(name):
    from tests.test_exact_inference import gather_graph, row_graph
    return {"probe": probe_graph, "gather": gather_graph, "rows": row_graph, "fuzz": fuzz_graph}[name]()


GRAPHS = ("probe", "gather", "rows", "fuzz")


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def _base(bal):
    """K with fx != fy, the measurements moved to it, and the inputs driver.build_inputs makes of them"""
    from gbp_poplar_amd import driver, hostlib
    obs = np.asarray(bal["observations"], np.float64).reshape(-1, 2).copy()
    obs[:, 1] = (obs[:, 1] - bal["cy"]) * (FY / bal["fy"]) + bal["cy"]
    K, state, _ = driver.build_inputs(dict(bal, fy=FY, observations=obs.ravel()), driver.Options(), hostlib)
    assert K[0] != K[4]
    return K, state


def _spd_priors(rng, means, width, s_range, cond):
    """(eta, Lambda) float32 per variable: Lambda = Q diag(s geomspace(1, 1 / c)) Q^T symmetric to the bit, eta = Lambda mean"""
    n = means.shape[0]
    lam = np.zeros((n, width, width), np.float32)
    for v in range(n):
        s = 10.0 ** rng.uniform(*s_range)
        c = 10.0 ** rng.uniform(0.0, cond)
        Q = np.linalg.qr(rng.normal(size=(width, width)))[0]
        A = (Q * (s * np.geomspace(1.0, 1.0 / c, width))) @ Q.T
        lam[v] = (0.5 * (A + A.T)).astype(np.float32)
    eta = np.einsum("vij,vj->vi", lam.astype(np.float64), means).astype(np.float32)
    return eta.ravel(), lam.ravel()


def wide_state(bal, seed, profile, ranges=None, damping_count=None):
    """(state, K): a complete gbp_state_in dict.  ranges: the log10 ranges of "wide" / "nonfinite" (default WIDE / NONFINITE);
    damping_count: one count for every factor in place of the draw from -15 .. 3 (the relinearising leg uploads -1)."""
    K, base = _base(bal)
    C, L, E = int(bal["n_cams"]), int(bal["n_lmks"]), int(bal["n_edges"])
    rng = np.random.default_rng([int(seed), {"placement": 1, "wide": 2, "nonfinite": 3}[profile]])
    state = dict(base)
    state["damping"] = rng.choice(PLACEMENT_DAMPING, E).astype(np.float32)
    state["damping_count"] = rng.integers(-15, 4, E).astype(np.int32)
    state["active_flag"] = (rng.random(E) >= INACTIVE_SHARE).astype(np.uint32)
    state["cam_weaken_flag"] = rng.integers(0, 8, C).astype(np.uint32)
    state["lmk_weaken_flag"] = rng.integers(0, 8, L).astype(np.uint32)
    if damping_count is not None:
        state["damping_count"] = np.full(E, damping_count, np.int32)
    if profile == "placement":
        state["meas_variances"] = rng.choice(PLACEMENT_VARIANCES, E).astype(np.float32)
        state["cam_scaling"] = rng.choice(PLACEMENT_SCALINGS, C).astype(np.float32)
        state["lmk_scaling"] = rng.choice(PLACEMENT_SCALINGS, L).astype(np.float32)
        for who, n, we, wl in (("cam", C, 6, 36), ("lmk", L, 3, 9)):
            f = (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)
            lam = base[who + "_priors_lambda"].reshape(n, wl)
            off = lam.reshape(n, we, we) * (1 - np.eye(we, dtype=np.float32))
            assert not off.any(), "the priors of set_prior_lambda are expected diagonal"
            state[who + "_priors_eta"] = (base[who + "_priors_eta"].reshape(n, we) * f[:, None]).ravel()
            state[who + "_priors_lambda"] = (lam * f[:, None]).ravel()
        return state, K
    r = ranges if ranges is not None else (WIDE if profile == "wide" else NONFINITE)
    state["meas_variances"] = (10.0 ** rng.uniform(*r["var"], E)).astype(np.float32)
    state["cam_scaling"] = (10.0 ** rng.uniform(*r["scaling"], C)).astype(np.float32)
    state["lmk_scaling"] = (10.0 ** rng.uniform(*r["scaling"], L)).astype(np.float32)
    cams = np.asarray(bal["cameras"], np.float64).astype(np.float32).astype(np.float64).reshape(C, 6)
    pts = np.asarray(bal["points"], np.float64).astype(np.float32).astype(np.float64).reshape(L, 3)
    state["cam_priors_eta"], state["cam_priors_lambda"] = _spd_priors(rng, cams, 6, r["s"], r["cond"])
    state["lmk_priors_eta"], state["lmk_priors_lambda"] = _spd_priors(rng, pts, 3, r["s"], r["cond"])
    return state, K


# ---- the program of legs P and W ------------------------------------------------------------------------------------------------------
def weakenings_applied(flag, k):
    """how often WeakenPriorVertex has scaled a prior after k WEAKEN_PRIORS: it acts on flags 1 .. 5 only (and counts them down), so a
    prior uploaded with flag 6 or 7 is never weakened"""
    flag = np.asarray(flag, np.int64)
    return np.where(flag <= 5, np.minimum(flag, k), 0)


def program(do, check):
    """LINEARISE, four sweeps with a weakening in front of sweeps 2, 3 and 4, three more weakenings (every flag of 1 .. 5 has counted
    down to 0), a burst of two sweeps.  do(verb, *args) runs a verb on everything that takes part; check(stage, weakenings so far) is
    called behind every step."""
    do("linearise")
    check("linearise", 0)
    k = 0
    for sweep in (1, 2, 3, 4):
        if sweep > 1:
            do("weaken_priors")
            k += 1
            check("weakening %d" % k, k)
        do("iterate", 1)
        check("sweep %d" % sweep, k)
    for _ in range(3):
        do("weaken_priors")
        k += 1
        check("weakening %d" % k, k)
    do("iterate", 2)
    check("burst of 2", k)



# ---- the measures ----------------------------------------------------------------------------------------------------------------
BELIEF_TENSORS = ("cam_eta", "cam_lambda", "lmk_eta", "lmk_lambda")
MEAN_COND_LIMIT = 1e4       # hoisted means are compared on PD variables whose float64 condition is at most this
MEAN_LEFT_OUT_CAP = 0.5
DEPTH_LIMIT = 1e-2          # the metric leaves out factors whose camera-frame depth is below this share of the point's norm |y| (shallow_factors)
METRIC_LEFT_OUT_CAP = 0.1
METRIC_ROUNDS = 12
PIVOT_MARGIN = 1e-6         # no LDL^T pivot may lie this close to zero, relative to the terms it is the difference of


def shallow_factors(cam_mean, lmk_mean, bal):
    """per factor, in float64: is the camera-frame depth (R y + t)_z below DEPTH_LIMIT of the point's norm |y|?  The depth is the sum
    of (R y)_z and t_z: where they cancel to less than a hundredth of |y|, one float32 ulp of either moves the projection by 1e-5 of
    itself and more, and the term is not a number float32 can be held to.  (Measured against |R y + t| instead, a factor at depth
    -0.008 between summands of 4.8 passes as 0.0106 of a camera-frame point of norm 0.76; one ulp of t_z then moves a sum of 2.4e5 px
    by 2.7 px.)  A non-finite mean counts as shallow."""
    from tests import ref64
    with np.errstate(all="ignore"):
        x = ref64.factor_points(cam_mean, lmk_mean, bal)
        p = np.einsum("nij,nj->ni", ref64.rodrigues(x[:, 3:6]), x[:, 6:9]) + x[:, 0:3]
        return ~(np.abs(p[:, 2]) >= DEPTH_LIMIT * np.linalg.norm(x[:, 6:9], axis=1))


SUM_ULPS = 8.0              # float32 ulps by which an operand of a metric term may differ between two float32 evaluations of it


def sum_tolerance(beliefs, bal, K, state):
    """How far two float32 evaluations of the metric of the SAME beliefs may lie apart, to first order, in float64: (for sum_norm, for
    sum_half_sq).  Engine and oracle hold bit-equal beliefs and evaluate z - pi(K (R y + t)) with the same formulas from means solved
    in float64 and rounded to float32; what may differ is the last bits of an operand (a mean's rounding, sin / cos, the order of a
    riding metric's operations).  Every summand of p = R y + t is given SUM_ULPS ulps (2^-23 relative each): |dp| <= c (|R| |y| + |t|),
    c = SUM_ULPS 2^-23; the pixel u = fx p0 / p2 + cx then moves by at most fx (dp0 / |p2| + |p0| dp2 / p2^2) + c (|u - cx| + |cx|),
    v alike; a term's norm by at most du + dv, half its square by at most |r| (du + dv).  The depth p2 in the denominator is what a
    shallow factor amplifies, which is why this is computed and not a constant."""
    from tests import ref64
    c = SUM_ULPS * 2.0 ** -23
    act = np.asarray(state["active_flag"]) == 1
    Km = np.asarray(K, np.float64).reshape(3, 3)
    cm = ref64.belief_means(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6)
    lm = ref64.belief_means(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3)
    x = ref64.factor_points(cm, lm, bal)[act]
    R = ref64.rodrigues(x[:, 3:6])
    p = np.einsum("nij,nj->ni", R, x[:, 6:9]) + x[:, 0:3]
    dp = c * (np.einsum("nij,nj->ni", np.abs(R), np.abs(x[:, 6:9])) + np.abs(x[:, 0:3]))
    z = np.asarray(state["measurements"], np.float64).reshape(-1, 2)[act]
    d = np.zeros(x.shape[0])
    r = np.zeros((x.shape[0], 2))
    for k, (f, c0) in enumerate(((Km[0, 0], Km[0, 2]), (Km[1, 1], Km[1, 2]))):
        u = f * p[:, k] / p[:, 2]
        d += abs(f) * (dp[:, k] / np.abs(p[:, 2]) + np.abs(p[:, k]) * dp[:, 2] / p[:, 2] ** 2) + c * (np.abs(u) + abs(c0))
        r[:, k] = z[:, k] - (u + c0)
    d += c * np.abs(r).sum(axis=1)
    return float(d.sum()), float((np.sqrt((r * r).sum(axis=1)) * d).sum())


def belief_errors(bal, beliefs, priors, messages, active):
    """per tensor: the largest per-variable error of the beliefs against ref64.belief_sums of the given priors and messages"""
    from tests import ref64
    sums = ref64.belief_sums(bal, priors, messages, active)
    got = {"cam_eta": beliefs["cam_beliefs_eta"], "cam_lambda": ref64.lower_mirrored(beliefs["cam_beliefs_lambda"], 6).reshape(-1, 36),
           "lmk_eta": beliefs["lmk_beliefs_eta"], "lmk_lambda": beliefs["lmk_beliefs_lambda"]}
    return {k: float(np.max(ref64.sum_error(got[k], *sums[k]))) for k in BELIEF_TENSORS}


def health(beliefs):
    """what float64 says of float32 beliefs: the non-PD variables (cameras, landmarks), the variables whose mean is non-finite, and
    the smallest distance of a pivot from zero relative to its terms (inf where nothing is finite)"""
    from tests import ref64
    out = {"nonpd": [], "nonfinite": [], "margin": np.inf}
    for who, w in (("cam", 6), ("lmk", 3)):
        lam, eta = beliefs[who + "_beliefs_lambda"], beliefs[who + "_beliefs_eta"]
        D, S = ref64.ldl_pivots(lam, w)
        with np.errstate(all="ignore"):
            out["nonpd"].append(~np.all(D > 0.0, axis=1))
            rel = np.abs(D) / S
        if np.isfinite(rel).any():
            out["margin"] = min(out["margin"], float(np.min(rel[np.isfinite(rel)])))
        out["nonfinite"].append(ref64.nonfinite_means(eta, lam, w))
    out["n_nonpd"] = int(sum(m.sum() for m in out["nonpd"]))
    out["n_nonfinite"] = int(sum(m.sum() for m in out["nonfinite"]))
    return out


def mean_errors(bal, mu, beliefs_before, active):
    """The hoisted means a sweep used (mu [9E]: per ACTIVE factor its camera's and its landmark's mean) against the float64 means of
    the beliefs that stood in front of that sweep, on the variables that are PD with a float64 condition of at most MEAN_COND_LIMIT:
    ({"cam_mean", "lmk_mean": largest per-variable relative error}, share of the variables with an active factor that were left out)"""
    from tests import ref64
    act = np.asarray(active) == 1
    mu = np.asarray(mu, np.float64).reshape(-1, 9)
    err, seen, kept = {}, 0, 0
    for who, w, ids, cols in (("cam", 6, bal["cam_id"], slice(0, 6)), ("lmk", 3, bal["lmk_id"], slice(6, 9))):
        lam = np.asarray(beliefs_before[who + "_beliefs_lambda"], np.float64).reshape(-1, w, w)
        if who == "cam":
            lam = ref64.lower_mirrored(lam, w)      # inv6x6 reads the lower triangle alone
        ids = np.asarray(ids, np.int64)
        used = np.zeros(lam.shape[0], bool)
        used[ids[act]] = True
        ok = used & ref64.positive_definite(beliefs_before[who + "_beliefs_lambda"], w)
        ok[ok] = np.linalg.cond(lam[ok]) <= MEAN_COND_LIMIT
        seen, kept = seen + int(used.sum()), kept + int(ok.sum())
        want = np.zeros((lam.shape[0], w))
        want[ok] = ref64.belief_means(np.asarray(beliefs_before[who + "_beliefs_eta"]).reshape(-1, w)[ok], lam[ok], w)
        sel = act & ok[ids]
        d = np.max(np.abs(mu[sel][:, cols] - want[ids[sel]]), axis=1) / np.max(np.abs(want[ids[sel]]), axis=1)
        err[who + "_mean"] = float(d.max()) if d.size else 0.0
    return err, 1.0 - kept / max(seen, 1)


def metric_errors(ev, beliefs, bal, K, state):
    """one metric record against ref64.metric_terms of the beliefs: ({"sum_norm", "sum_half_sq": |sum - sum64| / sum |term64|}, the
    share of the active factors whose float64 camera-frame depth is below DEPTH_LIMIT of the point's norm).  Such a factor's term is
    not a number float32 can be held to; its share is what the caller caps, and where it is not zero nothing is compared."""
    from tests import ref64
    act = np.asarray(state["active_flag"]) == 1
    with np.errstate(all="ignore"):
        norm, half = ref64.metric_terms(beliefs, bal, K, state["measurements"], state["active_flag"])
        cm = ref64.belief_means(beliefs["cam_beliefs_eta"], beliefs["cam_beliefs_lambda"], 6)
        lm = ref64.belief_means(beliefs["lmk_beliefs_eta"], beliefs["lmk_beliefs_lambda"], 3)
        shallow = shallow_factors(cm, lm, bal)[act]
    err = {"sum_norm": abs(ev["sum_norm"] - norm.sum()) / norm.sum(), "sum_half_sq": abs(ev["sum_half_sq"] - half.sum()) / half.sum()}
    return err, float(shallow.sum()) / max(int(act.sum()), 1)


# ---- leg H: six sweeps, the metric after each one through every call that computes it ---------------------------------------------------
H_STEPS = 3
H_CALLS = ("eval", "ba_loop", "iterate_eval_each", "iterate_eval_each", "eval", "ba_loop")      # loop indices 0 .. 5; gbp_ba_loop weakens in front of 1 and 5


def weakens(i, steps):
    """the reference's loop weakens the priors in front of the pass of loop index i (ba.cpp:1003-1006)"""
    return (i + 1) % 2 == 0 and i < 2 * steps


def metric_sweeps(x, native):
    """Runs H_CALLS on x (uploaded and linearised) and yields (loop index, call, metric record) behind every sweep.  native: x has
    iterate_eval_each and ba_loop (an engine); otherwise (the oracle, a shard group) the calls they stand for are made one by one."""
    for i, call in enumerate(H_CALLS):
        if call == "ba_loop" and native:
            ev = x.ba_loop(1, i, H_STEPS)[0]
        elif call == "iterate_eval_each" and native:
            ev = x.iterate_eval_each(1)[0]
        else:
            if call == "ba_loop" and weakens(i, H_STEPS):
                x.weaken_priors()
            x.iterate(1)
            ev = x.eval()
        yield i, call, ev


_METRIC_STATES = {}


def metric_state(oracle_mod, key, bal, state, K, make_oracle):
    """`state` with the factors switched off whose float64 camera-frame depth falls below DEPTH_LIMIT of the point's norm behind any
    sweep of leg H: a sum cannot leave a term out, so such factors leave the graph.  Found on the CPU oracle (which the engines equal bit
    for bit): run, switch off what was shallow, run again, until a run has none (at most METRIC_ROUNDS rounds).  Returns (state, share of the
    originally active factors switched off).  Kept per `key`."""
    from tests import ref64
    if key in _METRIC_STATES:
        return _METRIC_STATES[key]
    n0 = int((state["active_flag"] == 1).sum())
    st = dict(state, active_flag=state["active_flag"].copy())
    for _ in range(METRIC_ROUNDS):
        o = make_oracle()
        o.upload(st)
        o.linearise()
        act = st["active_flag"] == 1
        shallow = np.zeros(act.size, bool)
        for _i, _call, _ev in metric_sweeps(o, native=False):
            b = o.read()
            assert all_finite(b), "%r: the oracle's beliefs are not finite" % (key,)
            with np.errstate(all="ignore"):
                cm = ref64.belief_means(b["cam_beliefs_eta"], b["cam_beliefs_lambda"], 6)
                lm = ref64.belief_means(b["lmk_beliefs_eta"], b["lmk_beliefs_lambda"], 3)
                shallow |= act & shallow_factors(cm, lm, bal)
        o.close()
        if not shallow.any():
            break
        st["active_flag"][shallow] = 0
    else:
        raise AssertionError("%r: factors kept turning shallow" % (key,))
    out = _METRIC_STATES[key] = (st, 1.0 - int((st["active_flag"] == 1).sum()) / n0)
    return out


# ---- what the tests run ----------------------------------------------------------------------------------------------------------------
# graph -> (seed, decades the ranges were narrowed by).  Chosen among the first 200 seeds as the first (or, where the first sits on the
# edge of a condition, a later) seed that meets the conditions tests/test_wide_state_cpu.py asserts; "gather" and "rows" have no seed at
# the full ranges of WIDE that stays finite through the program and keeps half of its beliefs PD, and run one decade narrower.
WIDE_CASES = {"probe": (41, 0.0), "gather": (37, 1.0), "rows": (103, 1.0), "fuzz": (41, 0.0)}
# leg H against float64: (seed, narrowed) per graph AND per summation order (1: one device; 2, 3: a shard group's) — its sweeps are
# others than W's, and the orders' sweeps part after a rounding, so a seed whose shallow factors settle in one order need not settle in
# another.  The first seed of the first 200 that meets the conditions, at the widest ranges that have one; profiles/wide_state.md lists
# the seeds and ranges tried for each entry and for the orders that have none.  (The counters of leg H, and its sums against the oracle,
# run on WIDE_CASES: every graph, every order.)
METRIC_CASES = {"probe": {1: (41, 0.0), 2: (41, 0.0), 3: (41, 0.0)},
                "gather": {1: (36, 2.0), 2: (50, 2.0), 3: (0, 3.0)},
                "rows": {1: (40, 2.0), 2: (191, 1.0), 3: (40, 2.0)},
                "fuzz": {1: (99, 0.0), 2: (9, 0.0), 3: (41, 0.0)}}
RELIN_CASES = {"probe": (165, 0.0), "gather": (26, 0.0), "rows": (51, 0.0), "fuzz": (105, 0.0)}
NONFINITE_CASES = {"probe": 0, "gather": 0, "rows": 0, "fuzz": 0}
PLACEMENT_SEED = 0


def wide_case(name):
    bal = graph(name)
    seed, narrow = WIDE_CASES[name]
    state, K = wide_state(bal, seed, "wide", ranges=narrowed(WIDE, narrow))
    return bal, state, K


def metric_base_case(name, world=1):
    bal = graph(name)
    seed, narrow = METRIC_CASES[name][world]
    state, K = wide_state(bal, seed, "wide", ranges=narrowed(WIDE, narrow))
    return bal, state, K


def relin_case(name):
    bal = graph(name)
    seed, narrow = RELIN_CASES[name]
    state, K = wide_state(bal, seed, "wide", ranges=narrowed(RELIN, narrow), damping_count=RELIN_COUNT)
    return bal, state, K


def nonfinite_case(name):
    bal = graph(name)
    state, K = wide_state(bal, NONFINITE_CASES[name], "nonfinite")
    return bal, state, K


def placement_case(name):
    bal = graph(name)
    state, K = wide_state(bal, PLACEMENT_SEED, "placement")
    return bal, state, K


def all_finite(arrays):
    return all(bool(np.all(np.isfinite(v))) for v in arrays.values())


def nonfinite_variables(beliefs):
    """per variable (cameras, then landmarks): does its belief eta or Lambda hold a non-finite number?"""
    out = []
    for who, w in (("cam", 6), ("lmk", 3)):
        out.append(~np.all(np.isfinite(beliefs[who + "_beliefs_eta"].reshape(-1, w)), axis=1)
                   | ~np.all(np.isfinite(beliefs[who + "_beliefs_lambda"].reshape(-1, w * w)), axis=1))
    return np.concatenate(out)


def expected_priors(state, bal, k):
    """the uploaded priors after k WEAKEN_PRIORS, in float64: prior x scaling^weakenings_applied(flag, k)"""
    out = {}
    for who, we, wl in (("cam", 6, 36), ("lmk", 3, 9)):
        f = np.asarray(state[who + "_scaling"], np.float64) ** weakenings_applied(state[who + "_weaken_flag"], k)
        out[who + "_priors_eta"] = (np.asarray(state[who + "_priors_eta"], np.float64).reshape(-1, we) * f[:, None]).ravel()
        out[who + "_priors_lambda"] = (np.asarray(state[who + "_priors_lambda"], np.float64).reshape(-1, wl) * f[:, None]).ravel()
    return out


def ulps_off(got_f32, want_f64):
    """largest distance of float32 numbers from float64 ones in units of the float32 spacing at the wanted number"""
    want = np.asarray(want_f64, np.float64)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        d = np.abs(np.asarray(got_f32, np.float64) - want) / ulp
    return float(np.max(d)) if d.size else 0.0
