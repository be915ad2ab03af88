"""The CPU oracle alone on the states of tests/wide_state.py, against float64 (tests/ref64.py): the constants and the conditions
tests/test_gpu_wide_state.py rests on.

Every whole-graph test but these gets its inputs from driver.build_inputs: one variance, one prior block, one scaling, one flag, zero
damping — so a stream read from the wrong factor or variable changes nothing, and the variable side (beliefs, hoisted means, the
health counters, the metric records) only ever sees benign numbers.  Here every stream is drawn per factor / per variable, and the
"wide" profile draws full SPD priors over eight decades and variances over six.

HOW THE BOUNDS WERE SET.  As in tests/test_exact_inference.py: the oracle (restatement, device summation order, correctly rounded
trigonometry) ran every chosen (graph, seed); its error against float64 is *_ORACLE below, the largest over the graphs and over every
stage of the program.  Every engine has to meet 8 x that (float32 additions in another order), metric sums 4 x.  The measures:

  beliefs        per variable, max |belief - sum64| / max sum |terms| over the variable's entries, sum64 = ref64.belief_sums of the
                 priors and messages the same engine holds.  A camera's Lambda on its lower triangle: the upper triangle of a camera
                 message is not kept by the engines, and with beliefs that are not PD the two triangles differ by far more than rounding.
  hoisted means  per variable, ||mu - mean64||_inf / ||mean64||_inf against the float64 solve of the belief that stood in front of the
                 sweep, on PD variables of float64 condition <= 1e4 (the others' means are not numbers float32 can be held to);
                 how many are left out is asserted (cap: half).
  metric         |sum - sum64| / sum |term64| per record.  A factor whose float64 camera-frame depth is below 1e-2 of the point's norm
                 |y| (wide_state.shallow_factors) has a term float32 cannot be held to; a SUM cannot leave a term out, so leg H runs on wide_state.metric_state(): those
                 factors switched off, found on the oracle, their share asserted (cap: 10 %).  On the W states themselves (which
                 have shallow factors) the counters are checked all the same, and the sums against an oracle of the same summation
                 order within wide_state.sum_tolerance, a first-order float32 bound computed per record (run_counters).

What is asserted per (graph, seed) is what the GPU file takes for granted: finite where promised; between 10 % and 60 % of the
variables non-PD somewhere in the run and at least half PD at every stage; no LDL^T pivot within 1e-6 (relative) of zero, so the
health predicates are decided; at least 10 relinearisations on the relinearising leg; non-finite beliefs on the non-finite leg.
profiles/wide_state.md has the figures per graph, and the device's."""
import numpy as np
import pytest

from tests import ref64
from tests import wide_state as ws
from tests.test_exact_inference import _oracle, rounded_trig  # noqa: F401

GRAPHS = ws.GRAPHS

# ---- measured on the CPU oracle against ref64 (largest over the four graphs and every stage); see the module docstring --------------
W_ORACLE = {"cam_eta": 1.22e-7, "cam_lambda": 1.93e-7, "lmk_eta": 2.78e-7, "lmk_lambda": 3.03e-7}
M_ORACLE = {"cam_mean": 6.57e-6, "lmk_mean": 1.47e-4}
# H per graph AND per summation order (1: one device, 2 / 3: a shard group's), for the cases wide_state.METRIC_CASES has: these runs
# amplify a rounding, the orders' sweeps part, and the figure is set by whichever terms come next to the depth limit.
H_ORACLE = {"probe": {1: (9.43e-7, 5.86e-6), 2: (1.81e-6, 6.06e-6), 3: (1.04e-6, 4.50e-6)},
            "gather": {1: (4.83e-7, 2.90e-6), 2: (2.90e-6, 3.66e-5), 3: (1.85e-6, 1.85e-5)},
            "rows": {1: (2.80e-7, 5.12e-6), 2: (5.49e-7, 1.36e-5), 3: (3.80e-7, 8.80e-6)},
            "fuzz": {1: (4.84e-7, 2.89e-6), 2: (1.43e-6, 6.26e-6), 3: (2.11e-6, 2.00e-5)}}
assert {g: set(per) for g, per in H_ORACLE.items()} == {g: set(per) for g, per in ws.METRIC_CASES.items()}
H_ORACLE = {g: {w: dict(zip(("sum_norm", "sum_half_sq"), v)) for w, v in per.items()} for g, per in H_ORACLE.items()}
H_ORDERS = [(g, w) for g in GRAPHS for w in H_ORACLE[g]]
W_BOUND = {k: 8.0 * v for k, v in W_ORACLE.items()}
M_BOUND = {k: 8.0 * v for k, v in M_ORACLE.items()}
H_BOUND = {g: {w: {k: 4.0 * v for k, v in d.items()} for w, d in per.items()} for g, per in H_ORACLE.items()}
NONPD_SHARE = (0.10, 0.60)
MIN_RELINEARISATIONS = 10
MESSAGE_SHARE = 1e-3


def _sum_order(bal, world):
    """the landmark ranges of a `world`-shard group (None: one device): the order the oracle adds a camera's messages in"""
    from gbp_poplar_amd.distributed import landmark_partition
    return None if world == 1 else landmark_partition(bal["lmk_id"], bal["n_lmks"], world)


# ---- the graphs and the placement state ---------------------------------------------------------------------------------------------
def test_graphs_are_what_they_are_for():
    from gbp_poplar_amd import hostlib
    from tests import fuzz_support
    for name in GRAPHS:
        bal = ws.graph(name)
        assert 100 <= bal["n_edges"] <= 3200, (name, bal["n_edges"])
        pos_edge = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])["pos_edge"]
        assert (pos_edge == 0xFFFFFFFF).any(), name                     # padded rows
    bal = ws.graph("probe")
    assert (bal["n_cams"], bal["n_lmks"]) == (6, 40) and 100 <= bal["n_edges"] <= 160
    bal = ws.graph("fuzz")
    t = fuzz_support.graph_traits(bal)
    assert not t["sorted"] and t["duplicates"]
    pos_edge = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])["pos_edge"]
    real = pos_edge[pos_edge != 0xFFFFFFFF]
    assert not np.array_equal(real, np.arange(real.size))                # device order differs from file order


@pytest.mark.parametrize("name", GRAPHS)
def test_placement_state_is_nonuniform_and_exact(name):
    bal, state, K = ws.placement_case(name)
    assert K[0] == 500.0 and K[4] == ws.FY
    assert set(np.unique(state["meas_variances"])) == set(np.float32(ws.PLACEMENT_VARIANCES))
    assert set(np.unique(state["damping"])) == set(np.float32(ws.PLACEMENT_DAMPING))
    assert state["damping_count"].min() == -15 and state["damping_count"].max() == 3
    assert 0.05 <= 1.0 - state["active_flag"].mean() <= 0.25
    for who in ("cam", "lmk"):
        assert set(np.unique(state[who + "_scaling"])) <= set(np.float32(ws.PLACEMENT_SCALINGS)) and np.unique(state[who + "_scaling"]).size >= 2
        assert set(np.unique(state[who + "_weaken_flag"])) <= set(range(8)) and np.unique(state[who + "_weaken_flag"]).size >= 3
    for k, v in state.items():
        assert v.dtype in (np.float32, np.int32, np.uint32), k
    again, _ = ws.wide_state(bal, ws.PLACEMENT_SEED, "placement")
    for k in state:
        assert np.array_equal(state[k], again[k]), k                      # a pure function of its arguments


@pytest.mark.parametrize("name", GRAPHS)
def test_weakened_priors_follow_the_flags_on_the_oracle(name, oracle_mod, rounded_trig):
    """P's float64 side: after the k-th weakening the priors are the upload x scaling^n, n = min(flag, k) for flags 1 .. 5 and 0 for
    flags 0, 6 and 7 (WeakenPriorVertex acts on 1 .. 5 only: a flag above 5 never counts down) — exactly, the placement values being
    powers of two."""
    bal, state, K = ws.placement_case(name)
    orc = _oracle(oracle_mod, bal, K)
    orc.upload(state)
    for k in range(1, 7):
        orc.weaken_priors()
        got, want = orc.read_priors(), ws.expected_priors(state, bal, k)
        for t in want:
            assert ws.ulps_off(got[t], want[t]) == 0.0, (k, t)
    assert np.any(ws.weakenings_applied(state["lmk_weaken_flag"], 6) == 5) and np.any(state["lmk_weaken_flag"] > 5)


# ---- W: the program on the wide profile -------------------------------------------------------------------------------------------------
def run_wide(x, bal, state, K, what, after=None):
    """the program of legs P and W on x: per-stage float64 figures.  Returns a dict of the largest / smallest over the stages.
    after(stage): called behind every step, in front of the float64 figures (the GPU file compares with the oracle there)."""
    nv = bal["n_cams"] + bal["n_lmks"]
    rec = {"finite": True, "ever": np.zeros(nv, bool), "min_pd": 1.0, "margin": np.inf, "belief": dict.fromkeys(ws.BELIEF_TENSORS, 0.0),
           "mean": {"cam_mean": 0.0, "lmk_mean": 0.0}, "means_left_out": 0.0, "max_lambda": 0.0}
    before = [None]

    def do(verb, *a):
        if verb == "iterate":
            before[0] = x.read()
        getattr(x, verb)(*a)
        if verb == "iterate" and a[0] == 1 and rec["finite"]:
            err, left = ws.mean_errors(bal, x.mu()[0], before[0], state["active_flag"])
            rec["means_left_out"] = max(rec["means_left_out"], left)
            rec["mean"] = {k: max(v, err[k]) for k, v in rec["mean"].items()}

    def check(stage, k):
        if after is not None:
            after(stage)
        b, m = x.read(), x.messages()
        if not (ws.all_finite(b) and ws.all_finite(m)):
            rec["finite"] = False
            return
        h = ws.health(b)
        npd = np.concatenate(h["nonpd"])
        rec["ever"] |= npd
        rec["min_pd"], rec["margin"] = min(rec["min_pd"], 1.0 - npd.mean()), min(rec["margin"], h["margin"])
        rec["max_lambda"] = max(rec["max_lambda"], float(np.max(np.abs(m["cam_lambda"]))), float(np.max(np.abs(m["lmk_lambda"]))))
        err = ws.belief_errors(bal, b, x.read_priors(), m, state["active_flag"])
        rec["belief"] = {t: max(v, err[t]) for t, v in rec["belief"].items()}
        ev = x.eval()
        assert ev["n_nonpd"] == h["n_nonpd"] and ev["n_nonfinite"] == h["n_nonfinite"], (stage, ev, h["n_nonpd"], h["n_nonfinite"])

    x.upload(state)
    ws.program(do, check)
    rec["ever"] = float(rec["ever"].mean())
    print("W %s: finite %s, non-PD somewhere %.2f, PD at least %.2f, pivot margin %.1e, |message Lambda| up to %.1e | beliefs %s | means %s, left out %.2f"
          % (what, rec["finite"], rec["ever"], rec["min_pd"], rec["margin"], rec["max_lambda"], "  ".join("%s %.2e" % kv for kv in rec["belief"].items()),
             "  ".join("%s %.2e" % kv for kv in rec["mean"].items()), rec["means_left_out"]))
    return rec


def assert_wide_conditions(rec, what):
    assert rec["finite"], what
    assert NONPD_SHARE[0] <= rec["ever"] <= NONPD_SHARE[1], (what, rec["ever"])
    assert rec["min_pd"] >= 0.5, (what, rec["min_pd"])
    assert rec["margin"] >= ws.PIVOT_MARGIN, (what, rec["margin"])
    assert rec["means_left_out"] <= ws.MEAN_LEFT_OUT_CAP, (what, rec["means_left_out"])


def assert_wide_bounds(rec, what):
    for t in ws.BELIEF_TENSORS:
        assert rec["belief"][t] <= W_BOUND[t], (what, t, rec["belief"][t], W_BOUND[t])
    for t in M_BOUND:
        assert rec["mean"][t] <= M_BOUND[t], (what, t, rec["mean"][t], M_BOUND[t])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_conditions_hold_in_the_sharded_summation_orders_too(name, world, oracle_mod, rounded_trig):
    """a shard group adds a camera's messages rank by rank: other roundings, on which the same conditions and bounds must hold"""
    bal, state, K = ws.wide_case(name)
    rec = run_wide(_oracle(oracle_mod, bal, K, bounds=_sum_order(bal, world)), bal, state, K, "oracle %s in the order of %d shards" % (name, world))
    assert_wide_conditions(rec, (name, world))
    assert_wide_bounds(rec, (name, world))


@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_on_the_wide_state(name, oracle_mod, rounded_trig):
    bal, state, K = ws.wide_case(name)
    rec = run_wide(_oracle(oracle_mod, bal, K), bal, state, K, "oracle %s seed %d narrowed %g" % ((name,) + ws.WIDE_CASES[name]))
    assert_wide_conditions(rec, name)
    assert_wide_bounds(rec, name)
    for t in ws.BELIEF_TENSORS:                    # the recorded figures are the oracle's: none of them is out of date by a factor of two
        assert rec["belief"][t] <= 1.05 * W_ORACLE[t], (t, rec["belief"][t])
    for t in M_ORACLE:
        assert rec["mean"][t] <= 1.05 * M_ORACLE[t], (t, rec["mean"][t])


# ---- H: health counters and the metric ---------------------------------------------------------------------------------------------------
def metric_case(oracle_mod, name, world=1):
    """leg H's state for a summation order (a group of `world` shards rounds otherwise, and these runs amplify a rounding: which
    factors turn shallow, and the figure the terms next to the limit set, belong to the order)"""
    bal, state, K = ws.metric_base_case(name, world)
    st, off = ws.metric_state(oracle_mod, ("H", name, world) + ws.METRIC_CASES[name][world], bal, state, K,
                              lambda: _oracle(oracle_mod, bal, K, bounds=_sum_order(bal, world)))
    return bal, st, K, off


def run_metric(x, native, bal, state, K, what):
    """leg H on x alone: the counters exactly, the sums against float64; returns the largest errors"""
    x.upload(state)
    x.linearise()
    worst, seen_nonpd = {"sum_norm": 0.0, "sum_half_sq": 0.0}, 0
    for i, call, ev in ws.metric_sweeps(x, native):
        b = x.read()
        assert ws.all_finite(b), (what, i)
        h = ws.health(b)
        assert h["margin"] >= ws.PIVOT_MARGIN, (what, i, h["margin"])
        err, shallow = ws.metric_errors(ev, b, bal, K, state)
        print("H %s sweep %d %-17s n_nonpd %3d n_nonfinite %d | sum_norm %.6e off by %.2e, sum_half_sq off by %.2e"
              % (what, i, call, ev["n_nonpd"], ev["n_nonfinite"], ev["sum_norm"], err["sum_norm"], err["sum_half_sq"]))
        assert shallow == 0.0, (what, i, shallow)
        assert ev["n_active"] == int((state["active_flag"] == 1).sum())
        assert ev["n_nonpd"] == h["n_nonpd"], (what, i, call, ev["n_nonpd"], h["n_nonpd"])
        assert ev["n_nonfinite"] == h["n_nonfinite"], (what, i, call, ev["n_nonfinite"], h["n_nonfinite"])
        seen_nonpd = max(seen_nonpd, h["n_nonpd"])
        worst = {k: max(v, err[k]) for k, v in worst.items()}
    assert seen_nonpd > 0, what
    return worst


def run_counters(x, native, bal, state, K, what, shadow=None):
    """Leg H on the wide state as W uploads it, on every graph: behind every sweep, through gbp_eval, gbp_iterate_eval_each and
    gbp_ba_loop, n_nonpd and n_nonfinite exactly against float64 on x's own beliefs.  shadow: an oracle of x's summation order that
    makes the same calls one by one; its beliefs must equal x's bit for bit, its other counters x's, and its sums x's within
    wide_state.sum_tolerance (the float64 reference cannot be held here: the state has shallow factors).
    Returns per sweep (tolerance of sum_norm, |sum_norm - sum64 with every landmark index shifted by one|)."""
    x.upload(state)
    x.linearise()
    mine = ws.metric_sweeps(x, native)
    if shadow is not None:
        shadow.upload(state)
        shadow.linearise()
        mine = zip(mine, ws.metric_sweeps(shadow, False))
    seen_nonpd, out = 0, []
    for step in mine:
        (i, call, ev), other = step if shadow is not None else (step, None)
        b = x.read()
        assert ws.all_finite(b), (what, i)
        h = ws.health(b)
        assert h["margin"] >= ws.PIVOT_MARGIN, (what, i, h["margin"])
        assert ev["n_active"] == int((state["active_flag"] == 1).sum())
        assert ev["n_nonpd"] == h["n_nonpd"], (what, i, call, ev["n_nonpd"], h["n_nonpd"])
        assert ev["n_nonfinite"] == h["n_nonfinite"] == 0, (what, i, call, ev["n_nonfinite"], h["n_nonfinite"])
        seen_nonpd = max(seen_nonpd, h["n_nonpd"])
        tol = ws.sum_tolerance(b, bal, K, state)
        wrong = ref64.metric_terms(b, bal, K, state["measurements"], state["active_flag"], lmk_shift=1)[0].sum()
        out.append((tol[0], abs(wrong - ev["sum_norm"])))
        if other is not None:
            ob, oev = shadow.read(), other[2]
            for k in ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda"):
                assert np.array_equal(b[k], ob[k]), (what, i, k)
            for k in ("n_active", "n_relin", "n_robust", "n_nonpd", "n_nonfinite"):
                assert ev[k] == oev[k], (what, i, call, k, ev[k], oev[k])
            d = (abs(ev["sum_norm"] - oev["sum_norm"]), abs(ev["sum_half_sq"] - oev["sum_half_sq"]))
            print("H %s sweep %d %-17s n_nonpd %3d | sum_norm %.9e, %.2e from the oracle's (tolerance %.2e); sum_half_sq %.2e (tolerance %.2e)"
                  % (what, i, call, ev["n_nonpd"], ev["sum_norm"], d[0], tol[0], d[1], tol[1]))
            assert d[0] <= tol[0] and d[1] <= tol[1], (what, i, call, d, tol)
    assert seen_nonpd > 0, what
    return out


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_health_counters_on_every_graph(name, world, oracle_mod, rounded_trig):
    """the conditions of leg H's counters on the W state, in every summation order; and the tolerance of the sums is not blind: in at
    least half of the sweeps the float64 sum with every landmark index shifted by one lies 100 tolerances and more away"""
    bal, state, K = ws.wide_case(name)
    out = run_counters(_oracle(oracle_mod, bal, K, bounds=_sum_order(bal, world)), False, bal, state, K, "oracle %s, order of %d" % (name, world))
    sees = [wrong >= 100.0 * tol for tol, wrong in out]
    print("H counters, oracle %s in the order of %d: wrong landmark / tolerance per sweep %s" % (name, world, " ".join("%.0f" % (w / t) for t, w in out)))
    assert sum(sees) >= len(sees) // 2, sees


@pytest.mark.parametrize("name, world", H_ORDERS)
def test_oracle_health_counters_and_metric(name, world, oracle_mod, rounded_trig):
    bal, state, K, off = metric_case(oracle_mod, name, world)
    assert off <= ws.METRIC_LEFT_OUT_CAP, off
    worst = run_metric(_oracle(oracle_mod, bal, K, bounds=_sum_order(bal, world)), False, bal, state, K, "oracle %s, order of %d" % (name, world))
    print("H oracle %s seed %d narrowed %g, order of %d shard(s): %.3f of the active factors switched off as shallow, worst %s"
          % ((name,) + ws.METRIC_CASES[name][world] + (world, off, "  ".join("%s %.3e" % kv for kv in worst.items()))))
    for k, bound in H_BOUND[name][world].items():
        assert worst[k] <= bound, (name, world, k, worst[k])
        assert worst[k] <= 1.05 * H_ORACLE[name][world][k], (name, world, k, worst[k])


# ---- R and N: the conditions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_relinearises_on_the_relinearising_leg(name, oracle_mod, rounded_trig):
    """at least MIN_RELINEARISATIONS real ones: active factors whose potential changed in a sweep (n_relin also counts the inactive
    factors, whose uploaded count of -1 never moves)"""
    bal, state, K = ws.relin_case(name)
    orc = _oracle(oracle_mod, bal, K, **ws.RELIN_PARAMS)
    orc.upload(state)
    orc.linearise()
    changed, n_relin = 0, []
    fe = orc.factor_potentials()[0].reshape(-1, 9).copy()
    for _ in range(ws.RELIN_SWEEPS):
        orc.iterate(1)
        f2 = orc.factor_potentials()[0].reshape(-1, 9)
        changed += int(np.sum(np.any(f2 != fe, axis=1)))
        fe = f2.copy()
        n_relin.append(orc.eval()["n_relin"])
    b = orc.read()
    print("R %s seed %d narrowed %g: %d relinearisations in %d sweeps (n_relin per sweep %s)" % ((name,) + ws.RELIN_CASES[name] + (changed, ws.RELIN_SWEEPS, n_relin)))
    assert ws.all_finite(b) and ws.all_finite(orc.messages())
    assert changed >= MIN_RELINEARISATIONS, changed


@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_turns_nonfinite_on_the_nonfinite_leg(name, oracle_mod, rounded_trig):
    bal, state, K = ws.nonfinite_case(name)
    orc = _oracle(oracle_mod, bal, K)
    orc.upload(state)
    orc.linearise()
    orc.iterate(1)
    bad = ws.nonfinite_variables(orc.read())
    print("N %s seed %d: %d of %d variables non-finite after one sweep" % (name, ws.NONFINITE_CASES[name], bad.sum(), bad.size))
    assert 0 < bad.sum() < bad.size


# ---- not blind ------------------------------------------------------------------------------------------------------------------------------
def _beliefs_after(oracle_mod, bal, K, state, weakenings=0, sweeps=1):
    orc = _oracle(oracle_mod, bal, K)
    orc.upload(state)
    orc.linearise()
    for _ in range(weakenings):
        orc.weaken_priors()
    dampings = []
    for _ in range(sweeps):
        orc.iterate(1)
        dampings.append(orc.read()["damping"].copy())
    b = orc.read()
    scale = ref64.belief_sums(bal, orc.read_priors(), orc.messages(), state["active_flag"])
    return b, scale, dampings


def _moved(bal, a, b, scale):
    """per variable (cameras, landmarks): the largest of the four tensors' distances between two sets of beliefs, in the belief
    measure, over the bound of its tensor"""
    out = []
    for who, w in (("cam", 6), ("lmk", 3)):
        r = 0.0
        for t, width in ((who + "_eta", w), (who + "_lambda", w * w)):
            key = "%s_beliefs_%s" % (who, t.split("_")[1])
            ga, gb = a[key], b[key]
            if t == "cam_lambda":
                ga, gb = ref64.lower_mirrored(ga, 6).reshape(-1, 36), ref64.lower_mirrored(gb, 6).reshape(-1, 36)
            r = np.maximum(r, ref64.sum_error(ga, np.asarray(gb, np.float64).reshape(-1, width), scale[t][1]) / W_BOUND[t])
        out.append(r)
    return out


def _bits_differ(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda"))


def _roll(a):
    return np.roll(a, 1)


def _affected_by_factors(bal, factors):
    cams, lmks = np.zeros(bal["n_cams"], bool), np.zeros(bal["n_lmks"], bool)
    cams[bal["cam_id"][factors]] = True
    lmks[bal["lmk_id"][factors]] = True
    return cams, lmks


def _swap(a, width, i, j):
    a = a.reshape(-1, width).copy()
    a[[i, j]] = a[[j, i]]
    return a.ravel()


def _pair(values, ok):
    """two indices among `ok` whose values differ"""
    idx = np.flatnonzero(ok)
    for j in idx[1:]:
        if values[j] != values[idx[0]]:
            return int(idx[0]), int(j)
    raise AssertionError("no two variables differ")


@pytest.mark.parametrize("what", ["meas_variances", "damping", "damping_count", "priors", "scalings", "weaken_flags"])
@pytest.mark.parametrize("name", ["probe", "fuzz"])
def test_placement_streams_are_not_blind(name, what, oracle_mod, rounded_trig):
    """A stream that reached the wrong factor or variable is seen.  On the oracle, with the placement state: the perturbed upload
    changes belief bits, and moves the beliefs of at least 90 % of the variables it concerns by at least 100 x the bound of leg W
    (the distance taken in float64, in W's measure; the bound of the bit-for-bit leg P itself is zero)."""
    bal, state, K = ws.placement_case(name)
    act = state["active_flag"] == 1
    C = bal["n_cams"]
    weakenings, sweeps = 0, 1
    if what in ("meas_variances", "damping"):
        wrong = dict(state, **{what: _roll(state[what])})
    elif what == "damping_count":
        wrong, sweeps = dict(state, damping_count=_roll(state["damping_count"])), 2
    else:
        cdeg = np.bincount(bal["cam_id"][act], minlength=C) > 0
        ldeg = np.bincount(bal["lmk_id"][act], minlength=bal["n_lmks"]) > 0
        wrong, pairs = dict(state), {}
        for who, we, seen in (("cam", 6, cdeg), ("lmk", 3, ldeg)):
            flag, scal = state[who + "_weaken_flag"], state[who + "_scaling"]
            if what == "priors":
                i, j = _pair(state[who + "_priors_lambda"].reshape(-1, we * we)[:, 0], seen & (state[who + "_priors_lambda"].reshape(-1, we * we)[:, 0] != 0))
                wrong[who + "_priors_eta"] = _swap(state[who + "_priors_eta"], we, i, j)
                wrong[who + "_priors_lambda"] = _swap(state[who + "_priors_lambda"], we * we, i, j)
            elif what == "scalings":
                weakenings = 1
                i, j = _pair(scal, seen & (flag >= 1) & (flag <= 5) & (state[who + "_priors_lambda"].reshape(-1, we * we)[:, 0] != 0))
                wrong[who + "_scaling"] = _swap(scal, 1, i, j)
            else:
                weakenings = 6
                n = ws.weakenings_applied(flag, 6)
                i, j = _pair(n, seen & (state[who + "_priors_lambda"].reshape(-1, we * we)[:, 0] != 0))
                wrong[who + "_weaken_flag"] = _swap(flag, 1, i, j)
            pairs[who] = (i, j)
    a, scale, da = _beliefs_after(oracle_mod, bal, K, state, weakenings, sweeps)
    b, _, db = _beliefs_after(oracle_mod, bal, K, wrong, weakenings, sweeps)
    assert _bits_differ(a, b)
    if what == "meas_variances":
        cams, lmks = _affected_by_factors(bal, act & (state[what] != wrong[what]))
    elif what in ("damping", "damping_count"):      # the factors whose eta damping in one of the sweeps was another
        cams, lmks = _affected_by_factors(bal, act & np.any([x != y for x, y in zip(da, db)], axis=0))
    else:
        cams, lmks = np.zeros(C, bool), np.zeros(bal["n_lmks"], bool)
        cams[list(pairs["cam"])] = True
        lmks[list(pairs["lmk"])] = True
    mc, ml = _moved(bal, a, b, scale)
    moved = np.concatenate([mc[cams], ml[lmks]])
    share = float(np.mean(moved >= 100.0))
    print("not blind, %s / %s: %d variables concerned, %.0f %% moved by >= 100 x the bound (median %.0f x)" % (name, what, moved.size, 100 * share, np.median(moved)))
    assert moved.size >= 4 and share >= 0.9, (moved.size, share)


@pytest.mark.parametrize("name", GRAPHS)
def test_belief_sums_are_not_blind_to_a_missing_message(name, oracle_mod, rounded_trig):
    """Every message whose share of its variable's sum |terms| is at least 1e-3 moves the float64 sum, taken out, by at least 100 x the
    bound — and most messages have such a share.  And on the oracle: with such a factor switched off at the upload, one sweep leaves
    other belief bits on both of its variables."""
    bal, state, K = ws.wide_case(name)
    orc = _oracle(oracle_mod, bal, K)
    orc.upload(state)
    orc.linearise()
    orc.iterate(2)
    pri, msg = orc.read_priors(), orc.messages()
    full = ref64.belief_sums(bal, pri, msg, state["active_flag"])
    act = np.flatnonzero(state["active_flag"] == 1)
    big = checked = 0
    for e in act[:: max(1, act.size // 120)]:
        off = state["active_flag"].copy()
        off[e] = 0
        less = ref64.belief_sums(bal, pri, msg, off)
        for t, ids, w in (("cam_lambda", bal["cam_id"], 36), ("lmk_lambda", bal["lmk_id"], 9)):
            v = int(ids[e])
            m = ref64.lower_mirrored(msg["cam_lambda"], 6).reshape(-1, 36)[e] if t == "cam_lambda" else np.asarray(msg[t], np.float64).reshape(-1, w)[e]
            share = np.max(np.abs(m)) / np.max(full[t][1][v])
            checked += 1
            if share >= MESSAGE_SHARE:
                big += 1
                moved = float(ref64.sum_error(less[t][0], full[t][0], full[t][1])[v])
                assert moved >= 100.0 * W_BOUND[t], (e, t, share, moved)
    print("missing message, %s: %d of %d messages have a share >= %g" % (name, big, checked, MESSAGE_SHARE))
    assert big >= 0.5 * checked

    def after_one_sweep(active):
        o = _oracle(oracle_mod, bal, K)
        o.upload(dict(state, active_flag=active))
        o.linearise()
        o.iterate(1)
        return o.read(), o.messages()

    base, msg1 = after_one_sweep(state["active_flag"])
    full1 = ref64.belief_sums(bal, orc.read_priors(), msg1, state["active_flag"])
    tried = 0
    for e in act:
        c, l = int(bal["cam_id"][e]), int(bal["lmk_id"][e])
        shares = (np.max(np.abs(ref64.lower_mirrored(msg1["cam_lambda"], 6).reshape(-1, 36)[e])) / np.max(full1["cam_lambda"][1][c]),
                  np.max(np.abs(np.asarray(msg1["lmk_lambda"], np.float64).reshape(-1, 9)[e])) / np.max(full1["lmk_lambda"][1][l]))
        if min(shares) < MESSAGE_SHARE:
            continue
        off = state["active_flag"].copy()
        off[e] = 0
        other, _ = after_one_sweep(off)
        assert not np.array_equal(other["cam_beliefs_lambda"].reshape(-1, 36)[c], base["cam_beliefs_lambda"].reshape(-1, 36)[c]), e
        assert not np.array_equal(other["lmk_beliefs_lambda"].reshape(-1, 9)[l], base["lmk_beliefs_lambda"].reshape(-1, 9)[l]), e
        tried += 1
        if tried == 6:
            break
    assert tried == 6
