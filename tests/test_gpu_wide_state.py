"""Every path of the library on the states of tests/wide_state.py: per-factor variances, damping, counts and flags, per-variable
scalings, weaken flags and priors — none of them uniform — and priors and variances over many decades.

  P  placement    bit for bit against the oracle through LINEARISE, four sweeps and six weakenings, the upload as host arrays, device
                  tensors and views 4 bytes into a buffer; the weakened priors also against float64
  W  wide         the same program on the wide profile: bit for bit, the counters of gbp_eval, the beliefs against the float64 sum of
                  the priors and messages the engine itself holds, the hoisted means against float64 solves
  H  health       n_nonpd and n_nonfinite of gbp_eval, gbp_iterate_eval_each and gbp_ba_loop exactly against float64 on the engine's
                  own beliefs, on every graph and path; their sums against the oracle's of the same summation order within a computed
                  float32 tolerance, and, on states without shallow factors, against ref64.metric_terms
  R  relinearise  six relinearising sweeps bit for bit, n_relin and n_robust equal
  N  non-finite   one iteration that leaves non-finite beliefs: no error, no finite belief where the oracle's is not, n_nonfinite
                  against float64; the next upload computes as if nothing had happened

The graphs, seeds, ranges, bounds and measures, and the conditions all this rests on (asserted on the CPU oracle), are those of
tests/wide_state.py and tests/test_wide_state_cpu.py; profiles/wide_state.md has the figures.

A NOTE ON P.  WeakenPriorVertex scales a prior while its flag is 1 .. 5 and counts the flag down; a flag of 6 or 7 is never touched.
So after k weakenings a prior is the upload x scaling^n with n = min(flag, k) for flags up to 5 and n = 0 above (wide_state.
weakenings_applied) — not scaling^min(flag, k, 5) for every flag: the oracle, the reference's vertex and the kernels agree on this."""
import numpy as np
import pytest

from tests import wide_state as ws
from tests.test_exact_inference import EXACT_PATHS, _assert_state_equal, _engine, _gpu_path, _oracle, _Shards, rounded_trig  # noqa: F401
from tests.test_wide_state_cpu import (H_BOUND, H_ORDERS, assert_wide_bounds, assert_wide_conditions, metric_case, run_counters, run_metric,
                                       run_wide)

pytestmark = pytest.mark.gpu

PATHS = EXACT_PATHS + ["library_barriers", "tile_perm", "graph_unroll_2"]
GRAPHS = ws.GRAPHS
FORMS = ("host", "device", "offset")


def _path(path, bal, K, **kw):
    """_gpu_path of tests/test_exact_inference.py and three more: the persistent kernel with counter barriers, a tile permutation
    (without placed rows) forced through the layout options, and bursts of two replayed from a captured graph"""
    from gbp_poplar_amd import _lib, hostlib
    if path == "library_barriers":
        eng = _gpu_path("library_choice", bal, K, **kw)
        eng.persist_flow(0)
        return eng
    if path == "tile_perm":
        lib = _lib.load(hooks=True)
        for classes in (8, 2):      # (the product's eight landmark classes leave the four tiles of the smallest graph in place; two do not)
            opt = hostlib.layout_options(tile_min_tiles=1, row_placement=0, classes=classes)
            lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], options=opt)
            if not np.array_equal(lay["tile_perm"], np.arange(lay["n_tiles"])):
                break
        assert lay["tile_perm"].size == lay["n_tiles"] and lay["row_slot"].size == 0
        assert not np.array_equal(lay["tile_perm"], np.arange(lay["n_tiles"])), "tiles were not permuted"
        assert lib.gbp_debug_layout_options(opt) == 0
        try:
            eng = _engine(bal, K, **kw)
        finally:
            lib.gbp_debug_layout_options(None)
        assert eng.graph_state() != 2                       # permuted tiles never run in the persistent kernel
        return eng
    if path == "graph_unroll_2":
        return _engine(bal, K, persistent=-1, graph_unroll=2, **kw)
    return _gpu_path(path, bal, K, **kw)


def _sharded(x):
    return isinstance(x, _Shards)


def _oracle_for(oracle_mod, x, bal, K, **kw):
    return _oracle(oracle_mod, bal, K, bounds=x.bounds if _sharded(x) else None, **kw)


def _upload(x, state, form):
    """the upload as numpy arrays, torch tensors on the GPU, or views 4 bytes into larger buffers (fuzz_support.DeviceForms)"""
    from tests.fuzz_support import DeviceForms
    if form == "host":
        x.upload(state)
    else:
        DeviceForms(x, form).upload(state)


class _WithMu:
    """a shard group with the mu() of an engine: every shard's own factors put together"""

    def __init__(self, group):
        self.__dict__["g"] = group

    def __getattr__(self, name):
        return getattr(self.g, name)

    def mu(self):
        E = self.g.E
        out = np.zeros((E, 9), np.float32)
        for r, sh in enumerate(self.g.shards):
            own = self.g._own(r)[2]
            out[own] = sh.e.mu()[0].reshape(E, 9)[own]
        return out.ravel(), None


def _equal(eng, orc, what):
    """beliefs, both message sets, damping state, robust flags, potentials and priors, bit for bit"""
    _assert_state_equal(eng, orc)
    assert np.array_equal(eng.read()["robust_flag"], orc.read()["robust_flag"]), what
    for a, b in zip(eng.factor_potentials(), orc.factor_potentials()):
        assert np.array_equal(a, b, equal_nan=True), what
    pe, po = eng.read_priors(), orc.read_priors()
    for k in po:
        assert np.array_equal(pe[k], po[k], equal_nan=True), (what, k)


def _counters_equal(eng, orc, what, keys=("n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd")):
    g, o = eng.eval(), orc.eval()
    for k in keys:
        assert g[k] == o[k], (what, k, g[k], o[k])


# ---- P ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_placement_bit_for_bit(name, path, oracle_mod, rounded_trig):
    bal, state, K = ws.placement_case(name)
    eng = _path(path, bal, K)
    orc = _oracle_for(oracle_mod, eng, bal, K)
    first = (GRAPHS.index(name) + PATHS.index(path)) % 3      # every form leads on every path and on every graph but one
    forms = FORMS[first:] + FORMS[:first]
    if _sharded(eng):
        forms = ("host",)                                   # (a landmark-sharded ctx takes host arrays only: include/gbp_mi355x.h)
    _upload(eng, state, forms[0])
    orc.upload(state)

    def do(verb, *a):
        getattr(eng, verb)(*a)
        getattr(orc, verb)(*a)

    def check(stage, k):
        _equal(eng, orc, (stage, forms[0]))
        if stage.startswith("weakening"):
            got, want = eng.read_priors(), ws.expected_priors(state, bal, k)
            for t in want:
                assert ws.ulps_off(got[t], want[t]) <= 2.0, (stage, t, ws.ulps_off(got[t], want[t]))

    ws.program(do, check)
    if path == "graph_unroll_2":
        assert eng.graph_state() == 1                       # the burst of two was a replay
    for form in forms[1:]:       # the other two forms of the same upload: everything starts again (gbp_upload clears the messages, the oracle's does not: a new one)
        _upload(eng, state, form)
        orc = _oracle_for(oracle_mod, eng, bal, K)
        orc.upload(state)
        do("linearise")
        do("weaken_priors")                                 # the scalings and flags of this form, read_priors compared in _equal
        do("iterate", 2)
        _equal(eng, orc, form)


# ---- W ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_wide_state_bit_for_bit_and_against_float64(name, path, oracle_mod, rounded_trig):
    bal, state, K = ws.wide_case(name)
    eng = _path(path, bal, K)
    orc = _oracle_for(oracle_mod, eng, bal, K)

    class Both:
        """the verbs on engine and oracle, everything that is read from the engine"""

        def __getattr__(self, what):
            if what in ("upload", "linearise", "iterate", "weaken_priors"):
                def both(*a):
                    getattr(eng, what)(*a)
                    getattr(orc, what)(*a)
                return both
            return getattr(_WithMu(eng) if _sharded(eng) else eng, what)

    def lockstep(stage):
        _equal(eng, orc, stage)
        _counters_equal(eng, orc, stage)

    rec = run_wide(Both(), bal, state, K, "%s %s" % (path, name), after=lockstep)
    assert_wide_conditions(rec, (path, name))
    assert_wide_bounds(rec, (path, name))


# ---- H ------------------------------------------------------------------------------------------------------------------------------------
def _world(path):
    return int(path[-1]) if path.startswith("shards_") else 1


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_health_counters_on_every_graph_and_sums_against_the_oracle(name, path, oracle_mod, rounded_trig):
    """every graph, every path, through gbp_eval, gbp_iterate_eval_each and gbp_ba_loop (a shard group: gbp_eval on every shard), on
    the wide state as W uploads it: the counters exactly against float64 on the engine's own beliefs, the beliefs bit for bit and the
    sums within wide_state.sum_tolerance of an oracle in the same summation order making the same calls"""
    bal, state, K = ws.wide_case(name)
    eng = _path(path, bal, K)
    run_counters(eng, not _sharded(eng), bal, state, K, "%s %s" % (path, name), shadow=_oracle_for(oracle_mod, eng, bal, K))


# the sums against float64 need a state without shallow factors (wide_state.metric_state): the (graph, summation order) pairs of
# wide_state.METRIC_CASES, on every path of that order
H_FLOAT64 = [(g, p) for g in GRAPHS for p in PATHS if (g, _world(p)) in H_ORDERS]


def test_leg_h_against_float64_runs_on_every_graph_and_path():
    assert sorted(H_FLOAT64) == sorted((g, p) for g in GRAPHS for p in PATHS)


@pytest.mark.parametrize("name, path", H_FLOAT64)
def test_health_counters_and_metric_against_float64(name, path, oracle_mod, rounded_trig):
    """a shard group has no loop calls of its own here: its sweeps are followed by gbp_eval on every shard, the records added.  The
    state, seed and bound are those of the path's summation order (wide_state.METRIC_CASES, H_ORACLE of tests/test_wide_state_cpu.py);
    every graph has a case for every order."""
    bal, state, K, _ = metric_case(oracle_mod, name, _world(path))
    eng = _path(path, bal, K)
    worst = run_metric(eng, not _sharded(eng), bal, state, K, "%s %s" % (path, name))
    for k, bound in H_BOUND[name][_world(path)].items():
        assert worst[k] <= bound, (path, name, k, worst[k], bound)


# ---- R ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_relinearising_sweeps_bit_for_bit(name, path, oracle_mod, rounded_trig):
    bal, state, K = ws.relin_case(name)
    eng = _path(path, bal, K, **ws.RELIN_PARAMS)
    orc = _oracle_for(oracle_mod, eng, bal, K, **ws.RELIN_PARAMS)
    for x in (eng, orc):
        x.upload(state)
        x.linearise()
    done = 0
    for n in (1, 1, 2, 2):
        eng.iterate(n)
        orc.iterate(n)
        done += n
        _equal(eng, orc, done)
        _counters_equal(eng, orc, done, keys=("n_active", "n_relin", "n_robust"))
    assert done == ws.RELIN_SWEEPS


# ---- N ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_nonfinite_beliefs_are_reported_and_leave_nothing_behind(name, path, oracle_mod, rounded_trig):
    bal, state, K = ws.nonfinite_case(name)
    eng = _path(path, bal, K)
    orc = _oracle_for(oracle_mod, eng, bal, K)
    for x in (eng, orc):                                     # (an engine call that does not return GBP_OK raises)
        x.upload(state)
        x.linearise()
        x.iterate(1)
    g, o = eng.read(), orc.read()
    bad_g, bad_o = ws.nonfinite_variables(g), ws.nonfinite_variables(o)
    assert bad_o.any() and not np.any(bad_o & ~bad_g), (int(bad_o.sum()), int(bad_g.sum()))      # one way only: gbp_device_math.hpp
    ev = eng.eval()
    assert ev["n_nonfinite"] == ws.health(g)["n_nonfinite"] > 0, (ev["n_nonfinite"], ws.health(g)["n_nonfinite"])
    _, placement, _ = ws.placement_case(name)
    orc = _oracle_for(oracle_mod, eng, bal, K)               # (the oracle's upload keeps its messages, gbp_upload must not: a new oracle)
    for x in (eng, orc):
        x.upload(placement)
        x.linearise()
        x.iterate(1)
    _equal(eng, orc, "after the non-finite run")
    _counters_equal(eng, orc, "after the non-finite run", keys=("n_active", "n_relin", "n_robust", "n_nonpd"))
