"""k_sweep requests the operands of a relinearisation — FST_VAR, the camera's hoisted mean, its CAM_LIN record — ahead of the dmu test,
as LDS-DMA into a wave-private area, when the count in the packed word says that a lane of the wave may relinearise
(kIssueEarlyRelin, gbp_kernels.h).  Only WHEN the loads are issued changes, so every case compares the whole state with the oracle in
the device's conventions, bit for bit: the beliefs, both message sets, damping, damping_count, robust_flag and the potentials.  All on
{"persistent": -1}: the two-kernel path is the code that changed.
  (1) per-factor counts: in one sweep some lanes of a wave pass the count condition and others do not; over the sweeps a lane passes it
      and fails dmu (operands requested, never read), a lane relinearises, a wave requests nothing
  (2) a tile whose four rows are four cameras (the camera records differ by row), with inactive and pad lanes in it
  (3) the instantiation that skips all-pad segments (above 2 048 tiles of many small cameras)
  (4) the instantiation the metric rides in: iterate_eval_each through relinearising sweeps = {iterate(1); eval()}
  (5) both issue orders the test-hooks library holds (gbp_debug_force_sweep_policy + 8: requests behind the dmu test) give the same arrays
"""
import numpy as np
import pytest

from tests.conftest import small_synth
from tests.test_gpu_parity import _assert_state_equal, _sync_potentials

pytestmark = pytest.mark.gpu

BOUND = 10 - 8          # min_linear_iters - num_undamped_iters of GbpParams.defaults(): relin needs count + 1 > BOUND
RESET = -8              # the count a relinearising factor leaves: -num_undamped_iters
NOPAD = 0xFFFFFFFF
LATE = (0, 8)           # + gbp_debug_force_sweep_policy's argument: 0 = the product's issue order, 8 = requests behind the dmu test


@pytest.fixture
def rounded_trig(oracle_mod):
    """the oracle's sin / cos correctly rounded, as the kernels compute them: relinearised potentials are then equal bit for bit"""
    oracle_mod.set_trig_mode(1)
    yield
    oracle_mod.set_trig_mode(0)


def _both(eng, orc, verb, *a):
    getattr(eng, verb)(*a)
    getattr(orc, verb)(*a)


def _tiles(bal):
    """per tile (one wave of the sweep): the file indices of its factors, and the camera of each of its rows that holds one"""
    from gbp_poplar_amd import hostlib
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    pe = np.asarray(lay["pos_edge"]).reshape(-1, 64)
    cam = np.asarray(bal["cam_id"])
    edges = [t[t != NOPAD].astype(np.int64) for t in pe]
    rows = [[int(cam[r[r != NOPAD][0]]) for r in t.reshape(4, 16) if np.any(r != NOPAD)] for t in pe]
    return edges, rows, pe


def _engines(bal, oracle_mod, state_changes, **params):
    """engine (test-hooks library, two-kernel path) and oracle with the same parameters, uploaded, linearised, potentials in step"""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    state = dict(state, **state_changes)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True,
                    params=_cabi.GbpParams.defaults(persistent=-1, **params))
    orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**params))
    orc.set_sum_order(1)
    _both(eng, orc, "upload", state)
    _both(eng, orc, "linearise")
    _sync_potentials(eng, orc)
    assert eng.graph_state() != 2, "the two-kernel path was asked for"
    return eng, orc


def _assert_all_equal(eng, orc):
    _assert_state_equal(eng, orc)      # beliefs, both message sets, damping, damping_count
    assert np.array_equal(eng.read()["robust_flag"], orc.read()["robust_flag"])
    (ge, gl), (oe, ol) = eng.factor_potentials(), orc.factor_potentials()
    assert np.array_equal(ge, oe) and np.array_equal(gl, ol)


def _mixed_counts(bal):
    """tile 0: every other factor beyond the bound, the others far below it; tile 1: all far below (for the whole test); the rest beyond"""
    edges, rows, _ = _tiles(bal)
    cnt = np.full(len(bal["cam_id"]), 5, np.int32)
    cnt[edges[0][1::2]] = -15
    cnt[edges[1]] = -40
    return cnt, edges, rows


def _sweep_and_classify(eng, orc, edges, n_sweeps, seen, active=None):
    """n_sweeps single sweeps, all arrays compared behind each; seen: which situations occurred, read off damping_count"""
    for _ in range(n_sweeps):
        before = orc.read()["damping_count"].copy()
        _both(eng, orc, "iterate", 1)
        _assert_all_equal(eng, orc)
        after = orc.read()["damping_count"]
        live = np.ones(before.size, bool) if active is None else active != 0
        passes = live & (before + 1 > BOUND)
        relin = passes & (after == RESET)
        unused = passes & (after == before + 1)          # the count condition held, dmu did not: requested and not read
        assert np.array_equal(relin | unused, passes)
        seen["relin"] |= bool(relin.any())
        seen["unused"] |= bool(unused.any())
        for e in edges:
            if e.size == 0:
                continue
            seen["clear_wave"] |= not passes[e].any()
            seen["mixed_wave"] |= bool(passes[e].any() and not passes[e].all())
            seen["relin_beside_unused"] |= bool(relin[e].any() and unused[e].any())
    return seen


def _seen():
    return dict.fromkeys(("relin", "unused", "clear_wave", "mixed_wave", "relin_beside_unused"), False)


def test_counts_that_differ_inside_a_wave(oracle_mod, rounded_trig):
    """(1)"""
    bal = small_synth(n_cams=9, n_lmks=40, obs=3)
    cnt, edges, _ = _mixed_counts(bal)
    eng, orc = _engines(bal, oracle_mod, {"damping_count": cnt})
    seen = _sweep_and_classify(eng, orc, edges, 8, _seen())
    assert seen["unused"] and seen["relin"] and seen["clear_wave"] and seen["mixed_wave"], seen


def test_four_cameras_in_a_tile_with_inactive_and_pad_lanes(oracle_mod, rounded_trig):
    """(2) cameras of fewer than 16 factors: a row each, so the lanes of tile 0 read four different camera records; every third factor
    of the graph sleeps"""
    bal = small_synth(n_cams=9, n_lmks=40, obs=3)
    cnt, edges, rows = _mixed_counts(bal)
    _, _, pe = _tiles(bal)
    assert len(rows[0]) == 4 and len(set(rows[0])) == 4, rows[0]
    assert np.any(pe[0] == NOPAD), "tile 0 holds pad lanes"
    active = np.ones(cnt.size, np.uint32)
    active[::3] = 0
    assert 0 < np.sum(active[edges[0]] == 0) < edges[0].size
    cnt[edges[0]] = 5                                   # the whole tile beyond the bound, the sleepers too: they must not move
    eng, orc = _engines(bal, oracle_mod, {"damping_count": cnt, "active_flag": active})
    seen = _sweep_and_classify(eng, orc, edges, 8, _seen(), active)
    assert seen["unused"] and seen["relin"], seen
    got = eng.read()["damping_count"]
    assert np.array_equal(got[active == 0], cnt[active == 0])
    assert np.any(got[edges[0]] < 5), "a factor of tile 0 relinearised"


def test_segment_skipping_instantiation(oracle_mod, rounded_trig):
    """(3) the graph of case (f) of tests/test_cmsg_compact.py.  Every count test passes its dmu test here (the threshold is raised, in
    the engine and in the oracle), so the lanes beyond the bound relinearise in the first sweep and the others as they reach it."""
    from gbp_poplar_amd import hostlib
    bal = hostlib.synth_generate(2304, 14000, 10, 7)
    rng = np.random.default_rng(11)
    cnt = rng.choice(np.array([-3, 0, 1, 2, 5], np.int32), size=len(bal["cam_id"]))
    eng, orc = _engines(bal, oracle_mod, {"damping_count": cnt}, dmu_threshold=1e30)
    assert eng.sweep_variant() == (0, True)
    n_relin = 0
    for _ in range(3):
        before = orc.read()["damping_count"].copy()
        _both(eng, orc, "iterate", 1)
        _assert_all_equal(eng, orc)
        n_relin += int(np.sum((before + 1 > BOUND) & (orc.read()["damping_count"] == RESET)))
    assert n_relin > 1000


def test_metric_riding_through_relinearising_sweeps(oracle_mod, rounded_trig):
    """(4) k_sweep<EV>: a burst with the metric behind every iteration against single sweeps each followed by gbp_eval"""
    bal = small_synth(n_cams=9, n_lmks=40, obs=3)
    cnt, edges, _ = _mixed_counts(bal)
    eng, orc = _engines(bal, oracle_mod, {"damping_count": cnt})
    ref, _unused = _engines(bal, oracle_mod, {"damping_count": cnt})
    burst = eng.iterate_eval_each(8)
    singles = []
    for _ in range(8):
        ref.iterate(1)
        singles.append(ref.eval())
    orc.iterate(8)
    assert np.any(orc.read()["damping_count"] < np.minimum(cnt, 0)), "no factor relinearised in the burst"
    assert len(burst) == len(singles)
    for b, s in zip(burst, singles):
        assert b == s, (b, s)
    _assert_all_equal(eng, orc)
    _assert_all_equal(ref, orc)


def test_every_issue_order_gives_the_same_arrays(oracle_mod, rounded_trig):
    """(5) gbp_debug_force_sweep_policy(policy + 8): case (1) with the requests behind the dmu test (the sweep as it was) and ahead of it
    (what the product runs), each equal to the oracle and to each other"""
    from gbp_poplar_amd import _lib
    lib = _lib.load(hooks=True)
    bal = small_synth(n_cams=9, n_lmks=40, obs=3)
    cnt, edges, _ = _mixed_counts(bal)
    results = {}
    for late in LATE:
        policy = None
        if late:
            policy = results[0][0]                   # the policy the shape chose, + 8
            assert lib.gbp_debug_force_sweep_policy(policy + late) == 0
        try:
            eng, orc = _engines(bal, oracle_mod, {"damping_count": cnt})
        finally:
            lib.gbp_debug_force_sweep_policy(-1)
        pol, seg = eng.sweep_variant()
        assert not seg and pol in (0, 1) and (policy is None or pol == policy)
        seen = _sweep_and_classify(eng, orc, edges, 8, _seen())
        assert seen["unused"] and seen["relin"] and seen["clear_wave"], seen
        st, msg, pot = eng.read(), eng.messages(), eng.factor_potentials()
        results[late] = (pol, [st[k] for k in sorted(st)] + [msg[k] for k in sorted(msg)] + list(pot))
    for late in LATE[1:]:
        for a, b in zip(results[late][1], results[0][1]):
            assert np.array_equal(a, b, equal_nan=True), late
