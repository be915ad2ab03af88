"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on identical inputs.

Tolerances (SURVEY 8c / BASELINE.json north_star "within 1e-4 relative"):
  * stages without transcendentals, identical inputs, oracle in the device's summation order:
    BIT-EXACT (np.array_equal);
  * same, oracle in slot order (reference-equivalent order): <= 1e-6 per-variable relative;
  * relinearisation (sin/cos of the device maths library vs glibc): <= 1e-5 relative;
  * <= 3 sweeps from identical state: <= 1e-4; synthetic end-to-end RMSE: <= 1e-4 relative.
"""
import numpy as np
import pytest

from tests.conftest import per_var_rel, rel_err, seq_path, small_synth

pytestmark = pytest.mark.gpu


def _setup(bal, oracle_mod, slam=False, sum_order=1, per_factor_mu=0, hooks=True, **engine_params):
    """hooks=True: the engine runs libgbp_mi355x_test.so (the product sources + the gbp_debug_* hooks), so that
    messages, potentials and mu can be compared; hooks=False: the product library itself (whole-run tests)."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=slam)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                    params=_cabi.GbpParams.defaults(per_factor_mu=per_factor_mu, **engine_params), hooks=hooks)
    orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    orc.set_sum_order(sum_order)
    eng.upload(state)
    orc.upload(state)
    return eng, orc, opts, state, extra


def _golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name))


def _example(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name + ".py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bal(name):
    from gbp_poplar_amd import hostlib
    return hostlib.bal_read(seq_path(name))


def _sync_potentials(eng, orc):
    eta, lam = orc.factor_potentials()
    eng.set_factor_potentials(eta, lam)


def _assert_state_equal(eng, orc, exact=True, tol=0.0):
    g, o = eng.read(), orc.read()
    if not eng.hooks:      # product library: beliefs and per-factor scalars only (messages need the test hooks)
        for k in ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count",
                  "robust_flag"):
            assert np.array_equal(g[k], o[k], equal_nan=True) if exact else per_var_rel(g[k], o[k], 1) <= tol, k
        return
    gm, om = eng.messages(), orc.messages()
    mask = np.tile(np.tril(np.ones((6, 6), bool)).ravel(), eng.E)  # cam message Lambda: lower triangle is stored
    pairs = [("cam_beliefs_eta", g["cam_beliefs_eta"], o["cam_beliefs_eta"], 6),
             ("cam_beliefs_lambda", g["cam_beliefs_lambda"], o["cam_beliefs_lambda"], 36),
             ("lmk_beliefs_eta", g["lmk_beliefs_eta"], o["lmk_beliefs_eta"], 3),
             ("lmk_beliefs_lambda", g["lmk_beliefs_lambda"], o["lmk_beliefs_lambda"], 9),
             ("msg_cam_eta", gm["cam_eta"], om["cam_eta"], 6),
             ("msg_cam_lambda", gm["cam_lambda"][mask], om["cam_lambda"][mask], 21),
             ("msg_lmk_eta", gm["lmk_eta"], om["lmk_eta"], 3),
             ("msg_lmk_lambda", gm["lmk_lambda"], om["lmk_lambda"], 9)]
    for name, a, b, w in pairs:
        if exact:
            # equal_nan: a variable without any factor has a zero prior (dataio.cpp:76-95) whose weakening scale
            # is exp(-log(0)/5) = inf (ba.cpp:564) => NaN prior/belief in the reference, the oracle and here alike;
            # no factor ever reads it
            assert np.array_equal(a, b, equal_nan=True), "%s not bit-exact: per-var rel %.3e" % (name, per_var_rel(a, b, w))
        else:
            assert per_var_rel(a, b, w) <= tol, "%s: %.3e > %.1e" % (name, per_var_rel(a, b, w), tol)
    assert np.array_equal(g["damping"], o["damping"])
    assert np.array_equal(g["damping_count"], o["damping_count"])


@pytest.mark.parametrize("name", ["fr2robot2", "fr1xyz"])
def test_linearise_parity(name, oracle_mod):
    eng, orc, *_ = _setup(_bal(name), oracle_mod)
    eng.linearise()
    orc.linearise()
    g, o = eng.read(), orc.read()
    for k in ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda"):
        assert np.array_equal(g[k], o[k]), k          # beliefs = priors, no arithmetic beyond sums with zeros
    assert np.array_equal(g["robust_flag"], o["robust_flag"])
    ge, gl = eng.factor_potentials()
    oe, ol = orc.factor_potentials()
    assert per_var_rel(ge, oe, 9) <= 1e-5
    assert per_var_rel(gl, ol, 81) <= 1e-5


@pytest.mark.parametrize("per_factor_mu", [0, 1])
@pytest.mark.parametrize("name", ["fr2robot2", "fr1xyz"])
def test_sweep_bit_exact_from_identical_state(name, per_factor_mu, oracle_mod):
    """Prep + messages + beliefs: three sweeps with prior weakening, bit-for-bit (no relinearisation yet),
    with the belief means hoisted per variable (default) and with the literal per-factor mu tensors."""
    eng, orc, opts, *_ = _setup(_bal(name), oracle_mod, sum_order=1, per_factor_mu=per_factor_mu)
    eng.linearise()
    orc.linearise()
    _sync_potentials(eng, orc)
    for it in range(3):
        if (it + 1) % 2 == 0:
            eng.weaken_priors()
            orc.weaken_priors()
        eng.iterate(1)
        orc.iterate(1)
        _assert_state_equal(eng, orc, exact=True)
    gmu, gd = eng.mu()
    omu, od = orc.mu()
    assert np.array_equal(gmu, omu)
    if per_factor_mu:
        assert np.array_equal(gd, od)          # dmu is kept per factor only in the literal mode


def test_sweep_vs_slot_order_oracle(oracle_mod):
    """Same sweep against the oracle summing camera beliefs in ascending slot order."""
    eng, orc, *_ = _setup(_bal("fr1xyz"), oracle_mod, sum_order=0)
    eng.linearise()
    orc.linearise()
    _sync_potentials(eng, orc)
    eng.iterate(1)
    orc.iterate(1)
    _assert_state_equal(eng, orc, exact=False, tol=2e-6)


def _run_to_relin(eng, orc):
    eng.linearise()
    orc.linearise()
    _sync_potentials(eng, orc)
    for it in range(17):
        if ((it + 1) % 2 == 0) and it < 10:
            eng.weaken_priors()
            orc.weaken_priors()
        eng.iterate(1)
        orc.iterate(1)


@pytest.mark.parametrize("per_factor_mu", [0, 1])
def test_relinearising_sweeps_bit_exact(per_factor_mu, oracle_mod):
    """Sweeps 17..24 relinearise (count -15 -> 3).  With the oracle's trig in correctly-rounded mode
    (what the kernels compute) the whole state stays bit-for-bit equal through relinearisation."""
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, *_ = _setup(_bal("fr2robot2"), oracle_mod, sum_order=1, per_factor_mu=per_factor_mu)
        _run_to_relin(eng, orc)
        _assert_state_equal(eng, orc, exact=True)
        n_relin = 0
        for it in range(17, 25):
            eng.iterate(1)
            orc.iterate(1)
            n_relin += int(np.sum(orc.read()["damping_count"] == -8))
            ge, gl = eng.factor_potentials()
            oe, ol = orc.factor_potentials()
            assert np.array_equal(ge, oe) and np.array_equal(gl, ol), (it, per_var_rel(gl, ol, 81))
            _assert_state_equal(eng, orc, exact=True)
            assert np.array_equal(eng.read()["robust_flag"], orc.read()["robust_flag"])
        assert n_relin > 1000
    finally:
        oracle_mod.set_trig_mode(0)


def test_relinearising_sweep_vs_libm_oracle(oracle_mod):
    """The first relinearising sweep (17) from identical state against the LITERAL restatement (glibc sinf/cosf):
    SURVEY 8c's tolerances as written — relinearised potentials <= 1e-5 per factor, the state after the sweep <= 1e-4.
    (glibc's sinf/cosf differ from the correctly rounded value for ~1-2 % of arguments; one camera in ten then carries a
    1-ulp different sin or cos, which moves its factors' potentials by <= 4e-6 — measured on all three sequences,
    tests/test_oracle_trig_sensitivity.py.)"""
    eng, orc, opts, *_ = _setup(_bal("fr2robot2"), oracle_mod, sum_order=1)
    _run_to_relin(eng, orc)
    eng.iterate(1)
    orc.iterate(1)
    assert np.array_equal(eng.read()["damping_count"], orc.read()["damping_count"])
    assert int(np.sum(orc.read()["damping_count"] == -8)) > 500
    ge, gl = eng.factor_potentials()
    oe, ol = orc.factor_potentials()
    assert per_var_rel(ge, oe, 9) <= 1e-5 and per_var_rel(gl, ol, 81) <= 1e-5
    _assert_state_equal(eng, orc, exact=False, tol=1e-4)


def test_eval_matches_oracle(oracle_mod):
    eng, orc, *_ = _setup(_bal("fr2robot2"), oracle_mod)
    eng.linearise()
    orc.linearise()
    g, o = eng.eval(), orc.eval()
    assert g["n_active"] == o["n_active"] == 3551
    assert g["n_robust"] == o["n_robust"] == 3478          # 3 478 of 3 551 after LINEARISE
    assert abs(g["sum_norm"] - o["sum_norm"]) <= 1e-6 * o["sum_norm"]
    assert abs(g["sum_half_sq"] - o["sum_half_sq"]) <= 1e-6 * o["sum_half_sq"]
    # BASELINE.md known answer: initial 39.863837 px / cost 4 242 224.19
    assert abs(g["sum_norm"] / g["n_active"] - 39.863837) < 1e-4
    assert abs(g["sum_half_sq"] - 4242224.19) / 4242224.19 < 1e-6


def test_ba_trajectory_fr2robot2(oracle_mod):
    """./ba flow (LINEARISE, weaken at 1,3,5,7,9, 40 sweeps incl. relinearisations from sweep 17):
    beliefs bit-for-bit against the oracle (correctly-rounded trig, device summation order), metric <=1e-6."""
    from gbp_poplar_amd import driver
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, _ = _setup(_bal("fr2robot2"), oracle_mod, sum_order=1, hooks=False)
        tg = driver.run_ba(eng, state, opts, n_iters=40)
        to = driver.run_ba(orc, state, opts, n_iters=40)
    finally:
        oracle_mod.set_trig_mode(0)
    for (i, mg, cg, rg, bg), (_, mo, co, ro, bo) in zip(tg, to):
        assert abs(mg - mo) <= 1e-5 * mo and abs(cg - co) <= 1e-5 * co, (i, mg, mo)   # metric trig differs (device vs glibc)
        assert rg == ro and bg == bo, (i, rg, ro, bg, bo)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    # BASELINE.md reference-run known answers (iter: mean reproj / cost)
    known = {-1: (39.863837, 4242224.19), 0: (28.488358, 2182828.51), 1: (17.600413, 879065.88),
             2: (16.256836, 751254.21)}
    for i, m, c, *_ in tg:
        if i in known:
            assert abs(m - known[i][0]) <= 2e-6 * known[i][0] and abs(c - known[i][1]) <= 2e-6 * known[i][1], (i, m, c)


def test_ba_trajectory_vs_libm_oracle(oracle_mod):
    """Same flow against the literal (glibc trig, slot-order sums) oracle and against the committed golden trajectory
    of the reference-math build: 1e-4 (north_star tolerance) for the first sweeps, 1e-3 up to the first
    relinearisation (sweep 17; ulp differences amplify ~x3 per sweep).  Beyond it the relinearisation
    DECISION (dmu < 3e-3, gbp_codelets.cpp:280) flips for individual factors and any two arithmetic variants separate;
    the end-to-end statement for this sequence is the mean over the last 50 of 1500 iterations
    (test_other_sequences_1500_sweeps_bit_exact)."""
    from gbp_poplar_amd import driver
    eng, orc, opts, state, _ = _setup(_bal("fr2robot2"), oracle_mod, sum_order=0)
    tg = driver.run_ba(eng, state, opts, n_iters=17)
    to = driver.run_ba(orc, state, opts, n_iters=17)
    gold = _golden("trajectories.npz")["ba_fr2robot2"]
    for (i, mg, cg, *_), (_, mo, co, *_2) in zip(tg, to):
        tol = 1e-4 if i < 6 else 1e-3
        assert abs(mg - mo) <= tol * mo and abs(cg - co) <= 2 * tol * co, (i, mg, mo)
        if i >= 0:
            assert gold[i, 0] == i and abs(mg - gold[i, 1]) <= tol * gold[i, 1], (i, mg, gold[i, 1])


def test_synthetic_end_to_end(oracle_mod):
    """Synthetic graph (well conditioned): RMSE after 60 iterations within 1e-4 of the literal oracle,
    beliefs bit-for-bit against the oracle in correctly-rounded-trig / device-order mode."""
    from gbp_poplar_amd import driver
    bal = small_synth(n_cams=20, n_lmks=800, obs=8, seed=11)
    eng, orc, opts, state, _ = _setup(bal, oracle_mod, sum_order=0, hooks=False)
    tg = driver.run_ba(eng, state, opts, n_iters=60, eval_every=60)
    to = driver.run_ba(orc, state, opts, n_iters=60, eval_every=60)
    rg = np.sqrt(2 * tg[-1][2] / bal["n_edges"])
    ro = np.sqrt(2 * to[-1][2] / bal["n_edges"])
    assert abs(rg - ro) <= 1e-4 * ro, (rg, ro)
    assert tg[-1][1] < 0.5 * tg[0][1]                       # it actually converged
    g, o = eng.read(), orc.read()
    assert per_var_rel(g["cam_beliefs_eta"], o["cam_beliefs_eta"], 6) <= 1e-2
    assert per_var_rel(g["lmk_beliefs_eta"], o["lmk_beliefs_eta"], 3) <= 1e-2
    oracle_mod.set_trig_mode(1)
    try:
        orc2 = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], driver.k_matrix(bal))
        orc2.set_sum_order(1)
        driver.run_ba(orc2, state, opts, n_iters=60, eval_every=0)
    finally:
        oracle_mod.set_trig_mode(0)
    o2 = orc2.read()
    for k in g:
        assert np.array_equal(g[k], o2[k]), k


def test_slam_flow_bit_exact(oracle_mod):
    """./slam flow (keyframe insertion every 25 sweeps, NEW_KEYFRAME / READ_PRIORS, activation of factors,
    relinearisations after 18 active sweeps) against the oracle, bit for bit, in both mu modes."""
    from gbp_poplar_amd import driver, hostlib
    bal = _bal("fr2robot2")
    oracle_mod.set_trig_mode(1)
    try:
        reads = []
        for per_factor_mu in (0, 1):
            eng, orc, opts, state, extra = _setup(bal, oracle_mod, slam=True, sum_order=1, per_factor_mu=per_factor_mu, hooks=False)
            tg = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=25, max_iters=110, eval_every=10)
            if per_factor_mu == 0:
                to = driver.run_slam(orc, hostlib, bal, state, extra, opts, iters_between_kfs=25, max_iters=110, eval_every=10)
                ro = orc.read()
            reads.append(eng.read())
            for (i, mg, cg, rg, bg), (_, mo, co, ro_, bo) in zip(tg, to):
                assert abs(mg - mo) <= 1e-5 * mo and rg == ro_ and bg == bo, (i, mg, mo)
        for k in ro:
            assert np.array_equal(reads[0][k], ro[k]) and np.array_equal(reads[1][k], ro[k]), k
        assert np.sum(ro["damping_count"] == -8) + np.sum(ro["robust_flag"]) > 0
    finally:
        oracle_mod.set_trig_mode(0)


def test_nonzero_oldmu_needs_per_factor_mode():
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = small_synth(n_cams=5, n_lmks=30, obs=3, seed=2)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    state = dict(state)
    state["mu"] = np.full(9 * bal["n_edges"], 0.25, np.float32)
    state["oldmu"] = state["mu"].copy()
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
    with pytest.raises(GbpError, match="per_factor_mu"):
        eng.upload(state)
    eng2 = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                     params=_cabi.GbpParams.defaults(per_factor_mu=1), hooks=True)
    eng2.upload(state)
    eng2.linearise()
    eng2.iterate(1)
    assert np.all(eng2.mu()[1] > 0)       # dmu measured against the uploaded oldmu


def test_inactive_factors_and_ragged_degrees(oracle_mod):
    """SLAM-style activation: inactive factors send zero messages; cameras with 1..17 factors exercise row padding."""
    bal = small_synth(n_cams=9, n_lmks=40, obs=3, seed=3)
    eng, orc, opts, state, extra = _setup(bal, oracle_mod, slam=True, sum_order=1)
    eng.linearise()
    orc.linearise()
    _sync_potentials(eng, orc)
    for _ in range(2):
        eng.iterate(1)
        orc.iterate(1)
    _assert_state_equal(eng, orc, exact=True)
    gm = eng.messages()
    inactive = state["active_flag"] == 0
    assert inactive.any() and not gm["cam_eta"].reshape(-1, 6)[inactive].any()


def test_graph_replay_equals_direct_launches(oracle_mod):
    """gbp_iterate(20) (hipGraph replay, unroll 10) == 20 x gbp_iterate(1) (direct launches), bit for bit."""
    bal = _bal("fr2robot2")
    a, _, _, state, _ = _setup(bal, oracle_mod, persistent=-1)      # small graph: keep it off the persistent kernel
    b, _, _, _, _ = _setup(bal, oracle_mod, persistent=-1)
    a.linearise()
    b.linearise()
    assert a.graph_state() == 0
    a.prepare()                          # capture + instantiation + upload, no iteration executed
    assert a.graph_state() == 1 and a.timing()["iterations"] == 0
    a.iterate(20)
    for _ in range(20):
        b.iterate(1)
    assert b.graph_state() == 0          # single iterations never capture
    ra, rb = a.read(), b.read()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k


# ---- k_persist: the iteration loop inside one kernel launch (small graphs) ---------------------------------------

def _full_snapshot(eng):
    d = _gpu_snapshot(eng)
    d["mu"] = eng.mu()[0]                  # the hoisted means the last sweep used, per factor
    return d


def _ragged_bal():
    """Few factors, many landmarks (more belief waves than sweep tiles), a hub landmark of degree > 30, cameras with one row;
    with the parameters that make it relinearise early."""
    rng = np.random.default_rng(11)
    C, L, E = 9, 700, 1500
    cam_id = np.sort(rng.integers(0, C, E)).astype(np.uint32)
    lmk_id = rng.integers(0, L, E).astype(np.uint32)
    lmk_id[rng.random(E) < 0.03] = 5             # hub landmark: slots beyond the index record
    cam_id[:C] = np.arange(C)
    return _tiny_problem(list(cam_id), list(lmk_id), C, L, seed=3), dict(dmu_threshold=0.05, min_linear_iters=3, num_undamped_iters=2)


def _ragged_active(bal):
    return (np.random.default_rng(5).random(bal["n_edges"]) < 0.9).astype(np.uint32)


@pytest.mark.parametrize("flow", [1, 0], ids=["tagged_records", "barriers"])
@pytest.mark.parametrize("name", ["fr2robot2", "fr1xyz", "ragged", "all_cus"])
def test_persistent_kernel_equals_two_kernel_path(name, flow, oracle_mod):
    """gbp_iterate(n) through the persistent kernel — k_persist_flow (hand-offs through tagged records, the default for bursts
    without the metric) and k_persist<false> (sweep + device-wide barrier + beliefs + barrier) — n times in ONE launch, per-factor
    state in registers, leaves EVERY tensor — beliefs, both message sets, potentials, per-factor scalars, hoisted means —
    bit for bit as n x (k_sweep, k_beliefs) do: the ./ba flow with bursts of odd lengths, relinearisations included,
    on the two shipped small sequences and on a ragged synthetic graph (hub landmark of degree > 15, inactive factors,
    cameras with one row, waves with a belief role but no sweep tile)."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    opts = driver.Options()
    kw = {}
    if name == "ragged":
        bal, kw = _ragged_bal()
        opts.undamped_start = 2
    elif name == "all_cus":      # 64 000 factors = 250 workgroups: one per CU, no dispatch spread (the automatic choice since round 5)
        bal = hostlib.synth_generate(100, 6400, 10, 7)
    else:
        bal = _bal(name)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    if name == "ragged":
        state["active_flag"] = _ragged_active(bal)
    engs = [GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True,
                      params=_cabi.GbpParams.defaults(persistent=mode, **kw)) for mode in (0 if name == "all_cus" else 1, -1)]
    assert engs[0].graph_state() == 2 and engs[1].graph_state() != 2
    engs[0].persist_flow(flow)
    n_relin = 0
    for e in engs:
        e.upload(state)
        e.linearise()
    it = 0
    for burst in (1, 1, 2, 3, 5, 7, 2, 37, 64, 3, 100):       # ba.cpp:1001-1008: weaken priors before iterations 1,3,5,7,9
        for e in engs:
            left = burst
            i = it
            while left > 0:
                if (i + 1) % 2 == 0 and i < 10:
                    e.weaken_priors()
                k = 1
                while k < left and not ((i + k + 1) % 2 == 0 and i + k < 10):
                    k += 1
                e.iterate(k)
                i += k
                left -= k
        it += burst
        sa, sb = _full_snapshot(engs[0]), _full_snapshot(engs[1])
        for k in sa:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), (name, it, k)
        ea, eb = engs[0].eval(), engs[1].eval()
        assert ea == eb, (it, ea, eb)
        n_relin += ea["n_relin"]
    assert n_relin > 0 and engs[0].timing()["iterations"] == it


@pytest.mark.parametrize("mask,blocks,K", [(1, 256, 16), (3, 256, 16), (7, 256, 16), (5, 64, 16), (8, 256, 16), (1, 256, 4), (127, 256, 4)])
def test_tagged_records_are_never_seen_torn(mask, blocks, K):
    """VERDICT r05 item 2 / ADVICE r05: the persistent kernel's hand-offs rest on ONE property no manual promises — a 16-byte aligned
    store of one lane (buffer_store_dwordx4 sc1) is never observed torn by a wave on another XCD (buffer_load_dwordx4 sc1); a torn
    record would carry the awaited tag with a stale payload: silently wrong beliefs, invisible to the time-out.  The detector, on the
    box the suite runs on: up to 256 workgroups (one per CU) x 16 records per lane x 100 000 rounds, both halves (parities) of the
    double buffer, EVERY word of a record a function of its round, partners on other XCDs (odd masks: bid ^ mask lands on another XCD
    under round-robin placement; mask 8 = the same XCD, the control), the product's own store / load instructions
    (csrc/hooks/gbp_flow_torture.hip).  Not one record may be torn or corrupt, no wait may time out.  If this test ever fails on a device:
    gbp_params.persistent = -1 (or GBP_PERSIST=-1 for the CLIs) keeps every graph on the two-kernel path."""
    import ctypes
    from gbp_poplar_amd import _lib
    lib = _lib.load(hooks=True)
    rounds = 100000 if K == 16 else 200000
    out = (ctypes.c_uint64 * 4)()
    rc = lib.gbp_debug_flow_torture(blocks, K, rounds, mask, 0, out)
    assert rc == 0, lib.gbp_last_error(None)
    torn, corrupt, timeouts, checked = (int(x) for x in out)
    assert checked == blocks * 256 * K * rounds, (checked, blocks * 256 * K * rounds)
    assert (torn, corrupt, timeouts) == (0, 0, 0), {"torn": torn, "corrupt": corrupt, "timeouts": timeouts, "records_checked": checked}


def test_torn_record_detector_detects():
    """The control of the detector above: with one record in 64 stored tag first and payload a little later — what a tearing memory
    system would show — the same kernel must REPORT torn records (and nothing else: no corrupt record, no time-out)."""
    import ctypes
    from gbp_poplar_amd import _lib
    lib = _lib.load(hooks=True)
    out = (ctypes.c_uint64 * 4)()
    assert lib.gbp_debug_flow_torture(256, 16, 20000, 1, 1, out) == 0, lib.gbp_last_error(None)
    torn, corrupt, timeouts, checked = (int(x) for x in out)
    assert torn > 0 and corrupt == 0 and timeouts == 0 and checked == 256 * 256 * 16 * 20000, (torn, corrupt, timeouts, checked)


@pytest.mark.parametrize("name", ["fr1xyz", "fr2robot2", "all_cus"])
def test_persistent_kernel_redundant_records(name, oracle_mod):
    """The same question asked of k_persist_flow itself (test-hooks build, gbp_debug_persist_verify): every record of every hand-off of
    the default loop — beliefs, means, CAM_LIN, row sums, landmark messages, metric means — is published a second time with its payload
    complemented, and a consumer accepts a record only when both copies carry the same tag and then compares them.  A whole default
    run of the ./ba loop (gbp_ba_loop: prior weakening inside the launch, the metric after every iteration) and bursts without the
    metric: zero mismatches, and every tensor and every metric equal to the plain kernel's, bit for bit."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    opts = driver.Options()
    bal = hostlib.synth_generate(100, 6400, 10, 7) if name == "all_cus" else _bal(name)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    engs = [GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=0 if name == "all_cus" else 1))
            for _ in range(2)]
    assert all(e.graph_state() == 2 for e in engs)
    assert engs[0].persist_verify(True) == 0
    for e in engs:
        e.upload(state)
        e.linearise()
    n_iters = 150 if name == "all_cus" else 600
    evs = [e.ba_loop(n_iters, 0, int(opts.steps)) for e in engs]
    assert evs[0] == evs[1]
    it = n_iters
    for burst in (2, 5, 64, 100):
        for e in engs:
            e.ba_loop(burst, it, int(opts.steps), metrics=False)
        it += burst
    sa, sb = _full_snapshot(engs[0]), _full_snapshot(engs[1])
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (name, k)
    assert engs[0].eval() == engs[1].eval() and sum(e["n_relin"] for e in evs[0]) > 0
    assert engs[0].persist_verify(False) == 0, "a record and its redundant copy disagreed: a torn or stale 16-byte record"
    assert engs[0].graph_state() == 2 and "timed out" not in engs[0].last_error()


def test_persistent_kernel_full_run_vs_oracle(oracle_mod):
    """`./ba fr1xyz --eval_every 100` as the CLI issues it (bursts of up to 100 iterations inside k_persist), 600 sweeps
    of the chaotic sequence: every belief equal to the CPU oracle's, bit for bit."""
    from gbp_poplar_amd import driver
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, _ = _setup(_bal("fr1xyz"), oracle_mod, sum_order=1, hooks=False, persistent=1)
        assert eng.graph_state() == 2
        tg = driver.run_ba(eng, state, opts, n_iters=600, eval_every=100)
        to = driver.run_ba(orc, state, opts, n_iters=600, eval_every=100)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    assert [t[0] for t in tg] == [t[0] for t in to] and [t[3:] for t in tg] == [t[3:] for t in to]


@pytest.mark.parametrize("flow", [1, 0], ids=["tagged_records", "barriers"])
def test_iterate_eval_fused_metric_equals_separate_calls(flow, oracle_mod):
    """gbp_iterate_eval(n) — the iterations AND the metric in one launch of the persistent kernel on small graphs (what
    k_means and k_eval compute; k_persist_flow<true> or k_persist<true>) — against gbp_iterate(n) followed by gbp_eval(): metric sums, counters, health counters and
    every belief identical, single iterations (the reference's default loop) and bursts, two evaluations in flight."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    for name in ("fr2robot2", "fr1xyz"):
        bal = _bal(name)
        K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
        a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
        b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        c = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(persistent=-1))
        assert a.graph_state() == 2 and c.graph_state() != 2
        a.persist_flow(flow)
        for e in (a, b, c):
            e.upload(state)
            e.linearise()
        it = 0
        for n in [1] * 12 + [2, 1, 7, 1, 1, 30, 1]:
            for e in (a, b, c):
                i = it
                left = n
                while left > 0:          # ba.cpp:1003-1006: prior weakening before iterations 1,3,5,7,9 — as separate calls
                    if (i + 1) % 2 == 0 and i < 10:
                        e.weaken_priors()
                    k = 1
                    while k < left and not ((i + k + 1) % 2 == 0 and i + k < 10):
                        k += 1
                    last = left == k
                    if e is not b and last:      # a: fused into the k_persist launch; c: the two-call fallback behind the same entry point
                        e.iterate_eval(k)
                    else:
                        e.iterate(k)
                    i += k
                    left -= k
            it += n
            ea, eb, ec = a.eval_end(), b.eval(), c.eval_end()
            assert ea == eb == ec, (name, it, ea, eb, ec)
            ra, rb = a.read(), b.read()
            for k in ra:
                assert np.array_equal(ra[k], rb[k], equal_nan=True), (name, it, k)
        # two evaluations in flight, collected in order
        a.iterate_eval(1)
        a.iterate_eval(3)
        b.iterate(1)
        e1 = b.eval()
        b.iterate(3)
        e2 = b.eval()
        assert a.eval_end() == e1 and a.eval_end() == e2
        assert a.timing()["iterations"] == b.timing()["iterations"]


@pytest.mark.parametrize("flow", [1, 0], ids=["tagged_records", "barriers"])
def test_iterate_eval_each_equals_one_iteration_and_one_metric_at_a_time(flow, oracle_mod):
    """gbp_iterate_eval_each(n): n iterations with the metric after every one — ONE launch of the persistent kernel per burst on
    small graphs (k_persist_flow<true> or k_persist<true>), the metric of iteration k computed one iteration later — against n times {gbp_iterate(1); gbp_eval()}:
    every metric (sums, counters, health counters) and every belief identical.  Bursts of 1, a few, 129 and 600 (a launch carries
    at most 512 metrics), prior weakening between bursts, then gbp_iterate_eval and plain gbp_eval still work; c is the same
    entry point on the two-kernel path."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    for name in ("fr2robot2", "fr1xyz", "ragged"):
        opts, kw = driver.Options(), {}
        if name == "ragged":
            bal, kw = _ragged_bal()
            opts.undamped_start = 2
        else:
            bal = _bal(name)
        K, state, _ = driver.build_inputs(bal, opts, hostlib)
        if name == "ragged":
            state["active_flag"] = _ragged_active(bal)
        a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=1, **kw))
        b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
        c = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
        assert a.graph_state() == 2 and c.graph_state() != 2
        a.persist_flow(flow)
        for e in (a, b, c):
            e.upload(state)
            e.linearise()
        it = 0
        for n in (1, 1, 2, 2, 2, 2, 5, 1, 129, 0, 600 if name == "fr1xyz" else 40):
            if it in (1, 3, 5, 7, 9):
                for e in (a, b, c):
                    e.weaken_priors()
            ea = a.iterate_eval_each(n)
            ec = c.iterate_eval_each(n)
            eb = []
            for _ in range(n):
                b.iterate(1)
                eb.append(b.eval())
            assert len(ea) == n and ea == eb, (name, it, n, [i for i in range(n) if ea[i] != eb[i]][:5])
            assert ec == eb, (name, it, n)
            it += n
            ra, rb = a.read(), b.read()
            for k in ra:
                assert np.array_equal(ra[k], rb[k], equal_nan=True), (name, it, k)
        a.iterate_eval(3)
        b.iterate(3)
        assert a.eval_end() == b.eval()
        a.iterate(2)
        b.iterate(2)
        assert a.eval() == b.eval()
        assert a.timing()["iterations"] == b.timing()["iterations"]
        a.eval_begin()
        with pytest.raises(RuntimeError):
            a.iterate_eval_each(1)       # an evaluation is in flight
        a.eval_end()


@pytest.mark.parametrize("name", ["fr2robot2", "fr1xyz", "ragged"])
def test_ba_loop_equals_the_calls_it_stands_for(name, oracle_mod):
    """gbp_ba_loop(n, iter0, steps) — the body of the reference's loop, prior weakening included: ONE launch of the persistent kernel
    however many weakenings lie inside (WeakenPriorVertex applied by the kernel itself) — against the calls it stands for, one at a
    time on the two-kernel path: {gbp_weaken_priors where the loop weakens; gbp_iterate(1); gbp_eval()}.  Every metric, every tensor,
    the priors (READ_PRIORS) identical after calls that start inside, in front of and behind the weakening phase; c is the same entry
    point on the two-kernel path (its fall-back)."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    opts, kw = driver.Options(), {}
    if name == "ragged":
        bal, kw = _ragged_bal()
        opts.undamped_start = 2
    else:
        bal = _bal(name)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    if name == "ragged":
        state["active_flag"] = _ragged_active(bal)
    steps = int(opts.steps)
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=1, **kw))
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
    c = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
    assert a.graph_state() == 2 and b.graph_state() != 2
    for e in (a, b, c):
        e.upload(state)
        e.linearise()
    it = 0
    for n in (2, 1, 4, 9, 1, 0, 40, 600 if name == "fr1xyz" else 30):      # 2: one weakening inside; 4: two; 9: crosses the end of the phase; 600: two launches
        ea = a.ba_loop(n, it, steps)
        ec = c.ba_loop(n, it, steps)
        eb = []
        for i in range(it, it + n):
            if (i + 1) % 2 == 0 and i < 2 * steps:
                b.weaken_priors()
            b.iterate(1)
            eb.append(b.eval())
        assert len(ea) == n and ea == eb, (name, it, n, [i for i in range(n) if ea[i] != eb[i]][:5])
        assert ec == eb, (name, it, n)
        it += n
        sa, sb = _full_snapshot(a), _full_snapshot(b)
        for k in sa:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), (name, it, k)
        pa, pb = a.read_priors(), b.read_priors()
        for k in pa:
            assert np.array_equal(pa[k], pb[k]), (name, it, k)
    # a run that starts again (new upload: flags back to `steps`), the whole weakening phase and beyond in ONE call
    for e in (a, b):
        e.upload(state)
        e.linearise()
    ea = a.ba_loop(25, 0, steps)
    eb = []
    for i in range(25):
        if (i + 1) % 2 == 0 and i < 2 * steps:
            b.weaken_priors()
        b.iterate(1)
        eb.append(b.eval())
    assert ea == eb
    pa, pb = a.read_priors(), b.read_priors()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert a.timing()["iterations"] == b.timing()["iterations"]


@pytest.mark.parametrize("steps", [0, 3, 8])
def test_ba_loop_with_other_weakening_schedules(steps, oracle_mod):
    """--steps 0 (no weakening at all), 3 and 8 (weaken flags that start above five: WeakenPriorVertex acts on flags 1 .. 5 only): gbp_ba_loop
    with and without the metric, on the persistent path and on the two-kernel path, against the calls it stands for."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    opts = driver.Options()
    opts.steps = float(steps)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    engs = [GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True,
                      params=_cabi.GbpParams.defaults(persistent=m)) for m in (1, -1, 1, -1)]
    a, c, ap, b = engs          # a, c: with the metric (persistent / two-kernel); ap: without, persistent; b: call by call
    for e in engs:
        e.upload(state)
        e.linearise()
    it = 0
    for n in (5, 2, 14, 9):
        ea, ec = a.ba_loop(n, it, steps), c.ba_loop(n, it, steps)
        ap.ba_loop(n, it, steps, metrics=False)
        eb = []
        for i in range(it, it + n):
            if (i + 1) % 2 == 0 and i < 2 * steps:
                b.weaken_priors()
            b.iterate(1)
            eb.append(b.eval())
        assert ea == eb == ec, (steps, it, n)
        it += n
        sb, pb = _full_snapshot(b), b.read_priors()
        for e in (a, c, ap):
            se, pe = _full_snapshot(e), e.read_priors()
            for k in sb:
                assert np.array_equal(se[k], sb[k], equal_nan=True), (steps, it, k)
            for k in pb:
                assert np.array_equal(pe[k], pb[k]), (steps, it, k)


@pytest.mark.parametrize("name", ["fr2robot2", "fr1xyz", "ragged", "two_kernels_40k_factors"])
def test_ba_loop_without_the_metric_equals_the_calls_it_stands_for(name, oracle_mod):
    """gbp_ba_loop(n, iter0, steps, NULL): the passes without the metric, not blocking.  A weakening then rides in the launch of the
    persistent kernel (a) or, on the two-kernel path (c; and a graph too large for anything else), in the belief update of the
    iteration in front of it — against {gbp_weaken_priors where the loop weakens; gbp_iterate(1)} call by call (b): every tensor,
    the priors and the metric identical after calls that start inside, in front of and behind the weakening phase."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    opts, kw = driver.Options(), {}
    if name == "ragged":
        bal, kw = _ragged_bal()
        opts.undamped_start = 2
    elif name == "two_kernels_40k_factors":
        bal = hostlib.synth_generate(40, 4000, 10, 5)
    else:
        bal = _bal(name)
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    if name == "ragged":
        state["active_flag"] = _ragged_active(bal)
    steps = int(opts.steps)
    modes = (-1, -1, -1) if name == "two_kernels_40k_factors" else (1, -1, -1)
    a, b, c = [GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True,
                         params=_cabi.GbpParams.defaults(persistent=m, **kw)) for m in modes]
    for e in (a, b, c):
        e.upload(state)
        e.linearise()
    it = 0
    for n in (2, 1, 4, 9, 1, 0, 40, 25):
        a.ba_loop(n, it, steps, metrics=False)
        c.ba_loop(n, it, steps, metrics=False)
        for i in range(it, it + n):
            if (i + 1) % 2 == 0 and i < 2 * steps:
                b.weaken_priors()
            b.iterate(1)
        it += n
        sb = _full_snapshot(b)
        pb = b.read_priors()
        for e in (a, c):
            se, pe = _full_snapshot(e), e.read_priors()
            for k in sb:
                assert np.array_equal(se[k], sb[k], equal_nan=True), (name, it, k)
            for k in pb:
                assert np.array_equal(pe[k], pb[k]), (name, it, k)
        assert a.eval() == b.eval() == c.eval()
    assert a.timing()["iterations"] == b.timing()["iterations"] == c.timing()["iterations"]


@pytest.mark.parametrize("shape", ["tiles_permuted", "rows_placed", "per_factor_mu"])
def test_iterate_eval_each_rides_in_the_two_kernel_path(shape, oracle_mod):
    """gbp_iterate_eval_each on graphs that do NOT run in the persistent kernel (more than 256 workgroups, a permuted tile order, placed rows,
    per-factor means): the metric of iteration k rides in
    the sweep of iteration k + 1 (k_sweep<EV> / k_beliefs<EV>, bursts replayed from a hipGraph, one k_eval_fold per piece) —
    against n times {gbp_iterate(1); gbp_eval()} on a second engine: every metric (sums, counters, health counters) and every
    belief IDENTICAL; against the oracle: counters equal, sums within fp64 reassociation.  Shapes: a 200-camera graph whose
    sweep runs in the XCD-aware tile order; the config-5 shard shape in small (rows placed by landmark class, the camera sums
    found through row_slot); and per_factor_mu = 1, where the entry point keeps the plain loop.  Bursts of 1, 2 (the prior
    weakening rhythm), 25 (graph replays + remainder) and 130 (more than one piece of the ring would hold on a large graph)."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    kw = {}
    if shape == "rows_placed":
        bal = hostlib.synth_generate(4096, 40000, 10, 7)
    else:
        bal = hostlib.synth_generate(200, 20000, 10, 1)
        if shape == "per_factor_mu":
            kw = {"per_factor_mu": 1}
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**kw))
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**kw))
    assert a.graph_state() == 0
    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        for e in (a, b, orc):
            e.upload(state)
            e.linearise()
        it = 0
        for n in (1, 1, 2, 2, 2, 2, 0, 25, 1, 130 if shape == "tiles_permuted" else 12):
            if it in (1, 3, 5, 7, 9):
                for e in (a, b, orc):
                    e.weaken_priors()
            ea = a.iterate_eval_each(n)
            eb = []
            for _ in range(n):
                b.iterate(1)
                eb.append(b.eval())
            assert len(ea) == n and ea == eb, (shape, it, n, [(i, ea[i], eb[i]) for i in range(n) if ea[i] != eb[i]][:2])
            if it < 40:                                  # the oracle keeps pace for the first bursts
                for k in range(n):
                    orc.iterate(1)
                    eo = orc.eval()
                    for key in ("n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd"):
                        assert ea[k][key] == eo[key], (shape, it + k, key)
                    assert abs(ea[k]["sum_norm"] - eo["sum_norm"]) <= 1e-6 * eo["sum_norm"]
                    assert abs(ea[k]["sum_half_sq"] - eo["sum_half_sq"]) <= 1e-6 * eo["sum_half_sq"]
            it += n
            ra, rb = a.read(), b.read()
            for k in ra:
                assert np.array_equal(ra[k], rb[k], equal_nan=True), (shape, it, k)
        assert any(e["n_relin"] > 0 for e in ea)         # the bursts went through relinearisations
        if shape != "per_factor_mu":
            assert a.graph_state() == 1                  # the bursts of 12 and more replayed a captured graph
        a.iterate(10)                                    # the plain graph and the metric's graph live side by side
        b.iterate(10)
        assert a.eval() == b.eval()
        assert a.timing()["iterations"] == b.timing()["iterations"]
    finally:
        oracle_mod.set_trig_mode(0)


def test_persistent_kernel_is_chosen_by_size():
    """Automatic selection (gbp_params.persistent = 0): the shipped sequences run in k_persist, S1-sized graphs do not;
    a sharded ctx and per_factor_mu = 1 never do."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    for name, want in (("fr1xyz", 2), ("fr2robot2", 2)):
        bal = _bal(name)
        K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
        assert GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K).graph_state() == want
        assert GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                         params=_cabi.GbpParams.defaults(per_factor_mu=1)).graph_state() == 0
        assert GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                         shard=(0, 1, 0, bal["n_lmks"])).graph_state() == 0
    bal = small_synth(n_cams=200, n_lmks=20000, obs=10, seed=1)        # 200 000 factors: 782 workgroups
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    assert GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K).graph_state() == 0
    assert GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                     params=_cabi.GbpParams.defaults(persistent=1)).graph_state() == 0      # not co-resident: refused


# ---- committed golden fixtures (tests/golden/*.npz, produced with the REFERENCE's math layer) ----------------

def _gpu_snapshot(eng):
    r, m = eng.read(), eng.messages()
    fe, fl = eng.factor_potentials()
    d = dict(r)
    d.update({"msg_" + k: v for k, v in m.items()})
    d.update(fac_eta=fe, fac_lambda=fl)
    return d


def test_golden_tiny_state():
    """4 cams x 24 lmks: every tensor after LINEARISE and 4 sweeps.  `dev_` golden (device conventions):
    bit for bit.  `ref_` golden (reference math, libm trig, slot-order sums): 1e-5 after LINEARISE /
    1 sweep, 1e-4 up to 4 sweeps (north_star tolerance)."""
    from gbp_poplar_amd.engine import GbpEngine
    g = _golden("state_tiny.npz")
    bal = {k[4:]: g[k] for k in g.files if k.startswith("bal_")}
    state = {k[6:]: g[k] for k in g.files if k.startswith("state_")}
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], int(bal["n_cams"]), int(bal["n_lmks"]), g["K"], hooks=True)
    eng.upload(state)
    eng.linearise()
    snaps = {"lin": _gpu_snapshot(eng)}
    for it in range(4):
        if (it + 1) % 2 == 0:
            eng.weaken_priors()
        eng.iterate(1)
        snaps["it%d" % it] = _gpu_snapshot(eng)
    width = {"cam_beliefs_eta": 6, "cam_beliefs_lambda": 36, "lmk_beliefs_eta": 3, "lmk_beliefs_lambda": 9,
             "msg_cam_eta": 6, "msg_cam_lambda": 36, "msg_lmk_eta": 3, "msg_lmk_lambda": 9, "fac_eta": 9, "fac_lambda": 81}
    low = np.tile(np.tril(np.ones((6, 6), bool)).ravel(), eng.E)
    for tag, d in snaps.items():
        for k, v in d.items():
            dev, ref = g["dev_%s_%s" % (tag, k)], g["ref_%s_%s" % (tag, k)]
            if k == "msg_cam_lambda":        # only the lower triangle of a camera message is stored per factor
                v, dev, ref = v[low], dev[low], ref[low]
            assert np.array_equal(v, dev), ("dev", tag, k)
            if k in width:
                w = 21 if k == "msg_cam_lambda" else width[k]
                tol = 1e-5 if tag in ("lin", "it0") else 1e-4
                assert per_var_rel(v, ref, w) <= tol, ("ref", tag, k, per_var_rel(v, ref, w))
            else:
                assert np.array_equal(v, ref), ("ref", tag, k)


def test_golden_sequence_snapshots():
    """fr2robot2 belief snapshots at LINEARISE and sweeps 0,1,2,5 from the reference-math oracle."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    g = _golden("sequence_snapshots.npz")
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    eng.upload(state)
    eng.linearise()
    w = {"cam_beliefs_eta": 6, "cam_beliefs_lambda": 36, "lmk_beliefs_eta": 3, "lmk_beliefs_lambda": 9}
    r = eng.read()
    for k in w:
        assert np.array_equal(r[k], g["lin_" + k]), k
    for it in range(6):
        if (it + 1) % 2 == 0:
            eng.weaken_priors()
        eng.iterate(1)
        if it in (0, 1, 2, 5):
            r = eng.read()
            for k in w:
                err = per_var_rel(r[k], g["it%d_%s" % (it, k)], w[k])
                assert err <= (1e-4 if it <= 2 else 1e-3), (it, k, err)
        ev = eng.eval()
        m = ev["sum_norm"] / ev["n_active"]
        assert abs(m - g["traj_fr2robot2"][it + 1, 1]) <= 1e-4 * m, (it, m)


@pytest.mark.parametrize("per_factor_mu", [0, 1])
def test_golden_vertex_vectors(per_factor_mu):
    """SURVEY 8c pin 2: per-factor vertex outputs (factor potentials, the four messages, mu, damping state,
    robust flag) of 64 sampled fr2robot2 factors at sweeps {0, 1, 17, 18, 100}.
    `dev_` golden: bit for bit at every sweep, through 101 sweeps with ~40 % of factors relinearising at 17/18.
    `ref_` golden (reference math, libm trig, slot-order sums): 1e-4 at sweeps 0/1 (north_star tolerance), 1e-3
    at sweep 17 on the factors whose relinearisation decision agrees, as max |diff| / max |ref| over the sample
    (a single landmark message is a cancelling difference, so its own norm is not a stable yardstick: the two
    ORACLE conventions already differ by 1e-4 of it at sweep 1); later sweeps are chaotic and only
    pinned by `dev_`."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    g = _golden("vertex_vectors.npz")
    ids, sweeps = g["ids"], [int(s) for s in g["sweeps"]]
    bal = _bal("fr2robot2")
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                    params=_cabi.GbpParams.defaults(per_factor_mu=per_factor_mu), hooks=True)
    eng.upload(state)
    eng.linearise()
    low = np.tril(np.ones((6, 6), bool)).ravel()
    for it in range(max(sweeps) + 1):
        if (it + 1) % 2 == 0 and it < 10:
            eng.weaken_priors()
        eng.iterate(1)
        assert eng.eval()["n_relin"] == g["dev_n_relin"][it], it
        if it not in sweeps:
            continue
        r, m = eng.read(), eng.messages()
        fe, fl = eng.factor_potentials()
        mu, dmu = eng.mu()
        full = {"fac_eta": (fe, 9), "fac_lambda": (fl, 81), "mu": (mu, 9), "damping": (r["damping"], 1),
                "damping_count": (r["damping_count"], 1), "robust_flag": (r["robust_flag"], 1),
                "msg_cam_eta": (m["cam_eta"], 6), "msg_cam_lambda": (m["cam_lambda"], 36),
                "msg_lmk_eta": (m["lmk_eta"], 3), "msg_lmk_lambda": (m["lmk_lambda"], 9)}
        if per_factor_mu:
            full["dmu"] = (dmu, 1)          # hoisted mode keeps no per-factor dmu
        same = (g["ref_it%d_damping_count" % it] == r["damping_count"][ids][:, None]).ravel()
        for k, (v, w) in full.items():
            v = v.reshape(-1, w)[ids]
            dev, ref = g["dev_it%d_%s" % (it, k)], g["ref_it%d_%s" % (it, k)]
            if k == "msg_cam_lambda":       # only the lower triangle of a camera message is stored per factor
                v, dev, ref = v[:, low], dev[:, low], ref[:, low]
            assert np.array_equal(v, dev), ("dev", it, k)
            if it <= 17 and v.dtype == np.float32 and w > 1:
                tol = 1e-4 if it <= 1 else 1e-3
                err = rel_err(v[same], ref[same])
                assert same.sum() >= 60 and err <= tol, ("ref", it, k, err)
            elif it <= 1 and k != "dmu":    # damping state and flags: exact; dmu carries the trig ulps of LINEARISE
                assert np.array_equal(v, ref), ("ref", it, k)


def test_imported_standard_bal_problem_runs_bit_exact(tmp_path, oracle_mod):
    """A standard 9-parameter BAL file (per-camera focal length + radial distortion, -z cameras, landmark-major
    edges) goes through gbp_bal_import_standard and is then solved like any sequence: GPU == oracle bit for bit,
    and the error falls from the perturbed start to the pixel level."""
    from gbp_poplar_amd import driver, hostlib
    from tests.test_hostlib import _write_standard_bal
    src = str(tmp_path / "standard.txt")
    _write_standard_bal(src, np.random.default_rng(3), n_cams=12, n_lmks=300, point_noise=0.03)
    bal = hostlib.bal_import_standard(src)
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, _ = _setup(bal, oracle_mod)
        tg = driver.run_ba(eng, state, opts, n_iters=150, eval_every=50)
        to = driver.run_ba(orc, state, opts, n_iters=150, eval_every=50)
    finally:
        oracle_mod.set_trig_mode(0)
    _assert_state_equal(eng, orc)
    for (i, mg, cg, rg, bg), (_, mo, co, ro, bo) in zip(tg, to):     # the metric: a residual of ~1e-3 px is a
        assert abs(mg - mo) <= 1e-5 * mo + 1e-6 and rg == ro and bg == bo, (i, mg, mo)   # cancelling fp32 difference
    assert tg[0][1] > 2.0 and tg[-1][1] < 0.05 * tg[0][1], (tg[0], tg[-1])


# ---- sharded (multi-GPU) kernels exercised on ONE GPU -----------------------------------------------------

class _FakeDist:
    """all_gather between shard engines living in one process: copies every rank's send buffer into every
    rank's receive buffer (what RCCL does between GPUs)."""

    def __init__(self):
        self.members = []

    def gather_all(self):
        import torch
        for m in self.members:
            m.stream.synchronize()
        for dst in self.members:
            for r, src in enumerate(self.members):
                n = src.send.numel()                 # the receive buffer is [world][C * 44]
                dst.recv[r * n:(r + 1) * n].copy_(src.send)
        torch.cuda.synchronize()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_kernels_on_one_gpu_match_sharded_oracle(world, oracle_mod):
    """`world` landmark-shard contexts on the same GPU, exchange done by device copies: the sharded C-ABI path
    (gbp_iterate_begin/_end, refresh, linearise_factors, weaken on a sharded ctx, torch-owned buffers and
    stream) against the oracle in `world`-shard device order, bit for bit, through relinearisations."""
    import torch
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp, landmark_partition
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = landmark_partition(bal["lmk_id"], bal["n_lmks"], world)
    fake = _FakeDist()
    shards = []
    for r in range(world):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                        shard=(r, world, int(bounds[r]), int(bounds[r + 1])))
        sh = ShardedGbp(eng, bal["n_cams"], r, world, dist=None, device="cuda")
        sh._exchange = lambda: None          # the exchange is performed for all shards at once below
        fake.members.append(sh)
        shards.append(sh)

    def all_do(name, *a):
        for sh in shards:
            getattr(sh.e, name)(*a)

    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1, bounds)
        orc.upload(state)
        orc.linearise()
        all_do("upload", state)
        all_do("refresh_begin"); fake.gather_all(); all_do("refresh_end"); all_do("linearise_factors")
        for it in range(24):
            if (it + 1) % 2 == 0 and it < 10:
                all_do("weaken_priors")
                orc.weaken_priors()
            all_do("iterate_begin")
            if it % 2:
                all_do("iterate_local")          # landmark half first (what overlaps the all-gather on N GPUs)
            fake.gather_all()
            all_do("iterate_end")
            orc.iterate(1)
    finally:
        oracle_mod.set_trig_mode(0)
    ro = orc.read()
    lmk = np.asarray(bal["lmk_id"])
    n_relin = 0
    for r, sh in enumerate(shards):
        g = sh.read()
        assert np.array_equal(g["cam_beliefs_eta"], ro["cam_beliefs_eta"])
        assert np.array_equal(g["cam_beliefs_lambda"], ro["cam_beliefs_lambda"])
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        assert np.array_equal(g["lmk_beliefs_eta"][3 * lo:3 * hi], ro["lmk_beliefs_eta"][3 * lo:3 * hi])
        assert np.array_equal(g["lmk_beliefs_lambda"][9 * lo:9 * hi], ro["lmk_beliefs_lambda"][9 * lo:9 * hi])
        own = (lmk >= lo) & (lmk < hi)
        assert np.array_equal(g["damping_count"][own], ro["damping_count"][own])
        assert np.array_equal(g["robust_flag"][own], ro["robust_flag"][own])
        n_relin += int(np.sum(g["damping_count"][own] == -8))
    assert n_relin > 0
    evs = [sh.e.eval() for sh in shards]
    tot = {k: sum(e[k] for e in evs) for k in ("sum_norm", "sum_half_sq", "n_active", "n_relin", "n_robust")}
    eo = orc.eval()
    assert tot["n_active"] == eo["n_active"] and tot["n_relin"] == eo["n_relin"] and tot["n_robust"] == eo["n_robust"]
    assert abs(tot["sum_norm"] - eo["sum_norm"]) <= 1e-5 * eo["sum_norm"]


def test_row_placement_is_unobservable():
    """Graphs of many small cameras (fewer than 512 factors per camera, >= 2 048 tiles: BASELINE config 5's shape) get their
    16-factor rows laid out by landmark class inside windows of 32 cameras (gbp_layout.cpp, row placement).  A row stays whole
    and a camera's rows are added in the camera's own order, so nothing may change: the default engine against tile_order = 1
    (camera-major rows, sequential tiles) on a 4 096-camera x 40 000-landmark x 400 000-factor graph, bit for bit through the
    start of a BA run; and the same through the sharded C-ABI path of a 1-shard ctx."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    bal = hostlib.synth_generate(4096, 40000, 10, 7)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    ref = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(tile_order=1))
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=(0, 1, 0, bal["n_lmks"]))
    sh = ShardedGbp(eng, bal["n_cams"], 0, 1, dist=None, device="cuda")
    fake = _FakeDist()
    fake.members.append(sh)
    sh._exchange = lambda: None
    for e in (ref, eng):
        e.upload(state)
    ref.linearise()
    eng.refresh_begin(); fake.gather_all(); eng.refresh_end(); eng.linearise_factors()
    for it in range(14):
        if (it + 1) % 2 == 0 and it < 10:
            ref.weaken_priors()
            eng.weaken_priors()
        ref.iterate(1)
        eng.iterate_begin()
        fake.gather_all()
        eng.iterate_end()
    a, b = ref.read(), sh.read()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ea, eb = ref.eval(), eng.eval()
    assert ea["n_relin"] == eb["n_relin"] and ea["n_robust"] == eb["n_robust"] and ea["sum_norm"] == eb["sum_norm"]


@pytest.mark.parametrize("shape", ["config5_like", "ragged_small"])
def test_skipping_all_pad_segments_is_unobservable(shape):
    """on graphs of many small cameras the sweep neither loads nor stores the 64-byte segments of a tile that hold
    pad positions only (k_sweep<..., SEG>: a buffer descriptor per tile, out-of-range offsets for the lanes of an all-pad segment — the
    hardware returns zeros / drops the store without touching memory).  Pads are inactive factors whose records never change, so
    nothing may change: forced on against forced off (gbp_debug_force_seg_skip), every tensor incl. both message sets and the
    potentials, bit for bit through the start of a BA run with relinearisations, the plain sweep and the one the metric rides in
    (gbp_ba_loop with metrics), on a 4 096-camera x 40 000-landmark graph (rows placed, tiles permuted: the shape that selects it by
    itself) and on a small ragged graph with inactive factors where most segments of the last tiles are empty."""
    from gbp_poplar_amd import _cabi, _lib, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    lib = _lib.load(hooks=True)
    opts = driver.Options()
    kw = {}
    if shape == "config5_like":
        bal = hostlib.synth_generate(4096, 40000, 10, 7)
    else:
        bal, kw = _ragged_bal()
        opts.undamped_start = 2
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    if shape != "config5_like":
        state["active_flag"] = _ragged_active(bal)
    engs = []
    try:
        for mode in (1, 0):
            assert lib.gbp_debug_force_seg_skip(mode) == 0
            engs.append(GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True,
                                  params=_cabi.GbpParams.defaults(persistent=-1, **kw)))
    finally:
        lib.gbp_debug_force_seg_skip(-1)
    evs = []
    for e in engs:
        e.upload(state)
        e.linearise()
        out = e.ba_loop(14, 0, int(opts.steps))                    # the metric rides in k_sweep<EV, SEG>
        e.ba_loop(25, 14, int(opts.steps), metrics=False)           # k_sweep<SEG> from the hipGraph
        out += e.ba_loop(6, 39, int(opts.steps))
        evs.append(out)
    assert evs[0] == evs[1]
    sa, sb = _full_snapshot(engs[0]), _full_snapshot(engs[1])
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (shape, k)
    assert sum(e["n_relin"] for e in evs[0]) > 0 or shape == "config5_like"


def test_sharded_slam_keyframes_on_one_gpu(oracle_mod):
    """READ_PRIORS / NEW_KEYFRAME on landmark-shard contexts (two shards on one GPU, exchange by device copies): the
    incremental SLAM flow of slam.cpp:1018-1055 with a keyframe every 12 sweeps == the oracle in 2-shard order."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp, landmark_partition
    from gbp_poplar_amd.engine import GbpEngine
    world = 2
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True)
    C, L, E = bal["n_cams"], bal["n_lmks"], bal["n_edges"]
    bounds = landmark_partition(bal["lmk_id"], L, world)
    fake = _FakeDist()
    shards = []
    for r in range(world):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(r, world, int(bounds[r]), int(bounds[r + 1])))
        sh = ShardedGbp(eng, C, r, world, dist=None, device="cuda")
        sh._exchange = lambda: None
        fake.members.append(sh)
        shards.append(sh)

    class Group:                                  # the verbs run_slam calls, applied to every shard + one exchange
        def upload(self, st):
            for sh in shards:
                sh.e.upload(st)

        def linearise(self):
            for sh in shards:
                sh.e.refresh_begin()
            fake.gather_all()
            for sh in shards:
                sh.e.refresh_end()
                sh.e.linearise_factors()

        def iterate(self, n=1):
            for _ in range(n):
                for sh in shards:
                    sh.e.iterate_begin()
                fake.gather_all()
                for sh in shards:
                    sh.e.iterate_end()

        def weaken_priors(self):
            for sh in shards:
                sh.e.weaken_priors()

        def read(self):
            out = shards[0].read()
            for r, sh in enumerate(shards[1:], 1):
                g = sh.read()
                lo, hi = int(bounds[r]), int(bounds[r + 1])
                out["lmk_beliefs_eta"][3 * lo:3 * hi] = g["lmk_beliefs_eta"][3 * lo:3 * hi]
                out["lmk_beliefs_lambda"][9 * lo:9 * hi] = g["lmk_beliefs_lambda"][9 * lo:9 * hi]
                own = (np.asarray(bal["lmk_id"]) >= lo) & (np.asarray(bal["lmk_id"]) < hi)
                for k in ("damping", "damping_count", "robust_flag"):
                    out[k][own] = g[k][own]
            return out

        def read_priors(self):
            out = shards[0].read_priors()
            for r, sh in enumerate(shards[1:], 1):
                g = sh.read_priors()
                lo, hi = int(bounds[r]), int(bounds[r + 1])
                out["lmk_priors_eta"][3 * lo:3 * hi] = g["lmk_priors_eta"][3 * lo:3 * hi]
                out["lmk_priors_lambda"][9 * lo:9 * hi] = g["lmk_priors_lambda"][9 * lo:9 * hi]
            return out

        def new_keyframe(self, upd):
            for sh in shards:
                sh.e.new_keyframe(upd)

        def eval(self):
            evs = [sh.e.eval() for sh in shards]
            return {k: sum(e[k] for e in evs) for k in evs[0]}

    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], C, L, K)
        orc.set_sum_order(1, bounds)
        tg = driver.run_slam(Group(), hostlib, bal, state, extra, opts, iters_between_kfs=12, max_iters=70, eval_every=5)
        to = driver.run_slam(orc, hostlib, bal, state, extra, opts, iters_between_kfs=12, max_iters=70, eval_every=5)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = Group().read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k], equal_nan=True), k
    for (i, mg, cg, rg, bg), (_, mo, co, ro_, bo) in zip(tg, to):
        assert abs(mg - mo) <= 1e-5 * mo and rg == ro_ and bg == bo, (i, mg, mo)
    assert len(tg) > 10 and tg[-1][1] < tg[0][1]


def test_sharded_wrapper_world1_on_gpu(oracle_mod):
    """ShardedGbp with world = 1 on the GPU (torch stream + torch-owned exchange buffers) == plain engine."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    plain = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=(0, 1, 0, bal["n_lmks"]))
    sh = ShardedGbp(eng, bal["n_cams"], 0, 1, dist=None, device="cuda")
    ta = driver.run_ba(plain, state, opts, n_iters=25, eval_every=5)
    tb = driver.run_ba(sh, state, opts, n_iters=25, eval_every=5)
    assert ta == tb
    ra, rb = plain.read(), sh.read()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    # split-phase profiling (bench.py's roofline at N > 1): every gbp_iterate_begin brackets its sweep launch
    eng.timing(reset=True)
    eng.set_profiling(True)
    sh.iterate(7)
    eng.set_profiling(False)
    tm = eng.timing(reset=True)
    assert tm["iterations"] == 7 and 0.0 < tm["sweep_ms"] / 7 < 1.0, tm
    plain.iterate(7)
    ra, rb = plain.read(), sh.read()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k


# ---- edge cases and error behaviour of the C-ABI --------------------------------------------------------------

def _tiny_problem(cam_id, lmk_id, C, L, seed=0):
    """hand-made graph with well-posed geometry: cameras on a circle looking at points near the origin"""
    rng = np.random.default_rng(seed)
    cams = np.zeros((C, 6))
    for c in range(C):
        cams[c, :3] = [0.1 * c, -0.05 * c, 5.0 + 0.2 * c]
        cams[c, 3:] = [0.05 + 0.01 * c, -0.04, 0.03 * (c + 1)]
    pts = rng.uniform(-1, 1, (L, 3))
    obs = np.zeros((len(cam_id), 2))
    for e, (c, l) in enumerate(zip(cam_id, lmk_id)):
        w = cams[c, 3:]
        th = np.linalg.norm(w)
        k = w / th
        y = pts[l]
        Ry = y * np.cos(th) + np.cross(k, y) * np.sin(th) + k * np.dot(k, y) * (1 - np.cos(th))
        p = Ry + cams[c, :3]
        obs[e] = [500 * p[0] / p[2] + 320 + rng.normal(), 500 * p[1] / p[2] + 240 + rng.normal()]
    return {"n_cams": C, "n_lmks": L, "n_edges": len(cam_id), "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0,
            "cam_id": np.asarray(cam_id, np.uint32), "lmk_id": np.asarray(lmk_id, np.uint32),
            "observations": obs.ravel(), "cameras": (cams + rng.normal(0, 0.01, cams.shape) * (np.arange(C)[:, None] >= 2)).ravel(),
            "points": (pts + rng.normal(0, 0.05, pts.shape)).ravel()}


@pytest.mark.parametrize("case", ["three_factors", "camera_without_factors", "ragged_rows"])
def test_degenerate_graph_shapes(case, oracle_mod):
    """Fewer factors than one 16-lane row, a camera with no factor at all, cameras with 1, 16, 17 and 33
    factors (row padding on every boundary): bit-exact against the oracle through 4 sweeps."""
    if case == "three_factors":
        cam_id, lmk_id, C, L = [0, 1, 2], [0, 0, 1], 3, 2
    elif case == "camera_without_factors":
        cam_id, lmk_id, C, L = [0, 0, 2, 2, 3], [0, 1, 0, 2, 1], 4, 3
    else:
        deg = [1, 16, 17, 33]
        cam_id = sum(([c] * d for c, d in enumerate(deg)), [])
        lmk_id = sum((list(range(d)) for d in deg), [])
        C, L = 4, 33
    bal = _tiny_problem(cam_id, lmk_id, C, L)
    eng, orc, opts, state, _ = _setup(bal, oracle_mod, sum_order=1)
    eng.linearise()
    orc.linearise()
    _sync_potentials(eng, orc)
    for it in range(4):
        if it == 1:
            eng.weaken_priors()
            orc.weaken_priors()
        eng.iterate(1)
        orc.iterate(1)
        _assert_state_equal(eng, orc, exact=True)
    g, o = eng.eval(), orc.eval()
    assert g["n_active"] == o["n_active"] == len(cam_id) and g["n_nonpd"] == o["n_nonpd"]
    assert g["n_nonfinite"] == (1 if case == "camera_without_factors" else 0)   # the factor-less camera has a 0/0 mean


@pytest.mark.parametrize("seed", range(8))
def test_random_graph_structures_bit_exact(seed, oracle_mod):
    """Random wiring the shipped files never show: UNSORTED edge lists (slot order = file order, ba.cpp:267-279,
    must survive the device's camera-major re-ordering), duplicate (camera, landmark) factors, a hub landmark seen
    by every camera many times, landmarks without factors, random inactive factors, both mu modes.
    14 sweeps with prior weakening and frequent relinearisations (`--undamped_start 1`, loose dmu threshold):
    every belief, message, factor potential and damping state equals the oracle's bit for bit."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    rng = np.random.default_rng(100 + seed)
    C, L = int(rng.integers(2, 40)), int(rng.integers(3, 200))
    E = int(rng.integers(max(C, L), 12 * L))
    cam_id = rng.integers(0, C, E)
    lmk_id = rng.integers(0, max(1, L - 2), E)          # the last two landmarks stay factor-less
    lmk_id[rng.random(E) < 0.15] = 0                    # hub landmark
    cam_id[:C] = np.arange(C)                           # every camera has a factor (else its prior is NaN by design)
    bal = _tiny_problem(list(cam_id), list(lmk_id), C, L, seed=seed)
    opts = driver.Options()
    opts.undamped_start = 1
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    state["active_flag"] = (rng.random(E) < 0.9).astype(np.uint32)
    oracle_mod.set_trig_mode(1)
    try:
        kw = dict(dmu_threshold=0.05, min_linear_iters=3, num_undamped_iters=2)    # relinearise early and often
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, params=_cabi.GbpParams.defaults(per_factor_mu=seed % 2, **kw), hooks=True)
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], C, L, K, params=_cabi.GbpParams.defaults(**kw))
        orc.set_sum_order(1)
        for x in (eng, orc):
            x.upload(state)
            x.linearise()
        n_relin = 0
        for it in range(14):
            if (it + 1) % 2 == 0 and it < 10:
                eng.weaken_priors()
                orc.weaken_priors()
            eng.iterate(1)
            orc.iterate(1)
            _assert_state_equal(eng, orc, exact=True)
            g, o = eng.eval(), orc.eval()
            assert (g["n_relin"], g["n_robust"], g["n_active"]) == (o["n_relin"], o["n_robust"], o["n_active"])
            n_relin += g["n_relin"]
        fe, fl = eng.factor_potentials()
        oe, ol = orc.factor_potentials()
        assert np.array_equal(fe, oe) and np.array_equal(fl, ol)
    finally:
        oracle_mod.set_trig_mode(0)
    assert n_relin > 0


def test_xcd_aware_tile_order_is_unobservable():
    """gbp_params.tile_order only changes which XCD works on which landmark blocks (0) and sweep tiles (2, 3: a permutation
    table read once per wave; 3 — the local permutation — is what 0 selects by itself on large graphs): every tensor is
    identical to the sequential order (1), here on a graph of ~100 workgroups / 49 landmark blocks (not multiples of 8)."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = small_synth(n_cams=37, n_lmks=3100, obs=8, seed=21)
    opts = driver.Options()
    opts.undamped_start = 2
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    snaps = []
    for order in (1, 0, 2, 3):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                        params=_cabi.GbpParams.defaults(tile_order=order, dmu_threshold=0.05, min_linear_iters=3), hooks=True)
        traj = driver.run_ba(eng, state, opts, n_iters=25, eval_every=5)
        d = _gpu_snapshot(eng)
        d["mu"] = eng.mu()[0]
        snaps.append((traj, d))
    assert snaps[0][0] == snaps[1][0] == snaps[2][0] == snaps[3][0]
    assert sum(t[3] for t in snaps[0][0]) > 0                      # relinearisations happened
    for other in snaps[1:]:
        for k, v in snaps[0][1].items():
            assert np.array_equal(v, other[1][k], equal_nan=True), k


def test_error_codes_and_call_order():
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = small_synth(n_cams=4, n_lmks=20, obs=3, seed=5)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], 4, 20, K)
    for call in (eng.linearise, lambda: eng.iterate(1), eng.weaken_priors, eng.eval):
        with pytest.raises(GbpError, match="upload first"):          # GBP_ERR_STATE: nothing uploaded yet
            call()
    bad = dict(state)
    del bad["cam_priors_lambda"]
    with pytest.raises(GbpError, match="required"):
        eng.upload(bad)
    with pytest.raises(GbpError, match="out of range"):               # indices are validated at create
        GbpEngine(np.array([0, 9], np.uint32), np.array([0, 1], np.uint32), 4, 20, K)
    with pytest.raises(GbpError, match="bad shard"):
        GbpEngine(bal["cam_id"], bal["lmk_id"], 4, 20, K, shard=(2, 2, 0, 20))
    sh = GbpEngine(bal["cam_id"], bal["lmk_id"], 4, 20, K, shard=(0, 2, 0, 10))
    sh.upload(state)
    with pytest.raises(GbpError, match="sharded ctx"):
        sh.linearise()
    with pytest.raises(GbpError, match="sharded ctx"):
        sh.iterate(1)
    with pytest.raises(GbpError, match="exchange buffers not set"):
        sh.iterate_begin()
    sh.prepare()                                                       # nothing to capture on a sharded ctx: a no-op, not an error
    with pytest.raises(GbpError, match="gbp_comm_init"):
        import ctypes
        sh._chk(sh.lib.gbp_comm_init(sh.h, ctypes.create_string_buffer(4096), 0), "gbp_comm_init")   # not an initialised region
    eng.upload(state)
    eng.linearise()
    eng.iterate(0)                                                     # n = 0 is a no-op
    eng.iterate(3)
    t = eng.timing()
    assert t["iterations"] == 3 and t["algorithmic_bytes_per_iter"] == 1112 * bal["n_edges"] + 336 * 4 + 96 * 20


def test_eval_begin_end_pipelining():
    """gbp_eval in two halves: up to two metrics in flight while further iterations are queued; results equal the
    synchronous gbp_eval of the same beliefs (the CLIs print iteration i after queuing iteration i + 1)."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = _bal("fr2robot2")
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    for e in (a, b):
        e.upload(state)
        e.linearise()
    want, got = [], []
    for it in range(6):
        a.iterate(1)
        want.append(a.eval())
    b.iterate(1)
    b.eval_begin()
    for it in range(1, 6):
        b.iterate(1)                # queued before the previous metric is collected
        b.eval_begin()
        got.append(b.eval_end())
    with pytest.raises(GbpError, match="in flight"):
        b.eval()                    # the synchronous call refuses to jump the queue
    got.append(b.eval_end())
    assert got == want
    with pytest.raises(GbpError, match="no evaluation in flight"):
        b.eval_end()
    b.eval_begin(); b.eval_begin()
    with pytest.raises(GbpError, match="two evaluations already in flight"):
        b.eval_begin()
    assert b.eval_end() == b.eval_end() == want[-1]


def test_health_counters(oracle_mod):
    """A non-PD landmark prior (negative Lambda) must show up in n_nonpd after the belief refresh."""
    from gbp_poplar_amd import driver, hostlib
    bal = small_synth(n_cams=5, n_lmks=30, obs=3, seed=4)
    eng, orc, opts, state, _ = _setup(bal, oracle_mod)
    state = dict(state)
    lam = state["lmk_priors_lambda"].copy()
    lam[9 * 7:9 * 8] *= -1.0
    state["lmk_priors_lambda"] = lam
    eng.upload(state)
    orc.upload(state)
    eng.linearise()
    orc.linearise()
    g, o = eng.eval(), orc.eval()
    assert g["n_nonpd"] == o["n_nonpd"] == 1 and g["n_nonfinite"] == 0
    # ... and, counted per iteration, out of the launches of the persistent kernel that carry the metric (their health words travel
    # from the owners' device counters to the host's slots behind the launch's closing barrier)
    assert eng.graph_state() == 2
    ge = eng.iterate_eval_each(3)
    for k in range(3):
        orc.iterate(1)
        oe = orc.eval()
        assert (ge[k]["n_nonpd"], ge[k]["n_nonfinite"], ge[k]["n_active"]) == (oe["n_nonpd"], oe["n_nonfinite"], oe["n_active"]), (k, ge[k], oe)
    assert ge[0]["n_nonpd"] >= 1
    eng.iterate_eval(2)
    orc.iterate(2)
    g, o = eng.eval_end(), orc.eval()
    assert (g["n_nonpd"], g["n_nonfinite"]) == (o["n_nonpd"], o["n_nonfinite"]) and g["n_nonpd"] >= 1


@pytest.mark.parametrize("flow", [1, 0], ids=["tagged_records", "barriers"])
def test_health_counters_with_metric_calls_of_every_kind_interleaved(flow, oracle_mod):
    """Found by profiles/fuzz_parity.py (round 6, seed 19): gbp_eval between two gbp_ba_loop calls left its count in the health area it
    had used (only the NEXT gbp_eval's k_means reset it), and the barrier variant of the persistent kernel — which counts the metrics of
    a burst into both areas alternately — reported the first iteration of the next burst twice as unhealthy.  Now every user of the
    health words leaves them zero.  A graph with landmarks nobody observes (zero prior -> infinite weakening scale -> NaN belief from
    the first weakening on, by design: dataio.cpp:76-95, ba.cpp:564): gbp_eval, gbp_ba_loop, gbp_iterate_eval + gbp_eval_end and
    gbp_iterate_eval_each in turn on the persistent kernel against one call at a time on the two-kernel path — every metric equal."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal, kw = _ragged_bal()
    opts = driver.Options()
    opts.undamped_start = 2
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    steps = int(opts.steps)
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=1, **kw))
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
    assert a.graph_state() == 2
    a.persist_flow(flow)
    for e in (a, b):
        e.upload(state)
        e.linearise()
    it = [0]

    def step_b(n):
        out = []
        for i in range(it[0], it[0] + n):
            if (i + 1) % 2 == 0 and i < 2 * steps:
                b.weaken_priors()
            b.iterate(1)
            out.append(b.eval())
        return out

    assert a.eval() == b.eval()
    for n, kind in ((2, "loop"), (1, "eval"), (5, "loop"), (1, "eval"), (4, "loop"), (3, "iterate_eval"), (1, "eval"), (3, "each"), (2, "loop")):
        if kind == "eval":
            assert a.eval() == b.eval(), (kind, it[0])
            continue
        if kind == "loop":
            ea = a.ba_loop(n, it[0], steps)
            eb = step_b(n)
        else:
            assert it[0] >= 2 * steps      # (no weakening inside: these two calls know nothing of the loop's schedule)
            eb = step_b(n)
            if kind == "each":
                ea = a.iterate_eval_each(n)
            else:
                a.iterate_eval(n)
                ea, eb = [a.eval_end()], eb[-1:]
        assert ea == eb, (kind, it[0], [(x["n_nonfinite"], y["n_nonfinite"]) for x, y in zip(ea, eb)])
        it[0] += n
    assert eb[-1]["n_nonfinite"] > 0 and eb[-1]["n_nonpd"] > 0


def test_pad_lanes_do_not_wait_for_a_factorless_first_landmark_group():
    """Found by the seeded slice of the soak (tests/test_gpu_fuzz.py, SLAM seed 60099): a pad position names landmark 0 without being
    one of its factors.  Where landmarks 0 .. 15 — one wave's group in k_persist_flow — have no factor at all, their owner waits for
    nobody, runs iterations ahead and overwrites the half of its tagged records a pad lane still polled for the older tag: the tile wave
    waited 1.5 s for a tag that was gone, the launch timed out and the ctx left the persistent path (launch 7 and launch 3 of two runs of
    that seed: a race the tile usually won).  Pad lanes wait for nothing now.  Here: such a graph, 120 launches of every kind on the
    tagged-record kernel, none may time out, and the state equals the two-kernel path's bit for bit."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    from tests import fuzz_support as fz
    rng = np.random.default_rng(60099)
    bal = fz.random_problem(rng, size="tiny")
    bal["lmk_id"] = bal["lmk_id"] + np.uint32(16)          # landmarks 0 .. 15: no factor
    bal["n_lmks"] += 16
    bal["points"] = np.concatenate([rng.uniform(-1, 1, 48), bal["points"]])
    deg = np.bincount(bal["cam_id"], minlength=bal["n_cams"])
    assert (deg % 16 != 0).any()                           # pad positions exist
    opts = driver.Options()
    opts.undamped_start = 2
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    steps = int(opts.steps)
    kw = dict(dmu_threshold=0.02, min_linear_iters=3, num_undamped_iters=2)
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=1, **kw))
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
    assert a.graph_state() == 2
    for e in (a, b):
        e.upload(state)
        e.linearise()
    it, evs = 0, []
    for launch in range(120):
        n = 2 + launch % 3
        if launch % 3 == 0:
            a.iterate(n) if it >= 2 * steps else a.ba_loop(n, it, steps, metrics=False)
        elif launch % 3 == 1:
            evs = a.ba_loop(n, it, steps)
        else:
            a.ba_loop(n, it, steps, metrics=False)
        for i in range(it, it + n):
            if (i + 1) % 2 == 0 and i < 2 * steps:
                b.weaken_priors()
            b.iterate(1)
        it += n
        if launch % 3 == 1:
            eb = b.eval()
            assert all(evs[-1][k] == eb[k] or (evs[-1][k] != evs[-1][k] and eb[k] != eb[k]) for k in eb), (launch, evs[-1], eb)
    a.sync()
    assert a.graph_state() == 2 and "timed out" not in a.last_error(), a.last_error()
    sa, sb = fz.snapshot(a), fz.snapshot(b)
    for k in sb:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k


# ---- BASELINE.json's full size (S1: 1 000 cams x 100 000 lmks x 1 000 000 factors) ---------------------------------

@pytest.fixture(scope="module")
def s1():
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.synth_generate(1000, 100000, 10, 20200303)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    return bal, opts, K, state


def test_full_size_s1_bit_exact_first_sweeps(s1, oracle_mod):
    """LINEARISE + 3 sweeps (with one prior weakening) of the 1M-factor graph: every belief bit for bit against
    the oracle (device conventions), metric and counters equal."""
    from gbp_poplar_amd.engine import GbpEngine
    bal, opts, K, state = s1
    oracle_mod.set_trig_mode(1)
    try:
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        for e in (eng, orc):
            e.upload(state)
            e.linearise()
        ge, gl = eng.factor_potentials()
        oe, ol = orc.factor_potentials()
        assert np.array_equal(ge, oe) and np.array_equal(gl, ol)
        for it in range(3):
            if it == 1:
                eng.weaken_priors()
                orc.weaken_priors()
            eng.iterate(1)
            orc.iterate(1)
        g, o = eng.read(), orc.read()
        for k in g:
            assert np.array_equal(g[k], o[k]), k
        eg, eo = eng.eval(), orc.eval()
        assert eg["n_active"] == eo["n_active"] == 1000000 and eg["n_robust"] == eo["n_robust"]
        assert abs(eg["sum_norm"] - eo["sum_norm"]) <= 1e-6 * eo["sum_norm"] and eg["n_nonpd"] == eo["n_nonpd"] == 0
    finally:
        oracle_mod.set_trig_mode(0)


def test_full_size_s1_bit_exact_through_the_lockstep_relinearisation(s1, oracle_mod):
    """The ./ba flow on the 1M-factor graph through its FIRST LOCK-STEP RELINEARISATION: damping_count starts at -15
    (ba.cpp:581), so sweep 17 (0-based) is the first in which count > min_linear_iters - num_undamped_iters
    (gbp_codelets.cpp:280) and — the graph converges — nearly every factor relinearises in the same launch (all lanes in
    relin_core, every potential written back, the camera-only Jacobian terms taken from the per-camera CAM_LIN records).
    LINEARISE + 20 (or 30) sweeps, prior weakening on 1,3,5,7,9; oracle in the device's conventions.  The lock-step sweep is
    the first from 17 on in which the counters report > 900 000 relinearisations (sweep 18 on this graph).
      * after it: factor potentials (eta 9 + Lambda 81 per factor), every belief, damping, damping_count, robust_flag
        bit for bit, n_relin > 900 000 (so the test cannot pass vacuously);
      * after sweep 19 (29): state bit for bit again (the sweeps that consume the relinearised potentials);
      * a second engine (product library) runs sweeps 10..19 (29) as ONE gbp_iterate call = replays of the captured
        hipGraph: same final state."""
    from gbp_poplar_amd.engine import GbpEngine
    bal, opts, K, state = s1
    state_keys = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count",
                  "robust_flag")
    oracle_mod.set_trig_mode(1)
    try:
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        for e in (eng, orc):
            e.upload(state)
            e.linearise()

        def sweeps(e, first, last):
            for it in range(first, last + 1):
                if ((it + 1) % 2 == 0) and (it < opts.steps * 2):
                    e.weaken_priors()
                e.iterate(1)

        sweeps(eng, 0, 16)
        sweeps(orc, 0, 16)
        assert eng.eval()["n_relin"] == orc.eval()["n_relin"] == 0      # count <= 2 so far: nobody may relinearise yet
        lock = None
        for it in range(17, 24):                                        # the first sweep with dmu < 3e-3 on (nearly) every factor
            sweeps(eng, it, it)
            sweeps(orc, it, it)
            eg, eo = eng.eval(), orc.eval()
            assert eg["n_relin"] == eo["n_relin"] and eg["n_robust"] == eo["n_robust"], (it, eg, eo)
            if eg["n_relin"] > 900000:
                lock = it
                break
        assert lock is not None, "no lock-step relinearisation up to sweep 23: the test would be vacuous"
        ge, gl = eng.factor_potentials()
        oe, ol = orc.factor_potentials()
        assert np.array_equal(ge, oe), "potential eta after the lock-step relinearisation"
        assert np.array_equal(gl, ol), "potential Lambda after the lock-step relinearisation"
        del ge, gl, oe, ol
        g, o = eng.read(), orc.read()
        for k in state_keys:
            assert np.array_equal(g[k], o[k]), ("after the lock-step sweep %d" % lock, k)
        assert int((g["damping_count"] == -8).sum()) == eg["n_relin"]
        last = 10 * ((lock + 10) // 10) - 1                             # a multiple of 10 sweeps in total: 19 or 29
        sweeps(eng, lock + 1, last)
        sweeps(orc, lock + 1, last)
        g, o = eng.read(), orc.read()
        for k in state_keys:
            assert np.array_equal(g[k], o[k]), ("after sweep %d" % last, k)
        eng.close()

        eng2 = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)     # the product library
        eng2.upload(state)
        eng2.linearise()
        sweeps(eng2, 0, 9)
        eng2.iterate(last - 9)                   # sweeps 10..last (the lock-step one included) from the hipGraph
        assert eng2.graph_state() == 1
        g2 = eng2.read()
        for k in state_keys:
            assert np.array_equal(g2[k], o[k]), ("hipGraph burst", k)
        eng2.close()
    finally:
        oracle_mod.set_trig_mode(0)


def test_full_size_s1_default_loop_stays_on_the_device(s1):
    """The reference's default loop — the metric after EVERY iteration (ba.cpp:1001-1053) — on the 1M-factor graph:
    gbp_iterate_eval_each rides the metric in the two-kernel path (bursts from the hipGraph, no host hand-shake inside a burst).
    The ./ba flow for 45 iterations (through the lock-step relinearisation): every metric and the final state identical to
    {gbp_iterate(1); gbp_eval()} per iteration; and the burst costs what the iterations alone cost (<= 1.10 x gbp_iterate's time on
    the same engine: VERDICT r04 asks 1.05, measured in profiles/r05_configs.md)."""
    import time
    from gbp_poplar_amd.engine import GbpEngine
    bal, opts, K, state = s1
    a = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    b = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    for e in (a, b):
        e.upload(state)
        e.linearise()
    it, got, want = 0, [], []
    while it < 45:
        if ((it + 1) % 2 == 0) and it < 10:
            a.weaken_priors()
            b.weaken_priors()
        n = 1
        while it + n < 45 and not (((it + n + 1) % 2 == 0) and it + n < 10):
            n += 1
        got += a.iterate_eval_each(n)
        for _ in range(n):
            b.iterate(1)
            want.append(b.eval())
        it += n
    assert got == want, [(i, got[i], want[i]) for i in range(45) if got[i] != want[i]][:2]
    assert max(e["n_relin"] for e in got) > 900000 and got[-1]["n_active"] == 1000000
    ra, rb = a.read(), b.read()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k

    def timed(f, n):
        a.sync()
        t0 = time.perf_counter()
        f(n)
        a.sync()
        return (time.perf_counter() - t0) / n
    a.iterate(40)
    a.iterate_eval_each(40)              # both graphs captured, both warm
    t_plain = min(timed(a.iterate, 200) for _ in range(3))
    t_each = min(timed(a.iterate_eval_each, 200) for _ in range(3))
    assert t_each <= 1.10 * t_plain, (t_each, t_plain)


def test_full_size_s1_properties(s1):
    """Size-independent properties at full size: run-to-run determinism, hipGraph replay == direct launches,
    hoisted == per-factor mu, monotone convergence to the noise floor, healthy beliefs."""
    from gbp_poplar_amd import _cabi, driver
    from gbp_poplar_amd.engine import GbpEngine
    bal, opts, K, state = s1

    def run(per_factor_mu, graph):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                        params=_cabi.GbpParams.defaults(per_factor_mu=per_factor_mu))
        eng.upload(state)
        eng.linearise()
        ev = [eng.eval()]
        for it in range(10):                      # reference start-up: weaken on 1,3,5,7,9
            if (it + 1) % 2 == 0:
                eng.weaken_priors()
            eng.iterate(1)
        if graph:
            eng.iterate(40)                       # 4 replays of the captured 10-iteration graph
        else:
            for _ in range(40):
                eng.iterate(1)
        ev.append(eng.eval())
        return eng.read(), ev

    a, eva = run(0, True)
    b, _ = run(0, True)
    c, _ = run(0, False)
    d, _ = run(1, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), ("determinism", k)
        assert np.array_equal(a[k], c[k]), ("graph replay", k)
        assert np.array_equal(a[k], d[k]), ("hoisted vs per-factor mu", k)
    m0, m1 = driver.metric(eva[0]), driver.metric(eva[1])
    assert 7.0 < m0[2] < 10.0 and 1.25 < m1[2] < 1.40, (m0, m1)      # RMSE: 8.44 px -> 1.30 px (1 px pixel noise)
    assert eva[1]["n_nonfinite"] == 0 and eva[1]["n_nonpd"] == 0 and eva[1]["n_active"] == 1000000


# ---- BASELINE config 5 at size: 8 000 cams x 1 000 000 lmks x 10 000 000 factors, 8 landmark shards ------------------------

def test_upload_of_a_graph_beyond_the_staging_buffer(oracle_mod):
    """gbp_upload moves the per-factor streams in compact form (20 bytes per position) and k_upload_scatter writes the records: out of
    the pinned staging buffer up to 32 MB (every other test), through a device buffer of the call's own beyond — 1.8 M factors here.
    Two sweeps with a weakening, every belief and the per-factor state bit for bit against the oracle; inactive factors and non-default
    damping state in the upload."""
    from gbp_poplar_amd import driver, hostlib
    bal = hostlib.synth_generate(400, 180000, 10, 31)
    eng, orc, opts, state, _ = _setup(bal, oracle_mod, hooks=False)
    rng = np.random.default_rng(3)
    state = dict(state)
    state["active_flag"] = (rng.random(bal["n_edges"]) < 0.95).astype(np.uint32)
    state["damping"] = rng.choice(np.array([0.0, 0.4], np.float32), bal["n_edges"])
    state["damping_count"] = rng.integers(-15, 3, bal["n_edges"]).astype(np.int32)
    oracle_mod.set_trig_mode(1)
    try:
        for x in (eng, orc):
            x.upload(state)
            x.linearise()
        for it in range(2):
            if it == 1:
                eng.weaken_priors()
                orc.weaken_priors()
            eng.iterate(1)
            orc.iterate(1)
        _assert_state_equal(eng, orc, exact=True)
        g, o = eng.eval(), orc.eval()
    finally:
        oracle_mod.set_trig_mode(0)
    assert (g["n_active"], g["n_relin"], g["n_robust"]) == (o["n_active"], o["n_relin"], o["n_robust"]) and g["n_active"] < bal["n_edges"]


def test_config5_at_size_eight_shards_on_one_gpu(oracle_mod):
    """The graph of BASELINE config 5 through the SHARDED kernels: eight landmark-shard contexts (what the eight ranks
    of an 8-GPU run hold) on one GPU, camera partial sums exchanged by device copies (what the RCCL all-gather moves).
      * LINEARISE + 2 sweeps (one prior weakening): every belief and the damping / robust state bit for bit against the
        oracle in 8-shard order;
      * against the unsharded engine on the same graph: <= 2e-6 per sweep (only the association order of the camera
        sums differs: rows of 16 per shard, then rank order);
      * run-to-run determinism (second run from a fresh upload on the same contexts: identical bits);
      * 50 iterations of the ./ba flow converge to the pixel-noise floor (RMSE ~1.30 px), no non-finite / non-PD belief."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp, landmark_partition
    from gbp_poplar_amd.engine import GbpEngine
    world = 8
    bal = hostlib.synth_generate(8000, 1000000, 10, 20200303)
    C, L, E = bal["n_cams"], bal["n_lmks"], bal["n_edges"]
    assert (C, L, E) == (8000, 1000000, 10000000)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = landmark_partition(bal["lmk_id"], L, world)
    lmk = np.asarray(bal["lmk_id"])
    per_shard = np.diff(np.searchsorted(np.sort(lmk), bounds))
    assert per_shard.sum() == E and per_shard.max() - per_shard.min() <= 20           # balanced by factor count
    fake = _FakeDist()
    shards = []
    for r in range(world):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K, shard=(r, world, int(bounds[r]), int(bounds[r + 1])))
        sh = ShardedGbp(eng, C, r, world, dist=None, device="cuda")
        sh._exchange = lambda: None
        fake.members.append(sh)
        shards.append(sh)

    def all_do(name, *a):
        for sh in shards:
            getattr(sh.e, name)(*a)

    def group_start():
        all_do("upload", state)
        all_do("refresh_begin"); fake.gather_all(); all_do("refresh_end"); all_do("linearise_factors")

    def group_iterate(n, first=0):
        for it in range(first, first + n):
            if (it + 1) % 2 == 0 and it < 10:
                all_do("weaken_priors")
            all_do("iterate_begin")
            if it % 2:
                all_do("iterate_local")
            fake.gather_all()
            all_do("iterate_end")

    def group_read():
        out = shards[0].read()
        for r, sh in enumerate(shards[1:], 1):
            g = sh.read()
            assert np.array_equal(g["cam_beliefs_eta"], out["cam_beliefs_eta"])       # replicated cameras: identical on all ranks
            assert np.array_equal(g["cam_beliefs_lambda"], out["cam_beliefs_lambda"])
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            out["lmk_beliefs_eta"][3 * lo:3 * hi] = g["lmk_beliefs_eta"][3 * lo:3 * hi]
            out["lmk_beliefs_lambda"][9 * lo:9 * hi] = g["lmk_beliefs_lambda"][9 * lo:9 * hi]
            own = (lmk >= lo) & (lmk < hi)
            for k in ("damping", "damping_count", "robust_flag"):
                out[k][own] = g[k][own]
        return out

    group_start()
    group_iterate(2)
    g = group_read()

    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], C, L, K)
        orc.set_sum_order(1, bounds)
        orc.upload(state)
        orc.linearise()
        orc.iterate(1)
        orc.weaken_priors()
        orc.iterate(1)
        o = orc.read()
        orc.close()
        del orc
    finally:
        oracle_mod.set_trig_mode(0)
    for k in g:
        assert np.array_equal(g[k], o[k]), k

    plain = GbpEngine(bal["cam_id"], bal["lmk_id"], C, L, K)
    plain.upload(state)
    plain.linearise()
    plain.iterate(1)
    plain.weaken_priors()
    plain.iterate(1)
    p = plain.read()
    plain.close()
    for k, w in (("cam_beliefs_eta", 6), ("cam_beliefs_lambda", 36), ("lmk_beliefs_eta", 3), ("lmk_beliefs_lambda", 9)):
        assert per_var_rel(g[k], p[k], w) <= 4e-6, (k, per_var_rel(g[k], p[k], w))   # 2 sweeps x 2e-6
    assert np.array_equal(g["damping_count"], p["damping_count"]) and np.array_equal(g["robust_flag"], p["robust_flag"])

    group_start()                       # determinism: the same two sweeps again from a fresh upload
    group_iterate(2)
    g2 = group_read()
    for k in g:
        assert np.array_equal(g[k], g2[k]), ("determinism", k)

    group_iterate(48, first=2)          # ... and on to 50 iterations of the ./ba flow
    evs = [sh.e.eval() for sh in shards]
    tot = {k: sum(e[k] for e in evs) for k in evs[0]}
    m = driver.metric(tot)
    assert tot["n_active"] == E and tot["n_nonfinite"] == 0 and tot["n_nonpd"] == 0
    assert 1.25 < m[2] < 1.40, m        # RMSE at the 1 px pixel-noise floor (S1: 1.30)


def test_ba_mp_front_end_single_gpu(capsys):
    """examples/ba_torchrun.py (a caller with its own collective around the split-phase C-ABI) on one GPU prints the ba lines and converges."""
    ba_mp = _example("ba_torchrun")
    rc = ba_mp.main(["--bal_file", seq_path("fr2robot2"), "--n_iters", "40", "--eval_every", "10"])
    out = capsys.readouterr().out
    assert rc == 0 and "Initial Reprojection error: 39.8638" in out and out.count("Weakening priors") == 5
    last = [l for l in out.splitlines() if l.startswith("Iter 39 ")]
    assert last and 0.5 < float(last[0].split("Reprojection error ")[1].split(" ")[0]) < 5.0


def test_ba_mp_front_end_init_options(capsys):
    """The initialisation flags of ba.cpp:422-441 in the Python front end: --tn/--rn/--ltn with --seed reproduce, --avdepth_on
    re-places the landmarks (same host functions as the C++ CLIs: gbp_init_add_noise / gbp_init_av_depth)."""
    ba_mp = _example("ba_torchrun")
    outs = []
    for seed in ("4", "4", "5"):
        assert ba_mp.main(["--bal_file", seq_path("fr2robot2"), "--n_iters", "12", "--eval_every", "4", "--tn", "0.02", "--rn", "0.5",
                           "--ltn", "0.02", "--seed", seed]) == 0
        outs.append([l for l in capsys.readouterr().out.splitlines() if l.startswith(("Initial", "Iter "))])
    assert outs[0] == outs[1] and outs[0] != outs[2] and len(outs[0]) == 4
    assert ba_mp.main(["--bal_file", seq_path("fr1xyz"), "--n_iters", "2", "--avdepth_on", "1"]) == 0
    assert "Initial Reprojection error: 209.34" in capsys.readouterr().out          # the C++ CLI's value (tests/test_cli.py)


def test_ba_mp_front_end_slam_mode(capsys):
    """`ba_mp --slam` (what `./slam --ipus N` maps to) on one GPU: keyframes are added and the slam lines printed."""
    ba_mp = _example("ba_torchrun")
    rc = ba_mp.main(["--bal_file", seq_path("fr2robot2"), "--slam", "--iters_between_kfs", "20", "--eval_every", "19"])
    out = capsys.readouterr().out
    assert rc == 0 and "Initial Reprojection error: 32.7526" in out          # two keyframes active
    assert out.count("Adding keyframe") == 18 and "Adding keyframe 19," in out   # cameras 2..19 join one by one
    last = [l for l in out.splitlines() if l.startswith("Iters ")][-1]
    assert 0.5 < float(last.split("Reprojection error ")[1].split(" ")[0]) < 10.0


@pytest.mark.parametrize("kw", [{"relin_mode": 1}, {"dmu_threshold": 3e-2, "maxeta_damping": 0.25, "nstds": 1.5,
                                                     "num_undamped_iters": 4, "min_linear_iters": 6}])
def test_non_default_parameters_bit_exact(kw, oracle_mod):
    """gbp_params reach the kernels: relin_mode = reset (quirk C-1 'fixed') and non-default hyper-parameters
    (gbp_codelets.cpp:11-16) give the oracle's result bit for bit through relinearisations."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    oracle_mod.set_trig_mode(1)
    try:
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**kw))
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                                params=_cabi.GbpParams.defaults(**kw))
        orc.set_sum_order(1)
        tg = driver.run_ba(eng, state, opts, n_iters=30, eval_every=30)
        to = driver.run_ba(orc, state, opts, n_iters=30, eval_every=30)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    assert tg[-1][3] == to[-1][3] and tg[-1][4] == to[-1][4]


def test_slam_non_default_parameters_and_hoist_guard(oracle_mod):
    """SLAM flow with non-default hyper-parameters (hoisted means, the default): bit for bit against the oracle.  And
    the one combination the hoisted path cannot reproduce — a factor that could relinearise on its FIRST active sweep
    (damping_count + 1 > min_linear_iters - num_undamped_iters) — is refused by gbp_new_keyframe unless the ctx keeps the
    literal per-factor mu tensors, with which it matches the oracle again."""
    from gbp_poplar_amd import _cabi, driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True)

    def run(kw, per_factor_mu, n=80):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K,
                        params=_cabi.GbpParams.defaults(per_factor_mu=per_factor_mu, **kw))
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**kw))
        orc.set_sum_order(1)
        tg = driver.run_slam(eng, hostlib, bal, state, extra, opts, iters_between_kfs=20, max_iters=n, eval_every=10)
        to = driver.run_slam(orc, hostlib, bal, state, extra, opts, iters_between_kfs=20, max_iters=n, eval_every=10)
        g, o = eng.read(), orc.read()
        for k in g:
            assert np.array_equal(g[k], o[k]), (kw, k)
        assert [t[3:] for t in tg] == [t[3:] for t in to]
        return sum(t[3] for t in tg)

    oracle_mod.set_trig_mode(1)
    try:
        assert run({"dmu_threshold": 3e-2, "maxeta_damping": 0.25, "nstds": 1.5, "num_undamped_iters": 4, "min_linear_iters": 6}, 0) > 0
        risky = {"dmu_threshold": 10.0, "num_undamped_iters": 20, "min_linear_iters": 0}     # threshold -20 < -15 + 1
        with pytest.raises(GbpError, match="per_factor_mu"):
            run(risky, 0)
        assert run(risky, 1) > 0
    finally:
        oracle_mod.set_trig_mode(0)


def test_empty_landmark_shard(oracle_mod):
    """A rank whose landmark range is empty (more ranks than populated landmark ranges) still takes part in every
    exchange: its kernels run over pad tiles only, its partial sums are zero, the group result is unchanged."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    bal = small_synth(n_cams=6, n_lmks=40, obs=3, seed=9)
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    L = bal["n_lmks"]
    bounds = [0, L, L]                                   # rank 1 owns nothing
    fake = _FakeDist()
    shards = []
    for r in range(2):
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], L, K, shard=(r, 2, bounds[r], bounds[r + 1]))
        sh = ShardedGbp(eng, bal["n_cams"], r, 2, dist=None, device="cuda")
        fake.members.append(sh)
        shards.append(sh)
    plain = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], L, K)
    plain.upload(state)
    plain.linearise()
    for sh in shards:
        sh.e.upload(state)
        sh.e.refresh_begin()
    fake.gather_all()
    for sh in shards:
        sh.e.refresh_end()
        sh.e.linearise_factors()
    for it in range(6):
        if it % 2:
            plain.weaken_priors()
            for sh in shards:
                sh.e.weaken_priors()
        plain.iterate(1)
        for sh in shards:
            sh.e.iterate_begin()
        fake.gather_all()
        for sh in shards:
            sh.e.iterate_end()
    a, b, c = plain.read(), shards[0].read(), shards[1].read()
    for k in ("cam_beliefs_eta", "cam_beliefs_lambda"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k      # one non-empty shard == the plain engine
    assert np.array_equal(a["lmk_beliefs_eta"], b["lmk_beliefs_eta"])
    assert shards[1].e.eval()["n_active"] == 0


def test_rccl_single_rank_group_overlap_path():
    """The exact code path of an N-GPU run (RCCL all_gather_into_tensor with async_op, landmark half overlapped,
    stream-ordered camera combine) on a 1-rank RCCL group: must equal the plain single-GPU engine bit for bit."""
    import os
    import torch
    import torch.distributed as dist
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29600 + os.getpid() % 300)
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        bal = _bal("fr2robot2")
        opts = driver.Options()
        K, state, _ = driver.build_inputs(bal, opts, hostlib)
        plain = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=(0, 1, 0, bal["n_lmks"]))
        sh = ShardedGbp(eng, bal["n_cams"], 0, 1, dist=dist, device="cuda", always_collective=True)
        ta = driver.run_ba(plain, state, opts, n_iters=30, eval_every=10)
        tb = driver.run_ba(sh, state, opts, n_iters=30, eval_every=10)
        assert ta == tb
        ra, rb = plain.read(), sh.read()
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("single_stream", ["1", "0"])
def test_native_rccl_communicator_single_rank(single_stream, oracle_mod, monkeypatch):
    """The exchange owned by the C++ library: a sharded ctx with a 1-rank RCCL communicator (gbp_comm_unique_id /
    gbp_comm_init_rccl; librccl dlopen'ed by the library).  gbp_linearise / gbp_iterate / gbp_weaken_priors then run the
    sharded sequence — sweep, local partials, ncclAllGather on the second stream overlapped with the landmark beliefs,
    camera combine — first directly, then replayed from a captured hipGraph: equal to the plain engine bit for bit."""
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    plain = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    from gbp_poplar_amd import _cabi
    # "0": the >= 4-rank configuration (all-gather on a second, high-priority stream beside the landmark beliefs);
    # "1": the <= 2-rank default (one stream) — read by gbp_comm_init*
    monkeypatch.setenv("GBP_COMM_SINGLE_STREAM", single_stream)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=(0, 1, 0, bal["n_lmks"]),
                    params=_cabi.GbpParams.defaults(graph_unroll=10))      # the sharded graph is opt-in
    eng.comm_init_rccl(eng.comm_unique_id())
    assert eng.comm_transport() == "rccl"
    ta = driver.run_ba(plain, state, opts, n_iters=12, eval_every=4)
    tb = driver.run_ba(eng, state, opts, n_iters=12, eval_every=4)
    assert ta == tb
    plain.iterate(45)
    assert eng.graph_state() == 0
    eng.iterate(45)                       # 4 replays of the captured 10-iteration graph + 5 direct
    assert eng.graph_state() == 1         # kernels + ncclAllGather + the two-stream fork/join were captured
    ra, rb = plain.read(), eng.read()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    ea, eb = plain.eval(), eng.eval_global()
    assert ea == eb
    eng.comm_barrier()
    tm = eng.timing()
    assert tm["iterations"] == 12 + 45


# ---- BASELINE.json configs 1-3 end to end, bit for bit ---------------------------------------------------------

def _run_ba_recorded(engine, state, opts, n_iters):
    from gbp_poplar_amd import driver
    from tests.traj_util import EvalAt, wanted
    w = EvalAt(engine, wanted(n_iters))
    t = driver.run_ba(w, state, opts, n_iters=n_iters, eval_every=0)
    return t[0], w.array()


def _check_against_golden_trajectory(rows, initial, gold, gold_initial, end_to_end_tol):
    """SURVEY 8c tolerances, literally, against the reference-math trajectory (libm trig, slot-order sums):
    initial error and <= 3 sweeps within 1e-4; end to end = mean over the last 50 iterations within `end_to_end_tol`
    (None: chaotic input, band check by the caller)."""
    assert abs(initial[1] - gold_initial[0]) <= 1e-5 * gold_initial[0]
    assert np.array_equal(rows[:, 0], gold[:, 0])
    for k in range(3):
        assert abs(rows[k, 1] - gold[k, 1]) <= 1e-4 * gold[k, 1], (k, rows[k, 1], gold[k, 1])
        assert abs(rows[k, 3] - gold[k, 3]) <= 1e-4 * gold[k, 3], (k, rows[k, 3], gold[k, 3])
        assert rows[k, 5] == gold[k, 5] and rows[k, 6] == gold[k, 6]
    if end_to_end_tol is not None:
        for col in (1, 3):              # mean reprojection error, RMSE
            a, b = rows[-50:, col].mean(), gold[-50:, col].mean()
            assert abs(a - b) <= end_to_end_tol * b, (col, a, b)


def test_config1_fr1xyz_1500_sweeps_bit_exact(oracle_mod):
    """`./ba fr1xyz` defaults (1500 sweeps).  fr1xyz is chaotic in fp32 — ulp-level differences blow up within ~25
    sweeps — so equality of every belief after 1500 sweeps with ~1.5 M relinearisations is the strongest
    parity statement available; against the reference-math golden trajectory the first sweeps agree to 1e-4 and the
    final error sits in the converged band of BASELINE.md (end-to-end 1e-4 is not defined on a chaotic input)."""
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, _ = _setup(_bal("fr1xyz"), oracle_mod, sum_order=1, hooks=False)
        ig, tg = _run_ba_recorded(eng, state, opts, 1500)
        io, to = _run_ba_recorded(orc, state, opts, 1500)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    assert np.array_equal(tg[:, [0, 4, 5, 6]], to[:, [0, 4, 5, 6]])
    assert np.max(np.abs(tg[:, 1] - to[:, 1]) / to[:, 1]) <= 1e-5      # the metric's own trig: device vs glibc
    gold = _golden("trajectories.npz")
    _check_against_golden_trajectory(tg, ig, gold["ba_fr1xyz"], gold["ba_fr1xyz_initial"], None)
    assert 1.40 < tg[-1, 1] < 1.50, tg[-1]          # converged runs sit at 1.42-1.47 px
    assert 1.42 < gold["ba_fr1xyz"][-1, 1] < 1.47


@pytest.mark.parametrize("name,band", [("fr1desk", (1.2, 1.8)), ("fr2robot2", (0.86, 0.89))])
def test_other_sequences_1500_sweeps_bit_exact(name, band, oracle_mod):
    """The two other shipped sequences through the full default `./ba` run (1500 sweeps), bit for bit against the
    oracle in device conventions; fr2robot2 (well conditioned) also END TO END against the reference-math golden
    trajectory: mean reprojection error and RMSE averaged over the last 50 iterations within 2e-4 (SURVEY 8c asks 1e-3)."""
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, _ = _setup(_bal(name), oracle_mod, sum_order=1, hooks=False)
        ig, tg = _run_ba_recorded(eng, state, opts, 1500)
        io, to = _run_ba_recorded(orc, state, opts, 1500)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    assert np.array_equal(tg[:, [0, 4, 5, 6]], to[:, [0, 4, 5, 6]])
    assert band[0] < tg[-1, 1] < band[1], tg[-1]
    if name == "fr2robot2":
        gold = _golden("trajectories.npz")
        _check_against_golden_trajectory(tg, ig, gold["ba_fr2robot2"], gold["ba_fr2robot2_initial"], 2e-4)   # measured 6e-5


def test_config3_slam_fr2robot2_full_run_bit_exact(oracle_mod):
    """`./slam fr2robot2` defaults (700 sweeps per keyframe, 13 299 sweeps, 18 keyframe insertions): bit for bit
    against the oracle in device conventions, and end to end against the reference-math golden trajectory: first
    sweeps 1e-4, mean error / RMSE over the last 50 iterations within 2e-4 (SURVEY 8c asks 1e-3)."""
    from gbp_poplar_amd import driver, hostlib
    from tests.traj_util import EvalAt, wanted
    bal = _bal("fr2robot2")
    n_total = (bal["n_cams"] - 1) * 700 - 1
    oracle_mod.set_trig_mode(1)
    try:
        eng, orc, opts, state, extra = _setup(bal, oracle_mod, slam=True, sum_order=1, hooks=False)
        wg, wo = (EvalAt(x, wanted(n_total, head=30, every=700, tail=50)) for x in (eng, orc))
        ig = driver.run_slam(wg, hostlib, bal, state, extra, opts, eval_every=0)[0]
        driver.run_slam(wo, hostlib, bal, state, extra, opts, eval_every=0)
    finally:
        oracle_mod.set_trig_mode(0)
    g, o = eng.read(), orc.read()
    for k in g:
        assert np.array_equal(g[k], o[k]), k
    tg, to = wg.array(), wo.array()
    assert np.array_equal(tg[:, [0, 4, 5, 6]], to[:, [0, 4, 5, 6]])
    gold = _golden("trajectories.npz")
    _check_against_golden_trajectory(tg, ig, gold["slam_fr2robot2"], gold["slam_fr2robot2_initial"], 2e-4)   # measured 5e-5


def test_iterations_captured_into_a_callers_graph_use_the_two_kernel_path(oracle_mod):
    """the persistent kernel's barrier targets are launch arguments computed by the host, so a launch replayed from
    a graph would find its barriers already passed.  While the stream a caller handed over (gbp_set_stream) is being captured,
    gbp_iterate therefore queues plain k_sweep / k_beliefs launches: the caller's graph replays to the same state as the
    persistent path reaches."""
    import torch
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine
    bal = _bal("fr2robot2")
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)

    def make():
        e = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        e.upload(state)
        e.linearise()
        e.iterate(3)
        e.sync()
        return e

    ref, eng = make(), make()
    assert eng.graph_state() == 2                      # small graph: bursts normally run inside k_persist
    ref.iterate(12)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        eng.iterate(4)
    with torch.cuda.stream(stream):                    # (CUDAGraph.replay launches on torch's CURRENT stream, whatever stream captured it)
        for _ in range(3):
            graph.replay()
    stream.synchronize()                               # the caller's work on the caller's stream is the caller's to wait for: gbp_read
    eng.set_stream(0)                                  # orders against the ctx's stream only (it no longer goes through the NULL stream)
    g, o = eng.read(), ref.read()
    for k in g:
        assert np.array_equal(g[k], o[k], equal_nan=True), k
    eng.iterate(5)                                     # and the ctx is back on its own stream and path afterwards
    ref.iterate(5)
    g, o = eng.read(), ref.read()
    for k in g:
        assert np.array_equal(g[k], o[k], equal_nan=True), k


def test_capture_begun_with_bursts_in_flight_is_refused_not_broken(oracle_mod):
    """a caller who begins capturing their stream while k_persist bursts of the ctx are still unvalidated must get
    GBP_ERR_STATE ("gbp_sync before beginning a stream capture") from the next call — the library never synchronises a capturing
    stream, so the caller's capture stays valid, and after gbp_sync the same sequence works."""
    import torch
    from gbp_poplar_amd import driver, hostlib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal = _bal("fr2robot2")
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    ref = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    stream = torch.cuda.Stream()
    for e in (eng, ref):
        e.upload(state)
        e.linearise()
    eng.set_stream(stream.cuda_stream)
    assert eng.graph_state() == 2
    eng.iterate(6)                                     # a k_persist burst on the caller's stream, not yet validated
    ref.iterate(6)
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(8, device="cuda")
    with torch.cuda.graph(graph, stream=stream):
        x += 1                                         # (something of the caller's own in the capture)
        with pytest.raises(GbpError, match="gbp_sync before beginning a stream capture"):
            eng.iterate(1)
        with pytest.raises(GbpError, match="gbp_sync before beginning a stream capture"):
            eng.weaken_priors()
    graph.replay()                                     # the capture ended cleanly (an invalidated one raises at its end)
    stream.synchronize()
    assert float(x.sum()) == 8.0
    eng.sync()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=stream):
        eng.iterate(2)
    with torch.cuda.stream(stream):                    # (replay launches on torch's current stream)
        graph2.replay()
    stream.synchronize()
    eng.set_stream(0)
    ref.iterate(2)
    g, o = eng.read(), ref.read()
    for k in g:
        assert np.array_equal(g[k], o[k], equal_nan=True), k
