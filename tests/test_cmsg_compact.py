"""The compact camera-message record (CMSG: eta 6, the 3x3 inverse Bi 9, a format word; gbp_kernels.h).

A factor's message to its camera is carried from sweep to sweep as eta + Bi; the 21 lower-triangle entries of its Lambda are re-derived
from the potential and Bi by the loops that produced them.  Every state in which a record is NOT "Lambda = f(FAC, Bi)" has a case
here; each compares beliefs, BOTH message sets (the camera message through the hook that hands out the reference's 27 floats) and
the per-factor scalars with the oracle in the device's conventions, bit for bit:
  (a) sweeps 1, 2, 3 from zero messages                                        format 0 -> 1
  (b) through the first relinearising sweeps of fr1xyz                         the message of the potential as it was BEFORE the sweep rewrote it
  (c) NEW_KEYFRAME activates factors in the middle of a run                    format 0 records beside format 1 in one tile
  (d) LINEARISE under live messages, then more sweeps                          format 2 (literal, side array) and the way back to 1
  (e) the same bursts on the two-kernel path and on the path the library picks (the persistent kernel on these graphs), and one
      recovered time-out of the persistent kernel                              its prologue / last iteration / snapshot speak the same format
  (f) a graph above 2 048 tiles of many small cameras                          the instantiation that skips all-pad segments (buffer loads / stores)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import seq_path, small_synth
from tests.test_gpu_parity import _assert_state_equal, _bal, _run_to_relin, _setup, _sync_potentials

pytestmark = pytest.mark.gpu

# two-kernel path / whatever the library chooses (on the graphs below: bursts of >= 2 iterations inside the persistent kernel)
PATHS = [pytest.param({"persistent": -1}, id="two_kernels"), pytest.param({}, id="library_choice")]


def _small():
    return small_synth(n_cams=9, n_lmks=40, obs=3)


@pytest.fixture
def rounded_trig(oracle_mod):
    """the oracle's sin / cos correctly rounded, as the kernels compute them: relinearised potentials are then equal bit for bit"""
    oracle_mod.set_trig_mode(1)
    yield
    oracle_mod.set_trig_mode(0)


def _both(eng, orc, verb, *a):
    getattr(eng, verb)(*a)
    getattr(orc, verb)(*a)


def _start(bal, oracle_mod, **params):
    eng, orc, *_ = _setup(bal, oracle_mod, sum_order=1, **params)
    _both(eng, orc, "linearise")
    _sync_potentials(eng, orc)
    return eng, orc


def _potentials_equal(eng, orc):
    (ge, gl), (oe, ol) = eng.factor_potentials(), orc.factor_potentials()
    assert np.array_equal(ge, oe) and np.array_equal(gl, ol)


def test_first_sweeps_from_zero_messages(oracle_mod):
    """(a) the zero fill of the upload is format 0; the first sweep must read it as a zero message (NOT as f(FAC, Bi = 0), which is
    Lambda_cc) and leave format 1, which sweeps 2 and 3 re-derive."""
    eng, orc = _start(_small(), oracle_mod, persistent=-1)
    _assert_state_equal(eng, orc)                   # the hook on format-0 records
    for _ in range(3):
        _both(eng, orc, "iterate", 1)
        _assert_state_equal(eng, orc)
    assert np.any(eng.messages()["cam_lambda"] != 0)


def test_relinearising_sweeps_rederive_from_the_old_potential(oracle_mod, rounded_trig):
    """(b) a sweep that relinearises rewrites FAC; the message it read was produced by the potential as loaded."""
    eng, orc, *_ = _setup(_bal("fr1xyz"), oracle_mod, sum_order=1, persistent=-1)
    _run_to_relin(eng, orc)
    _assert_state_equal(eng, orc)
    n_relin = 0
    for _ in range(3):                                   # the first relinearising sweep and two beyond it
        _both(eng, orc, "iterate", 1)
        n_relin += int(np.sum(orc.read()["damping_count"] == -8))
        _potentials_equal(eng, orc)
        _assert_state_equal(eng, orc)
    assert n_relin > 0


@pytest.mark.parametrize("params", PATHS)
def test_keyframe_activates_factors_beside_live_ones(params, oracle_mod):
    """(c) the factors of cameras 6..8 sleep through five sweeps (their records stay format 0 while their neighbours' are format 1:
    a camera of this graph is one 16-lane row, a tile holds four), NEW_KEYFRAME wakes them, five more sweeps."""
    bal = _small()
    from gbp_poplar_amd import driver, hostlib
    _, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    asleep = np.asarray(bal["cam_id"]) >= 6
    assert 0 < asleep.sum() < asleep.size
    eng, orc, *_ = _setup(bal, oracle_mod, sum_order=1, **params)
    state = dict(state, active_flag=np.where(asleep, 0, 1).astype(np.uint32))
    _both(eng, orc, "upload", state)
    _both(eng, orc, "linearise")
    _sync_potentials(eng, orc)
    _both(eng, orc, "iterate", 3)
    _both(eng, orc, "iterate", 2)
    _assert_state_equal(eng, orc)
    upd = {"damping_count": np.full(asleep.size, -15, np.int32), "active_flag": np.ones(asleep.size, np.uint32)}
    _both(eng, orc, "new_keyframe", upd)
    _both(eng, orc, "iterate", 1)
    _assert_state_equal(eng, orc)
    _both(eng, orc, "iterate", 4)
    _assert_state_equal(eng, orc)
    lam = eng.messages()["cam_lambda"].reshape(-1, 36)
    assert np.all(np.any(lam != 0, axis=1))


@pytest.mark.parametrize("params", PATHS)
def test_linearise_under_live_messages(params, oracle_mod, rounded_trig):
    """(d), (e) bursts of 3 + 2 sweeps, then LINEARISE: the potentials change under live messages, so every derived record becomes
    literal (format 2) — read back by the hook, by the next burst (the sweep, or the prologue of the persistent kernel), which
    returns the records to format 1 for the burst after it."""
    eng, orc = _start(_small(), oracle_mod, **params)
    if not params:
        assert eng.graph_state() == 2, eng.last_error()
    _both(eng, orc, "iterate", 3)
    _assert_state_equal(eng, orc)
    _both(eng, orc, "iterate", 2)
    _assert_state_equal(eng, orc)
    before = eng.factor_potentials()[1].copy()
    _both(eng, orc, "linearise")
    assert not np.array_equal(before, eng.factor_potentials()[1])
    _potentials_equal(eng, orc)
    _assert_state_equal(eng, orc)                   # the hook on format-2 records
    _both(eng, orc, "iterate", 2)
    _assert_state_equal(eng, orc)
    _both(eng, orc, "iterate", 3)
    _assert_state_equal(eng, orc)
    _both(eng, orc, "linearise")                    # a second time: the side array exists, a captured graph was dropped for it
    _both(eng, orc, "iterate", 1)
    _potentials_equal(eng, orc)
    _assert_state_equal(eng, orc)


_RECOVERY_CODE = """
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from gbp_poplar_amd import _cabi, driver, hostlib
from gbp_poplar_amd.engine import GbpEngine
from oracle import oracle as om
from tests.test_gpu_parity import _assert_state_equal, _sync_potentials
om.load("restatement")
bal = hostlib.bal_read(%(seq)r)
K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
eng = GbpEngine(bal['cam_id'], bal['lmk_id'], bal['n_cams'], bal['n_lmks'], K, hooks='exp', params=_cabi.GbpParams.defaults(persistent=1))
orc = om.Oracle(bal['cam_id'], bal['lmk_id'], bal['n_cams'], bal['n_lmks'], K)
orc.set_sum_order(1)
for e in (eng, orc):
    e.upload(state); e.linearise()
_sync_potentials(eng, orc)
for e in (eng, orc):
    e.iterate(1)                                     # two kernels: format-1 records in the snapshot the recovery restores
assert eng.graph_state() == 2, eng.last_error()
for e in (eng, orc):
    e.iterate(6)                                     # the launch that times out; undone and replayed on the two-kernel path
eng.sync()
assert eng.graph_state() != 2, 'the ctx should have left the persistent path'
_assert_state_equal(eng, orc)
for e in (eng, orc):
    e.iterate(2)
_assert_state_equal(eng, orc)
print('RECOVERED :: %%s' %% eng.last_error())
"""


def test_persistent_kernel_time_out_recovery_keeps_the_format():
    """(e) one launch of the persistent kernel whose workgroups cannot all be resident (the placement switch of the experiments build,
    as in test_persistent_kernel_time_out_is_recovered): the snapshot it is undone from holds format-1 records, the two-kernel replay
    reads them."""
    from gbp_poplar_amd import _lib
    assert os.path.exists(_lib.EXP_LIB_PATH), "experiments build absent (python -m gbp_poplar_amd.build --experiments)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _RECOVERY_CODE % {"root": root, "seq": seq_path("fr1xyz")}
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GBP_PERSIST_SPREAD="8"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RECOVERED")][-1]
    assert "warning:" in line and "timed out" in line, line


def test_segment_skipping_sweep_on_many_small_cameras(oracle_mod):
    """(f) 2 304 cameras of ~61 factors: above 2 048 tiles, the unused tails of the cameras' last rows above 1 % of the positions — the
    shape on which the sweep moves its tiles through per-tile buffer descriptors and skips the all-pad segments.  A skipped segment
    reads as zeros: format 0."""
    from gbp_poplar_amd import hostlib
    bal = hostlib.synth_generate(2304, 14000, 10, 7)
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    pads = 4 * int(np.sum(np.all(np.asarray(lay["pos_edge"]).reshape(-1, 4) == 0xFFFFFFFF, axis=1)))      # positions in all-pad segments
    assert lay["n_tiles"] >= 2048 and pads * 100 >= lay["Ep"], (lay["n_tiles"], pads, lay["Ep"])      # what gbp_create asks for
    eng, orc = _start(bal, oracle_mod, persistent=-1)
    for n in (1, 1, 2):
        _both(eng, orc, "iterate", n)
        _assert_state_equal(eng, orc)
