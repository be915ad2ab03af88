"""The split memory image of the landmark messages (gbp_kernels.h): LMSG holds the message alone — 12 floats = 3 float4 per factor in
device order — and the factor's scalar state lives in three planes by device position (FST_PACKED, FST_DAMP, FST_VAR).  The register
image of a factor did not change, so every case compares the whole state with the oracle bit for bit (beliefs, both message sets,
damping, damping_count, robust_flag), on the two-kernel path and on the path the library picks:
  1. a graph whose cameras are one 16-lane row and whose tiles hold pads: sweeps from the upload, bursts, LINEARISE under live messages
  2. every landmark at 12 and at 18 observations: the second batch of gathers (slots 10..14) and the slots beyond the index record
  3. the state paths: upload of non-default scalars, read() behind relinearising sweeps, NEW_KEYFRAME from host and from device
     arrays, the counters of eval()
  4. the literal per-factor mu tensors (the sweep then reads the variance plane every time)
  5. the instantiation that skips all-pad segments (liveness per float4 of the 3 KiB message block)
  6. without a GPU: the address maps (tile float4 index <-> record, piece; LDS slot; segment liveness) through the test hooks
"""
import numpy as np
import pytest

from tests.conftest import small_synth
from tests.test_gpu_parity import _assert_state_equal, _bal, _run_to_relin, _setup, _sync_potentials, _tiny_problem

gpu = pytest.mark.gpu

# two-kernel path / whatever the library chooses (on the small graphs below: bursts of >= 2 iterations inside the persistent kernel)
PATHS = [pytest.param({"persistent": -1}, id="two_kernels"), pytest.param({}, id="library_choice")]


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


def _equal(eng, orc):
    _assert_state_equal(eng, orc)
    assert np.array_equal(eng.read()["robust_flag"], orc.read()["robust_flag"])


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("params", PATHS)
def test_rows_of_one_camera_and_tiles_with_pads(params, oracle_mod, rounded_trig):
    bal = small_synth(9, 40, 3)
    from gbp_poplar_amd import hostlib
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    pos_edge = np.asarray(lay["pos_edge"])
    assert np.any(pos_edge == 0xFFFFFFFF) and lay["n_rows"] <= 2 * bal["n_cams"] and lay["n_tiles"] < bal["n_cams"]      # pads; cameras of one or two rows, several to a tile
    eng, orc = _start(bal, oracle_mod, **params)
    _equal(eng, orc)
    for _ in range(3):                                   # sweeps 1, 2, 3 from the upload's zero messages
        _both(eng, orc, "iterate", 1)
        _equal(eng, orc)
    _both(eng, orc, "iterate", 3)
    _equal(eng, orc)
    _both(eng, orc, "iterate", 2)
    _equal(eng, orc)
    _both(eng, orc, "linearise")                         # reads the variance plane, rewrites the robust flag in the packed plane
    _equal(eng, orc)
    _both(eng, orc, "iterate", 2)
    _equal(eng, orc)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("params", PATHS)
@pytest.mark.parametrize("degree", [12, 18])
def test_landmark_degrees_on_every_gather_path(degree, params, oracle_mod):
    """every landmark seen by all `degree` cameras: 12 takes the second batch of gathers (slots 10..14), 18 the slots behind the
    fifteen of the index record (lmk_fpos); 70 landmarks are more than the 64 of one workgroup of the belief kernel"""
    n_lmks = 70
    cam_id = np.repeat(np.arange(degree), n_lmks)
    lmk_id = np.tile(np.arange(n_lmks), degree)
    bal = _tiny_problem(cam_id.tolist(), lmk_id.tolist(), degree, n_lmks)
    assert np.all(np.bincount(bal["lmk_id"], minlength=n_lmks) == degree)
    eng, orc = _start(bal, oracle_mod, **params)
    for _ in range(3):
        _both(eng, orc, "iterate", 1)
        _equal(eng, orc)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("params", PATHS)
def test_upload_of_non_default_scalars(params, oracle_mod):
    bal = small_synth(9, 40, 3)
    from gbp_poplar_amd import driver, hostlib
    _, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    rng = np.random.default_rng(3)
    E = len(bal["cam_id"])
    state = dict(state, damping=rng.uniform(0.0, 0.5, E).astype(np.float32),
                 damping_count=rng.choice(np.array([-15, -4, 0, 1], np.int32), E).astype(np.int32),
                 active_flag=(rng.uniform(size=E) < 0.8).astype(np.uint32))
    assert 0 < state["active_flag"].sum() < E
    eng, orc, *_ = _setup(bal, oracle_mod, sum_order=1, **params)
    _both(eng, orc, "upload", state)
    g = eng.read()
    assert np.array_equal(g["damping"], state["damping"]) and np.array_equal(g["damping_count"], state["damping_count"])
    _both(eng, orc, "linearise")
    _sync_potentials(eng, orc)
    _equal(eng, orc)
    _both(eng, orc, "iterate", 1)
    _equal(eng, orc)
    _both(eng, orc, "iterate", 2)
    _equal(eng, orc)
    g, o = eng.eval(), orc.eval()
    assert g["n_active"] == o["n_active"] == int(state["active_flag"].sum())


@gpu
def test_read_and_eval_counters_behind_relinearising_sweeps(oracle_mod, rounded_trig):
    """fr1xyz through its first relinearising sweeps: the damping plane is rewritten (0 at the relinearisation), the packed plane carries
    the new counts and robust flags, the variance plane is read by the relinearising lanes; read() from host and device arrays, and the
    counters of eval()"""
    eng, orc, *_ = _setup(_bal("fr1xyz"), oracle_mod, sum_order=1, persistent=-1)
    _run_to_relin(eng, orc)
    _equal(eng, orc)
    n_relin = 0
    for _ in range(3):
        _both(eng, orc, "iterate", 1)
        n_relin += int(np.sum(orc.read()["damping_count"] == -8))
        _equal(eng, orc)
        g, o = eng.eval(), orc.eval()
        for k in ("n_active", "n_relin", "n_robust"):
            assert g[k] == o[k], k
    assert n_relin > 0 and np.any(orc.read()["robust_flag"] != 0)
    o = orc.read()
    d = eng.read(device=True)
    eng.sync()
    for k in ("damping", "damping_count", "robust_flag"):
        assert np.array_equal(d[k].cpu().numpy().astype(o[k].dtype), o[k]), k


@gpu
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host_arrays", "device_arrays"])
@pytest.mark.parametrize("params", PATHS)
def test_keyframe_edits_the_packed_plane(params, device_arrays, oracle_mod):
    bal = small_synth(9, 40, 3)
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
    _equal(eng, orc)
    upd = {"damping_count": np.full(asleep.size, -15, np.int32), "active_flag": np.ones(asleep.size, np.uint32)}
    orc.new_keyframe(upd)
    if device_arrays:
        import torch
        dev = eng.device()
        eng.new_keyframe({"damping_count": torch.from_numpy(upd["damping_count"]).to(dev),
                          "active_flag": torch.from_numpy(upd["active_flag"].astype(np.int32)).to(dev)})
    else:
        eng.new_keyframe(upd)
    _both(eng, orc, "iterate", 1)
    _equal(eng, orc)
    _both(eng, orc, "iterate", 2)
    _equal(eng, orc)
    g, o = eng.eval(), orc.eval()
    assert g["n_active"] == o["n_active"] == asleep.size


# ---- 4 ----------------------------------------------------------------------------------------------------------------
@gpu
def test_literal_per_factor_mu(oracle_mod):
    eng, orc = _start(small_synth(9, 40, 3), oracle_mod, per_factor_mu=1)
    for _ in range(3):
        _both(eng, orc, "iterate", 1)
        _equal(eng, orc)


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@gpu
def test_segment_skipping_sweep(oracle_mod):
    """2 304 cameras of ~61 factors: the sweep moves its tiles through per-tile buffer descriptors and skips the all-pad segments —
    twelve float4 of the message block each"""
    from gbp_poplar_amd import hostlib
    bal = hostlib.synth_generate(2304, 14000, 10, 7)
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    pads = 4 * int(np.sum(np.all(np.asarray(lay["pos_edge"]).reshape(-1, 4) == 0xFFFFFFFF, axis=1)))      # positions in all-pad segments
    assert lay["n_tiles"] >= 2048 and pads * 100 >= lay["Ep"], (lay["n_tiles"], pads, lay["Ep"])      # what gbp_create asks for
    eng, orc = _start(bal, oracle_mod, persistent=-1)
    for n in (1, 1, 2):
        _both(eng, orc, "iterate", n)
        _equal(eng, orc)


# ---- 6: the address maps, on the host -----------------------------------------------------------------------------------
def _layout_with_pads():
    from gbp_poplar_amd import hostlib
    bal = hostlib.synth_generate(40, 600, 5, 3)
    return hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])


def _maps():
    m = np.asarray(_layout_with_pads()["lmsg_maps"], np.int64).reshape(-1, 4)
    return 3, m.shape[0], m


def test_tile_index_maps_are_a_bijection():
    g, n, m = _maps()
    assert (g, n) == (3, 192)                              # 12 floats per message, 64 messages: 3 KiB
    rec, piece, back, slot = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    assert np.array_equal(back, np.arange(n))             # (record, piece) -> float4 index inverts float4 index -> (record, piece)
    assert rec.min() == 0 and rec.max() == 63 and piece.min() == 0 and piece.max() == g - 1
    assert len({(r, q) for r, q in zip(rec.tolist(), piece.tolist())}) == n      # every piece of every record exactly once
    assert sorted(slot.tolist()) == list(range(n))        # the LDS stage: every slot exactly once, none beyond the 3 KiB
    # a message is contiguous in memory: float 0..2 eta, 3..11 Lambda — pieces 0, 1, 2 of record r are the float4 3r, 3r + 1, 3r + 2
    assert np.array_equal(np.arange(n) // g, rec) and np.array_equal(np.arange(n) % g, piece)


def test_lds_stage_is_free_of_bank_conflicts():
    """ds_read_b128 serves 16 lanes at a time out of 64 dword banks, ds_write_b128 8 lanes out of 32 (the rule the sweep's stage has
    always been laid out by): a group is conflict-free when its lanes' float4 start in distinct banks modulo the group's bank count.
    Checked for contiguous groups of 16 and for the groups of 16 the hardware forms for the 16-byte read.
    Both sides of the transpose: record order (lane r, piece q of record r) and tile order (access k, float4 64 k + lane)."""
    g, n, m = _maps()
    slot_of = {(int(r), int(q)): int(s) for r, q, s in m[:, [0, 1, 3]]}

    # the lanes ds_read_b128 serves together on gfx950: four groups of 16, not contiguous
    hw_read_groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    hw_read_groups += [[l + 32 for l in grp] for grp in hw_read_groups]
    assert sorted(sum(hw_read_groups, [])) == list(range(64))

    def check(slots_of_wave):
        s = np.asarray(slots_of_wave) * 4                 # first dword of each lane's float4
        groups = [(list(range(g0, g0 + 16)), 64) for g0 in range(0, 64, 16)] + [(grp, 64) for grp in hw_read_groups]
        groups += [(list(range(g0, g0 + 8)), 32) for g0 in range(0, 64, 8)]
        for lanes, banks in groups:
            b = (s[lanes] % banks) // 4                   # a 16-byte access covers 4 consecutive banks: distinct multiples of 4
            assert len(set(b.tolist())) == len(lanes), (lanes, b)

    for q in range(g):                                    # record order, reads and writes
        check([slot_of[(lane, q)] for lane in range(64)])
    for k in range(g):                                    # tile order
        check([int(m[64 * k + lane, 3]) for lane in range(64)])


def test_segment_liveness_agrees_with_the_device_order():
    """bit s of a tile's mask = lanes 4s .. 4s + 3 hold a factor (what gbp_create derives from pos_edge): a float4 of the message block
    is live exactly when the record it belongs to lies in such a segment — on a layout that has all-pad segments"""
    lay = _layout_with_pads()
    seg_has_factor = np.any(np.asarray(lay["pos_edge"]).reshape(-1, 16, 4) != 0xFFFFFFFF, axis=2)      # [tile][segment]
    assert np.any(~seg_has_factor) and np.any(seg_has_factor)
    assert len({tuple(t) for t in seg_has_factor.tolist()}) > 1                                        # more than one mask
    rec = np.asarray(lay["lmsg_maps"], np.int64).reshape(-1, 4)[:, 0]
    live = np.asarray(lay["lmsg_live"]).reshape(lay["n_tiles"], -1)
    assert live.shape[1] == rec.size == 192
    assert np.array_equal(live != 0, seg_has_factor[:, rec // 4])
    # a dead segment's twelve float4 are contiguous: nothing of a live record is skipped, nothing of a dead one is moved
    assert np.array_equal(live.reshape(lay["n_tiles"], 16, 12) != 0, np.repeat(seg_has_factor[:, :, None], 12, axis=2))
