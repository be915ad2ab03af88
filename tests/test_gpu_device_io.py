"""Device-resident arrays (include/gbp_mi355x.h): gbp_upload / gbp_read / gbp_read_priors / gbp_new_keyframe with DEVICE pointers —
torch tensors on the engine's GPU through GbpEngine — against the host-array forms of the same calls and against the CPU oracle in the
device's conventions (row-tree camera sums, correctly rounded trig: the set-up of tests/test_gpu_parity.py).  Every comparison is exact:
both sides run the same device arithmetic on the same bits."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import seq_path, small_synth

pytestmark = pytest.mark.gpu

BELIEFS = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda")
STATE = BELIEFS + ("damping", "damping_count", "robust_flag")


def _bal(name):
    from gbp_poplar_amd import hostlib
    if name == "synth_2048_tiles":
        return small_synth(n_cams=64, n_lmks=22000, obs=6, seed=5)      # 132 000 factors: >= 2 048 tiles of 64 positions
    return hostlib.bal_read(seq_path(name))


def _inputs(bal, slam=False):
    from gbp_poplar_amd import driver, hostlib
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=slam)
    return K, state, extra, opts


def _engine(bal, K, hooks=False, **params):
    from gbp_poplar_amd import _cabi
    from gbp_poplar_amd.engine import GbpEngine
    return GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**params), hooks=hooks)


def _t(a, offset=False):
    """numpy array -> torch tensor on the GPU, same bits (uint32 flags as int32); offset: a view that starts 4 bytes into a larger buffer"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy())
    if not offset:
        return t.cuda()
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = big[1:]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dev(d, offset=False):
    return {k: _t(v, offset) for k, v in d.items() if v is not None}


def _np(d):
    out = {}
    for k, v in d.items():
        a = v.cpu().numpy()
        out[k] = a.view(np.uint32) if k.endswith("_flag") else a
    return out


def _equal(a, b, keys=None, what=""):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _loop(e, n, steps, i0=0):
    """passes i0 .. i0 + n - 1 of the default flow: weakening where the reference's loop weakens, then the iteration"""
    if hasattr(e, "ba_loop"):
        e.ba_loop(n, i0, steps, metrics=False)
        return
    for i in range(i0, i0 + n):
        if (i + 1) % 2 == 0 and i < 2 * steps:
            e.weaken_priors()
        e.iterate(1)


def _oracle_run(oracle_mod, bal, K, state, steps, n=30):
    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        orc.upload(state)
        orc.linearise()
        _loop(orc, n, steps)
        return orc.read()
    finally:
        oracle_mod.set_trig_mode(0)


@pytest.mark.parametrize("name", ["fr1xyz", "fr2robot2", "synth_2048_tiles"])
def test_device_upload_and_read_equal_the_oracle_and_the_host_path(name, oracle_mod):
    """upload(device tensors) -> linearise -> the default flow's first 30 passes -> read(device=True): every belief, damping,
    damping_count and robust_flag equals the oracle and the host-array run on a second ctx."""
    bal = _bal(name)
    K, state, _, opts = _inputs(bal)
    steps = int(opts.steps)
    d, h = _engine(bal, K), _engine(bal, K)
    if name == "synth_2048_tiles":
        assert d.timing()["device_bytes_allocated"] > 0 and (bal["n_edges"] + 63) // 64 >= 2048
    d.upload(_dev(state))
    h.upload(state)
    for e in (d, h):
        e.linearise()
        _loop(e, 30, steps)
    out = d.read(device=True)
    d.sync()
    g, hh = _np(out), h.read()
    _equal(g, hh, STATE, "host path")
    _equal(g, _oracle_run(oracle_mod, bal, K, state, steps), STATE, "oracle")
    # ... and the host-array read of the device-uploaded ctx, the device read of the host-uploaded one, READ_PRIORS both ways
    _equal(d.read(), hh, STATE, "host read of the device-uploaded ctx")
    o2 = h.read(device=True)
    p2 = h.read_priors(device=True)
    h.sync()
    _equal(_np(o2), hh, STATE, "device read of the host-uploaded ctx")
    _equal(_np(p2), d.read_priors(), None, "priors")


@pytest.mark.parametrize("case", ["hoisted", "per_factor_mu", "null_optionals", "non_default_parameters"])
def test_internal_state_after_a_device_upload_equals_the_host_upload(case):
    """factor potentials, messages and mu (test hooks) after upload + linearise + 3 iterations, device arrays against host arrays"""
    bal = _bal("fr2robot2")
    K, state, _, opts = _inputs(bal)
    kw = {}
    if case == "per_factor_mu":
        kw = {"per_factor_mu": 1}
        rng = np.random.default_rng(3)
        state["oldmu"] = (rng.standard_normal(9 * bal["n_edges"]) * 1e-3).astype(np.float32)
        state["mu"] = state["oldmu"].copy()
        state["damping"] = rng.random(bal["n_edges"]).astype(np.float32) * 0.3
    elif case == "null_optionals":
        for k in ("damping", "damping_count", "cam_scaling", "lmk_scaling", "cam_weaken_flag", "lmk_weaken_flag"):
            state.pop(k, None)
    elif case == "non_default_parameters":
        kw = {"relin_mode": 1, "dmu_threshold": 3e-2, "maxeta_damping": 0.25, "nstds": 1.5, "per_factor_mu": 1}
    d, h = _engine(bal, K, hooks=True, **kw), _engine(bal, K, hooks=True, **kw)
    d.upload(_dev(state))
    h.upload(state)
    for step in range(2):
        for x, y in zip(d.factor_potentials() + d.mu(), h.factor_potentials() + h.mu()):
            assert np.array_equal(x, y), (case, step)
        md, mh = d.messages(), h.messages()
        _equal(md, mh, None, (case, step))
        _equal(d.read(), h.read(), STATE, (case, step))
        _equal(d.read_priors(), h.read_priors(), None, (case, step))
        for e in (d, h):
            e.linearise()
            e.iterate(3)


def test_mu_on_a_hoisted_ctx_is_the_callers_duty():
    """per_factor_mu = 0: the host path refuses a non-zero oldmu after looking at it; device arrays are not read back — the header
    makes zeros the caller's duty and says the members are not read: the upload succeeds and computes what a zero oldmu computes."""
    from gbp_poplar_amd.engine import GbpError
    bal = _bal("fr2robot2")
    K, state, _, _ = _inputs(bal)
    bad = dict(state, oldmu=np.ones(9 * bal["n_edges"], np.float32))
    d, h = _engine(bal, K), _engine(bal, K)
    with pytest.raises(GbpError, match="per_factor_mu"):
        h.upload(bad)
    h.upload(state)
    d.upload(_dev(bad))
    for e in (d, h):
        e.linearise()
        e.iterate(3)
    _equal(d.read(), h.read(), STATE)


class _DeviceSide:
    """an engine whose arrays stay on the GPU: what driver.run_slam hands to its host helper are CPU copies of the device reads, what it
    hands back goes up as device tensors"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def upload(self, state):
        self.e.upload(_dev(state))

    def read(self):
        out = self.e.read(device=True)
        self.e.sync()
        return _np(out)

    def read_priors(self):
        out = self.e.read_priors(device=True)
        self.e.sync()
        return _np(out)

    def new_keyframe(self, upd):
        self.e.new_keyframe(_dev(upd))


def test_slam_flow_device_side(oracle_mod):
    """read -> read_priors -> host helper on CPU copies -> new_keyframe over four keyframes of fr2robot2, device arrays throughout:
    identical to the host-array flow and to the oracle"""
    from gbp_poplar_amd import driver, hostlib
    bal = _bal("fr2robot2")
    K, state, extra, opts = _inputs(bal, slam=True)
    d, h = _engine(bal, K), _engine(bal, K)
    run = lambda e: driver.run_slam(e, hostlib, bal, state, extra, opts, iters_between_kfs=25, max_iters=110, eval_every=10)
    oracle_mod.set_trig_mode(1)
    try:
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        td, th, to = run(_DeviceSide(d)), run(h), run(orc)
        ro = orc.read()
    finally:
        oracle_mod.set_trig_mode(0)
    assert td == th and len(td) == len(to)
    rd, rh = d.read(), h.read()
    _equal(rd, rh, STATE, "host flow")
    _equal(rd, ro, STATE, "oracle")
    _equal(d.read_priors(), h.read_priors())
    # a host-array keyframe behind device-array ones (the host shadow of the active flags is read back first)
    upd = {"damping_count": np.full(bal["n_edges"], -15, np.int32), "active_flag": np.ones(bal["n_edges"], np.uint32)}
    for e in (d, h):
        e.new_keyframe(upd)
        e.iterate(3)
    _equal(d.read(), h.read(), STATE, "host keyframe behind device keyframes")


def test_calls_are_ordered_on_the_ctx_stream():
    """the inputs overwritten on the ctx's stream right behind upload; the outputs consumed by a torch op queued on that stream with
    no host synchronisation in between"""
    import torch
    bal = _bal("synth_2048_tiles")
    K, state, _, _ = _inputs(bal)
    d, h = _engine(bal, K), _engine(bal, K)
    s = torch.cuda.Stream()
    d.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev = _dev(state)
        d.upload(dev)
        for t in dev.values():
            t.fill_(7)
        d.linearise()
        d.iterate(5)
        out = d.read(device=True)
        doubled = {k: out[k] * 2 for k in BELIEFS}
        count1 = out["damping_count"] + 1
    s.synchronize()
    h.upload(state)
    h.linearise()
    h.iterate(5)
    hh = h.read()
    for k in BELIEFS:
        assert np.array_equal(doubled[k].cpu().numpy(), hh[k] * np.float32(2), equal_nan=True), k
    assert np.array_equal(count1.cpu().numpy(), hh["damping_count"] + 1)
    d.set_stream(None)


def test_views_with_only_four_byte_alignment():
    """every member a view that starts 4 bytes into a larger tensor, inputs and outputs"""
    import torch
    bal = _bal("fr2robot2")
    K, state, _, _ = _inputs(bal, slam=True)
    d, h = _engine(bal, K, hooks=True), _engine(bal, K, hooks=True)
    d.upload(_dev(state, offset=True))
    h.upload(state)
    for e in (d, h):
        e.linearise()
        e.iterate(4)
    hh, hp = h.read(), h.read_priors()
    mk = lambda ref: {k: torch.full((v.size + 1,), -1, dtype=torch.int32 if v.dtype != np.float32 else torch.float32, device="cuda")[1:] for k, v in ref.items()}
    out, pri = mk(hh), mk(hp)
    d.read(out=out)
    d.read_priors(out=pri)
    d.sync()
    _equal(_np(out), hh, STATE)
    _equal(_np(pri), hp)
    upd = dict(hp, damping_count=np.full(bal["n_edges"], -15, np.int32), active_flag=np.ones(bal["n_edges"], np.uint32),
               cam_weaken_flag=np.full(bal["n_cams"], 2, np.uint32), lmk_weaken_flag=np.full(bal["n_lmks"], 1, np.uint32))
    upd["cam_priors_eta"] = upd["cam_priors_eta"] * np.float32(1.5)
    d.new_keyframe(_dev(upd, offset=True))
    h.new_keyframe(upd)
    for e in (d, h):
        e.weaken_priors()
        e.iterate(3)
    _equal(d.read(), h.read(), STATE)
    _equal(d.read_priors(), h.read_priors())
    _equal(d.messages(), h.messages())


@pytest.mark.parametrize("path", ["persistent_kernel", "hipgraph"])
def test_device_read_between_bursts_leaves_the_next_burst_alone(path):
    import torch
    bal = _bal("fr1xyz")
    K, state, _, _ = _inputs(bal)
    kw = {"persistent": 1} if path == "persistent_kernel" else {"persistent": -1, "graph_unroll": 5}
    d, h = _engine(bal, K, **kw), _engine(bal, K, **kw)
    for e in (d, h):
        e.upload(state)
        e.linearise()
    seen = []
    for burst in range(3):
        d.iterate(10)
        h.iterate(10)
        out = d.read(device=True)
        pri = d.read_priors(device=True)
        seen.append((out, pri))
        assert d.graph_state() == (2 if path == "persistent_kernel" else 1)
    d.sync()
    _equal(_np(seen[-1][0]), h.read(), STATE)
    d.iterate(10)
    h.iterate(10)
    _equal(d.read(), h.read(), STATE)
    assert torch.equal(seen[0][1]["cam_priors_eta"], seen[-1][1]["cam_priors_eta"])


def _struct_upload(eng, members):
    """gbp_upload with a hand-made struct: addresses straight into the C-ABI (GbpEngine itself refuses a mix before the call)"""
    from gbp_poplar_amd import _cabi as cabi
    s = cabi.GbpStateIn()
    for name, ctype in s._fields_:
        if members.get(name) is not None:
            setattr(s, name, C.cast(C.c_void_p(members[name]), ctype))
    return eng.lib.gbp_upload(eng.h, C.byref(s))


def test_rejections_leave_the_ctx_untouched(oracle_mod):
    """GBP_ERR_INVALID with the member's name: a struct that mixes host and device members, device pointers on a
    partial landmark shard (and a tensor of another GPU where there is one); pinned host memory is host memory.  The ctx then runs
    the whole flow and equals the oracle."""
    import torch
    from gbp_poplar_amd.engine import GbpError
    bal = _bal("fr2robot2")
    K, state, _, opts = _inputs(bal)
    steps = int(opts.steps)
    d = _engine(bal, K)
    d.upload(state)
    d.linearise()
    d.iterate(2)
    before = d.read()
    dev = _dev(state)
    host = {k: np.ascontiguousarray(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in state.items()}
    mixed = {k: t.data_ptr() for k, t in dev.items()}
    mixed["meas_variances"] = host["meas_variances"].ctypes.data
    assert _struct_upload(d, mixed) == -1
    assert "meas_variances" in d.last_error() and "host" in d.last_error()
    mixed = {k: a.ctypes.data for k, a in host.items()}
    mixed["cam_priors_lambda"] = dev["cam_priors_lambda"].data_ptr()
    assert _struct_upload(d, mixed) == -1 and "cam_priors_lambda" in d.last_error()
    out = d.read(device=True)      # (a mixed read struct)
    s_out = {"cam_beliefs_eta": out["cam_beliefs_eta"], "damping": torch.zeros(bal["n_edges"])}
    with pytest.raises(TypeError, match="damping"):
        d.read(out=s_out)
    if torch.cuda.device_count() > 1:
        other = dict(dev, damping=dev["damping"].to("cuda:1"))
        with pytest.raises((TypeError, GbpError)):
            d.upload(other)
        assert _struct_upload(d, {k: t.data_ptr() for k, t in other.items()}) == -1 and "another GPU" in d.last_error()
    d.sync()
    _equal(d.read(), before, STATE, "after the refused calls")
    # pinned host memory is host memory: today's path
    pinned = {k: torch.from_numpy(a).pin_memory() for k, a in host.items()}
    assert _struct_upload(d, {k: t.data_ptr() for k, t in pinned.items()}) == 0
    d.upload(dev)
    d.linearise()
    _loop(d, 30, steps)
    _equal(d.read(), _oracle_run(oracle_mod, bal, K, state, steps), STATE, "oracle")
    # a partial landmark shard: out of scope, refused; its host path is what it was
    L = bal["n_lmks"]
    sh = _engine_shard(bal, K, (0, 2, 0, L // 2))
    sh.upload(state)
    ref = sh.read()
    with pytest.raises(GbpError, match="sharded"):
        sh.upload(dev)
    with pytest.raises(GbpError, match="sharded"):
        sh.read(device=True)
    _equal(sh.read(), ref, STATE, "shard")


def _engine_shard(bal, K, shard):
    from gbp_poplar_amd.engine import GbpEngine
    return GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=shard)


def test_example_device_loop_equals_the_host_array_loop():
    """examples/slam_device_loop.py: read(device=True) -> tensor arithmetic on the GPU -> new_keyframe, against the same loop on host arrays"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "slam_device_loop.py")
    spec = importlib.util.spec_from_file_location("slam_device_loop", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bal = _bal("fr2robot2")
    dev, host = mod.run(bal, True, keyframes=2, iters=10), mod.run(bal, False, keyframes=2, iters=10)
    assert dev == host and np.isfinite(dev[0])


def test_managed_memory_is_refused_by_name():
    """hipMallocManaged memory reports as device-accessible but is not device memory: GBP_ERR_INVALID naming the member, ctx untouched"""
    bal = _bal("fr2robot2")
    K, state, _, _ = _inputs(bal)
    d = _engine(bal, K)
    d.upload(state)
    d.linearise()
    d.iterate(2)
    before = d.read()
    host = {k: np.ascontiguousarray(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in state.items()}
    loaded = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l]      # the ONE HIP runtime of this process
    assert loaded
    hip = C.CDLL(loaded[0])
    hip.hipMallocManaged.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipFree.argtypes = [C.c_void_p]
    m = C.c_void_p()
    rc = hip.hipMallocManaged(C.byref(m), host["damping"].nbytes, 1)
    if rc != 0 or not m.value:
        pytest.skip("hipMallocManaged is not available here (status %d)" % rc)
    try:
        man = {k: a.ctypes.data for k, a in host.items()}
        man["damping"] = m.value
        assert _struct_upload(d, man) == -1
        assert "damping" in d.last_error() and "managed" in d.last_error()
        from gbp_poplar_amd import _cabi as cabi
        o = cabi.GbpStateOut()
        o.damping = C.cast(C.c_void_p(m.value), cabi.c_f32p)
        assert d.lib.gbp_read(d.h, C.byref(o)) == -1 and "managed" in d.last_error()
    finally:
        hip.hipFree(m)
    _equal(d.read(), before, STATE, "after the refused calls")


def test_oldmu_is_the_one_uploaded_when_mu_differs():
    """per_factor_mu = 1, device arrays with mu != oldmu: the host path refuses that after comparing the arrays; with device arrays
    equality is the caller's duty and the header says which one counts — oldmu.  The result equals a host upload of mu = oldmu."""
    from gbp_poplar_amd.engine import GbpError
    bal = _bal("fr2robot2")
    K, state, _, _ = _inputs(bal)
    rng = np.random.default_rng(11)
    old = (rng.standard_normal(9 * bal["n_edges"]) * 1e-3).astype(np.float32)
    other = (rng.standard_normal(9 * bal["n_edges"]) * 1e-3).astype(np.float32)
    d, h = _engine(bal, K, hooks=True, per_factor_mu=1), _engine(bal, K, hooks=True, per_factor_mu=1)
    with pytest.raises(GbpError, match="mu != oldmu"):
        h.upload(dict(state, mu=other, oldmu=old))
    h.upload(dict(state, mu=old, oldmu=old))
    d.upload(_dev(dict(state, mu=other, oldmu=old)))
    for x, y in zip(d.mu(), h.mu()):
        assert np.array_equal(x, y)
    for e in (d, h):
        e.linearise()
        e.iterate(3)
    for x, y in zip(d.mu() + d.factor_potentials(), h.mu() + h.factor_potentials()):
        assert np.array_equal(x, y)
    _equal(d.read(), h.read(), STATE)
