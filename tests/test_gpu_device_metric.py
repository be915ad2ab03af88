"""The metric in device memory (include/gbp_mi355x.h, "Device-resident arrays"): gbp_eval / gbp_iterate_eval_each / gbp_ba_loop with an
`out` on the ctx's GPU — GbpEngine's device=True / out=... — against the host-pointer forms of the same calls on a twin engine with
identical inputs.  Every comparison is on the bytes of the 56-byte records: both forms run the same device arithmetic in the same
order, the fold of the partial sums included (sum_eval on the host, k_eval_fold_part / k_eval_fold on the device)."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.conftest import seq_path

pytestmark = pytest.mark.gpu

STATE = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
PATHS = {"persistent_kernel": {}, "riding": {"persistent": -1}, "fallback": {"per_factor_mu": 1}}
_CACHE = {}


def _bal(name):
    from gbp_poplar_amd import hostlib
    if name not in _CACHE:
        if name == "synth_240":
            _CACHE[name] = hostlib.synth_generate(6, 60, 4, 3)            # 240 factors: one 256-position block
        elif name == "synth_270k":
            _CACHE[name] = hostlib.synth_generate(64, 30000, 9, 5)        # 270 000 factors: > 4 096 tiles, eval_blocks at its cap of 1 024
        else:
            _CACHE[name] = hostlib.bal_read(seq_path(name))
    return _CACHE[name]


def _inputs(bal):
    from gbp_poplar_amd import driver, hostlib
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    return K, state, opts


def _engine(bal, K, state, hooks=False, **params):
    from gbp_poplar_amd import _cabi
    from gbp_poplar_amd.engine import GbpEngine
    e = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**params), hooks=hooks)
    e.upload(state)
    e.linearise()
    return e


def _twins(name, **params):
    bal = _bal(name)
    K, state, opts = _inputs(bal)
    return _engine(bal, K, state, **params), _engine(bal, K, state, **params), bal, K, state, opts


def _host_bytes(res):
    """the records of a host-form call (a dict, or a list of dicts) as the library wrote them"""
    res = [res] if isinstance(res, dict) else res
    return b"".join(struct.pack("<dd5Q", *(r[k] for k in ("sum_norm", "sum_half_sq", "n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd"))) for r in res)


def _dev_bytes(raw):
    return raw.cpu().numpy().tobytes()


def _same_records(dev_raw, host_res, what):
    d, h = np.frombuffer(_dev_bytes(dev_raw), np.uint8), np.frombuffer(_host_bytes(host_res), np.uint8)
    assert d.size == h.size and d.size % 56 == 0, what
    if not np.array_equal(d, h):
        bad = np.flatnonzero((d.reshape(-1, 56) != h.reshape(-1, 56)).any(axis=1))
        raise AssertionError("%s: records %s differ, first: device %s, host %s" % (what, bad[:8], struct.unpack("<dd5Q", d.reshape(-1, 56)[bad[0]].tobytes()),
                                                                                   struct.unpack("<dd5Q", h.reshape(-1, 56)[bad[0]].tobytes())))


def _same_state(d, h, what):
    d.sync()
    for a, b in ((d.read(), h.read()), (d.read_priors(), h.read_priors())):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _raw(n=None):
    import torch
    return torch.full((7,) if n is None else (n, 7), -1, dtype=torch.int64, device="cuda")


# ---- 1. bit-equality, every path x every call ----
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["synth_240", "fr1xyz"])
def test_every_call_on_every_path_equals_the_host_form(name, path, oracle_mod):
    d, h, bal, K, state, _ = _twins(name, **PATHS[path])
    assert (d.graph_state() == 2) == (path == "persistent_kernel")
    # gbp_eval
    raw = _raw()
    views = d.eval(out=raw)
    d.sync()
    _same_records(raw, h.eval(), "eval")
    assert views["n_active"].item() == bal["n_edges"] and views["sum_norm"].dtype.is_floating_point
    if name == "synth_240":      # the yardstick is the oracle, not only the library's other path (as test_gpu_parity.test_eval_matches_oracle)
        orc = oracle_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
        orc.set_sum_order(1)
        orc.upload(state)
        orc.linearise()
        o = orc.eval()
        g = {k: v.item() for k, v in views.items()}
        assert g["n_active"] == o["n_active"] and g["n_robust"] == o["n_robust"]
        assert abs(g["sum_norm"] - o["sum_norm"]) <= 1e-6 * o["sum_norm"]
        assert abs(g["sum_half_sq"] - o["sum_half_sq"]) <= 1e-6 * o["sum_half_sq"]
    # gbp_ba_loop: weakens in front of passes 1, 3 and 5
    got = d.ba_loop(12, 0, 3, device=True)
    want = h.ba_loop(12, 0, 3)
    d.sync()
    assert got["sum_norm"].shape == (12,) and [int(x) for x in got["n_active"].cpu()] == [w["n_active"] for w in want]
    import torch
    raw12 = torch.stack([got[k].view(torch.int64) for k in got], dim=1)      # (the returned columns view ONE buffer of records: put together again)
    _same_records(raw12, want, "ba_loop")
    _same_state(d, h, "ba_loop")
    # gbp_iterate_eval_each
    raw7 = _raw(7)
    d.iterate_eval_each(7, out=raw7)
    want = h.iterate_eval_each(7)
    d.sync()
    _same_records(raw7, want, "iterate_eval_each")
    # ... and one more gbp_eval, two device forms back to back
    a, b = _raw(), _raw()
    d.eval(out=a)
    d.eval(out=b)
    d.sync()
    w = h.eval()
    _same_records(a, w, "eval after the loops")
    _same_records(b, h.eval(), "second eval")
    assert d.graph_state() == h.graph_state()
    _same_state(d, h, "end")
    assert _host_bytes(d.eval()) == _host_bytes(h.eval())


# ---- 2. piece boundaries ----
@pytest.mark.parametrize("path,n", [("riding", 260), ("persistent_kernel", 515)])
def test_bursts_longer_than_one_piece(path, n):
    """the riding path folds pieces of at most 256 iterations (the ring of per-tile records), the persistent kernel takes at most 512
    metrics per launch (kSeriesMax): the pieces queue behind each other"""
    d, h, *_ = _twins("synth_240", **PATHS[path])
    raw = _raw(n)
    d.iterate_eval_each(n, out=raw)
    want = h.iterate_eval_each(n)
    d.sync()
    _same_records(raw, want, path)
    _same_state(d, h, path)


# ---- 3. more than 4 096 tiles: k_eval's blocks are strided, its 1 024 block sums are folded per block ----
def test_big_graph_with_strided_eval_blocks():
    d, h, bal, *_ = _twins("synth_270k")
    assert bal["n_edges"] > 4096 * 64
    raw, raw3 = _raw(), _raw(3)
    d.eval(out=raw)
    d.iterate_eval_each(3, out=raw3)
    d.sync()
    _same_records(raw, h.eval(), "eval")
    _same_records(raw3, h.iterate_eval_each(3), "iterate_eval_each")
    _same_state(d, h, "big")


# ---- 4. ordering ----
@pytest.mark.parametrize("path", ["riding", "persistent_kernel"])
def test_the_call_returns_before_the_stream_drains_and_is_ordered_on_it(path):
    import torch
    d, h, *_ = _twins("fr1xyz", **PATHS[path])
    n = 6
    s = torch.cuda.Stream()
    d.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        raw = _raw(n)
        d.iterate_eval_each(n, out=raw)                  # warm-up: first-use allocations, graph capture
        busy = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GiB: ~0.5 ms of HBM traffic per pass over it
        for _ in range(200):
            busy.mul_(1.0001)
        d.iterate_eval_each(n, out=raw)
        assert not s.query(), "the device form waited for the stream"
        first = raw.clone()                                # queued behind the call, no synchronisation in between
        d.iterate_eval_each(n, out=raw)
        running = not s.query()
    d.sync()
    assert running, "the second burst waited for the first"
    h.iterate_eval_each(n)
    _same_records(first, h.iterate_eval_each(n), "the clone queued behind the first call")
    _same_records(raw, h.iterate_eval_each(n), "the second call into the same buffer")
    d.set_stream(None)
    _same_state(d, h, path)


# ---- 5. health counters ----
def test_health_counters_with_host_and_device_forms_interleaved():
    """a graph with landmarks nobody observes (NaN beliefs from the first weakening on: tests/test_gpu_parity.py,
    test_health_counters_with_metric_calls_of_every_kind_interleaved): the double-buffered health words are left by every device form
    as the host form leaves them, whatever metric call comes next"""
    from gbp_poplar_amd import driver, hostlib
    from tests.test_gpu_parity import _ragged_bal
    bal, kw = _ragged_bal()
    opts = driver.Options()
    opts.undamped_start = 2
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    steps = int(opts.steps)
    probe = _engine(bal, K, state, persistent=1, **kw)
    last = probe.ba_loop(2 * steps + 9, 0, steps)[-1]
    assert last["n_nonfinite"] >= 1 and last["n_nonpd"] >= 1
    d, h = _engine(bal, K, state, persistent=1, **kw), _engine(bal, K, state, persistent=1, **kw)
    assert d.graph_state() == 2
    it = 0
    seen_unhealthy = False
    plan = (("eval", 0, True), ("loop", 2, True), ("eval", 0, False), ("loop", 5, False), ("eval", 0, True), ("loop", 4, True),
            ("iterate_eval", 3, False), ("eval", 0, True), ("each", 3, True), ("begin_end", 0, False), ("loop", 2, True), ("each", 2, False),
            ("eval", 0, True), ("each", 1, True), ("iterate_eval", 1, False), ("loop", 3, True))
    for kind, n, dev in plan:
        what = (kind, n, dev, it)
        if kind in ("iterate_eval", "each"):
            assert it >= 2 * steps      # (no weakening inside: these calls know nothing of the loop's schedule)
        if kind == "eval":
            want = h.eval()
            if dev:
                raw = _raw()
                d.eval(out=raw)
        elif kind == "loop":
            want = h.ba_loop(n, it, steps)
            if dev:
                raw = _raw(n)
                d.ba_loop(n, it, steps, out=raw)
        elif kind == "each":
            want = h.iterate_eval_each(n)
            if dev:
                raw = _raw(n)
                d.iterate_eval_each(n, out=raw)
        elif kind == "iterate_eval":
            h.iterate_eval(n)
            want = h.eval_end()
        else:
            h.eval_begin()
            want = h.eval_end()
        if dev:
            d.sync()
            _same_records(raw, want, what)
            rows = raw.reshape(-1, 7)
            seen_unhealthy |= bool(((rows[:, 5] > 0) & (rows[:, 6] > 0)).any())
        else:
            if kind == "eval":
                got = d.eval()
            elif kind == "loop":
                got = d.ba_loop(n, it, steps)
            elif kind == "each":
                got = d.iterate_eval_each(n)
            elif kind == "iterate_eval":
                d.iterate_eval(n)
                got = d.eval_end()
            else:
                d.eval_begin()
                got = d.eval_end()
            assert _host_bytes(got) == _host_bytes(want), what
        it += n
    assert seen_unhealthy
    assert _host_bytes(d.eval()) == _host_bytes(h.eval())
    _same_state(d, h, "health")


# ---- 6. rejections ----
def _eval_at(eng, address):
    from gbp_poplar_amd import _cabi as cabi
    return eng.lib.gbp_eval(eng.h, C.cast(C.c_void_p(address), C.POINTER(cabi.GbpEvalOut)))


def test_rejections_leave_the_ctx_untouched():
    import torch
    from gbp_poplar_amd import _cabi as cabi
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    d, h, bal, K, state, _ = _twins("synth_240")
    for e in (d, h):
        e.iterate(3)
    # a tensor on the CPU, another dtype, another shape: TypeError before the library is called
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(7, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")):
        with pytest.raises(TypeError):
            d.eval(out=bad)
    for bad in (torch.zeros((4, 7), dtype=torch.int64), torch.zeros((4, 7), dtype=torch.int32, device="cuda"), torch.zeros((5, 7), dtype=torch.int64, device="cuda"),
                torch.zeros((7, 4), dtype=torch.int64, device="cuda").t()):
        with pytest.raises(TypeError):
            d.iterate_eval_each(4, out=bad)
        with pytest.raises(TypeError):
            d.ba_loop(4, 0, 3, out=bad)
    # a device address that is only 4-byte aligned (an int64 tensor cannot start there: the addresses go straight into the C-ABI)
    big = torch.zeros(2 * 7 * 4 + 2, dtype=torch.int32, device="cuda")
    odd = big.data_ptr() + 4
    assert odd % 8 == 4
    ptr = C.cast(C.c_void_p(odd), C.POINTER(cabi.GbpEvalOut))
    assert _eval_at(d, odd) == -1 and "8-byte" in d.last_error() and "out" in d.last_error()
    assert d.lib.gbp_iterate_eval_each(d.h, 4, ptr) == -1 and "8-byte" in d.last_error()
    assert d.lib.gbp_ba_loop(d.h, 4, 0, 3, ptr) == -1 and "8-byte" in d.last_error()
    torch.cuda.synchronize()
    assert int(big.abs().sum()) == 0
    # an evaluation in flight: GBP_ERR_STATE as in the host forms
    d.eval_begin()
    with pytest.raises(GbpError, match="in flight"):
        d.eval(device=True)
    with pytest.raises(GbpError, match="in flight"):
        d.ba_loop(2, 0, 3, device=True)
    assert _host_bytes(d.eval_end()) == _host_bytes(h.eval())
    # pinned host memory is host memory: today's path, blocking
    pinned = torch.zeros(7, dtype=torch.int64).pin_memory()
    assert _eval_at(d, pinned.data_ptr()) == 0
    assert pinned.numpy().tobytes() == _host_bytes(h.eval())
    # a landmark-sharded ctx
    sh = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, shard=(0, 2, 0, bal["n_lmks"] // 2))
    sh.upload(state)
    before = sh.read()
    with pytest.raises(GbpError, match="sharded"):
        sh.eval(device=True)
    with pytest.raises(GbpError, match="sharded"):
        sh.iterate_eval_each(2, device=True)
    with pytest.raises(GbpError, match="sharded"):
        sh.ba_loop(2, 0, 3, device=True)
    after = sh.read()
    for k in STATE:
        assert np.array_equal(after[k], before[k], equal_nan=True), k
    # the ctx is where its twin is
    assert _host_bytes(d.eval()) == _host_bytes(h.eval())
    _same_state(d, h, "after the refused calls")


def test_managed_memory_is_refused_by_name():
    d, h, *_ = _twins("synth_240")
    assert d.eval(device=True)["n_active"].item() == h.eval()["n_active"]
    loaded = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l]      # the ONE HIP runtime of this process
    assert loaded
    hip = C.CDLL(loaded[0])
    hip.hipMallocManaged.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipFree.argtypes = [C.c_void_p]
    m = C.c_void_p()
    rc = hip.hipMallocManaged(C.byref(m), 4 * 56, 1)
    if rc != 0 or not m.value:
        pytest.skip("hipMallocManaged is not available here (status %d)" % rc)
    try:
        from gbp_poplar_amd import _cabi as cabi
        ptr = C.cast(C.c_void_p(m.value), C.POINTER(cabi.GbpEvalOut))
        assert _eval_at(d, m.value) == -1 and "managed" in d.last_error() and "out" in d.last_error()
        assert d.lib.gbp_iterate_eval_each(d.h, 4, ptr) == -1 and "managed" in d.last_error()
        assert d.lib.gbp_ba_loop(d.h, 4, 0, 3, ptr) == -1 and "managed" in d.last_error()
    finally:
        hip.hipFree(m)
    assert _host_bytes(d.eval()) == _host_bytes(h.eval())
    _same_state(d, h, "after the refused calls")


# ---- 7. timing ----
@pytest.mark.parametrize("path", list(PATHS))
def test_timing_counts_the_iterations_of_the_device_forms(path):
    d, h, *_ = _twins("synth_240", **PATHS[path])
    t0d, t0h = d.timing()["iterations"], h.timing()["iterations"]
    d.eval(device=True)
    h.eval()
    assert d.timing()["iterations"] == t0d and h.timing()["iterations"] == t0h
    d.iterate_eval_each(6, device=True)
    h.iterate_eval_each(6)
    assert d.timing()["iterations"] - t0d == 6 == h.timing()["iterations"] - t0h
    d.ba_loop(5, 0, 3, device=True)
    h.ba_loop(5, 0, 3)
    d.sync()
    assert d.timing()["iterations"] - t0d == 11 == h.timing()["iterations"] - t0h
