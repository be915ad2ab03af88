"""Several contexts in one process: what they share, and what the header promises about it.

A ctx is tested thoroughly alone.  What contexts SHARE is process-wide state of csrc/gbp_api_persist.cpp and csrc/gbp_api_ctx.cpp; a
regression there changes no bit of any result (a persistent launch that starved is restored and replayed on the two-kernel path,
identically) — it shows as a ctx that silently left the persistent path, as a `warning:` in gbp_last_error, or as a use of a stream
somebody destroyed.  Every test here therefore ends with the same three assertions (tests/multi_ctx_support.py: compare): every ctx
bit-identical to ITS OWN calls run alone (every tensor of read(), both message sets, priors, potentials, metric records; NaN == NaN),
every ctx that was on the persistent path alone still on it (graph_state() == 2), and no `warning:` / time-out in last_error().

WHY THESE TESTS CAN SEE A MISSING WAIT.  Every workgroup of a launch of the persistent kernel spins until ALL workgroups of its grid
are resident.  Two such grids that each fit the device but not together, dispatched side by side, can each hold CUs the other needs:
both sit in their bounded wait (1.5 s), give up, and are recovered.  The library prevents that by making a launch from another ctx or
stream wait for an event recorded behind the previous launch.  If the wait were missing, nothing would happen as long as the grids fit
together — so each test asserts, as its precondition, that every persistent ctx alone reports graph_state() == 2 AND that the workgroup
counts (gbp_debug_persist_roles, the launcher's own function) of the contexts in flight sum to more than the device's
multi_processor_count: "half" graphs of 162 - 168 workgroups each (two: > 256), or six shipped sequences (2 x (63 + 70 + 20) = 306).
Correct code never lets two grids compete, so the tests provoke nothing; the sensitivity is this argument, not a run with the wait
taken out.

WHICH TEST HOLDS WHAT
  process-wide words of gbp_api_persist.cpp
    g_persist_mu            test_one_host_thread_per_context (four threads launch and create — the probe takes the lock too — at once)
    g_persist_event[16]     test_interleaved_without_sync (the event is what B's launch waits for behind A's, every turn),
                            test_more_streams_than_hardware_queues (six waiters on aliased queues)
    g_persist_last_ctx[16]  test_destroyed_with_launches_in_flight (persist_forget rewrites it; A2 may get A's address),
                            test_interleaved_without_sync
    g_persist_last_stream[16]  test_moved_between_caller_streams (same ctx, other stream: must wait),
                            test_caller_stream_destroyed_after_set_stream_0 (the word still names a stream that is gone: compared, never used)
  sentences of include/gbp_mi355x.h and of gbp_api_persist.cpp
    "the launches of one process are serialised by the library" (gbp_params.persist_coop)
                            test_interleaved_without_sync, test_more_streams_than_hardware_queues, test_one_host_thread_per_context,
                            test_drawn_plan_interleaved, test_mixed_kinds_at_once
    the creation-time probe runs "behind the device's last k_persist launch, so that it does not compete with one"
                            test_destroyed_with_launches_in_flight (A2 is created while B's launches are in flight),
                            test_one_host_thread_per_context, test_drawn_plan_interleaved (close + create in mid-run)
    "no stream handle of another ctx is ever touched (it may have been destroyed by its owner)"
                            test_destroyed_with_launches_in_flight, test_moved_between_caller_streams,
                            test_caller_stream_destroyed_after_set_stream_0 (streams really destroyed: hipStreamDestroy, not torch's pool)
    a ctx that changes its stream still orders behind its own earlier launch
                            test_moved_between_caller_streams
    cooperative launches (persist_coop = 1) beside plain ones, a replayed hipGraph and the ctx-less libraries on a further stream
                            test_mixed_kinds_at_once
    gbp_last_error(NULL) is the calling thread's; c->err / c->warn are the ctx's
                            test_two_threads_read_their_own_creation_error, test_a_failing_call_leaves_the_other_ctx_alone
                            (and tests/sanitize/create_threads_main.cpp under TSan and ASan, tests/test_host_sanitizers.py)
  meaning (the baseline is the same library): test_float64_anchor_inside_an_interleaved_run — tests/test_exact_inference.py's hub tree,
  run between two half graphs, meets that module's A_BOUND against tests/ref64.py.

profiles/multi_ctx.md has the workgroup counts, the device's CU count and the wall time of every test here."""
import threading

import numpy as np
import pytest

from tests import multi_ctx_support as mc

pytestmark = pytest.mark.gpu

ASYNC = mc.BURSTS                # with verbs=ASYNC the metric goes to device records: no call of the plan blocks
JOIN_TIMEOUT = 60.0              # seconds a thread may take for a plan that runs in well under ten


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _precondition(p, want, among=None):
    """every persistent ctx ran in the persistent kernel when alone, and the grids in flight do not fit the device together"""
    for i, (c, w) in enumerate(zip(p["contexts"], want)):
        if c["persistent"] >= 0:
            assert w["created_state"] == 2 and w["graph_state"] == 2, "ctx %d (%s) alone: graph_state %d: %s" % (i, c["graph"], w["graph_state"], w["last_error"])
    total, over = mc.over_device(p, _cus(), among)
    print("workgroups in flight %d (%s), CUs %d" % (total, " + ".join(str(c["grid"][0]) for i, c in enumerate(p["contexts"])
                                                                         if c["persistent"] >= 0 and (among is None or i in among)), _cus()))
    assert over, "the grids sum to %d workgroups, the device has %d CUs: a missing wait could not show" % (total, _cus())


def _interleaved(p, runner=mc.run, among=None, **kw):
    want = mc.baseline(p)
    _precondition(p, want, among)
    got = runner(p, **kw)
    mc.compare_all(p, got, want)
    return got, want


# ---- one thread ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", ["own", "caller"])
def test_interleaved_without_sync(streams):
    """two half graphs and a shipped sequence, bursts queued A, B, C, A, ... with no sync and no blocking call between them"""
    p = mc.plan(11, 3, graphs=["half0", "half1", "fr1xyz"], persistent=[0, 1, 0], coop=[0] * 3, streams=[streams] * 3, rounds=6, others=0.0, verbs=ASYNC)
    assert [i for i, _, _ in p["calls"]] == [0, 1, 2] * 6 and not any(a[-1] == "host" for _, v, a in p["calls"] if v in ("ba_loop_metric", "iterate_eval_each"))
    _interleaved(p, among=(0, 1))


def test_more_streams_than_hardware_queues():
    """six contexts of shipped-sequence size on six streams (three of their own, three of torch's): more streams than the four hardware
    queues a process gets here, so streams alias onto queues and a waiting launch can sit in front of the one it waits for"""
    p = mc.plan(12, 6, graphs=list(mc.SEQUENCES) * 2, persistent=[0] * 6, coop=[0] * 6, streams=["own", "caller"] * 3, rounds=5, others=0.0, verbs=ASYNC)
    _interleaved(p)


@pytest.mark.parametrize("seed", mc.PLAN_SEEDS[:2])
def test_drawn_plan_interleaved(seed):
    """a drawn plan with every verb (blocking calls, reads, weakenings, stream changes, close + create in mid-run) on two halves and two
    sequences, from one thread"""
    p = mc.plan(seed, 4, graphs=["half0", "half1", "fr1desk", "fr2robot2"], persistent=[0, 0, 0, -1], coop=[0] * 4)
    _interleaved(p, among=(0, 1))


# ---- one host thread per context -------------------------------------------------------------------------------------------------
def test_one_host_thread_per_context():
    """four threads, one ctx each (created in its thread), two of them half graphs; they start together and run their plan's calls"""
    p = mc.plan(mc.PLAN_SEEDS[2], 4, graphs=["half1", "fr1xyz", "half2", "fr2robot2"], persistent=[0, 0, 1, 0], coop=[0] * 4)
    want = mc.baseline(p)
    _precondition(p, want, among=(0, 2))
    try:
        got = mc.run_threads(p, timeout=JOIN_TIMEOUT)
    except TimeoutError as err:      # a thread is stuck in the library: nothing more may be launched on this GPU by this session
        pytest.exit("test_one_host_thread_per_context: %s" % err, returncode=1)
    mc.compare_all(p, got, want)


# ---- life times ------------------------------------------------------------------------------------------------------------------
def test_destroyed_with_launches_in_flight():
    """A queues bursts and is destroyed at once; B launches; A2 is created (its probe behind B's launches) and runs: B and A2 equal their
    baselines.  (A's own results before the destroy are device records: compared too.)"""
    calls = [(1, "iterate", 30), (0, "iterate", 40), (0, "ba_loop_metric", (30, 40, mc.BA_STEPS, "device")), (0, "destroy", None),
             (1, "ba_loop", (40, 30, mc.BA_STEPS)), (1, "iterate_eval_each", (20, "device")), (0, "create", None), (1, "iterate", 25),
             (0, "iterate", 35), (1, "iterate", 25), (0, "ba_loop_metric", (20, 35, mc.BA_STEPS, "device")), (1, "iterate", 10)]
    p = mc.plan(13, 2, graphs=["half0", "half1"], persistent=[0, 0], coop=[0, 0], streams=["own", "caller"], calls=calls)
    _interleaved(p)


def test_moved_between_caller_streams():
    """A runs on a caller's stream, is moved to a new one between bursts — the old stream is DESTROYED at once — while B keeps launching"""
    calls = [(0, "iterate", 30), (1, "iterate", 30), (0, "set_stream", "fresh"), (0, "ba_loop", (30, 30, mc.BA_STEPS)), (1, "iterate", 30),
             (0, "iterate_eval_each", (20, "device")), (0, "set_stream", "fresh"), (0, "iterate", 40), (1, "ba_loop_metric", (30, 60, mc.BA_STEPS, "device")),
             (0, "set_stream", "new"), (0, "iterate", 20), (1, "iterate", 20)]
    p = mc.plan(14, 2, graphs=["half0", "half2"], persistent=[0, 0], coop=[0, 0], streams=["hip", "own"], calls=calls)
    _interleaved(p)


def test_caller_stream_destroyed_after_set_stream_0():
    """A leaves the caller's stream for its own (set_stream(0)) and the caller destroys the stream; the process-wide "last stream" word
    still holds the handle when B launches next"""
    calls = [(1, "iterate", 20), (0, "iterate", 40), (0, "set_stream", "own"), (1, "iterate", 40), (0, "iterate", 30), (1, "iterate", 30),
             (0, "ba_loop_metric", (20, 70, mc.BA_STEPS, "device")), (1, "iterate", 10)]
    p = mc.plan(15, 2, graphs=["half1", "half2"], persistent=[0, 0], coop=[0, 0], streams=["hip", "hip"], calls=calls)
    _interleaved(p)


# ---- mixed kinds -----------------------------------------------------------------------------------------------------------------
def _stateless_inputs():
    """a resection and a location problem (9 and 11 cameras of 0 .. 1000 views) as device tensors"""
    import torch
    from tests import locate_support as ls
    from tests import resect_support as rs
    cycle = [0, 2, 3, 5, 6, 63, 64, 65, 127, 129, 1000]
    dev = lambda a, ints=False: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if ints else np.ascontiguousarray(a)).cuda()
    r = rs.degree_scene(np.resize(cycle, 9), seed=209, n_lmks=1000)[0]
    l = ls.scene(np.resize(cycle, 11), seed=311, outlier_share=0.2, noise=0.5, n_lmks=1000)[0]
    ins = {"resect": ([dev(r[k], True) for k in ("lmk_id", "cam_start")], r["K"], dev(r["cam_mean"]), dev(r["lmk_mean"]), dev(r["measurements"])),
           "locate": ([dev(l[k], True) for k in ("lmk_id", "cam_start")], l["K"], dev(l["lmk_mean"]), dev(l["measurements"]))}
    torch.cuda.synchronize()
    return ins


def _stateless_calls(ins, stream):
    """resect.cameras and locate.cameras queued on `stream`, nothing waited for: -> their result tensors"""
    import torch
    from gbp_poplar_amd import locate, resect
    with torch.cuda.stream(stream):
        (idx, K, cam_mean, lmk_mean, z) = ins["resect"]
        a = resect.cameras(idx[0], idx[1], None, K, cam_mean.clone(), lmk_mean, z)      # (cam_mean is refined in place)
        (idx, K, lmk_mean, z) = ins["locate"]
        b = locate.cameras(idx[0], idx[1], None, K, lmk_mean, z)
    return {"resect": a, "locate": b}


@pytest.mark.parametrize("coop", [0, 1], ids=["plain", "cooperative"])
def test_mixed_kinds_at_once(coop):
    """queued without a sync between them: a persistent ctx, a two-kernel ctx replaying its hipGraph, a third persistent ctx launched
    plainly or cooperatively, a shipped sequence, and resect.cameras / locate.cameras on a further stream after every second turn"""
    import torch
    p = mc.plan(16, 4, graphs=["half0", "half1", "half2", "fr2robot2"], persistent=[0, -1, 1, 0], coop=[0, 0, coop, 0], streams=["own", "own", "caller", "own"],
                rounds=5, others=0.0, verbs=ASYNC)
    want = mc.baseline(p)
    if coop and want[2]["created_state"] != 2:
        pytest.skip(want[2]["last_error"])      # the device (or its driver) refuses cooperative launches: the library's reason
    _precondition(p, want, among=(0, 2))
    assert want[1]["graph_state"] == 1, "the two-kernel ctx replays a captured hipGraph (bursts of >= graph_unroll iterations)"
    ins = _stateless_inputs()
    side = torch.cuda.Stream()
    alone = _stateless_calls(ins, side)
    torch.cuda.synchronize()
    alone = {k: {f: t.cpu().numpy() for f, t in v.items()} for k, v in alone.items()}
    assert (alone["resect"]["status"] == 0).any() and (alone["locate"]["n_inliers"] > 0).any()
    held = []
    got = mc.run(p, between=lambda k, ctxs: held.append(_stateless_calls(ins, side)) if k % 8 == 7 else None)
    mc.compare_all(p, got, want)
    torch.cuda.synchronize()
    assert len(held) >= 2
    for res in held:
        for k, v in res.items():
            for f, t in v.items():
                mc.fz.same(t.cpu().numpy(), alone[k][f], "%s.cameras beside the contexts: %s" % (k, f))


# ---- the float64 anchor ------------------------------------------------------------------------------------------------------------
def test_float64_anchor_inside_an_interleaved_run():
    """test_exact_inference's hub tree (dmu_threshold = 0, undamped: exact marginals after diameter + 2 sweeps) as one of three
    interleaved contexts: its marginals meet A_BOUND against float64 exact inference of the potentials it holds"""
    from tests import test_exact_inference as ex
    bal = mc.graph("hub")[0]
    sweeps = ex.diameter(bal) + ex.A_SWEEPS_OVER_DIAMETER
    g = ex._Exact("A hub tree", bal, sweeps, maxeta_damping=0.0)
    assert 10 <= sweeps <= 50
    calls = [(0, "iterate", 30), (2, "iterate", 30), (1, "iterate", sweeps), (0, "ba_loop", (30, 30, mc.BA_STEPS)), (2, "iterate", 30), (0, "iterate", 20)]
    p = mc.plan(17, 3, graphs=["half0", "hub", "half1"], persistent=[0, 0, 0], coop=[0] * 3, streams=["own", "caller", "own"],
                params=[{}, dict(g.params), {}], calls=calls)
    got, _ = _interleaved(p, among=(0, 2))
    final = got[1]["final"]
    for k in g.state:      # the joint's priors and flags are the ones the ctx uploaded
        assert np.array_equal(np.asarray(g.state[k]), np.asarray(mc.graph("hub")[2][k])), k
    err = g.errors(final, g.exact(final["fac_eta"], final["fac_lambda"]))
    print("hub tree inside the interleaved run after %d sweeps: %s" % (sweeps, "  ".join("%s %.3e" % kv for kv in err.items())))
    for k in ex.TENSORS:
        assert err[k] <= ex.A_BOUND[k], (k, err[k], ex.A_BOUND[k])


# ---- errors stay with their owner ------------------------------------------------------------------------------------------------------
def test_a_failing_call_leaves_the_other_ctx_alone():
    """GBP_ERR_STATE from gbp_new_keyframe before the upload on A: B's last_error() and the thread's creation error are unchanged"""
    from gbp_poplar_amd import _lib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    bal, K, state = mc.graph("fr2robot2")
    A = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
    B = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, hooks=True)
    try:
        B.upload(state)
        B.linearise()
        B.iterate(12)
        before_b, before_thread = B.last_error(), _lib.load(hooks=True).gbp_last_error(None)
        with pytest.raises(GbpError, match=r"status -4"):
            A.new_keyframe({"damping_count": np.zeros(bal["n_edges"], np.int32)})
        assert "upload" in A.last_error() and A.last_error() != before_b
        assert B.last_error() == before_b and _lib.load(hooks=True).gbp_last_error(None) == before_thread
        B.iterate(12)
        B.sync()
        assert B.graph_state() == 2 and mc.no_warning(B.last_error())
    finally:
        A.close()
        B.close()


def test_two_threads_read_their_own_creation_error():
    """two threads make creations that fail — an empty cam_id on one, n_cams = 0 on the other, then an index out of range and a bad shard,
    whose texts differ —, meet, and each reads ITS text from gbp_last_error(NULL); the main thread's stays empty"""
    from gbp_poplar_amd import _lib
    from gbp_poplar_amd.engine import GbpEngine, GbpError
    lib = _lib.load(hooks=True)
    K = [500, 0, 320, 0, 500, 240, 0, 0, 1]
    cam, lmk = np.array([0, 0, 1, 1], np.uint32), np.array([0, 1, 1, 2], np.uint32)
    empty = np.zeros(0, np.uint32)
    attempts = [[(dict(cam_id=empty, lmk_id=empty, n_cams=2, n_lmks=3), "null or empty problem"), (dict(cam_id=cam, lmk_id=lmk + 7, n_cams=2, n_lmks=3), "index out of range")],
                [(dict(cam_id=cam, lmk_id=lmk, n_cams=2, n_lmks=3, shard=(2, 2, 0, 3)), "bad shard"), (dict(cam_id=cam, lmk_id=lmk, n_cams=0, n_lmks=3), "null or empty problem")]]
    gate = threading.Barrier(2)
    seen, errors = [[], []], []

    def work(t):
        try:
            for kw, _ in attempts[t]:
                with pytest.raises(GbpError):
                    GbpEngine(kw["cam_id"], kw["lmk_id"], kw["n_cams"], kw["n_lmks"], K, shard=kw.get("shard"), hooks=True)
                gate.wait(JOIN_TIMEOUT)                      # both have failed, each in its own way ...
                seen[t].append(lib.gbp_last_error(None).decode())
                gate.wait(JOIN_TIMEOUT)                      # ... and read before either fails again
        except BaseException as err:      # noqa: B902
            errors.append(err)
            gate.abort()

    before = lib.gbp_last_error(None)
    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_TIMEOUT)
    assert not any(th.is_alive() for th in threads) and not errors, errors
    for t in range(2):
        for (_, text), got in zip(attempts[t], seen[t]):
            assert text in got, (t, text, got)
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    assert lib.gbp_last_error(None) == before
