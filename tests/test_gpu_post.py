"""The solution readout on the GPU (libgbp_mi355x_post.so, gbp_poplar_amd/post.py, GbpEngine.solution, `ba --cov_file`).

The device results are compared BIT FOR BIT (NaNs equal NaNs) with the host twin — the same header, post/post_math.hpp, compiled by the
host compiler into a stand-alone program (tests/sanitize/post_math_main.cpp, run as a process) — whose meaning tests/test_post_cpu.py
checks against float64; for the residual's rotation it evaluates the GPU math library's sinf / cosf, not the host libm's.  On a tree
the covariances are checked against the exact marginals as well (the bound and what it can see: post_support.tree_covariance_check;
the CPU oracle uses 0.9 % of it)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import post_support as ps
from tests.conftest import seq_path
from tests.test_gpu_parity import _tiny_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = os.path.join(ROOT, "gbp_poplar_amd", "bin", "ba")
CANARY = 0x7FA5A5A5      # (as a float: a NaN no computation produces)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ps.compile_host(str(tmp_path_factory.mktemp("post_host") / "post_math"), sanitize=False)


def _all_to_all(n_cams, n_lmks):
    cam_id = np.repeat(np.arange(n_cams), n_lmks)
    lmk_id = np.tile(np.arange(n_lmks), n_cams)
    return _tiny_problem(cam_id.tolist(), lmk_id.tolist(), n_cams, n_lmks)


def _inputs(bal):
    from gbp_poplar_amd import driver, hostlib
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    return K, state, int(opts.steps)


def _engine(bal, K, hooks=False, **params):
    from gbp_poplar_amd import _cabi
    from gbp_poplar_amd.engine import GbpEngine
    return GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**params), hooks=hooks)


@pytest.fixture(scope="module")
def tiny():
    """(bal, K, state, beliefs): _tiny_problem, 6 cameras x 60 landmarks all to all, after 12 passes of the default loop on the engine"""
    bal = _all_to_all(6, 60)
    K, state, steps = _inputs(bal)
    eng = _engine(bal, K)
    eng.upload(state)
    eng.linearise()
    eng.ba_loop(12, 0, steps, metrics=False)
    b = eng.read()
    eng.close()
    assert all(np.isfinite(b[k]).all() for k in ps.BELIEFS)
    return bal, K, state, b


def _pool(tiny_beliefs):
    """the blocks the kernels are run on: the four hand-made ones of each width, then the tiny problem's beliefs"""
    h = ps.hand_made_beliefs()
    return {k: np.concatenate([h[k], tiny_beliefs[k]]) for k in ps.BELIEFS}


def _take(pool, n_c, n_l):
    """n_c cameras and n_l landmarks out of the pool, cycling through it"""
    out = {}
    for k, w in (("cam_beliefs_eta", 6), ("cam_beliefs_lambda", 36), ("lmk_beliefs_eta", 3), ("lmk_beliefs_lambda", 9)):
        rows = pool[k].reshape(-1, w)
        n = n_c if k.startswith("cam") else n_l
        out[k] = rows[np.arange(n) % rows.shape[0]].ravel().copy()
    return out


def _dev(a, offset):
    """numpy -> tensor on the GPU, same bits; a view inside a canary-filled buffer: at a 16-byte-aligned base (offset = False: 4 words
    in) or 4 bytes past one (5 words in), with canaries on both sides"""
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype != np.float32 else a
    lead = 5 if offset else 4
    big = torch.full((a.size + lead + 4,), CANARY, dtype=torch.int32, device="cuda")
    v = big[lead:lead + a.size].view(torch.float32 if a.dtype == np.float32 else torch.int32)
    v.copy_(torch.from_numpy(a.copy()))
    assert a.size == 0 or v.data_ptr() % 16 == (4 if offset else 0)
    return v, big


def _out(n, offset, dtype=np.float32):
    return _dev(np.zeros(n, dtype), offset)


def _canaries_intact(big, n, offset):
    lead = 5 if offset else 4
    h = big.cpu().numpy()
    return bool((h[:lead] == CANARY).all() and (h[lead + n:] == CANARY).all())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


MOMENT_SHAPES = [(1, 0), (0, 1), (3, 254), (70, 5)]      # one lane; no cameras; the camera / landmark switch inside a workgroup and a tail in a second; cameras across a wave boundary


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n_c,n_l", MOMENT_SHAPES)
def test_moments_equal_the_host_program(n_c, n_l, offset, tiny, host_exe, tmp_path):
    import torch
    from gbp_poplar_amd import hostlib, post
    b = _take(_pool(tiny[3]), n_c, n_l)
    want = ps.run_host(host_exe, tmp_path, b)
    ins = [_dev(b[k], offset) for k in ps.BELIEFS]
    outs = [_out(w * (n_c if name.startswith("cam") else n_l), offset, dt) for name, w, dt in ps.OUTPUTS]
    rc = post.load().gbp_post_moments(_stream(), n_c, n_l, *[_ptr(v) for v, _ in ins], *[_ptr(v) for v, _ in outs])
    assert rc == 0, post.load().gbp_post_last_error()
    torch.cuda.current_stream().synchronize()
    got = {name: (v.cpu().numpy().view(np.uint32) if dt == np.uint32 else v.cpu().numpy()) for (name, _, dt), (v, _) in zip(ps.OUTPUTS, outs)}
    for name, _, _ in ps.OUTPUTS:
        assert _same(got[name], want[name]), name
    for (name, w, _), (v, big) in zip(ps.OUTPUTS, outs):
        assert _canaries_intact(big, v.numel(), offset), name
    with np.errstate(all="ignore"):
        cams, pts = hostlib.belief_means(n_c, n_l, *[b[k] for k in ps.BELIEFS])
    assert _same(got["cam_mean"].astype(np.float64), cams) and _same(got["lmk_mean"].astype(np.float64), pts)
    if n_c >= 4:      # the hand-made blocks lead the pool: swapped / indefinite -> not PD, zero -> nothing finite, SPD 1e6 -> fine
        assert got["cam_status"][:4].tolist() == [2, 2, 3, 0]
    # the Python face on the same tensors
    m = post.moments({k: v for k, (v, _) in zip(ps.BELIEFS, ins)})
    torch.cuda.current_stream().synchronize()
    for name, _, dt in ps.OUTPUTS:
        assert _same(m[name].cpu().numpy().view(dt), want[name]), name


def test_moments_with_every_optional_output_null_but_one(tiny, host_exe, tmp_path):
    import torch
    from gbp_poplar_amd import post
    b = _take(_pool(tiny[3]), 70, 5)
    want = ps.run_host(host_exe, tmp_path, b)
    ins = [_dev(b[k], False) for k in ps.BELIEFS]
    cov, big = _out(36 * 70, False)
    rc = post.load().gbp_post_moments(_stream(), 70, 5, *[_ptr(v) for v, _ in ins], None, _ptr(cov), None, None, None, None)
    assert rc == 0, post.load().gbp_post_last_error()
    torch.cuda.current_stream().synchronize()
    assert _same(cov.cpu().numpy(), want["cam_cov"]) and _canaries_intact(big, cov.numel(), False)


def _edge_case(tiny, n_e):
    """the first n_e edges of the tiny problem (file order: sorted by camera), a third of them inactive"""
    bal, K, state, b = tiny
    sub = {"cam_id": bal["cam_id"][:n_e], "lmk_id": bal["lmk_id"][:n_e], "n_cams": bal["n_cams"], "n_lmks": bal["n_lmks"]}
    active = (np.arange(n_e) % 3 != 1).astype(np.uint32)
    return sub, K, state["measurements"][:2 * n_e], active, b


RESIDUAL_CASES = [pytest.param(True, True, False, id="flags-cov-aligned"), pytest.param(False, True, True, id="all_active-cov-offset4"),
                  pytest.param(True, False, False, id="flags-no_cov")]


@pytest.mark.parametrize("flags,cov,offset", RESIDUAL_CASES)
@pytest.mark.parametrize("n_e", [1, 63, 65, 257])
def test_residuals_equal_the_host_program(n_e, flags, cov, offset, tiny, host_exe, tmp_path):
    """gbp_post_residuals against the host program on the same inputs, bit for bit: residuals, reprojection covariances, the exact zeros
    of inactive edges; bases 16-byte aligned and 4 bytes past (the camera covariance's 16-byte and 4-byte loads).  The host program
    runs with trig = "device": the residual goes through eval_cam_rot's sinf / cosf, which IEEE 754 does not pin — with the host libm's
    the E = 257 cases differ in 8 and 17 of 514 residual words (the device library's cosf lies one ulp below glibc's for cameras 3 and 4
    of the tiny problem; nothing else differs) — so the twin evaluates the GPU library's algorithm (tests/sanitize/post_math_main.cpp)."""
    import torch
    from gbp_poplar_amd import post
    sub, K, z, active, b = _edge_case(tiny, n_e)
    n_c, n_l = sub["n_cams"], sub["n_lmks"]
    want = ps.run_host(host_exe, tmp_path, b, sub["cam_id"], sub["lmk_id"], K, z, active if flags else None, want_cov=cov, trig="device")
    lib = post.load()
    ins = [_dev(b[k], offset) for k in ps.BELIEFS]
    mo = [_out(w * (n_c if name.startswith("cam") else n_l), offset, dt) for name, w, dt in ps.OUTPUTS]
    assert lib.gbp_post_moments(_stream(), n_c, n_l, *[_ptr(v) for v, _ in ins], *[_ptr(v) for v, _ in mo]) == 0, lib.gbp_post_last_error()
    cam_mean, cam_cov, lmk_mean, lmk_cov = (v for v, _ in mo[:4])
    ids = [_dev(sub[k], offset)[0] for k in ("cam_id", "lmk_id")]
    zz, act = _dev(z, offset)[0], _dev(active, offset)[0]
    (res, res_big), (rc_, rc_big) = _out(2 * n_e, offset), _out(3 * n_e, offset)
    k9 = (C.c_float * 9)(*[float(x) for x in np.asarray(K).ravel()])
    rc = lib.gbp_post_residuals(_stream(), n_c, n_l, n_e, _ptr(ids[0]), _ptr(ids[1]), k9, _ptr(cam_mean), _ptr(lmk_mean), _ptr(zz),
                                _ptr(act) if flags else None, _ptr(cam_cov) if cov else None, _ptr(lmk_cov) if cov else None, _ptr(res),
                                _ptr(rc_) if cov else None)
    assert rc == 0, lib.gbp_post_last_error()
    torch.cuda.current_stream().synchronize()
    got_r, got_s = res.cpu().numpy(), rc_.cpu().numpy()
    assert _canaries_intact(res_big, 2 * n_e, offset) and _canaries_intact(rc_big, 3 * n_e, offset)
    if flags:      # inactive edges: exactly zero
        off = active == 0
        assert not got_r.reshape(-1, 2)[off].any() and (not cov or not got_s.reshape(-1, 3)[off].any())
    n_bad = int((got_r.view(np.uint32) != want["residual"].view(np.uint32)).sum())
    print("E %d: %d of %d residual words differ from the host program" % (n_e, n_bad, 2 * n_e))
    assert _same(got_r, want["residual"])
    if cov:
        assert _same(got_s, want["reproj_cov"])
    else:
        assert not got_s.any()      # untouched
    # the Python face: the same results from tensors
    out = post.residuals(ids[0], ids[1], K, {"cam_mean": cam_mean, "lmk_mean": lmk_mean}, zz, act if flags else None,
                         covs={"cam_cov": cam_cov, "lmk_cov": lmk_cov} if cov else None)
    torch.cuda.current_stream().synchronize()
    assert _same(out["residual"].cpu().numpy(), got_r) and (("reproj_cov" in out) == cov) and (not cov or _same(out["reproj_cov"].cpu().numpy(), got_s))


def _degenerate(bal, state):
    """two cameras and a tenth of the landmarks with a zero prior and every incident edge inactive: their belief stays the zero block"""
    cams, lmks = [3, 6], list(range(0, bal["n_lmks"], 10))
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    for c in cams:
        s["cam_priors_eta"][6 * c:6 * c + 6] = 0
        s["cam_priors_lambda"][36 * c:36 * c + 36] = 0
    for l in lmks:
        s["lmk_priors_eta"][3 * l:3 * l + 3] = 0
        s["lmk_priors_lambda"][9 * l:9 * l + 9] = 0
    s["active_flag"][np.isin(bal["cam_id"], cams) | np.isin(bal["lmk_id"], lmks)] = 0
    return s, cams, lmks


@pytest.mark.parametrize("mode", ["host_arrays", "device_on_torch_stream"])
def test_engine_solution_after_a_burst(mode):
    import torch
    from gbp_poplar_amd import hostlib, post
    bal = _all_to_all(8, 40)
    K, state, _ = _inputs(bal)
    state, bad_c, bad_l = _degenerate(bal, state)
    eng = _engine(bal, K)
    z, act = state["measurements"], state["active_flag"]
    if mode == "host_arrays":
        eng.upload(state)
        eng.linearise()
        eng.iterate(5)
        sol = eng.solution(z, act)
    else:      # the ctx on torch's stream: nothing synchronises; a marker kernel behind the call, then ONE wait for the stream
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            eng.upload(state)
            eng.linearise()
            eng.iterate(5)
            zd, ad = torch.from_numpy(np.ascontiguousarray(z, np.float32)).cuda(), torch.from_numpy(act.view(np.int32).copy()).cuda()
            torch.cuda.current_stream().synchronize()      # (the inputs' copies; nothing of the readout is queued yet)
            sol = eng.solution(zd, ad, device=True)
            marker = torch.ones(1, device="cuda") * 2.0
            torch.cuda.current_stream().synchronize()
            assert float(marker.cpu()[0]) == 2.0 and all(v.is_cuda for v in sol.values())
            sol = {k: (v.cpu().numpy().view(np.uint32) if k.endswith("status") else v.cpu().numpy()) for k, v in sol.items()}
    r = eng.read()
    m = post.moments(r)
    res = post.residuals(bal["cam_id"], bal["lmk_id"], K, m, z, act, covs=m)
    assert sorted(sol) == sorted(list(m) + list(res))
    for k in m:
        assert _same(sol[k], m[k]), k
    for k in res:
        assert _same(sol[k], res[k]), k
    with np.errstate(all="ignore"):
        cams, pts = hostlib.belief_means(bal["n_cams"], bal["n_lmks"], *[r[k] for k in ps.BELIEFS])
    assert _same(sol["cam_mean"].astype(np.float64), cams) and _same(sol["lmk_mean"].astype(np.float64), pts)
    status = np.concatenate([sol["cam_status"], sol["lmk_status"]])
    ev = eng.eval()
    assert int((status & 1).sum()) == ev["n_nonfinite"] and int((status >> 1 & 1).sum()) == ev["n_nonpd"], (ev, status.nonzero())
    assert np.flatnonzero(sol["cam_status"]).tolist() == bad_c and np.flatnonzero(sol["lmk_status"]).tolist() == bad_l
    assert ev["n_nonfinite"] == len(bad_c) + len(bad_l)
    eng.close()


def test_on_a_tree_the_covariances_are_the_exact_marginals():
    """the hub tree of tests/test_exact_inference.py, dmu_threshold = 0, diameter + 2 sweeps: GbpEngine.solution() against ref64.marginals"""
    from tests import test_exact_inference as tei
    bal, _ = tei.hub_tree()
    g = tei._Exact("A hub tree", bal, tei.diameter(bal) + tei.A_SWEEPS_OVER_DIAMETER, maxeta_damping=0.0)
    eng = tei._engine(bal, g.K, **g.params)
    eng.upload(g.state)
    eng.linearise()
    ex = g.exact(*eng.factor_potentials())
    eng.iterate(g.sweeps)
    sol = eng.solution()
    assert not sol["cam_status"].any() and not sol["lmk_status"].any()
    ps.tree_covariance_check(ex, sol, tei.A_BOUND, "engine")
    eng.close()


def _parse_cov_file(path):
    lines = open(path).read().splitlines()
    n_c, n_l = (int(x) for x in lines[0].split())
    assert len(lines) == 1 + n_c + n_l
    cams = np.array([[np.float32(x) for x in l.split()] for l in lines[1:1 + n_c]], np.float32).reshape(n_c, 42)
    lmks = np.array([[np.float32(x) for x in l.split()] for l in lines[1 + n_c:]], np.float32).reshape(n_l, 12)
    return {"cam_mean": cams[:, :6].ravel(), "cam_cov": cams[:, 6:].ravel(), "lmk_mean": lmks[:, :3].ravel(), "lmk_cov": lmks[:, 3:].ravel()}


def _untimed(stdout):
    return [l for l in stdout.splitlines() if "time" not in l.lower()]


def test_ba_cov_file(tmp_path):
    """`ba fr2robot2 --n_iters 50 --out_file a --cov_file b`: the stdout of the run without --cov_file (the lines that report times
    aside), C + L lines in b, and the values of engine.solution() after the same run to the nine printed digits (= every bit)"""
    from gbp_poplar_amd import driver, hostlib
    from tests.test_gpu_sharded_solution import _cli
    a, b, a2 = (str(tmp_path / n) for n in ("a.txt", "b.txt", "a2.txt"))
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "50", "--out_file"]
    rc, out, err = _cli(base + [a, "--cov_file", b])
    assert rc == 0, err[-2000:]
    rc2, out2, err2 = _cli(base + [a2])
    assert rc2 == 0, err2[-2000:]
    assert _untimed(out.replace(a, "A")) == _untimed(out2.replace(a2, "A"))
    got = _parse_cov_file(b)
    bal = hostlib.bal_read(seq_path("fr2robot2"))
    assert got["cam_mean"].size == 6 * bal["n_cams"] and got["lmk_mean"].size == 3 * bal["n_lmks"]
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    eng = _engine(bal, K)
    driver.run_ba(eng, state, opts, n_iters=50)
    sol = eng.solution()
    eng.close()
    for k in got:
        assert _same(got[k], sol[k]), k
    ref = hostlib.bal_read(a)      # --out_file of the same run: the same means
    assert _same(got["cam_mean"].astype(np.float64), ref["cameras"]) and _same(got["lmk_mean"].astype(np.float64), ref["points"])


def test_ba_cov_file_from_two_ranks(tmp_path):
    """--ipus 2: rank 0 writes the file from the gathered beliefs --out_file uses — the means of both files are the same numbers, every
    covariance is there and finite, with a positive diagonal"""
    from gbp_poplar_amd import hostlib
    from tests.test_gpu_sharded_solution import _cli
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    rc, out, err = _cli([BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "50", "--ipus", "2", "--transport", "host", "--out_file", a, "--cov_file", b])
    assert rc == 0, err[-2000:]
    got, ref = _parse_cov_file(b), hostlib.bal_read(a)
    assert _same(got["cam_mean"].astype(np.float64), ref["cameras"]) and _same(got["lmk_mean"].astype(np.float64), ref["points"])
    for k, w in (("cam_cov", 6), ("lmk_cov", 3)):
        cov = got[k].reshape(-1, w, w)
        assert np.isfinite(cov).all() and (np.diagonal(cov, axis1=1, axis2=2) > 0).all(), k


def test_sharded_solution_is_the_readout_of_the_gathered_read():
    """ShardedGbp.solution(gather=True) over two GbpEngine shards on the GPU (one thread per rank, the collective of
    tests/test_gpu_sharded_solution.py): every rank returns post.moments / post.residuals of its gathered read — the complete solution,
    the same bits on both ranks, no variable flagged."""
    import threading
    import torch
    from gbp_poplar_amd import driver, hostlib, post
    from gbp_poplar_amd.distributed import ShardedGbp
    from gbp_poplar_amd.engine import GbpEngine
    from tests.test_gpu_sharded_solution import _ThreadGroup
    bal = hostlib.synth_generate(14, 260, 5, 5)
    n_c, n_l, world = bal["n_cams"], bal["n_lmks"], 2
    opts = driver.Options()
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    bounds = [0, 101, n_l]
    shards = [ShardedGbp(GbpEngine(bal["cam_id"], bal["lmk_id"], n_c, n_l, K, shard=(r, world, bounds[r], bounds[r + 1])), n_c, r, world,
                         dist=None, device="cuda") for r in range(world)]

    def exchange():      # the all-gather of the camera partials, by device copies
        for sh in shards:
            sh.stream.synchronize()
        for dst in shards:
            for r, src in enumerate(shards):
                n = src.send.numel()
                dst.recv[r * n:(r + 1) * n].copy_(src.send)
        torch.cuda.synchronize()

    def everyone(*verbs):
        for sh in shards:
            for v in verbs:
                getattr(sh.e, v)()

    for sh in shards:
        sh.e.upload(state)
    everyone("refresh_begin")
    exchange()
    everyone("refresh_end", "linearise_factors")
    for _ in range(6):
        everyone("iterate_begin")
        exchange()
        everyone("iterate_end")
    group = _ThreadGroup(world)
    got, reads, errors = [None] * world, [None] * world, []

    def rank_runs(r):
        try:
            shards[r].dist = group.member(r)      # from here on the rank has a collective
            got[r] = shards[r].solution(state["measurements"], state["active_flag"], gather=True)
            reads[r] = shards[r].read(gather=True)
        except Exception as exc:      # noqa: BLE001 - reported by the main thread
            errors.append((r, repr(exc)))
            group.bar.abort()

    threads = [threading.Thread(target=rank_runs, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(90)
    assert not errors and not any(t.is_alive() for t in threads), errors
    want = post.moments(reads[0])
    want.update(post.residuals(bal["cam_id"], bal["lmk_id"], K, want, state["measurements"], state["active_flag"], covs=want))
    assert np.isfinite(want["lmk_cov"]).all() and want["residual"].any() and not want["cam_status"].any() and not want["lmk_status"].any()
    for r in range(world):
        assert sorted(got[r]) == sorted(want)
        for k, v in want.items():
            assert _same(got[r][k], v), (r, k)
