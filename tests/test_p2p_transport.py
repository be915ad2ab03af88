"""The direct peer-memory transport of the sharded camera exchange (`gbp_comm_init(ctx, region, 3)`, `--transport p2p`): every rank reads
its peers' partial sums straight out of their device memory (HIP IPC), one host barrier per exchange.  On one GPU the forked ranks are
separate processes, so IPC maps one process's buffer into another's exactly as across peer GPUs: every run here must compute what the
host-staged transport computes, bit for bit.  The ranks of the state comparison are fresh processes (tests/rank_worker.py) started by
the launcher the multi-process suites share (tests/rank_group.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import seq_path
from tests.rank_group import GROUPS
from tests.test_cli import BA, LINE, ROOT, SLAM, run


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


def _body(out, slam=False):
    """the lines that carry the run's numbers: initial metric, weakenings, per-iteration metric (slam: keyframes)"""
    keep = ("Initial", "Iters ", "Adding keyframe") if slam else ("Initial", "Weakening", "Iter ")
    return [l.strip() for l in out.splitlines() if l.strip().startswith(keep)]


# ---- CPU: the flag ----------------------------------------------------------------------------------------------------------------

def test_help_lists_p2p_transport():
    for exe in (BA, SLAM):
        rc, out, _ = run([exe, "--help"])
        assert rc == 0 and "--transport" in out and "auto | rccl | host | p2p" in out, exe


def test_transport_p2p_is_parsed():
    """--transport p2p (and its number, 3) gets past the parser: the run then stops at the missing input file, not at the value."""
    for value in ("p2p", "3"):
        rc, _, err = run([BA, "--transport", value])
        assert rc == 1 and "--bal_file" in err and "invalid option value" not in err, (value, err)
    rc, _, err = run([BA, "--bal_file", "/nonexistent/file.txt", "--transport", "p2p"])
    assert rc == 1 and "unable to open file" in err and "invalid option value" not in err


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_exchange_layout_under_asan_ubsan(tmp_path):
    """The layouts of the exchange buffer X and the result buffer R (csrc/gbp_comm.hpp) for world in {1, 2, 3, 8, 64} x C in {0, 1, 3, 5,
    1000}: X's 2 * world slots disjoint and tiling the buffer, parity 1 world * C * 44 floats behind parity 0, at least 16 bytes; R's
    parity ceil(C / world) records, every slice of slice_bounds fitting it — a stand-alone program under ASan + UBSan
    (tests/sanitize/exchange_layout_main.cpp)."""
    exe = str(tmp_path / "exchange_layout")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           os.path.join(ROOT, "tests", "sanitize", "exchange_layout_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "exchange_layout: ok (25 shapes)" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


# ---- GPU: the executables ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 8])
def test_ba_ipus_n_p2p_equals_host_staged(world):
    """`ba --ipus N --transport p2p` through the five weakenings and the relinearising sweeps (17+): the printed run is the host-staged
    transport's, line for line."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "24", "--ipus", str(world)]
    rc_h, out_h, err_h = run(base + ["--transport", "host"])
    rc_p, out_p, err_p = run(base + ["--transport", "p2p"])
    assert rc_h == 0, err_h[-2000:]
    assert rc_p == 0, err_p[-2000:]
    assert "Exchange between the %d ranks: p2p" % world in out_p
    body = _body(out_p)
    assert len(LINE.findall(out_p)) == 24 and sum(l.startswith("Weakening") for l in body) == 5
    assert body == _body(out_h)


@pytest.mark.gpu
def test_slam_ipus_2_p2p_equals_host_staged():
    """`slam --ipus 2 --transport p2p`: NEW_KEYFRAME after every 8 sweeps goes through the transport's all-gather; keyframe and
    iteration lines equal the host-staged run's."""
    base = [SLAM, "--bal_file", seq_path("fr2robot2"), "--iters_between_kfs", "8", "--ipus", "2"]
    rc_h, out_h, err_h = run(base + ["--transport", "host"])
    rc_p, out_p, err_p = run(base + ["--transport", "p2p"])
    assert rc_h == 0, err_h[-2000:]
    assert rc_p == 0, err_p[-2000:]
    assert "Exchange between the 2 ranks: p2p" in out_p
    body = _body(out_p, slam=True)
    assert sum("Adding keyframe" in l for l in body) == 18 and sum(l.startswith("Iters ") for l in body) > 0
    assert body == _body(out_h, slam=True)


@pytest.mark.gpu
def test_p2p_with_one_forked_rank_equals_plain_run():
    """--force_sharded 1 --transport p2p: a 1-rank communicator (its own buffer, no mapping): the run of the plain single-GPU ctx."""
    base = [BA, "--bal_file", seq_path("fr2robot2"), "--n_iters", "60", "--eval_every", "20"]
    rc1, out1, err1 = run(base)
    rc2, out2, err2 = run(base + ["--force_sharded", "1", "--transport", "p2p"])
    assert rc1 == 0 and rc2 == 0, (err1[-500:], err2[-1500:])
    assert "Exchange between the 1 ranks: p2p" in out2
    assert LINE.findall(out1) == LINE.findall(out2) and len(LINE.findall(out1)) == 3


# ---- GPU: the whole state, bit for bit, against the host-staged transport ---------------------------------------------------------

def _ranks(out_dir, world, transport):
    """`world` fresh processes (tests/rank_worker.py, scenario `iterate`) through the shared launcher; per rank (arrays, info)"""
    from gbp_poplar_amd import hostlib
    return GROUPS.ranks_of("tests.rank_worker", world, (transport, "iterate"), lambda: out_dir,
                           lambda: int(hostlib.bal_read(seq_path("fr2robot2"))["n_cams"]), 300)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_p2p_state_bit_identical_to_host_staged(world, tmp_path):
    """LINEARISE, 30 iterations, WEAKEN_PRIORS, 5 more, gbp_eval_global, gbp_comm_probe on `world` real processes: every rank's
    beliefs, damping, damping counts and robust flags are the host-staged transport's, bit for bit, and so are the global metric sums."""
    host = _ranks(str(tmp_path / "host"), world, 2)
    p2p = _ranks(str(tmp_path / "p2p"), world, 3)
    names = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")
    for r, ((a_h, i_h), (a_p, i_p)) in enumerate(zip(host, p2p)):
        assert i_h["describe"]["transport"] == "host-staged" and i_p["describe"]["transport"] == "p2p"
        assert i_p["describe"]["rank"] == r and i_p["describe"]["world"] == world
        assert i_p["probe_us"] > 0
        assert i_p["eval"] == i_h["eval"], r
        for k in names:
            assert np.array_equal(a_p[k], a_h[k]), (r, k)
    assert all(i["eval"] == p2p[0][1]["eval"] for _, i in p2p)      # gbp_eval_global: the same sums on every rank
    assert np.array_equal(p2p[0][0]["cam_beliefs_eta"], p2p[-1][0]["cam_beliefs_eta"])      # replicated cameras agree across ranks
