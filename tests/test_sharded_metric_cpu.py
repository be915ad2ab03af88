"""The sharded default loop without a GPU: the two pure functions behind it — whether the metric rides in the sharded iteration
(metric_rides, csrc/gbp_transport.hpp) and the CLIs' rank-order sum of a burst's metric records (csrc/gbp_metric_gather.hpp) — as a
stand-alone program under ASan + UBSan, and the spelling of the transports the CLIs accept."""
import os
import shutil
import subprocess

import pytest

from tests.test_cli import BA, ROOT, SLAM


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not (os.path.exists(BA) and os.path.exists(SLAM)):
        from gbp_poplar_amd import build
        build.build()


def run(cmd, timeout=60):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_metric_gather_and_decision_under_asan_ubsan(tmp_path):
    """metric_sum_ranks reproduces gbp_eval_global's arithmetic (every field as a double, acc = 0 + r0 + r1 ..., counters back through
    + 0.5) on hand-made records — world 1, 2, 8; a record of zeros; counters near 2^32; sums whose order matters in fp64, so a reversed
    order gives other bits — inside exactly the bytes the launcher maps; metric_rides answers every transport at world 1 and 4, non-hoisted,
    profiling and capturing, with a non-empty reason wherever it says no (tests/sanitize/metric_gather_main.cpp)."""
    exe = str(tmp_path / "metric_gather")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "metric_gather_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "metric_gather: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


def test_help_names_both_spellings_of_the_host_transport():
    for exe in (BA, SLAM):
        rc, out, _ = run([exe, "--help"])
        assert rc == 0 and "auto | rccl | host | p2p | p2p-slices | measured" in out and "host-staged" in out, exe


def test_transport_host_staged_is_parsed():
    """--transport host-staged (the name gbp_comm_transport reports) is the transport `host` names: both get past the parser, and the run
    then stops at the missing input file, not at the value."""
    for value in ("host", "host-staged", "2"):
        rc, _, err = run([BA, "--transport", value])
        assert rc == 1 and "--bal_file" in err and "invalid option value" not in err, (value, err)
        rc, _, err = run([SLAM, "--bal_file", "/nonexistent/file.txt", "--transport", value])
        assert rc == 1 and "unable to open file" in err and "invalid option value" not in err, (value, err)
    rc, _, err = run([BA, "--bal_file", "/nonexistent/file.txt", "--transport", "host-stagd"])
    assert rc == 1 and "invalid option value" in err
