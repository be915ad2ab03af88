"""The pass planner of the loop drivers without a GPU: PassWalk (csrc/gbp_loop_plan.hpp) decides where gbp_iterate, gbp_ba_loop,
gbp_iterate_eval_each and the recovery of the persistent kernel cut the reference's loop into pieces and where its prior weakenings
fall — checked as a stand-alone program under ASan + UBSan against the loop as the reference writes it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pass_walk_equals_the_literal_loop_under_asan_ubsan(tmp_path):
    """Every n in 0..40 x i0 in 0..12 x steps in 0..8 x cap in {1, 2, 3, 7, 512, 4096} x weaken_inside in {0, 1}: the pieces tile the
    passes i0 .. i0 + n - 1 in order, none empty, none longer than cap; the weakenings in front of pieces plus those interior to pieces
    are the literal loop's `if ((i + 1) % 2 == 0 && i < 2 * steps)`, at the same positions; no interior weakening without weaken_inside;
    one piece with weaken_inside and cap >= n; none at all with steps = 0; and the same with steps2 up to 2^31 - 2 and loop indices round
    2^31 and 2^32 (tests/sanitize/loop_plan_main.cpp)."""
    exe = str(tmp_path / "loop_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", os.path.join(ROOT, "tests", "sanitize", "loop_plan_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "loop_plan: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
