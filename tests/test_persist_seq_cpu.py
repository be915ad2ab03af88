"""The numbering of the persistent kernel's launches without a GPU: csrc/gbp_persist_seq.hpp turns the number of a ctx's last launch
into the next one, into the tags of its records and into "the shadows are cleared in front of this launch" — checked as a stand-alone
program under ASan + UBSan round every multiple of 2^19 and round 2^32."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_numbers_and_tags_under_asan_ubsan(tmp_path):
    """No launch is numbered 0 (the status word's "no launch failed") and no tag0 is 0 (the tag of a record nobody wrote): the numbers
    whose low 19 bits are zero are skipped, nothing else; a launch's 4 097 tags stay inside its own 8 192; inside a tag period of
    2^19 - 1 launches no tag0 comes twice and the period's first launch is announced exactly once; persist_seq_before orders numbers
    across the 32-bit wrap (tests/sanitize/persist_seq_main.cpp)."""
    exe = str(tmp_path / "persist_seq")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", os.path.join(ROOT, "tests", "sanitize", "persist_seq_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "persist_seq: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
