"""What the ctx-less libraries get from gbp_poplar_amd/stateless/stateless_export.hpp, without a GPU: ONE header defines the error text,
yet libgbp_mi355x_post.so and libgbp_mi355x_seed.so, loaded into one process as every Python user and bin/ba, bin/slam load them, each
keep a text of their own, per thread.  The failing calls fail their argument checks, which precede every HIP call.  What all four
libraries (post, seed, resect, locate) get from stateless/ and gbp_poplar_amd/_stateless.py: the ctypes signatures of the bindings are
the public headers' (tests/stateless_cabi.py), and the shared host index is right under the sanitizers, as a program of its own."""
import ctypes as C
import os
import subprocess
import threading

import pytest

from tests import host_twin, stateless_cabi

P = C.c_void_p(64)      # any non-NULL address: a call that fails its argument checks touches neither the array nor HIP


def _libs():
    from gbp_poplar_amd import post, seed
    return post.load(), seed.load()


def _post_fails(post):
    assert post.gbp_post_moments(None, 2, 3, None, *[P] * 9) == -1                      # cam_eta is NULL


def _post_succeeds(post):
    assert post.gbp_post_moments(None, 0, 0, *[None] * 10) == 0                         # no variable: nothing to launch


def _seed_fails(seed):
    assert seed.gbp_seed_keyframe(None, 3, 3, 2, P, P, P, P, P) == -1                   # src is not below n_cams


def _seed_succeeds(seed):
    assert seed.gbp_seed_landmarks(None, 0, 0, 0, None, None, None, (C.c_float * 9)(), *[None] * 11) == 0      # no landmark


def _both_directions():
    """-> the two texts the calling thread is left with: the readout's names cam_eta, the seeding's src"""
    post, seed = _libs()
    _post_succeeds(post)
    _seed_succeeds(seed)
    assert post.gbp_post_last_error() == b"" and seed.gbp_seed_last_error() == b""
    _seed_fails(seed)
    seed_text = seed.gbp_seed_last_error()
    assert post.gbp_post_last_error() == b"" and seed_text.startswith(b"gbp_seed_keyframe:") and b"src" in seed_text
    _post_succeeds(post)                                 # a success clears only its own library's text
    assert post.gbp_post_last_error() == b"" and seed.gbp_seed_last_error() == seed_text
    _seed_succeeds(seed)
    assert seed.gbp_seed_last_error() == b""
    _post_fails(post)
    post_text = post.gbp_post_last_error()
    assert seed.gbp_seed_last_error() == b"" and post_text.startswith(b"gbp_post_moments:") and b"cam_eta" in post_text
    _seed_succeeds(seed)
    assert post.gbp_post_last_error() == post_text and seed.gbp_seed_last_error() == b""
    _seed_fails(seed)
    assert post.gbp_post_last_error() == post_text and seed.gbp_seed_last_error() == seed_text
    return post_text, seed_text


def test_a_failure_of_one_library_is_not_in_the_others_text():
    _both_directions()


def test_a_second_thread_has_texts_of_its_own():
    post, seed = _libs()
    mine = _both_directions()
    seen = {}

    def second():
        try:
            seen["start"] = (post.gbp_post_last_error(), seed.gbp_seed_last_error())      # before this thread's first call
            seen["end"] = _both_directions()
            _post_succeeds(post)                         # ... and leaves empty texts behind: the first thread's must not follow
            _seed_succeeds(seed)
        except BaseException as e:      # noqa: B902 — handed to the test's thread
            seen["error"] = e

    t = threading.Thread(target=second)
    t.start()
    t.join()
    assert "error" not in seen, seen["error"]
    assert seen["start"] == (b"", b"") and seen["end"] == mine
    assert (post.gbp_post_last_error(), seed.gbp_seed_last_error()) == mine


LIBRARIES = ["post", "seed", "resect", "locate"]


@pytest.mark.parametrize("name", LIBRARIES)
def test_the_bindings_call_every_export_with_the_headers_parameter_list(name):
    """per export: as many ctypes argtypes as the public header declares parameters, each of the header's kind (pointer — an array
    parameter and the options pointer too —, uint32_t, size_t, int), and the restype of the declared return value"""
    import importlib
    stateless_cabi.check_signatures(importlib.import_module("gbp_poplar_amd." + name), "gbp_mi355x_%s.h" % name)


def test_index_and_its_check_under_the_sanitizers(tmp_path):
    """gbp_poplar_amd/stateless/stateless_index.hpp compiled for the host under ASan + UBSan into a program of its own
    (tests/sanitize/stateless_index_main.cpp: the cases and the expected texts are there), run as a process"""
    exe = host_twin.compile_host(os.path.join("tests", "sanitize", "stateless_index_main.cpp"), str(tmp_path / "stateless_index"), sanitize=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "stateless_index: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
