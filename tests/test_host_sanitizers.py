"""AddressSanitizer + UBSan over the CPU-side C/C++ (the whole host side of the C-ABI library — gbp_api_*.cpp with the device code stubbed out, negative
tests of every export that needs no device —, the host helpers, the device-order builder of gbp_create and the oracle).  GPU sanitizers are
not available on this pool, so this is the memory-safety gate of everything that runs on the host; the harness is
tests/sanitize/host_sanitize_main.cpp.  The same host side under eight threads that call gbp_create at once — the per-thread creation error —
is tests/sanitize/create_threads_main.cpp, under ThreadSanitizer and under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

from gbp_poplar_amd import build      # the recipe only: importing it loads no library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


CXX = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-DGBP_BUILD_TEST_HOOKS", "-I/opt/rocm/include", "-c"]
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lm", "-pthread", "-Wl,-rpath,/opt/rocm/lib"]
# The GPUs are hidden from the children (their env only), so that gbp_create finds none on any machine and no harness ever holds a ctx
# that could launch.  Observed on an MI355X machine with the ordinary library: gbp_device_count() = 1 as the machine is set up,
# 0 under ROCR_VISIBLE_DEVICES=-1 and HIP_VISIBLE_DEVICES=-1 (either alone gives 0 as well).
NO_GPU = {"ROCR_VISIBLE_DEVICES": "-1", "HIP_VISIBLE_DEVICES": "-1"}


def _compile(srcs, san, out_dir):
    from concurrent.futures import ThreadPoolExecutor

    def one(src):
        obj = os.path.join(out_dir, os.path.basename(src) + ".o")
        subprocess.check_call(CXX + list(san) + [src, "-o", obj], cwd=ROOT)
        return obj
    with ThreadPoolExecutor(4) as ex:
        return list(ex.map(one, srcs))


@pytest.fixture(scope="module")
def library_objects(tmp_path_factory):
    """The host side of the library — build.HOST_SRCS — and tests/sanitize/kernel_stubs.cpp in place of its device code, compiled once per
    set of sanitizer flags: -> the object files"""
    made = {}

    def objects(san):
        key = tuple(san)
        if key not in made:
            srcs = [os.path.join(build.CSRC, f) for f in build.HOST_SRCS] + [os.path.join(ROOT, "tests", "sanitize", "kernel_stubs.cpp")]
            made[key] = _compile(srcs, san, str(tmp_path_factory.mktemp("host_objects")))
        return list(made[key])
    return objects


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_code_and_oracle_under_asan_ubsan(tmp_path, library_objects):
    exe = str(tmp_path / "host_sanitize")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-ffp-contract=off"]
    objs = []
    for src in ("oracle/oracle_gbp.c", "oracle/oracle_math.c"):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call(["gcc", "-std=c11", "-c", os.path.join(ROOT, src), "-o", obj] + san, cwd=ROOT)
        objs.append(obj)
    # The host side of the library itself — build.HOST_SRCS, every translation unit of the product but the device code: the C-ABI
    # (gbp_api_*.cpp), the device order, the transports of the multi-rank exchange, the host helpers — compiled with g++ under the
    # sanitizers; the device code is replaced by tests/sanitize/kernel_stubs.cpp (every launcher aborts: nothing here may reach a launch;
    # a launcher that gbp_kernels.h declares and the stubs lack, or declare otherwise, fails the link below), the HIP / RCCL headers and
    # libamdhip64 are on the image.  api_negative.cpp calls every export that needs no device with NULL / negative / out-of-order arguments.
    harness = [os.path.join(ROOT, "tests", "sanitize", f) for f in ("layout_sanitize.cpp", "api_negative.cpp", "host_sanitize_main.cpp")]
    cxx_objs = library_objects(san) + _compile(harness, san, str(tmp_path))
    subprocess.check_call(["g++"] + cxx_objs + objs + san + LINK + ["-o", exe], cwd=ROOT)
    # The GPUs are hidden from the child (NO_GPU).  With a driver but no visible GPU the ROCr runtime leaves two small allocations of its
    # own at exit: tests/sanitize/lsan.supp names that library and nothing else.
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "sanitize", "lsan.supp"), **NO_GPU)
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "sanitize: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_gbp_create_from_eight_threads(sanitizer, tmp_path, library_objects):
    """gbp_last_error(NULL) belongs to the calling thread: eight threads make creations that fail for different reasons (invalid problems
    and a valid one that finds no device) and each reads its own text — tests/sanitize/create_threads_main.cpp, a stand-alone program over
    the host side of the library and the kernel stubs, once under ThreadSanitizer and once under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "create_threads")
    san = ["-fsanitize=" + sanitizer, "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    if sanitizer != "thread":
        san.insert(1, "-fno-sanitize-recover=all")      # (the flags of the test above: its objects are used again)
    main = _compile([os.path.join(ROOT, "tests", "sanitize", "create_threads_main.cpp")], san, str(tmp_path))
    subprocess.check_call(["g++"] + library_objects(san) + main + san + LINK + ["-o", exe], cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "sanitize", "lsan.supp"), **NO_GPU)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    if sanitizer == "thread" and "unexpected memory mapping" in p.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow on this kernel")
    assert p.returncode == 0 and "create_threads: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_threaded_host_code_under_tsan(tmp_path):
    """The host code that runs on several threads — the file reader (one piece of the file per thread) and the prior strengths (one range
    of factors per thread) — under ThreadSanitizer: results equal to the single-threaded ones, no report (tests/sanitize/host_threads_main.cpp)."""
    exe = str(tmp_path / "host_threads")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=thread", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           os.path.join(ROOT, "gbp_poplar_amd", "csrc", "gbp_host.cpp"), os.path.join(ROOT, "tests", "sanitize", "host_threads_main.cpp"), "-o", exe], cwd=ROOT)
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    if "unexpected memory mapping" in p.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow on this kernel")
    assert p.returncode == 0 and "tsan: ok" in p.stdout and "ThreadSanitizer" not in p.stderr, (p.returncode, p.stdout[-300:], p.stderr[-3000:])
