"""The harness of the stand-alone host twins (tests/sanitize/*_math_main.cpp: the arithmetic header of a ctx-less library compiled for
the host, run as a process, never loaded into python): how one is compiled, and how one is run on a flat input file."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")


def compile_host(main, exe, sanitize):
    """the host twin: g++, no FMA contraction (the device is built with -ffp-contract=off too); sanitize: ASan + UBSan"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-O1", "-ffp-contract=off", "-Wall",
                           "-Wno-unknown-pragmas", "-Wno-unused-function"] + san + [main, "-o", exe], cwd=ROOT)
    return exe


def run(exe, tmp, stem, parts, outputs, trig="libm", timeout=120):
    """`exe <tmp>/<stem>_in.bin <tmp>/<stem>_out.bin trig` on the arrays `parts`, written one after the other -> dict of the arrays
    the program wrote, cut from its output file by `outputs`: (name, dtype, elements) in file order, which must account for every byte.
    The program has to end with status 0 and its "<stem>_math: ok" line."""
    fin, fout = os.path.join(str(tmp), stem + "_in.bin"), os.path.join(str(tmp), stem + "_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(a.tobytes())
    p = subprocess.run([exe, fin, fout, trig], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0 and stem + "_math: ok" in p.stdout, (p.returncode, p.stdout[-300:], p.stderr[-3000:])
    raw = open(fout, "rb").read()
    out, at = {}, 0
    for name, dt, n in outputs:
        out[name] = np.frombuffer(raw, dt, n, at).copy()
        at += 4 * n
    assert at == len(raw)
    return out
