"""Every device source names what it uses by #include: each helper header and kernel unit under csrc/kernels/, the four hook
files and the experiments file passes the device pass of hipcc ON ITS OWN (-fsyntax-only), with the product's -std and defines —
none of them may depend on the line of gbp_kernels.hip at which it is pasted in.  No GPU needed."""
import os
import subprocess

import pytest

from gbp_poplar_amd import build as b

UNITS = sorted(os.path.join("kernels", f) for f in os.listdir(os.path.join(b.CSRC, "kernels")))
HOOKS = sorted(os.path.join("hooks", f) for f in os.listdir(os.path.join(b.CSRC, "hooks")))
LAB = [os.path.join("experiments", "gbp_lab_kernels.hip")]


def _defines(rel):
    if rel in HOOKS:
        return ["-DGBP_BUILD_TEST_HOOKS"]
    if rel in LAB:
        return ["-DGBP_BUILD_EXPERIMENTS"]
    return []


@pytest.mark.parametrize("rel", UNITS + HOOKS + LAB)
def test_device_source_compiles_on_its_own(rel):
    try:
        hipcc = b.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not present")
    std = [f for f in b.FLAGS if f.startswith("-std=")]
    cmd = [hipcc, "--cuda-device-only", "-fsyntax-only", "--offload-arch=" + b.ARCH, "-x", "hip"] + std + _defines(rel) + \
          ["-Wno-pragma-once-outside-header", os.path.join(b.CSRC, rel)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout
