"""Device-resident arrays, the part that needs no GPU: the argument checks GbpEngine makes before a device tensor reaches the C-ABI
(torch's `meta` device stands in for the GPU: nothing is allocated, no device is initialised), and the ISA metadata of the kernels
behind the device-pointer calls (no scratch, no spills)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
C_, L_, E_ = 3, 5, 7


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the C-ABI was reached (%s): the arguments should have been refused before" % name)


def _engine():
    """a GbpEngine without a ctx: only its argument checking can run"""
    from gbp_poplar_amd.engine import GbpEngine
    e = GbpEngine.__new__(GbpEngine)
    e.C, e.L, e.E, e.h, e.lib = C_, L_, E_, None, _NoLibrary()
    return e


def _state(device="meta"):
    import torch
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=device)
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=device)
    return {"damping": f(E_), "damping_count": i(E_), "active_flag": i(E_), "cam_scaling": f(C_), "lmk_scaling": f(L_),
            "cam_weaken_flag": i(C_), "lmk_weaken_flag": i(L_), "cam_priors_eta": f(6 * C_), "cam_priors_lambda": f(36 * C_),
            "lmk_priors_eta": f(3 * L_), "lmk_priors_lambda": f(9 * L_), "measurements": f(2 * E_), "meas_variances": f(E_)}


def test_well_formed_device_tensors_pass_the_checks():
    from gbp_poplar_amd import _cabi as cabi
    import torch
    keep = []
    s = cabi.fill_struct_device(cabi.GbpStateIn(), _state(), _engine()._sizes(), torch.device("meta"), keep)
    assert len(keep) == 13 and not s.mu and not s.oldmu


@pytest.mark.parametrize("call", ["upload", "new_keyframe", "read", "read_priors"])
def test_wrong_dtype_is_refused(call):
    import torch
    e = _engine()
    if call == "upload":
        bad = dict(_state(), measurements=torch.zeros(2 * E_, dtype=torch.float64, device="meta"))
        with pytest.raises(TypeError, match="measurements.*float64"):
            e.upload(bad)
    elif call == "new_keyframe":
        with pytest.raises(TypeError, match="damping_count.*float32"):
            e.new_keyframe({"damping_count": torch.zeros(E_, dtype=torch.float32, device="meta")})
    elif call == "read":
        with pytest.raises(TypeError, match="robust_flag.*int64"):
            e.read(out={"robust_flag": torch.zeros(E_, dtype=torch.int64, device="meta")})
    else:
        with pytest.raises(TypeError, match="cam_priors_eta.*float16"):
            e.read_priors(out={"cam_priors_eta": torch.zeros(6 * C_, dtype=torch.float16, device="meta")})


def test_non_contiguous_tensor_is_refused_not_copied():
    import torch
    e = _engine()
    strided = torch.zeros(2 * 6 * C_, dtype=torch.float32, device="meta")[::2]
    assert strided.numel() == 6 * C_ and not strided.is_contiguous()
    with pytest.raises(TypeError, match="cam_priors_eta is not contiguous"):
        e.upload(dict(_state(), cam_priors_eta=strided))
    with pytest.raises(TypeError, match="cam_beliefs_eta is not contiguous"):
        e.read(out={"cam_beliefs_eta": strided})


def test_host_and_device_members_in_one_call_are_refused():
    import torch
    e = _engine()
    with pytest.raises(TypeError, match="meas_variances: a host array beside device tensors"):
        e.upload(dict(_state(), meas_variances=np.zeros(E_, np.float32)))
    with pytest.raises(TypeError, match="active_flag: a host array beside device tensors"):
        e.new_keyframe({"damping_count": torch.zeros(E_, dtype=torch.int32, device="meta"), "active_flag": torch.zeros(E_, dtype=torch.int32)})
    with pytest.raises(TypeError, match="torch tensors on the engine's GPU"):
        e.read(out={"damping": np.zeros(E_, np.float32)})


def test_wrong_size_and_unknown_member_are_refused():
    import torch
    e = _engine()
    with pytest.raises(TypeError, match="lmk_priors_lambda has 44 elements, expected 45"):
        e.upload(dict(_state(), lmk_priors_lambda=torch.zeros(44, dtype=torch.float32, device="meta")))
    with pytest.raises(TypeError, match="no member 'beliefs'"):
        e.read(out={"beliefs": torch.zeros(4, device="meta")})


def test_host_arrays_take_the_path_they_always_took():
    """numpy arrays (and CPU tensors) are not device tensors: they go through fill_struct, conversions included, as before"""
    import torch
    from gbp_poplar_amd import _cabi as cabi
    assert not cabi.any_device_tensor({"a": np.zeros(3), "b": torch.zeros(3), "c": None})
    assert cabi.any_device_tensor({"a": np.zeros(3), "b": torch.zeros(3, device="meta")})
    keep = []
    s = cabi.fill_struct(cabi.GbpStateIn(), {"damping": np.zeros(E_, np.float64)}, keep)
    assert keep[0].dtype == np.float32 and s.damping and not s.mu


DEVICE_IO_KERNELS = ("k_upload_dev", "k_read_state_dev", "k_keyframe_state_dev", "k_rec_copy")


@pytest.mark.parametrize("libname", ["libgbp_mi355x.so", "libgbp_mi355x_test.so"])
def test_device_io_kernels_use_no_scratch_and_spill_nothing(libname):
    """from the gfx950 code object's metadata (amdhsa.kernels notes): private segment 0, no SGPR / VGPR spills"""
    lib = os.path.join(ROOT, "gbp_poplar_amd", libname)
    if not os.path.exists(lib) or not os.path.exists(READELF):
        pytest.skip("library or llvm-readelf not present")
    tmp = tempfile.mkdtemp(prefix="gbp_isa_")
    try:
        shutil.copy(lib, tmp)
        subprocess.run([OBJDUMP, "--offloading", libname], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert len(co) == 1, os.listdir(tmp)
        notes = subprocess.run([READELF, "--notes", co[0]], cwd=tmp, check=True, stdout=subprocess.PIPE, text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m or not any(k in m.group(1) for k in DEVICE_IO_KERNELS):
            continue
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")}
        found[m.group(1)] = vals
        assert vals == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (m.group(1), vals)
    assert len(found) == 5, sorted(found)      # k_rec_copy<true> and <false>
