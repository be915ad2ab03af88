"""What the ctx-less libraries' bindings (post.py, seed.py) share: checking the device tensors a call reads in place, their addresses, the
stream handle, and the staging of numpy arrays through the current GPU.  Nothing here converts or copies a device tensor."""
import ctypes as C

import numpy as np

from . import _cabi as cabi

F32, U32 = ("torch.float32",), ("torch.int32", "torch.uint32")


def device_of(arrays):
    dev = {a.device for a in arrays if cabi.is_device_tensor(a)}
    if len(dev) != 1:
        raise TypeError("expected torch tensors on ONE GPU, got %s" % (sorted(map(str, dev)) or "none"))
    return dev.pop()


def tensor(name, a, dtypes, count, device):
    """`a` as the library reads it: a contiguous tensor of one of `dtypes` with `count` elements on `device` (nothing is converted)"""
    if not cabi.is_device_tensor(a):
        raise TypeError("%s: a host array beside device tensors — one call takes host arrays or device tensors, not both" % name)
    if a.device != device:
        raise TypeError("%s is on %s, the other arrays on %s" % (name, a.device, device))
    if str(a.dtype) not in dtypes:
        raise TypeError("%s: dtype %s, expected %s (no silent conversion of device tensors)" % (name, a.dtype, dtypes[0]))
    if not a.is_contiguous():
        raise TypeError("%s is not contiguous (no silent copy of device tensors)" % name)
    if a.numel() != count:
        raise TypeError("%s has %d elements, expected %d" % (name, a.numel(), count))
    return a


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p()


def stream_handle(stream):
    import torch
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return int(getattr(stream, "cuda_stream", stream))


def to_device(a, ints, error, what):
    """a numpy array (or None) -> a flat tensor on the current GPU: float32, or the uint32 bits as int32.  Without a GPU: error(...),
    naming `what` runs there."""
    import torch
    if a is None:
        return None
    if not torch.cuda.is_available():
        raise error("no HIP device: %s runs on the GPU (there is no CPU path)" % what)
    a = np.ascontiguousarray(a, dtype=np.uint32 if ints else np.float32).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if ints else a).to("cuda")
