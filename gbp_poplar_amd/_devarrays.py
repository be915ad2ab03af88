"""What the ctx-less libraries' bindings (post.py, seed.py) share: checking the device tensors a call reads in place, their addresses, the
stream handle, the return-code check, and the host round trip of a call that is given numpy arrays (staged through the current GPU).
Nothing here converts or copies a device tensor."""
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


def check(rc, what, last_error, error):
    """a library's return code: error("<what>: <the library's text of the failure> (status <rc>)") unless it is GBP_OK"""
    if rc != 0:
        raise error("%s: %s (status %d)" % (what, last_error().decode(), rc))


def k9(K):
    """the nine pin-hole entries as the float [9] the libraries take (host)"""
    return (C.c_float * 9)(*[float(x) for x in np.asarray(K, dtype=np.float64).reshape(9)])


def on_host(arrays):
    """does a call take the host round trip: none of its arrays (name -> array or None) is a device tensor"""
    return not any(cabi.is_device_tensor(a) for a in arrays.values())


def round_trip(arrays, ints, device_form, uints, error, what):
    """The numpy face of a call: stage `arrays` (those named in `ints` as uint32 bits; error, what: see to_device), run
    device_form(staged), wait until every stream of the GPU has finished, and hand its results (a dict or a tuple of tensors) back as
    numpy, the ones named in `uints` as uint32."""
    import torch
    res = device_form({k: to_device(v, k in ints, error, what) for k, v in arrays.items()})
    torch.cuda.synchronize()
    if isinstance(res, dict):
        return {k: (v.cpu().numpy().view(np.uint32) if k in uints else v.cpu().numpy()) for k, v in res.items()}
    return tuple(v.cpu().numpy() for v in res)
