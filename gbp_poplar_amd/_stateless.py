"""What the ctx-less libraries' bindings (post.py, seed.py, resect.py, locate.py) share.  A Binding is one library: where it is, how it
is loaded, its return-code check, its options, its host index.  A Call is one of its functions as a table: the arrays it reads, the
arrays it writes, how the counts follow, the C argument order; Binding.call does the rest — checking the device tensors a call reads in
place, their addresses, the stream handle, the outputs that were not passed, and the host round trip of a call that is given numpy
arrays (staged through the current GPU).  Nothing here converts or copies a device tensor."""
import collections
import ctypes as C
import os

import numpy as np

from . import _cabi as cabi
from ._loader import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
F32, U32 = ("torch.float32",), ("torch.int32", "torch.uint32")
VP, U32P, F32P = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)      # (device array pointers are passed as void*)


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


def k9(K):
    """the nine pin-hole entries as the float [9] the libraries take (host)"""
    return (C.c_float * 9)(*[float(x) for x in np.asarray(K, dtype=np.float64).reshape(9)])


def on_host(arrays):
    """does a call take the host round trip: none of its arrays (name -> array or None) is a device tensor"""
    return not any(cabi.is_device_tensor(a) for a in arrays.values())


def _host_u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return a, a.ctypes.data_as(U32P)


def index_dims(ids, start, item, start_name, n_name, **more):
    """the dimensions of a call on an index: "E" edges, `item` items, "<item> + 1" entries of the start array, and `more`"""
    if start.numel() == 0:
        raise TypeError("%s is empty: it has %s + 1 entries" % (start_name, n_name))
    return dict(more, **{"E": ids.numel(), item: start.numel() - 1, item + " + 1": start.numel()})


# One function of a library, as a table.
#   fn       its name
#   inputs   (name, "u32" | "f32", entries per unit, dimension[, True: may be None])
#   outputs  (name, "u32" | "f32", entries per unit, dimension[, the input without which it is neither allocated nor accepted])
#   dims     arrays -> {dimension: count}
#   args     the C argument list: "stream", "K", "opts", "workspace", a dimension or an array, in the header's order
#   options  the Options class, alloc: how an output that was not passed is made ("zeros", or "empty" where the call writes every
#   entry), returns: the inputs the result holds too (updated in place), workspace: (the export that sizes it, its dimension)
Call = collections.namedtuple("Call", "fn inputs outputs dims args options alloc returns workspace", defaults=(None, "zeros", (), None))
_KINDS = {"u32": U32, "f32": F32}


class Binding:
    """libgbp_mi355x_<name>.so: sigs (export -> (restype, argtypes): every symbol its header declares), its ABI version, the error a
    failure raises, and what has no CPU path (in the error for numpy arrays without a GPU)."""

    def __init__(self, name, sigs, abi_version, error, what):
        self.name, self.sigs, self.abi_version, self.error, self.what = name, sigs, abi_version, error, what
        self.LIB_PATH = os.path.join(HERE, "libgbp_mi355x_%s.so" % name)
        self._lib = None

    def symbols(self):
        return sorted(self.sigs)

    def load(self):
        if self._lib is None:
            self._lib = load_library(self.LIB_PATH, "gbp_%s_abi_version" % self.name, self.abi_version, self.sigs)
        return self._lib

    def check(self, rc, what, error=None):
        """a return code: error("<what>: <the library's text of the failure> (status <rc>)") unless it is GBP_OK"""
        if rc != 0:
            raise (error or self.error)("%s: %s (status %d)" % (what, getattr(self.load(), "gbp_%s_last_error" % self.name)().decode(), rc))

    def default_options(self, Options, **changes):
        o = Options()
        self.check(getattr(self.load(), "gbp_%s_default_options" % self.name)(C.byref(o)), "gbp_%s_default_options" % self.name)
        for k, v in changes.items():
            if k not in dict(Options._fields_):
                raise TypeError("gbp_%s_options has no field %r" % (self.name, k))
            setattr(o, k, v)
        return o

    def index(self, ids, n):
        """HOST.  (start [n + 1], edges [E]) uint32 of gbp_<name>_index"""
        fn = "gbp_%s_index" % self.name
        ids, p_ids = _host_u32(ids)
        start, edges = np.zeros(int(n) + 1, np.uint32), np.zeros(ids.size, np.uint32)
        self.check(getattr(self.load(), fn)(int(n), ids.size, p_ids, start.ctypes.data_as(U32P), edges.ctypes.data_as(U32P)), fn)
        return start, edges

    def check_index(self, start_name, start, edges, n_edges=None, error=None):
        """HOST.  gbp_<name>_check_index; edges None: start alone, against n_edges edges (default: its own last entry).  error: the
        class to raise (default: the library's own)"""
        fn = "gbp_%s_check_index" % self.name
        start, p_start = _host_u32(start)
        if start.size == 0:
            raise (error or self.error)("%s: %s is empty" % (fn, start_name))
        if edges is None:
            n_edges, p_edges = int(start[-1]) if n_edges is None else int(n_edges), None
        else:
            edges, p_edges = _host_u32(edges)
            n_edges = edges.size
        self.check(getattr(self.load(), fn)(start.size - 1, n_edges, p_start, p_edges), fn, error)

    def call(self, spec, arrays, K=None, options=None, out=None, stream=None, workspace=None, values=None, host_check=None):
        """spec.fn on `arrays` (name -> array or None, every input of spec).  Device tensors: they are checked, the outputs not in
        `out` are made, the call is queued on `stream`; -> {name: tensor} of spec.returns and the outputs.  numpy arrays: host_check()
        (the index) first, then the same staged through device tensors, one synchronise; -> the same dict as numpy, the integer outputs
        as uint32.  values: further dimensions (scalars of the C argument list)."""
        import torch
        out = dict(out or {})
        unknown = set(out) - {o[0] for o in spec.outputs}
        if unknown:
            raise TypeError("out: unknown arrays %s" % sorted(unknown))
        for o in spec.outputs:
            if o[0] in out and len(o) > 4 and arrays[o[4]] is None:
                raise TypeError("out: %s needs %s" % (o[0], o[4]))
        for s in spec.inputs:
            if len(s) == 4 and arrays[s[0]] is None:
                raise TypeError("%s is None: the call needs it" % s[0])
        both = dict(arrays, **out)      # (the two sets of names are disjoint)
        if on_host(both):
            if host_check:
                host_check()
            ints = {s[0] for s in spec.inputs + spec.outputs if s[1] == "u32"}
            staged = {k: to_device(v, k in ints, self.error, self.what) for k, v in both.items()}
            res = self.call(spec, {k: staged[k] for k in arrays}, K, options, {k: staged[k] for k in out}, stream, None, values)
            torch.cuda.synchronize()
            uints = {o[0] for o in spec.outputs if o[1] == "u32"}
            return {k: (v.cpu().numpy().view(np.uint32) if k in uints else v.cpu().numpy()) for k, v in res.items()}
        dev = device_of([a for a in both.values() if a is not None])
        d = dict(spec.dims(arrays), **(values or {}))
        t = {s[0]: None if arrays[s[0]] is None else tensor(s[0], arrays[s[0]], _KINDS[s[1]], s[2] * d[s[3]], dev) for s in spec.inputs}
        res = {k: t[k] for k in spec.returns}
        for o in spec.outputs:
            if o[0] in out:
                res[o[0]] = tensor(o[0], out[o[0]], _KINDS[o[1]], o[2] * d[o[3]], dev)
            elif len(o) == 4 or arrays[o[4]] is not None:
                res[o[0]] = getattr(torch, spec.alloc)(o[2] * d[o[3]], dtype=torch.int32 if o[1] == "u32" else torch.float32, device=dev)
        lib = self.load()
        if spec.workspace:
            need = int(getattr(lib, spec.workspace[0])(d[spec.workspace[1]]))
            if workspace is None:
                workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
            elif not cabi.is_device_tensor(workspace) or workspace.device != dev or workspace.numel() * workspace.element_size() < need:
                raise TypeError("workspace: expected a tensor of at least %d bytes on %s" % (need, dev))
        if spec.options:
            opts = options if options is not None else self.default_options(spec.options)
            if not isinstance(opts, spec.options):
                raise TypeError("options: expected a %s.Options (%s.default_options(...))" % (self.name, self.name))
        special = {"stream": lambda: VP(stream_handle(stream)), "K": lambda: k9(K), "opts": lambda: C.byref(opts), "workspace": lambda: ptr(workspace)}
        with torch.cuda.device(dev):      # (an absent array — an optional input, an output that is not made — is NULL)
            argv = [special[a]() if a in special else d[a] if a in d else ptr(res[a] if a in res else t.get(a)) for a in spec.args]
            self.check(getattr(lib, spec.fn)(*argv), spec.fn)
        return res
