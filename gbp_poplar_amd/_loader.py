"""How every native library of the package is loaded (_lib.py, post.py, seed.py, resect.py, locate.py).  There is no CPU fallback: a library that is missing,
stale or lacks a declared symbol fails loudly."""
import ctypes as C
import os


def load_library(path, abi_symbol, abi_version, sigs):
    """CDLL(path) with every function of `sigs` (name -> (restype, argtypes)) bound, after `abi_symbol`() has answered `abi_version`."""
    if not os.path.exists(path):
        raise RuntimeError(
            "native library %s is missing — build it with `python -m gbp_poplar_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback." % path)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and dlopens it by path, so
    # if this library (linked against /opt/rocm's copy) initialised the GPU first, a later `import torch`
    # would bring up a second runtime that finds "No HIP GPUs".  Loading torch's runtime first makes our
    # DT_NEEDED libamdhip64.so.7 resolve to the copy already in the process.  (The C++ CLIs never load torch.)
    if os.environ.get("GBP_NO_TORCH") != "1":
        try:
            import torch
            torch.cuda.is_available()
        except ImportError:
            pass
    lib = C.CDLL(path)
    abi = getattr(lib, abi_symbol)      # first: a stale .so gets the rebuild message, not an AttributeError for a new symbol
    abi.restype = C.c_int
    abi.argtypes = []
    if abi() != abi_version:
        raise RuntimeError("%s has ABI version %d, these bindings were written for %d — rebuild (python -m gbp_poplar_amd.build)"
                           % (path, abi(), abi_version))
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib
