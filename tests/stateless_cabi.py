"""The C-ABI checks every ctx-less library passes (tests/test_post_cpu.py, tests/test_seed_cpu.py, tests/test_resect_cpu.py,
tests/test_locate_cpu.py, tests/test_stateless_cpu.py): the library exports its public header and nothing else, every export is defined
once, through the guard macros of gbp_poplar_amd/stateless/stateless_export.hpp, and the Python bindings call every export with the
header's parameter list."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gbp_poplar_amd")
MACROS = os.path.join(PKG, "stateless", "stateless_export.hpp")


def declared(header):
    """the gbp_* functions include/<header> declares, sorted"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:GBP_API\s+)?(?:const\s+char\s*\*|int|void|size_t)\s+(gbp_\w+)\s*\(", src, flags=re.M)))


def signatures(header):
    """name -> (kind of the return value, [kind per parameter]) of every gbp_* function include/<header> declares; a kind is "pointer"
    (an array parameter such as `const float K[9]` too), "uint32_t", "size_t", "int" or, for a return value, "void" """
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)

    def kind(text):
        if "*" in text or "[" in text:
            return "pointer"
        words = [w for w in text.split() if w != "const"]
        assert words and words[0] in ("uint32_t", "size_t", "int", "void"), text
        return words[0]

    out = {}
    for ret, name, params in re.findall(r"^\s*(?:GBP_API\s+)?((?:const\s+)?\w+\s*\*?)\s*(gbp_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = (kind(ret), [] if params == ["void"] else [kind(p) for p in params])
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_uint32: "uint32_t", C.c_size_t: "size_t", C.c_int: "int"}[t]


def check_signatures(module, header):
    """what ctypes was told of every export (module.load().<name>: restype, argtypes) is the header's declaration, kind by kind"""
    declared_sigs = signatures(header)
    assert sorted(declared_sigs) == declared(header) == module.symbols()
    lib = module.load()
    for name, (ret, params) in declared_sigs.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, len(fn.argtypes or ()), len(params))
        assert [_ctypes_kind(t) for t in fn.argtypes] == params, (name, params)
        assert _ctypes_kind(fn.restype) == ret, (name, fn.restype, ret)


def check_exports(module, header, exports, abi_version):
    """header == exports == module.symbols() == `nm -D` of the library; the library's and the module's ABI version are abi_version"""
    assert declared(header) == exports == module.symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", module.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == set(exports)
    name = os.path.basename(module.LIB_PATH)[len("libgbp_mi355x_"):-len(".so")]
    assert getattr(module.load(), "gbp_%s_abi_version" % name)() == getattr(module, "GBP_%s_ABI_VERSION" % name.upper()) == abi_version


def check_guard(name, header, exports):
    """Every export of library `name` (sources: gbp_poplar_amd/<name>/) is defined exactly once, through GBP_STATELESS_EXPORT[_T]; no
    file of the library says `extern "C"` or defines a gbp_* function plainly; the macros catch everything; nothing of the library is
    defined inside csrc/ (whose every *.cpp goes into the core library)."""
    src_dir = os.path.join(PKG, name)
    defined, stray = {}, []
    for f in sorted(os.listdir(src_dir)):
        if not f.endswith((".cpp", ".hip", ".hpp")):
            continue
        src = re.sub(r"//[^\n]*", "", open(os.path.join(src_dir, f)).read())
        for m in re.finditer(r"^GBP_STATELESS_EXPORT(?:_T)?\(\s*(?:[^,()]+,\s*[^,]+,\s*)?(gbp_\w+)\s*,", src, flags=re.M):
            defined.setdefault(m.group(1), []).append(f)
        if 'extern "C"' in src:
            stray.append(f)
        stray += ["%s: %s" % (f, m.group(1)) for m in re.finditer(r"^(?:int|void|size_t|const char\s*\*)\s+(gbp_\w+)\s*\(", src, flags=re.M)]
    assert not stray, stray
    assert set(defined) == set(declared(header)) == set(exports) and all(len(v) == 1 for v in defined.values()), defined
    macro = open(MACROS).read()
    assert macro.count("catch (...)") >= 2 and "guarded(#name" in macro
    for dirpath, _, files in os.walk(os.path.join(PKG, "csrc")):
        for f in files:
            assert "gbp_%s_" % name not in open(os.path.join(dirpath, f)).read() or f == "cli_common.hpp", f
