"""The C-ABI checks every ctx-less library passes (tests/test_post_cpu.py, tests/test_seed_cpu.py): the library exports its public header
and nothing else, and every export is defined once, through the guard macros of gbp_poplar_amd/stateless/stateless_export.hpp."""
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
