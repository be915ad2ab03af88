"""Build recipe of the native library (in-tree, gfx950 only).

    python -m gbp_poplar_amd.build        -> gbp_poplar_amd/libgbp_mi355x.so       the product (+ bin/ba, bin/slam, bin/bal_convert)
                                             gbp_poplar_amd/libgbp_mi355x_test.so  the same sources + the test hooks of
                                                                                   include/gbp_mi355x_debug.h (tests/ only)
                                             gbp_poplar_amd/libgbp_mi355x_post.so  the solution readout (post/, include/gbp_mi355x_post.h)
                                             gbp_poplar_amd/libgbp_mi355x_seed.so  landmark / keyframe seeding (seed/, include/gbp_mi355x_seed.h)
                                             gbp_poplar_amd/libgbp_mi355x_resect.so  camera resection (resect/, include/gbp_mi355x_resect.h)
                                             gbp_poplar_amd/libgbp_mi355x_locate.so  camera location with no pose guess (locate/, include/gbp_mi355x_locate.h)
    python -m gbp_poplar_amd.build --experiments
                                          -> gbp_poplar_amd/libgbp_mi355x_exp.so   + csrc/experiments/: timing ablations / mapping
                                                                                   experiments (profiles/*.py only)

hipcc cross-compiles for gfx950 without a GPU.  -ffp-contract=off: results are compared
bit-for-bit with the CPU oracle, so no FMA contraction on either side.

Every translation unit is compiled to an object of its own (gbp_poplar_amd/_obj/<variant>/, in parallel, only when it or a
header changed) and the objects are linked: the device code (gbp_kernels.hip = the units of csrc/kernels/ as ONE translation unit,
~25 s) is not recompiled for an edit of the host side of the C-ABI, whose translation units are plain C++ (no device pass).  The
objects of all the variants asked for, and those of the ctx-less libraries (SATELLITES: a table entry each, one recipe), are
compiled in one pool.
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "_obj")
LIB = os.path.join(HERE, "libgbp_mi355x.so")
TEST_LIB = os.path.join(HERE, "libgbp_mi355x_test.so")  # + gbp_debug_* (include/gbp_mi355x_debug.h): what tests/ load for stage-level checks
EXP_LIB = os.path.join(HERE, "libgbp_mi355x_exp.so")    # + timing ablations and mapping experiments (profiles/*.py only)
POST_LIB = os.path.join(HERE, "libgbp_mi355x_post.so")  # the solution readout
SEED_LIB = os.path.join(HERE, "libgbp_mi355x_seed.so")  # landmark / keyframe seeding
RESECT_LIB = os.path.join(HERE, "libgbp_mi355x_resect.so")  # camera resection against the map
LOCATE_LIB = os.path.join(HERE, "libgbp_mi355x_locate.so")  # camera location with no pose guess
# The libraries without a ctx, each one HIP translation unit with the product's flags and an export map of its own:
# name (= its directory under _obj/) -> (source directory, source, export map, library).  stateless/ is what they share.
STATELESS = os.path.join(HERE, "stateless")
SATELLITES = {
    "post": (os.path.join(HERE, "post"), "gbp_post.hip", "gbp_post_exports.map", POST_LIB),
    "seed": (os.path.join(HERE, "seed"), "gbp_seed.hip", "gbp_seed_exports.map", SEED_LIB),
    "resect": (os.path.join(HERE, "resect"), "gbp_resect.hip", "gbp_resect_exports.map", RESECT_LIB),
    "locate": (os.path.join(HERE, "locate"), "gbp_locate.hip", "gbp_locate_exports.map", LOCATE_LIB),
}
SATELLITE_USES = {"locate": ["resect"]}      # the satellites whose headers a satellite includes
BIN = os.path.join(HERE, "bin")
ARCH = "gfx950"
# -fvisibility=hidden: the library exports the gbp_* functions of include/*.h (GBP_API) and nothing else
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
DEVICE_SRCS = ["gbp_kernels.hip"]                        # HIP: host + gfx950 device pass
# the C-ABI (gbp_ctx.hpp names what each holds), the device order, the exchange transports, the host helpers: plain C++.
# The rule (the Makefile states the same one): every csrc/*.cpp that is not the main of a CLI
HOST_SRCS = sorted(f for f in os.listdir(CSRC) if f.endswith(".cpp") and not f.endswith("_main.cpp"))
LIB_SRCS = DEVICE_SRCS + HOST_SRCS
CLI_SRCS = {"ba": "ba_main.cpp", "slam": "slam_main.cpp", "bal_convert": "bal_convert_main.cpp"}


def hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP extension cannot be built (there is no CPU fallback)")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _headers():
    """Every file under csrc/ that is not itself a compiled translation unit (a csrc/*.cpp, gbp_kernels.hip): the headers, the
    kernel units, hooks and experiments that gbp_kernels.hip #includes, the export map.  (The Makefile states the same rule.)"""
    inc = os.path.join(HERE, "..", "include")
    hdr = [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs
           if not (d == CSRC and (f.endswith(".cpp") or f in DEVICE_SRCS))]
    return hdr + [os.path.join(inc, f) for f in os.listdir(inc)] + [os.path.abspath(__file__)]


def _deps():
    """every file a library depends on (bench.py stamps its traffic figures with a hash over these)"""
    return sorted(set([os.path.join(CSRC, s) for s in LIB_SRCS] + _headers()))


def _compile(src, obj, defines, verbose):
    cmd = [hipcc(), "-c", "-o", obj] + FLAGS + defines
    if src.endswith(".hip"):
        cmd += ["--offload-arch=" + ARCH, "-x", "hip"]
    else:
        cmd += ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc()))), "include")]
    cmd.append(src)
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


# variant (= its directory under _obj/) -> the library, the defines of its objects
VARIANTS = {
    "product": (LIB, []),
    "test": (TEST_LIB, ["-DGBP_BUILD_TEST_HOOKS"]),
    "exp": (EXP_LIB, ["-DGBP_BUILD_EXPERIMENTS", "-DGBP_BUILD_TEST_HOOKS"]),
}


def _stale_objects(name, srcs, deps, force):
    """(every object of library `name` (under _obj/<name>/), [(source, object)] of those that have to be compiled): an object is
    stale against its own source and `deps`"""
    odir = os.path.join(OBJ, name)
    os.makedirs(odir, exist_ok=True)
    objs, todo = [], []
    for s in srcs:
        obj = os.path.join(odir, os.path.splitext(os.path.basename(s))[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, deps + [s]):
            todo.append((s, obj))
    return objs, todo


def _link(target, objs, export_map, extra, verbose):
    cmd = [hipcc(), "-shared", "-o", target, "--offload-arch=" + ARCH] + objs + extra + ["-Wl,--version-script=" + export_map]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _recipes(variants, satellites):
    """library -> (name, sources, what its objects depend on beside their source, defines, export map, extra link flags)"""
    hdr = _headers()
    out = {}
    for v in variants:      # (-pthread: the host helpers' reader threads, for a libc that still keeps them in libpthread)
        lib, defines = VARIANTS[v]
        out[lib] = (v, [os.path.join(CSRC, s) for s in LIB_SRCS], hdr, defines, os.path.join(CSRC, "gbp_exports.map"), ["-ldl", "-pthread"])
    for n in satellites:    # stale against its own directory, stateless/ and the core's headers; the map only links
        src_dir, src, export_map, lib = SATELLITES[n]
        used = [SATELLITES[u][0] for u in SATELLITE_USES.get(n, [])]
        own = [os.path.join(d, f) for d in [src_dir, STATELESS] + used for f in os.listdir(d) if f != export_map]
        out[lib] = (n, [os.path.join(src_dir, src)], hdr + own, [], os.path.join(src_dir, export_map), [])
    return out


def _build_libs(variants, force, verbose, satellites=()):
    """The stale objects of ALL the libraries in one pool (a variant's device translation unit takes as long as the rest of it
    together, so three variants one after the other leave most cores idle), each library linked once its own objects are there."""
    recipes = _recipes(variants, satellites)
    plan = {lib: _stale_objects(r[0], r[1], r[2], force) for lib, r in recipes.items()}
    todo = [(s, o, lib) for lib in plan for s, o in plan[lib][1]]
    todo.sort(key=lambda t: (os.path.basename(t[0]) not in DEVICE_SRCS, not t[0].endswith(".hip")))          # the long compiles first
    with concurrent.futures.ThreadPoolExecutor(min(len(todo), 16) or 1) as ex:
        done = {lib: [] for lib in plan}
        for s, o, lib in todo:
            done[lib].append(ex.submit(_compile, s, o, recipes[lib][3], verbose))
        for lib, (_, _, _, _, export_map, extra) in recipes.items():
            for f in done[lib]:
                f.result()
            if done[lib] or force or _stale(lib, plan[lib][0] + [export_map]):
                _link(lib, plan[lib][0], export_map, extra, verbose)


def build(force=False, verbose=False, test_hooks=True, variants=None):
    """variants: the libraries to build (names of VARIANTS); by default the product, the test-hooks build unless test_hooks is
    false, and the experiments build where one exists (kept in step with the sources, never created by default).  The ctx-less
    libraries (SATELLITES) are always built."""
    if variants is None:
        variants = ["product"] + (["test"] if test_hooks else []) + (["exp"] if os.path.exists(EXP_LIB) else [])
    _build_libs(list(variants), force, verbose, list(SATELLITES))
    os.makedirs(BIN, exist_ok=True)
    inc = os.path.join(HERE, "..", "include")
    cli_deps = [os.path.join(CSRC, f) for f in ("cli_common.hpp", "gbp_transport.hpp", "gbp_metric_gather.hpp")] + [os.path.join(inc, f) for f in os.listdir(inc)] + [LIB, POST_LIB, SEED_LIB, RESECT_LIB, LOCATE_LIB]
    for name, src in CLI_SRCS.items():
        path = os.path.join(CSRC, src)
        exe = os.path.join(BIN, name)
        if os.path.exists(path) and (force or _stale(exe, cli_deps + [path])):
            # the CLIs are plain C++ on top of the C-ABI: host compiler, linked against the in-tree library
            # (ba / slam: + the readout, seeding, resection and location libraries, and the HIP runtime for the device arrays --cov_file / --lmk_init /
            # --kf_init hand them)
            rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
            post = [] if name == "bal_convert" else ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-lgbp_mi355x_post", "-lgbp_mi355x_seed", "-lgbp_mi355x_resect", "-lgbp_mi355x_locate",
                                                     "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")]
            cmd = [shutil.which("g++") or "g++", "-o", exe, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", path,
                   "-L" + HERE, "-lgbp_mi355x"] + post + ["-Wl,-rpath,$ORIGIN/.."]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    return LIB


def build_experiments(force=False, verbose=False):
    """The measurement build: the product sources + test hooks + the ablated / experimental kernel instantiations.
    Loaded only by profiles/*.py (GBP_LIB)."""
    _build_libs(["exp"], force, verbose)
    return EXP_LIB


if __name__ == "__main__":
    exp = "--experiments" in sys.argv
    print(build(force="--force" in sys.argv, verbose=True, variants=["product", "test", "exp"] if exp else None))
    if exp:
        print(EXP_LIB)
