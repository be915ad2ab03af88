"""The randomised parity soak as a library: one generator for profiles/fuzz_parity.py (long hand runs) and tests/test_gpu_fuzz.py (the
seeded slice in the suite).

    plan(kind, seed, ...)   draws EVERYTHING of a seed — graph, parameters, path wishes, the list of calls — and predicts the path the
                            library will choose, without a GPU: a plain dict.  The draws are a pure function of (kind, seed, arguments).
    run(plan)               executes the record on the GPU and compares; raises Mismatch at the first difference.

kind "ba": three runs in lock step —
  * A: the two-kernel path (persistent = -1), the literal loop of single gbp_iterate(1) / gbp_weaken_priors calls, against the ORACLE
    (device summation order) after each of the first 10 iterations and after the last, bit for bit;
  * B: the path the library chooses, driven in bursts by one of {gbp_iterate(k) + gbp_weaken_priors, gbp_ba_loop with the metric,
    gbp_ba_loop without, gbp_weaken_priors + gbp_iterate_eval_each(k)}, against A after the bursts the plan marks, every tensor bit for
    bit, the metric records of every pass against A's gbp_eval.  What the plan varies on B: host arrays or device tensors (also views
    4 bytes into a larger buffer) for upload and reads; the metric as host records, device=True or a slice of a caller's buffer whose
    other rows must stay untouched; `steps` and the base loop index of gbp_ba_loop; gbp_sync after a burst or not (the next call then
    settles the launches in flight: a read in either form, a weakening, a LINEARISE); a LINEARISE in mid-run; bursts one past kSeriesMax
    and kPersistChunk on graphs of at most 1 000 factors.
kind "slam": ./slam's flow through gbp_poplar_amd/driver.py, the product against the oracle and against itself kept off the persistent
  kernel, the state calls of one of the two runs through device tensors.
kind "shard": a landmark-sharded group of contexts in one process against the oracle.
The graphs: unsorted and camera-sorted edge lists, duplicate (camera, landmark) factors, hub landmarks of degree > 15, landmarks without
a factor, ~10 % inactive factors.  Test infrastructure: the oracle is the checker here, never the product."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gbp_poplar_amd import _cabi, _lib, driver, hostlib  # noqa: E402

CLI_STEPS = int(driver.Options().steps)
LONG_BURSTS = (513, 600, 4097)          # one and many past kSeriesMax (512), one past kPersistChunk (4 096)
LONG_MAX_EDGES = 1000
DRIVERS = ("gbp_iterate bursts", "gbp_ba_loop + metric", "gbp_ba_loop", "gbp_iterate_eval_each")
METRIC_FORMS = ("host", "device", "slice")
STATE_FORMS = ("host", "device", "offset")
PATH_NAMES = ("persistent-tagged", "persistent-barriers", "persistent-redundant", "hipGraph/direct")
SENTINEL = -0x5A5A5A5A5A5A5A5B


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------- graphs
def random_problem(rng, slam=False, big=False, max_edges=300000, size=None):
    """size None: as the soak has always drawn (log-uniform, up to max_edges).  "tiny" / "small" / "mid" / "tiles": the size classes of the
    suite's slice — at most 1 000 factors; the persistent kernel's range; between the persistent kernel's range and 2 048 tiles; just past
    2 048 tiles with enough cameras for row placement; "half": 600 - 680 tiles, a persistent grid of 150 - 170 workgroups.  (The classes aim;
    plan() measures what came out with the library's own layout.)"""
    if slam:      # a keyframe sequence: sorted by camera (slam.cpp relies on it), every keyframe sees a window of the landmarks that moves on
        C_ = int(rng.integers(3, 31))
        L = int(np.exp(rng.uniform(np.log(20), np.log(3000))))
        per_cam = rng.integers(4, max(5, min(L, 250)), C_)
        if big:      # one SLAM seed in 250: beyond 4 M positions — NEW_KEYFRAME's streams and READ_PROG's state no longer fit the staging buffer
            C_, L = int(rng.integers(12, 16)), int(rng.integers(300000, 400000))
            per_cam = rng.integers(300000, 380000, C_)
        width = max(4, int(L * rng.uniform(0.1, 0.6)))
        cam_id = np.repeat(np.arange(C_), per_cam)
        centre = (np.arange(C_) / max(C_ - 1, 1) * max(L - width, 1)).astype(np.int64)
        lmk_id = np.concatenate([np.sort((centre[c] + rng.integers(0, width, per_cam[c])) % L) for c in range(C_)])
        E = int(cam_id.size)
    else:
        C_ = int(rng.integers(2, 121))
        L = int(np.exp(rng.uniform(np.log(3), np.log(30000))))
        if big:      # one seed in fifty: beyond 1.6 M positions (gbp_upload's device-buffer path), thousands of tiles (the shape rules of the sweep)
            C_, L = int(rng.integers(200, 3000)), int(rng.integers(150000, 220000))
        E = int(min(max_edges, rng.integers(max(C_, L), max(C_, L) + 11 * L + 1)))
        if big:
            E = int(rng.integers(1700000, 2100000))
        if size == "tiny":
            C_, L = min(C_, 24), int(np.exp(rng.uniform(np.log(3), np.log(150))))
            E = int(min(LONG_MAX_EDGES, rng.integers(max(C_, L), max(C_, L) + 11 * L + 1)))
        elif size == "small":
            L = int(np.exp(rng.uniform(np.log(3), np.log(4000))))
            E = int(rng.integers(max(C_, L), max(C_, L) + 11 * L + 1))
        elif size == "mid":
            L = int(rng.integers(10000, 30000))
            E = int(rng.integers(70000, min(120000, 11 * L)))
        elif size == "tiles":
            C_, L = int(rng.integers(300, 421)), int(rng.integers(15000, 30000))      # (rows are placed where a camera has few factors)
            E = int(rng.integers(133000, 150000))
        elif size == "half":      # 600 - 680 tiles: a persistent grid of more than half an MI355X's CUs (tests/multi_ctx_support.py)
            C_, L = int(rng.integers(8, 33)), int(rng.integers(2000, 3500))
            E = int(rng.integers(38500, 42000))
        cam_id = rng.integers(0, C_, E)
        if rng.random() < 0.5:                                   # half of the graphs: a few cameras see almost everything
            m = rng.random(E) < 0.5
            cam_id[m] = rng.integers(0, min(C_, 3), int(m.sum()))
        lmk_id = rng.integers(0, max(1, L - 2), E)               # the last two landmarks stay factor-less
        for _ in range(int(rng.integers(0, 3))):
            lmk_id[rng.random(E) < rng.uniform(0.005, 0.1)] = int(rng.integers(0, max(1, L - 2)))      # hub landmarks
        cam_id[:C_] = np.arange(C_)                              # every camera has a factor (else its prior is NaN by design)
        if rng.random() < 0.3:                                   # some files ARE sorted by camera
            o = np.argsort(cam_id, kind="stable")
            cam_id, lmk_id = cam_id[o], lmk_id[o]
    cams = np.zeros((C_, 6))
    c = np.arange(C_)
    cams[:, 0], cams[:, 1], cams[:, 2] = 0.1 * c, -0.05 * c, 5.0 + 0.2 * c
    cams[:, 3], cams[:, 4], cams[:, 5] = 0.05 + 0.01 * (c % 40), -0.04, 0.03 * ((c % 25) + 1)
    pts = rng.uniform(-1, 1, (L, 3))
    w = cams[cam_id, 3:]
    th = np.linalg.norm(w, axis=1, keepdims=True)
    k = w / th
    y = pts[lmk_id]
    Ry = y * np.cos(th) + np.cross(k, y) * np.sin(th) + k * np.sum(k * y, axis=1, keepdims=True) * (1 - np.cos(th))
    p = Ry + cams[cam_id, :3]
    obs = np.stack([500 * p[:, 0] / p[:, 2] + 320, 500 * p[:, 1] / p[:, 2] + 240], axis=1) + rng.normal(0, 1, (E, 2))
    return {"n_cams": C_, "n_lmks": L, "n_edges": E, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0,
            "cam_id": np.asarray(cam_id, np.uint32), "lmk_id": np.asarray(lmk_id, np.uint32), "observations": obs.ravel(),
            "cameras": (cams + rng.normal(0, 0.01, cams.shape) * (np.arange(C_)[:, None] >= 2)).ravel(),
            "points": (pts + rng.normal(0, 0.05, pts.shape)).ravel()}


def graph_traits(bal):
    """what the docstring promises of the graphs, measured on one"""
    cam, lmk, L = bal["cam_id"].astype(np.int64), bal["lmk_id"].astype(np.int64), bal["n_lmks"]
    deg = np.bincount(lmk, minlength=L)
    return {"sorted": bool(np.all(np.diff(cam) >= 0)), "duplicates": bool(np.unique(cam * L + lmk).size < cam.size),
            "hub": bool(deg.max() > 15), "factorless": bool((deg == 0).any())}


def predict_path(bal, per_factor_mu, tile_order, persistent):
    """(n_tiles, positions, does the library run this graph in the persistent kernel?) — from the device order the test-hooks library
    builds on the host and the grid its persistent kernel would take (gbp_debug_layout_build, gbp_debug_persist_roles): no GPU, and no
    copy of a padding or sizing rule.  What is restated is the list of conditions of persist_setup: means hoisted, no tile permutation,
    no placed rows, at most one workgroup per CU (256) with the metric roles."""
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], tile_order=tile_order)
    dims = (C.c_uint32 * 4)()
    lib = _lib.load(hooks=True)
    assert lib.gbp_debug_persist_roles(lay["n_tiles"], bal["n_cams"], bal["n_lmks"], 1, dims, None, 0) == 0
    ok = persistent >= 0 and per_factor_mu == 0 and lay["tile_perm"].size == 0 and lay["row_slot"].size == 0 and int(dims[0]) <= 256
    return int(lay["n_tiles"]), int(lay["Ep"]), bool(ok), bool(lay["tile_perm"].size), bool(lay["row_slot"].size)


def weakens(i, steps):
    """the reference's loop weakens the priors in front of the pass of loop index i (ba.cpp:1003-1006)"""
    return (i + 1) % 2 == 0 and i < 2 * steps


# ---------------------------------------------------------------- plans
def _params_draw(rng, lo, hi):
    return dict(dmu_threshold=float(rng.choice([0.05, 0.02, 3e-3])), min_linear_iters=int(rng.integers(2, lo)), num_undamped_iters=int(rng.integers(1, hi)))


def plan_ba(seed, big=False, max_edges=300000, size=None, wish=None, widen=True):
    """wish (the suite's stratification; None = everything drawn): dict with any of path 0..3 (PATH_NAMES), drive 0..3, upload
    (STATE_FORMS), seg -1 / 0 / 1.  widen=False: the call patterns of the soak before they were widened (measurements)."""
    wish = wish or {}
    rng = np.random.default_rng(7000 + seed)          # the stream the soak has always used: graph, parameters, path, driver, bursts
    rw = np.random.default_rng(17000 + seed)         # the widened call patterns draw from a stream of their own
    bal = random_problem(rng, big=big, max_edges=max_edges, size=size)
    E = bal["n_edges"]
    undamped_start = int(rng.integers(1, 4))
    active = (rng.random(E) < 0.9).astype(np.uint32)
    kw = _params_draw(rng, 6, 4)
    kw.update(per_factor_mu=int(rng.integers(0, 2)), tile_order=int(rng.integers(0, 4)))
    seg = int(rng.integers(-1, 2))
    if size == "tiles":      # tile_perm, placed rows and SEG: the default order, hoisted means
        kw["tile_order"] = kw["per_factor_mu"] = 0
    elif wish.get("path", 3) < 3:      # eligible for the persistent kernel: hoisted means, no tile permutation
        kw["tile_order"], kw["per_factor_mu"] = kw["tile_order"] % 2, 0
    elif "path" in wish and size != "mid" and kw["tile_order"] < 2:
        kw["per_factor_mu"] = 1      # a small graph kept off the persistent kernel: literal per-factor means (or, as drawn, a tile permutation)
    seg = wish.get("seg", seg)
    n_tiles, positions, persist, perm, placed = predict_path(bal, kw["per_factor_mu"], kw["tile_order"], 0)
    flow = verify = -1
    if persist:
        flow = int(rng.integers(0, 2))
        if flow == 1:
            verify = int(rng.integers(0, 2))
        if "path" in wish and wish["path"] < 3:
            flow, verify = (1, 0) if wish["path"] == 0 else (0, -1) if wish["path"] == 1 else (1, 1)
    drive = int(rng.integers(0, 3))
    if widen:
        drive = wish.get("drive", int(rw.integers(0, 4)))
    total = int(rng.integers(24, 60)) if E < 1000000 else int(rng.integers(12, 20))
    if n_tiles >= 2048 and size == "tiles":
        total = int(rng.integers(12, 21))
    lengths, it = [], 0
    while it < total:
        lengths.append(int(min(total - it, rng.choice([1, 1, 2, 3, 5, 8, 13, 21]))))
        it += lengths[-1]
    p = {"kind": "ba", "seed": seed, "size": size, "bal": bal, "traits": graph_traits(bal), "undamped_start": undamped_start, "active_flag": active,
         "kw": kw, "seg": seg, "n_tiles": n_tiles, "positions": positions, "persist": persist, "tile_perm": perm, "row_placement": placed,
         "flow": flow, "verify": verify, "drive": drive, "widen": widen,
         "path": 3 if not persist else 1 if flow == 0 else 2 if verify == 1 else 0}
    if not widen:
        p.update(steps=CLI_STEPS, base=0, upload="host", linearise_after=-1, final_forms=False,
                 bursts=[{"n": n, "metric": "host", "sync": True, "check": True, "read": "host", "eval": "host"} for n in lengths])
        return p
    steps = int(rw.choice([0, 1, 3, CLI_STEPS]))
    base = max(0, int(rw.choice([0, 1, 2 * steps - 2, 2 * steps - 1])))
    upload = wish.get("upload", STATE_FORMS[int(rw.integers(0, 3))])
    if E <= LONG_MAX_EDGES and rw.random() < 0.6:      # at most one of each, anywhere among the bursts
        for n in LONG_BURSTS:
            if rw.random() < 0.5:
                lengths.insert(int(rw.integers(0, len(lengths) + 1)), n)
    lin = int(rw.integers(0, len(lengths))) if rw.integers(0, 4) == 0 else -1
    offset_reads = upload == "offset"
    bursts = []
    for b, n in enumerate(lengths):
        bursts.append({"n": n, "metric": METRIC_FORMS[int(rw.integers(0, 3))], "sync": bool(rw.integers(0, 2)),
                       "check": bool(b == len(lengths) - 1 or rw.random() < 0.75),
                       "read": "host" if b % 2 == 0 else ("offset" if offset_reads else "device"), "eval": ("host", "device")[int(rw.integers(0, 2))]})
    p.update(steps=steps, base=base, upload=upload, linearise_after=lin, final_forms=True, bursts=bursts)
    return p


def plan_slam(seed, big=False, widen=True):
    rng = np.random.default_rng(9000 + seed)
    rw = np.random.default_rng(19000 + seed)
    bal = random_problem(rng, slam=True, big=big)
    kw = _params_draw(rng, 8, 6)
    pf, persistent = int(rng.integers(0, 2)), int(rng.choice([0, 0, -1]))
    ibk = int(rng.integers(4, 40))
    every = int(rng.choice([1, 1, 3, 10]))
    max_iters = int(rng.integers(40, 260)) if not big else int(rng.integers(30, 50))
    if big:
        ibk = int(rng.integers(4, 9))
        pf = (seed // 1000) % 2
    n_tiles, positions, persist, _, _ = predict_path(bal, pf, 0, persistent)
    form = STATE_FORMS[int(rw.integers(0, 3))] if widen else "host"
    return {"kind": "slam", "seed": seed, "bal": bal, "traits": graph_traits(bal), "kw": kw, "per_factor_mu": pf, "persistent": persistent, "ibk": ibk,
            "every": every, "max_iters": max_iters, "n_tiles": n_tiles, "positions": positions, "persist": persist, "form": form,
            "second_form": ("device" if form == "host" else "host") if widen else None, "widen": widen}


def plan_shard(seed, max_edges=300000, size=None):
    from gbp_poplar_amd.distributed import landmark_partition
    rng = np.random.default_rng(11000 + seed)
    bal = random_problem(rng, max_edges=max_edges, size=size)
    undamped_start = int(rng.integers(1, 4))
    active = (rng.random(bal["n_edges"]) < 0.9).astype(np.uint32)
    kw = _params_draw(rng, 6, 4)
    world = int(rng.choice([2, 3, 4, 5, 8]))
    bounds = landmark_partition(bal["lmk_id"], bal["n_lmks"], world)
    total = int(rng.integers(12, 40))
    return {"kind": "shard", "seed": seed, "bal": bal, "traits": graph_traits(bal), "undamped_start": undamped_start, "active_flag": active, "kw": kw,
            "world": world, "bounds": [int(b) for b in bounds], "total": total, "local_first": [bool(rng.random() < 0.5) for _ in range(total)],
            "steps": CLI_STEPS}


def kind_of(seed):
    """every fourth seed ./slam's flow, every eighth a sharded group"""
    return "slam" if seed % 4 == 3 else "shard" if seed % 8 == 5 else "ba"


def plan(kind, seed, **kw):
    return {"ba": plan_ba, "slam": plan_slam, "shard": plan_shard}[kind](seed, **kw)


def soak_plan(seed, max_edges=300000):
    """the seed as a long run of profiles/fuzz_parity.py draws it (the big graphs included)"""
    kind = kind_of(seed)
    if kind == "slam":
        return plan_slam(seed, big=(seed % 1000 == 999))
    if kind == "shard":
        return plan_shard(seed, max_edges=max_edges)
    return plan_ba(seed, big=(seed % 50 == 49), max_edges=max_edges)


# ---- the suite's slice: SUITE_SEEDS, stratified so that tests/test_fuzz_plan_cpu.py's coverage holds by construction ----
SUITE_FIRST = 60000
SUITE_COUNT = 120
SUITE_SEEDS = tuple(range(SUITE_FIRST, SUITE_FIRST + SUITE_COUNT))


def suite_plan(seed, widen=True):
    """Seed SUITE_FIRST + i.  i % 4 == 3: SLAM; i % 8 == 5: sharded (small graphs); the others "ba": i % 8 in {0, 2, 4} the persistent
    kernel's size range, the 45 of them walking path wish x driver x upload form (every fifth at most 1 000 factors: the long bursts);
    i % 8 in {1, 6} between 65 536 and 131 072 positions — except i in {9, 49, 89}: 2 048 tiles or more, SEG on / off / by shape."""
    i = seed - SUITE_FIRST
    assert 0 <= i < SUITE_COUNT, seed
    kind = kind_of(i)
    if kind == "slam":
        return plan_slam(seed, widen=widen)
    if kind == "shard":
        return plan_shard(seed, size="small")
    q, r = divmod(i, 8)
    if r in (0, 2, 4):
        idx = 3 * q + r // 2
        return plan_ba(seed, size="tiny" if idx % 5 == 0 else "small", wish={"path": idx % 4, "drive": (idx // 4) % 4, "upload": STATE_FORMS[(idx // 4 + idx // 16) % 3]}, widen=widen)
    idx = 2 * q + (r == 6)
    if r == 1 and q % 5 == 1:
        return plan_ba(seed, size="tiles", wish={"path": 3, "drive": q // 5 % 4 + 1 & 3, "seg": q // 5 - 1, "upload": STATE_FORMS[q // 5]}, widen=widen)
    return plan_ba(seed, size="mid", wish={"path": 3, "drive": (idx // 2) % 4, "upload": STATE_FORMS[idx % 3]}, widen=widen)


def describe(p):
    """the plan in one line"""
    b = p["bal"]
    s = "%s seed %d: C %d L %d E %d, %d tiles" % (p["kind"], p["seed"], b["n_cams"], b["n_lmks"], b["n_edges"], p.get("n_tiles", -1))
    if p["kind"] == "ba":
        kw = p["kw"]
        s += " | mu %d order %d seg %+d | B predicted %s, driven by %s | steps %d base %d upload %s linearise after burst %d | bursts %s" % (
            kw["per_factor_mu"], kw["tile_order"], p["seg"], PATH_NAMES[p["path"]], DRIVERS[p["drive"]], p["steps"], p["base"], p["upload"], p["linearise_after"],
            " ".join("%d%s%s%s" % (x["n"], x["metric"][0], "s" if x["sync"] else "", "" if x["check"] else "-") for x in p["bursts"]))
    elif p["kind"] == "slam":
        s += " | mu %d persistent %d (predicted %s) | keyframe every %d, metric every %d, at most %d iterations | state calls %s / %s" % (
            p["per_factor_mu"], p["persistent"], "k_persist_flow" if p["persist"] else "hipGraph/direct", p["ibk"], p["every"], p["max_iters"], p["form"], p["second_form"])
    else:
        s += " | world %d, %d iterations" % (p["world"], p["total"])
    return s


# ---------------------------------------------------------------- comparing
def ev_equal(a, b):
    """two metric dicts (or lists of them), NaN == NaN (a graph that diverges does so on both sides, bit for bit)"""
    if isinstance(a, list):
        return len(a) == len(b) and all(ev_equal(x, y) for x, y in zip(a, b))
    return all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def same(a, b, what):
    if not np.array_equal(a, b, equal_nan=True):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            raise Mismatch("%s: shapes %r vs %r" % (what, a.shape, b.shape))
        bad = np.flatnonzero(~((a == b) | (np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))))
        raise Mismatch("%s differs in %d of %d entries (first at %d: %r vs %r)" % (what, bad.size, a.size, bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]]))


def snapshot(eng, form=None):
    """every tensor of the engine; form: how a DeviceForms proxy reads the state (None: as the engine reads by default)"""
    d = dict(eng.read() if form is None else eng.read(form=form))
    d.update({"msg_" + k: v for k, v in eng.messages().items()})
    fe, fl = eng.factor_potentials()
    d.update(fac_eta=fe, fac_lambda=fl, mu=eng.mu()[0])
    return d


def against_oracle(eng, orc, it, potentials=False):
    g, o = eng.read(), orc.read()
    for k in ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag"):
        same(g[k], o[k], "A vs oracle after iteration %d: %s" % (it, k))
    gm, om = eng.messages(), orc.messages()
    mask = np.tile(np.tril(np.ones((6, 6), bool)).ravel(), eng.E)      # cam message Lambda: the lower triangle is stored
    same(gm["cam_eta"], om["cam_eta"], "A vs oracle after iteration %d: cam message eta" % it)
    same(gm["cam_lambda"][mask], om["cam_lambda"][mask], "A vs oracle after iteration %d: cam message lambda" % it)
    same(gm["lmk_eta"], om["lmk_eta"], "A vs oracle after iteration %d: lmk message eta" % it)
    same(gm["lmk_lambda"], om["lmk_lambda"], "A vs oracle after iteration %d: lmk message lambda" % it)
    if potentials:
        fe, fl = eng.factor_potentials()
        oe, ol = orc.factor_potentials()
        same(fe, oe, "A vs oracle: factor eta")
        same(fl, ol, "A vs oracle: factor lambda")


class Clock:
    def __init__(self):
        self.t, self.acc = time.perf_counter(), {}

    def lap(self, name):
        n = time.perf_counter()
        self.acc[name] = self.acc.get(name, 0.0) + n - self.t
        self.t = n


# ---------------------------------------------------------------- the state calls through device tensors
class DeviceForms:
    """A thin proxy around GbpEngine: forwards everything, and does upload / read / read_priors / new_keyframe in `form` — "host": numpy
    arrays as ever; "device": torch tensors on the GPU; "offset": tensors that are views 4 bytes into a larger buffer (not 16-byte
    aligned).  It takes and hands back numpy either way, so driver.py drives the device forms unchanged.  A device-form read is followed
    by sync() before its tensors are copied to the host: the read itself had to settle whatever was in flight."""
    _IN = {"upload": _cabi.GbpStateIn, "new_keyframe": _cabi.GbpKfUpdate}

    def __init__(self, eng, form="host"):
        self.__dict__["_e"] = eng
        self.__dict__["form"] = form

    def __getattr__(self, name):
        return getattr(self._e, name)

    def __setattr__(self, name, value):
        if name == "form":
            self.__dict__["form"] = value
        else:
            setattr(self._e, name, value)

    def _buffer(self, n, dtype, offset):
        import torch
        if not offset:
            return torch.empty(n, dtype=dtype, device=self._e.device())
        return torch.empty(n + 5, dtype=dtype, device=self._e.device())[1:n + 1]

    def _send(self, struct, arrays, offset):
        import torch
        types = dict(struct._fields_)
        out = {}
        for k, a in arrays.items():
            if a is None:
                continue
            ints = types[k] is not _cabi.c_f32p
            a = np.ascontiguousarray(a, dtype=(np.int32 if types[k] is _cabi.c_i32p else np.uint32) if ints else np.float32).reshape(-1)
            t = self._buffer(a.size, torch.int32 if ints else torch.float32, offset)
            t.copy_(torch.from_numpy(a.view(np.int32) if ints else a))
            out[k] = t
        torch.cuda.current_stream().synchronize()      # the ctx runs on a stream of its own: the inputs are complete before it reads them
        return out

    def _receive(self, call, struct, form):
        import torch
        if form == "host":
            return call()
        if form == "device":
            out = call(device=True)
        else:
            sz = self._e._sizes()
            out = call(out={n: self._buffer(sz[n], torch.float32 if t is _cabi.c_f32p else torch.int32, True) for n, t in struct._fields_})
        self._e.sync()
        types = dict(struct._fields_)
        return {k: (v.cpu().numpy().view(np.uint32) if types[k] is _cabi.c_u32p else v.cpu().numpy()) for k, v in out.items()}

    def upload(self, state, form=None):
        form = form or self.form
        self._e.upload(state if form == "host" else self._send(_cabi.GbpStateIn, state, form == "offset"))

    def new_keyframe(self, upd, form=None):
        form = form or self.form
        self._e.new_keyframe(upd if form == "host" else self._send(_cabi.GbpKfUpdate, upd, form == "offset"))

    def read(self, form=None):
        return self._receive(self._e.read, _cabi.GbpStateOut, form or self.form)

    def read_priors(self, form=None):
        return self._receive(self._e.read_priors, _cabi.GbpPriorsOut, form or self.form)


class _Records:
    """the metric records of one call of B in the form the plan drew; list() once B is known to have finished (after a blocking call)"""

    def __init__(self, eng, n, form):
        import torch
        self.form, self.n, self.big, self.kw = form, n, None, {}
        if form == "device":
            self.kw = {"device": True}
        elif form == "slice":      # rows 2 .. 2 + n of a caller's larger buffer; the other rows must stay as they are
            self.big = torch.full((n + 5, 7), SENTINEL, dtype=torch.int64, device=eng.device())
            torch.cuda.current_stream().synchronize()
            self.kw = {"out": self.big[2:2 + n]}
        self.res = None

    def list(self, what):
        if self.form == "host":
            return self.res
        cols = {k: v.cpu().numpy() for k, v in self.res.items()}
        if self.big is not None:
            rest = np.concatenate([self.big[:2].cpu().numpy().ravel(), self.big[2 + self.n:].cpu().numpy().ravel()])
            if not np.all(rest == SENTINEL):
                raise Mismatch("%s: rows of the caller's buffer outside the slice handed over were written" % what)
        return [{k: (float(v[j]) if v.dtype == np.float64 else int(v[j])) for k, v in cols.items()} for j in range(self.n)]


def _eval(eng, form):
    if form == "host":
        return eng.eval()
    r = eng.eval(device=True)
    eng.sync()
    return {k: (float(v.cpu().numpy()[0]) if k in _cabi.EVAL_F64 else int(v.cpu().numpy()[0])) for k, v in r.items()}


# ---------------------------------------------------------------- runs
def _engines():
    from gbp_poplar_amd.engine import GbpEngine
    from oracle import oracle as orc_mod
    return GbpEngine, orc_mod


def run_ba(p):
    GbpEngine, orc_mod = _engines()
    lib = _lib.load(hooks=True)
    ck = Clock()
    bal, kw, steps, base, drive = p["bal"], p["kw"], p["steps"], p["base"], p["drive"]
    C_, L, E = bal["n_cams"], bal["n_lmks"], bal["n_edges"]
    opts = driver.Options()
    opts.undamped_start = p["undamped_start"]
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    state["active_flag"] = p["active_flag"]
    assert lib.gbp_debug_force_seg_skip(p["seg"]) == 0
    try:
        A = GbpEngine(bal["cam_id"], bal["lmk_id"], C_, L, K, hooks=True, params=_cabi.GbpParams.defaults(persistent=-1, **kw))
        B = DeviceForms(GbpEngine(bal["cam_id"], bal["lmk_id"], C_, L, K, hooks=True, params=_cabi.GbpParams.defaults(persistent=0, **kw)))
    finally:
        lib.gbp_debug_force_seg_skip(-1)
    okw = {k: v for k, v in kw.items() if k not in ("per_factor_mu", "tile_order")}
    O = orc_mod.Oracle(bal["cam_id"], bal["lmk_id"], C_, L, K, params=_cabi.GbpParams.defaults(**okw))
    O.set_sum_order(1)
    try:
        if (B.graph_state() == 2) != p["persist"]:
            raise Mismatch("B's path after gbp_create is %d, the plan predicted %s (%s)" % (B.graph_state(), PATH_NAMES[p["path"]], B.last_error()))
        if p["persist"]:
            B.persist_flow(p["flow"])
            if p["flow"] == 1:
                B.persist_verify(p["verify"])
        A.upload(state)
        O.upload(state)
        B.upload(state, form=p["upload"])
        for x in (A, B, O):
            x.linearise()
        ck.lap("setup")
        it = n_relin = 0
        metric = drive in (1, 3)
        pending = []      # (records of B, A's metrics of the same passes, what)
        for b, burst in enumerate(p["bursts"]):
            n = burst["n"]
            evA = []
            i = it
            while i < it + n:
                if weakens(base + i, steps):
                    A.weaken_priors()
                    O.weaken_priors()
                k = 1
                if not metric and i >= 10:      # nothing is looked at in between: up to the next weakening in one call
                    while i + k < it + n and not weakens(base + i + k, steps):
                        k += 1
                A.iterate(k)
                ck.lap("A")
                O.iterate(k)
                ck.lap("oracle")
                if metric or i < 10:
                    evA.append(A.eval())
                ck.lap("A")
                if i < 10:
                    against_oracle(A, O, i)
                    ck.lap("compare")
                    eo = O.eval()
                    if (evA[-1]["n_relin"], evA[-1]["n_robust"], evA[-1]["n_active"]) != (eo["n_relin"], eo["n_robust"], eo["n_active"]):
                        raise Mismatch("counts after iteration %d: %r vs oracle %r" % (i, evA[-1], eo))
                i += k
            what = "burst %d (%d passes from loop index %d, metric form %s)" % (b, n, base + it, burst["metric"])
            if drive in (0, 3):
                left, i = n, it
                while left > 0:
                    if weakens(base + i, steps):
                        B.weaken_priors()
                    k = 1
                    while k < left and not weakens(base + i + k, steps):
                        k += 1
                    if drive == 0:
                        B.iterate(k)
                    else:
                        r = _Records(B, k, burst["metric"])
                        r.res = B.iterate_eval_each(k, **r.kw)
                        pending.append((r, evA[len(evA) - left:len(evA) - left + k], what + ", passes %d.." % i))
                    i += k
                    left -= k
            elif drive == 1:
                r = _Records(B, n, burst["metric"])
                r.res = B.ba_loop(n, base + it, steps, **r.kw)
                pending.append((r, evA[-n:], what))
            else:
                B.ba_loop(n, base + it, steps, metrics=False)
            it += n
            if burst["sync"]:
                B.sync()
            ck.lap("B")
            if b == p["linearise_after"]:      # LINEARISE under live messages; B's launches may still be in flight
                for x in (A, B, O):
                    x.linearise()
            if not burst["check"]:
                continue
            sa, sb = snapshot(A), snapshot(B, form=burst["read"])
            for k in sa:
                same(sb[k], sa[k], "B (%s read) vs A after %d iterations: %s" % (burst["read"], it, k))
            for r, ea, w in pending:
                eb = r.list(w)
                if not ev_equal(eb, ea):
                    j = next(j for j in range(len(ea)) if not ev_equal(eb[j], ea[j]))
                    raise Mismatch("metric of %s, record %d: B %r vs A %r" % (w, j, eb[j], ea[j]))
            pending = []
            ea, eb = A.eval(), _eval(B, burst["eval"])
            if not ev_equal(ea, eb):
                raise Mismatch("gbp_eval (%s form) after %d iterations: B %r vs A %r" % (burst["eval"], it, eb, ea))
            n_relin += ea["n_relin"]
            ck.lap("compare")
        against_oracle(A, O, it - 1, potentials=True)
        if p["final_forms"]:      # both forms of the same state, once per seed
            other = "offset" if p["upload"] == "offset" else "device"
            for name in ("read", "read_priors"):
                h, d = getattr(B, name)(form="host"), getattr(B, name)(form=other)
                for k in h:
                    same(d[k], h[k], "B's %s, %s form vs host form: %s" % (name, other, k))
            pa = A.read_priors()
            ph = B.read_priors(form="host")
            for k in pa:
                same(ph[k], pa[k], "priors, B vs A: %s" % k)
        path = B.graph_state()
        if (path == 2) != p["persist"]:
            raise Mismatch("B ended on path %d, the plan predicted %s (%s)" % (path, PATH_NAMES[p["path"]], B.last_error()))
        if p["verify"] == 1:
            bad = B.persist_verify(0)
            if bad:
                raise Mismatch("the redundant-record check counted %d records that differed from their copy" % bad)
        desc = "C %d L %d E %d | mu %d order %d seg %+d | B: %s%s, driven by %s | %d iterations, relinearisations seen %d" % (
            C_, L, E, kw["per_factor_mu"], kw["tile_order"], p["seg"],
            {2: "k_persist_flow", 1: "hipGraph", 0: "direct", -1: "direct"}[path],
            "" if path != 2 else (" (tagged records%s)" % (", redundant check" if p["verify"] == 1 else "") if p["flow"] == 1 else " (barriers)"),
            DRIVERS[drive], it, n_relin)
        ck.lap("compare")
        desc += " | s: " + ", ".join("%s %.2f" % kv for kv in ck.acc.items())
        return desc, n_relin
    finally:
        A.close()
        B.close()


def run_slam(p):
    """./slam's flow (slam.cpp:1013-1103 as gbp_poplar_amd/driver.py drives it: NEW_KEYFRAME / READ_PRIORS, activation of factors, re-armed
    damping counts, the weakening schedule restarting at every keyframe) on a random keyframe sequence: the PRODUCT library on the path it
    chooses (or kept off the persistent kernel) against the oracle — counts of every printed line exact, every belief and per-factor state
    bit for bit at the end, the priors (READ_PRIORS) too — and against a second run of the product with persistent = -1 and the other
    form of the state calls: every printed line, counts and metric, bit for bit."""
    GbpEngine, orc_mod = _engines()
    bal, kw = p["bal"], p["kw"]
    C_, L, E = bal["n_cams"], bal["n_lmks"], bal["n_edges"]
    opts = driver.Options()
    K, state, extra = driver.build_inputs(bal, opts, hostlib, slam=True)
    G = DeviceForms(GbpEngine(bal["cam_id"], bal["lmk_id"], C_, L, K, hooks=False,
                              params=_cabi.GbpParams.defaults(per_factor_mu=p["per_factor_mu"], persistent=p["persistent"], **kw)), p["form"])
    O = orc_mod.Oracle(bal["cam_id"], bal["lmk_id"], C_, L, K, params=_cabi.GbpParams.defaults(**kw))
    O.set_sum_order(1)
    G2 = None
    try:
        run = dict(iters_between_kfs=p["ibk"], max_iters=p["max_iters"], eval_every=p["every"])
        tg = driver.run_slam(G, hostlib, bal, state, extra, opts, **run)
        path = G.graph_state()
        if (path == 2) != p["persist"]:
            raise Mismatch("slam: the product ended on path %d, the plan predicted %s (%s)" % (path, "k_persist_flow" if p["persist"] else "hipGraph/direct", G.last_error()))
        to = driver.run_slam(O, hostlib, bal, state, extra, opts, **run)
        to = {r[0]: r for r in to}
        n_relin = 0
        worst = (0.0, None)
        for (i, mg, cg, rg, bg) in tg:
            if i not in to:
                continue
            _, mo, co, ro_, bo = to[i]
            if (rg, bg) != (ro_, bo):
                raise Mismatch("slam: line of iteration %d: GPU (%.9g, relins %d, robust %d) vs oracle (%.9g, %d, %d)" % (i, mg, rg, bg, mo, ro_, bo))
            # The metric is not a bit-exact quantity between the two (the means are solved differently, z - h(x) cancels ~500 px coordinates in fp32,
            # and a point near a camera's plane amplifies an ulp without bound): 1e-5 relative + 1e-4 px as in tests/test_gpu_parity.py is what
            # well-posed sequences keep; a line beyond it is reported, and it is the STATE below that decides — bit for bit.
            if mg == mg and mo == mo:
                dev = abs(mg - mo) / (1e-5 * mo + 1e-4)
                if dev > worst[0]:
                    worst = (dev, (i, mg, mo))
            n_relin += rg
        g, o = G.read(form="host"), O.read()
        for k in o:
            same(g[k], o[k], "slam: final %s" % k)
        pg, po = G.read_priors(form="host"), O.read_priors()
        for k in po:
            same(pg[k], po[k], "slam: final %s" % k)
        if p["second_form"] is not None:
            G2 = DeviceForms(GbpEngine(bal["cam_id"], bal["lmk_id"], C_, L, K, hooks=False,
                                       params=_cabi.GbpParams.defaults(per_factor_mu=p["per_factor_mu"], persistent=-1, **kw)), p["second_form"])
            t2 = driver.run_slam(G2, hostlib, bal, state, extra, opts, **run)
            if len(t2) != len(tg):
                raise Mismatch("slam: %d printed lines with persistent = -1, %d on the chosen path" % (len(t2), len(tg)))
            for a, b2 in zip(tg, t2):
                if not all(x == y or (x != x and y != y) for x, y in zip(a, b2)):
                    raise Mismatch("slam: line of iteration %d: chosen path (%s state calls) %r vs persistent = -1 (%s state calls) %r" % (a[0], p["form"], a, p["second_form"], b2))
            g2 = G2.read(form="host")
            for k in g:
                same(g2[k], g[k], "slam: final %s, persistent = -1 vs the chosen path" % k)
        desc = "SLAM C %d L %d E %d | mu %d | keyframe every %d, metric every %d, %d iterations | path %s | relinearisations seen %d" % (
            C_, L, E, p["per_factor_mu"], p["ibk"], p["every"], min((C_ - 1) * p["ibk"] - 1, p["max_iters"]),
            {2: "k_persist_flow", 1: "hipGraph", 0: "direct", -1: "direct"}[path], n_relin)
        if worst[0] > 1.0:
            desc += " | metric of iteration %d beyond 1e-5 rel + 1e-4 px (GPU %.9g, oracle %.9g) with every tensor bit-equal at the end" % worst[1]
        return desc, n_relin
    finally:
        G.close()
        if G2 is not None:
            G2.close()


class GatherAll:
    """the all-gather between shard contexts living in one process (what RCCL does between GPUs): every rank's send buffer into every
    rank's receive buffer, by device copies"""

    def __init__(self):
        self.members = []

    def __call__(self):
        import torch
        for m in self.members:
            m.stream.synchronize()
        for dst in self.members:
            for r, src in enumerate(self.members):
                n = src.send.numel()
                dst.recv[r * n:(r + 1) * n].copy_(src.send)
        torch.cuda.synchronize()


def run_shard(p):
    """`world` landmark-shard contexts (2..8, ranges balanced by factor count — ranks without a landmark included) on the one GPU, the
    exchange by device copies: the sharded C-ABI verbs (gbp_iterate_begin / _local / _end, gbp_refresh_*, gbp_linearise_factors,
    gbp_weaken_priors on a sharded ctx) against the oracle summing in `world`-shard device order — camera beliefs identical on every rank
    and equal to the oracle's, every rank's own landmark beliefs and per-factor state, bit for bit."""
    from gbp_poplar_amd.distributed import ShardedGbp
    GbpEngine, orc_mod = _engines()
    bal, kw, world, bounds, total, steps = p["bal"], p["kw"], p["world"], np.asarray(p["bounds"]), p["total"], p["steps"]
    C_, L, E = bal["n_cams"], bal["n_lmks"], bal["n_edges"]
    opts = driver.Options()
    opts.undamped_start = p["undamped_start"]
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    state["active_flag"] = p["active_flag"]
    gather = GatherAll()
    shards = []
    try:
        for r in range(world):
            eng = GbpEngine(bal["cam_id"], bal["lmk_id"], C_, L, K, shard=(r, world, int(bounds[r]), int(bounds[r + 1])), params=_cabi.GbpParams.defaults(**kw))
            sh = ShardedGbp(eng, C_, r, world, dist=None, device="cuda")
            gather.members.append(sh)
            shards.append(sh)

        def all_do(name, *a):
            for sh in shards:
                getattr(sh.e, name)(*a)

        O = orc_mod.Oracle(bal["cam_id"], bal["lmk_id"], C_, L, K, params=_cabi.GbpParams.defaults(**kw))
        O.set_sum_order(1, bounds)
        O.upload(state)
        O.linearise()
        all_do("upload", state)
        all_do("refresh_begin"); gather(); all_do("refresh_end"); all_do("linearise_factors")
        lmk = np.asarray(bal["lmk_id"])
        n_relin = 0
        for it in range(total):
            if weakens(it, steps):
                all_do("weaken_priors")
                O.weaken_priors()
            all_do("iterate_begin")
            if p["local_first"][it]:
                all_do("iterate_local")          # the landmark half first (what overlaps the all-gather on N GPUs)
            gather()
            all_do("iterate_end")
            O.iterate(1)
            if it < 6 or it == total - 1:
                ro = O.read()
                for r, sh in enumerate(shards):
                    g = sh.read()
                    same(g["cam_beliefs_eta"], ro["cam_beliefs_eta"], "world %d rank %d after iteration %d: cam_beliefs_eta" % (world, r, it))
                    same(g["cam_beliefs_lambda"], ro["cam_beliefs_lambda"], "world %d rank %d after iteration %d: cam_beliefs_lambda" % (world, r, it))
                    lo, hi = int(bounds[r]), int(bounds[r + 1])
                    same(g["lmk_beliefs_eta"][3 * lo:3 * hi], ro["lmk_beliefs_eta"][3 * lo:3 * hi], "world %d rank %d after iteration %d: lmk_beliefs_eta" % (world, r, it))
                    same(g["lmk_beliefs_lambda"][9 * lo:9 * hi], ro["lmk_beliefs_lambda"][9 * lo:9 * hi], "world %d rank %d after iteration %d: lmk_beliefs_lambda" % (world, r, it))
                    own = (lmk >= lo) & (lmk < hi)
                    for k in ("damping", "damping_count", "robust_flag"):
                        same(g[k][own], ro[k][own], "world %d rank %d after iteration %d: %s" % (world, r, it, k))
                evs = [sh.e.eval() for sh in shards]
                eo = O.eval()
                for k in ("n_active", "n_relin", "n_robust"):
                    if sum(e[k] for e in evs) != eo[k]:
                        raise Mismatch("world %d after iteration %d: %s summed over the ranks %d vs oracle %d" % (world, it, k, sum(e[k] for e in evs), eo[k]))
                n_relin += eo["n_relin"]
        desc = "SHARDED world %d (landmark ranges %s) C %d L %d E %d | %d iterations | relinearisations seen %d" % (
            world, "/".join(str(int(bounds[r + 1] - bounds[r])) for r in range(world)), C_, L, E, total, n_relin)
        return desc, n_relin
    finally:
        for sh in shards:
            sh.e.close()


def run(p):
    """execute a plan; (one-line description of what ran, relinearisations seen).  The oracle must be loaded with device trigonometry:
    prepare() does it."""
    return {"ba": run_ba, "slam": run_slam, "shard": run_shard}[p["kind"]](p)


def prepare():
    from oracle import oracle as orc_mod
    orc_mod.load("restatement")
    orc_mod.set_trig_mode(1)
    return _lib.load(hooks=True)


def one_seed(seed, lib=None, max_edges=300000):
    return run(plan_ba(seed, big=(seed % 50 == 49), max_edges=max_edges))


def slam_seed(seed):
    return run(plan_slam(seed, big=(seed % 1000 == 999)))


def shard_seed(seed, max_edges=300000):
    return run(plan_shard(seed, max_edges=max_edges))


# ---------------------------------------------------------------- the oracle alone (tests/test_fuzz_plan_cpu.py)
def oracle_walk(p, passes):
    """The literal loop of a "ba" plan on the oracle alone, `passes` passes from the plan's base index: (final state, the loop indices it
    weakened in front of).  No GPU."""
    from oracle import oracle as orc_mod
    bal, kw = p["bal"], p["kw"]
    opts = driver.Options()
    opts.undamped_start = p["undamped_start"]
    K, state, _ = driver.build_inputs(bal, opts, hostlib)
    state["active_flag"] = p["active_flag"]
    okw = {k: v for k, v in kw.items() if k not in ("per_factor_mu", "tile_order")}
    O = orc_mod.Oracle(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K, params=_cabi.GbpParams.defaults(**okw))
    O.set_sum_order(1)
    O.upload(state)
    O.linearise()
    weakened = []
    for i in range(p["base"], p["base"] + passes):
        if weakens(i, p["steps"]):
            O.weaken_priors()
            weakened.append(i)
        O.iterate(1)
    out = dict(O.read())
    out.update(O.read_priors())
    O.close()
    return out, weakened
