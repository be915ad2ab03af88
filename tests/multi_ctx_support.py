"""Several contexts in one process: a deterministic schedule of calls and the isolated baseline it is compared with.

    plan(seed, n_ctx, ...)   draws, without a GPU, the contexts (graph, persistent, persist_coop, own or caller's stream) and ONE global list of
                             calls (ctx index, verb, argument).  A pure function of its arguments: a plain dict of names and numbers (the
                             graphs themselves are built from their names by graph(), cached).
    baseline(plan)           runs every context's OWN calls alone, everything else idle, and keeps what the calls returned and the final
                             state: the reference.  It is the same library, so what it anchors is isolation, not meaning; a hub-tree context
                             (tests/test_exact_inference.py) under float64 exact inference anchors meaning.
    run(plan)                the same calls in the plan's global order from one thread; run_threads(plan): one host thread per context.
    compare(got, want)       every tensor bit for bit (NaN == NaN), metric records included, graph_state() and the absence of a warning.

Graphs: the three shipped sequences (14 - 61 workgroups without the metric) and "half<k>" — fuzz_support.random_problem(size="half"),
600 - 680 tiles, a persistent grid of 150 - 170 workgroups: more than half of an MI355X's 256 CUs, so two of them fit one at a time and
not together.  grid(name) takes the counts from gbp_debug_persist_roles (the function the launcher uses), on the host.

Why an interleaved run can see a missing wait between two launches of the persistent kernel: every workgroup of such a launch spins until
ALL workgroups of its grid are resident.  Two grids whose sum exceeds the device's CUs and that are dispatched side by side can each hold
CUs the other one needs; both then sit in their bounded wait (1.5 s), give up, and the library restores the state and replays on the
two-kernel path — bit-identical results, but graph_state() drops from 2 and a `warning:` is left in gbp_last_error.  Those two are what
compare() asserts beside the bits, and over_device() is the precondition without which the assertion could not fail."""
import ctypes as C
import functools
import threading

import numpy as np

from tests import fuzz_support as fz
from tests.conftest import seq_path

SEQUENCES = ("fr1xyz", "fr1desk", "fr2robot2")
HALVES = ("half0", "half1", "half2")
HALF_SEED = 31000
BURSTS = ("iterate", "ba_loop", "ba_loop_metric", "iterate_eval_each")
OTHERS = ("weaken_priors", "set_stream", "sync", "read", "close")
VERBS = BURSTS + OTHERS
BA_STEPS = 3                    # gbp_ba_loop(n, iter0, 3): weakenings in front of the loop indices 1, 3 and 5 of a context
PLAN_SEEDS = (1, 2, 3, 4)       # the committed seeds of the drawn plans (tests/test_multi_ctx_plan_cpu.py: every verb occurs over them)
STATE_KEYS = ("cam_beliefs_eta", "cam_beliefs_lambda", "lmk_beliefs_eta", "lmk_beliefs_lambda", "damping", "damping_count", "robust_flag")


# ---------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def graph(name):
    """(bal, K, state) of a graph name: a shipped sequence, "half<k>", or "hub" (test_exact_inference.hub_tree)"""
    from gbp_poplar_amd import driver, hostlib
    if name in SEQUENCES:
        bal = hostlib.bal_read(seq_path(name))
    elif name.startswith("half"):
        bal = fz.random_problem(np.random.default_rng(HALF_SEED + int(name[4:])), size="half")
    elif name == "hub":
        from tests.test_exact_inference import hub_tree
        bal = hub_tree()[0]
    else:
        raise ValueError(name)
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    return bal, K, state


@functools.lru_cache(maxsize=None)
def grid(name):
    """(workgroups of a launch without the metric, with the metric after every pass, tiles) as the launcher of the persistent kernel
    computes them — on the host, through the test-hooks library"""
    from gbp_poplar_amd import _lib, hostlib
    bal = graph(name)[0]
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    nb = []
    for with_metric in (0, 1):
        dims = (C.c_uint32 * 4)()
        assert _lib.load(hooks=True).gbp_debug_persist_roles(lay["n_tiles"], bal["n_cams"], bal["n_lmks"], with_metric, dims, None, 0) == 0
        nb.append(int(dims[0]))
    return nb[0], nb[1], int(lay["n_tiles"])


def over_device(plan, cus, among=None):
    """the smallest launches (no metric) of the persistent contexts (all, or those of the indices `among`) — their sum, and whether it
    exceeds the device's CU count: only then can two of their launches, dispatched side by side, starve each other"""
    total = sum(grid(c["graph"])[0] for i, c in enumerate(plan["contexts"]) if c["persistent"] >= 0 and (among is None or i in among))
    return total, total > cus


# ---------------------------------------------------------------- plans
def plan(seed, n_ctx, graphs=None, persistent=None, coop=None, streams=None, rounds=6, burst=(10, 50), others=0.35, verbs=VERBS, params=None,
         calls=None):
    """n_ctx contexts and their calls.  graphs / persistent / coop / streams: one entry per context, or None = drawn (streams: "own", or
    "caller" = a torch.cuda.Stream; given only: "hip" = a stream the test creates and destroys through the runtime).  The calls go round
    robin over the contexts, `rounds` times; each turn is a burst verb of `burst` iterations, preceded with probability `others` by one
    of the other verbs — all of them restricted to `verbs`.  params: further gbp_params members per context (a list of dicts).  At most a
    few hundred iterations per context: rounds x burst[1].  calls: the list of calls written out by the caller instead (the tests of life
    times; beside VERBS it may use "destroy" and "create", the two halves of "close", and set_stream "fresh": a new "hip" stream)."""
    rng = np.random.default_rng(52000 + seed)
    pick = lambda given, draw: [given[i] if given is not None else draw() for i in range(n_ctx)]
    names = pick(graphs, lambda: (SEQUENCES + HALVES)[int(rng.integers(0, 6))])
    pers = pick(persistent, lambda: int(rng.choice([0, 0, 1, -1])))
    coops = pick(coop, lambda: int(rng.integers(0, 4) == 0))
    strs = pick(streams, lambda: ("own", "caller")[int(rng.integers(0, 2))])
    contexts = [{"graph": names[i], "persistent": pers[i], "persist_coop": coops[i] if pers[i] >= 0 else 0, "stream": strs[i],
                 "params": dict(params[i]) if params else {}, "grid": grid(names[i])} for i in range(n_ctx)]
    if calls is not None:
        return {"seed": seed, "contexts": contexts, "calls": [tuple(c) for c in calls]}
    bursts = [v for v in BURSTS if v in verbs]
    rest = [v for v in OTHERS if v in verbs]
    done = [0] * n_ctx          # loop index of each context: gbp_ba_loop continues the reference's loop where the context stands
    calls = []
    for _ in range(rounds):
        for i in range(n_ctx):
            if rest and rng.random() < others:
                v = rest[int(rng.integers(0, len(rest)))]
                arg = None
                if v == "set_stream":
                    arg = ("new", "own")[int(rng.integers(0, 3) == 0)]
                elif v == "read":
                    arg = ("host", "device")[int(rng.integers(0, 2))]
                elif v == "close":
                    done[i] = 0
                calls.append((i, v, arg))
            v = bursts[int(rng.integers(0, len(bursts)))]
            n = int(rng.integers(burst[0], burst[1] + 1))
            form = ("host", "device")[int(rng.integers(0, 2))] if "sync" in verbs else "device"      # (a host record is a blocking call)
            if v == "iterate":
                calls.append((i, v, n))
            elif v == "ba_loop":
                calls.append((i, v, (n, done[i], BA_STEPS)))
            elif v == "ba_loop_metric":
                calls.append((i, v, (n, done[i], BA_STEPS, form)))
            else:
                calls.append((i, v, (n, form)))
            done[i] += n
    return {"seed": seed, "contexts": contexts, "calls": calls}


def describe(p):
    return "seed %d | %s | %s" % (p["seed"], "  ".join("%d:%s p%+d c%d %s %r" % (i, c["graph"], c["persistent"], c["persist_coop"], c["stream"], c["grid"])
                                                        for i, c in enumerate(p["contexts"])),
                                  " ".join("%d.%s%s" % (i, v, "" if a is None else "(%s)" % (a,)) for i, v, a in p["calls"]))


# ---------------------------------------------------------------- streams the test owns
class HipStream:
    """A stream created and DESTROYED through the HIP runtime of this process (torch.cuda.Stream objects come from a pool that torch
    never gives back: dropping one destroys nothing)."""
    _hip = None

    def __init__(self):
        if HipStream._hip is None:
            path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)      # the ONE runtime torch and the library share
            HipStream._hip = C.CDLL(path)
        h = C.c_void_p()
        assert HipStream._hip.hipStreamCreateWithFlags(C.byref(h), C.c_uint(1)) == 0      # hipStreamNonBlocking
        self.cuda_stream = int(h.value)

    def destroy(self):
        if self.cuda_stream:
            assert HipStream._hip.hipStreamDestroy(C.c_void_p(self.cuda_stream)) == 0
            self.cuda_stream = 0


# ---------------------------------------------------------------- running a plan
class Ctx:
    """One context of a plan on the GPU: the engine, the stream objects it runs on, what its calls returned."""

    def __init__(self, spec):
        self.spec = spec
        self.bal, self.K, self.state = graph(spec["graph"])
        self.eng = None
        self.streams = []            # the caller's stream the context runs on (and, for torch's, whatever else is to stay alive)
        self.out = []                # (verb, result) of the calls that return something; device results converted by finish()
        self.last = None             # the verb of the context's last call
        self.create()

    def create(self):
        import torch
        from gbp_poplar_amd import _cabi
        from gbp_poplar_amd.engine import GbpEngine
        kw = dict(self.spec["params"], persistent=self.spec["persistent"], persist_coop=self.spec["persist_coop"])
        self.eng = GbpEngine(self.bal["cam_id"], self.bal["lmk_id"], self.bal["n_cams"], self.bal["n_lmks"], self.K,
                             params=_cabi.GbpParams.defaults(**kw), hooks=True)
        self.created_state, self.created_error = self.eng.graph_state(), self.eng.last_error()
        if self.spec["stream"] in ("caller", "hip"):      # torch's stream, or one the test creates and destroys itself
            self.streams = [torch.cuda.Stream() if self.spec["stream"] == "caller" else HipStream()]
            self.eng.set_stream(self.streams[-1].cuda_stream)
        self.eng.upload(self.state)
        self.eng.linearise()

    def _destroy_streams(self, streams):
        for s in streams:
            if isinstance(s, HipStream):
                s.destroy()

    def call(self, verb, arg):
        try:
            self._call(verb, arg)
        finally:
            self.last = verb

    def _call(self, verb, arg):
        import torch
        e = self.eng
        if verb == "set_stream":
            # What gbp_set_stream promises is about launches of the persistent kernel: it settles those in flight, and the next one orders
            # behind the last.  Other work of the ctx still in flight on the old stream (the two-kernel path, a weakening) is the caller's to
            # wait for, as with any work moved between streams — so the caller does, except right behind a burst of the persistent kernel.
            if e.graph_state() != 2 or self.last not in BURSTS:
                e.sync()
            old = self.streams
            if arg in ("new", "fresh"):      # torch's next stream / a stream of the test's own; the old object is dropped (destroyed)
                self.streams = [torch.cuda.Stream() if arg == "new" else HipStream()]
                e.set_stream(self.streams[-1].cuda_stream)
            else:                            # back on the ctx's own stream; the caller's stream is destroyed behind it
                e.set_stream(0)
                self.streams = []
            self._destroy_streams(old)
        elif verb == "destroy":              # ("close" in two halves, for the tests of life times: whatever is in flight, no sync first)
            e.close()
            self._destroy_streams(self.streams)
            self.streams = []
        elif verb == "create":
            self.create()
        elif verb == "iterate":
            e.iterate(arg)
        elif verb == "ba_loop":
            e.ba_loop(arg[0], arg[1], arg[2], metrics=False)
        elif verb == "ba_loop_metric":
            self.out.append((verb, e.ba_loop(arg[0], arg[1], arg[2], device=arg[3] == "device")))
        elif verb == "iterate_eval_each":
            self.out.append((verb, e.iterate_eval_each(arg[0], device=arg[1] == "device")))
        elif verb == "weaken_priors":
            e.weaken_priors()
        elif verb == "sync":
            e.sync()
        elif verb == "read":
            self.out.append((verb, e.read(device=arg == "device")))
        elif verb == "close":
            self._call("destroy", None)
            self.create()
        else:
            raise ValueError(verb)

    def finish(self):
        """everything the context holds, on the host: the results of its calls, every tensor of read(), both message sets, the priors,
        graph_state() and the text of last_error()"""
        e = self.eng
        e.sync()
        trace = {"calls": [(v, _to_host(r)) for v, r in self.out]}
        final = dict(e.read())
        final.update({"msg_" + k: v for k, v in e.messages().items()})
        final.update(e.read_priors())
        final["fac_eta"], final["fac_lambda"] = e.factor_potentials()
        trace.update(final=final, graph_state=e.graph_state(), last_error=e.last_error(), created_state=self.created_state)
        return trace

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None
        self._destroy_streams(self.streams)
        self.streams = []


def _to_host(r):
    """the result of a call as numpy: a list of metric dicts -> {field: array}, device tensors -> arrays"""
    if isinstance(r, list):
        return {k: np.array([x[k] for x in r]) for k in r[0]} if r else {}
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in r.items()}


def baseline(p):
    """every context alone: its own calls in the plan's order, nothing else in flight"""
    import torch
    traces = []
    for i, spec in enumerate(p["contexts"]):
        torch.cuda.synchronize()
        x = Ctx(spec)
        try:
            for j, verb, arg in p["calls"]:
                if j == i:
                    x.call(verb, arg)
            traces.append(x.finish())
        finally:
            x.close()
    torch.cuda.synchronize()
    return traces


def run(p, between=None):
    """the calls of all contexts in the plan's global order, from this thread; between(k, ctxs): called in front of call k (the tests of
    life times destroy and drop things there)"""
    ctxs = [Ctx(spec) for spec in p["contexts"]]
    try:
        for k, (i, verb, arg) in enumerate(p["calls"]):
            if between is not None:
                between(k, ctxs)
            ctxs[i].call(verb, arg)
        return [x.finish() for x in ctxs]
    finally:
        for x in ctxs:
            x.close()


def run_threads(p, timeout=60.0):
    """one host thread per context: the engine is created in its thread, the threads start their calls together behind a barrier.  A
    thread that has not returned within `timeout` seconds raises here — nothing more is launched (the caller must not go on to the GPU)."""
    n = len(p["contexts"])
    gate = threading.Barrier(n)
    traces, errors = [None] * n, [None] * n

    def work(i):
        x = None
        try:
            x = Ctx(p["contexts"][i])
            gate.wait(timeout)
            for j, verb, arg in p["calls"]:
                if j == i:
                    x.call(verb, arg)
            traces[i] = x.finish()
        except BaseException as err:      # noqa: B902 (handed to the test's thread)
            errors[i] = err
            gate.abort()
        finally:
            if x is not None:
                x.close()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    stuck = [i for i, t in enumerate(threads) if t.is_alive()]
    if stuck:
        raise TimeoutError("the threads of the contexts %r have not returned after %.0f s" % (stuck, timeout))
    for err in errors:
        if err is not None:
            raise err
    return traces


# ---------------------------------------------------------------- comparing
def no_warning(text):
    return text == "" or ("warning:" not in text and "timed out" not in text)


def compare(got, want, who):
    """one context's trace against its baseline: bits, path, no warning"""
    assert len(got["calls"]) == len(want["calls"]), who
    for k, ((v, a), (w, b)) in enumerate(zip(got["calls"], want["calls"])):
        assert v == w and set(a) == set(b), (who, k, v, w)
        for f in a:
            fz.same(a[f], b[f], "%s: call %d (%s): %s" % (who, k, v, f))
    for f in want["final"]:
        fz.same(got["final"][f], want["final"][f], "%s: final %s" % (who, f))
    assert got["graph_state"] == want["graph_state"], "%s: graph_state %d, alone %d (%s)" % (who, got["graph_state"], want["graph_state"], got["last_error"])
    assert no_warning(got["last_error"]), "%s: %s" % (who, got["last_error"])
    assert no_warning(want["last_error"]), "%s alone: %s" % (who, want["last_error"])


def compare_all(p, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        compare(g, w, "ctx %d (%s)" % (i, p["contexts"][i]["graph"]))
