"""A ctx that lives long enough for the counters of the persistent kernel's protocol to wrap.

Three counters keep counting for the life of a ctx (csrc/gbp_persist_seq.hpp, gbp_api_persist.cpp): the launch number persist.seq — its
low 19 bits make the tags of a launch's records, the whole 32 bits are what a time-out reports —, and the arrival counter of the
barriers with its host twin persist.epoch_base.  No run of the suite makes the half a million launches or the 2^32 arrivals that lead to
a wrap: gbp_debug_persist_counters puts a ctx in front of one.  The preset is a faithful stand-in for the long history only if the
shadows hold what real launches would have left, so every leg first runs at least two ordinary launches at the preset value and crosses
the wrap with real launches.

  references   (a) a twin ctx of the same build with untouched counters through the identical calls: EVERYTHING bit for bit, every field
                   of every metric record included (same kernel, same grid, same fold order) — two untouched twins are first compared
                   with each other, per graph;
               (b) a twin with persistent = -1: state, messages, potentials, priors, hoisted means and the integer counters of the metric
                   bit for bit, the two sums of a burst's last record within wide_state.sum_tolerance;
               (c) the CPU oracle on the final state of the leg (fuzz_support.against_oracle).
  every case   ends with graph_state() == 2, no warning in last_error() (no recovery happened), and a readback that shows that the counter
               really crossed: the value read after is numerically below the preset (tag and arrival legs: of the 19 / 32 bits that
               wrap); no launch was numbered 0 or got tag0 = 0.
  graphs       the smallest on which each grid form exists: "probe" (151 factors, 3 / 5 workgroups, every 4th dispatch slot), "gather"
               (1 409 factors, 18 / 30 workgroups), "big" (the smallest synth_generate(8, L, 2) graph, L in steps of 250, whose launch
               with the metric after every pass has more than 128 workgroups: every slot; its other launches 85: every 2nd slot).
  inputs       tests/wide_state.py: the placement profile on every graph, the relinearising one (a factor relinearises inside the bursts:
               the potentials change) on the two whose conditions tests/test_wide_state_cpu.py asserts.  The legs that compare metric
               sums run "gather" on the relinearising profile (PROFILE below).

  T  tag wrap, plain bursts, with what a keyframe loop does between them; one variant uploads two launches before the wrap
  K  tag wrap, every burst kind on every tag value round the wrap
  S  a record of one tag period ago under the tag a launch waits for: the metric means (written only by launches that carry the metric)
     and the second half of the landmark messages and row sums (written only by launches of two passes or more)
  A  the arrival counter across 2^32: a target of exactly 0, arrivals that straddle, the barrier kernel with 2^32 inside a burst
  Q  the 32-bit launch number across 0, device-form bursts left unvalidated on both sides

gbp_iterate(1) runs on the two-kernel path by design (a single iteration is as fast from two launches): a burst of one pass makes no
launch of the persistent kernel and does not advance persist.seq — the legs run such bursts too and count launches by the readback.
(c) is left out for T on "big": 4 096 oracle iterations of 10 500 factors are a minute of CPU.  profiles/long_lived.md has what each leg
showed before and after the fix."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import fuzz_support as fz
from tests import wide_state as ws
from tests.test_exact_inference import _engine, _oracle, rounded_trig  # noqa: F401

pytestmark = pytest.mark.gpu

PERIOD = 1 << 19
MASK = PERIOD - 1
GRAPHS = ("probe", "gather", "big")
# the profile of the legs that compare metric sums: "gather" has beliefs that are singular in float64 under the placement profile (no
# tolerance can be computed for them, wide_state.sum_tolerance) and runs them on the relinearising one, whose priors are full SPD blocks
PROFILE = {"probe": "placement", "gather": "relin", "big": "placement"}
CASES = [("probe", "placement"), ("gather", "placement"), ("big", "placement"), ("probe", "relin"), ("gather", "relin")]
INT_FIELDS = ("n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd")
BA_STEPS = 3                 # gbp_ba_loop(3, 1, 3): a weakening in front of pass 1 (a launch of its own) and one inside the launch, in front of pass 3


# ---- graphs and inputs ---------------------------------------------------------------------------------------------------------------
def _grid(bal, with_metric):
    """(workgroups of a launch of the persistent kernel, tiles) by the function the kernel's launcher uses, on the host"""
    from gbp_poplar_amd import _lib, hostlib
    lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
    dims = (C.c_uint32 * 4)()
    assert _lib.load(hooks=True).gbp_debug_persist_roles(lay["n_tiles"], bal["n_cams"], bal["n_lmks"], int(with_metric), dims, None, 0) == 0
    return int(dims[0]), int(lay["n_tiles"])


@functools.lru_cache(maxsize=None)
def big_graph_size():
    from gbp_poplar_amd import hostlib
    for n_lmks in range(4000, 8001, 250):
        nb = _grid(hostlib.synth_generate(8, n_lmks, 2, 7), True)[0]
        if nb > 128:
            assert nb <= 256, nb      # under the automatic limit
            return n_lmks
    raise AssertionError("no synth_generate(8, L, 2) graph with more than 128 workgroups")


@functools.lru_cache(maxsize=None)
def _case(name, profile):
    from gbp_poplar_amd import hostlib
    if name == "big":
        assert profile == "placement"
        bal = hostlib.synth_generate(8, big_graph_size(), 2, 7)
        state, K = ws.wide_state(bal, ws.PLACEMENT_SEED, "placement")
        return bal, state, K, {}
    if profile == "relin":
        return ws.relin_case(name) + (dict(ws.RELIN_PARAMS),)
    return ws.placement_case(name) + ({},)


def test_graphs_have_the_grid_forms_they_are_for():
    """every 4th dispatch slot up to 64 workgroups, every 2nd up to 128, every slot above (persist_spread)"""
    grids = {g: (_grid(_case(g, "placement")[0], False)[0], _grid(_case(g, "placement")[0], True)[0]) for g in GRAPHS}
    assert grids["probe"] == (3, 5) and _case("probe", "placement")[0]["n_edges"] == 151
    assert grids["gather"][1] <= 64 and _case("gather", "placement")[0]["n_edges"] == 1409
    assert 64 < grids["big"][0] <= 128 < grids["big"][1] <= 256, grids


# ---- the engines of a leg ----------------------------------------------------------------------------------------------------------------
def _ev_list(res, n):
    """metric records of a device-form call as a list of dicts (after a sync)"""
    cols = {k: v.cpu().numpy() for k, v in res.items()}
    return [{k: (float(v[j]) if v.dtype == np.float64 else int(v[j])) for k, v in cols.items()} for j in range(n)]


class Leg:
    """S: the ctx whose counters are preset; A: the untouched twin; B: persistent = -1; O: the oracle (or None).  Every verb runs on all
    of them; check() compares."""

    def __init__(self, name, profile, oracle_mod, oracle=True, barriers=False):
        self.name, self.profile = name, profile
        self.bal, self.state, self.K, self.kw = _case(name, profile)
        self.S, self.A = _engine(self.bal, self.K, **self.kw), _engine(self.bal, self.K, **self.kw)
        self.B = _engine(self.bal, self.K, persistent=-1, **self.kw)
        self.O = _oracle(oracle_mod, self.bal, self.K, **self.kw) if oracle else None
        self.oracle_mod = oracle_mod
        if name == "probe":
            oracle_mod.set_threads(1)      # (151 factors: the oracle's thread team costs more than it gives)
        for x in (self.S, self.A):
            assert x.graph_state() == 2, x.last_error()
            if barriers:
                x.persist_flow(0)
        assert self.B.graph_state() != 2
        self.active = np.array(self.state["active_flag"], np.uint32)
        self.held = []               # device-form records not compared yet: (what, n, [S, A, B results])
        self.launches = []           # numbers the launches of S got, by the readback
        self.preset = None
        self.done = 0
        self.upload()
        self.fac0 = self.S.factor_potentials()

    def close(self):
        if self.name == "probe":
            self.oracle_mod.set_threads(int(os.environ.get("OMP_NUM_THREADS", "1")))
        for x in (self.S, self.A, self.B, self.O):
            if x is not None:
                x.close()

    def everyone(self):
        return [x for x in (self.S, self.A, self.B, self.O) if x is not None]

    def upload(self):
        self.active = np.array(self.state["active_flag"], np.uint32)
        if self.O is not None and self.done:      # (gbp_upload clears the messages, the oracle's upload keeps them: a new oracle)
            self.O.close()
            self.O = _oracle(self.oracle_mod, self.bal, self.K, **self.kw)
        self.done = 0
        for x in self.everyone():
            x.upload(self.state)
            x.linearise()

    # ---- the counters ----
    def counters(self):
        return self.S.persist_counters()

    def set_counters(self, seq=None, epoch_base=None):
        self.preset = self.S.persist_counters(seq=seq, epoch_base=epoch_base)
        assert (seq is None or self.preset[0] == seq & 0xffffffff) and (epoch_base is None or self.preset[1] == epoch_base & 0xffffffff)

    # ---- bursts ----
    def burst(self, kind, n, check=True, launches=1):
        """one call of `kind` on every engine; compares its records and (check) everything else.  launches: how many launches of the
        persistent kernel the call is (asserted on S by the readback; the numbers they got are kept)"""
        before = self.counters()[0]
        res = []
        for x in (self.S, self.A, self.B):
            if kind == "plain":
                x.iterate(n)
                res.append(None)
            elif kind == "at_end":
                x.iterate_eval(n)
                res.append([x.eval_end()])
            elif kind == "each":
                res.append(x.iterate_eval_each(n))
            elif kind == "ba":
                res.append(x.ba_loop(n, 1, BA_STEPS))
            elif kind == "each_dev":
                res.append(x.iterate_eval_each(n, device=True))
            elif kind == "ba_dev":
                res.append(x.ba_loop(n, 1, BA_STEPS, device=True))
            else:
                raise ValueError(kind)
        if self.O is not None:
            if kind in ("ba", "ba_dev"):
                for k in range(n):
                    if ws.weakens(1 + k, BA_STEPS):
                        self.O.weaken_priors()
                    self.O.iterate(1)
            else:
                self.O.iterate(n)
        self.done += n
        after = self.counters()[0]
        got = []
        s = before
        while s != after and len(got) <= launches + 1:      # the numbers in between: +1 each, a skipped number is no launch
            s = (s + 1) & 0xffffffff
            got.append(s)
        if len(got) == launches + 1:                         # one more number than launches: one was skipped — only ever a multiple of 2^19
            skipped = [g for g in got if g & MASK == 0]
            assert len(skipped) == 1, (kind, n, before, after)
            got.remove(skipped[0])
        assert len(got) == launches, "%s(%d) made %d launches of the persistent kernel (seq %d -> %d), expected %d" % (kind, n, len(got), before, after, launches)
        self.launches += got
        what = "%s(%d) as launch %s after %d passes" % (kind, n, ["0x%x" % g for g in got], self.done)
        if kind.endswith("_dev"):
            self.held.append((what, n, res))
        elif res[0] is not None:
            self._records(what, res, sums=check)
        if check:
            self.check(what)
        return got

    def _records(self, what, res, sums):
        s, a, b = res
        assert fz.ev_equal(s, a), "%s: the metric differs from the untouched twin's: %r vs %r" % (what, s, a)
        for k, (x, y) in enumerate(zip(s, b)):
            for f in INT_FIELDS:
                assert x[f] == y[f], "%s: %s of record %d differs from persistent = -1: %r vs %r" % (what, f, k, x[f], y[f])
        if sums:      # the last record is the metric of the beliefs S holds now
            x, y = s[-1], b[-1]
            beliefs = self.S.read()
            if ws.all_finite(beliefs) and all(np.isfinite(x[f]) and np.isfinite(y[f]) for f in ("sum_norm", "sum_half_sq")):
                tol = ws.sum_tolerance(beliefs, self.bal, self.K, dict(self.state, active_flag=self.active))
                for f, t in zip(("sum_norm", "sum_half_sq"), tol):
                    assert abs(x[f] - y[f]) <= t, "%s: %s differs from persistent = -1 by %.3g, tolerance %.3g (%r vs %r)" % (what, f, abs(x[f] - y[f]), t, x[f], y[f])
            else:
                assert all((x[f] == y[f]) or (x[f] != x[f] and y[f] != y[f]) for f in ("sum_norm", "sum_half_sq")), (what, x, y)

    def release(self):
        """the device-form records held back: compared once everything has been waited for (the state has moved on: no tolerance)"""
        for x in (self.S, self.A, self.B):
            x.sync()
        for what, n, res in self.held:
            self._records(what, [_ev_list(r, n) for r in res], sums=False)
        self.held = []

    # ---- what a keyframe loop does between bursts ----
    def weaken_priors(self):
        for x in self.everyone():
            x.weaken_priors()

    def keyframe(self, share):
        """NEW_KEYFRAME: `share` of the inactive factors become active, every count re-armed as slam.cpp does, the weaken flags set again"""
        rng = np.random.default_rng(len(self.launches) + 77)
        off = np.flatnonzero(self.active == 0)
        on = off[rng.random(off.size) < share] if share < 1.0 else off
        self.active = self.active.copy()
        self.active[on] = 1
        E, Cn, L = self.bal["n_edges"], self.bal["n_cams"], self.bal["n_lmks"]
        upd = {"damping_count": np.full(E, -15, np.int32), "active_flag": self.active,
               "cam_weaken_flag": rng.integers(0, 8, Cn).astype(np.uint32), "lmk_weaken_flag": rng.integers(0, 8, L).astype(np.uint32)}
        for x in self.everyone():
            x.new_keyframe(upd)
        return on.size

    def read_forms(self, form):
        """gbp_read in `form` on S and A: equal to each other and to the host form"""
        host = self.S.read()
        for x in (self.S, self.A):
            got = fz.DeviceForms(x, form).read()
            for k in host:
                fz.same(got[k], host[k], "read in %s form: %s" % (form, k))

    # ---- comparing ----
    def check(self, what):
        snap = fz.snapshot(self.S)
        snap.update(self.S.read_priors())
        for who, x in (("the untouched twin", self.A), ("persistent = -1", self.B)):
            other = fz.snapshot(x)
            other.update(x.read_priors())
            for k in snap:
                fz.same(snap[k], other[k], "%s: %s against %s" % (what, k, who))

    def finish(self, crossed):
        """the end of every case; crossed(preset, after) says whether the readback shows the wrap"""
        self.release()
        self.check("end of the leg")
        if self.O is not None:
            fz.against_oracle(self.S, self.O, self.done, potentials=True)
            po, ps = self.O.read_priors(), self.S.read_priors()
            for k in po:
                fz.same(ps[k], po[k], "priors against the oracle: %s" % k)
        if self.profile == "relin":
            assert not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(self.fac0, self.S.factor_potentials())), "no factor relinearised in this leg"
        for x in (self.S, self.A):
            err = x.last_error()
            assert x.graph_state() == 2 and (err == "" or (err.startswith("info: gbp_create") and "warning" not in err and "timed out" not in err)), err
        after = self.counters()
        assert crossed(self.preset, after), "the counters did not cross the wrap: preset %r, after %r, launches %r" % (self.preset, after, self.launches)
        # no launch numbered 0 (the status word's "no launch failed"), none with tag0 = 0 (the tag of a record nobody wrote)
        assert all(g & MASK for g in self.launches), "launch numbers with tag0 = 0: %r" % (["0x%x" % g for g in self.launches if not g & MASK],)


def _tag_crossed(preset, after):
    return (after[0] & MASK) < (preset[0] & MASK)


def _arrivals_crossed(preset, after):
    return after[1] < preset[1]


@pytest.fixture
def leg(oracle_mod, rounded_trig, request):
    made = []

    def make(name, profile, **kw):
        made.append(Leg(name, profile, oracle_mod, **kw))
        return made[-1]

    yield make
    for x in made:
        x.close()


# ---- the hook --------------------------------------------------------------------------------------------------------------------------
def test_counters_hook_reads_sets_and_refuses():
    from gbp_poplar_amd.engine import GbpError
    bal, state, K, kw = _case("probe", "placement")
    eng, off = _engine(bal, K, **kw), _engine(bal, K, persistent=-1, **kw)
    for x in (eng, off):
        x.upload(state)
        x.linearise()
    assert eng.persist_counters() == (0, 0)
    eng.iterate(2)
    eng.iterate_eval(2)
    eng.eval_end()
    seq, arrivals = eng.persist_counters()
    assert seq == 2 and arrivals == _grid(bal, False)[0]      # two launches, one of them with a barrier of every workgroup
    assert eng.persist_counters(seq=77) == (77, arrivals) and eng.persist_counters(epoch_base=5) == (77, 5)
    assert eng.persist_counters(seq=0xfffffffe, epoch_base=0xffffffff) == (0xfffffffe, 0xffffffff) == eng.persist_counters()
    with pytest.raises(GbpError, match="does not run in the persistent kernel"):
        off.persist_counters()
    with pytest.raises(GbpError, match="does not run in the persistent kernel"):
        off.persist_counters(seq=1)
    for x in (eng, off):
        x.close()


# ---- (a) rests on this: two untouched twins agree ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_two_untouched_twins_agree_bit_for_bit(name, leg):
    """every burst kind, a keyframe and a weakening, nothing preset: S and A are two ctxs of one build through the same calls"""
    x = leg(name, PROFILE[name])
    for kind, n in (("plain", 2), ("at_end", 3), ("each", 5), ("ba", 3), ("each_dev", 3), ("ba_dev", 3), ("plain", 7), ("at_end", 16)):
        x.burst(kind, n, check=not kind.endswith("_dev"), launches=2 if (kind, n) == ("at_end", 16) else 1)
        if kind == "each":
            x.keyframe(0.5)
            x.weaken_priors()
    x.preset = (1, 1)
    x.finish(lambda preset, after: after[0] == 9)      # (nothing to cross: nine launches, numbered 1 .. 9)


# ---- T ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, profile", CASES)
def test_tag_wrap_plain_bursts_of_a_keyframe_loop(name, profile, leg):
    """bursts of 1, 2, 7, 4 096, 1, 3 and 2 passes from persist.seq = 2^19 - 4: the launches get 0x7fffd, 0x7fffe, 0x7ffff — the 4 096
    passes on the largest tag there is — and the two behind the wrap; between them WEAKEN_PRIORS, NEW_KEYFRAME activating factors, gbp_read
    in device and host form.  No upload."""
    x = leg(name, profile, oracle=name != "big")
    x.set_counters(seq=PERIOD - 4)
    x.burst("plain", 1, launches=0)
    assert x.burst("plain", 2) == [PERIOD - 3]
    x.weaken_priors()
    assert x.burst("plain", 7) == [PERIOD - 2]
    assert x.keyframe(0.5) > 0
    assert x.burst("plain", 4096) == [PERIOD - 1]
    x.read_forms("device")
    x.burst("plain", 1, launches=0)
    x.weaken_priors()
    x.burst("plain", 3)
    x.read_forms("host")
    assert x.keyframe(1.0) > 0
    x.burst("plain", 2)
    x.finish(_tag_crossed)


def test_tag_wrap_with_an_upload_two_launches_before(leg):
    """gbp_upload zeroes the arrival counter and its host twin, not the launch number: the tags go on where they were"""
    x = leg("probe", "placement")
    x.set_counters(seq=PERIOD - 6)
    x.burst("plain", 2)
    x.burst("at_end", 3)
    seq, arrivals = x.counters()
    assert seq == PERIOD - 4 and arrivals == _grid(x.bal, False)[0]
    x.upload()
    assert x.counters() == (PERIOD - 4, 0)
    assert x.burst("plain", 2) == [PERIOD - 3]
    assert x.burst("at_end", 5) == [PERIOD - 2]
    assert x.burst("each", 3) == [PERIOD - 1]
    x.burst("plain", 3)
    x.burst("at_end", 2)
    x.finish(_tag_crossed)


# ---- K ------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("plain", "at_end", "series_host", "series_device")      # the four BurstKinds
K_CASES = [("probe", "placement"), ("gather", "relin"), ("big", "placement")]


@pytest.mark.parametrize("rotation", range(4))
@pytest.mark.parametrize("name, profile", K_CASES)
def test_tag_wrap_every_burst_kind_on_every_tag(name, profile, rotation, leg):
    """the four kinds on the launches 0x7fffe, 0x7ffff and the two behind the wrap, rotated so that every kind meets every one; the
    series kinds as gbp_iterate_eval_each and gbp_ba_loop in turn; nothing waits between a device-form burst and the launch behind it"""
    x = leg(name, profile)
    x.set_counters(seq=PERIOD - 5)
    x.burst("plain", 2)
    x.burst("plain", 3)
    assert x.counters()[0] == PERIOD - 3
    numbers = []
    for slot in range(4):
        kind = KINDS[(slot + rotation) % 4]
        if kind == "series_host":
            kind = "each" if rotation % 2 == 0 else "ba"
        elif kind == "series_device":
            kind = "ba_dev" if rotation % 2 == 0 else "each_dev"
        numbers += x.burst(kind, 3, check=not kind.endswith("_dev"))
    assert numbers[:2] == [PERIOD - 2, PERIOD - 1] and len(numbers) == 4
    x.finish(_tag_crossed)


# ---- S ------------------------------------------------------------------------------------------------------------------------------------
S_VARIANTS = {
    # first call, fillers (four of them, then as many more as the tags need), the call on the first one's tag one period later
    "metric_at_end": (("at_end", 3), ("plain", 2), ("at_end", 3)),
    "metric_each": (("each", 5), ("plain", 2), ("each", 5)),                 # (from its third pass on a launch has rewritten both halves itself)
    "metric_each_two_passes": (("each", 2), ("plain", 2), ("each", 2)),      # ... a launch of two passes has not
    "other_pass_count": (("at_end", 3), ("plain", 2), ("at_end", 4)),        # the control: its tags are not the stale records'
    "second_half": (("plain", 2), ("each", 1), ("plain", 2)),                # launches of one pass leave the second half of LMSG / ROWP alone
}


@pytest.mark.parametrize("variant", sorted(S_VARIANTS))
@pytest.mark.parametrize("name", GRAPHS)
def test_records_of_one_tag_period_ago(name, variant, leg):
    """A launch at a small number, launches that do not write the shadow in question, then — across a real wrap of the low 19 bits — the
    same call as the launch whose low 19 bits are the first one's: the shadows then hold, under exactly the tags this launch waits for,
    what the first launch published.  (The preset stands for the launches of a whole period that do not touch those shadows.)
    Before the launch that begins a tag period cleared the shadows, metric_at_end, metric_each_two_passes and second_half failed on
    every graph (probe: sum_norm 306.54 / 332.36 against 201.05 / 203.68; every camera belief wrong); metric_each passed — from its
    third pass on such a launch has rewritten both halves of the metric shadows itself — and so did the control."""
    first, filler, again = S_VARIANTS[variant]
    x = leg(name, PROFILE[name])
    x.burst("plain", 2)
    (m,) = x.burst(*first)
    for _ in range(4):
        x.burst(*filler)
    x.set_counters(seq=PERIOD - 2)
    for _ in range(8):      # across the wrap with real launches, up to the number in front of m's twin
        if (x.counters()[0] & MASK) == ((m - 1) & MASK) and x.counters()[0] > PERIOD:
            break
        x.burst(*filler)
    else:
        raise AssertionError("never reached the launch in front of 0x%x: %r" % (m, x.launches))
    (m2,) = x.burst(*again)
    assert m2 & MASK == m & MASK and m2 != m, (m, m2)
    x.burst("plain", 2)
    x.finish(_tag_crossed)


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ("target_zero", "straddle"))
@pytest.mark.parametrize("name", GRAPHS)
def test_arrival_counter_wraps_at_the_barrier_of_a_metric_launch(name, where, leg):
    """the one barrier of a launch that carries the metric: its target epoch_base + workgroups is exactly 0 (the metric at the end), or
    the arrivals straddle 2^32 from 2^32 - workgroups / 2 (the metric after every pass: the larger grid)"""
    x = leg(name, PROFILE[name])
    kind, n = ("at_end", 3) if where == "target_zero" else ("each", 3)
    nb = _grid(x.bal, kind == "each")[0]
    start = -nb if where == "target_zero" else -(nb // 2)
    x.set_counters(epoch_base=start - 2 * nb)
    for k in (1, 0):
        x.burst(kind, n)
        x.burst("plain", 2)
        assert x.counters()[1] == (start - k * nb) & 0xffffffff, (x.counters(), nb)      # every launch with the metric: one arrival per workgroup
    x.burst(kind, n)
    assert x.counters()[1] == (0 if where == "target_zero" else nb - nb // 2)
    x.finish(_arrivals_crossed)


@pytest.mark.parametrize("metric", (False, True))
@pytest.mark.parametrize("name", GRAPHS)
def test_arrival_counter_wraps_inside_a_burst_of_the_barrier_kernel(name, metric, leg):
    """k_persist (gbp_debug_persist_flow(ctx, 0)): a burst of 9 passes is 17 barriers, 18 with the metric; 2^32 arrivals fall between the
    8th and the 9th of the third burst"""
    x = leg(name, PROFILE[name], barriers=True)
    kind = "at_end" if metric else "plain"
    nb, per = _grid(x.bal, False)[0], 18 if metric else 17
    x.set_counters(epoch_base=-(8 * nb + nb // 2) - 2 * per * nb)
    for k in (1, 0):
        x.burst(kind, 9)
        assert x.counters()[1] == (-(8 * nb + nb // 2) - k * per * nb) & 0xffffffff, (x.counters(), nb, per)
    x.burst(kind, 9)
    x.finish(_arrivals_crossed)


# ---- Q ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_launch_number_crosses_zero(name, leg):
    """from persist.seq = 0xfffffffb: two ordinary launches, then six of mixed kinds across 0 — two device-form series bursts stay
    unvalidated in front of a gbp_eval_end, whose persist_check(ctx, upto) then compares launch numbers of both sides of the wrap.  No
    launch is numbered 0: the one behind 0xffffffff is 1."""
    x = leg(name, PROFILE[name])
    x.set_counters(seq=0xfffffffb)
    x.burst("plain", 2)
    x.burst("plain", 3)
    assert x.counters()[0] == 0xfffffffd
    assert x.burst("each_dev", 3, check=False) == [0xfffffffe]
    assert x.burst("each_dev", 2, check=False) == [0xffffffff]
    first = x.burst("at_end", 2)           # its gbp_eval_end validates up to this launch: the two in front of it are across the wrap
    x.burst("ba_dev", 3, check=False)
    x.burst("at_end", 3)
    x.burst("each", 2)
    assert first == [1], "the launch behind 0xffffffff was numbered %r" % (first,)
    x.finish(lambda preset, after: after[0] < preset[0] and after[0] == 4)
