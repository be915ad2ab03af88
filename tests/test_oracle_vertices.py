"""Pin of the oracle's VERTEX layer (oracle_gbp.c: the seven vertex classes of the reference's ba/gbp_codelets.cpp).

1. against the reference's own compute() bodies — gbp_codelets.cpp compiled unmodified against our stand-in for the Poplar field
   wrappers (oracle/poplar_standin, oracle/ref_vertex_adapter.cpp; `make -C oracle ref`, out of tree, build container only): the
   restatement's orc_vertex_* equal rv_* BIT FOR BIT on every generated case of tests/vertex_cases.py, the case set meets its
   conditions (finite outside the non-finite group, every decision boundary hit on both sides and exactly on it), and the
   regenerated fixture equals the committed one;
2. everywhere: against tests/golden/vertex_cases.npz (the reference vertices' outputs on a sub-sample of every group), bit for
   bit, and in trig mode 1 against its `dev_` outputs.

What this does not pin: the graph wiring of ba.cpp and the summation order of popops::reduceWithOutput.
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import vertex_cases as vc

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vertex_cases.npz"))
HAVE_REF = orc.have("ref_vertices")
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference-vertex build absent (make -C oracle ref; needs /root/reference)")


def same_bits(a, b):
    """bit for bit, NaNs of any payload equal to each other (the non-finite group)"""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _run_mine(X, op, trig=0):
    orc.set_trig_mode(trig)
    try:
        return vc.run_cpu(orc.vertex_api("restatement"), X, op)
    finally:
        orc.set_trig_mode(0)


@pytest.fixture(scope="module")
def full():
    X, g = vc.all_cases()
    has_ref = vc.field(X, "relin_mode")[:, 0] == 0
    ref = orc.vertex_api("ref_vertices")
    assert orc.load("ref_vertices").rv_impl_name() == b"reference"
    return {"X": X, "g": g, "has_ref": has_ref, "ref": {op: vc.run_cpu(ref, X[has_ref], op) for op in (0, 1)}}


@needs_ref
def test_restatement_equals_reference_vertices_bit_for_bit(full):
    X, g, has_ref = full["X"], full["g"], full["has_ref"]
    assert len(X) >= 18000 and has_ref.sum() == len(X) - (g == vc.GID["relin_reset"]).sum()
    for op in (0, 1):
        mine = _run_mine(X[has_ref], op)
        ok = same_bits(mine, full["ref"][op])
        bad = np.nonzero(~ok.all(axis=1))[0]
        assert bad.size == 0, (op, bad[:5], [vc.GROUPS[i] for i in g[has_ref][bad[:5]]],
                               [k for k, (o, w) in vc.OUT_OFF.items() if not ok[bad[0], o:o + w].all()])
    W = vc.weaken_cases()
    a, b = vc.run_weaken(orc.vertex_api("ref_vertices"), W), vc.run_weaken(orc.vertex_api("restatement"), W)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@needs_ref
def test_case_set_meets_its_conditions_on_the_reference(full):
    """Checked with the reference's vertices alone: all-finite outputs outside the non-finite group; every branch taken and
    refused in every boundary group; each boundary hit exactly; at least a quarter of the conditioning cases with a non-positive
    pivot; the non-finite group is non-finite.  Prints the case and branch counts (the figures the documents quote)."""
    X, g = full["X"][full["has_ref"]], full["g"][full["has_ref"]]
    y0, y1 = full["ref"][0], full["ref"][1]
    rel, rob1, rob0 = vc.relinearised(X, y1), vc.field(y1, "robust", True)[:, 0] == 1, vc.field(y0, "robust", True)[:, 0] == 1
    act = vc.field(X, "active")[:, 0] == 1
    print("\ngroup          cases  relinearised  robust(op 1)  robust(op 0)  active")
    for gi, name in enumerate(vc.GROUPS):
        m = g == gi
        n_all = int((full["g"] == gi).sum())
        print("%-13s %6d %13d %13d %13d %7d" % (name, n_all, rel[m].sum(), rob1[m].sum(), rob0[m].sum(), act[m].sum()))
    nonf = g == vc.GID["nonfinite"]
    assert vc.finite_rows(y0)[~nonf].all() and vc.finite_rows(y1)[~nonf].all()
    assert 8 <= nonf.sum() <= 32 and not (vc.finite_rows(y0)[nonf] & vc.finite_rows(y1)[nonf]).any()
    # branches: relinearised / not, robust / not, active / not — none empty
    for m in (rel, rob1, rob0, act):
        assert m[~nonf].any() and (~m[~nonf]).any()
    # damping_count: both outcomes for every parameter set, and count 0 picks up maxeta_damping
    m = g == vc.GID["count"]
    for prm in vc.PARAMS:
        p = m & (vc.field(X, "nund")[:, 0] == prm[1])
        thr = prm[3] - prm[1]
        still = vc.field(y1, "dmu", True)[:, 0] == 0
        cin = vc.field(X, "count")[:, 0]
        assert np.array_equal(rel[p & still], cin[p & still] + 1 > thr) and rel[p & still].any() and (~rel[p & still]).any()
        assert (cin[p & still] + 1 == thr).any() and (cin[p & still] + 1 == thr + 1).any()      # exactly on / first past the test
        assert not rel[p & ~still].any()
        zero = p & (cin == 0)
        assert np.all(vc.field(y1, "damping", True)[zero, 0] == np.float32(prm[0]))
    # dmu: thirds below / on / above the threshold; only "below" relinearises
    m = g == vc.GID["dmu"]
    d, t = vc.field(y1, "dmu", True)[m, 0], vc.field(X, "thr")[m, 0]
    assert (d == t).sum() * 3 == m.sum() and (d < t).sum() * 3 == m.sum() and (d > t).sum() * 3 == m.sum()
    assert np.array_equal(rel[m], d < t)
    assert np.all(np.abs(d.view(np.int32) - t.view(np.int32)) <= 1)
    # err: thirds below / on / above Nstds * sqrt(var), for RelineariseFactorVertex and PrepMessageVertex alike
    m = g == vc.GID["err"]
    mu = vc.field(y1, "mu", True)[m]
    err = vc.err_of(X[m], mu, 0)
    thr = (vc.field(X, "nstds")[m, 0] * np.sqrt(vc.field(X, "var")[m, 0])).astype(np.float32)
    assert rel[m].all() and (err == thr).sum() * 3 == m.sum() and (err > thr).sum() * 3 == m.sum()
    assert np.all(np.abs(err.view(np.int32) - thr.view(np.int32)) <= 1)
    assert np.array_equal(rob1[m], err > thr) and np.array_equal(rob0[m], err > thr)
    # inactive: messages zero, everything else untouched
    m = g == vc.GID["inactive"]
    assert not act[m].any() and np.abs(vc.field(X, "pce")[m]).sum() > 0 and np.abs(vc.field(X, "fl")[m]).sum() > 0
    for k in ("mce", "mcl", "mle", "mll"):
        assert not vc.field(y1, k, True)[m].any()
    for k, kin in (("fe", "fe"), ("fl", "fl"), ("mu", "oldmu"), ("damping", "damping"), ("count", "count"), ("robust", "robust")):
        assert np.array_equal(vc.field(y1, k, True)[m], vc.field(X, kin)[m]), k
    # conditioning: non-positive pivots, scales
    m = g == vc.GID["conditioning"]
    p3, p6 = vc.schur_pivots(X[m])
    nonpos = (p3 <= 0).any(axis=1) | (p6 <= 0).any(axis=1)
    print("conditioning: %d of %d cases with a non-positive pivot (3x3: %d, 6x6: %d)" % (nonpos.sum(), m.sum(), (p3 <= 0).any(axis=1).sum(), (p6 <= 0).any(axis=1).sum()))
    assert nonpos.sum() * 4 >= m.sum()
    for k in ("cbl", "lbl"):
        top = np.max(np.abs(vc.field(X, k)[m]), axis=1)
        assert top.min() < 1e-5 and top.max() > 1e7
    # geometry: ranges
    m = g == vc.GID["geometry"]
    w = np.linalg.norm(vc.field(X, "oldmu")[m, 3:6].astype(np.float64), axis=1)
    assert rel[m].all() and 1e-6 < w.min() < 3e-6 and w.max() > 5.9
    # WeakenPriorVertex: weakened / not
    W = vc.weaken_cases()
    o = vc.run_weaken(orc.vertex_api("ref_vertices"), W)
    weak = o["flag"] != W["flag"]
    print("weaken: %d cases, %d weakened" % (len(weak), weak.sum()))
    assert np.array_equal(weak, (W["flag"] >= 1) & (W["flag"] <= 5)) and weak.any() and (~weak).any()


@needs_ref
def test_regenerated_golden_equals_the_committed_one():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    new = mg.vertex_cases()
    assert sorted(new) == sorted(G.files)
    for k, v in new.items():
        v = np.asarray(v)
        assert v.shape == G[k].shape and v.tobytes() == G[k].astype(v.dtype).tobytes(), k


def test_restatement_reproduces_the_golden_vertex_outputs_bit_for_bit():
    """`ref_`: the reference's own vertex classes (libm trig) — trig mode 0 here calls the host's libm as well; `dev_`: trig mode 1."""
    x, has_ref = G["x"], G["has_ref"]
    assert set(G["group"]) == set(range(len(vc.GROUPS))) and has_ref.sum() >= 90
    for op in (0, 1):
        mine = _run_mine(x, op)
        ok = same_bits(mine[has_ref], G["ref_op%d" % op][has_ref])
        assert ok.all(), ("ref", op, np.nonzero(~ok.all(axis=1))[0][:5])
        ok = same_bits(_run_mine(x, op, trig=1), G["dev_op%d" % op])
        assert ok.all(), ("dev", op, np.nonzero(~ok.all(axis=1))[0][:5])
    W = {k[len("weaken_in_"):]: G[k] for k in G.files if k.startswith("weaken_in_")}
    o = vc.run_weaken(orc.vertex_api("restatement"), W)
    for k, v in o.items():
        assert np.array_equal(v, G["weaken_ref_" + k]), k


def test_committed_cases_are_the_generated_ones():
    """The fixture's inputs are rows of the generator's output (so the GPU test, which regenerates the full set, and the fixture
    speak about the same cases), and the generator is deterministic."""
    X, g = vc.all_cases()
    assert np.array_equal(G["index"], vc.golden_subset(g))
    assert X[G["index"]].tobytes() == G["x"].tobytes() and np.array_equal(g[G["index"]], G["group"])
    assert np.array_equal(G["full_counts"][:, 0], np.bincount(g, minlength=len(vc.GROUPS)))
    # the potentials have the form the device stores: symmetric Lambda_cc / Lambda_ll, Lambda_lc = Lambda_cl^T
    fl = vc.field(X, "fl")
    assert np.array_equal(fl[:, :36].reshape(-1, 6, 6), fl[:, :36].reshape(-1, 6, 6).transpose(0, 2, 1))
    assert np.array_equal(fl[:, 72:].reshape(-1, 3, 3), fl[:, 72:].reshape(-1, 3, 3).transpose(0, 2, 1))
    assert np.array_equal(fl[:, 54:72].reshape(-1, 3, 6), fl[:, 36:54].reshape(-1, 6, 3).transpose(0, 2, 1))


def test_relin_mode_reset_is_relinearisation_on_a_zeroed_potential():
    """relin_mode 1 has no counterpart in the reference; it is pinned through mode 0: a relinearising case equals the same case
    with a zeroed potential, a non-relinearising one is unchanged."""
    X, g = vc.all_cases()
    x = np.array(X[g == vc.GID["relin_reset"]])
    y = _run_mine(x, 1)
    rel = vc.relinearised(x, y)
    assert rel.any() and (~rel).any()
    x0 = x.copy()
    vc.field(x0, "relin_mode")[:] = 0
    vc.field(x0, "fe")[rel] = 0
    vc.field(x0, "fl")[rel] = 0
    assert same_bits(y, _run_mine(x0, 1)).all()
