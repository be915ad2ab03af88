"""The device's VERTEX layer — relin_core and factor_update of csrc/kernels/gbp_vertex.hpp, the per-lane code of every sweep kernel —
against the vertex cases of tests/vertex_cases.py, one lane per case through the test hook gbp_debug_vertex:

  * == the restatement (oracle_gbp.c, trig mode 1: the device's convention) on the FULL generated set, ops 0 / 1 / 2, bit for bit;
  * == tests/golden/vertex_cases.npz `dev_` on the committed sub-sample, bit for bit;
  * against its `ref_` — the outputs of the REFERENCE's own vertex classes (libm trig) — flags and counters equal, floats within
    the tolerances of test_gpu_parity.py::test_golden_vertex_vectors (1e-4 where no relinearisation happens, 1e-3 where one does,
    as max |diff| / max |ref| over the sample).

Non-finite group: bits are not compared (gbp_device_math.hpp: skipped structural zeros differ for non-finite inputs); every output
tensor that is non-finite in the restatement / the reference is non-finite on the device, and the integer outputs are equal.
This file reads the fixture and the restatement only — never the reference.
"""
import os

import numpy as np
import pytest

from tests import vertex_cases as vc
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vertex_cases.npz"))
FLOAT_FIELDS = [k for k, _ in vc.OUT_FIELDS if k not in vc.INT_FIELDS]
INT_FIELDS = [k for k, _ in vc.OUT_FIELDS if k in vc.INT_FIELDS]


def _dev(op, X):
    from gbp_poplar_amd import _cabi as cabi
    from gbp_poplar_amd._lib import load
    lib = load(hooks=True)
    X = np.ascontiguousarray(X, np.float32)
    out = np.zeros((X.shape[0], vc.W_OUT), np.float32)
    rc = lib.gbp_debug_vertex(op, cabi.ptr(X.reshape(-1), cabi.c_f32p), cabi.ptr(out.reshape(-1), cabi.c_f32p), X.shape[0])
    assert rc == 0, lib.gbp_last_error(None)
    return out


def _check_bits(dev, exp, X, group, op, what):
    """op 2 computes what op 1 computes; only `mu` means something else there (the hoisted means of the variables, which exist
    whether or not the factor is active), so it is compared on active factors."""
    nonf = group == vc.GID["nonfinite"]
    for k in FLOAT_FIELDS + INT_FIELDS:
        if op == 0 and k not in vc.OP0_FIELDS:
            assert not vc.field(dev, k, True).view(np.uint32).any(), (what, op, k)      # op 0 leaves zeros elsewhere
            continue
        d, e = vc.field(dev, k, True), vc.field(exp, k, True)
        rows = ~nonf
        if op == 2 and k == "mu":
            rows = rows & (vc.field(X, "active")[:, 0] == 1)
        bad = np.nonzero(rows & ~(d == e).all(axis=1))[0]
        assert bad.size == 0, (what, op, k, bad[:5], [vc.GROUPS[i] for i in group[bad[:5]]], d[bad[:2]], e[bad[:2]])
        # the non-finite group: non-finite where the expectation is, integers equal
        if k in vc.INT_FIELDS:
            assert np.array_equal(d[nonf], e[nonf]), (what, op, k)
        else:
            want = ~np.isfinite(e[nonf]).all(axis=1)
            if op == 2 and k == "mu":
                want &= vc.field(X, "active")[nonf, 0] == 1
            got = ~np.isfinite(d[nonf]).all(axis=1)
            assert not (want & ~got).any(), (what, op, k, np.nonzero(want & ~got)[0])


@pytest.fixture(scope="module")
def restated(oracle_mod):
    X, g = vc.all_cases()
    api = oracle_mod.vertex_api("restatement")
    oracle_mod.set_trig_mode(1)
    try:
        exp = {op: vc.run_cpu(api, X, op) for op in (0, 1)}
    finally:
        oracle_mod.set_trig_mode(0)
    return X, g, exp


@pytest.mark.parametrize("op", [0, 1, 2])
def test_device_vertices_equal_the_restatement_on_every_case(restated, op):
    X, g, exp = restated
    assert len(X) >= 18000 and len(X) % 64 != 0 and set(g) == set(range(len(vc.GROUPS)))
    dev = _dev(op, X)
    _check_bits(dev, exp[min(op, 1)], X, g, op, "restatement")
    # ragged launches (n = 1, below / above one wavefront, a prime) give the same rows
    for n in (1, 63, 65, 257):
        lo = len(X) - n - 7
        assert _dev(op, X[lo:lo + n]).tobytes() == dev[lo:lo + n].tobytes(), n


@pytest.mark.parametrize("op", [0, 1, 2])
def test_device_vertices_equal_the_golden_dev_outputs(op):
    x, g = G["x"], G["group"]
    _check_bits(_dev(op, x), G["dev_op%d" % min(op, 1)], x, g, op, "golden dev_")


def check_against_reference_outputs(dev, ref, x, group, has_ref, op):
    """flags and counters equal; floats within 1e-4 (no relinearisation) / 1e-3 (relinearisation: trig enters), per group and
    tensor as max |diff| / max |ref| over the sample.  Returns the figures."""
    figures = []
    relin = np.ones(len(x), bool) if op == 0 else vc.relinearised(x, ref)
    for gi, name in enumerate(vc.GROUPS):
        m = (group == gi) & has_ref
        if not m.any():
            continue
        for k in INT_FIELDS:
            assert np.array_equal(vc.field(dev, k, True)[m], vc.field(ref, k, True)[m]), (name, op, k)
        if name == "nonfinite":
            for k in FLOAT_FIELDS:
                if op == 0 and k not in vc.OP0_FIELDS:
                    continue
                want = ~np.isfinite(vc.field(ref, k, True)[m]).all(axis=1)
                if op == 2 and k == "mu":
                    want &= vc.field(x, "active")[m, 0] == 1
                assert not (want & np.isfinite(vc.field(dev, k, True)[m]).all(axis=1)).any(), (name, op, k)
            continue
        for k in FLOAT_FIELDS:
            if op == 0 and k not in vc.OP0_FIELDS:
                continue
            for tol, rows in ((1e-3, m & relin), (1e-4, m & ~relin)):
                if op == 2 and k == "mu":
                    rows = rows & (vc.field(x, "active")[:, 0] == 1)
                if rows.any():
                    err = rel_err(vc.field(dev, k, True)[rows], vc.field(ref, k, True)[rows])
                    figures.append((name, op, k, tol, err))
                    print("%-13s op %d %-8s tol %.0e  err %.3e" % (name, op, k, tol, err))
                    assert err <= tol, (name, op, k, tol, err)
    return figures


@pytest.mark.parametrize("op", [0, 1, 2])
def test_device_vertices_against_the_reference_vertices_outputs(op):
    x, g, has_ref = G["x"], G["group"], G["has_ref"]
    assert has_ref.sum() >= 100
    check_against_reference_outputs(_dev(op, x), G["ref_op%d" % min(op, 1)], x, g, has_ref, op)
