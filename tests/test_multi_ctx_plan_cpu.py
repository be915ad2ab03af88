"""The schedules of tests/test_gpu_multi_ctx.py without a GPU (tests/multi_ctx_support.py): a plan is a pure function of its arguments,
every verb occurs over the committed seeds, and the workgroup counts the tests' precondition adds up are the ones
gbp_debug_persist_roles gives for the graph's own layout (host code of the test-hooks library)."""
import ctypes as C

import numpy as np

from tests import multi_ctx_support as mc

MI355X_CUS = 256


def test_plans_are_a_pure_function_of_their_arguments():
    for seed in mc.PLAN_SEEDS:
        a, b = mc.plan(seed, 4), mc.plan(seed, 4)
        assert a == b and mc.describe(a) == mc.describe(b)
    assert mc.plan(1, 4) != mc.plan(2, 4)
    fixed = dict(graphs=["half0", "half1", "fr2robot2"], persistent=[0, 0, 0], coop=[0, 0, 0], streams=["own"] * 3, others=0.0, verbs=mc.BURSTS)
    a, b = mc.plan(7, 3, **fixed), mc.plan(7, 3, **fixed)
    assert a == b
    assert [i for i, _, _ in a["calls"]] == [0, 1, 2] * 6, "round robin A, B, C, A, ..."
    for name in ("half0", "fr2robot2"):      # the graphs are rebuilt from their names to the same bits
        mc.graph.cache_clear()
        g1 = mc.graph(name)
        mc.graph.cache_clear()
        g2 = mc.graph(name)
        assert all(np.array_equal(g1[0][k], g2[0][k]) for k in g1[0]) and all(np.array_equal(g1[2][k], g2[2][k]) for k in g1[2])


def test_every_verb_and_every_kind_of_context_occurs_over_the_committed_seeds():
    plans = [mc.plan(s, 4) for s in mc.PLAN_SEEDS]
    calls = [c for p in plans for c in p["calls"]]
    seen = {v for _, v, _ in calls}
    print("verbs over seeds %r: %s" % (mc.PLAN_SEEDS, {v: sum(w == v for _, w, _ in calls) for v in mc.VERBS}))
    assert seen == set(mc.VERBS), set(mc.VERBS) - seen
    assert {a for _, v, a in calls if v == "set_stream"} == {"new", "own"}
    assert {a for _, v, a in calls if v == "read"} == {"host", "device"}
    assert {a[3] for _, v, a in calls if v == "ba_loop_metric"} == {a[1] for _, v, a in calls if v == "iterate_eval_each"} == {"host", "device"}
    ctxs = [c for p in plans for c in p["contexts"]]
    assert {c["persistent"] for c in ctxs} == {-1, 0, 1} and {c["persist_coop"] for c in ctxs} == {0, 1} and {c["stream"] for c in ctxs} == {"own", "caller"}
    assert any(c["graph"] in mc.HALVES for c in ctxs) and any(c["graph"] in mc.SEQUENCES for c in ctxs)
    for p in plans:
        per_ctx = [sum(a if v == "iterate" else a[0] for j, v, a in p["calls"] if j == i and v in mc.BURSTS) for i in range(4)]
        assert all(10 <= (a if v == "iterate" else a[0]) <= 50 for _, v, a in p["calls"] if v in mc.BURSTS) and max(per_ctx) <= 300, per_ctx
    # gbp_ba_loop continues the loop where the context stands (its base index: the passes since the last upload)
    for p in plans:
        done = [0] * 4
        for i, v, a in p["calls"]:
            if v == "close":
                done[i] = 0
            if v in ("ba_loop", "ba_loop_metric"):
                assert a[1] == done[i] and a[2] == mc.BA_STEPS
            if v in mc.BURSTS:
                done[i] += a if v == "iterate" else a[0]


def test_workgroup_counts_are_the_launchers():
    from gbp_poplar_amd import _lib, hostlib
    lib = _lib.load(hooks=True)
    # the shipped sequences: small grids — each of them twice (the six contexts of the aliasing test) is more than an MI355X
    assert mc.grid("fr1xyz") == (63, 108, 208) and mc.grid("fr2robot2") == (20, 39, 60)      # (the counts tests/test_persist_roles.py pins)
    assert all(14 <= mc.grid(n)[0] <= 80 for n in mc.SEQUENCES) and 2 * sum(mc.grid(n)[0] for n in mc.SEQUENCES) > MI355X_CUS
    for name in mc.HALVES + mc.SEQUENCES + ("hub",):
        bal = mc.graph(name)[0]
        lay = hostlib.layout_build(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"])
        nb0, nb1, tiles = mc.grid(name)
        assert tiles == lay["n_tiles"] and lay["tile_perm"].size == 0 and lay["row_slot"].size == 0      # (else the graph never runs in the persistent kernel)
        for with_metric, nb in ((0, nb0), (1, nb1)):
            dims = (C.c_uint32 * 4)()
            assert lib.gbp_debug_persist_roles(tiles, bal["n_cams"], bal["n_lmks"], with_metric, dims, None, 0) == 0
            assert dims[0] == nb and 4 * nb >= tiles and nb <= MI355X_CUS      # one wave per tile; under the automatic limit of persist_setup
            if dims[1]:      # separated roles: every tile and every camera (with the metric: every metric mean too) has a wave of its own
                assert 4 * nb >= tiles + bal["n_cams"] * (2 if with_metric else 1), (name, with_metric, list(dims))
    for name in mc.HALVES:
        nb0, nb1, tiles = mc.grid(name)
        print("%s: %d tiles, %d / %d workgroups" % (name, tiles, nb0, nb1))
        assert 600 <= tiles <= 680 and 150 <= nb0 <= 170 and nb0 > MI355X_CUS // 2, (name, nb0, tiles)
    # what the GPU tests add up: two halves exceed an MI355X, the three sequences and one half do not
    p = mc.plan(0, 3, graphs=["half0", "half1", "fr2robot2"], persistent=[0, 0, 0], coop=[0, 0, 0], streams=["own"] * 3)
    total, over = mc.over_device(p, MI355X_CUS)
    assert total == mc.grid("half0")[0] + mc.grid("half1")[0] + 20 and over
    assert mc.over_device(p, MI355X_CUS, among=(0, 2)) == (mc.grid("half0")[0] + 20, False)
    q = mc.plan(0, 2, graphs=["half0", "half1"], persistent=[0, -1], coop=[0, 0], streams=["own"] * 2)
    assert mc.over_device(q, MI355X_CUS) == (mc.grid("half0")[0], False), "a two-kernel context launches no persistent grid"
