"""A seeded slice of the randomised parity soak (profiles/fuzz_parity.py) in the suite: tests/fuzz_support.py's plans for SUITE_SEEDS —
random graphs x random parameters x random call patterns, the path the library chooses against the literal loop on the two-kernel path
and that against the oracle, bit for bit; ./slam's flow on every fourth seed, a sharded group on every eighth.  What the list covers is
pinned without a GPU by tests/test_fuzz_plan_cpu.py; the times of the cases are in profiles/fuzz_slice.md."""
import time

import pytest

from tests import fuzz_support as fz

GROUP = 4      # seeds per case: a case stays at a few seconds (profiles/fuzz_slice.md)
GROUPS = [fz.SUITE_SEEDS[i:i + GROUP] for i in range(0, len(fz.SUITE_SEEDS), GROUP)]


@pytest.fixture(scope="module")
def soak():
    from oracle import oracle as orc
    fz.prepare()
    yield
    orc.set_trig_mode(0)


@pytest.mark.gpu
@pytest.mark.parametrize("seeds", GROUPS, ids=["%d-%d" % (g[0], g[-1]) for g in GROUPS])
def test_seeded_slice_of_the_parity_soak(seeds, soak):
    """Per seed: the path B took is the one its plan predicted (a probe that left the persistent path fails here, it does not test
    less), and everything the runners compare holds — no tolerance anywhere."""
    for seed in seeds:
        p = fz.suite_plan(seed)
        t0 = time.perf_counter()
        try:
            desc, _ = fz.run(p)
        except fz.Mismatch as e:
            raise AssertionError("seed %d: %s\n  plan: %s\n  rerun: python profiles/fuzz_parity.py --suite-seed %d" % (seed, e, fz.describe(p), seed)) from None
        print("seed %d ok in %.2f s: %s" % (seed, time.perf_counter() - t0, desc))
