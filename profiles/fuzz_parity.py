#!/usr/bin/env python3
"""Randomised parity soak on the GPU: random graphs x random parameters x random call patterns, three runs of each in lock step.

    python profiles/fuzz_parity.py [seconds=600] [first_seed=0] [max_edges=300000]
    python profiles/fuzz_parity.py --suite-seed N      (one seed of the slice tests/test_gpu_fuzz.py runs, as the suite plans it)

The generator, the three seed runners and the comparisons live in tests/fuzz_support.py (plan(kind, seed) draws, run(plan) executes):
one copy for this script and for the suite.  What a seed draws, as that module's docstring has it in full:

Per seed (everything below drawn from the seed; B's call patterns — forms of the state calls and of the metric, steps and base
loop index, gbp_sync or not, LINEARISE in mid-run, long bursts, gbp_iterate_eval_each — are listed in tests/fuzz_support.py):
  * a graph the shipped files never show — 2..120 cameras, 3..30 000 landmarks (log-uniform), up to 12 factors per landmark, the edge
    list UNSORTED (slot order = file order, ba.cpp:267-279), duplicate (camera, landmark) factors, hub landmarks, landmarks without a
    factor, ~10 % inactive factors; parameters that relinearise early and often; per_factor_mu 0 / 1; tile_order 0..3; the all-pad
    segment skipping of the sweep forced on / off / left to the library;
  * A: the two-kernel path, one gbp_iterate(1) at a time (gbp_weaken_priors where ba.cpp:1001-1008 weakens) — against the ORACLE
    (oracle/, device summation order) after every one of the first 10 iterations and after the last: every belief, both message sets,
    damping state, and at the end the factor potentials, bit for bit;
  * B: the path the library chooses by itself for that size (k_persist_flow in one launch per burst, or the hipGraph replay), driven in
    bursts of random length by one of {gbp_iterate(k) + gbp_weaken_priors, gbp_ba_loop with the metric, gbp_ba_loop without}; the
    persistent kernel with tagged records or barriers, with or without its redundant-record check — against A after every burst:
    every tensor incl. the hoisted means, bit for bit; the metrics gbp_ba_loop returns against A's gbp_eval() after each iteration.
Every fourth seed runs ./slam's flow instead (slam_seed below), every eighth a landmark-sharded group of contexts (shard_seed).
The first mismatch stops the run with the seed and what differed; the summary line goes to stdout (copied to profiles/ by hand).
test infrastructure: the oracle is the checker here, never the product.
"""
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")      # the oracle's OpenMP team: a box of 256 cores spins on small graphs otherwise
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.fuzz_support import (GatherAll, Mismatch, against_oracle, describe, ev_equal, one_seed, prepare, random_problem, run, same,  # noqa: E402,F401
                                shard_seed, slam_seed, snapshot, soak_plan, suite_plan)


def suite_seed(seed):
    prepare()
    p = suite_plan(seed)
    print(describe(p), flush=True)
    t0 = time.time()
    try:
        desc, _ = run(p)
    except Mismatch as e:
        print("seed %d: MISMATCH — %s" % (seed, e), flush=True)
        return 1
    print("seed %d ok in %.2f s: %s" % (seed, time.time() - t0, desc), flush=True)
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--suite-seed":
        return suite_seed(int(sys.argv[2]))
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    max_edges = int(sys.argv[3]) if len(sys.argv) > 3 else 300000
    prepare()
    t0 = time.time()
    seed, done, relin_runs, paths = first, 0, 0, {}
    while time.time() - t0 < budget:
        try:
            desc, nr = run(soak_plan(seed, max_edges))
        except Mismatch as e:
            print("seed %d: MISMATCH — %s" % (seed, e), flush=True)
            return 1
        print("seed %d ok: %s" % (seed, desc), flush=True)
        relin_runs += nr > 0
        key = (desc.split("| B: ")[1].split(" |")[0] if "| B: " in desc else "sharded, world " + desc.split()[2] if desc.startswith("SHARDED")
               else "SLAM flow on " + desc.split("| path ")[1].split(" |")[0])
        paths[key] = paths.get(key, 0) + 1
        done += 1
        seed += 1
    print("SUMMARY: %d seeds (%d..%d) in %.0f s, no mismatch; %d of them relinearised; B's path and driver: %s"
          % (done, first, seed - 1, time.time() - t0, relin_runs, ", ".join("%s x %d" % kv for kv in sorted(paths.items()))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
