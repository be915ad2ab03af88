"""How fast a ctx reaches the wraps of the persistent kernel's counters (profiles/long_lived.md): launches per second of the
shortest bursts a keyframe loop makes, on the graphs of tests/test_gpu_long_lived.py.

    python profiles/long_lived.py            one JSON line per graph

Per graph: launches / s of gbp_iterate(2) queued back to back (the host does not wait: what a loop that never reads reaches), of
gbp_iterate_eval_each(1) (blocking: one metric per launch, a loop that prints every iteration), the time of one burst of 4 096 passes,
and from them the wall time of one tag period (2^19 - 1 launches) and of 2^32 arrivals at one barrier of every workgroup per launch."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import test_gpu_long_lived as ll  # noqa: E402
from tests.test_exact_inference import _engine  # noqa: E402


def main():
    for name in ll.GRAPHS:
        bal, state, K, kw = ll._case(name, "placement")
        eng = _engine(bal, K, **kw)
        eng.upload(state)
        eng.linearise()
        eng.iterate(2)
        eng.sync()
        assert eng.graph_state() == 2
        n = 4000
        t = time.perf_counter()
        for _ in range(n):
            eng.iterate(2)
        eng.sync()
        plain = n / (time.perf_counter() - t)
        n = 2000
        t = time.perf_counter()
        for _ in range(n):
            eng.iterate_eval_each(1)
        each = n / (time.perf_counter() - t)
        eng.upload(state)
        eng.linearise()
        eng.sync()
        t = time.perf_counter()
        eng.iterate(4096)
        eng.sync()
        long_ms = 1e3 * (time.perf_counter() - t)
        nb = ll._grid(bal, True)[0]
        print(json.dumps({"graph": name, "factors": int(bal["n_edges"]), "workgroups_plain": ll._grid(bal, False)[0], "workgroups_metric_each": nb,
                          "iterate2_launches_per_s": round(plain), "eval_each1_launches_per_s": round(each), "burst_4096_ms": round(long_ms, 2),
                          "tag_period_s_at_iterate2": round((2 ** 19 - 1) / plain, 1), "tag_period_s_at_eval_each1": round((2 ** 19 - 1) / each, 1),
                          "arrival_wrap_h_at_eval_each1": round(2 ** 32 / (nb * each) / 3600.0, 1)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
