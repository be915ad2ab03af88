"""The metric in device memory against the host forms (profiles/device_metric.md): host time from call to return and to the end of
gbp_sync, and the device time gbp_timing reports per iteration, for gbp_eval on S1 and gbp_ba_loop(100, 0, 5) on S1 and fr1xyz.
    python profiles/device_metric.py [--host-only] [--reps N]     one process, one GPU (--host-only: a library without the device forms, through GBP_LIB)
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python profiles/device_metric.py --trace
                                                                  one default ba_loop(100, 0, 5, device=True) on fr1xyz and 20 device evals on S1:
                                                                  launch counts, duration of k_eval_fold_part per record"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gbp_poplar_amd import driver, hostlib                       # noqa: E402
from gbp_poplar_amd.engine import GbpEngine                      # noqa: E402


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def timed(eng, prepare, call, reps, iters):
    """per repetition: prepare (not timed), sync, [call -> return -> sync]; ms — and the device time per iteration of gbp_timing, us"""
    ret, tot, dev = [], [], []
    for _ in range(reps + 1):      # (the first repetition is the warm-up)
        prepare()
        eng.sync()
        eng.timing(reset=True)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        eng.sync()
        t2 = time.perf_counter()
        ret.append((t1 - t0) * 1e3)
        tot.append((t2 - t0) * 1e3)
        if iters:
            t = eng.timing()
            assert t["iterations"] == iters, t
            dev.append(t["total_ms"] * 1e3 / iters)
    out = {"return_ms": stats(ret[1:]), "return_and_sync_ms": stats(tot[1:])}
    if iters:
        out["device_us_per_iteration"] = stats(dev[1:])
    return out


def graph(name):
    bal = hostlib.synth_generate(1000, 100000, 10, 20200303) if name == "S1" else hostlib.bal_read(os.path.join(ROOT, "data", "sequences", name + ".txt"))
    K, state, _ = driver.build_inputs(bal, driver.Options(), hostlib)
    eng = GbpEngine(bal["cam_id"], bal["lmk_id"], bal["n_cams"], bal["n_lmks"], K)
    return eng, state


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    host_only = "--host-only" in sys.argv
    trace = "--trace" in sys.argv
    import torch
    for name in ("fr1xyz", "S1"):
        eng, state = graph(name)

        def fresh():
            eng.upload(state)
            eng.linearise()

        fresh()
        eng.iterate(5)
        if trace:
            if name == "fr1xyz":
                fresh()
                eng.ba_loop(100, 0, 5, device=True)
            else:
                for _ in range(20):
                    eng.eval(device=True)
            eng.sync()
            eng.close()
            continue
        out = {"graph": name, "graph_state": eng.graph_state(), "reps": reps}
        if name == "S1":
            out["eval_host"] = timed(eng, lambda: None, eng.eval, reps, 0)
        out["ba_loop_host"] = timed(eng, fresh, lambda: eng.ba_loop(100, 0, 5), reps, 100)
        if not host_only:
            raw1 = torch.empty(7, dtype=torch.int64, device="cuda")
            raw = torch.empty((100, 7), dtype=torch.int64, device="cuda")
            if name == "S1":
                out["eval_device"] = timed(eng, lambda: None, lambda: eng.eval(out=raw1), reps, 0)
            out["ba_loop_device"] = timed(eng, fresh, lambda: eng.ba_loop(100, 0, 5, out=raw), reps, 100)
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
