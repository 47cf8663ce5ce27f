"""A/B of config 4 on one GPU: the ten alpha-sweep datasets x 8 chains (N = 161, b = 80) sampled by SweepRunner as ONE problem group
(grouped=True: one graph, one kernel pair per leapfrog slot for all 80 chains) and per handle (grouped=False: ten handles, ten host
threads), alternating, three times each: 200 burn-in transitions, then 100 timed ones.  Prints samples/s, leapfrogs/s, us per slot and
slots per transition (sampler_run_stats of the timed run: the group's own, or per handle the mean over the ten) and asserts that both
paths give the same last sample for every unit.
    python tools/exp_group_ab.py [--reps 3] [--burnin 200] [--steps 100] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(datasets, grouped, a):
    from magi_v2_amd.sweep import SweepRunner
    run = SweepRunner(0, datasets, 8, 0, 1, bandsize=80, grouped=grouped)
    try:
        run.init(a.seed, num_results=a.steps, num_burnin_steps=a.burnin)
        run.run(a.burnin)
        t0 = time.perf_counter()
        lf = run.run(a.steps)
        dt = time.perf_counter() - t0
        stats = [run.group.sampler_run_stats()] if run.group is not None else [e.sampler_run_stats() for e in run.engines]
        slots = float(np.mean([s for s, _ in stats]))
        flat, ids = run.samples()
    finally:
        run.close()
    units = len(ids)
    return dict(grouped=grouped, samples_per_s=units * a.steps / dt, leapfrogs_per_s=lf / dt, seconds=dt, slots=slots,
                us_per_slot=dt / slots * 1e6 if grouped else None, slots_per_transition=slots / a.steps), flat[:, -1], ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--burnin", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from magi_v2_amd.sweep import alpha_sweep_datasets
    datasets = alpha_sweep_datasets(os.path.join(ROOT, "tests", "golden", "seir_alpha_sweep.npz"))
    rows, last = [], {}
    for r in range(a.reps):
        for grouped in (True, False):
            res, lastrow, ids = one(datasets, grouped, a)
            res["rep"] = r
            rows.append(res)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
            if grouped in last:
                assert np.array_equal(last[grouped][0], lastrow), "a path changed its own samples between repetitions"
            last[grouped] = (lastrow, ids)
    assert last[True][1] == last[False][1]
    assert np.array_equal(last[True][0], last[False][0]), "grouped and per-handle paths differ"
    summ = {}
    for grouped in (True, False):
        sel = [x for x in rows if x["grouped"] == grouped]
        summ["grouped" if grouped else "per_handle"] = {k: round(float(np.median([x[k] for x in sel])), 3)
                                                        for k in ("samples_per_s", "leapfrogs_per_s", "slots_per_transition")}
        if grouped:
            summ["grouped"]["us_per_slot"] = round(float(np.median([x["us_per_slot"] for x in sel])), 3)
    summ["speedup"] = round(summ["grouped"]["samples_per_s"] / summ["per_handle"]["samples_per_s"], 3)
    summ["units_identical"] = True
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"runs": rows, "summary": summ, "burnin": a.burnin, "steps": a.steps, "reps": a.reps}, fh, indent=1)


if __name__ == "__main__":
    main()
