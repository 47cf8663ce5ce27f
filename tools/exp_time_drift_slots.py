"""What a time-dependent drift costs per leapfrog slot: the seasonal SEIR of magi_v2_amd.drift_examples (traced, uses t) next to the
compiled-in seir3 (the same system without the forcing) on the same data, grid and matrices in one run: N grid points over [0, 4], dense,
one chain and eight chains.  Per case: device time per issued slot of a timed sampler run (magi_sampler_run / magi_sampler_run_stats) and
the mean in-sampler durations of the streaming and the point kernel (magi_sampler_profile).  Recorded, not gated.
    python tools/exp_time_drift_slots.py [--grid 1024] [--burnin 100] [--steps 50] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(drift_obj, name, I, X_obs, chains, a):
    from magi_v2_amd import host
    from magi_v2_amd.engine import MagiEngine
    eng = MagiEngine(0, drift=None if isinstance(drift_obj, str) else drift_obj)
    try:
        Xi = host.linear_interpolate(X_obs)
        hp = host.hparams_initial(Xi)
        D = X_obs.shape[1]
        eng.build_matrices(I, hp["phi1s"], np.full(D, 0.5), 2.01, bandsize=None, want_host=False)
        N_ds, beta, idx, y = host.observation_bookkeeping(X_obs, X_obs)
        Xhat = host.cubic_smoother(I, Xi)
        LB = host.sigma_sqs_lower_bound(Xhat)
        eng.set_times(I)
        eng.set_problem(Xi.mean(axis=0), N_ds.astype(np.float64), idx, y, beta, LB, drift_obj)
        P = eng.P
        th0 = np.array([6.0, 0.6, 1.8, 0.4])[:P]
        sp0, tp0 = host.softplus_inverse_inits(hp["sigma_sqs"], th0, LB)
        rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
        cfg = eng.default_cfg(num_results=a.steps, num_burnin_steps=a.burnin, max_tree_depth=a.depth)
        eng.sampler_init(cfg, rep(Xhat), rep(sp0), rep(tp0), seed=a.seed, chain_ids=list(range(chains)))
        eng.sampler_run(a.burnin)
        lf, ms = eng.sampler_run(a.steps)
        slots, graphs = eng.sampler_run_stats()
        kernel = eng.stream_kernel_name(chains)
        eng.sampler_init(cfg, rep(Xhat), rep(sp0), rep(tp0), seed=a.seed, chain_ids=list(range(chains)))
        eng.sampler_run(a.burnin)
        stream_us, point_us, plf = eng.sampler_profile(a.profile_slots)
    finally:
        eng.close()
    return dict(drift=name, chains=chains, stream_kernel=kernel, leapfrogs=int(lf), slots=int(slots), device_ms=round(ms, 3),
                us_per_slot=round(ms * 1e3 / max(slots, 1), 3), leapfrogs_per_s=round(lf / (ms * 1e-3), 1),
                stream_us=round(stream_us, 3), point_us=round(point_us, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--profile-slots", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from magi_v2_amd import drift
    from magi_v2_amd.drift_examples import TIME_EXAMPLES, rk4, seir_seasonal
    I, X = rk4(seir_seasonal, [0.02, 0.01, 0.0], np.array([6.0, 0.6, 1.8, 0.4]), 4.0, a.grid, substeps=4)
    X_obs = X + np.random.default_rng(0).normal(0.0, 1.0, X.shape) * (0.05 * X.std(axis=0))
    X_obs[1::2] = np.nan
    seasonal = drift.resolve(*TIME_EXAMPLES["seir_seasonal"])
    rows = []
    for chains in (1, 8):
        for d, name in ((seasonal, "seir_seasonal"), ("seir3", "seir3")):
            r = case(d, name, I, X_obs, chains, a)
            rows.append(r)
            print(json.dumps(r), flush=True)
    summ = {}
    for chains in (1, 8):
        t, b = (next(r for r in rows if r["chains"] == chains and r["drift"] == n) for n in ("seir_seasonal", "seir3"))
        summ[f"{chains}_chains"] = {k + "_ratio": round(t[k] / b[k], 4) for k in ("us_per_slot", "stream_us", "point_us")}
    print(json.dumps(summ), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"grid": a.grid, "T": 4.0, "burnin": a.burnin, "steps": a.steps, "max_tree_depth": a.depth, "rows": rows, "time_dependent_over_seir3": summ}, fh, indent=1)


if __name__ == "__main__":
    main()
