"""Time the posterior-summary step of predict(summary=True, keep_samples=False) -- MagiEngine.sampler_summary, everything on the device --
against the route every caller had to take before: sampler_samples() (all draws to the host) + numpy mean / sd / quantile.

    python tools/exp_summary.py [--out profiles/r08_exp_summary.json] [--results 1000] [--grid 1024]

Shapes: BASELINE config 2 (1 chain, N = 1024 x 4 dense) and config 3's per-GPU share (8 chains), ``--results`` draws per chain.  The chains are
sampled with a shallow tree and stale_cache=0 (with the reference-faithful stale cache a short run at this size may never move: every column
is then constant and the lag loop has nothing to do); the record says how many columns moved and their median R-hat / ESS.  Each route is a host clock around a
call that ends in a device synchronise (both block until their results are on the host), one untimed warm-up, then the median of ``--reps``."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magi_v2_amd import host                      # noqa: E402
from magi_v2_amd.engine import MagiEngine         # noqa: E402
from magi_v2_amd.sweep import problem_setup       # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def med(a):
    a = np.asarray(a)[np.isfinite(a)]
    return float(np.median(a)) if a.size else None


def host_route(eng, LB, timing):
    t0 = time.perf_counter()
    X, sp, tp = eng.sampler_samples()
    t1 = time.perf_counter()
    sig, th = host.transform_samples(sp, tp, LB)
    res = {}
    for name, a in (("X", X), ("sigma_sqs", sig), ("thetas", th)):
        pooled = a.reshape((-1,) + a.shape[2:])
        res[name] = (pooled.mean(axis=0), pooled.std(axis=0, ddof=1), np.quantile(pooled, PROBS, axis=0))
    timing.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_exp_summary.json"))
    ap.add_argument("--results", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burnin", type=int, default=100)
    a = ap.parse_args()
    I, X_obs, _, _ = host.synthetic_seir(a.grid)
    pb = problem_setup(I, X_obs, 3)
    eng = MagiEngine(0)
    eng.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, want_host=False)
    eng.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    rows = []
    for name, C in (("config2", 1), ("config3_share", 8)):
        rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
        cfg = eng.default_cfg(num_results=a.results, num_burnin_steps=a.burnin, max_tree_depth=5, stale_cache=0)
        eng.sampler_init(cfg, rep(pb["Xhat"]), rep(pb["sig_pre0"]), rep(pb["th_pre0"]), seed=7)
        eng.sampler_run(a.results + a.burnin)
        dev_ms, dev_all = median_ms(lambda: eng.sampler_summary(probs=PROBS), a.reps)
        timing = []
        host_ms, host_all = median_ms(lambda: host_route(eng, pb["LB"], timing), a.reps)
        got, ref = eng.sampler_summary(probs=PROBS), host_route(eng, pb["LB"], timing)
        err = max(float(np.abs(got[b]["mean"] - ref[b][0]).max() / np.abs(ref[b][0]).max()) for b in ("X", "sigma_sqs", "thetas"))
        qerr = max(float(np.abs(got[b]["quantiles"] - ref[b][2]).max() / np.abs(ref[b][2]).max()) for b in ("X", "sigma_sqs", "thetas"))
        row = {"shape": name, "chains": C, "results": a.results, "N": eng.N, "D": eng.D, "sample_bytes": int(C * a.results * (eng.N * eng.D + eng.D + eng.P) * 8),
               "device_summary_ms": round(dev_ms, 3), "device_summary_ms_all": dev_all, "host_route_ms": round(host_ms, 3), "host_route_ms_all": host_all,
               "host_download_ms": round(float(np.median([t[0] for t in timing[1:]])), 3),
               "host_numpy_ms": round(float(np.median([t[1] for t in timing[1:]])), 3),
               "speedup": round(host_ms / dev_ms, 2), "mean_rel_diff": err, "quantile_rel_diff": qerr,
               "constant_X_columns": int((got["X"]["sd"] == 0).sum()), "median_rhat_X": med(got["X"]["rhat"]), "median_ess_X": med(got["X"]["ess"]),
               "ess_thetas": [round(float(v), 1) for v in got["thetas"]["ess"]], "rhat_thetas": [round(float(v), 4) for v in got["thetas"]["rhat"]]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_summary.py", "what": "summary step of predict(summary=True, keep_samples=False) (device: mean, sd, 3 quantiles, "
                   "rhat, ess, mcse_mean of every column) vs sampler_samples() + numpy mean / sd / quantile (no diagnostics); host clock around "
                   "calls that end in a device synchronise, median of reps after one warm-up", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
