"""Time the posterior predictive check of predict(ppc=True, keep_samples=False) -- MagiEngine.sampler_ppc: replicated observations, their
mean / sd / quantiles, PIT values and discrepancy p-values, everything on the device -- against the route a caller had to take without
it: sampler_samples() (all draws to the host) + the definitions of include/magi_hip.h as vectorised float64 numpy expressions over
[S, n_obs] (Philox noise from the oracle's generator, so the two routes draw the same replicates).

    python tools/exp_ppc.py [--out profiles/r18_exp_ppc.json] [--results 1000] [--grid 1024]

Shapes: BASELINE config 2 (1 chain, N = 1024 x 4 dense) and config 3's per-GPU share (8 chains), ``--results`` draws per chain, sampled as
tools/exp_elpd.py samples them.  Each route is a host clock around a call that ends in a device synchronise (both block until their
results are on the host), one untimed warm-up, then the median of ``--reps``; the host route's download and numpy parts are reported
separately.  There is no pass bar: the file records what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.special import erfc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magi_v2_amd import host                      # noqa: E402
from magi_v2_amd.engine import MagiEngine         # noqa: E402
from magi_v2_amd.sweep import problem_setup       # noqa: E402
from oracle.magi_oracle import _u01, philox4x32   # noqa: E402

STREAM_PPC = 5
PROBS = (0.025, 0.5, 0.975)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def host_route(eng, pb, seed, timing):
    """Identity links, no weights (the benchmark problem): y_rep = x + sigma z0, u_obs = (y - x) / sigma."""
    t0 = time.perf_counter()
    X, sp, _ = eng.sampler_samples()
    t1 = time.perf_counter()
    N, D = eng.N, eng.D
    C, R = X.shape[:2]
    S = C * R
    idx = np.asarray(pb["idx"])
    order = np.argsort((idx % D) * N + idx // D, kind="stable")          # the device's order: ascending d N + i
    idx = idx[order]
    y = np.asarray(pb["y"])[order]
    comp = idx % D
    K = idx.shape[0]
    sd = np.sqrt(np.log1p(np.exp(sp)) + np.asarray(pb["LB"])).reshape(S, D)[:, comp]
    x = X.reshape(S, N * D)[:, idx]
    r0, r1, r2, r3 = philox4x32(np.arange(K, dtype=np.uint64)[None, :], (np.arange(S) % R).astype(np.uint64)[:, None],
                                (np.arange(S) // R).astype(np.uint64)[:, None], STREAM_PPC, seed)
    z0 = np.sqrt(-2.0 * np.log(_u01(r0, r1))) * np.cos(2.0 * np.pi * _u01(r2, r3))
    y_rep = x + sd * z0
    u = (y - x) / sd
    out = {"mean": y_rep.mean(axis=0), "sd": y_rep.std(axis=0, ddof=1), "quantiles": np.quantile(y_rep, PROBS, axis=0),
           "pit": (0.5 * erfc(-u / np.sqrt(2.0))).mean(axis=0)}
    pval = np.full((D, 4), np.nan)
    for d in range(D):
        c = comp == d
        if not c.any():
            continue
        T = []
        for v in (u[:, c], z0[:, c]):
            ss = (v * v).sum(axis=1)
            T.append(np.stack([ss, v.mean(axis=1), np.abs(v).max(axis=1), (v[:, :-1] * v[:, 1:]).sum(axis=1) / ss], axis=1))
        pval[d] = (T[1] >= T[0]).mean(axis=0)
    out["pval"] = pval
    timing.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_exp_ppc.json"))
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
    seed = 11
    for name, C in (("config2", 1), ("config3_share", 8)):
        rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
        cfg = eng.default_cfg(num_results=a.results, num_burnin_steps=a.burnin, max_tree_depth=5, stale_cache=0)
        eng.sampler_init(cfg, rep(pb["Xhat"]), rep(pb["sig_pre0"]), rep(pb["th_pre0"]), seed=7)
        eng.sampler_run(a.results + a.burnin)
        dev_ms, dev_all = median_ms(lambda: eng.sampler_ppc(seed=seed, probs=PROBS), a.reps)
        draws_ms, draws_all = median_ms(lambda: eng.sampler_ppc(seed=seed, probs=PROBS, return_draws=True), a.reps)
        timing = []
        host_ms, host_all = median_ms(lambda: host_route(eng, pb, seed, timing), a.reps)
        got, ref = eng.sampler_ppc(seed=seed, probs=PROBS), host_route(eng, pb, seed, timing)
        diff = {s: float(np.nanmax(np.abs(got[s] - ref[s]) / np.maximum(1.0, np.abs(ref[s])))) for s in ("mean", "sd", "quantiles", "pit")}
        pv = np.stack([got["pvalues"][s] for s in host.PPC_STATS], axis=1)
        diff["pval"] = float(np.nanmax(np.abs(pv - ref["pval"])))
        down = float(np.median([t[0] for t in timing[1:]]))
        row = {"shape": name, "chains": C, "results": a.results, "N": eng.N, "D": eng.D, "n_obs": got["n_obs"],
               "sample_bytes": int(C * a.results * (eng.N * eng.D + eng.D + eng.P) * 8),
               "device_ppc_ms": round(dev_ms, 3), "device_ppc_ms_all": dev_all, "device_ppc_with_y_rep_ms": round(draws_ms, 3),
               "device_ppc_with_y_rep_ms_all": draws_all, "host_route_ms": round(host_ms, 3), "host_route_ms_all": host_all,
               "host_download_ms": round(down, 3), "host_numpy_ms": round(float(np.median([t[1] for t in timing[1:]])), 3),
               "speedup": round(host_ms / dev_ms, 2), "device_faster_than_download_alone": bool(dev_ms < down), "max_diff": diff,
               "pvalues": {s: np.round(v, 4).tolist() for s, v in got["pvalues"].items()}, "pit_ks": np.round(got["pit_ks"], 4).tolist(),
               "n_T_excluded": got["n_T_excluded"].tolist(), "n_nonfinite": got["n_nonfinite"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_ppc.py", "what": "posterior predictive check of predict(ppc=True, keep_samples=False) (device: replicates, mean / sd / "
                   "quantiles, PIT and discrepancy p-values of every observation) vs sampler_samples() + the vectorised float64 numpy route; host clock "
                   "around calls that end in a device synchronise, median of reps after one warm-up.  The host route leaves out two things the device computes -- the count of draws excluded for a non-finite "
                   "discrepancy (n_T_excluded) and of columns with a non-finite replicate (n_nonfinite) -- which favours the host route slightly", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
