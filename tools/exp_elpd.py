"""Time the model-comparison step of predict(elpd=True, keep_samples=False) -- MagiEngine.sampler_elpd: pointwise log-likelihood, WAIC and
PSIS-LOO, everything on the device -- against the route every caller had to take before: sampler_samples() (all draws to the host) + the
vectorised float64 numpy route (log-likelihood and WAIC as array expressions, PSIS per observation on a sorted tail).

    python tools/exp_elpd.py [--out profiles/r13_exp_elpd.json] [--results 1000] [--grid 1024]

Shapes: BASELINE config 2 (1 chain, N = 1024 x 4 dense) and config 3's per-GPU share (8 chains), ``--results`` draws per chain, sampled as
tools/exp_summary.py samples them.  Each route is a host clock around a call that ends in a device synchronise (both block until their
results are on the host), one untimed warm-up, then the median of ``--reps``; the host route's download, log-likelihood + WAIC and PSIS
parts are reported separately."""
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


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def gpd_fit(x):
    """Zhang and Stephens' fit of the ascending exceedances x (include/magi_hip.h) -> (khat, sigma)."""
    n = len(x)
    m = 30 + int(np.sqrt(n))
    j = np.arange(1, m + 1)
    th = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x[(n + 2) // 4 - 1])
    k = np.mean(np.log1p(-th[:, None] * x[None, :]), axis=1)
    l = n * (np.log(-th / k) - k - 1.0)
    w = 1.0 / np.sum(np.exp(l[None, :] - l[:, None]), axis=1)
    t = np.sum(th * w)
    k = np.mean(np.log1p(-t * x))
    return (k * n + 5.0) / (n + 10.0), -k / t


def psis_columns(ll):
    """ll [S][K] -> (elpd_loo [K], khat [K]) as include/magi_hip.h defines them; one argpartition + sort of the tail per column."""
    S, K = ll.shape
    M = int(min(S // 5, np.ceil(3.0 * np.sqrt(S))))
    elpd, khat = np.empty(K), np.full(K, np.inf)
    p = (np.arange(1, M + 1) - 0.5) / M
    lp = np.log1p(-p)
    with np.errstate(all="ignore"):
        for c in range(K):
            l = ll[:, c]
            r = -l
            r = r - r.max()
            lw = r.copy()
            if M >= 5:
                o = np.argsort(r, kind="stable")
                tail, cut = o[S - M:], r[o[S - M - 1]]
                if r[tail[-1]] > r[tail[0]]:
                    ec = np.exp(cut)
                    kh, s = gpd_fit(np.exp(r[tail]) - ec)
                    khat[c] = kh
                    if np.isfinite(kh):
                        lw[tail] = np.log(ec + (s / kh * np.expm1(-kh * lp) if kh != 0 else -s * lp))
            lw = np.minimum(lw, 0.0)
            a = l + lw
            A, B = a.max(), lw.max()
            elpd[c] = A + np.log(np.exp(a - A).sum()) - B - np.log(np.exp(lw - B).sum())
    return elpd, khat


def host_route(eng, pb, timing):
    t0 = time.perf_counter()
    X, sp, _ = eng.sampler_samples()
    t1 = time.perf_counter()
    N, D = eng.N, eng.D
    idx = np.asarray(pb["idx"])
    order = np.argsort((idx % D) * N + idx // D, kind="stable")          # the device's order: ascending d N + i
    idx = idx[order]
    y = np.asarray(pb["y"])[order]
    S = X.shape[0] * X.shape[1]
    s2 = (np.log1p(np.exp(sp)) + np.asarray(pb["LB"])).reshape(S, D)[:, idx % D]
    ll = -0.5 * (np.log(2.0 * np.pi * s2) + (X.reshape(S, N * D)[:, idx] - y) ** 2 / s2)
    mx = ll.max(axis=0)
    lpd = mx + np.log(np.exp(ll - mx).sum(axis=0)) - np.log(S)
    p_waic = ll.var(axis=0, ddof=1)
    t2 = time.perf_counter()
    elpd_loo, khat = psis_columns(ll)
    timing.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
    return {"lpd": lpd, "p_waic": p_waic, "elpd_waic": lpd - p_waic, "elpd_loo": elpd_loo, "khat": khat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_exp_elpd.json"))
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
        dev_ms, dev_all = median_ms(lambda: eng.sampler_elpd(), a.reps)
        waic_ms, waic_all = median_ms(lambda: eng.sampler_elpd(loo=False), a.reps)
        timing = []
        host_ms, host_all = median_ms(lambda: host_route(eng, pb, timing), a.reps)
        got, ref = eng.sampler_elpd(), host_route(eng, pb, timing)
        diff = {s: float(np.nanmax(np.abs(got["pointwise"][s] - ref[s]) / np.maximum(1.0, np.abs(ref[s])))) for s in ("lpd", "elpd_waic", "elpd_loo", "khat")}
        row = {"shape": name, "chains": C, "results": a.results, "N": eng.N, "D": eng.D, "n_obs": got["n_obs"],
               "sample_bytes": int(C * a.results * (eng.N * eng.D + eng.D + eng.P) * 8),
               "device_elpd_ms": round(dev_ms, 3), "device_elpd_ms_all": dev_all, "device_waic_only_ms": round(waic_ms, 3), "device_waic_only_ms_all": waic_all,
               "host_route_ms": round(host_ms, 3), "host_route_ms_all": host_all,
               "host_download_ms": round(float(np.median([t[0] for t in timing[1:]])), 3),
               "host_numpy_loglik_waic_ms": round(float(np.median([t[1] for t in timing[1:]])), 3),
               "host_numpy_psis_ms": round(float(np.median([t[2] for t in timing[1:]])), 3),
               "speedup": round(host_ms / dev_ms, 2), "max_rel_diff": diff, "elpd_loo": got["elpd_loo"], "se_elpd_loo": got["se_elpd_loo"],
               "elpd_waic": got["elpd_waic"], "n_khat_bad": got["n_khat_bad"], "n_nonfinite": got["n_nonfinite"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_elpd.py", "what": "model-comparison step of predict(elpd=True, keep_samples=False) (device: pointwise log-likelihood, "
                   "lpd, WAIC, PSIS-LOO and khat of every observation) vs sampler_samples() + the vectorised float64 numpy route; host clock around "
                   "calls that end in a device synchronise, median of reps after one warm-up", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
