"""Time MAGI_v2.posterior_at's device route -- MagiEngine.sampler_gp_predict: cross blocks, weights, the application GEMM on the resident
samples, statistics, all on the device -- against the host route it replaces: get_dense() (the dense C^-1 to the host) + sampler_samples()
(every draw to the host) + scipy kv for the T x N cross blocks + numpy for the products and the summaries.

    python tools/exp_gp_predict.py [--out profiles/r15_exp_gp_predict.json] [--results 1000] [--grid 1024] [--times 4096]

Shapes: BASELINE config 2 (1 chain, N = 1024 x 4 dense) and config 3's per-GPU share (8 chains), ``--results`` draws per chain, T = ``--times``
new times uniform over the grid's span; summaries only, and with the draws.  The chains are sampled as tools/exp_summary.py samples them.
Device time per stage: HIP events (option gp_profile, a synchronisation per stage), a run of its own.  Whole calls: a host clock around calls that
end in a device synchronise, one untimed warm-up, then ``--reps`` (7) runs per leg, the two routes alternating.  The host route runs with the
thread quota of the box as it is set (numpy's BLAS, OMP_NUM_THREADS)."""
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
FP64_MFMA_PEAK_TFLOPS = 78.6                       # AMD's data sheet, MI355X fp64 matrix
NU = 2.01


def host_route(eng, pb, t_new, parts):
    """What a caller did before: everything to the host, scipy for the Matern blocks, numpy for the rest (means and variances of x(t*) and
    x'(t*), mean / sd / quantiles of the conditional means; no R-hat, no ESS)."""
    from scipy.special import gamma, kv
    t0 = time.perf_counter()
    C_inv, _, _ = eng.get_dense()
    X, _, _ = eng.sampler_samples()
    t1 = time.perf_counter()
    I = np.asarray(pb["I"], dtype=np.float64).reshape(-1)
    pooled = X.reshape(-1, X.shape[2], X.shape[3])
    out = {}
    t_kv = 0.0
    for d in range(X.shape[3]):
        phi1, phi2, mu = pb["hp"]["phi1s"][d], pb["hp"]["phi2s"][d], pb["mu"][d]
        tk = time.perf_counter()
        dlt = t_new[:, None] - I[None, :]
        c = np.sqrt(2 * NU) / phi2
        u = c * np.abs(dlt)
        same = u == 0.0
        u[same] = 1.0
        A = phi1 * 2.0 ** (1.0 - NU) / gamma(NU)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            uv = u ** NU
            Ks, pKs = A * uv * kv(NU, u), -A * c * np.sign(dlt) * uv * kv(NU - 1.0, u)
        Ks[~np.isfinite(Ks)] = 0.0
        pKs[~np.isfinite(pKs)] = 0.0
        Ks[same], pKs[same] = phi1, 0.0
        t_kv += time.perf_counter() - tk
        W, Wd = Ks @ C_inv[d], pKs @ C_inv[d]
        xc = (pooled[:, :, d] - mu).T
        x_new, dx_new = mu + (W @ xc).T, (Wd @ xc).T
        out[d] = (x_new.mean(axis=0), x_new.std(axis=0, ddof=1), np.quantile(x_new, PROBS, axis=0), dx_new.mean(axis=0), dx_new.std(axis=0, ddof=1),
                  np.quantile(dx_new, PROBS, axis=0), np.maximum(phi1 - (W * Ks).sum(axis=1), 0.0))
    parts.append(((t1 - t0) * 1e3, t_kv * 1e3, (time.perf_counter() - t1) * 1e3 - t_kv * 1e3))
    return out


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_exp_gp_predict.json"))
    ap.add_argument("--results", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--times", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--no-host", action="store_true", help="device legs only (stage times, whole calls): a short run")
    a = ap.parse_args()
    I, X_obs, _, _ = host.synthetic_seir(a.grid)
    pb = problem_setup(I, X_obs, 3)
    eng = MagiEngine(0)
    eng.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], NU, want_host=False)
    eng.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    grid = np.asarray(pb["I"], dtype=np.float64).reshape(-1)
    t_new = np.linspace(grid.min(), grid.max(), a.times)
    N, D, T = eng.N, eng.D, a.times
    at = lambda **kw: eng.sampler_gp_predict(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], t_new, probs=PROBS, **kw)
    rows = []
    for name, C in (("config2", 1), ("config3_share", 8)):
        rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
        cfg = eng.default_cfg(num_results=a.results, num_burnin_steps=a.burnin, max_tree_depth=5, stale_cache=0)
        eng.sampler_init(cfg, rep(pb["Xhat"]), rep(pb["sig_pre0"]), rep(pb["th_pre0"]), seed=7)
        eng.sampler_run(a.results + a.burnin)
        S = C * a.results
        # stages on the device clock (a run of its own: the events synchronise)
        eng.set_option("gp_profile", 1)
        at()
        stages = []
        for _ in range(a.reps):
            at()
            stages.append(eng.gp_profile())
        eng.set_option("gp_profile", 0)
        stage_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        gemm_flops = 2.0 * 2 * D * T * N * S                   # W and Wd against the draws
        weights_flops = 2.0 * 2 * D * T * N * N
        # whole calls, the two routes alternating
        at()
        parts = []
        if not a.no_host:
            host_route(eng, pb, t_new, parts)
        dev, hst, drw = [], [], []
        for _ in range(a.reps):
            dev.append(timed(at)[0])
            if not a.no_host:
                hst.append(timed(lambda: host_route(eng, pb, t_new, parts))[0])
            drw.append(timed(lambda: at(return_draws=True))[0])
        row = {"shape": name, "chains": C, "results": a.results, "N": N, "D": D, "T": T, "draws": S,
               "stage_ms": {k: round(v, 3) for k, v in stage_ms.items()}, "stage_ms_all": [{k: round(v, 3) for k, v in s.items()} for s in stages],
               "application_gemm_gflop": round(gemm_flops / 1e9, 1),
               "application_gemm_fraction_of_fp64_mfma_peak": round(gemm_flops / (stage_ms["application_gemm"] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 4),
               "weights_fraction_of_fp64_mfma_peak_with_variances": round(weights_flops / (stage_ms["weights"] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 4),
               "device_summaries_ms": round(float(np.median(dev)), 3), "device_summaries_ms_all": [round(t, 3) for t in dev],
               "device_with_draws_ms": round(float(np.median(drw)), 3), "device_with_draws_ms_all": [round(t, 3) for t in drw],
               "draws_bytes_to_host": int(2 * S * T * D * 8), "threads": os.environ.get("OMP_NUM_THREADS")}
        if not a.no_host:
            got, ref = at(), host_route(eng, pb, t_new, parts)
            err = max(float(np.abs(got["X"]["mean"][:, d] - ref[d][0]).max() / np.abs(ref[d][0]).max()) for d in range(D))
            derr = max(float(np.abs(got["dX"]["mean"][:, d] - ref[d][3]).max() / np.abs(ref[d][3]).max()) for d in range(D))
            p = np.asarray(parts[1:])
            row.update({
               "host_route_ms": round(float(np.median(hst)), 3), "host_route_ms_all": [round(t, 3) for t in hst],
               "host_download_ms": round(float(np.median(p[:, 0])), 3), "host_scipy_kv_ms": round(float(np.median(p[:, 1])), 3),
               "host_numpy_ms": round(float(np.median(p[:, 2])), 3),
               "host_download_share": round(float(np.median(p[:, 0]) / np.median(hst)), 4),
               "host_over_device_summaries": round(float(np.median(hst) / np.median(dev)), 2), "mean_rel_diff": err, "dmean_rel_diff": derr})
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_gp_predict.py", "what": "MagiEngine.sampler_gp_predict (x and x' at T new times from the device-resident samples: "
                   "conditional means, variances, mean / sd / 3 quantiles / rhat / ess / mcse of both) vs get_dense() + sampler_samples() + scipy kv + "
                   "numpy (means, variances, mean / sd / quantiles; no diagnostics); stages: HIP events; whole calls: host clock, reps alternating runs "
                   "per leg after one warm-up", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
