"""Time the rank-normalised diagnostics of predict(summary=True, rank_diagnostics=True) -- MagiEngine.sampler_rank_diagnostics, everything
on the device -- against the route a caller has without it: sampler_samples() (all draws to the host) + scipy rankdata + ndtri + a
vectorised numpy ESS (FFT autocovariances, Geyer truncation) of the four derived series, and sampler_summary before and after in the same
session (the new unit must not move it).

    python tools/exp_rank.py [--out profiles/r20_exp_rank.json] [--results 1000] [--grid 1024] [--device-only]

Shapes: those of tools/exp_summary.py -- BASELINE config 2 (1 chain, N = 1024 x 4 dense) and config 3's per-GPU share
(8 chains), ``--results`` draws per chain, sampled with a shallow tree and stale_cache=0.  Each route is a host clock around a call that
ends in a device synchronise, one untimed warm-up, then the median of ``--reps`` (the host route: ``--host-reps``).  ``--device-only``
runs the device calls alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/exp_rank.py --device-only)."""
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

TAIL = 0.05
DIAG = ("rhat_rank", "ess_bulk", "ess_tail")


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def rhat_ess(a):
    """Split R-hat and ESS (include/magi_hip.h's definitions, all lags) of the series a[C][R][K] in float64, every column at once."""
    C, R, K = a.shape
    n, M = R // 2, 2 * C
    zs = np.concatenate([a[:, :n], a[:, R - n:]], axis=0)
    mean = zs.mean(axis=1)
    zc = zs - mean[:, None]
    W = ((zc ** 2).sum(axis=1) / (n - 1)).mean(axis=0)
    varp = (n - 1) / n * W + (mean.var(axis=0, ddof=1) if M > 1 else 0.0)
    f = np.fft.rfft(zc, n=2 * n, axis=1)
    acov = np.fft.irfft(f * np.conj(f), n=2 * n, axis=1)[:, :n].mean(axis=0) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = 1.0 - (W - acov) / varp
        rho[0] = 1.0
        pairs = n // 2
        P = rho[0:2 * pairs:2] + rho[1:2 * pairs:2]
        first = np.where((P < 0).any(axis=0), (P < 0).argmax(axis=0), pairs)
        Pm = np.minimum.accumulate(P, axis=0) * (np.arange(pairs)[:, None] < first[None, :])
        tau = np.maximum(-1.0 + 2.0 * Pm.sum(axis=0), 1.0 / np.log10(M * n))
        return np.sqrt(varp / W), M * n / tau


def host_diagnostics(a, block=512):
    """The three diagnostics of a[C][R][...] on the host, ``block`` columns at a time."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    C, R = a.shape[:2]
    S = C * R
    flat = a.reshape(C, R, -1)
    out = {s: np.empty(flat.shape[2]) for s in DIAG}
    for k0 in range(0, flat.shape[2], block):
        y = flat[:, :, k0:k0 + block].reshape(S, -1)
        z = lambda v: ndtri((rankdata(v, axis=0) - 0.375) / (S + 0.25)).reshape(C, R, -1)
        v = np.sort(y, axis=0)
        rz, ez = rhat_ess(z(y))
        rf, _ = rhat_ess(z(np.abs(y - np.median(y, axis=0))))
        lo = rhat_ess((y <= v[int(np.floor((S - 1) * TAIL))]).astype(np.float64).reshape(C, R, -1))[1]
        hi = rhat_ess((y <= v[int(np.floor((S - 1) * (1.0 - TAIL)))]).astype(np.float64).reshape(C, R, -1))[1]
        sl = slice(k0, k0 + y.shape[1])
        out["rhat_rank"][sl], out["ess_bulk"][sl], out["ess_tail"][sl] = np.maximum(rz, rf), ez, np.minimum(lo, hi)
    return {s: v.reshape(a.shape[2:]) for s, v in out.items()}


def host_route(eng, LB, timing):
    t0 = time.perf_counter()
    X, sp, tp = eng.sampler_samples()
    t1 = time.perf_counter()
    sig, th = host.transform_samples(sp, tp, LB)
    res = {name: host_diagnostics(a) for name, a in (("X", X), ("sigma_sqs", sig), ("thetas", th))}
    timing.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_exp_rank.json"))
    ap.add_argument("--results", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--device-only", action="store_true")
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
        sum_before, sum_before_all = median_ms(lambda: eng.sampler_summary(), a.reps)
        dev_ms, dev_all = median_ms(lambda: eng.sampler_rank_diagnostics(), a.reps)
        sum_after, sum_after_all = median_ms(lambda: eng.sampler_summary(), a.reps)
        got = eng.sampler_rank_diagnostics()
        finite = lambda v: np.asarray(v)[np.isfinite(v)]
        row = {"shape": name, "chains": C, "results": a.results, "N": eng.N, "D": eng.D, "columns": int(eng.N * eng.D + eng.D + eng.P),
               "sample_bytes": int(C * a.results * (eng.N * eng.D + eng.D + eng.P) * 8),
               "device_rank_ms": round(dev_ms, 3), "device_rank_ms_all": dev_all,
               "sampler_summary_ms_before": round(sum_before, 3), "sampler_summary_ms_before_all": sum_before_all,
               "sampler_summary_ms_after": round(sum_after, 3), "sampler_summary_ms_after_all": sum_after_all,
               "median_rhat_rank_X": float(np.median(finite(got["X"]["rhat_rank"]))), "median_ess_bulk_X": float(np.median(finite(got["X"]["ess_bulk"]))),
               "median_ess_tail_X": float(np.median(finite(got["X"]["ess_tail"]))),
               "rhat_rank_thetas": [round(float(v), 4) for v in got["thetas"]["rhat_rank"]],
               "ess_bulk_thetas": [round(float(v), 1) for v in got["thetas"]["ess_bulk"]], "ess_tail_thetas": [round(float(v), 1) for v in got["thetas"]["ess_tail"]]}
        if not a.device_only:
            timing = []
            host_ms, host_all = median_ms(lambda: host_route(eng, pb["LB"], timing), a.host_reps)
            timed = timing[1:]                                        # the runs host_ms is the median of: not the warm-up, not the run below
            ref = host_route(eng, pb["LB"], [])
            with np.errstate(invalid="ignore"):
                diff = {s: float(np.nanmax(np.abs(got["X"][s] - ref["X"][s]) / np.abs(ref["X"][s]))) for s in DIAG}
            row.update({"host_route_ms": round(host_ms, 3), "host_route_ms_all": host_all,
                        "host_download_ms": round(float(np.median([t[0] for t in timed])), 3),
                        "host_rank_ess_ms": round(float(np.median([t[1] for t in timed])), 3),
                        "speedup": round(host_ms / dev_ms, 2), "max_rel_diff_X": diff})
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    if a.device_only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_rank.py", "what": "rank-normalised R-hat, bulk and tail ESS of every column of the device-resident samples "
                   "(sampler_rank_diagnostics) vs sampler_samples() + scipy rankdata / ndtri + vectorised numpy FFT ESS of the four derived series "
                   "(float64); sampler_summary timed before and after in the same session; host clock around calls that end in a device "
                   "synchronise, median of reps after one warm-up", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
