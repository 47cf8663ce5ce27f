"""Time the error-controlled integrators (MagiEngine.ode_solve(method="dopri5" / "ros23"), magi_ode_solve_adaptive) against the two routes a
caller had before: the device's RK4 (magi_ode_solve) at the fewest sub-steps that are as accurate, and scipy.solve_ivp on the host.

    python tools/exp_ode_adaptive.py [--out profiles/r14_exp_ode_adaptive.json] [--draws 1000 8000] [--resources profiles/r14_kernel_resource_usage.txt]

Cases and draws: those of tests/ode_adaptive_reference.py (T = 41 output times; chain8 33), S draws perturbed by <= 5 %.
Accuracy: worst |x - truth| / (atol + rtol |truth|) over the first ``--truth`` draws, truth = solve_ivp (Radau with the analytic Jacobian on
  the stiff cases, DOP853 otherwise) at rtol 1e-12, atol 1e-14.  The RK4 partner of a method is the smallest power of two of ``substeps``
  <= 1024 whose error on those draws is no larger than the method's, where one exists.
Device times: host clock around ode_solve(return_draws=False) -- upload, kernel, statistics, download of mean / sd / status -- one untimed
  warm-up, then the median of ``--reps``.
Host route: solve_ivp (Radau + Jacobian on the stiff cases, RK45 otherwise) at the same rtol / atol on the first ``--scipy-draws`` draws through
  a pool of ``--procs`` processes (started before the GPU is opened; they never open it), scaled to S draws.
Divergence: per wave of 64 draws, max / mean of accepted + rejected steps -- what the slowest lane costs its wave."""
import argparse
import functools
import json
import multiprocessing as mp
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOL = 1e-9
STIFF = ("robertson", "van_der_pol", "forced_relaxation")
PLAN = (("robertson", ("ros23",)), ("van_der_pol", ("dopri5", "ros23")), ("forced_relaxation", ("ros23", "dopri5")),
        ("seir3", ("dopri5", "ros23")), ("lotka_volterra", ("dopri5", "ros23")), ("seir_seasonal", ("dopri5", "ros23")),
        ("chain8", ("dopri5", "ros23")))


@functools.lru_cache(maxsize=None)
def _drift(name):
    from magi_v2_amd import drift
    from tests import ode_adaptive_reference as R
    if name in R.BUILTIN:
        return drift.builtin_drift(name)
    return drift.resolve(*R.TRACED[name])


def host_solve(job):
    """One draw through solve_ivp (runs in a pool process; never touches the GPU)."""
    from scipy.integrate import solve_ivp
    name, x0, th, t_out, method, rtol, atol = job
    d = _drift(name)
    f = lambda t, y: d.f_np(np.array([t]), y[None], th)[0]
    kw = {}
    if method == "Radau":
        kw["jac"] = lambda t, y: d.jac_np(y[None], th, np.array([t]) if d.time_dependent else None)[0][0]
    sol = solve_ivp(f, (t_out[0], t_out[-1]), x0, t_eval=t_out, method=method, rtol=rtol, atol=atol, **kw)
    return sol.y.T if sol.success else np.full((len(t_out), len(x0)), np.nan)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def resources(path):
    """{(drift or "base", kernel): (VGPRs, scratch B/lane, occupancy)} from a table of tools/resource_usage.py."""
    out, block = {}, "base"
    if not path or not os.path.exists(path):
        return out
    for line in open(path):
        m = re.match(r"# hipcc .*ode_adaptive\.hip(?: for the traced drift (\w+))?", line)
        if m:
            block = m.group(1) or "base"
        m = re.match(r"(k_ode_\w+<[\d, ]+>).*?\|\s*(\d+) \|\s*\d+ \|\s*\d+ \|\s*(\d+) \|\s*(\d+) \|", line)
        if m:
            out[(block, m.group(1))] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_exp_ode_adaptive.json"))
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "r14_kernel_resource_usage.txt"))
    ap.add_argument("--draws", type=int, nargs="+", default=[1000, 8000])
    ap.add_argument("--truth", type=int, default=16)
    ap.add_argument("--scipy-draws", type=int, default=64)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-6)
    a = ap.parse_args()
    pool = mp.get_context("spawn").Pool(a.procs)
    from magi_v2_amd.engine import DRIFT_IDS, MagiEngine
    from tests import ode_adaptive_reference as R
    res = resources(a.resources)
    err_of = lambda x, truth: float(np.nanmax(np.abs(x - truth) / (ATOL + a.rtol * np.abs(truth)))) if np.isfinite(x).all() else float("inf")
    rows = []
    for name, methods in PLAN:
        case, d = R.CASES[name], _drift(name)
        x0, th = R.draws(case, max(a.draws))
        nt = a.truth
        truth = np.stack(pool.map(host_solve, [(name, x0[s], th[s], case.t, "Radau" if name in STIFF else "DOP853", 1e-12, 1e-14) for s in range(nt)]))
        t0 = time.perf_counter()
        sci = np.stack(pool.map(host_solve, [(name, x0[s], th[s], case.t, "Radau" if name in STIFF else "RK45", a.rtol, ATOL) for s in range(a.scipy_draws)]))
        scipy_ms_per_draw = (time.perf_counter() - t0) * 1e3 / a.scipy_draws
        scipy_err = err_of(sci[:nt], truth)
        eng = MagiEngine(0) if d.is_builtin else MagiEngine(0, drift=d)
        dr = name if d.is_builtin else d
        block = "base" if d.is_builtin else name
        drift_id = DRIFT_IDS[name] if d.is_builtin else 3
        rk4_err = {}
        for k in range(11):
            out = eng.ode_solve(x0[:nt], th[:nt], case.t, substeps=1 << k, drift=dr)
            rk4_err[1 << k] = err_of(out["trajectories"], truth)
        for method in methods:
            out = eng.ode_solve(x0[:nt], th[:nt], case.t, drift=dr, method=method, rtol=a.rtol, atol=ATOL)
            err = err_of(out["trajectories"], truth)
            partner = next((s for s, e in rk4_err.items() if e <= err), None)
            for S in a.draws:
                run = lambda **kw: eng.ode_solve(x0[:S], th[:S], case.t, drift=dr, return_draws=False, **kw)
                ms, all_ms = median_ms(lambda: run(method=method, rtol=a.rtol, atol=ATOL), a.reps)
                o = run(method=method, rtol=a.rtol, atol=ATOL)
                n = (o["n_accepted"] + o["n_rejected"]).astype(np.float64)
                pad = np.concatenate([n, np.full(-len(n) % 64, n[-1])]).reshape(-1, 64)
                spread = pad.max(axis=1) / pad.mean(axis=1)
                row = {"case": name, "D": case.D, "method": method, "rtol": a.rtol, "atol": ATOL, "S": S, "T": len(case.t),
                       "error_over_tol": round(err, 3), "adaptive_ms": round(ms, 3), "adaptive_ms_all": all_ms, "n_failed": o["n_failed"],
                       "steps_mean": round(float(n.mean()), 1), "steps_max": int(n.max()), "rejected_share": round(float(o["n_rejected"].sum() / n.sum()), 4),
                       "wave_spread_mean": round(float(spread.mean()), 4), "wave_spread_max": round(float(spread.max()), 4),
                       "rk4_error_over_tol_by_substeps": {str(s): (round(e, 3) if np.isfinite(e) else None) for s, e in rk4_err.items()},
                       "rk4_partner_substeps": partner,
                       "scipy_method": "Radau+jac" if name in STIFF else "RK45", "scipy_error_over_tol": round(scipy_err, 3),
                       "scipy_ms_per_draw_one_process": round(scipy_ms_per_draw * a.procs, 3),
                       "scipy_ms_scaled_to_S": round(scipy_ms_per_draw * S, 1), "scipy_procs": a.procs, "scipy_draws_timed": a.scipy_draws}
                if partner is not None:
                    rms, rall = median_ms(lambda: run(substeps=partner), a.reps)
                    row.update(rk4_ms=round(rms, 3), rk4_ms_all=rall, rk4_over_adaptive=round(rms / ms, 2))
                row["scipy_over_adaptive"] = round(scipy_ms_per_draw * S / ms, 1)
                kern = f"k_ode_adaptive<{drift_id}, {eng.ODE_METHODS[method]}>"
                if (block, kern) in res:
                    row["vgprs"], row["scratch_bytes_per_lane"], row["occupancy_waves_per_simd"] = res[(block, kern)]
                print(json.dumps(row), flush=True)
                rows.append(row)
        eng.close()
    pool.close()
    pool.join()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/exp_ode_adaptive.py", "what": "magi_ode_solve_adaptive (dopri5, ros23) vs magi_ode_solve at the fewest power-of-two "
                   "sub-steps of equal accuracy, and vs scipy.solve_ivp on a pool of host processes; host clock around calls that end in a device "
                   "synchronise, median of reps after one warm-up; errors against solve_ivp at rtol 1e-12 on the first draws", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
