"""Time the forward sensitivities and Fisher information of MagiEngine.ode_sensitivities -- one call, everything on the device -- against
(a) MagiEngine.ode_solve of the same draws, which prices the sensitivities, and (b) the route a caller has without it: central differences
through 2 (P + D) + 1 ode_solve calls whose trajectories cross to the host, plus the Fisher information in numpy.

    python tools/exp_sens.py [--out profiles/r21_exp_sens.json] [--outputs 1024] [--reps 5] [--device-only]

Shapes: BASELINE config 2's (SEIR-4, T = 1024 outputs at dt = 0.025, 1000 draws, all P + D = 7 columns) and eight chains' 8000 draws;
the draws are the truth's theta and x0 perturbed by <= 5 %.  The observations of the Fisher information are every second output of
every component, weight 1, a variance per draw.  Each route is a host clock around calls that end in a device synchronise, one untimed
warm-up, then the median of ``--reps``.  The sensitivity call is timed without the download of the draws' sensitivities (means, sds and
the Fisher information alone cross: what posterior_sensitivities asks for), and once with it.  ``columns``: the same call with 1, 2, 4
and all 7 columns -- a lane integrates the state again for every column, so the time per column is where that recomputation shows.
``--device-only`` runs the device calls alone (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magi_v2_amd.engine import MagiEngine         # noqa: E402

DRIFT, D, P = "seir4", 4, 3
THETA, X0, DT = np.array([6.0, 0.6, 1.8]), np.array([0.99, 0.01, 0.0, 0.0]), 0.025
FD_REL = 1e-6                                     # central-difference step: FD_REL max(|value|, 1e-3) -- the step a caller has to guess


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(t, 3) for t in out]


def draws(S, seed=0):
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (S, D + P))
    return X0[None] * (1.0 + 0.05 * u[:, :D]), THETA[None] * (1.0 + 0.05 * u[:, D:])


def observations(T, S, seed=1):
    j = np.arange(0, T, 2)
    return {"j": np.repeat(j, D), "comp": np.tile(np.arange(D), len(j)), "weight": None,
            "sigma_sq": np.random.default_rng(seed).uniform(1e-4, 4e-4, (S, D)), "link": None}


def fd_route(eng, x0, th, t, obs):
    """Central differences through ode_solve, then F[s] = sum_k s_a s_b / sigma^2 in numpy: (sens [S, T, D, Q], fim_mean)."""
    base = eng.ode_solve(x0, th, t, drift=DRIFT)["trajectories"]
    cols = []
    for q in range(P + D):
        xp, xm, tp, tm = x0.copy(), x0.copy(), th.copy(), th.copy()
        v = th[:, q] if q < P else x0[:, q - P]
        h = FD_REL * np.maximum(np.abs(v), 1e-3)
        if q < P:
            tp[:, q] += h
            tm[:, q] -= h
        else:
            xp[:, q - P] += h
            xm[:, q - P] -= h
        up = eng.ode_solve(xp, tp, t, drift=DRIFT)["trajectories"]
        dn = eng.ode_solve(xm, tm, t, drift=DRIFT)["trajectories"]
        cols.append((up - dn) / (2.0 * h)[:, None, None])
    sens = np.stack(cols, axis=3)
    z = sens[:, obs["j"], obs["comp"], :]                                   # [S, n_obs, Q]
    F = np.einsum("sk,ska,skb->sab", 1.0 / obs["sigma_sq"][:, obs["comp"]], z, z)
    ok = np.isfinite(base).all(axis=(1, 2))
    return sens, F[ok].mean(axis=0)


def measure(eng, S, T, reps, device_only):
    x0, th = draws(S)
    t = DT * np.arange(T)
    obs = observations(T, S)
    Q = P + D
    res = {"draws": S, "outputs": T, "columns_all": Q, "n_obs": int(len(obs["j"]))}
    res["sens_fim_ms"], res["sens_fim_ms_all"] = median_ms(lambda: eng.ode_sensitivities(x0, th, t, obs=obs, return_draws=False, drift=DRIFT), reps)
    res["solve_ms"], res["solve_ms_all"] = median_ms(lambda: eng.ode_solve(x0, th, t, return_draws=False, drift=DRIFT), reps)
    res["sens_over_solve"] = res["sens_fim_ms"] / res["solve_ms"]
    res["columns"] = {}
    for n in (1, 2, 4, Q):
        ms, _ = median_ms(lambda: eng.ode_sensitivities(x0, th, t, wrt=list(range(n)), return_draws=False, drift=DRIFT), reps)
        res["columns"][str(n)] = ms
    res["ms_per_column"] = (res["columns"][str(Q)] - res["columns"]["1"]) / (Q - 1)
    if device_only:
        return res
    res["sens_fim_with_draws_ms"], _ = median_ms(lambda: eng.ode_sensitivities(x0, th, t, obs=obs, drift=DRIFT), max(1, reps // 2))
    res["fd_route_ms"], res["fd_route_ms_all"] = median_ms(lambda: fd_route(eng, x0, th, t, obs), max(1, reps // 2))
    res["fd_route_solves"] = 2 * Q + 1
    res["fd_over_sens"] = res["fd_route_ms"] / res["sens_fim_ms"]
    res["fd_over_sens_with_draws"] = res["fd_route_ms"] / res["sens_fim_with_draws_ms"]
    dev = eng.ode_sensitivities(x0, th, t, obs=obs, drift=DRIFT)
    fd, fd_fim = fd_route(eng, x0, th, t, obs)
    scale = np.abs(dev["sens"]).max(axis=(0, 1, 2))
    res["fd_vs_device_rel_per_column"] = (np.abs(fd - dev["sens"]).max(axis=(0, 1, 2)) / scale).tolist()
    res["fd_vs_device_fim_mean_rel"] = float(np.abs(fd_fim - dev["fim_mean"]).max() / np.abs(dev["fim_mean"]).max())
    res["n_failed"], res["n_fim_excluded"] = dev["n_failed"], dev["n_fim_excluded"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_exp_sens.json"))
    ap.add_argument("--outputs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    eng = MagiEngine(0)
    try:
        out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "drift": DRIFT, "substeps": 4, "fd_rel_step": FD_REL, "clock": "host, around synchronising calls",
               "shapes": {"config2_1000_draws": measure(eng, 1000, a.outputs, a.reps, a.device_only),
                          "eight_chains_8000_draws": measure(eng, 8000, a.outputs, a.reps, a.device_only)}}
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    if not a.device_only:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
