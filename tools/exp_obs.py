"""Dev: what the observation model costs per leapfrog slot on the default path -> profiles/r12_exp_obs.json.

    python tools/exp_obs.py --parent-lib PATH/libmagi_hip.so [--repeats 7] [--out profiles/r12_exp_obs.json]

  Config 2's shape (SEIR N = 1024 x 4, dense), fixed-L HMC (L = 32, fixed step: every slot is a full leapfrog of every chain), device time
  per slot issued, at one chain (k_stream<1>) and at 8 chains (config 3's per-GPU share, k_stream_sep<CW=8>).  Legs: the library built from
  the parent commit (loaded through MAGI_HIP_LIB), this library with the model never set, this library with a model set (log links on S
  and R, weights in (0.25, 4) on a random half of the observations; data and start floored at 1e-3 there, inside the log's domain)
  -- ALTERNATING, `--repeats` times each.  The json holds every repeat, each leg's median, the spread
  (max - min) of the parent's own repeats and the difference of the medians; the bar for the unset leg is that spread.

Every leg is a child process of its own under a time limit; the first leg that fails or runs out of time ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OBS_SYMBOLS = ("magi_set_obs_model", "magi_get_obs_model")
N, HMC_L, SEED = 1024, 32, 808
LINKS = ["log", "identity", "identity", "log"]
FLOOR = 1e-3


def child_slot(parent, model, chains):
    import numpy as np
    import bench
    from magi_v2_amd import engine, host
    if parent:                                    # the parent library has no observation-model entry points: do not ask it for them
        for name in OBS_SYMBOLS:
            engine._SYMBOLS.pop(name, None)
    I, X_obs, _, _ = host.synthetic_seir(N, seed=0)
    pb = bench.setup_problem(host, I, X_obs, 3)
    eng = engine.MagiEngine(0)
    eng.build_matrices(I, pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=None, want_host=False)
    y, Xhat = np.array(pb["y"], dtype=np.float64), np.array(pb["Xhat"], dtype=np.float64)
    if model:                                     # the log-linked components inside the link's domain (the synthetic data are clipped at 0)
        logged = np.isin(np.asarray(pb["idx"]) % 4, (0, 3))
        y[logged] = np.maximum(y[logged], FLOOR)
        Xhat[:, [0, 3]] = np.maximum(Xhat[:, [0, 3]], FLOOR)
    eng.set_problem(pb["mu"], pb["N_ds"], pb["idx"], y, pb["beta"], pb["LB"], "seir4")
    th_pre0 = pb["th_pre0"]
    if model:
        rng = np.random.default_rng(SEED)
        w = np.ones(len(y))
        half = rng.permutation(len(y))[: len(y) // 2]
        w[half] = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(half)))
        eng.set_obs_model(LINKS, w)
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    cfg = eng.default_cfg(num_results=120, num_burnin_steps=20, stale_cache=0, mode=1, hmc_leapfrogs=HMC_L, step_size=1e-5, num_adaptation_steps=0)
    eng.sampler_init(cfg, rep(Xhat), rep(pb["sig_pre0"]), rep(th_pre0), seed=SEED)
    kernel = eng.stream_kernel_name(chains)
    eng.sampler_run(20)
    out = []
    for _ in range(5):
        lf, ms = eng.sampler_run(20)
        slots, _ = eng.sampler_run_stats()
        out.append(ms * 1e3 / slots)
    eng.close()
    return {"us_per_slot_runs": out, "us_per_slot": float(np.median(out)), "kernel": kernel}


def run_child(args, lib, limit):
    env = dict(os.environ)
    if lib:
        env["MAGI_HIP_LIB"] = lib
    else:
        env.pop("MAGI_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"leg {args} ended with status {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chains", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_exp_obs.json"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_slot(a.child[0] == "parent", a.child[1] == "set", int(a.child[2]))))
        return
    import numpy as np
    out = {"shape": f"SEIR N = {N} x 4, dense", "mode": f"fixed-L HMC, L = {HMC_L}", "set_leg": {"obs_link": LINKS, "obs_weight": "(0.25, 4) on a random half"}}
    for chains in [int(c) for c in a.chains.split(",")]:
        runs = {"parent": [], "unset": [], "set": []}
        kernel = None
        for _ in range(a.repeats):                       # the three legs alternate
            if a.parent_lib:
                runs["parent"].append(run_child(["parent", "unset", str(chains)], os.path.abspath(a.parent_lib), 180)["us_per_slot"])
            r = run_child(["this", "unset", str(chains)], None, 180)
            kernel = r["kernel"]
            runs["unset"].append(r["us_per_slot"])
            runs["set"].append(run_child(["this", "set", str(chains)], None, 180)["us_per_slot"])
        s = {"chains": chains, "kernel": kernel, "us_per_slot": runs, "median": {k: float(np.median(v)) for k, v in runs.items() if v}}
        s["set_minus_unset_us"] = s["median"]["set"] - s["median"]["unset"]
        if runs["parent"]:
            s["parent_spread_us"] = float(max(runs["parent"]) - min(runs["parent"]))
            s["unset_minus_parent_us"] = s["median"]["unset"] - s["median"]["parent"]
            s["inside_parent_spread"] = bool(abs(s["unset_minus_parent_us"]) <= s["parent_spread_us"])
        else:
            s["parent"] = "not measured (no --parent-lib)"
        out[f"chains_{chains}"] = s
        print(json.dumps(s), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
