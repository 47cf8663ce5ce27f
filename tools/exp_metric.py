"""Dev: what the diagonal metric costs per leapfrog slot and what it buys per sample -> profiles/r09_exp_metric.json.

    python tools/exp_metric.py [--parent-lib PATH/libmagi_hip.so] [--repeats 3] [--out profiles/r09_exp_metric.json]

  slot     config 2's shape (SEIR N = 1024 x 4, dense), 8 chains, fixed-L HMC (L = 32, fixed step: every slot is a full leapfrog of every
           chain), device time per slot issued.  Legs: this library with the metric unset and with a metric set; with --parent-lib (the
           library built from the parent commit, loaded through MAGI_HIP_LIB) the parent, ALTERNATING with this library, `--repeats`
           times each.  The json holds every repeat, the spread of the parent's own repeats and the difference of the means.
  config2  N = 1024 x 4, one chain, 400 + 100 transitions, same seed, engine-level predict(adapt_metric=False / True): leapfrogs per
           sample, samples/s of the 100 results and the summary kernel's min ESS/s.

Every leg is a child process of its own under a time limit; the first leg that fails or runs out of time ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METRIC_SYMBOLS = ("magi_sampler_set_metric", "magi_sampler_get_metric", "magi_sampler_metric_window", "magi_sampler_adapt_metric")
N, CHAINS, HMC_L, SEED = 1024, 8, 32, 808


def _engine(parent):
    import numpy as np
    import bench
    from magi_v2_amd import engine, host
    if parent:                                    # the parent library has no metric entry points: do not ask it for them
        for name in METRIC_SYMBOLS:
            engine._SYMBOLS.pop(name, None)
    I, X_obs, _, _ = host.synthetic_seir(N, seed=0)
    pb = bench.setup_problem(host, I, X_obs, 3)
    eng = engine.MagiEngine(0)
    eng.build_matrices(I, pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=None, want_host=False)
    eng.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    return eng, pb, np


def child_slot(parent, metric):
    eng, pb, np = _engine(parent)
    rep = lambda v: np.repeat(np.asarray(v)[None], CHAINS, axis=0)
    cfg = eng.default_cfg(num_results=120, num_burnin_steps=20, stale_cache=0, mode=1, hmc_leapfrogs=HMC_L, step_size=1e-5, num_adaptation_steps=0)
    eng.sampler_init(cfg, rep(pb["Xhat"]), rep(pb["sig_pre0"]), rep(pb["th_pre0"]), seed=SEED)
    if metric:
        rng = np.random.default_rng(1)
        lu = lambda *shape: np.exp(rng.uniform(np.log(0.5), np.log(2.0), shape)) ** 2
        eng.sampler_set_metric(lu(CHAINS, N, 4), lu(CHAINS, 4), lu(CHAINS, 3))
    eng.sampler_run(20)
    out = []
    for _ in range(5):
        lf, ms = eng.sampler_run(20)
        slots, _ = eng.sampler_run_stats()
        out.append(ms * 1e3 / slots)
    eng.close()
    return {"us_per_slot_runs": out, "us_per_slot": float(np.median(out))}


def child_config2(adapt):
    from magi_v2_amd import host
    eng, pb, np = _engine(False)
    B, R = 400, 100
    cfg = eng.default_cfg(num_results=R, num_burnin_steps=B, stale_cache=0)
    eng.sampler_init(cfg, pb["Xhat"][None], pb["sig_pre0"][None], pb["th_pre0"][None], seed=SEED)
    n_adapt = int(0.8 * B)
    windows = []
    if adapt:
        _, _, windows = eng.sampler_warmup(host.warmup_schedule(B, n_adapt))
        eng.sampler_run(B - n_adapt)
    else:
        eng.sampler_run(B)
    lf, ms = eng.sampler_run(R)
    d = eng.sampler_diag()
    summ = eng.sampler_summary()
    ess = min(float(np.nanmin(summ[k]["ess"])) for k in ("X", "sigma_sqs", "thetas"))
    out = {"adapt_metric": bool(adapt), "leapfrogs_per_sample": float(d.leapfrogs_taken[0, B:].mean()), "leapfrogs_per_burnin_transition": float(d.leapfrogs_taken[0, :B].mean()),
           "samples_per_s": R / (ms * 1e-3), "min_ess": ess, "min_ess_per_s": ess / (ms * 1e-3), "results_device_ms": ms,
           "step_size_last": float(d.step_size[0, -1]), "mean_tree_depth": float(d.tree_depth[0, B:].mean()),
           "windows": [(w["start"], w["stop"], float(w["step_size"][0])) for w in windows]}
    eng.close()
    return out


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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_exp_metric.json"))
    ap.add_argument("--legs", default="slot,config2")
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        res = child_slot(a.child[1] == "parent", a.child[2] == "set") if kind == "slot" else child_config2(a.child[1] == "on")
        print(json.dumps(res))
        return
    import numpy as np
    out = {"shape": f"SEIR N = {N} x 4, dense", "slot": "not measured", "config2": "not measured"}
    if "slot" in a.legs:
        runs = {"parent": [], "unset": [], "set": []}
        for _ in range(a.repeats):                       # parent and this library alternate
            if a.parent_lib:
                runs["parent"].append(run_child(["slot", "parent", "unset"], os.path.abspath(a.parent_lib), 180)["us_per_slot"])
            runs["unset"].append(run_child(["slot", "this", "unset"], None, 180)["us_per_slot"])
            runs["set"].append(run_child(["slot", "this", "set"], None, 180)["us_per_slot"])
        s = {"chains": CHAINS, "mode": f"fixed-L HMC, L = {HMC_L}", "us_per_slot": runs, "mean": {k: float(np.mean(v)) for k, v in runs.items() if v}}
        s["metric_set_minus_unset_us"] = s["mean"]["set"] - s["mean"]["unset"]
        if runs["parent"]:
            s["parent_spread_us"] = float(max(runs["parent"]) - min(runs["parent"]))
            s["unset_minus_parent_us"] = s["mean"]["unset"] - s["mean"]["parent"]
            s["inside_parent_spread"] = bool(abs(s["unset_minus_parent_us"]) <= s["parent_spread_us"])
        else:
            s["parent"] = "not measured (no --parent-lib)"
        out["slot"] = s
        print(json.dumps(s), flush=True)
    if "config2" in a.legs:
        off = run_child(["config2", "off"], None, 240)
        on = run_child(["config2", "on"], None, 240)
        out["config2"] = {"chains": 1, "burnin": 400, "results": 100, "seed": SEED, "off": off, "on": on,
                          "leapfrogs_per_sample_ratio_off_over_on": off["leapfrogs_per_sample"] / on["leapfrogs_per_sample"]}
        print(json.dumps(out["config2"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
