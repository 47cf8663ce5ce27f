"""The reference's vignette (vignette.ipynb cells 3-8) run through this package: same calls, numpy in place of tf.*.

    python examples/vignette_seir.py            # needs an MI355X and the built library (python -m magi_v2_amd.build)

Data: the 81 thinned rows of data/SEIR_seed=0.csv held in tests/golden/g3_pipeline.npz (every 50th row, t <= 4)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import magi_v2  # noqa: E402  (the drop-in module)
from magi_v2_amd.host import compare_elpd  # noqa: E402


def f_vec(t, X, thetas):
    """SEIR with S implicit (vignette.ipynb cell 3); theta = (beta, gamma, sigma)."""
    S = 1.0 - np.reshape(np.sum(X, axis=1), (-1, 1))
    return np.concatenate([(thetas[0] * S * X[:, 1:2]) - (thetas[2] * X[:, 0:1]),
                           (thetas[2] * X[:, 0:1]) - (thetas[1] * X[:, 1:2]),
                           (thetas[1] * X[:, 1:2])], axis=1)


def report(tag, results, model):
    th = results["thetas_samps"].reshape(-1, 3)
    print(f"[{tag}] theta posterior mean {np.round(th.mean(axis=0), 3)} sd {np.round(th.std(axis=0), 3)} (truth 6, 0.6, 1.8); "
          f"mean tree depth {results['kernel_results']['tree_depth'].mean():.2f}, {results['minutes_elapsed']} min")
    # the reconstructed trajectory: the ODE solved on the GPU from every draw's x(0) and theta; its posterior mean against the observations
    pt = model.posterior_trajectories(results, return_draws=False)
    at_obs = np.abs(pt["t"][:, None] - np.asarray(model.ts_obs, dtype=np.float64).reshape(1, -1)).argmin(axis=0)      # grid index of every observation time
    rmse = np.sqrt(np.nanmean((pt["mean"][at_obs] - model.X_obs) ** 2, axis=0))
    print(f"[{tag}] reconstructed-trajectory RMSE against the observations per component {np.round(rmse, 4)} "
          f"({pt['n_failed']} of {pt['status'].size} trajectories not finite)")


def main():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "g3_pipeline.npz"))
    ts_obs, X_obs = g["seir3_ts_obs"], g["seir3_X_obs"]
    model = magi_v2.MAGI_v2(D_thetas=3, ts_obs=ts_obs, X_obs=X_obs, bandsize=80, f_vec=f_vec)

    # 1. the vignette's calls, unchanged.  As coded, the reference fits the GP hyper-parameters on the linearly interpolated
    #    grid and initialises theta through a reshape quirk; restated faithfully that gives tiny noise levels, theta_init < 0
    #    (-> 0.007 through the -5 fallback) and a poor posterior (DESIGN.md section 8 -- the notebook's printed 5.83 / 0.565 /
    #    1.77 is stale output of an unseeded run).
    model.initial_fit(discretization=1, verbose=True)
    print("fitted on the grid: phi2", np.round(model.phi2s, 3), "sigma", np.round(np.sqrt(model.sigma_sqs_init), 4), "theta_init", np.round(model.thetas_init, 3))
    report("reference defaults", model.predict(num_results=500, num_burnin_steps=500, verbose=True), model)

    # 2. this package's documented alternative: fit the hyper-parameters on the observation times, start theta at 1
    model.initial_fit(discretization=1, hparam_fit_on="observed")
    sigma_fit = model.sigma_sqs_init.copy()
    model.thetas_init = np.ones(3)
    print("fitted on the observed rows: phi2", np.round(model.phi2s, 3), "sigma", np.round(np.sqrt(sigma_fit), 4))
    fitted_phi = model.predict(num_results=500, num_burnin_steps=500, n_chains=4, seed=1, elpd=True)
    report("fit on observed rows", fitted_phi, model)

    # 3. user-supplied hyper-parameters (the reference lets users overwrite them, magi_v2.py:77-80)
    model.initial_fit(discretization=1, hparams={"phi2s": [0.5, 0.5, 0.5], "sigma_sqs": sigma_fit})
    model.thetas_init = np.ones(3)
    fixed_phi = model.predict(num_results=500, num_burnin_steps=500, n_chains=4, seed=1, elpd=True)
    report("phi2 = 0.5, fitted noise", fixed_phi, model)

    # 4. which of the two do the data prefer?  PSIS-LOO of the observations under the hyper-parameters of step 2 against those of step 3,
    #    computed on the GPU from the samples each run left there.  Both runs see the same observations through the same (identity) link,
    #    so their pointwise values pair up.  An elpd_diff within a couple of se_diff decides nothing; observations with khat > 0.7 are
    #    those the posterior cannot predict without them, and their elpd_loo is not reliable.
    for row in compare_elpd({"fitted phi2": fitted_phi["elpd"], "phi2 = 0.5": fixed_phi["elpd"]}):
        print(f"[model comparison] {row['name']}: elpd_loo {row['elpd']:.1f} (se {row['se']:.1f}), p_loo {row['p']:.1f}, "
              f"elpd_diff {row['elpd_diff']:.1f} (se {row['se_diff']:.1f}), {row['n_khat_bad']} observation(s) with khat > 0.7")


if __name__ == "__main__":
    main()
