"""Shared helpers for the tests (oracle side only; product code never imports this)."""
import contextlib
import os

import numpy as np

from oracle import magi_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_g4(tag):
    return np.load(os.path.join(GOLDEN, f"g4_logpost_{tag}.npz"))


def problem_from_g4(g, band=None):
    return orc.Problem(I=g["I"], mu=g["mu"], C_inv=orc.band_part(g["C_inv"], band), m=orc.band_part(g["m"], band),
                       K_inv=orc.band_part(g["K_inv"], band), N_ds=g["N_ds"], obs_idx=g["obs_idx"], y=g["y"],
                       beta=float(g["beta"]), LB=g["LB"], drift=str(g["drift"]), P=len(g["theta_true"]))


def engine_for(pr, band=None, device=0, matrices=None, drift=None, options=None):
    """A MagiEngine loaded with the oracle problem's constants (UNmasked matrices + bandsize:
    the engine applies the band mask itself, as the reference does after building).
    ``drift``: a traced magi_v2_amd.drift.Drift -> the engine of the library compiled for it, its times the problem's grid.
    ``options``: {name: value} for set_option BEFORE the matrices are packed."""
    from magi_v2_amd.engine import MagiEngine
    eng = MagiEngine(device) if drift is None else MagiEngine(device, drift=drift)
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    C_inv, m, K_inv = matrices if matrices is not None else (pr.C_inv, pr.m, pr.K_inv)
    eng.set_matrices(C_inv, m, K_inv, bandsize=band)
    if drift is not None:
        eng.set_times(pr.I)
    eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, pr.drift if drift is None else drift)
    return eng


def synthetic_seir_problem(N, seed=0, dt=0.025, alpha=0.05, band=None, phi=None):
    """BASELINE configs 2/3/5: SEIR-4 truth by RK4 (beta=6, gamma=.6, sigma=1.8,
    x0=(.99,.01,0,0)), uniform grid dt, observations at even grid indices with noise
    N(0, (alpha*range_d)^2) from PCG64(seed).  Matrices come from the ORACLE build (tests only)."""
    th = np.array([6.0, 0.6, 1.8])

    def f(x):
        S, E, I, R = x
        return np.array([-th[0] * S * I, th[0] * S * I - th[2] * E, th[2] * E - th[1] * I, th[1] * I])

    sub = 25
    h = dt / sub
    x = np.array([0.99, 0.01, 0.0, 0.0])
    truth = np.zeros((N, 4))
    truth[0] = x
    for i in range(1, N):
        for _ in range(sub):
            k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
            x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        truth[i] = x
    I = np.arange(N) * dt
    rng = np.random.Generator(np.random.PCG64(seed))
    rngs = truth.max(axis=0) - truth.min(axis=0)
    X_obs = np.full((N, 4), np.nan)
    obs_rows = np.arange(0, N, 2)
    X_obs[obs_rows] = truth[obs_rows] + rng.normal(size=(len(obs_rows), 4)) * (alpha * rngs)
    X_obs[X_obs < 0.0] = 0.0
    return I, X_obs, truth, th


# ---- structureless problems: matrices in which every 128 x 128 block matters ------------------------------------------------
# Matern-built C^-1, m, K^-1 are numerically banded (entries at lag >= 32 are <= 1e-8 of the largest one), so a comparison on them sees the
# diagonal operator blocks and their neighbours only (tests/test_structureless_cpu.py measures it).  Users may upload any matrices
# (magi_set_matrices; the reference lets them overwrite the attributes): the fixture below has i.i.d. entries instead.

STRUCTURELESS_BOX = {"seir3": (0.05, 0.3), "seir4": (0.05, 0.3), "sirw": (0.05, 0.3), "seir_seasonal": (0.05, 0.3),
                     "hill_pow": (0.5, 1.5)}                                                       # drift -> (low, high) of every component; others (0.1, 0.9)
STRUCTURELESS_THETA = {"seir3": [6.0, 0.6, 1.8], "seir4": [6.0, 0.6, 1.8], "sirw": [2.0, 0.5, 0.3, 1.0, 0.2], "seir_seasonal": [6.0, 0.6, 1.8, 0.4],
                       "ptrans": [0.07, 0.6, 0.05, 0.3, 0.017, 0.3],
                       # magi_v2_amd.drift_examples.EDGE_EXAMPLES (tests/test_drift_edges_*.py): no two parameters of a drift alike
                       "logistic1": [0.8, 1.3], "chain8": [0.6, 0.9, 0.5, 0.8, 0.4, 0.7, 0.55, 1.1], "cascade7": [0.6, 0.9, 0.5, 0.8, 0.4, 0.7, 0.95, 0.45],
                       "hill_pow": [1.0, 2.0, 0.8, 0.5], "mixed3": [0.7, 0.9, 0.6, 0.8, 1.1, 0.5]}       # nominal parameters; others 0.5
STRUCTURELESS_SIG_PRE = -3.0                                                                       # nominal sigma_pre of every component


def structureless_theta(drift):
    return np.asarray(STRUCTURELESS_THETA.get(drift, [0.5] * orc.DRIFTS[drift][2]), dtype=np.float64)


def structureless_problem(N, drift, seed, spd=False, band=None):
    """(orc.Problem, X[N, D]): everything from numpy.random.default_rng(seed), no golden file.

    Matrices: C^-1, m, K^-1 [D, N, N] with i.i.d. N(0, 1/N) entries, non-symmetric on purpose; ``spd``: C^-1 and K^-1 are A A^T + I/2 with
    the same kind of A (a proper density for the sampler, its far blocks as large as its near ones).  ``band``: the Problem holds the
    reference's band_part(., b, b) of them and ``pr.unmasked`` the three full stacks -- what the engine is given next to the bandsize
    (``engine_for(pr, band, matrices=pr.unmasked)``).
    Everything else as the other helpers build it: grid of spacing 0.025, a smooth state X inside the drift's box (STRUCTURELESS_BOX; one
    sinusoid per component), observations of it at the even grid indices with noise N(0, (0.01 range_d)^2), mu = column means of the
    interpolated observations, LB = (0.01 std_d)^2, N_ds and beta = D N / sum N_ds from the observation mask.
    Scaling: unscaled, (t1 + t2) / beta is ~ 1e-2 of |t3 + t4| and the VALUE would not see the matrices.  C^-1 and K^-1 are each multiplied by
    the factor that makes t1 / beta = t2 / beta = |t3 + t4| / 4 at (X, sigma_pre = STRUCTURELESS_SIG_PRE, theta = structureless_theta(drift)) on
    the (masked) matrices -- a negative factor flips a stack's sign, which leaves its distribution what it was (not with ``spd``, where both
    terms are positive).  tests/test_structureless_cpu.py asserts (t1 + t2) / beta >= 0.1 |t3 + t4| at the states the tests use."""
    _, D, P = orc.DRIFTS[drift]
    rng = np.random.default_rng(seed)
    I = np.arange(N) * 0.025
    lo, hi = STRUCTURELESS_BOX.get(drift, (0.1, 0.9))
    u = np.arange(N) / max(N - 1, 1)
    waves, phases = rng.integers(1, 4, D), rng.uniform(0.0, 2.0 * np.pi, D)
    X = lo + (hi - lo) * (0.5 + 0.4 * np.sin(2.0 * np.pi * waves[None, :] * u[:, None] + phases[None, :]))
    X_obs = np.full((N, D), np.nan)
    rows = np.arange(0, N, 2)
    X_obs[rows] = X[rows] + rng.normal(size=(len(rows), D)) * (0.01 * np.ptp(X, axis=0))
    N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
    beta = float(D * N / N_ds.sum())
    idx = np.where(~np.isnan(X_obs).flatten())[0]
    y = X_obs.reshape(-1)[idx]
    mu = orc.linear_interpolate(X_obs).mean(axis=0)
    LB = orc.sigma_sqs_lower_bound(X)

    def stack():
        A = rng.normal(size=(D, N, N)) / np.sqrt(N)
        return A @ np.transpose(A, (0, 2, 1)) + 0.5 * np.eye(N) if spd else A

    C_inv, m, K_inv = stack(), rng.normal(size=(D, N, N)) / np.sqrt(N), stack()
    pr = orc.Problem(I=I, mu=mu, C_inv=band_part_copy(C_inv, band), m=band_part_copy(m, band), K_inv=band_part_copy(K_inv, band), N_ds=N_ds,
                     obs_idx=idx, y=y, beta=beta, LB=LB, drift=drift, P=P)
    th_pre = np.log(np.expm1(structureless_theta(drift)))
    t1, t2, t3, t4, _, _ = orc.logpost_terms(X, np.full(D, STRUCTURELESS_SIG_PRE), th_pre, pr)
    sC, sK = 0.25 * beta * abs(t3 + t4) / t1, 0.25 * beta * abs(t3 + t4) / t2
    assert not spd or (sC > 0 and sK > 0)
    pr.C_inv *= sC
    pr.K_inv *= sK
    pr.unmasked = (C_inv * sC, m, K_inv * sK) if band is not None else (pr.C_inv, pr.m, pr.K_inv)
    return pr, X


def band_part_copy(A, b):
    """orc.band_part, always a new array (the fixture scales its stacks in place)."""
    return A.copy() if b is None else orc.band_part(A, b)


def structureless_states(pr, X, n, seed):
    """n states around the fixture's nominal one: (X[n, N, D], sigma_pre[n, D], theta_pre[n, P]) -- X + 1 % of the box of i.i.d. noise (so the
    state is no longer smooth: every grid point carries its own value), sigma_pre = -3 + 0.3 z, theta_pre = softplus^-1(theta) + 0.05 z
    (small steps: the quadratic forms of the indefinite stacks keep the sign the fixture's scaling gave them)."""
    rng = np.random.default_rng([seed, n])
    lo, hi = STRUCTURELESS_BOX.get(pr.drift, (0.1, 0.9))
    Xb = X[None] + 0.01 * (hi - lo) * rng.standard_normal((n,) + X.shape)
    sp = STRUCTURELESS_SIG_PRE + 0.3 * rng.standard_normal((n, pr.D))
    tp = np.log(np.expm1(structureless_theta(pr.drift)))[None] + 0.05 * rng.standard_normal((n, pr.P))
    return Xb, sp, tp


# ---- shuffled grids: Matern problems in which every 128 x 128 block of the FACTORS matters -----------------------------------------
# On a sorted grid the Cholesky factor of Kappa and its inverse are numerically block-bidiagonal, so the blocked factorisation, the
# triangular inverse and the fit's S^-1 are only ever seen through their diagonal blocks and first neighbours
# (tests/test_shuffled_grid_cpu.py measures it).  The same grid in shuffled order is legal input: the Matern blocks are element-wise
# functions of (I_i, I_j) -- |I_i - I_j| and the sign of I_i - I_j -- and no build or fit entry point asks for sorted times (only
# `bandsize` and the banded packing assume them).  Kappa(I[perm]) = P Kappa P^T has the eigenvalues, hence the condition number, of the
# sorted matrix, so every conditioning-limited bar of the sorted tests applies unchanged -- while its Cholesky factor fills in completely.


def shuffled_grid(N, seed, dt=0.025):
    """(I_sorted, perm): the uniform grid of spacing dt and numpy.random.default_rng(seed).permutation(N); the shuffled grid is I_sorted[perm]."""
    return np.arange(N) * dt, np.random.default_rng(seed).permutation(N)


# ---- the NUTS state machine, branch by branch -------------------------------------------------------------------------------------
# One table of sampler configurations for tests/test_sampler_branches_cpu.py (which PROVES, with the oracle's census, that every case
# takes the branches it is listed for, that a device deciding them wrongly would show, and that no decision of a case sits on a rounding
# knife-edge) and tests/test_sampler_branches_gpu.py (which runs every case on the device, draw for draw against the oracle).
#
# Every case: theta_0 = 1 and the fixture's initial state, stale cache off, chain ids BRANCH_CHAINS (the census and the claims are chain
# 20's; chain 21 is the last chain of every batch and is compared too).  `cfg`: the device's magi_sampler_cfg fields.
#
# Per case, measured on the CPU (numpy oracle; chain 20): depths of the transitions | census entries that justify the claims | largest
# numpy-vs-C-port discrepancy over chains 20 and 21 as a fraction of the GPU tolerance of the worst field (bound: 1e-2) and of `energy`
# in absolute terms.  Integer diagnostics are identical between the two CPU runs in every case.
#
#   case                depths (chain 20)             census entries behind the claims                                  worst fraction       |d energy|
#   u_last              3 1 3 5 7 7 6                 u_end(5, last) 1; max_depth(7) 1; wasted_accept(5, acc) 1           2.7e-3 log_accept    4.4e-11
#   u_early_l2          1 1 3 4 7 6 5                 u_end(2, early) 1; max_depth(7) 1                                   1.4e-4 log_accept    5.2e-12
#   u_early_l4          1 1 2 3 6 7 6                 u_end(4, early) 1; wasted_accept(5, acc) 1                          3.6e-4 target        2.3e-11
#   u_early_l3 (b = 5)  1 1 1 3 4 4 6                 u_end(3, early) 1, u_end(3, last) 1; wasted_accept(3 / 5, acc)      3.2e-6 log_accept    1.4e-12
#   u_early_l5_depth8   5 3 5 7 8 8 8                 u_end(3, early) 1, u_end(5, early) 1, u_end(7, last) 1;             5.3e-3 step_size     7.7e-10
#                                                     check(7) 2 of which 1 fails; cap 12; wasted_accept(4 / 7, acc) 3
#   depth9              7 2 7 9 7 7 7                 511 leapfrogs; check(7) 4+, check(8) 1+, none fails                 5.5e-3 step_size     3.2e-9
#   depth10_fixed_step  10 8 8 8                      1023 leapfrogs; check(7), check(8), check(9) 1; cap 12              3.6e-3 log_accept    5.4e-10
#   div_mid             1 1 1 3 1 1 1                 div(leaf 2, depth 2) 1; div_accepted 1; wasted_accept(2, acc) 1     7.2e-4 step_size     2.0e-12
#   div_mid_seir3 (b20) 1 1 1 3 1 1 1                 div(leaf 1, depth 2) 1; div_accepted 1; wasted_accept(2, acc) 1     6.3e-3 step_size     2.4e-11
#   max_depth_1         1 1 1 1 1 1 1                 max_depth(1) 5, every transition one leaf                           1.8e-3 step_size     4.6e-11
#   min_temp            2 1 2 4 5 6 5 6 6             9 transitions, 1/ln(k+2) < 0.5 from k = 6; u_end(3, early) 2,       7.1e-4 target        1.9e-11
#                                                     u_end(4, early) 1; wasted_accept(4 / 5, acc) 3
#   anneal_off          4 1 6 6 6 6 6                 beta_temp = 1                                                       7.1e-3 log_accept    1.6e-9
#   target_accept       1 1 1 5 5 5 5                 step_size leaves the 0.75 run's at transition 1                     3.1e-3 step_size     3.9e-9
#   adapt_0 / 2 / all   1.. / 4 1 6.. / 2 1 1 4 5 6 6 5   step_size: at-boundary then frozen / before, at, frozen / before    0 / 2.6e-4 / 7.0e-4  <= 3.3e-11
#   hmc_div             (L = 8)                       a step with u <= ediff rejected because -ediff >= 0.2               3.6e-3 step_size     1.3e-10
#   u_early_member2     1 1 3 4 7 6 4                 u_end(2, early) 1; max_depth(7) 1 (second member of the group)      5.5e-5 target        1.7e-11
#
# Checkpoint levels 10 and 11 stay unreached (a level-10 check needs a transition of >= 2047 leapfrogs).  NaN energies are not taken by these
# cases; DOMAIN_CASES below reach them.
#
BRANCH_CHAINS = (20, 21)

# tolerances of the device-vs-oracle comparison, (rtol, atol); X: atol = 1e-8 max|X|.  Those of
# test_deep_trees_match_oracle_draw_for_draw_in_every_kernel_family / test_chain_matches_oracle_draw_for_draw (tests/test_sampler_gpu.py).
BRANCH_TOL = {"step_size": (1e-9, 0.0), "log_accept_ratio": (1e-7, 1e-9), "target_log_prob": (1e-8, 0.0), "X": (0.0, 1e-8),
              "sig_pre": (1e-7, 1e-9), "th_pre": (1e-7, 1e-9)}
# `energy` has no earlier tolerance.  Largest |energy_numpy - energy_C| over the table (both chains): 3.9e-9 (target_accept, |energy| ~ 9.4e3);
# ENERGY_CPU_DISCREPANCY bounds it (tests/test_sampler_branches_cpu.py asserts that per case); atol = 100 x that (a third summation order, and the leapfrog amplification the
# other fields' tolerances already allow) next to rtol 1e-8.
ENERGY_CPU_DISCREPANCY = 4e-9
ENERGY_TOL = (1e-8, 100.0 * ENERGY_CPU_DISCREPANCY)


class BranchCase:
    def __init__(self, name, tag, band, seed, cfg, claims, burnin=4, results=3, variant=None, batches=(1, 2, 3)):
        self.name, self.tag, self.band, self.seed, self.cfg, self.claims = name, tag, band, seed, dict(cfg), tuple(claims)
        self.burnin, self.results, self.variant, self.batches = burnin, results, variant, tuple(batches)

    def __repr__(self):
        return self.name


_DEEP = dict(step_size=2e-3, max_tree_depth=6)
BRANCH_CASES = [
    BranchCase("u_last", "sirw_N41", None, 808, dict(step_size=2e-3, max_tree_depth=7), ('u_last_high', 'max_depth_7', 'wasted_accept')),
    BranchCase("u_early_l2", "sirw_N41", None, 808, dict(step_size=1e-2, max_tree_depth=7), ('u_early_12', 'max_depth_7'), batches=(1, 2, 3, 9)),
    BranchCase("u_early_l4", "sirw_N41", None, 5, dict(step_size=1e-2, max_tree_depth=7), ('u_early_34', 'wasted_accept')),
    BranchCase("u_early_l3", "sirw_N41", 5, 5, dict(step_size=3e-2, max_tree_depth=7), ('u_early_34', 'wasted_accept')),
    BranchCase("u_early_l5_depth8", "sirw_N41", None, 808, dict(step_size=1.2e-4, max_tree_depth=12), ('u_early_34', 'u_early_high', 'u_last_high', 'fail_ge_7', 'depth_cap_12', 'wasted_accept')),
    BranchCase("depth9", "seir4_N81", None, 17, dict(step_size=2e-4, max_tree_depth=10), ('depth_ge_9', 'checks_7_8')),
    BranchCase("depth10_fixed_step", "seir4_N81", None, 7, dict(step_size=1.6e-5, max_tree_depth=12, num_adaptation_steps=0), ('depth_ge_9', 'depth_ge_10', 'checks_7_8', 'check_9', 'depth_cap_12'), burnin=2, results=2),
    BranchCase("div_mid", "seir4_N81", None, 5, dict(step_size=3e-2, max_tree_depth=7, max_energy_diff=1.0), ('div_mid', 'div_accepted', 'wasted_accept'), batches=(1, 2, 3, 9)),
    BranchCase("div_mid_seir3", "seir3_N161", 20, 7, dict(step_size=3.75e-3, max_tree_depth=7, max_energy_diff=0.1), ('div_mid', 'div_accepted', 'wasted_accept')),
    BranchCase("max_depth_1", "seir3_N161", None, 7, dict(step_size=3e-3, max_tree_depth=1), ('max_depth_1',)),
    BranchCase("min_temp", "sirw_N41", None, 808, dict(_DEEP, step_size=2.5e-3, min_temp=0.5), ('min_temp_binds', 'u_early_34', 'wasted_accept'), burnin=5, results=4),
    BranchCase("anneal_off", "seir4_N81", None, 808, dict(_DEEP, anneal=0), ('anneal_off',)),
    BranchCase("target_accept", "seir3_N161", None, 808, dict(_DEEP, step_size=3e-3, target_accept_prob=0.6), ('target_accept_0.6',)),
    BranchCase("adapt_0", "seir3_N161", None, 808, dict(_DEEP, num_adaptation_steps=0), ('adapt_0',), burnin=5),
    BranchCase("adapt_2", "seir4_N81", None, 808, dict(_DEEP, num_adaptation_steps=2), ('adapt_2',), burnin=5),
    BranchCase("adapt_all", "sirw_N41", None, 7, dict(_DEEP, step_size=3e-3, num_adaptation_steps=20), ('adapt_all', 'wasted_accept'), burnin=5),
    BranchCase("hmc_div", "seir4_N81", None, 7, dict(step_size=2.5e-4, mode=1, hmc_leapfrogs=8, max_energy_diff=0.2), ('hmc_div_reject',), burnin=5),
    BranchCase("u_early_member2", "sirw_N41", None, 808, dict(step_size=1e-2, max_tree_depth=7), ('u_early_12', 'max_depth_7'), variant=(1.02, 1.05), batches=()),
]


def branch_case(name):
    return next(c for c in BRANCH_CASES if c.name == name)


def branch_problem(case):
    """(fixture, orc.Problem with the reference's band mask, unmasked orc.Problem) of a case; `variant` = (y factor, K^-1 factor): another
    problem of the same shape (a second member for a problem group)."""
    import dataclasses
    g = load_g4(case.tag)
    prs = [problem_from_g4(g, case.band), problem_from_g4(g, None)]
    if case.variant is not None:
        ys, ks = case.variant
        prs = [dataclasses.replace(p, y=p.y * ys, K_inv=p.K_inv * ks) for p in prs]
    return g, prs[0], prs[1]


def c_port_logpost_grad(X, sig_pre, th_pre, beta_temp, pr):
    """oracle/logpost_c.py behind the signature of orc.logpost_grad: an independent summation order of the same function."""
    from oracle import logpost_c
    lp, _, gX, gs, gt = logpost_c.logpost_grad(X, sig_pre, th_pre, beta_temp, pr)
    return lp, gX, gs, gt


def branch_oracle_kwargs(case):
    """The arguments of orc.sample_chain that restate the case's device cfg."""
    kw = dict(stale_cache=False)
    for k, v in case.cfg.items():
        if k in ("step_size", "max_tree_depth", "max_energy_diff", "target_accept_prob", "min_temp", "num_adaptation_steps"):
            kw[k] = v
        elif k == "anneal":
            kw[k] = bool(v)
        elif k == "hmc_leapfrogs":
            kw[k] = v
        elif k != "mode":
            raise KeyError(k)
    assert ("hmc_leapfrogs" in case.cfg) == (case.cfg.get("mode", 0) == 1)
    return kw


_branch_runs = {}


def branch_oracle_run(case, chain, port="numpy"):
    """(sample_chain's output, trace, census) of one chain of a case, computed once per session and shared: treat it as read-only."""
    import collections
    key = (case.name, chain, port)
    if key not in _branch_runs:
        g, pr, _ = branch_problem(case)
        trace, events = [], collections.Counter()
        out = orc.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=chain,
                               trace=trace, events=events, logpost_grad=c_port_logpost_grad if port == "c" else None,
                               **branch_oracle_kwargs(case))
        _branch_runs[key] = (out, trace, events)
    return _branch_runs[key]


def _u_end(ev, levels, last):
    return any(k[0] == "u_end" and k[1] in levels and k[2] == last for k in ev)


HIGH = range(5, 13)
# branch -> predicate(case, census of chain 20, its trace): is the branch taken?  Every key must be claimed by a case (asserted).
BRANCHES = {
    "u_early_12": lambda c, ev, tr: _u_end(ev, (1, 2), False),              # a subtree ended before its last leaf by a level-1/2 check
    "u_early_34": lambda c, ev, tr: _u_end(ev, (3, 4), False),              # ... by a level-3/4 check (levels 1, 2 passing)
    "u_early_high": lambda c, ev, tr: _u_end(ev, HIGH, False),              # ... by a level >= 5 check alone (levels 1-4 passing)
    "u_last_high": lambda c, ev, tr: _u_end(ev, HIGH, True),                # a level >= 5 check fails at the subtree's last leaf
    "depth_ge_9": lambda c, ev, tr: any(r.depth >= 9 for _, r, _ in tr),
    "depth_ge_10": lambda c, ev, tr: any(r.depth >= 10 for _, r, _ in tr),
    "checks_7_8": lambda c, ev, tr: ev[("check", 7)] > 0 and ev[("check", 8)] > 0,
    "check_9": lambda c, ev, tr: ev[("check", 9)] > 0,                      # (levels 10, 11 need 2047 leapfrogs in one transition: unreached)
    "fail_ge_7": lambda c, ev, tr: any(ev[("check_fail", k)] > 0 for k in range(7, 13)),
    "div_mid": lambda c, ev, tr: c.cfg.get("max_energy_diff", 1000.0) < 1000 and any(k[0] == "div" and k[1] > 0 and k[2] >= 2 for k in ev),
    "div_accepted": lambda c, ev, tr: ev[("div_accepted",)] > 0,
    "max_depth_7": lambda c, ev, tr: c.cfg.get("max_tree_depth") == 7 and ev[("max_depth", 7)] > 0,
    "max_depth_1": lambda c, ev, tr: c.cfg.get("max_tree_depth") == 1 and ev[("max_depth", 1)] > 0 and all(r.leapfrogs == 1 for _, r, _ in tr),
    "depth_cap_12": lambda c, ev, tr: c.cfg.get("max_tree_depth") == 12,
    "wasted_accept": lambda c, ev, tr: any(k[0] == "wasted_accept" and k[1] >= 1 and k[2] for k in ev),  # (>= 2 leaves, a proposal to keep)
    "min_temp_binds": lambda c, ev, tr: c.cfg.get("min_temp") == 0.5 and len(tr) >= 8 and 1.0 / np.log(len(tr) - 1 + 2.0) < 0.5,
    "anneal_off": lambda c, ev, tr: c.cfg.get("anneal") == 0,
    "target_accept_0.6": lambda c, ev, tr: c.cfg.get("target_accept_prob") == 0.6,
    "adapt_0": lambda c, ev, tr: c.cfg.get("num_adaptation_steps") == 0 and c.burnin >= 5,
    "adapt_2": lambda c, ev, tr: c.cfg.get("num_adaptation_steps") == 2 and c.burnin >= 5,
    "adapt_all": lambda c, ev, tr: c.cfg.get("num_adaptation_steps", -1) >= c.burnin + c.results and c.burnin >= 5,
    "hmc_div_reject": lambda c, ev, tr: c.cfg.get("mode") == 1 and any(
        r.has_divergence and not r.is_accepted and np.log1p(-orc.rng_uniform(0, k, BRANCH_CHAINS[0], orc.STREAM_MERGE, c.seed)) <= r.log_accept_ratio
        for k, r, _ in tr),                                                 # (u <= ediff <=> u <= min(ediff, 0): only divergence rejects it)
}


# ---- leaves with non-finite energies ------------------------------------------------------------------------------------------------
# A leapfrog step that leaves the domain of a square-root or logarithmic drift gives a NaN energy; TFP, the oracle and csrc/decide.h
# count such a leaf as energy -inf: it diverges and ends its sub-tree and the transition.  The two drifts of
# magi_v2_amd.drift_examples.DOMAIN_EXAMPLES reach it from theta_0 = 1 at ordinary step sizes.  Fixture and case table for
# tests/test_nonfinite_cpu.py (the proof on the oracle alone: every case takes what it claims, no leaf of a compared chain is within
# rounding of the domain's edge, no decision sits on a rounding knife-edge, a device without the NaN rule would fail) and
# tests/test_nonfinite_gpu.py (the device draw for draw against the oracle).  Everything here is CPU-only: the matrices are
# orc.build_all's, the oracle's Jacobians complex-step derivatives of the callable.

# drift -> (generating theta, x(0), T); the component whose sign decides whether a point is inside the domain is component 0 in both
DOMAIN_TRUTH = {"sqrt_outflow": (np.array([0.5, 1.0, 0.8]), [1.0, 0.2], 3.6), "gompertz": (np.array([1.0, 1.0, 0.5, 0.3]), [0.02, 0.1], 3.0)}
DOMAIN_MARGIN = 1e-6               # every entry a sqrt / log sees is at least this far from 0, as a fraction of max|X|: 100 x the X tolerance

_domain_rec = None                 # while a list: the oracle's drift appends (min of component 0, max|X|, min |component 0|) per evaluation, NaNs for a non-finite state


def _domain_oracle_drift(f_vec):
    def fn(X, th):
        X, th = np.asarray(X, dtype=np.float64), np.asarray(th, dtype=np.float64)
        if _domain_rec is not None:
            fin = bool(np.isfinite(X).all())
            _domain_rec.append((float(X[:, 0].min()) if fin else np.nan, float(np.abs(X).max()) if fin else np.nan,
                                float(np.abs(X[:, 0]).min()) if fin else np.nan))
        with np.errstate(all="ignore"):
            n, D = X.shape
            J, T = np.zeros((n, D, D)), np.zeros((n, D, len(th)))
            for k in range(D):                                                 # complex step (tests/test_drift_cpu.py), independent of sympy
                Xc = X.astype(complex); Xc[:, k] += 1e-30j
                J[:, :, k] = np.imag(f_vec(None, Xc, th.astype(complex))) / 1e-30
            for p in range(len(th)):
                tc = th.astype(complex); tc[p] += 1e-30j
                T[:, :, p] = np.imag(f_vec(None, X.astype(complex), tc)) / 1e-30
            return np.asarray(f_vec(None, X, th), dtype=np.float64), J, T
    return fn


@contextlib.contextmanager
def domain_drifts():
    """The DOMAIN_EXAMPLES drifts registered with the oracle (``orc.DRIFTS``, which ``Problem.drift`` names) for the duration only: other
    tests iterate over that table."""
    from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES
    added = {name: (_domain_oracle_drift(f_vec), D, P) for name, (f_vec, D, P) in DOMAIN_EXAMPLES.items() if name not in orc.DRIFTS}
    orc.DRIFTS.update(added)
    try:
        yield
    finally:
        for name in added:
            del orc.DRIFTS[name]


class DomainCase(BranchCase):
    """A BranchCase on a DOMAIN_EXAMPLES drift: `tag` is the drift's name; N grid points; `shift` is added to x(0) of component 0: the same system, its data
    and its initial state inside the domain's interior (the second member of a problem group)."""

    def __init__(self, name, drift, band, seed, cfg, claims, N=41, shift=0.0, **kw):
        super().__init__(name, drift, band, seed, cfg, claims, **kw)
        self.N, self.shift = N, shift


_domain_problems = {}


def domain_problem(case):
    """(fixture {"Xhat_init", "sigma_sqs_init"}, orc.Problem with the reference's band mask, unmasked orc.Problem): the recipe of
    tests/test_user_drift_gpu.py::make_problem (rk4 truth, every other grid point observed, initial hyper-parameters with phi2 = 1.5) with
    observation noise 0.01 and the oracle's own matrix build."""
    from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES, rk4
    key = (case.tag, case.N, case.band, case.shift)
    if key not in _domain_problems:
        f_vec, D, P = DOMAIN_EXAMPLES[case.tag]
        truth, x0, T = DOMAIN_TRUTH[case.tag]
        I, X = rk4(f_vec, [x0[0] + case.shift] + list(x0[1:]), truth, T, case.N)
        X_obs = X + np.random.default_rng(0).normal(0, 0.01, X.shape)
        X_obs[1::2] = np.nan
        Xi = orc.linear_interpolate(X_obs)
        hp = orc.hparams_initial(Xi)
        C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], np.full(D, 1.5), 2.01, bandsize=None)
        N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
        idx = np.where(~np.isnan(X_obs).flatten())[0]
        Xhat = orc.cubic_smoother(I, Xi)
        mk = lambda b: orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=band_part_copy(C_inv, b), m=band_part_copy(m, b), K_inv=band_part_copy(K_inv, b),
                                   N_ds=N_ds, obs_idx=idx, y=X_obs.reshape(-1)[idx], beta=float(D * case.N / N_ds.sum()),
                                   LB=orc.sigma_sqs_lower_bound(Xhat), drift=case.tag, P=P)
        _domain_problems[key] = ({"Xhat_init": Xhat, "sigma_sqs_init": hp["sigma_sqs"]}, mk(case.band), mk(None))
    return _domain_problems[key]


class Census(dict):
    """The counter orc.nuts_one_step fills, which also keeps the order of its increments: ``log`` = [(key, drift evaluations so far)]."""

    def __init__(self, clock):
        super().__init__()
        self.log, self.clock = [], clock

    def __missing__(self, key):
        return 0

    def __setitem__(self, key, value):
        self.log.append((key, self.clock()))
        super().__setitem__(key, value)


class DomainRun:
    """One oracle chain of a case: ``out`` (sample_chain's), ``trace``, ``events`` (the census), ``evals`` (one record per drift evaluation:
    min of component 0, max|X|, min|component 0|; NaN for a non-finite state) and, from the census' log,
    ``nan_leaves`` = [(transition, leaf index in its sub-tree, sub-tree depth)] and ``ordinary`` = the same for divergent leaves of finite energy
    (NUTS only: fixed-L HMC has no census)."""

    def __init__(self, out, trace, events, evals, hmc):
        self.out, self.trace, self.events, self.evals = out, trace, events, evals
        ends = 1 + np.cumsum([r.leapfrogs for _, r, _ in trace])               # (evaluation 0 is the initial state's)
        self.first_eval = np.concatenate([[1], ends[:-1]])
        self.nan_leaves, self.ordinary, self.wasted = [], [], []
        where = lambda clock: int(np.searchsorted(ends, clock, side="left"))     # the transition whose leaf was evaluation number clock - 1
        pending = False
        for key, clock in events.log:
            if key == ("nan",):
                pending = True
            elif key[0] == "div":
                (self.nan_leaves if pending else self.ordinary).append((where(clock), key[1], key[2]))
                pending = False
            elif key[0] == "wasted_accept":
                self.wasted.append((where(clock), key[1], key[2]))
        assert hmc or len(self.nan_leaves) == events[("nan",)]

    def nan_transitions(self):
        return sorted({k for k, _, _ in self.nan_leaves})

    def outside(self, k):
        """Leaves of transition k (in evaluation order) whose state is outside the domain or non-finite."""
        a = self.first_eval[k]
        return [j for j in range(self.trace[k][1].leapfrogs) if not self.evals[a + j][0] > 0.0]


_domain_runs = {}


def domain_oracle_run(case, chain, logpost_grad=None, cache=True, **over):
    """DomainRun of one chain of a case, computed once per session and shared (read-only).  ``logpost_grad`` / ``over``: another log
    posterior / other sample_chain arguments (not cached)."""
    global _domain_rec
    key = (case.name, chain)
    if not cache or logpost_grad is not None or over or key not in _domain_runs:
        fx, pr, _ = domain_problem(case)
        trace, evals = [], []
        events = Census(lambda: len(evals))
        _domain_rec = evals
        try:
            with domain_drifts():
                out = orc.sample_chain(pr, fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=chain,
                                       trace=trace, events=events, logpost_grad=logpost_grad, **dict(branch_oracle_kwargs(case), **over))
        finally:
            _domain_rec = None
        run = DomainRun(out, trace, events, evals, "hmc_leapfrogs" in case.cfg)
        if logpost_grad is not None or over or not cache:
            return run
        _domain_runs[key] = run
    return _domain_runs[key]


def _nan_tr(run, k):
    r = run.trace[k][1]
    return r.has_divergence and r.log_accept_ratio == -np.inf


# claim -> predicate(case, {chain: DomainRun}): does the case take it?  NUTS claims are read off the census of chain 20 unless they say otherwise.
DOMAIN_BRANCHES = {
    # the first leaf of a transition is NaN: one leapfrog, log_accept_ratio = -inf, not accepted, has_divergence
    "nan_first_leaf": lambda c, runs: any(
        (it, d) == (0, 0) and runs[20].trace[k][1].leapfrogs == 1 and _nan_tr(runs[20], k) and not runs[20].trace[k][1].is_accepted
        for k, it, d in runs[20].nan_leaves),
    # a NaN leaf at index >= 1 of a sub-tree of depth >= 2 in a transition that had accepted a proposal, which survives
    "nan_mid_subtree": lambda c, runs: any(
        it >= 1 and d >= 2 and runs[20].trace[k][1].is_accepted and runs[20].trace[k][1].has_divergence and (k, d, True) in runs[20].wasted
        for k, it, d in runs[20].nan_leaves) and runs[20].events[("div_accepted",)] > 0,
    "nan_last_leaf": lambda c, runs: any(d >= 1 and it == (1 << d) - 1 for k, it, d in runs[20].nan_leaves),
    # >= 2 accepted transitions after the run's last NaN transition
    "recovers": lambda c, runs: bool(runs[20].nan_leaves) and sum(
        int(r.is_accepted) for k, r, _ in runs[20].trace if k > runs[20].nan_transitions()[-1]) >= 2,
    # a transition index at which chain 20 takes a NaN leaf and chain 21 does not, and one the other way round
    "one_of_the_batch": lambda c, runs: bool(set(runs[20].nan_transitions()) - set(runs[21].nan_transitions()))
    and bool(set(runs[21].nan_transitions()) - set(runs[20].nan_transitions())),
    # adaptation on: the step size falls after a -inf ratio
    "adapts": lambda c, runs: "num_adaptation_steps" not in c.cfg and any(
        k + 1 < min(int(0.8 * c.burnin), len(runs[20].trace)) and runs[20].trace[k][1].log_accept_ratio == -np.inf
        and runs[20].trace[k + 1][2] < runs[20].trace[k][2] for k in runs[20].nan_transitions()),
    # fixed-L HMC whose trajectory leaves the domain before its last leaf: rejected, has_divergence, log_accept_ratio = -inf
    "hmc_nan": lambda c, runs: c.cfg.get("mode") == 1 and c.cfg.get("hmc_leapfrogs") == 8 and any(
        run.outside(k) and run.outside(k)[0] < 7 and not r.is_accepted and r.has_divergence and r.log_accept_ratio == -np.inf
        for run in (runs[20],) for k, r, _ in run.trace),
    # an ordinary divergence, of finite energy
    "ordinary_div": lambda c, runs: bool(runs[20].ordinary),
    "two_operator_blocks": lambda c, runs: c.N == 161 and c.band == 20 and bool(runs[20].nan_leaves),
    "interior": lambda c, runs: c.shift > 0 and all(not runs[ch].nan_leaves and all(e[0] >= 0.3 for e in runs[ch].evals) for ch in BRANCH_CHAINS),
}

# Every case: theta_0 = 1, 6 burn-in + 4 kept transitions, stale cache off, chains BRANCH_CHAINS.  Measured on the CPU (chain 20 | chain 21): NaN leaves as
# (transition, leaf index in its sub-tree, sub-tree depth) | smallest |argument of sqrt / log| / max|X| over all evaluated states (bound DOMAIN_MARGIN)
# | float64 vs long-double operator products, worst fraction of the device tolerance (bound 1e-2) | device vs oracle on an MI355X, the same fraction.
#
#   case                 NaN leaves, chain 20 | chain 21                              margin    CPU vs CPU            device vs oracle
#   sqrt_deep            (1, 0, 0) (7, 13, 4) | (1, 0, 0)                             1.5e-4    9.0e-4 log_accept     1.4e-3 log_accept
#   sqrt_last_leaf       (7, 3, 2) (9, 0, 2) | (2, 0, 3) (8, 0, 0) (9, 0, 0)          1.6e-4    2.4e-3 step_size      5.2e-3 step_size
#   gompertz_first_leaf  (0, 0, 0) (1, 0, 0) (2, 0, 0) | the same                     2.7e-4    2.9e-6 log_accept     3.5e-6 log_accept
#   sqrt_hmc             outside from leaf 1 or 2 of 8 in transitions 0, 1, 4, 9      1.2e-5    3.2e-6 target         1.8e-5 target
#   gompertz_hmc         outside from leaf 0 or 2 of 8 in transitions 0, 1, 2         4.4e-5    6.0e-6 target         1.3e-5 target
#   sqrt_n161 (b = 20)   (0, 0, 0) (1, 0, 0) (2, 0, 0) | the same                     2.7e-5    2.6e-4 log_accept     4.0e-4 log_accept
#   sqrt_interior        none (every evaluated x >= 0.3; second member of the group)  2.1e-1    1.8e-3 target         9.5e-3 target (group)
#
# In every case and on every kernel the device has every integer diagnostic and every -inf of log_accept_ratio where the oracle has them.
_D6 = dict(max_tree_depth=6)
_HMC8 = dict(mode=1, hmc_leapfrogs=8)
DOMAIN_CASES = [
    DomainCase("sqrt_deep", "sqrt_outflow", None, 6, dict(_D6, step_size=1e-3),
               ("nan_first_leaf", "nan_mid_subtree", "recovers", "adapts", "ordinary_div"), burnin=6, results=4, batches=(1, 2, 3, 9)),
    DomainCase("sqrt_last_leaf", "sqrt_outflow", None, 808, dict(_D6, step_size=3e-3),
               ("nan_mid_subtree", "nan_last_leaf", "one_of_the_batch", "ordinary_div"), burnin=6, results=4),
    DomainCase("gompertz_first_leaf", "gompertz", None, 808, dict(_D6, step_size=3e-2),
               ("nan_first_leaf", "recovers", "adapts", "ordinary_div"), burnin=6, results=4, batches=(1, 2, 3, 9)),
    DomainCase("sqrt_hmc", "sqrt_outflow", None, 808, dict(_HMC8, step_size=3e-3), ("hmc_nan",), burnin=6, results=4, batches=(1, 3)),
    DomainCase("gompertz_hmc", "gompertz", None, 808, dict(_HMC8, step_size=3e-3), ("hmc_nan",), burnin=6, results=4, batches=(1, 3)),
    DomainCase("sqrt_n161", "sqrt_outflow", 20, 808, dict(_D6, step_size=3e-3),
               ("nan_first_leaf", "recovers", "adapts", "ordinary_div", "two_operator_blocks"), N=161, burnin=6, results=4, batches=(1, 3)),
    DomainCase("sqrt_interior", "sqrt_outflow", None, 6, dict(_D6, step_size=1e-3), ("interior",), shift=3.0, burnin=6, results=4, batches=()),
]


def domain_case(name):
    return next(c for c in DOMAIN_CASES if c.name == name)


# ---- one handle through many states ---------------------------------------------------------------------------------------------------
# The drivers keep one handle alive and move it through states (new band, new shape, new data, new drift, new batch, a sampler after a
# sampler, the instruments of bench.py); every other GPU comparison builds a fresh handle per state.  Case tables of
# tests/test_reuse_cpu.py (the proof, on the oracle alone, that a stale answer would be seen and that every history passes through the
# kernel families and storage modes it names) and tests/test_reuse_gpu.py (the re-used handle against a fresh one bit for bit, the fresh
# one against the oracle).
#
# States (ReuseState): "A" = structureless_problem(384, "sirw", spd=True) -- three block rows, three basis functions; "A/b<k>": A's matrices
# under the band mask k; "B": the same shape from another seed; "A+B": B's data on A's matrices; "E" = the seir4 fixture of that N;
# "A+E": E's data and drift on A's matrices (P = 3 against 5: dimp changes); "C41" / "C161": g4_logpost_sirw_N41 / g4_logpost_seir3_N161;
# "T" / "T+0.37": seir_seasonal at N = 41 on oracle-built matrices, the drift evaluated at the grid / at the grid + 0.37.

REUSE_TB = 128                                              # edge of an operator block (csrc/magi_internal.h: MAGI_TB)
REUSE_N = 384
REUSE_BANDS = (None, 20, 0, 43, None, 20)                   # transition 1: dense -> 20 -> 0 -> 43 -> dense -> 20
REUSE_SHAPES = ("A", "C41", "C161", "A")                    # transition 2
REUSE_DATA = ("A", "A+B", "A", "A+E", "A")                  # transition 3: other data, back, other drift (P 5 -> 3), back
# transition 4: (batch, option stream_family set on the live handle, the kernel that then serves the batch)
REUSE_BATCHES = ((9, "mc", "k_stream_sep<CW=16>"), (2, "auto", "k_stream<2>"), (16, "auto", "k_stream_sep<CW=16>"),
                 (8, "auto", "k_stream_sep<CW=8>"), (1, "valu", "k_stream<1>"), (3, "mc", "k_stream_sep<CW=8>"),
                 (17, "auto", "k_stream_sep<CW=16>"))
REUSE_BYTES = (("A", None), ("A", 20), ("A", 43), ("A", 0), ("C161", 20))   # transition 7: (state, band); at band 0 only "none missing"
REUSE_TIME_SHIFT = 0.37
REUSE_NUTS = dict(num_burnin_steps=4, num_results=3, step_size=2e-3, max_tree_depth=6, stale_cache=0)
REUSE_HMC = dict(num_burnin_steps=3, num_results=2, step_size=2e-3, mode=1, hmc_leapfrogs=8, stale_cache=0)
REUSE_GROW = dict(REUSE_NUTS, num_burnin_steps=8, num_results=6)      # the run that sizes the grow-only output buffers: 3 chains, to its end
REUSE_SEED = 808


def reuse_band_tables(N, band):
    """What csrc/pack.hip derives from (N, band), restated from its comments: (three-phase storage banded?, W, fb, wb, nb) -- banded rows of
    W = 2 b + 1 columns when 2 b + 1 < N; the single-phase operators have band fb = 3 b when 6 b + 1 < N (else dense, fb = -1); a block is
    kept when |bi - bj| <= wb = min(nb, (max(fb, 1) - 1) / TB + 1), every block when fb < 0."""
    nb = (N + REUSE_TB - 1) // REUSE_TB
    banded = band is not None and 2 * band + 1 < N
    fb = 3 * band if band is not None and 6 * band + 1 < N else -1
    wb = nb if fb < 0 else min(nb, (max(fb, 1) - 1) // REUSE_TB + 1)
    return banded, (2 * band + 1 if banded else N), fb, wb, nb


def reuse_block_counts(N, D, band):
    """(independent count, the library's count) of 128 x 128 operator blocks.  Independent: the masked index set {|i - j| <= fb} (all pairs
    when the single-phase operators are dense) built in numpy, the blocks that hold at least one of its entries counted -- lower block
    triangle for FH and FK, all blocks for FE.  The library's: |bi - bj| <= wb over the same triangles."""
    _, _, fb, wb, nb = reuse_band_tables(N, band)
    i = np.arange(N)
    inside = np.ones((N, N), dtype=bool) if fb < 0 else np.abs(i[:, None] - i[None, :]) <= fb
    pad = np.zeros((nb * REUSE_TB, nb * REUSE_TB), dtype=bool)
    pad[:N, :N] = inside
    hit = pad.reshape(nb, REUSE_TB, nb, REUSE_TB).any(axis=(1, 3))
    lower = np.tril(np.ones((nb, nb), dtype=bool))
    bi = np.arange(nb)
    kept = np.abs(bi[:, None] - bi[None, :]) <= wb
    count = lambda keep: D * (2 * int((keep & lower).sum()) + int(keep.sum()))
    assert not (hit & ~kept).any()                           # the library never drops a block the mask leaves an entry in
    return count(hit), count(kept)


def reuse_auto_kernel(n_tasks, n, family, separable=True):
    """The streaming kernel of a batch of n chains as tests/conftest.py documents the rule: "mc" -> the matrix-core kernel; "valu" ->
    k_stream<1> / <2>; "auto" -> matrix cores from three chains up when blocks x chain pairs > 320.  Separable drifts (all built-in ones,
    seir_seasonal) take k_stream_sep with the 8-column mirror up to 8 chains, the 16-column one beyond."""
    mc = family == "mc" or (family == "auto" and n >= 3 and n_tasks * ((n + 1) // 2) > 320)
    if not mc:
        return "k_stream<2>" if n >= 2 else "k_stream<1>"
    return "k_stream_mc" if not separable else "k_stream_sep<CW=8>" if n <= 8 else "k_stream_sep<CW=16>"


class ReuseState:
    """One state of a handle: ``pr`` the oracle's problem (band mask applied), ``matrices`` the unmasked stacks the engine is given next to
    ``band``, ``drift`` a traced Drift or None, ``times`` what set_times gets (traced drifts), ``batch`` = (X[17, N, D], sig_pre[17, D],
    th_pre[17, P]): pre-transformed states, no two alike; a batch of n evaluates / starts its chains at the first n, chain k with id 20 + k."""

    def __init__(self, name, pr, matrices, band, batch, drift=None, times=None):
        self.name, self.pr, self.matrices, self.band, self.batch, self.drift, self.times = name, pr, matrices, band, batch, drift, times

    def states(self, n):
        return tuple(a[:n] for a in self.batch)

    def __repr__(self):
        return self.name


_reuse_states = {}
REUSE_MAX_BATCH = 17


def _reuse_batch_around(X0, s0, t0, seed):
    """17 states around (X0, sig_pre0, th_pre0): X + 1e-3 max|X| z, sig_pre + 0.1 z, th_pre + 0.05 z."""
    rng = np.random.default_rng(seed)
    n = REUSE_MAX_BATCH
    return (X0[None] + 1e-3 * np.abs(X0).max() * rng.standard_normal((n,) + X0.shape), s0[None] + 0.1 * rng.standard_normal((n, len(s0))),
            t0[None] + 0.05 * rng.standard_normal((n, len(t0))))


def reuse_state(name):
    """The ReuseState of a name of the table above; built once per session and shared: read-only."""
    import dataclasses
    if name in _reuse_states:
        return _reuse_states[name]
    from tests.test_structureless_cpu import fixture
    base, _, band = name.partition("/b")
    if band:
        a, b = reuse_state(base), int(band)
        pr = dataclasses.replace(a.pr, C_inv=orc.band_part(a.pr.C_inv, b), m=orc.band_part(a.pr.m, b), K_inv=orc.band_part(a.pr.K_inv, b))
        st = ReuseState(name, pr, a.matrices, b, a.batch, a.drift, a.times)
    elif name in ("A", "B", "E"):
        pr, X = fixture(REUSE_N, "seir4" if name == "E" else "sirw", spd=True, salt=1 if name == "B" else 0)
        st = ReuseState(name, pr, (pr.C_inv, pr.m, pr.K_inv), None, structureless_states(pr, X, REUSE_MAX_BATCH, 0))
    elif name in ("A+B", "A+E"):
        a, o = reuse_state("A"), reuse_state(name[2:])
        pr = dataclasses.replace(o.pr, C_inv=a.pr.C_inv, m=a.pr.m, K_inv=a.pr.K_inv)
        st = ReuseState(name, pr, a.matrices, None, o.batch)
    elif name in ("C41", "C161"):
        g = load_g4("sirw_N41" if name == "C41" else "seir3_N161")
        pr = problem_from_g4(g, None)
        st = ReuseState(name, pr, (pr.C_inv, pr.m, pr.K_inv), None,
                        _reuse_batch_around(g["state_X"][1], g["state_sig_pre"][1], g["state_th_pre"][1], len(pr.I)))
    elif name == "C41*":                                                   # other data on C41's matrices (a group member changed later)
        a = reuse_state("C41")
        st = ReuseState(name, dataclasses.replace(a.pr, y=a.pr.y * 1.02, mu=a.pr.mu * 1.01), a.matrices, None, a.batch)
    elif name in ("T", "T+0.37"):
        from magi_v2_amd import drift as drift_mod
        from magi_v2_amd.drift_examples import TIME_EXAMPLES
        from tests.test_time_drift_cpu import fixture_data, oracle_drift_at
        f_vec, D, P = TIME_EXAMPLES["seir_seasonal"]
        I, X, X_obs, truth, phi2 = fixture_data("seir_seasonal")
        times = I + (REUSE_TIME_SHIFT if name != "T" else 0.0)
        oname = "seir_seasonal@reuse" + name[1:]                       # (in the oracle's drift table only inside reuse_oracle_logpost)
        Xi = orc.linear_interpolate(X_obs)
        hp = orc.hparams_initial(Xi)
        C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], np.full(D, phi2), 2.01, bandsize=None)
        N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
        idx = np.where(~np.isnan(X_obs).flatten())[0]
        Xhat = orc.cubic_smoother(I, Xi)
        LB = orc.sigma_sqs_lower_bound(Xhat)
        pr = orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=C_inv, m=m, K_inv=K_inv, N_ds=N_ds, obs_idx=idx, y=X_obs.reshape(-1)[idx],
                         beta=float(D * len(I) / N_ds.sum()), LB=LB, drift=oname, P=P)
        X0, s0, t0 = orc.initial_state(Xhat, hp["sigma_sqs"], truth, LB)
        st = ReuseState(name, pr, (C_inv, m, K_inv), None, _reuse_batch_around(X0, s0, t0, 41), drift_mod.resolve(f_vec, D, P), times)
        st.oracle_entry = (oracle_drift_at(f_vec, times), D, P)
    else:
        raise KeyError(name)
    _reuse_states[name] = st
    return st


def reuse_band_state(band):
    return reuse_state("A" if band is None else f"A/b{band}")


def reuse_oracle_logpost(st, X, sp, tp, temp):
    """orc.logpost_grad of a ReuseState; the drift-table entry of a traced state is registered for the call only (other tests iterate
    over that table)."""
    entry = getattr(st, "oracle_entry", None)
    if entry is None:
        return orc.logpost_grad(X, sp, tp, temp, st.pr)
    orc.DRIFTS[st.pr.drift] = entry
    try:
        return orc.logpost_grad(X, sp, tp, temp, st.pr)
    finally:
        del orc.DRIFTS[st.pr.drift]
