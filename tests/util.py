"""Shared helpers for the tests (oracle side only; product code never imports this)."""
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

STRUCTURELESS_BOX = {"seir3": (0.05, 0.3), "seir4": (0.05, 0.3), "sirw": (0.05, 0.3), "seir_seasonal": (0.05, 0.3)}   # drift -> (low, high) of every component; others (0.1, 0.9)
STRUCTURELESS_THETA = {"seir3": [6.0, 0.6, 1.8], "seir4": [6.0, 0.6, 1.8], "sirw": [2.0, 0.5, 0.3, 1.0, 0.2], "seir_seasonal": [6.0, 0.6, 1.8, 0.4],
                       "ptrans": [0.07, 0.6, 0.05, 0.3, 0.017, 0.3]}                               # nominal parameters; others 0.5
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
