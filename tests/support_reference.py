"""Reference of the per-parameter supports of theta (include/magi_hip.h: magi_set_theta_support).

``logpost_grad_supported(kinds, bounds)`` restates ``orc.logpost_grad`` with the table

    kind        theta(pre)           d theta / d pre   log-Jacobian term     its derivative
    positive    softplus(pre)        sg                pre - softplus(pre)   1 - sg
    lower lo    lo + softplus(pre)   sg                pre - softplus(pre)   1 - sg
    upper hi    hi - softplus(pre)   -sg               pre - softplus(pre)   1 - sg
    real        pre                  1                 0                     0

in the oracle's own order of operations: with every parameter positive the two agree bit for bit (tests/test_support_cpu.py).  It drives
``orc.sample_chain(logpost_grad=...)`` / ``tests.metric_reference.sample_chain(initial=..., logpost_grad=...)``: the oracle's NUTS / HMC
transition acts on ``pre`` and needs no change.  ``fault`` restates what a device that got one row wrong would compute -- the
sensitivity cases of tests/test_support_cpu.py."""
import contextlib
import functools

import numpy as np

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M

POSITIVE, LOWER, UPPER, REAL = host.THETA_POSITIVE, host.THETA_LOWER, host.THETA_UPPER, host.THETA_REAL
FAULTS = ("ignored", "upper_sign", "real_jacobian")      # all-positive on the same pre; d theta / d pre = +sg for upper; 1 - sg kept for real


def logpost_grad_supported(kinds, bounds, fault=None):
    """A function with the signature of ``orc.logpost_grad`` under the supports (kinds, bounds) of host.theta_support."""
    kinds, bounds = np.asarray(kinds), np.asarray(bounds, dtype=np.float64)
    if fault == "ignored":
        kinds, bounds = np.zeros_like(kinds), np.zeros_like(bounds)
    real, upper, lower = kinds == REAL, kinds == UPPER, kinds == LOWER

    def fn(X, sig_pre, th_pre, beta_temp, pr):
        D = pr.D
        sp_s = np.log(1.0 + np.exp(sig_pre))
        sigma_sqs = sp_s + pr.LB
        with np.errstate(over="ignore", invalid="ignore"):
            sp_t = np.log(1.0 + np.exp(th_pre))
            sg_t = 1.0 / (1.0 + np.exp(-th_pre))
        thetas = np.where(real, th_pre, np.where(upper, bounds - sp_t, np.where(lower, bounds + sp_t, sp_t)))
        dth_dpre = np.where(real, 1.0, np.where(upper & (fault != "upper_sign"), -sg_t, sg_t))
        ljd_t = np.where(real & (fault not in ("real_jacobian", "real_jacobian_full")), 0.0, 1.0 - sg_t)
        sg_s = 1.0 / (1.0 + np.exp(-sig_pre))
        lj_s = np.sum(sig_pre - sp_s)
        lj_t = np.sum(np.where(real & (fault != "real_jacobian_full"), 0.0, th_pre - sp_t))

        xc = (X - pr.mu).T[:, :, None]
        Cx = pr.C_inv @ xc
        CTx = np.transpose(pr.C_inv, (0, 2, 1)) @ xc
        t1 = np.sum(xc * Cx)
        f, J, T = orc.DRIFTS[pr.drift][0](X, thetas)
        r = f.T[:, :, None] - (pr.m @ xc)
        Kr = pr.K_inv @ r
        KTr = np.transpose(pr.K_inv, (0, 2, 1)) @ r
        t2 = np.sum(r * Kr)
        g = (Kr + KTr)[:, :, 0]
        t3 = np.sum(pr.N_ds * np.log(2.0 * np.pi * sigma_sqs))
        cols = pr.obs_idx % D
        resid = X.reshape(-1)[pr.obs_idx] - pr.y
        t4 = np.sum(np.square(resid) * (1.0 / sigma_sqs)[cols])
        logp = beta_temp * (-0.5 * (((1.0 / pr.beta) * (t1 + t2)) + (t3 + t4)) + lj_s + lj_t)

        mTg = (np.transpose(pr.m, (0, 2, 1)) @ g[:, :, None])[:, :, 0]
        d12 = (Cx + CTx)[:, :, 0] - mTg + np.einsum("dn,nde->en", g, J)
        d4 = np.zeros(X.size)
        np.add.at(d4, pr.obs_idx, 2.0 * resid / sigma_sqs[cols])
        gX = beta_temp * (-0.5 * ((1.0 / pr.beta) * d12.T + d4.reshape(X.shape)))
        SS = np.zeros(D)
        np.add.at(SS, cols, np.square(resid))
        dsig = pr.N_ds / sigma_sqs - SS / sigma_sqs ** 2
        gsig = beta_temp * (-0.5 * dsig * sg_s + (1.0 - sg_s))
        dth = np.einsum("dn,ndp->p", g, T)
        gth = beta_temp * (-0.5 * (1.0 / pr.beta) * dth * dth_dpre + ljd_t)
        return logp, gX, gsig, gth
    return fn


# ---- the sampler cases of tests/test_support_gpu.py; tests/test_support_cpu.py holds each to the sensitivity conditions --------------------------

SPEC_N41 = ["real", ("lower", 0.5), ("upper", 3.0)]
THETA0_N41 = np.array([-0.4, 1.0, 1.0])
_NUTS7 = dict(step_size=1e-2, max_tree_depth=7, stale_cache=0)
_ALL = ((1, "auto"), (2, "auto"), (3, "mc"), (9, "mc"))          # k_stream<1>, k_stream<2>, k_stream_sep<8>, k_stream_sep<16>


class SupportCase(M.MetricCase):
    """A row of tests.metric_reference's kind with the parameters' supports and their starting values on the natural scale."""

    def __init__(self, name, kind, N, band, cfg, runs, spec, theta0, **kw):
        super().__init__(name, kind, N, band, cfg, runs, **kw)
        self.spec, self.theta0 = list(spec), theta0          # (theta0: values, or a callable that gives them)


_NUTS6 = dict(step_size=2e-3, max_tree_depth=6, stale_cache=0)


def _nominal(drift, negate=()):
    """The structureless fixture's nominal parameters of a drift, the entries ``negate`` negated (resolved by case_init: the drift's oracle
    entry is registered by then)."""
    def theta0():
        from tests.util import structureless_theta
        th = np.array(structureless_theta(drift), dtype=np.float64)
        th[list(negate)] *= -1.0
        return th
    return theta0


CASES = [
    # 4 + 4 transitions.  The first seven have the reference leapfrogs [2, 1, 63, 127, 127, 63, 127] (chain 20) and [3, 1, 63, 127, 127, 127, 127]
    # (chain 21), the two leading ones diverge; the eighth is there because a Jacobian derivative kept for the real parameter first shows in
    # an integer diagnostic of chain 21 in transition 7 (chains 20, 22, 28: transitions 5, 6, 3) -- tests/test_support_cpu.py
    SupportCase("nuts_n41", "seir", 41, None, _NUTS7, _ALL, SPEC_N41, THETA0_N41, dt=0.1, results=4),
    # (Philox seeds, step sizes and transition counts of the rows below: the first of those tried at which every fault of
    #  tests/test_support_cpu.py shows in an integer diagnostic of every compared chain -- chosen on the reference alone)
    SupportCase("nuts_n41_stale", "seir", 41, None, dict(_NUTS7, stale_cache=1), ((1, "auto"),), SPEC_N41, THETA0_N41, dt=0.1, seed=809),
    # (fixed-L HMC has one integer diagnostic that can move, is_accepted, and the Jacobian derivative kept for the real parameter moves the
    #  energy error by little: seeds 808 .. 862 leave one of the two chains blind to it over 16 transitions; under 863 transition 13 shows it)
    SupportCase("hmc_n41", "seir", 41, None, dict(step_size=1e-2, mode=1, hmc_leapfrogs=8, stale_cache=0), ((1, "auto"), (3, "mc")), SPEC_N41, THETA0_N41, dt=0.1,
                seed=863, results=12),
    SupportCase("nuts_n161_b20", "seir", 161, 20, _NUTS7, ((1, "auto"), (3, "mc")), SPEC_N41, THETA0_N41, seed=4, results=4),
    # not separable: k_stream_mc.  Bounds one unit / one half away from the nominal value
    SupportCase("nuts_ptrans_n41", "traced", 41, None, _NUTS6, ((3, "mc"),),
                ["positive", "real", ("upper", 1.0), ("lower", 0.01), "real", "positive"], _nominal("ptrans"), drift="ptrans"),
    # time-dependent: the forcing amplitude A is real and starts negative
    SupportCase("nuts_fhn_forced_n41", "time", 41, None, _NUTS6, ((1, "auto"), (3, "mc")),
                ["positive", ("lower", 0.05), ("upper", 5.0), "real"], [0.2, 0.2, 3.0, -0.5], drift="fhn_forced", results=12),
]


def case(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def case_support(name):
    c = case(name)
    return host.theta_support(c.spec, len(c.spec))


@functools.lru_cache(maxsize=None)
def _fhn_problem():
    """The forced FitzHugh-Nagumo fixture of tests/test_time_drift_cpu.py (non-uniform grid, every second row unobserved) with the
    oracle's own matrix build: (orc.Problem, (X0, sig_pre0, th_pre0 at the generating parameters), traced Drift)."""
    from magi_v2_amd import drift as drift_mod
    from magi_v2_amd.drift_examples import TIME_EXAMPLES
    from tests.test_time_drift_cpu import fixture_data
    f_vec, D, P = TIME_EXAMPLES["fhn_forced"]
    I, _, X_obs, truth, phi2 = fixture_data("fhn_forced")
    Xi = orc.linear_interpolate(X_obs)
    hp = orc.hparams_initial(Xi)
    C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], np.full(D, phi2), 2.01, bandsize=None)
    N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
    idx = np.where(~np.isnan(X_obs).flatten())[0]
    Xhat = orc.cubic_smoother(I, Xi)
    pr = orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=C_inv, m=m, K_inv=K_inv, N_ds=N_ds, obs_idx=idx, y=X_obs.reshape(-1)[idx],
                     beta=float(D * len(I) / N_ds.sum()), LB=orc.sigma_sqs_lower_bound(Xhat), drift="fhn_forced", P=P)
    return pr, orc.initial_state(Xhat, hp["sigma_sqs"], truth, pr.LB), drift_mod.resolve(f_vec, D, P)


def case_problem(c):
    """``tests.metric_reference.case_problem`` with the kind "time": the forced FitzHugh-Nagumo fixture above."""
    if c.kind == "time":
        pr, init, d = _fhn_problem()
        return pr, pr, init, d
    return M.case_problem(c)


@contextlib.contextmanager
def oracle_drifts(c):
    """The oracle's drift-table entry of a case's traced drift, for the duration."""
    if c.kind == "time":
        from magi_v2_amd.drift_examples import TIME_EXAMPLES
        from tests.test_time_drift_cpu import oracle_drift_at
        f_vec, D, P = TIME_EXAMPLES[c.drift]
        had = orc.DRIFTS.get(c.drift)
        orc.DRIFTS[c.drift] = (oracle_drift_at(f_vec, _fhn_problem()[0].I), D, P)
        try:
            yield
        finally:
            if had is None:
                del orc.DRIFTS[c.drift]
            else:
                orc.DRIFTS[c.drift] = had
    else:
        with M.oracle_drifts(c):
            yield


def case_init(c):
    """(X0, sig_pre0, th_pre0) of a case: the problem's own X and sigma, theta0 through host.theta_pre_inits."""
    X0, s0, _ = case_problem(c)[2]
    with oracle_drifts(c):
        th0 = np.asarray(c.theta0() if callable(c.theta0) else c.theta0, dtype=np.float64)
    return X0, s0, host.theta_pre_inits(th0, *case_support(c.name))


_runs = {}


def case_run(c, chain, fault=None):
    """(sample_chain's output, trace) of one chain of a case under its supports (``fault``: as logpost_grad_supported); once per session."""
    key = (c.name, chain, fault)
    if key not in _runs:
        pr = case_problem(c)[0]
        trace = []
        lg = logpost_grad_supported(*case_support(c.name), fault=fault)
        with oracle_drifts(c):
            out = M.sample_chain(pr, None, None, None, c.results, c.burnin, chain=chain, initial=case_init(c), logpost_grad=lg, trace=trace,
                                 **M.oracle_kwargs(c))
        _runs[key] = (out, trace)
    return _runs[key]


# ---- the oscillator of magi_v2_amd.drift_examples.SIGNED_EXAMPLES: x' = a y, y' = b x + c y ------------------------------------------------------

OSC_TRUTH = np.array([1.0, -2.0, -0.3])
OSC_SPEC = ["positive", "real", "real"]
OSC_BARS = dict(rel=0.25, x=0.1)          # |mean - truth| <= rel |truth| per parameter; max |E[X] - X_true| < x


def oscillator_data(N=41, T=8.0, sd=0.05, seed=3):
    """(I [N], X_obs [N, 2] every point observed, X_true): the exact solution of the linear system from x(0) = (1, 0), noise N(0, sd^2)."""
    a, b, c = OSC_TRUTH
    A = np.array([[0.0, a], [b, c]])
    w, V = np.linalg.eig(A)
    I = np.linspace(0.0, T, N)
    k = np.linalg.solve(V, np.array([1.0, 0.0], dtype=complex))
    X = np.real((V[None] * np.exp(w[None, None, :] * I[:, None, None])) @ k)
    rng = np.random.Generator(np.random.PCG64(seed))
    return I, X + sd * rng.normal(size=X.shape), X


def oscillator_drift(X, th):
    """The oracle's drift-table entry of the oscillator: (f [N, D], J [N, D, D] = df_d/dx_e, T [N, D, P] = df_d/dtheta_p)."""
    x, y = X[:, 0], X[:, 1]
    N = X.shape[0]
    f = np.stack([th[0] * y, th[1] * x + th[2] * y], axis=1)
    J = np.zeros((N, 2, 2))
    J[:, 0, 1] = th[0]
    J[:, 1, 0] = th[1]
    J[:, 1, 1] = th[2]
    T = np.zeros((N, 2, 3))
    T[:, 0, 0] = y
    T[:, 1, 1] = x
    T[:, 1, 2] = y
    return f, J, T


def oscillator_bars(th_samps_natural, X_samps, X_true):
    """The recovery bars (OSC_BARS; b and c negative) on pooled draws: returns (posterior means, max |E[X] - X_true|) after asserting them."""
    mean = np.asarray(th_samps_natural).reshape(-1, 3).mean(axis=0)
    dx = float(np.abs(np.asarray(X_samps).reshape((-1,) + X_true.shape).mean(axis=0) - X_true).max())
    print(f"oscillator: posterior mean of theta {mean.tolist()} (truth {OSC_TRUTH.tolist()}), max|E[X] - X_true| = {dx:.4f}")
    assert np.all(np.abs(mean - OSC_TRUTH) <= OSC_BARS["rel"] * np.abs(OSC_TRUTH)), mean
    assert mean[1] < 0.0 and mean[2] < 0.0, mean
    assert dx < OSC_BARS["x"], dx
    return mean, dx
