"""Reference of the priors on the parameter entries and of known noise variances (include/magi_hip.h: magi_set_prior).

``logpost_grad_prior(sig_prior, th_prior, kinds, bounds)`` restates ``orc.logpost_grad`` under the supports of tests/support_reference.py
(the same table, the same order of operations) and the priors

    kind        log p(v)                               d log p / dv
    flat        0                                      0
    normal      -(v - m)^2 / (2 s^2)                   -(v - m) / s^2
    lognormal   -log v - (log v - m)^2 / (2 s^2)       -(1 + (log v - m) / s^2) / v
    gamma       (k - 1) log v - r v                    (k - 1) / v - r
    invgamma    -(a + 1) log v - b / v                 -(a + 1) / v + b / v^2
    fixed c     sigma^2 = c; the entry's log-Jacobian term becomes -pre^2 / 2 (gradient -pre); t3, t4 use c

on the natural scale v (sigma^2 = softplus(pre) + LB, theta under its support), inside the tempered bracket next to the log-Jacobian terms.
With every prior flat it is the oracle bit for bit (tests/test_prior_cpu.py).  ``fault`` restates what a device that got one rule wrong
would compute -- the sensitivity cases of tests/test_prior_cpu.py.  ``long=True``: the operator products in np.longdouble (another rounding:
the knife-edge condition of the branch tests)."""
import functools

import numpy as np

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import support_reference as S

FLAT, NORMAL, LOGNORMAL, GAMMA, INVGAMMA, FIXED = (host.PRIOR_FLAT, host.PRIOR_NORMAL, host.PRIOR_LOGNORMAL, host.PRIOR_GAMMA, host.PRIOR_INVGAMMA,
                                                   host.PRIOR_FIXED)
# prior ignored (a fixed variance sampled as ever); the prior outside the tempered bracket; dv/dpre dropped from the prior's gradient; lognormal
# without its -log v; a normal prior evaluated on pre; +sg for dv/dpre of an upper-bounded parameter in the prior's gradient; a fixed variance
# without -pre^2 / 2; a fixed variance whose t3, t4 stay on softplus(pre) + LB
FAULTS = ("ignored", "untempered", "no_chain", "lognormal_logv", "on_pre", "upper_sign", "fixed_no_normal", "fixed_softplus")


def log_prior(kinds, a, b, v, fault=None):
    """(sum-ready log p [n], d log p / dv [n]) of the entries' priors at their natural values v; zeros for flat and fixed entries."""
    kinds, a, b, v = np.asarray(kinds), np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(v)
    lp, dlp = np.zeros(v.shape, dtype=v.dtype), np.zeros(v.shape, dtype=v.dtype)
    for j, k in enumerate(kinds):
        x = v[j]
        if k == NORMAL:
            lp[j], dlp[j] = -(x - a[j]) ** 2 / (2.0 * b[j] ** 2), -(x - a[j]) / b[j] ** 2
        elif k == LOGNORMAL:
            lx = np.log(x)
            keep = 0.0 if fault == "lognormal_logv" else 1.0
            lp[j], dlp[j] = -keep * lx - (lx - a[j]) ** 2 / (2.0 * b[j] ** 2), -(keep + (lx - a[j]) / b[j] ** 2) / x
        elif k == GAMMA:
            lp[j], dlp[j] = (a[j] - 1.0) * np.log(x) - b[j] * x, (a[j] - 1.0) / x - b[j]
        elif k == INVGAMMA:
            lp[j], dlp[j] = -(a[j] + 1.0) * np.log(x) - b[j] / x, -(a[j] + 1.0) / x + b[j] / x ** 2
    return lp, dlp


def logpost_grad_prior(sig_prior=None, th_prior=None, kinds=None, bounds=None, fault=None, long=False, temp_of=None):
    """A function with the signature of ``orc.logpost_grad`` under the priors (each None or the (kinds, a, b) of host.prior_spec) and the
    supports (kinds, bounds) of host.theta_support (None: all positive).  ``temp_of`` (the fault "untempered" inside a sampler, which calls
    the function at beta_temp = 1 and tempers what it returns): gives the temperature the caller is about to multiply by, so that the prior
    can be left out of it."""
    if fault == "ignored":
        sig_prior = th_prior = None
    _long = {}

    def fn(X, sig_pre, th_pre, beta_temp, pr):
        D, P = pr.D, pr.P
        ks, as_, bs = sig_prior if sig_prior is not None else host.prior_spec(None, D, "sigma_sq")
        kt, at, bt = th_prior if th_prior is not None else host.prior_spec(None, P, "theta")
        skinds, sbounds = (kinds, bounds) if kinds is not None else host.theta_support(None, P)
        skinds, sbounds = np.asarray(skinds), np.asarray(sbounds, dtype=np.float64)
        real, upper, lower = skinds == S.REAL, skinds == S.UPPER, skinds == S.LOWER
        fixed = np.asarray(ks) == FIXED
        sp_s = np.log(1.0 + np.exp(sig_pre))
        sigma_sqs = sp_s + pr.LB
        if fault != "fixed_softplus":
            sigma_sqs = np.where(fixed, as_, sigma_sqs)
        with np.errstate(over="ignore", invalid="ignore"):
            sp_t = np.log(1.0 + np.exp(th_pre))
            sg_t = 1.0 / (1.0 + np.exp(-th_pre))
        thetas = np.where(real, th_pre, np.where(upper, sbounds - sp_t, np.where(lower, sbounds + sp_t, sp_t)))
        dth_dpre = np.where(real, 1.0, np.where(upper, -sg_t, sg_t))
        ljd_t = np.where(real, 0.0, 1.0 - sg_t)
        sg_s = 1.0 / (1.0 + np.exp(-sig_pre))
        own = 0.0 if fault == "fixed_no_normal" else 1.0
        lj_s = np.sum(np.where(fixed, -0.5 * own * sig_pre * sig_pre, sig_pre - sp_s))
        lj_t = np.sum(np.where(real, 0.0, th_pre - sp_t))
        # the priors, on the natural values (a normal one on pre under the fault "on_pre")
        pre_n_s, pre_n_t = (np.asarray(ks) == NORMAL) & (fault == "on_pre"), (np.asarray(kt) == NORMAL) & (fault == "on_pre")
        lp_s, dlp_s = log_prior(ks, as_, bs, np.where(pre_n_s, sig_pre, sigma_sqs), fault)
        lp_t, dlp_t = log_prior(kt, at, bt, np.where(pre_n_t, th_pre, thetas), fault)
        dv_s = np.where(pre_n_s | (fault == "no_chain"), 1.0, sg_s)
        dv_t = np.where(pre_n_t | (fault == "no_chain"), 1.0, np.where(upper & (fault == "upper_sign"), sg_t, dth_dpre))
        lprior = np.sum(lp_s) + np.sum(lp_t)
        pg_s, pg_t = dlp_s * dv_s, dlp_t * dv_t

        if long and id(pr) not in _long:
            _long[id(pr)] = tuple(np.asarray(m_, dtype=np.longdouble) for m_ in (pr.C_inv, pr.m, pr.K_inv))
        Ci, m, Ki = _long[id(pr)] if long else (pr.C_inv, pr.m, pr.K_inv)
        up = (lambda v: np.asarray(v, dtype=np.longdouble)) if long else (lambda v: v)
        xc = up((X - pr.mu).T[:, :, None])
        Cx = Ci @ xc
        CTx = np.transpose(Ci, (0, 2, 1)) @ xc
        t1 = np.sum(xc * Cx)
        f, J, T = orc.DRIFTS[pr.drift][0](X, thetas)
        r = up(f.T[:, :, None]) - (m @ xc)
        Kr = Ki @ r
        KTr = np.transpose(Ki, (0, 2, 1)) @ r
        t2 = np.sum(r * Kr)
        g = (Kr + KTr)[:, :, 0]
        t3 = np.sum(pr.N_ds * np.log(2.0 * np.pi * sigma_sqs))
        cols = pr.obs_idx % D
        resid = X.reshape(-1)[pr.obs_idx] - pr.y
        t4 = np.sum(np.square(resid) * (1.0 / sigma_sqs)[cols])
        core = -0.5 * (((1.0 / pr.beta) * (t1 + t2)) + (t3 + t4)) + lj_s + lj_t
        bt = beta_temp * (temp_of() if temp_of is not None else 1.0)          # ("untempered": the prior divided by what it will be multiplied by)
        logp = beta_temp * core + beta_temp * lprior / bt if fault == "untempered" else beta_temp * (core + lprior)

        mTg = (np.transpose(m, (0, 2, 1)) @ g[:, :, None])[:, :, 0]
        d12 = (Cx + CTx)[:, :, 0] - mTg + np.einsum("dn,nde->en", g, up(J))
        d4 = np.zeros(X.size)
        np.add.at(d4, pr.obs_idx, 2.0 * resid / sigma_sqs[cols])
        gX = beta_temp * (-0.5 * ((1.0 / pr.beta) * np.asarray(d12, dtype=np.float64).T + d4.reshape(X.shape)))
        SS = np.zeros(D)
        np.add.at(SS, cols, np.square(resid))
        dsig = pr.N_ds / sigma_sqs - SS / sigma_sqs ** 2
        gs0 = -0.5 * dsig * sg_s + (1.0 - sg_s)
        if fixed.any():          # its own term -pre^2 / 2; t3, t4 give no gradient (unless the fault leaves them on softplus(pre) + LB)
            gs0 = np.where(fixed, (-0.5 * dsig * sg_s if fault == "fixed_softplus" else 0.0) - own * sig_pre, gs0)
        dth = np.asarray(np.einsum("dn,ndp->p", g, up(T)), dtype=np.float64)
        gt0 = -0.5 * (1.0 / pr.beta) * dth * dth_dpre + ljd_t
        if fault == "untempered":
            gsig, gth = beta_temp * gs0 + beta_temp * pg_s / bt, beta_temp * gt0 + beta_temp * pg_t / bt
        else:
            gsig, gth = beta_temp * (gs0 + pg_s), beta_temp * (gt0 + pg_t)
        return float(logp), gX, gsig, gth
    return fn


# ---- the sampler cases of tests/test_prior_gpu.py; tests/test_prior_cpu.py holds each to the sensitivity and the knife-edge conditions ----------

# SEIR-4 (D = 4, P = 3) under the supports of tests/support_reference.py (real, lower 0.5, upper 3.0): every kind on a sigma^2 entry, one fixed;
# normal priors on the real and the upper-bounded parameter, a lognormal one on the lower-bounded
SIG_N41 = [("invgamma", 3.0, 2e-4), ("fixed", 2.5e-4), ("gamma", 2.0, 4e3), ("lognormal", -8.0, 0.5)]
TH_N41 = [("normal", -0.8, 0.05), ("lognormal", 0.5, 0.1), ("normal", 1.5, 0.05)]
_ALL = ((1, "auto"), (2, "auto"), (8, "mc"), (9, "mc"))          # k_stream<1>, k_stream<2>, k_stream_sep<8>, k_stream_sep<16>


class PriorCase(S.SupportCase):
    """A row of tests.support_reference's kind with the priors of the sigma^2 and the theta entries; ``sig0``: sigma_pre of the fixed entries
    at the start (a value away from 0, so that their own term -pre^2 / 2 shows)."""

    def __init__(self, name, kind, N, band, cfg, runs, spec, theta0, sig_prior, th_prior, sig0=1.5, **kw):
        super().__init__(name, kind, N, band, cfg, runs, spec, theta0, **kw)
        self.sig_prior, self.th_prior, self.sig0 = sig_prior, th_prior, sig0


_PT_SPEC = ["positive", "real", ("upper", 1.0), ("lower", 0.01), "real", "positive"]
CASES = [
    PriorCase("nuts_n41", "seir", 41, None, S._NUTS7, _ALL, S.SPEC_N41, S.THETA0_N41, SIG_N41, TH_N41, dt=0.1, results=4),
    PriorCase("hmc_n41", "seir", 41, None, dict(step_size=5e-3, mode=1, hmc_leapfrogs=8, stale_cache=0), ((1, "auto"), (8, "mc")), S.SPEC_N41, S.THETA0_N41,
              SIG_N41, TH_N41, dt=0.1, seed=863, results=12),
    PriorCase("nuts_n161_b20", "seir", 161, 20, S._NUTS7, ((1, "auto"),), S.SPEC_N41, S.THETA0_N41, SIG_N41, TH_N41, seed=4, results=4),
    # not separable: k_stream_mc.  D = 5, P = 6: the densities on (0, inf) sit on the positive and the lower-bounded parameters
    PriorCase("nuts_ptrans_n41", "traced", 41, None, S._NUTS6, ((3, "mc"),), _PT_SPEC, S._nominal("ptrans"),
              [("gamma", 2.0, 20.0), ("fixed", 0.05), ("invgamma", 3.0, 0.1), ("lognormal", -3.0, 1.0), ("normal", 0.05, 0.02)],
              [("gamma", 2.0, 10.0), ("normal", 0.5, 0.2), ("normal", 0.1, 0.1), ("invgamma", 3.0, 1.0), ("normal", 0.0, 0.05), ("lognormal", -1.0, 0.5)],
              drift="ptrans", results=4),
]


def case(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def case_tables(name):
    """((kinds, bounds) of the supports, (kinds, a, b) of the sigma^2 priors, (kinds, a, b) of the theta priors) of a case."""
    c = case(name)
    sup = host.theta_support(c.spec, len(c.spec))
    return sup, host.prior_spec(c.sig_prior, len(c.sig_prior), "sigma_sq"), host.prior_spec(c.th_prior, len(c.th_prior), "theta", sup)


def case_init(c):
    """(X0, sig_pre0, th_pre0) of a case: the problem's own X and sigma (a fixed entry at c.sig0), theta0 through host.theta_pre_inits."""
    X0, s0, _ = S.case_problem(c)[2]
    sup, sp, _ = case_tables(c.name)
    with S.oracle_drifts(c):
        th0 = np.asarray(c.theta0() if callable(c.theta0) else c.theta0, dtype=np.float64)
    return X0, np.where(sp[0] == FIXED, c.sig0, s0), host.theta_pre_inits(th0, *sup)


_runs = {}
# the warm-up of tests/test_metric_gpu.py on the N = 41 case under its priors: warmup_schedule(40, 32, 8, 4, 8) -- windows [8, 12) and [12, 24)
# become metrics -- then 13 more transitions, 5 of them results; depth <= 2.  (Philox seed 816: the first from 808 on at which rounding the
# operator products in longdouble moves the step sizes behind the metric restarts by less than 1/100 of their 1e-9 bar as well -- the
# variance over a four-state window amplifies it to 2e-11 .. 1e-9 under the others)
WARM = dict(burnin=40, results=5, max_tree_depth=2, sched=(40, 32, 8, 4, 8), seed=816)


def warm_run(chain, fault=None, long=False):
    """sample_chain's output of one chain of the warm-up case (the N = 41 case's problem, supports, priors and start)."""
    return case_run(case("nuts_n41"), chain, fault, long, warm=True)[0]


def case_run(c, chain, fault=None, long=False, warm=False):
    """(sample_chain's output, trace) of one chain of a case under its priors and supports; once per session.  ``warm``: the schedule WARM
    instead of the case's own transitions."""
    key = (c.name, chain, fault, long, warm)
    kw = dict(M.oracle_kwargs(c))
    n_res, n_burn = c.results, c.burnin
    if warm:
        n_res, n_burn = WARM["results"], WARM["burnin"]
        kw.update(seed=WARM["seed"], max_tree_depth=WARM["max_tree_depth"], windows=[(a, b) for a, b, adapt in host.warmup_schedule(*WARM["sched"]) if adapt])
    if key not in _runs:
        pr = S.case_problem(c)[0]
        sup, sp, tp = case_tables(c.name)
        trace = []
        # (the sampler tempers what the function returns: the fault "untempered" needs the temperature of the transition in progress)
        now, temperature = {"t": 1.0}, orc.temperature
        def recording(step, min_temp):
            now["t"] = temperature(step, min_temp)
            return now["t"]
        lg = logpost_grad_prior(sp, tp, *sup, fault=fault, long=long, temp_of=(lambda: now["t"]) if fault == "untempered" else None)
        orc.temperature = recording
        try:
            with S.oracle_drifts(c), np.errstate(all="ignore"):
                out = M.sample_chain(pr, None, None, None, n_res, n_burn, chain=chain, initial=case_init(c), logpost_grad=lg, trace=trace, **kw)
        finally:
            orc.temperature = temperature
        _runs[key] = (out, trace)
    return _runs[key]


# ---- end to end: a flat prior against an informative one on the N = 41 golden problem ------------------------------------------------------------

# (depth <= 3: over 400 transitions the chain then keeps its integers and its draws to 2e-10 when the operator products are rounded in
#  np.longdouble instead; from depth 4 on rounding is amplified until the two runs part -- nothing a device could be compared with)
E2E = dict(results=200, burnin=200, seed=5, chain=0, max_tree_depth=3, entry=0)


@functools.lru_cache(maxsize=None)
def e2e_problem():
    from tests.util import load_g4, problem_from_g4
    g = load_g4("sirw_N41")
    return g, problem_from_g4(g, None)


_e2e = {}


def e2e_prior():
    """A normal prior on theta_0 centred at 3.0, sd 0.05: the flat posterior of that parameter has mean 0.44 and sd 0.25."""
    return [("normal", 3.0, 0.05), None, None, None, None]


def e2e_run(th_prior_spec, long=False):
    """(theta draws [results, P] on the natural scale, sample_chain's output) of the end-to-end chain under a theta prior specification
    (None: flat)."""
    key = (repr(th_prior_spec), long)
    if key not in _e2e:
        g, pr = e2e_problem()
        tp = None if th_prior_spec is None else host.prior_spec(th_prior_spec, pr.P, "theta")
        lg = logpost_grad_prior(None, tp, long=long)
        out = M.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), E2E["results"], E2E["burnin"], seed=E2E["seed"], chain=E2E["chain"],
                             stale_cache=False, max_tree_depth=E2E["max_tree_depth"], logpost_grad=lg)
        _e2e[key] = (np.log(1.0 + np.exp(out[2])), out)
    return _e2e[key]
