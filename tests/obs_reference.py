"""Reference of the observation model: log and square-root links and known observation weights (include/magi_hip.h: magi_set_obs_model;
DESIGN 4.2e).

``logpost_grad_obs(links, weight, ...)`` restates ``orc.logpost_grad`` under the supports and priors of tests/prior_reference.py (the same
tables, the same order of operations) and the observation model

    link       g(x)      g'(x)            t4 = sum_d (1 / sigma^2_d) sum_{k in obs_d} w_k (g_d(x_k) - g_d(y_k))^2
    identity   x         1                dt4 / dx_k = 2 w_k (g_d(x_k) - g_d(y_k)) g_d'(x_k) / sigma^2_d
    log        log x     1 / x            t3 = sum_d N_d log(2 pi sigma^2_d) as ever
    sqrt       sqrt x    1 / (2 sqrt x)

with the link evaluated at observed points only.  With identity links and no weights it is the oracle and prior_reference bit for bit
(tests/test_obs_cpu.py).  ``fault`` restates what a device that got one rule wrong would compute -- the sensitivity cases of
tests/test_obs_cpu.py.  ``long=True``: the operator products in np.longdouble (another rounding: the knife-edge condition)."""
import contextlib
import functools

import numpy as np

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import support_reference as S
from tests import prior_reference as PR

IDENTITY, LOG, SQRT = host.LINK_IDENTITY, host.LINK_LOG, host.LINK_SQRT
LINKS_SEIR4 = (LOG, IDENTITY, SQRT, LOG)          # mixed links of the SEIR-4 fixtures: S, E, I, R
# the model ignored; g' dropped from the gradient; g(x) - y with the datum left on the natural scale; g' = 1 / sqrt x under the sqrt link; the
# weights ignored; squared; in the gradient but not in t4; the sigma^2 gradient from the unweighted sum; the link evaluated at unobserved
# points too (0 x g(x) added there: NaN where x is outside the domain)
FAULTS = ("ignored", "no_chain", "y_untransformed", "sqrt_half", "weight_ignored", "weight_squared", "weight_grad_only", "sigma_grad_unweighted",
          "link_everywhere")


def link_g(links, cols, v):
    """(g(v), g'(v)) of the entries' links: links[cols[k]] applies to v[k]."""
    lk = np.asarray(links)[cols]
    v = np.asarray(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(lk == LOG, np.log(v), np.where(lk == SQRT, np.sqrt(v), v))
        dg = np.where(lk == LOG, 1.0 / v, np.where(lk == SQRT, 0.5 / np.sqrt(v), 1.0))
    return g, dg


def logpost_grad_obs(links=None, weight=None, sig_prior=None, th_prior=None, kinds=None, bounds=None, fault=None, long=False, record=None):
    """A function with the signature of ``orc.logpost_grad`` under the observation model -- ``links``: codes [D] or None; ``weight``: [n_obs]
    aligned with ``pr.obs_idx`` or None -- the priors (each None or the (kinds, a, b) of host.prior_spec) and the supports (kinds, bounds) of
    host.theta_support (None: all positive).  ``record``: a list that receives, per evaluation, (the smallest x at an observed point of a
    linked component, max|X|) -- how far the states of a run stay from a link's edge."""
    if fault == "ignored":
        links = weight = None
    _long = {}

    def fn(X, sig_pre, th_pre, beta_temp, pr):
        D, P = pr.D, pr.P
        lk = np.zeros(D, dtype=np.int64) if links is None else np.asarray(links, dtype=np.int64)
        ks, as_, bs = sig_prior if sig_prior is not None else host.prior_spec(None, D, "sigma_sq")
        kt, at, bt = th_prior if th_prior is not None else host.prior_spec(None, P, "theta")
        skinds, sbounds = (kinds, bounds) if kinds is not None else host.theta_support(None, P)
        skinds, sbounds = np.asarray(skinds), np.asarray(sbounds, dtype=np.float64)
        real, upper, lower = skinds == S.REAL, skinds == S.UPPER, skinds == S.LOWER
        fixed = np.asarray(ks) == PR.FIXED
        sp_s = np.log(1.0 + np.exp(sig_pre))
        sigma_sqs = np.where(fixed, as_, sp_s + pr.LB)
        with np.errstate(over="ignore", invalid="ignore"):
            sp_t = np.log(1.0 + np.exp(th_pre))
            sg_t = 1.0 / (1.0 + np.exp(-th_pre))
        thetas = np.where(real, th_pre, np.where(upper, sbounds - sp_t, np.where(lower, sbounds + sp_t, sp_t)))
        dth_dpre = np.where(real, 1.0, np.where(upper, -sg_t, sg_t))
        ljd_t = np.where(real, 0.0, 1.0 - sg_t)
        sg_s = 1.0 / (1.0 + np.exp(-sig_pre))
        lj_s = np.sum(np.where(fixed, -0.5 * sig_pre * sig_pre, sig_pre - sp_s))
        lj_t = np.sum(np.where(real, 0.0, th_pre - sp_t))
        lp_s, dlp_s = PR.log_prior(ks, as_, bs, sigma_sqs)
        lp_t, dlp_t = PR.log_prior(kt, at, bt, thetas)
        lprior = np.sum(lp_s) + np.sum(lp_t)
        pg_s, pg_t = dlp_s * sg_s, dlp_t * dth_dpre

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

        # ---- the observation terms ----
        cols = pr.obs_idx % D
        x_obs = X.reshape(-1)[pr.obs_idx]
        if record is not None:
            linked = lk[cols] != IDENTITY
            record.append((float(x_obs[linked].min()) if linked.any() and np.isfinite(X).all() else np.nan, float(np.abs(X).max())))
        gx, dg = link_g(lk, cols, x_obs)
        gy = pr.y if fault == "y_untransformed" else link_g(lk, cols, pr.y)[0]
        if fault == "no_chain":
            dg = np.ones_like(dg)
        if fault == "sqrt_half":
            dg = np.where(lk[cols] == SQRT, 2.0 * dg, dg)
        w = np.ones(len(pr.obs_idx)) if weight is None or fault == "weight_ignored" else np.asarray(weight, dtype=np.float64)
        if fault == "weight_squared":
            w = w * w
        resid = gx - gy
        w_val = np.ones_like(w) if fault == "weight_grad_only" else w            # the weight t4 (and the sum behind the sigma^2 gradient) sees
        t4 = np.sum(w_val * np.square(resid) * (1.0 / sigma_sqs)[cols])
        if fault == "link_everywhere":          # 0 x g(x) from every unobserved entry
            seen = np.zeros(X.size, dtype=bool)
            seen[pr.obs_idx] = True
            rest = np.where(~seen)[0]
            t4 = t4 + np.sum(0.0 * link_g(lk, rest % D, X.reshape(-1)[rest])[0])
        core = -0.5 * (((1.0 / pr.beta) * (t1 + t2)) + (t3 + t4)) + lj_s + lj_t
        logp = beta_temp * (core + lprior)

        mTg = (np.transpose(m, (0, 2, 1)) @ g[:, :, None])[:, :, 0]
        d12 = (Cx + CTx)[:, :, 0] - mTg + np.einsum("dn,nde->en", g, up(J))
        d4 = np.zeros(X.size)
        np.add.at(d4, pr.obs_idx, 2.0 * w * resid * dg / sigma_sqs[cols])
        if fault == "link_everywhere":
            d4[rest] = 0.0 * link_g(lk, rest % D, X.reshape(-1)[rest])[1]
        gX = beta_temp * (-0.5 * ((1.0 / pr.beta) * np.asarray(d12, dtype=np.float64).T + d4.reshape(X.shape)))
        SS = np.zeros(D)
        np.add.at(SS, cols, (np.ones_like(w) if fault == "sigma_grad_unweighted" else w_val) * np.square(resid))
        dsig = pr.N_ds / sigma_sqs - SS / sigma_sqs ** 2
        gs0 = -0.5 * dsig * sg_s + (1.0 - sg_s)
        if fixed.any():
            gs0 = np.where(fixed, -sig_pre, gs0)
        dth = np.asarray(np.einsum("dn,ndp->p", g, up(T)), dtype=np.float64)
        gt0 = -0.5 * (1.0 / pr.beta) * dth * dth_dpre + ljd_t
        fn.terms = (float(t3), float(t4))
        return float(logp), gX, beta_temp * (gs0 + pg_s), beta_temp * (gt0 + pg_t)
    return fn


def draw_weights(n_obs, seed):
    """Weights in (0.25, 4), log-uniform, on a random half of the observations; 1 elsewhere."""
    rng = np.random.default_rng([seed, 977])
    w = np.ones(n_obs)
    half = rng.permutation(n_obs)[: n_obs // 2]
    w[half] = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(half)))
    return w


def unobserve(pr, d):
    """The problem without any observation of component d (N_d = 0; beta as it was: a constant of the fixture)."""
    import dataclasses
    keep = pr.obs_idx % pr.D != d
    N_ds = np.array(pr.N_ds, dtype=np.float64)
    N_ds[d] = 0.0
    out = dataclasses.replace(pr, obs_idx=pr.obs_idx[keep], y=pr.y[keep], N_ds=N_ds)
    if hasattr(pr, "unmasked"):
        out.unmasked = pr.unmasked
    return out


# ---- the log-posterior fixtures of tests/test_obs_gpu.py; tests/test_obs_cpu.py holds each to the sensitivity and the conditioning conditions -----

class LogpostFixture:
    """tests/util.structureless_problem(N, drift) (states in (0.05, 0.3), or (0.1, 0.9) for the traced drifts: both links defined; every
    operator block counts) under ``links`` and the weights of draw_weights.  ``batches``: [(states, stream_family)] the device evaluates;
    ``unobserved``: a component without any observation; ``neg`` = (row, component): an UNOBSERVED entry of a log-linked component that every
    state holds at -0.07 -- without consequence, unless the link is evaluated there (fault "link_everywhere"); ``sig_prior`` / ``support``:
    specifications of host.prior_spec / host.theta_support (composition cases)."""

    def __init__(self, name, N, drift, links, batches, band=None, unobserved=None, neg=(1, 0), sig_prior=None, support=None, kind="builtin"):
        self.name, self.N, self.drift, self.links, self.batches, self.band = name, N, drift, tuple(links), tuple(batches), band
        self.unobserved, self.neg, self.sig_prior, self.support, self.kind = unobserved, neg, sig_prior, support, kind

    def __repr__(self):
        return self.name


_FAM = lambda ns: tuple((n, f) for n in ns for f in ("auto", "mc"))
LOGPOST = [
    LogpostFixture("seir4_n127", 127, "seir4", LINKS_SEIR4, _FAM((1, 3))),
    LogpostFixture("seir4_n129", 129, "seir4", LINKS_SEIR4, _FAM((1, 2, 3, 9))),                      # k_stream<1>, <2>, k_stream_sep<8>, <16>
    LogpostFixture("seir4_n257", 257, "seir4", LINKS_SEIR4, _FAM((1, 3))),
    LogpostFixture("seir4_n129_unobserved", 129, "seir4", LINKS_SEIR4, _FAM((1, 3)), unobserved=1),
    LogpostFixture("seir4_n257_b20", 257, "seir4", LINKS_SEIR4, _FAM((1, 3)), band=20),
    # not separable: k_stream_mc + point_block.  The drift takes log of component 0, so the negative unobserved entry sits in component 1
    LogpostFixture("gompertz_n129", 129, "gompertz", (SQRT, LOG), ((1, "auto"), (3, "mc")), neg=(1, 1), kind="domain"),
    LogpostFixture("seasonal_n129", 129, "seir_seasonal", (LOG, SQRT, IDENTITY), ((1, "auto"), (3, "mc")), kind="traced"),      # uses t
    # composition: a fixed sigma^2 on a linked, weighted component; a lower-bounded theta
    LogpostFixture("seir4_n129_fixed", 129, "seir4", LINKS_SEIR4, ((1, "auto"), (3, "mc")), sig_prior=[("fixed", 0.04), None, ("gamma", 2.0, 10.0), None]),
    LogpostFixture("seir4_n129_lower", 129, "seir4", LINKS_SEIR4, ((1, "auto"), (3, "mc")), support=[("lower", 1.0), "positive", "real"]),
]
NEG_VALUE = -0.07


def logpost_fixture(name):
    return next(f for f in LOGPOST if f.name == name)


@contextlib.contextmanager
def fixture_drifts(fx):
    """The oracle's drift-table entry of a fixture's traced drift, for the duration."""
    if fx.kind == "domain":
        from tests.util import domain_drifts
        with domain_drifts():
            yield
    elif fx.kind == "traced":
        from tests.test_structureless_cpu import register_traced
        had = fx.drift in orc.DRIFTS
        register_traced(fx.drift, fx.N)
        try:
            yield
        finally:
            if not had:
                del orc.DRIFTS[fx.drift]
    else:
        yield


_built = {}


def logpost_build(fx):
    """(orc.Problem, weights [n_obs], (X[n, N, D], sig_pre[n, D], th_pre[n, P]) for the largest batch, tables) of a fixture; once per session,
    read-only.  ``tables`` = dict(links, sig_prior, th_prior, kinds, bounds) as logpost_grad_obs takes them.  Call inside fixture_drifts."""
    if fx.name not in _built:
        from tests.util import structureless_problem, structureless_states
        seed = 52361 + 17 * fx.N + sum(map(ord, fx.drift))
        pr, X = structureless_problem(fx.N, fx.drift, seed, band=fx.band)
        if fx.unobserved is not None:
            pr = unobserve(pr, fx.unobserved)
        n = max(b for b, _ in fx.batches)
        Xb, sp, tp = structureless_states(pr, X, n, 3)
        assert fx.links[fx.neg[1]] == LOG and fx.neg[0] % 2 == 1          # (odd rows are unobserved)
        Xb[:, fx.neg[0], fx.neg[1]] = NEG_VALUE
        sup = host.theta_support(fx.support, pr.P) if fx.support is not None else None
        if sup is not None:                                               # the same natural parameters under the supports
            tp = np.stack([host.theta_pre_inits(host.transform_samples(sp[i], tp[i], pr.LB)[1], *sup) for i in range(n)])
            tp[:, np.asarray(sup[0]) == host.THETA_REAL] *= -1.0          # (a real entry at a negative value)
        tables = dict(links=np.asarray(fx.links), sig_prior=host.prior_spec(fx.sig_prior, pr.D, "sigma_sq") if fx.sig_prior is not None else None,
                      th_prior=None, kinds=None if sup is None else sup[0], bounds=None if sup is None else sup[1])
        _built[fx.name] = (pr, draw_weights(len(pr.obs_idx), fx.N), (Xb, sp, tp), tables)
    return _built[fx.name]


def figures(got, ref):
    """The compared quantities of one state, each as the GPU tests measure it: the value and t3, t4 relative to themselves, every gradient
    relative to its own largest entry.  got / ref = (logp, gX, gsig, gth, t3, t4).  A figure that is not finite counts as infinite."""
    out = {"value": abs(got[0] - ref[0]) / abs(ref[0])}
    for k, name in ((1, "dX"), (2, "dsigma"), (3, "dtheta")):
        out[name] = np.abs(np.asarray(got[k]) - ref[k]).max() / np.abs(ref[k]).max()
    out["t3"], out["t4"] = abs(got[4] - ref[4]) / abs(ref[4]), abs(got[5] - ref[5]) / abs(ref[5])
    return {k: (float(v) if np.isfinite(v) else np.inf) for k, v in out.items()}


def reference_of(fx, state, temp, fault=None, long=False):
    """(logp, gX, gsig, gth, t3, t4) of state ``state`` of a fixture on the reference."""
    pr, w, (Xb, sp, tp), tb = logpost_build(fx)
    fn = logpost_grad_obs(tb["links"], w, tb["sig_prior"], tb["th_prior"], tb["kinds"], tb["bounds"], fault=fault, long=long)
    with np.errstate(all="ignore"):
        out = fn(Xb[state], sp[state], tp[state], temp, pr)
    return out + fn.terms


# ---- the sampler cases of tests/test_obs_gpu.py; tests/test_obs_cpu.py holds each to the sensitivity and the knife-edge conditions -----------------

# SEIR-4 from x(0) = (0.6, 0.1, 0.2, 0.1) over one time unit: every component stays in [0.1, 0.6], so both links are defined along the
# whole trajectory; 10 % multiplicative noise on every other grid point.  ``r0``: x(0) of R instead of 0.1 -- the domain case starts R at
# 3e-3, where a leapfrog trajectory of step 1e-2 crosses 0 at an observed point of its log link.
X0_SEIR4 = (0.6, 0.1, 0.2, 0.1)
THETA_SEIR4 = np.array([6.0, 0.6, 1.8])
T_SEIR4 = 1.0


@functools.lru_cache(maxsize=None)
def obs_problem(N, band=None, r0=None, noise=0.1):
    """(fixture {"Xhat_init", "sigma_sqs_init"}, orc.Problem with the reference's band mask, unmasked orc.Problem, weights [n_obs]) -- the
    recipe of tests/metric_reference.seir_problem on multiplicative data: rk4 truth, y = x exp(noise z) at the even grid indices from
    default_rng(N), oracle-built matrices with the reference's initial hyper-parameters, sigma^2 started on each link's scale."""
    from magi_v2_amd.drift_examples import rk4
    from tests.util import band_part_copy
    x0 = list(X0_SEIR4)
    if r0 is not None:
        x0[3] = r0
    I, truth = rk4(host.NUMPY_DRIFTS["seir4"], x0, THETA_SEIR4, T_SEIR4, N)
    rng = np.random.default_rng(N)
    X_obs = np.full(truth.shape, np.nan)
    rows = np.arange(0, N, 2)
    X_obs[rows] = truth[rows] * np.exp(noise * rng.standard_normal((len(rows), 4)))
    Xi = orc.linear_interpolate(X_obs)
    hp = orc.hparams_initial(Xi)
    C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], hp["phi2s"], 2.01, bandsize=None)
    N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
    idx = np.where(~np.isnan(X_obs).flatten())[0]
    Xhat = orc.cubic_smoother(I, Xi)
    links = np.asarray(LINKS_SEIR4)
    w = draw_weights(len(idx), N)
    LB, sig0 = host.link_sigma_defaults(links, X_obs, Xhat, None, orc.sigma_sqs_lower_bound(Xhat), hp["sigma_sqs"], False)
    mk = lambda b: orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=band_part_copy(C_inv, b), m=band_part_copy(m, b), K_inv=band_part_copy(K_inv, b), N_ds=N_ds,
                               obs_idx=idx, y=X_obs.reshape(-1)[idx], beta=float(4 * N / N_ds.sum()), LB=LB, drift="seir4", P=3)
    return {"Xhat_init": Xhat, "sigma_sqs_init": sig0}, mk(band), mk(None), w


class ObsCase(M.MetricCase):
    """A row of tests.metric_reference's kind on ``obs_problem(N, band, r0)`` under LINKS_SEIR4 and the fixture's weights; ``warm``: a
    warm-up that adapts the metric (the schedule of tests/prior_reference.WARM) instead of the case's own transitions."""

    def __init__(self, name, N, band, cfg, runs, r0=None, theta0=(1.0, 1.0, 1.0), warm=False, **kw):
        super().__init__(name, "obs", N, band, cfg, runs, **kw)
        self.r0, self.theta0, self.warm = r0, tuple(theta0), warm


_NUTS6 = dict(step_size=2e-3, max_tree_depth=6, stale_cache=0)
_ALL = ((1, "auto"), (2, "auto"), (3, "mc"), (9, "mc"))          # k_stream<1>, k_stream<2>, k_stream_sep<8>, k_stream_sep<16>
CASES = [
    ObsCase("nuts_n41", 41, None, _NUTS6, _ALL, results=4),
    ObsCase("hmc_n41", 41, None, dict(step_size=2e-4, mode=1, hmc_leapfrogs=8, stale_cache=0), ((1, "auto"), (3, "mc")), results=8),
    ObsCase("nuts_n161_b20", 161, 20, _NUTS6, ((1, "auto"), (3, "mc")), results=4),
    ObsCase("warm_n41", 41, None, _NUTS6, ((1, "auto"), (2, "auto")), warm=True),
    # R starts at 2e-3 under its log link: leaves with R <= 0 at an observed point (tests/test_obs_cpu.py reads them off the census)
    ObsCase("domain_n41", 41, None, dict(step_size=1e-2, max_tree_depth=6, stale_cache=0), ((1, "auto"), (3, "mc")), r0=3e-3, burnin=6, results=4),
]
# the warm-up of tests/prior_reference.py (two windows become metrics, then 13 more transitions, 5 of them results; depth <= 2).  Philox seed
# 1087: the first from 808 on at which rounding the operator products in longdouble moves every compared float of chains 20 and 21 by at
# most 1/100 of its bar -- the variance over a four-state window amplifies it to 0.04 .. 150 x the bars under the 279 seeds before it
WARM = dict(PR.WARM, seed=1087)


def case(name):
    return next(c for c in CASES if c.name == name)


def case_problem(c):
    """(masked orc.Problem, unmasked orc.Problem, (X0, sig_pre0, th_pre0), weights) of a case."""
    fx, pr, dense, w = obs_problem(c.N, c.band, c.r0)
    return pr, dense, orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.asarray(c.theta0), pr.LB), w


_runs = {}


def case_run(c, chain, fault=None, long=False, census=False):
    """(sample_chain's output, trace, record, events) of one chain of a case under its observation model; once per session.  ``record``:
    logpost_grad_obs's, one entry per evaluated state; ``events``: the oracle's census (``census=True``; NUTS only)."""
    key = (c.name, chain, fault, long, census)
    if key not in _runs:
        pr, _, init, w = case_problem(c)
        kw = dict(M.oracle_kwargs(c))
        n_res, n_burn = c.results, c.burnin
        if c.warm:
            n_res, n_burn = WARM["results"], WARM["burnin"]
            kw.update(seed=WARM["seed"], max_tree_depth=WARM["max_tree_depth"], windows=[(a, b) for a, b, adapt in host.warmup_schedule(*WARM["sched"]) if adapt])
        trace, record = [], []
        lg = logpost_grad_obs(LINKS_SEIR4, w, fault=fault, long=long, record=record)
        events = None
        with np.errstate(all="ignore"):
            if census:
                from tests.util import Census
                events = Census(lambda: len(record))
                fx = obs_problem(c.N, c.band, c.r0)[0]          # (orc.sample_chain forms the same initial state from the fixture)
                out = orc.sample_chain(pr, fx["Xhat_init"], fx["sigma_sqs_init"], np.asarray(c.theta0), n_res, n_burn, chain=chain, trace=trace,
                                       events=events, logpost_grad=lg, **kw)
            else:
                out = M.sample_chain(pr, None, None, None, n_res, n_burn, chain=chain, initial=init, logpost_grad=lg, trace=trace, **kw)
        _runs[key] = (out, trace, record, events)
    return _runs[key]



# ---- end to end: predator-prey data with 10 % multiplicative noise through predict(obs_link=..., obs_weight=...) -----------------------------------

# (depth <= 3, 200 + 200 transitions: the setting of tests/prior_reference.E2E -- deeper, a reference parts from its longdouble twin.  T = 2:
#  two thirds of a cycle, which the cubic smoother behind Xhat_init follows; over T = 4 it undershoots 0.  Philox seed 8: this posterior is
#  stiff -- steps of 4e-4 -- and the chain amplifies rounding strongly, under identity links as under log links: of the seeds 1 .. 24 only 8
#  keeps float64 and longdouble operator products within 1/100 of the bars (draws to 3e-11; 4e-8 .. 1e-2 under the others) -- chosen on the
#  reference alone, tests/test_obs_cpu.py asserts it)
E2E = dict(N=41, T=2.0, noise=0.1, data_seed=12, results=200, burnin=200, seed=8, max_tree_depth=3, links=("log", "log"), phi2=1.5,
           truth=(1.5, 1.0, 3.0, 1.0), x0=(1.0, 1.5))


@functools.lru_cache(maxsize=None)
def e2e_data(data_seed=None):
    """(I [N], X_obs [N, 2] every point observed, X_true, weights [N, 2]): the Lotka-Volterra trajectory of drift_examples.rk4 times
    exp(0.1 z), z from default_rng(data_seed); weights 1, 2 or 4 -- a point that is the mean of so many replicates."""
    from magi_v2_amd.drift_examples import lotka_volterra, rk4
    e = E2E
    I, X = rk4(lotka_volterra, list(e["x0"]), np.asarray(e["truth"]), e["T"], e["N"])
    rng = np.random.default_rng(e["data_seed"] if data_seed is None else data_seed)
    X_obs = X * np.exp(e["noise"] * rng.standard_normal(X.shape))
    return I, X_obs, X, rng.choice([1.0, 2.0, 4.0], size=X.shape)


def e2e_oracle_drift(I):
    """The oracle's drift-table entry of the predator-prey system (Jacobians by complex step)."""
    from magi_v2_amd.drift_examples import lotka_volterra
    from tests.test_time_drift_cpu import oracle_drift_at
    return oracle_drift_at(lotka_volterra, np.asarray(I).reshape(-1)), 2, 4


def e2e_reference(pr, Xhat_init, sig_pre0, th_pre0, links, weight, long=False):
    """(theta draws [results, P] on the natural scale, sample_chain's output) of the end-to-end chain on the reference: ``pr`` holds the
    matrices, LB and data of the model under test, ``weight`` [n_obs] or None."""
    e = E2E
    lg = logpost_grad_obs(None if links is None else host.obs_model_spec(links, pr.D), weight, long=long)
    with np.errstate(all="ignore"):
        out = M.sample_chain(pr, None, None, None, e["results"], e["burnin"], seed=e["seed"], chain=0, stale_cache=False, max_tree_depth=e["max_tree_depth"],
                             initial=(Xhat_init, sig_pre0, th_pre0), logpost_grad=lg)
    return np.log(1.0 + np.exp(out[2])), out


@functools.lru_cache(maxsize=None)
def e2e_twin():
    """The end-to-end problem with the ORACLE's matrix build and initial values (the device builds its own from the same data): what
    tests/test_obs_cpu.py holds to the knife-edge condition.  Returns (orc.Problem, Xhat_init, sig_pre0, th_pre0, weights [n_obs])."""
    I, X_obs, _, W = e2e_data()
    hp = orc.hparams_initial(X_obs)
    C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], np.full(2, E2E["phi2"]), 2.01, bandsize=None)
    Xhat = orc.cubic_smoother(I, X_obs)
    links = host.obs_model_spec(E2E["links"], 2)
    LB, sig0 = host.link_sigma_defaults(links, X_obs, Xhat, W, orc.sigma_sqs_lower_bound(Xhat), hp["sigma_sqs"], False)
    idx = np.arange(X_obs.size)
    orc.DRIFTS["lotka_volterra"] = e2e_oracle_drift(I)
    pr = orc.Problem(I=I, mu=X_obs.mean(axis=0), C_inv=C_inv, m=m, K_inv=K_inv, N_ds=np.full(2, float(len(I))), obs_idx=idx, y=X_obs.reshape(-1), beta=1.0,
                     LB=LB, drift="lotka_volterra", P=4)
    sig_pre0, th_pre0 = host.softplus_inverse_inits(sig0, np.ones(4), LB)
    return pr, Xhat, sig_pre0, th_pre0, W.reshape(-1)
