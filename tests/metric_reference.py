"""Reference of the diagonal-metric sampler (csrc: DevChains::scale / macc, metric.hip; include/magi_hip.h: magi_sampler_set_metric ...).

HMC with M^-1 = diag(s^2) on q is HMC with the identity metric on z = q / s, so the reference is the ORACLE's own transition --
``orc.nuts_one_step`` / ``orc.hmc_one_step``, untouched -- driven in whitened space: state z, ``fn(z) = (L(s z), s grad L(s z))``, the cached
gradient s g, the same Philox draws.  ``sample_chain`` below restates ``orc.sample_chain``'s loop around it (temperature schedule, stale
cache, dual averaging) and adds what the device adds: the metric switching at given transitions, window sums with the device's shift,
the regularised variances with their relative floor, the step-size rule and the restart of dual averaging.

Between transitions the chain is kept in q (as the device keeps it): z = q / s going in, q = s z coming out.  With s = 1 both are exact,
and the loop is ``orc.sample_chain``'s bit for bit (tests/test_metric_cpu.py)."""
import contextlib
import functools
import zlib

import numpy as np

from oracle import magi_oracle as orc

KAPPA, REL_FLOOR = 5.0, 1e-3


def pack_metric(inv_mass_X, inv_mass_sig, inv_mass_th):
    """s = sqrt(inverse mass) in the oracle's packed state order, from the host layouts ([N, D], [D], [P])."""
    return np.sqrt(orc.pack(np.asarray(inv_mass_X, dtype=np.float64), np.asarray(inv_mass_sig, dtype=np.float64), np.asarray(inv_mass_th, dtype=np.float64)))


def unpack_inv_mass(s, N, D, P):
    X, sg, th = orc.unpack(s * s, N, D, P)
    return np.ascontiguousarray(X), sg.copy(), th.copy()


def whitened_fn(fn_L, pos_scale, grad_scale=None):
    """fn(z) = (L(a z), b grad L(a z)); the metric s is a = b = s.  A device that applied s to one of its two updates only is a = 1, b = s
    (momentum update only) or a = s, b = 1 (position update only): the sensitivity cases of tests/test_metric_cpu.py."""
    a = pos_scale
    b = pos_scale if grad_scale is None else grad_scale

    def fn(z):
        L, g = fn_L(a * z)
        return L, b * g
    return fn


def window_sums(states, shift):
    """(S1, S2) of the device's window: sums of (q - c) and (q - c)^2 over the states, c = the state at the window's start."""
    d = np.asarray(states) - shift[None]
    return d.sum(axis=0), (d * d).sum(axis=0)


def metric_from_sums(S1, S2, n, kappa=KAPPA, rel_floor=REL_FLOOR):
    """(s, var, med) of metric.hip: var = (S2 - S1^2 / n) / (n - 1) clipped at 0, med = numpy.median(var), inverse mass
    n / (n + kappa) var + kappa / (n + kappa) rel_floor med, s its square root; s is None when med is not > 0 (the metric is kept)."""
    var = np.maximum((S2 - S1 * S1 / n) / (n - 1.0), 0.0)
    med = float(np.median(var))
    if not med > 0.0 or not np.isfinite(var).all():
        return None, var, med
    v = n / (n + kappa) * var + kappa / (n + kappa) * rel_floor * med
    return np.sqrt(v), var, med


def restart_step_size(eps_old, s_old, s_new):
    """The step along the stiffest coordinate is kept: eps min(s) is what bounds a stable leapfrog step."""
    return eps_old * float(np.min(s_old)) / float(np.min(s_new))


def sample_chain(pr, Xhat_init, sigma_sqs_init, thetas_init, num_results, num_burnin_steps, seed, chain=0, step_size=0.1, target_accept_prob=0.75,
                 max_tree_depth=10, min_temp=0.1, stale_cache=True, anneal=True, hmc_leapfrogs=None, max_energy_diff=1000.0, num_adaptation_steps=None,
                 logpost_grad=None, metric=None, windows=(), kappa=KAPPA, rel_floor=REL_FLOOR, restart=None, initial=None, trace=None, fork_at=None, resume=None):
    """``orc.sample_chain`` under a diagonal metric.

    ``metric``: {transition index k: s} -- from transition k on the metric is s (a packed vector of sqrt inverse masses, ``pack_metric``;
    None = identity; a pair (a, b) = the mis-applied metric of ``whitened_fn``).
    ``windows``: [(start, stop)] -- a window opens in front of transition ``start`` and its ``stop - start`` states become the metric
    behind transition ``stop - 1``; ``restart``: {stop: restart_adapt_steps} (default: the adaptation steps left, n_adapt - stop, as
    MagiEngine.sampler_warmup gives; a negative value leaves step size and dual averaging alone).
    ``initial``: (X0, sig_pre0, th_pre0) pre-transformed instead of the three *_init arguments.
    ``fork_at``: a transition index k -- ``extra["fork"]`` holds the chain as it stands behind transition k - 1, in front of a window's
    adaptation there; ``resume``: such a record -- the run starts at its transition with its state, metric and dual averaging (two
    continuations of one warm-up without running it twice).
    Returns (X_samps, sig_samps, th_samps, info, extra): the first four as ``orc.sample_chain`` (info additionally over ALL transitions
    under ``extra["all"]``), extra = dict(all, s: the final metric (None = identity), adapted: [dict(stop, s, var, med, step_size, states)],
    da: the final dual-averaging state, q: the final state)."""
    N, D, P = pr.N, pr.D, pr.P
    X0, s0, t0 = initial if initial is not None else orc.initial_state(Xhat_init, sigma_sqs_init, thetas_init, pr.LB)
    q = orc.pack(np.asarray(X0, dtype=np.float64), np.asarray(s0, dtype=np.float64), np.asarray(t0, dtype=np.float64))
    fn_L = orc.make_fn_L(pr, logpost_grad)
    L, gL = fn_L(q)
    num_adapt = int(0.8 * num_burnin_steps) if num_adaptation_steps is None else int(num_adaptation_steps)
    n_adapt0 = num_adapt               # (restarts count the adaptation steps left from the run's own total)
    da = orc.dual_averaging_init(step_size)
    total = num_burnin_steps + num_results
    out_q = np.zeros((num_results, q.shape[0]))
    keys = ("step_size", "log_accept_ratio", "leapfrogs", "depth", "has_divergence", "reach_max_depth", "target_log_prob", "energy", "is_accepted", "beta_temp")
    every = {k: [] for k in keys}
    metric = dict(metric or {})
    opens = {a: b for a, b in windows}
    closes = {b: a for a, b in windows}
    ones = np.ones_like(q)
    s_cur = None                       # identity
    win = None                         # (shift, [states]) of the open window
    adapted = []
    temp_prev = orc.temperature(0, min_temp) if anneal else 1.0
    fork, first = None, 0
    if resume is not None:
        first, q, L, gL, da, num_adapt, temp_prev, s_cur = (resume[f] for f in ("k", "q", "L", "gL", "da", "num_adapt", "temp_prev", "s"))
        for key in keys:
            every[key] = [np.nan] * first
    for k in range(first, total):
        if k in metric:
            s_cur = metric[k]
        if k in opens:
            win = (q.copy(), [])
        a, b = (ones, ones) if s_cur is None else s_cur if isinstance(s_cur, tuple) else (s_cur, s_cur)
        fz = whitened_fn(fn_L, a, b)
        temp = orc.temperature(k, min_temp) if anneal else 1.0
        tc = temp_prev if stale_cache else temp
        z = q / a
        if hmc_leapfrogs is None:
            res = orc.nuts_one_step(z, tc * L, tc * (b * gL), da.step_size, temp, fz, k, chain, seed, max_tree_depth=max_tree_depth, max_energy_diff=max_energy_diff)
        else:
            res = orc.hmc_one_step(z, tc * L, tc * (b * gL), da.step_size, temp, fz, k, chain, seed, hmc_leapfrogs, max_energy_diff=max_energy_diff)
        ss_used = da.step_size
        if res.is_accepted:
            q = a * res.q
            L, gL = fn_L(q)            # (the evaluation the transition made at a z: the same product, the same bits; gL un-whitened)
            temp_prev = temp
        else:
            temp_prev = tc
        da = orc.dual_averaging_update(da, res.log_accept_ratio, num_adapt, target_accept_prob)
        if trace is not None:
            trace.append((k, res, ss_used))
        row = dict(step_size=ss_used, log_accept_ratio=res.log_accept_ratio, leapfrogs=res.leapfrogs, depth=res.depth, has_divergence=res.has_divergence,
                   reach_max_depth=res.reach_max_depth, target_log_prob=res.target_log_prob, energy=res.energy, is_accepted=res.is_accepted, beta_temp=temp)
        for key in keys:
            every[key].append(row[key])
        if k >= num_burnin_steps:
            out_q[k - num_burnin_steps] = q
        if win is not None:
            win[1].append(q.copy())
        if fork_at == k + 1:
            fork = dict(k=k + 1, q=q.copy(), L=L, gL=gL.copy(), da=da, num_adapt=num_adapt, temp_prev=temp_prev, s=s_cur)
        if k + 1 in closes and win is not None:
            stop, n = k + 1, len(win[1])
            S1, S2 = window_sums(win[1], win[0])
            s_new, var, med = metric_from_sums(S1, S2, n, kappa, rel_floor)
            r = (restart or {}).get(stop, max(n_adapt0 - stop, 0))
            s_old = ones if s_cur is None else s_cur
            if r >= 0:
                da = orc.dual_averaging_init(da.step_size if s_new is None else restart_step_size(da.step_size, s_old, s_new))
                num_adapt = r
            if s_new is not None:
                s_cur = s_new
            adapted.append(dict(stop=stop, s=s_new, var=var, med=med, step_size=da.step_size, states=np.array(win[1]), shift=win[0]))
            win = None
    X_samps = out_q[:, : N * D].reshape(num_results, D, N).transpose(0, 2, 1)
    info = {key: np.asarray(v[num_burnin_steps:]) for key, v in every.items()}
    extra = dict(all={key: np.asarray(v) for key, v in every.items()}, s=s_cur, adapted=adapted, da=da, q=q, fork=fork)
    return X_samps, out_q[:, N * D: N * D + D], out_q[:, N * D + D:], info, extra


# ---- the whitening itself, against Stan's scheme in q-space (fixed-L HMC) -----------------------------------------------------------------

def hmc_one_step_qspace(q, cur_target, cur_grad, step_size, temp, fn_L, step, chain, key, num_leapfrog, s, max_energy_diff=1000.0):
    """One fixed-L HMC transition with M^-1 = diag(s^2) written the textbook way, in q: p ~ N(0, M) (= z / s with z the Philox normals),
    K = p^T M^-1 p / 2, p += eps/2 grad, q += eps M^-1 p.  Returns (accepted, q, energy, init_energy, target)."""
    import math
    Minv = s * s
    p = orc.rng_normal(q.shape[0], step, chain, key) / s
    init_energy = cur_target - 0.5 * np.dot(p, Minv * p)
    x, tgt, grd = q, cur_target, cur_grad
    for _ in range(num_leapfrog):
        p_half = p + 0.5 * step_size * grd
        x = x + step_size * (Minv * p_half)
        Lx, gLx = fn_L(x)
        tgt, grd = temp * Lx, temp * gLx
        p = p_half + 0.5 * step_size * grd
    energy = tgt - 0.5 * np.dot(p, Minv * p)
    if np.isnan(energy):
        energy = -np.inf
    ediff = energy - init_energy
    u = math.log1p(-orc.rng_uniform(0, step, chain, orc.STREAM_MERGE, key))
    accept = bool(u <= ediff) and bool(-ediff < max_energy_diff)
    return accept, (x if accept else q), (energy if accept else init_energy), init_energy, (tgt if accept else cur_target)


# ---- fixtures and the case table of tests/test_metric_cpu.py (conditions on this reference alone) and tests/test_metric_gpu.py ------------------


@functools.lru_cache(maxsize=None)
def seir_problem(N, band=None, dt=0.025):
    """(fixture {"Xhat_init", "sigma_sqs_init"}, orc.Problem with the reference's band mask, unmasked orc.Problem): SEIR-4 on
    tests/util.synthetic_seir_problem(N, dt=dt), oracle-built matrices with the reference's initial hyper-parameters.  Shared: read-only."""
    from tests.util import band_part_copy, synthetic_seir_problem
    I, X_obs, _, _ = synthetic_seir_problem(N, dt=dt)
    Xi = orc.linear_interpolate(X_obs)
    hp = orc.hparams_initial(Xi)
    C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], hp["phi2s"], 2.01, bandsize=None)
    N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
    idx = np.where(~np.isnan(X_obs).flatten())[0]
    Xhat = orc.cubic_smoother(I, Xi)
    mk = lambda b: orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=band_part_copy(C_inv, b), m=band_part_copy(m, b), K_inv=band_part_copy(K_inv, b), N_ds=N_ds,
                               obs_idx=idx, y=X_obs.reshape(-1)[idx], beta=float(4 * N / N_ds.sum()), LB=orc.sigma_sqs_lower_bound(Xhat), drift="seir4", P=3)
    return {"Xhat_init": Xhat, "sigma_sqs_init": hp["sigma_sqs"]}, mk(band), mk(None)


class MetricCase:
    """One row of the GPU table.  ``kind``: "seir" (seir_problem(N, band)) or "edge" (the spd fixture of a traced drift of
    magi_v2_amd.drift_examples.EDGE_EXAMPLES / EXAMPLES at N grid points); ``runs``: [(chains, stream_family)] -- the batches the device runs;
    chain ids 20 .. 20 + chains - 1, the first and the last compared.  cfg: the device's magi_sampler_cfg fields."""

    def __init__(self, name, kind, N, band, cfg, runs, drift="seir4", burnin=4, results=3, seed=808, dt=None, key=None, salts=None):
        self.name, self.kind, self.N, self.band, self.cfg, self.runs, self.drift = name, kind, N, band, dict(cfg), tuple(runs), drift
        self.burnin, self.results, self.seed = burnin, results, seed
        self.dt = 4.0 / (N - 1) if dt is None else dt          # "seir": grid spacing (default: the epidemic's four time units on every grid)
        self.key = key if key is not None else name            # names the case's metric draws (cases that share it share their metrics)
        self.salts = dict(salts or {})                         # chain -> which draw of its metric (default 0), chosen so that the conditions of
                                                               # tests/test_metric_cpu.py hold: a mis-applied metric shows in an integer diagnostic

    def __repr__(self):
        return self.name

    def chains(self):
        return sorted({20} | {20 + n - 1 for n, _ in self.runs})


_NUTS = dict(step_size=2e-3, max_tree_depth=6)
_ALL = ((1, "auto"), (2, "auto"), (3, "mc"), (9, "mc"))          # k_stream<1>, k_stream<2>, k_stream_sep<8>, k_stream_sep<16>
# Grid spacing, Philox seed and the draw of each chain's metric (``salts``) are chosen so that the trees of a case do not all end at the depth
# cap and every mis-application of the metric shows in an integer diagnostic (tests/test_metric_cpu.py asserts it per compared chain): at
# dt = 0.1 nearly every tree of the N = 41 chains has 63 leapfrogs with or without the metric.
CASES = [
    MetricCase("nuts_n41", "seir", 41, None, dict(_NUTS, stale_cache=0), _ALL, dt=0.07, salts={20: 5, 21: 3, 28: 6}),
    MetricCase("nuts_n41_stale", "seir", 41, None, dict(_NUTS, stale_cache=1), ((1, "auto"), (3, "mc")), dt=0.07, key="nuts_n41"),
    # (step 2e-4: at 2e-3, eight blind leapfrogs from theta_0 = 1 overflow exp() in the oracle and on the device alike -- nothing to compare)
    MetricCase("hmc_n41", "seir", 41, None, dict(step_size=2e-4, mode=1, hmc_leapfrogs=8, stale_cache=0), ((1, "auto"), (2, "auto"), (3, "mc")),
               salts={20: 4, 21: 11, 22: 19}),
    MetricCase("nuts_n161_b20", "seir", 161, 20, dict(_NUTS, stale_cache=0), ((1, "auto"), (3, "mc")), seed=2),
    MetricCase("nuts_ptrans_n41", "traced", 41, None, dict(_NUTS, stale_cache=0), ((3, "mc"),), drift="ptrans"),        # not separable: k_stream_mc
    MetricCase("nuts_chain8_n129", "edge", 129, None, dict(_NUTS, stale_cache=0), ((1, "auto"),), drift="chain8"),      # D = 8: eight component lanes
]


def case(name):
    return next(c for c in CASES if c.name == name)


def _inits(pr, X):
    """(sigma_sqs_init, thetas_init) of a structureless fixture: its nominal sigma_pre and parameters (tests/util.py)."""
    from tests.util import STRUCTURELESS_SIG_PRE, structureless_theta
    return np.log1p(np.exp(STRUCTURELESS_SIG_PRE)) + pr.LB, structureless_theta(pr.drift)


def case_problem(c):
    """(masked orc.Problem, unmasked orc.Problem, (X0, sig_pre0, th_pre0), traced Drift or None) of a case.  A traced drift's oracle entry
    is registered in ``orc.DRIFTS`` by the call (the tests' own fixtures remove theirs; "ptrans" stays, as tests/test_structureless_cpu.py
    leaves it)."""
    if c.kind == "seir":
        fx, pr, dense = seir_problem(c.N, c.band, c.dt)
        return pr, dense, orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), pr.LB), None
    if c.kind == "traced":
        from tests.test_structureless_cpu import fixture, register_traced
        pr, X = fixture(c.N, c.drift, spd=True)
        d = register_traced(c.drift, c.N)
    else:
        from tests import test_drift_edges_cpu as E
        assert c.N == E.N_FIX
        with E.edge_drifts():
            pr, X = E.fixture(c.drift, spd=True)
            sig0, th0 = _inits(pr, X)
        return pr, pr, orc.initial_state(X, sig0, th0, pr.LB), E.traced(c.drift)
    sig0, th0 = _inits(pr, X)
    return pr, pr, orc.initial_state(X, sig0, th0, pr.LB), d


def case_metric(c, chain):
    """The fixed metric of a chain of a case: inverse masses log-uniform in [0.3, 3]^2 per entry -- s in [0.3, 3], parameter entries
    included, another draw per chain.  Returns s in packed order."""
    pr = case_problem(c)[0]
    rng = np.random.default_rng([zlib.crc32(c.key.encode()), chain, 4711, c.salts.get(chain, 0)])
    return np.exp(rng.uniform(np.log(0.3), np.log(3.0), pr.N * pr.D + pr.D + pr.P))


def oracle_kwargs(c):
    kw = dict(step_size=c.cfg["step_size"], stale_cache=bool(c.cfg.get("stale_cache", 1)), seed=c.seed)
    if "num_adaptation_steps" in c.cfg:
        kw["num_adaptation_steps"] = c.cfg["num_adaptation_steps"]
    if c.cfg.get("mode", 0) == 1:
        kw["hmc_leapfrogs"] = c.cfg["hmc_leapfrogs"]
    else:
        kw["max_tree_depth"] = c.cfg["max_tree_depth"]
    return kw


_runs = {}


def case_run(c, chain, metric="fixed", **over):
    """sample_chain's output of one chain of a case under ``metric``: "fixed" (case_metric from transition 0), None (identity) or a
    {transition: s} table; computed once per session and shared (read-only) unless ``over`` changes other arguments."""
    key = (c.name, chain, metric if not isinstance(metric, dict) else None)
    if over or isinstance(metric, dict) or key not in _runs:
        pr, _, init, _ = case_problem(c)
        table = {0: case_metric(c, chain)} if metric == "fixed" else metric
        trace = []
        out = sample_chain(pr, None, None, None, c.results, c.burnin, chain=chain, initial=init, metric=table, trace=trace, **dict(oracle_kwargs(c), **over))
        if over or isinstance(metric, dict):
            return out, trace
        _runs[key] = (out, trace)
    return _runs[key]



@contextlib.contextmanager
def oracle_drifts(c):
    """The oracle's drift-table entry of a case's traced drift, for the duration (the EDGE_EXAMPLES are registered by their own fixture only)."""
    if c.kind == "edge":
        from tests import test_drift_edges_cpu as E
        with E.edge_drifts():
            yield
    else:
        yield


INT_FIELDS = (("tree_depth", "depth"), ("leapfrogs_taken", "leapfrogs"), ("has_divergence", "has_divergence"), ("reach_max_depth", "reach_max_depth"),
              ("is_accepted", "is_accepted"))
