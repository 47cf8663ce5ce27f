"""A re-used handle against a fresh one across every change of MODEL state (case tables and reference: tests/reuse_model_reference.py).

tests/test_reuse_gpu.py takes a handle through matrices, bands, problem data, times, batches and kernel families; each feature's own file
checks, on an engine built for that test, that set-then-unset equals never-set.  The drivers (predict, predict_many, SweepRunner) push
model after model into ONE engine: here one handle crosses the supports of theta, the priors (a fixed variance REPLACES an LB entry), the
observation model (dYobs rewritten in place, a weight plane that stays allocated), the matrices under a model, P under a model, the metric
buffers across capacity and P, the post-processing calls inside a paused run, a group re-initialised after its members changed, and the
direct-launch route of magi_sampler_run.  At every stop

  1. re-used == fresh, BIT FOR BIT: a second handle taken straight to the stop gives the same three-phase log posterior, the same fused one
     in even and odd slots, the same short NUTS run with its sampler_summary and sampler_elpd (both read tsup, prior, LB, links and weights
     from the handle) and the same fixed-L HMC run (_observe_model: tests/test_reuse_gpu.py's _observe, which ends on its HMC run, restated
     with the two post-processing calls behind the NUTS run);
  2. fresh == reference (obs_reference.logpost_grad_obs under the stop's tables) at the project's bars: 1e-10 three-phase, 1e-9 fused;
  3. nothing is vacuous: every compared run has finite samples, >= 1 leapfrog per transition and, for HMC, the fixed L.

tests/test_reuse_model_cpu.py proves on the reference alone that the answer of the stop BEFORE each transition differs by >= 1000 x those
bars.  A bit difference here is a missing invalidation in csrc/ (DESIGN 4.2)."""
import numpy as np
import pytest

from magi_v2_amd import host
from tests import reuse_model_reference as R
from tests.test_reuse_gpu import _assert_same, _collect, _engine, _load, _refused, _run, _set_problem
from tests.test_structureless_gpu import _assert_close

pytestmark = pytest.mark.gpu

E_BADARG = -1
CFG12 = dict(num_burnin_steps=8, num_results=4, step_size=2e-3, max_tree_depth=5, stale_cache=0)          # the 12 transitions of the paused runs
IDS = lambda n: list(range(20, 20 + n))
S = R.stop_state


def _refused_arg(call):
    """MAGI_E_BADARG: the handle stays as it was."""
    from magi_v2_amd.engine import MagiHipError
    with pytest.raises(MagiHipError) as e:
        call()
    assert e.value.code == E_BADARG, str(e.value)


def _flat(x, prefix, out=None):
    """Nested dicts / tuples of arrays and numbers -> {dotted key: array}; None entries are left out."""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k, v in x.items():
            _flat(v, f"{prefix}.{k}", out)
    elif isinstance(x, (tuple, list)) and not (x and np.isscalar(x[0])):
        for k, v in enumerate(x):
            _flat(v, f"{prefix}.{k}", out)
    elif x is not None and not isinstance(x, str):
        out[prefix] = np.asarray(x)
    return out


def _post(eng, **sel):
    """sampler_summary and sampler_elpd (with the log-likelihood itself) of the finished run."""
    out = _flat(eng.sampler_summary(**sel), "summary")
    out.update(_flat(eng.sampler_elpd(loglik=True, **sel), "elpd"))
    assert np.isfinite(out["summary.X.mean"]).all() and np.isfinite(out["summary.sigma_sqs.mean"]).all() and np.isfinite(out["summary.thetas.mean"]).all()
    assert np.isfinite(out["elpd.loglik"]).all() and out["elpd.n_nonfinite"] == 0 and out["summary.n_nonfinite"] == 0
    return out


def _honest(run, hmc_L=None):
    """No vacuous equality: finite samples and state, a leapfrog in every transition, the fixed L of an HMC run."""
    for k in ("X", "sig_pre", "th_pre", "state.X", "state.sig_pre", "state.th_pre", "state.step_size", "diag.step_size"):
        assert np.isfinite(run[k]).all(), k
    lf = run["diag.leapfrogs_taken"]
    assert lf.min() >= 1 and (hmc_L is None or (lf == hmc_L).all())
    return run


def _observe_model(eng, st, n):
    args = st.states(n)
    out = {}
    eng.set_option("fused_parity", 0)
    for tag, kw in (("three", {}), ("even", dict(fused=True))):
        out.update(zip((f"{tag}.L", f"{tag}.gX", f"{tag}.gs", f"{tag}.gt"), eng.logpost_grad(*args, R.TEMP, **kw)))
    eng.set_option("fused_parity", 1)
    out.update(zip(("odd.L", "odd.gX", "odd.gs", "odd.gt"), eng.logpost_grad(*args, R.TEMP, fused=True)))
    eng.set_option("fused_parity", 0)
    out.update({"nuts." + k: v for k, v in _honest(_run(eng, st, n, R.NUTS)).items()})
    out.update({"nuts." + k: v for k, v in _post(eng).items()})
    out.update({"hmc." + k: v for k, v in _honest(_run(eng, st, n, R.HMC), R.HMC["hmc_leapfrogs"]).items()})
    return out


def _apply(eng, st, order="support"):
    """The model of a stop on a handle whose problem is set."""
    s = st.spec
    if order == "support":
        eng.set_theta_support(s["support"])
        eng.set_prior(s["sig_prior"], s["th_prior"])
        eng.set_obs_model(s["link"], s["weight"])
    else:
        eng.set_obs_model(s["link"], s["weight"])
        eng.set_prior(s["sig_prior"], s["th_prior"])
        eng.set_theta_support(s["support"])


def _assert_model(eng, st):
    """The getters return the stop's tables."""
    pr, s = st.pr, st.spec
    kinds, bounds = eng.theta_support()
    want = host.theta_support(s["support"], pr.P)
    assert np.array_equal(kinds, want[0]) and np.array_equal(bounds, want[1]), (st.name, kinds, bounds)
    got_s, got_t = eng.prior()
    for got, ref in ((got_s, host.prior_spec(s["sig_prior"], pr.D, "sigma_sq")), (got_t, host.prior_spec(s["th_prior"], pr.P, "theta"))):
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), (st.name, got, ref)
    links, w = eng.obs_model()
    assert np.array_equal(links, host.obs_model_spec(s["link"], pr.D)), (st.name, links)
    assert np.array_equal(w, np.ones(len(pr.obs_idx)) if s["weight"] is None else s["weight"]), st.name


def _raw_set_support(eng, spec, P):
    from magi_v2_amd.engine import _dp, _ip
    kinds, bounds = host.theta_support(spec, P)
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    return eng._lib.magi_set_theta_support(eng._h, int(P), kinds.ctypes.data_as(_ip), bounds.ctypes.data_as(_dp))


def _raw_set_prior(eng, sig_spec, th_spec, D, P):
    """magi_set_prior itself: the engine's wrapper checks the theta priors against the supports before it calls."""
    from magi_v2_amd.engine import _dp, _ip
    ks, as_, bs = host.prior_spec(sig_spec, D, "sigma_sq")
    kt, at, bt = host.prior_spec(th_spec, P, "theta")
    kinds = np.ascontiguousarray(np.concatenate([ks, kt]), dtype=np.int32)
    a, b = np.ascontiguousarray(np.concatenate([as_, at])), np.ascontiguousarray(np.concatenate([bs, bt]))
    return eng._lib.magi_set_prior(eng._h, int(D + P), kinds.ctypes.data_as(_ip), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp))


def _move(eng, old, new, order):
    """old's model -> new's on a live handle by set_theta_support, set_prior and set_obs_model alone.  Support first: where new's support
    does not allow a theta prior old installed, the library refuses it (asserted, nothing changed) until the theta priors are flat."""
    s = new.spec
    if order == "support":
        if not R.prior_allowed(old.spec["th_prior"], s["support"], new.pr.P):
            _refused_arg(lambda: eng.set_theta_support(s["support"]))
            _assert_model(eng, old)
            eng.set_prior(old.spec["sig_prior"], None)
        eng.set_theta_support(s["support"])
        eng.set_prior(s["sig_prior"], s["th_prior"])
        eng.set_obs_model(s["link"], s["weight"])
    else:
        eng.set_obs_model(s["link"], s["weight"])
        eng.set_prior(s["sig_prior"], s["th_prior"])
        eng.set_theta_support(s["support"])


_fresh = {}


def _fresh_model(stop, n, family="auto"):
    """_observe_model of a handle taken straight to the stop, held to the reference (log posterior); once per session, read-only."""
    key = (stop, n, family)
    if key not in _fresh:
        st = S(stop)
        eng = _engine(st, {"stream_family": family})
        try:
            _load(eng, st)
            _apply(eng, st)
            _assert_model(eng, st)
            obs = _observe_model(eng, st, n)
            kernel = eng.stream_kernel_name(n)
        finally:
            eng.close()
        X, sp, tp = st.states(n)
        fn = st.reference()
        for c in range(n):
            truth = fn(X[c], sp[c], tp[c], R.TEMP, st.pr)
            _assert_close([obs[f"three.{f}"][c] for f in ("L", "gX", "gs", "gt")], truth, 1e-10, f"{stop.name} fresh {kernel} three-phase {c}/{n}")
            _assert_close([obs[f"even.{f}"][c] for f in ("L", "gX", "gs", "gt")], truth, 1e-9, f"{stop.name} fresh {kernel} fused {c}/{n}")
        _fresh[key] = obs
    return _fresh[key]


def _check(eng, st, what, batches=R.PAIR):
    for n, family in batches:
        eng.set_option("stream_family", family)
        _assert_same(_observe_model(eng, st, n), _fresh_model(st.stop, n, family), f"{what}: {st.name}, {n} states, {family}")


# ---- 1: the model walk ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["support", "obs"])
def test_model_walk_on_one_problem(order):
    """B129 at band 20: M0 -> M1 -> M2 -> M3 -> M4 -> M0 -> M2 with no set_problem in between, once as (support, prior, obs model) and
    once as (obs model, prior, support).  M2 -> M3 moves the fixed variance from component 2 to component 0 (LB[2] returns from lb_orig),
    M3 -> M4 leaves the tables allocated and unused and the weight plane rewritten, M0 -> M2 returns to tables that were in force before.
    The two orders the library refuses -- M3's real support over M2's installed lognormal prior, M2's lognormal prior under M3's real
    support -- are MAGI_E_BADARG and change nothing."""
    stops = [S(s) for s in R.HISTORIES["1 model walk"]]
    m = R.MODELS
    eng = _engine(stops[0])
    try:
        _load(eng, stops[0])
        _check(eng, stops[0], f"walk[{order}] 0")
        for k, (old, new) in enumerate(zip(stops[:-1], stops[1:]), 1):
            _move(eng, old, new, order)
            _refused(lambda: eng.sampler_run(1))
            _assert_model(eng, new)
            if new.stop.model == "M2":
                _refused_arg(lambda: eng.set_theta_support(m["M3"]["support"][5]))
            if new.stop.model == "M3":
                assert _raw_set_prior(eng, m["M2"]["sig_prior"], m["M2"]["th_prior"][5], 4, 5) == E_BADARG
            _assert_model(eng, new)
            _check(eng, new, f"walk[{order}] {k}")
    finally:
        eng.close()


# ---- 2: matrices under a model ----------------------------------------------------------------------------------------------------------

def _model_calls_refused(eng, st):
    """Between a matrix change of another shape and set_problem: the three model calls and their getters return MAGI_E_STATE."""
    s = st.spec
    _refused(lambda: eng.set_theta_support(s["support"]))
    _refused(lambda: eng.set_prior(s["sig_prior"], s["th_prior"]))
    _refused(lambda: eng.set_obs_model(s["link"], s["weight"]))
    _refused(eng.theta_support)
    _refused(eng.prior)
    _refused(eng.obs_model)


def _built_under_m2(eng, st, fresh):
    """build_matrices from the golden hyper-parameters on a B41 handle, M2 set before the build (re-used) or after it and a set_problem
    (fresh) -> the three-phase and the fused log posterior of two states."""
    x = st.extra
    eng.set_option("stream_family", "auto")
    if fresh:
        eng.build_matrices(x["I"], x["phi1s"], x["phi2s"], 2.01, want_host=False)
        _set_problem(eng, st)
        _apply(eng, st)
    else:
        _apply(eng, st)
        eng.build_matrices(x["I"], x["phi1s"], x["phi2s"], 2.01, want_host=False)
        _refused(lambda: eng.sampler_run(1))
    _assert_model(eng, st)
    out = {}
    for tag, kw in (("three", {}), ("even", dict(fused=True))):
        out.update(zip((f"{tag}.L", f"{tag}.gX", f"{tag}.gs", f"{tag}.gt"), eng.logpost_grad(*st.states(2), R.TEMP, **kw)))
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def test_matrices_change_under_a_model():
    """M2 in force on B129.  What include/magi_hip.h (magi_set_matrices) says a matrix change does to the model:
    set_matrices with other values of the SAME shape forgets the problem -- the model calls and their getters return MAGI_E_STATE until
    set_problem, which resets every table; with M2 set again the handle equals a fresh one given the new matrices, set_problem and M2.
    pack_resident dense -> 20 -> dense KEEPS the model: supports, priors with the fixed variance in LB's place, links, weights and the
    transformed data equal that fresh handle's.  Then the shape B129 -> B41 -> B129: MAGI_E_STATE until set_problem, a fresh M0 after it;
    on B41 build_matrices at the unchanged shape keeps a model as pack_resident does.  Then M2 under another n_obs."""
    h = [S(s) for s in R.HISTORIES["2 matrices under a model"]]
    eng = _engine(h[0])
    try:
        _load(eng, h[0])
        _apply(eng, h[0])
        _check(eng, h[0], "M2 on B129")
        eng.set_matrices(*h[1].matrices, bandsize=None)
        _refused(lambda: eng.sampler_run(1))
        _model_calls_refused(eng, h[0])
        _set_problem(eng, h[1])
        _assert_model(eng, S(R.Stop("B129v", None, "sirw", "M0")))              # (set_problem has reset every table)
        _apply(eng, h[1])
        _check(eng, h[1], "set_matrices, same shape")
        for k in (2, 3):
            eng.pack_resident(h[k].band)
            _refused(lambda: eng.sampler_run(1))
            _assert_model(eng, h[k])
            _check(eng, h[k], f"pack_resident -> {h[k].band}")
        for k in (4, 5):
            eng.set_matrices(*h[k].matrices, bandsize=None)
            _model_calls_refused(eng, h[0])
            _set_problem(eng, h[k])
            _assert_model(eng, h[k])                                          # (M0)
            _check(eng, h[k], f"shape -> {h[k].stop.base}")
            if k == 4:
                b41 = S(R.Stop("B41", None, "sirw", "M2"))
                fresh = _engine(b41)
                try:
                    _assert_same(_built_under_m2(eng, b41, False), _built_under_m2(fresh, b41, True), "build_matrices at an unchanged shape under M2")
                finally:
                    fresh.close()
        _set_problem(eng, h[6])
        _refused_arg(lambda: eng.set_obs_model(h[0].spec["link"], h[0].spec["weight"]))       # (the weights of the earlier n_obs)
        _assert_model(eng, S(R.Stop("B129-", None, "sirw", "M0")))
        _apply(eng, h[6])
        _assert_model(eng, h[6])
        _check(eng, h[6], "M2 under another n_obs")
    finally:
        eng.close()


# ---- 3: P under a model -----------------------------------------------------------------------------------------------------------------

def test_parameter_count_changes_under_a_model():
    """B41: sirw (P = 5) under M1 -> set_problem(seir4, P = 3): the tables are reset, 5-entry tables are refused, 3-entry ones accepted;
    back to sirw, where the 3-entry tables are refused.  (dim changes each time; at N = 41, D = 4 both round up to dimp = 176.)"""
    h = [S(s) for s in R.HISTORIES["3 P under a model"]]
    m1 = R.MODELS["M1"]
    eng = _engine(h[0])
    try:
        _load(eng, h[0])
        _apply(eng, h[0])
        _check(eng, h[0], "sirw under M1")
        _set_problem(eng, h[1])
        _refused(lambda: eng.sampler_run(1))
        _assert_model(eng, h[1])
        assert _raw_set_support(eng, m1["support"][5], 5) == E_BADARG
        assert _raw_set_prior(eng, m1["sig_prior"], m1["th_prior"][5], 4, 5) == E_BADARG
        _assert_model(eng, h[1])
        _check(eng, h[1], "seir4, tables reset")
        _apply(eng, h[2])
        _assert_model(eng, h[2])
        _check(eng, h[2], "seir4 under 3-entry M1")
        _set_problem(eng, h[3])
        _assert_model(eng, h[3])
        assert _raw_set_support(eng, m1["support"][3], 3) == E_BADARG
        assert _raw_set_prior(eng, m1["sig_prior"], m1["th_prior"][3], 4, 3) == E_BADARG
        _check(eng, h[3], "back to sirw")
    finally:
        eng.close()


# ---- 4: the metric's lifecycle ----------------------------------------------------------------------------------------------------------

def _metric(tag, n, st):
    return R.metric_arrays(tag, n, len(st.pr.I), st.pr.D, st.pr.P)


def _init(eng, st, n, cfg_kw):
    eng.sampler_init(eng.default_cfg(**cfg_kw), *st.states(n), seed=R.SEED, chain_ids=IDS(n))


def _with_metric(eng):
    out = _honest(_collect(eng))
    out.update(zip(("metric.X", "metric.sig", "metric.th"), eng.sampler_metric()))
    return out


def _adapted_run(eng, st):
    """Nine chains: a window over the first 8 of 12 transitions -> the metric, dual averaging restarted with 3 adaptation steps left."""
    _init(eng, st, 9, CFG12)
    assert all((a == 1.0).all() for a in eng.sampler_metric())
    eng.sampler_metric_window(True)
    eng.sampler_run(8)
    ss, kept = eng.sampler_adapt_metric(8, restart_adapt_steps=3)
    assert kept < 9 and np.isfinite(ss).all()                                 # (a chain that never moved in the window keeps its metric)
    eng.sampler_run(4)
    out = _with_metric(eng)
    out["restart_step_size"] = ss
    assert not (out["metric.X"] == 1.0).all()
    return out


def _two_metrics_run(eng, st):
    """Metric A for 3 transitions, B from the fourth on: replaced between two sampler_run calls, the graph kept."""
    _init(eng, st, 2, R.NUTS)
    eng.sampler_set_metric(*_metric("A", 2, st))
    eng.sampler_run(3)
    eng.sampler_set_metric(*_metric("B", 2, st))
    eng.sampler_run(4)
    return _with_metric(eng)


def _on_fresh(st, fn):
    eng = _engine(st)
    try:
        _load(eng, st)
        return fn(eng, st)
    finally:
        eng.close()


def _plain_run(n):
    def fn(eng, st):
        _init(eng, st, n, R.NUTS)
        eng.sampler_run(7)
        return _with_metric(eng)
    return fn


def _metric_c_run(eng, st):
    _init(eng, st, 2, R.NUTS)
    eng.sampler_set_metric(*_metric("C", 2, st))
    eng.sampler_run(7)
    return _with_metric(eng)


def test_metric_lifecycle_on_one_handle():
    """B41.  Two chains under a fixed metric; sampler_init with nine (capacity grows: the three metric buffers go with the chains), a
    window, adapt_metric with a restart (it overwrites the handle's n_adapt), the run finished; sampler_init with one chain and its own
    num_adaptation_steps: identity metric, no leftover n_adapt, sampler_metric all ones -- a fresh handle's run.  set_problem with the other
    P, a metric of that size, a run.  Then a window left open across sampler_init: adapt_metric is MAGI_E_STATE and the run a fresh
    handle's.  Then metric A replaced by B between two sampler_run calls with no graph drop."""
    st, st4 = S(R.Stop("B41", None, "sirw", "M0")), S(R.Stop("B41", None, "seir4", "M0"))
    eng = _engine(st)
    try:
        _load(eng, st)
        _init(eng, st, 2, R.NUTS)
        eng.sampler_set_metric(*_metric("A", 2, st))
        eng.sampler_run(7)
        _honest(_collect(eng))
        _assert_same(_adapted_run(eng, st), _on_fresh(st, _adapted_run), "nine chains adapted after two under a fixed metric")
        one = _plain_run(1)(eng, st)
        assert all((one[k] == 1.0).all() for k in ("metric.X", "metric.sig", "metric.th"))
        _assert_same(one, _on_fresh(st, _plain_run(1)), "one chain after an adapted run")
        _set_problem(eng, st4)
        _assert_same(_metric_c_run(eng, st4), _on_fresh(st4, _metric_c_run), "a metric under the other P")
        _set_problem(eng, st)
        _init(eng, st, 2, R.NUTS)
        eng.sampler_metric_window(True)
        eng.sampler_run(3)
        _init(eng, st, 2, R.NUTS)
        _refused(lambda: eng.sampler_adapt_metric(3))
        eng.sampler_run(7)
        _assert_same(_with_metric(eng), _on_fresh(st, _plain_run(2)), "sampler_init over an open window")
        _assert_same(_two_metrics_run(eng, st), _on_fresh(st, _two_metrics_run), "metric replaced between two runs")
    finally:
        eng.close()


# ---- 5: post-processing against a paused run --------------------------------------------------------------------------------------------

PAUSED = R.Stop("B41", None, "sirw", "M2")
_whole = {}


def _model_engine(st):
    eng = _engine(st)
    _load(eng, st)
    _apply(eng, st)
    return eng


def _whole_run():
    """The uninterrupted 12 transitions of two chains on a fresh handle; once per session, read-only."""
    if "run" not in _whole:
        st = S(PAUSED)
        eng = _model_engine(st)
        try:
            _init(eng, st, 2, CFG12)
            eng.sampler_run(12)
            _whole["run"] = _honest(_collect(eng))
        finally:
            eng.close()
    return _whole["run"]


def _pause_call(eng, call, st):
    """One post-processing call with small inputs of its own -> its outputs, flattened."""
    x = st.extra
    I, phi1, phi2, N, D, P = x["I"], x["phi1s"], x["phi2s"], len(st.pr.I), st.pr.D, st.pr.P
    rng = np.random.default_rng(17)
    t_new = np.array([-0.1, 0.02, 0.5, 1.234, float(I[-1]) + 0.3])
    x0, th = 0.2 + 0.1 * rng.random((4, D)), 0.5 + 0.5 * rng.random((4, P))
    t_out = np.linspace(0.0, 1.0, 6)
    if call == "summarize":
        out = eng.summarize(rng.standard_normal((2, 8, 5)))
    elif call == "elpd":
        out = eng.elpd(-1.0 + 0.3 * rng.standard_normal((2, 50, 7)))
    elif call == "gp_predict":
        out = eng.gp_predict(I, phi1, phi2, st.pr.mu, t_new, st.batch[0][:3])
    elif call == "matern_cross":
        out = eng.matern_cross(t_new, I, float(phi1[0]), float(phi2[0]))
    elif call == "ode_solve_rk4":
        out = eng.ode_solve(x0, th, t_out, drift="sirw")
    elif call == "ode_solve_adaptive":
        out = [eng.ode_solve(x0, th, t_out, drift="sirw", method=m, rtol=1e-6, atol=1e-9) for m in ("dopri5", "ros23")]
    elif call == "dense_apply":
        out = [eng.dense_apply(w, rng.standard_normal((D, N, 2)), transpose=t) for w, t in (("m", False), ("K_inv", True))]
    elif call == "theta_init":
        out = eng.theta_init("sirw", x["Xhat_init"], st.pr.mu, 20, want_trace=True)
    else:
        assert call == "fit_hparams"
        X = x["Xhat_init"]
        hp = host.hparams_initial(X)
        pri = [host.fourier_phi2_prior(X[:, d]) for d in range(D)]
        out = eng.fit_hparams(I, X, X.mean(axis=0), [p[0] for p in pri], [p[1] for p in pri], hp["sigma_sqs"], hp["phi1s"], hp["phi2s"], hp["sigma_sqs"],
                              num_iters=3, want_trace=True)
    return _flat(out, call)


@pytest.mark.parametrize("call", sorted(R.PAUSE_CALLS))
def test_post_processing_call_inside_a_paused_run(call):
    """A NUTS run of 12 transitions paused after 5; one call; the remaining 7.  include/magi_hip.h (magi_sampler_run) says for every one of
    these calls that the continued run is the uninterrupted one bit for bit (R.PAUSE_CALLS restates it; a call listed "refused" would have
    to end the run with MAGI_E_STATE).  The call's own outputs equal those of a handle that never sampled (the Adam loop of fit_hparams
    aside: finite)."""
    from magi_v2_amd.engine import MagiHipError
    st = S(PAUSED)
    whole = _whole_run()
    eng = _model_engine(st)
    try:
        _init(eng, st, 2, CFG12)
        eng.sampler_run(5)
        assert list(eng.sampler_steps_done()) == [5, 5]
        got = _pause_call(eng, call, st)
        try:
            eng.sampler_run(7)
            outcome = "continues"
        except MagiHipError as e:
            assert e.code == -5, str(e)
            outcome = "refused"
        assert outcome == R.PAUSE_CALLS[call]
        if outcome == "continues":
            _assert_same(_collect(eng), whole, f"run continued behind {call}")
    finally:
        eng.close()
    bare = _engine(st)
    try:
        _load(bare, st)
        ref = _pause_call(bare, call, st)
    finally:
        bare.close()
    assert not any(np.isnan(v).any() for v in got.values() if v.dtype.kind == "f"), call
    if call != "fit_hparams":
        _assert_same(got, ref, f"{call} inside a paused run against a handle that never sampled")


def test_post_processing_of_a_finished_run_repeats_and_leaves_it_alone():
    """After the 12 transitions: sampler_summary, sampler_elpd and sampler_gp_predict in two orders, twice each -- the same bits every time;
    samples, diagnostics and sampler state unchanged; a new sampler_init and run equals the fresh handle's."""
    st = S(PAUSED)
    x = st.extra
    t_new = np.array([-0.1, 0.02, 0.5, 1.234, float(x["I"][-1]) + 0.3])
    eng = _model_engine(st)
    calls = {"summary": lambda: _flat(eng.sampler_summary(), "s"), "elpd": lambda: _flat(eng.sampler_elpd(loglik=True), "e"),
             "gp": lambda: _flat(eng.sampler_gp_predict(x["I"], x["phi1s"], x["phi2s"], t_new, return_draws=True), "g")}
    try:
        _init(eng, st, 2, CFG12)
        eng.sampler_run(12)
        before = _collect(eng)
        _assert_same(before, _whole_run(), "the run itself")
        first = {}
        for name in ("summary", "elpd", "gp", "summary", "elpd", "gp", "gp", "elpd", "summary", "gp", "elpd", "summary"):
            got = calls[name]()
            assert np.isfinite(got[{"summary": "s.X.mean", "elpd": "e.loglik", "gp": "g.X_draws"}[name]]).all()
            _assert_same(got, first.setdefault(name, got), f"{name} repeated")
        _assert_same(_collect(eng), before, "samples, diagnostics and state behind the post-processing calls")
        _init(eng, st, 2, CFG12)
        eng.sampler_run(12)
        _assert_same(_collect(eng), _whole_run(), "a new run behind the post-processing calls")
    finally:
        eng.close()


# ---- 6: a group re-initialised ----------------------------------------------------------------------------------------------------------

_member = {}


def _member_run(stop, per):
    """A fresh handle of a member at a stop: NUTS on its first ``per`` states, with summary and elpd; once per session, read-only."""
    key = (stop, per)
    if key not in _member:
        st = S(stop)
        eng = _model_engine(st)
        try:
            out = _honest(_run(eng, st, per, R.NUTS))
            out.update(_post(eng))
            _member[key] = out
        finally:
            eng.close()
    return _member[key]


def _group_run(g, sts, per):
    states = [np.concatenate([st.states(per)[k] for st in sts]) for k in range(3)]
    g.sampler_init(g.default_cfg(**R.NUTS), *states, seed=R.SEED, chain_ids=IDS(per) * len(sts))
    g.sampler_run(R.NUTS["num_burnin_steps"] + R.NUTS["num_results"])
    return _collect(g)


def _assert_members(g, got, stops, per, what):
    for m, stop in enumerate(stops):
        fresh = _member_run(stop, per)
        mine = {k: v[m * per:(m + 1) * per] for k, v in got.items()}
        mine.update(_post(g, member=m))
        _assert_same(mine, fresh, f"{what}: member {m} ({stop.name}), {per} chains each")


def test_group_reinitialised_after_its_members_changed():
    """Two B41 members, member 0 under M2: init and run with one and with two chains each.  Then member 0 moves M2 -> M3 and member 1 gets
    other matrices of the same shape by set_matrices, which forgets its problem: the group refuses to initialise until that member's
    set_problem.  Then the SAME group initialised again: every member's chains, its sampler_summary and its sampler_elpd are those of a
    fresh handle of that member."""
    from magi_v2_amd.engine import MagiGroup
    h0, h1 = R.HISTORIES["6 group member 0"], R.HISTORIES["6 group member 1"]
    sts = [S(h0[0]), S(h1[0])]
    engs = [_model_engine(st) for st in sts]
    g = MagiGroup(engs)
    try:
        for per in (1, 2):
            _assert_members(g, _group_run(g, sts, per), [h0[0], h1[0]], per, "group")
        _move(engs[0], S(h0[0]), S(h0[1]), "support")
        engs[1].set_matrices(*S(h1[1]).matrices, bandsize=None)
        sts = [S(h0[1]), S(h1[1])]
        _refused_arg(lambda: _group_run(g, sts, 2))
        _set_problem(engs[1], sts[1])
        _assert_model(engs[0], sts[0])
        _assert_members(g, _group_run(g, sts, 2), [h0[1], h1[1]], 2, "group re-initialised")
    finally:
        g.close()
        for e in engs:
            e.close()


# ---- 7: direct launches -----------------------------------------------------------------------------------------------------------------

def test_direct_launches_equal_graph_replay(stream_family):
    """Option no_graph: magi_sampler_run launches the leapfrog slots directly.  One, two and five chains on B41 under M2 -- k_stream<1>,
    k_stream<2> (twice) under "auto", the matrix-core kernel under "mc" -- equal the graph replay bit for bit."""
    st = S(PAUSED)
    eng = _model_engine(st)
    try:
        for n in (1, 2, 5):
            want = {"auto": {1: "k_stream<1>", 2: "k_stream<2>", 5: "k_stream<2>"}[n], "mc": "k_stream_sep<CW=8>"}[stream_family]
            assert eng.stream_kernel_name(n) == want
            eng.set_option("no_graph", 0)
            graph = _honest(_run(eng, st, n, R.NUTS))
            eng.set_option("no_graph", 1)
            _assert_same(_honest(_run(eng, st, n, R.NUTS)), graph, f"direct launches, {n} chains, {stream_family}")
    finally:
        eng.close()


def test_direct_launches_toggled_inside_a_run_and_on_a_group():
    """no_graph switched on, and off, between two sampler_run calls of one paused run: the run continues unchanged.  A group of two B41
    members launched directly equals its graph replay."""
    from magi_v2_amd.engine import MagiGroup
    st = S(PAUSED)
    whole = _whole_run()
    eng = _model_engine(st)
    try:
        for first in (0, 1):
            eng.set_option("no_graph", first)
            _init(eng, st, 2, CFG12)
            eng.sampler_run(5)
            eng.set_option("no_graph", 1 - first)
            eng.sampler_run(7)
            _assert_same(_collect(eng), whole, f"no_graph {first} -> {1 - first} inside a run")
    finally:
        eng.close()
    sts = [S(PAUSED), S(R.Stop("B41", None, "sirw", "M0"))]
    engs = [_model_engine(s) for s in sts]
    g = MagiGroup(engs)
    try:
        assert g.stream_kernel_name(4) == "k_stream_group<2>"
        graph = _honest(_group_run(g, sts, 2))
        g.set_option("no_graph", 1)
        _assert_same(_honest(_group_run(g, sts, 2)), graph, "group, direct launches")
    finally:
        g.close()
        for e in engs:
            e.close()
