"""Observation model on the device (magi_set_obs_model: log and square-root links, known observation weights) against tests/obs_reference.py.

Bars are the project's own: 1e-10 for the three-phase log posterior and gradient, 1e-9 for the fused form (even and odd slots bit for bit
equal), of the value, t3, t4 and of each gradient's largest entry; ``tests.util.BRANCH_TOL`` / ``ENERGY_TOL`` for sampler runs, every integer
diagnostic exact.  tests/test_obs_cpu.py holds the reference, the fixtures and the case table on the CPU: every named wrong implementation
would fail here."""
import ctypes as C

import numpy as np
import pytest

from magi_v2_amd import host
from magi_v2_amd.engine import MagiEngine, MagiHipError
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import obs_reference as OR
from tests import util as U
from tests.test_metric_gpu import _assert_chain, _cfg, _ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


# ---- log posterior and gradient ------------------------------------------------------------------------------------------------------------------

def _fixture_engine(fx, family):
    """The engine of a log-posterior fixture under its supports, priors and observation model (inside OR.fixture_drifts)."""
    from magi_v2_amd import drift as drift_mod
    from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES, TIME_EXAMPLES
    pr, w, _, _ = OR.logpost_build(fx)
    d = None if fx.kind == "builtin" else drift_mod.resolve(*(DOMAIN_EXAMPLES | TIME_EXAMPLES)[fx.drift])
    eng = U.engine_for(pr, fx.band, matrices=pr.unmasked if fx.band is not None else None, drift=d, options={"stream_family": family})
    if fx.support is not None:
        eng.set_theta_support(fx.support)
    if fx.sig_prior is not None:
        eng.set_prior(fx.sig_prior, None)
    eng.set_obs_model(list(fx.links), w)
    return eng


def _evaluate(eng, Xb, sp, tp, temp):
    """(three-phase, fused in an even slot, fused in an odd slot), each (logp, gX, gsig, gth, terms) with a leading state axis."""
    n = len(Xb)
    args = (Xb, sp, tp) if n > 1 else (Xb[0], sp[0], tp[0])
    lift = (lambda out: out) if n > 1 else (lambda out: tuple(np.asarray(a)[None] for a in out))
    eng.set_option("fused_parity", 0)
    three = lift(eng.logpost_grad(*args, temp, want_terms=True))
    even = lift(eng.logpost_grad(*args, temp, want_terms=True, fused=True))
    eng.set_option("fused_parity", 1)
    odd = lift(eng.logpost_grad(*args, temp, want_terms=True, fused=True))
    eng.set_option("fused_parity", 0)
    return three, even, odd


def _assert_state(got, i, ref, bar, what):
    fig = OR.figures((got[0][i], got[1][i], got[2][i], got[3][i], got[4][i][2], got[4][i][3]), ref)
    print(what, " ".join(f"{k} {v:.2e}" for k, v in fig.items()), f"(bar {bar:g})")
    for k, v in fig.items():
        assert v <= bar, (what, k, v, bar)


_KERNELS = {(1, "auto"): "k_stream<1>", (2, "auto"): "k_stream<2>", (3, "auto"): "k_stream<2>", (9, "auto"): "k_stream<2>"}


@pytest.mark.parametrize("fx", OR.LOGPOST, ids=repr)
def test_log_posterior_gradient_and_terms_match_the_reference(fx):
    """Structureless fixtures at N = 127, 129, 257 (states in (0.05, 0.3): both links defined; every operator block counts) under mixed links
    and weights in (0.25, 4) on a random half of the points: a component without observations, a band, a non-separable traced drift
    (k_stream_mc + point_block), a drift that uses t, a fixed sigma^2 on a linked and weighted component, a lower-bounded theta.  Batches of
    1, 2, 3 and 9 states on the VALU kernels and, with stream_family = mc, on the matrix-core ones.  Every state carries a negative entry at
    an unobserved point of a log-linked component: finite, and equal to the reference."""
    temp = 0.8
    with OR.fixture_drifts(fx):
        _, _, (Xb, sp, tp), _ = OR.logpost_build(fx)
        refs = [OR.reference_of(fx, i, temp) for i in range(len(Xb))]
        for family in sorted({f for _, f in fx.batches}):
            eng = _fixture_engine(fx, family)
            try:
                for n in sorted(b for b, f in fx.batches if f == family):
                    name = eng.stream_kernel_name(n)
                    if family == "auto":
                        assert name.startswith(_KERNELS[(n, "auto")]), name
                    elif n >= 3:
                        assert name.startswith("k_stream_mc" if fx.drift == "gompertz" else "k_stream_sep"), name
                    three, even, odd = _evaluate(eng, Xb[:n], sp[:n], tp[:n], temp)
                    for a, b in zip(even, odd):
                        np.testing.assert_array_equal(a, b, err_msg=f"{fx} {name}: fused, even against odd slot, {n} states")
                    for i in range(n):
                        assert np.isfinite(three[0][i]) and np.isfinite(even[0][i])
                        _assert_state(three, i, refs[i], 1e-10, f"{fx} {name} three-phase state {i}/{n}")
                        _assert_state(even, i, refs[i], 1e-9, f"{fx} {name} fused state {i}/{n}")
            finally:
                eng.close()


@pytest.mark.parametrize("family", ["auto", "mc"])
def test_a_state_outside_a_links_domain_is_nan_and_leaves_the_batch_untouched(family):
    """Batch of three on the N = 129 fixture: state 1 has x < 0 at an OBSERVED point of the log-linked component 0 (state 2: x < 0 at an
    observed point of the sqrt-linked component 2, in a second call).  Both forms return NaN for it; the other two states are what they are
    without it, to the bit.  (Negative at unobserved points only -- every state of the fixture -- is finite: the test above.)"""
    fx = OR.logpost_fixture("seir4_n129")
    _, _, (Xb, sp, tp), _ = OR.logpost_build(fx)
    Xb, sp, tp = Xb[:3], sp[:3], tp[:3]
    eng = _fixture_engine(fx, family)
    try:
        clean = _evaluate(eng, Xb, sp, tp, 0.8)
        for bad, comp in ((1, 0), (2, 2)):
            Xo = Xb.copy()
            Xo[bad, 4, comp] = -0.01                      # (even rows are observed)
            for form, ref in zip(_evaluate(eng, Xo, sp, tp, 0.8), clean):
                assert np.isnan(form[0][bad]) and np.isfinite(ref[0][bad])
                for i in set(range(3)) - {bad}:
                    for a, b in zip(form, ref):
                        np.testing.assert_array_equal(a[i], b[i])
    finally:
        eng.close()


# ---- sampler, draw for draw ----------------------------------------------------------------------------------------------------------------------

def _case_engine(c, family="auto", model=True, weights=True):
    pr, dense, _, w = OR.case_problem(c)
    eng = U.engine_for(dense, c.band, options={"stream_family": family})
    if model:
        eng.set_obs_model(list(OR.LINKS_SEIR4), w if weights else None)
    return eng


def _case_states(c, n):
    return tuple(np.repeat(np.asarray(v)[None], n, axis=0) for v in OR.case_problem(c)[2])


@pytest.mark.parametrize("c,chains,family", [(c, n, f) for c in OR.CASES if not c.warm for n, f in c.runs], ids=repr)
def test_sampler_matches_the_reference_draw_for_draw(c, chains, family):
    """The table of tests/obs_reference.py under links (log, identity, sqrt, log) and weights, annealing on: NUTS with trees of depth <= 6
    on k_stream<1>, <2>, k_stream_sep<8>, <16>; fixed-L HMC; N = 161 under band 20; and the domain case, whose trajectories cross 0 at an
    observed point of a log link behind an accepted proposal (the leaf counts as energy -inf).  Chain ids 20 ..., the first and the last
    compared: every integer diagnostic exact, floats within BRANCH_TOL / ENERGY_TOL."""
    ids = _ids(chains)
    eng = _case_engine(c, family)
    try:
        name = eng.stream_kernel_name(chains)
        assert name.startswith({1: "k_stream<1>", 2: "k_stream<2>"}.get(chains, "k_stream_sep")), name
        if chains in (3, 9):
            assert ("16" in name) == (chains == 9), name
        eng.sampler_init(_cfg(eng, c), *_case_states(c, chains), seed=c.seed, chain_ids=ids)
        lf, _ = eng.sampler_run(c.burnin + c.results)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert lf == d.leapfrogs_taken.sum()
    for i in sorted({0, chains - 1}):
        _assert_chain(f"{c.name} {name} chain {ids[i]}", i, d, samples, OR.case_run(c, ids[i])[0], c.burnin)


@pytest.mark.parametrize("chains", [1, 2])
def test_warmup_that_adapts_the_metric_matches_the_reference_under_the_model(chains):
    """sampler_warmup over warmup_schedule(40, 32, 8, 4, 8) on the N = 41 case (obs_reference.WARM): two windows become metrics, dual
    averaging restarts, then 13 more transitions, 5 of them results."""
    c, w = OR.case("warm_n41"), OR.WARM
    ids = _ids(chains)
    eng = _case_engine(c)
    try:
        eng.sampler_init(_cfg(eng, c, num_burnin_steps=w["burnin"], num_results=w["results"], max_tree_depth=w["max_tree_depth"]), *_case_states(c, chains),
                         seed=w["seed"], chain_ids=ids)
        _, _, windows = eng.sampler_warmup(host.warmup_schedule(*w["sched"]))
        eng.sampler_run(w["burnin"] + w["results"] - w["sched"][1])
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert [(x["start"], x["stop"]) for x in windows] == [(8, 12), (12, 24)]
    for i in sorted({0, chains - 1}):
        _assert_chain(f"warm-up chain {ids[i]}", i, d, samples, OR.case_run(c, ids[i])[0], w["burnin"])


def _assert_same_run(a, b):
    (sa, da), (sb, db) = a, b
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)
    for f in da.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(da, f), getattr(db, f), err_msg=f)


def _run_case(eng, c, chains, pieces=None):
    total = c.burnin + c.results
    eng.sampler_init(_cfg(eng, c), *_case_states(c, chains), seed=c.seed, chain_ids=_ids(chains))
    for n in (pieces or [total]):
        eng.sampler_run(n)
    return eng.sampler_samples(), eng.sampler_diag()


def test_pause_and_resume_across_the_domain_case_is_bit_identical_and_a_checkpoint_is_refused_under_another_model():
    """The domain case in one run, in runs of one transition each (a pause in front of and behind every transition with a leaf outside the
    domain), and resumed from a checkpoint on a fresh handle; the checkpoint is refused under other links, other weights and no model."""
    c = OR.case("domain_n41")
    total = c.burnin + c.results
    w = OR.case_problem(c)[3]
    eng = _case_engine(c)
    try:
        whole = _run_case(eng, c, 2)
        assert whole[1].has_divergence[0, 5] and whole[1].is_accepted[0, 5]          # (chain 20, transition 5: the census of tests/test_obs_cpu.py)
        _assert_same_run(whole, _run_case(eng, c, 2, [1] * total))
        eng.sampler_init(_cfg(eng, c), *_case_states(c, 2), seed=c.seed, chain_ids=_ids(2))
        eng.sampler_run(5)
        ck = eng.sampler_checkpoint()
    finally:
        eng.close()
    eng = _case_engine(c)
    try:
        eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=_ids(2))
        eng.sampler_run(total - 5)
        (sa, da), (sb, db) = whole, (eng.sampler_samples(), eng.sampler_diag())
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(da.leapfrogs_taken[:, 5:], db.leapfrogs_taken[:, 5:])
        np.testing.assert_array_equal(da.energy[:, 5:], db.energy[:, 5:])
        w2 = w.copy()
        w2[0] *= 2.0
        for links, wt in ((None, None), ([OR.LOG, OR.IDENTITY, OR.SQRT, OR.SQRT], w), (list(OR.LINKS_SEIR4), w2), (list(OR.LINKS_SEIR4), None)):
            eng.set_obs_model(links, wt)
            with pytest.raises(MagiHipError) as err:
                eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=_ids(2))
            assert err.value.code == -1
    finally:
        eng.close()


@pytest.mark.parametrize("per", [1, 2])
def test_group_members_with_different_models_equal_their_own_handles_bit_for_bit(per):
    """Two members of one shape on k_stream_group<1> and <2>: the case's links and weights, and (sqrt, log, identity, log) without weights."""
    c = OR.case("nuts_n41")
    w = OR.case_problem(c)[3]
    models = [(list(OR.LINKS_SEIR4), w), (["sqrt", "log", None, "log"], None)]
    start = _case_states(c, per)
    ids = _ids(per)
    own = []
    for links, wt in models:
        eng = _case_engine(c, model=False)
        try:
            eng.set_obs_model(links, wt)
            eng.sampler_init(_cfg(eng, c), *start, seed=c.seed, chain_ids=ids)
            eng.sampler_run(c.burnin + c.results)
            own.append((eng.sampler_samples(), eng.sampler_diag()))
        finally:
            eng.close()
    engs = [_case_engine(c, model=False) for _ in models]
    try:
        for e, (links, wt) in zip(engs, models):
            e.set_obs_model(links, wt)
        g = MagiEngine.group(engs)
        try:
            with pytest.raises(MagiHipError) as err:
                g.set_obs_model("log", None)
            assert err.value.code == -5
            both = [np.concatenate([v, v]) for v in start]
            g.sampler_init(_cfg(g, c), *both, seed=c.seed, chain_ids=ids + ids)
            g.sampler_run(c.burnin + c.results)
            samples, d = g.sampler_samples(), g.sampler_diag()
        finally:
            g.close()
    finally:
        for e in engs:
            e.close()
    assert own[0][1].energy.tolist() != own[1][1].energy.tolist()
    for m in range(2):
        sl = slice(m * per, (m + 1) * per)
        for a, b in zip(samples, own[m][0]):
            np.testing.assert_array_equal(a[sl], b)
        for f in d.__dataclass_fields__:
            np.testing.assert_array_equal(getattr(d, f)[sl], getattr(own[m][1], f), err_msg=f)


# ---- the default path ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,chains,family", [("nuts_n41", 1, "auto"), ("nuts_n41", 2, "auto"), ("nuts_n41", 3, "mc"), ("nuts_ptrans_n41", 3, "mc")])
def test_identity_links_without_weights_and_set_then_reset_are_the_model_never_set_bit_for_bit(case, chains, family):
    """Log posterior (both forms) and a NUTS run with every diagnostic on the cases of the metric table, one kernel of each family
    (k_stream<1>, <2>, k_stream_sep, k_stream_mc): a handle that never saw the call, one after set_obs_model(all identity, None), one after
    set-then-reset."""
    c = M.case(case)
    pr, dense, init, d = M.case_problem(c)
    runs = []
    for how in ("never", "identity", "reset"):
        eng = U.engine_for(dense, c.band, drift=d, options={"stream_family": family})
        try:
            if how == "identity":
                eng.set_obs_model(["identity"] * pr.D, None)
            elif how == "reset":
                eng.set_obs_model(["sqrt"] + [None] * (pr.D - 1), np.full(len(pr.obs_idx), 2.0))
                assert eng.obs_model()[0][0] == host.LINK_SQRT
                eng.set_obs_model(None, None)
            links, wt = eng.obs_model()
            assert links.tolist() == [0] * pr.D and (wt == 1.0).all()
            states = [np.repeat(np.asarray(v)[None], chains, axis=0) for v in init]
            forms = [eng.logpost_grad(*states, 0.7, want_terms=True, fused=fused) for fused in (False, True)]
            eng.sampler_init(_cfg(eng, c), *states, seed=c.seed, chain_ids=_ids(chains))
            eng.sampler_run(c.burnin + c.results)
            runs.append((forms, (eng.sampler_samples(), eng.sampler_diag())))
        finally:
            eng.close()
    for forms, run in runs[1:]:
        for fa, fb in zip(forms, runs[0][0]):
            for a, b in zip(fa, fb):
                np.testing.assert_array_equal(a, b)
        _assert_same_run(run, runs[0][1])
    assert runs[0][1][1].leapfrogs_taken.max() >= 31


# ---- the contract --------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_rejected_leave_the_handle_as_it_was_and_the_model_round_trips():
    c = OR.case("nuts_n41")
    pr, _, _, w = OR.case_problem(c)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    eng = _case_engine(c)
    try:
        good = _run_case(eng, c, 1)
    finally:
        eng.close()
    eng = _case_engine(c)
    try:
        lib, h = eng._lib, eng._h
        n = len(pr.obs_idx)
        L = np.asarray(OR.LINKS_SEIR4, dtype=np.int32)
        arr = lambda v, t, p: None if v is None else np.ascontiguousarray(v, dtype=t).ctypes.data_as(p)
        call = lambda D, links, n_obs, wt: lib.magi_set_obs_model(h, D, arr(links, np.int32, ip), n_obs, arr(wt, np.float64, dp))
        def weight(k, v):
            out = w.copy(); out[k] = v
            return out
        assert call(3, L[:3], n, w) == -1 and call(5, np.append(L, 0), n, w) == -1                               # another D
        assert call(4, L, n - 1, w[:-1]) == -1 and call(4, L, n + 1, np.append(w, 1.0)) == -1                    # another n_obs
        assert call(4, [3, 0, 0, 0], n, w) == -1 and call(4, [0, 0, -1, 0], n, w) == -1                         # a link out of range
        for v in (0.0, -1.0, np.nan, np.inf):                                                                    # a weight not finite or not > 0
            assert call(4, L, n, weight(7, v)) == -1
        links, wt = eng.obs_model()                                                                              # the model round-trips, untouched
        assert links.tolist() == list(OR.LINKS_SEIR4) and wt.tolist() == w.tolist()
        gl, gw = np.zeros(4, dtype=np.int32), np.zeros(n)
        assert lib.magi_get_obs_model(h, 4, gl.ctypes.data_as(ip), n, None) == 0 and lib.magi_get_obs_model(h, 4, None, n, gw.ctypes.data_as(dp)) == 0
        assert gl.tolist() == list(OR.LINKS_SEIR4) and gw.tolist() == w.tolist()
        assert lib.magi_get_obs_model(h, 3, gl.ctypes.data_as(ip), n, None) == -1 and lib.magi_get_obs_model(h, 4, None, n + 1, gw.ctypes.data_as(dp)) == -1
        with pytest.raises(ValueError):
            eng.set_obs_model(["logit"] * 4, None)                                                               # (the host refuses an unknown name)
        _assert_same_run(good, _run_case(eng, c, 1))
        # a datum outside its link's domain: y = 0 under log, y < 0 under sqrt (y = 0 is inside sqrt's)
        y = np.array(pr.y, dtype=np.float64)
        first = {d: int(np.where(pr.obs_idx % 4 == d)[0][0]) for d in range(4)}
        y[first[0]], y[first[2]] = 0.0, 0.0
        eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, y, pr.beta, pr.LB, pr.drift)
        assert eng.obs_model()[0].tolist() == [0, 0, 0, 0] and (eng.obs_model()[1] == 1.0).all()                  # magi_set_problem has reset the model
        assert call(4, [1, 0, 0, 0], n, None) == -1 and call(4, [0, 0, 2, 0], n, None) == 0
        y[first[2]] = -1e-3
        eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, y, pr.beta, pr.LB, pr.drift)
        assert call(4, [0, 0, 2, 0], n, None) == -1 and call(4, [0, 1, 0, 1], n, None) == 0
        assert eng.obs_model()[0].tolist() == [0, 1, 0, 1]
    finally:
        eng.close()
    fresh = MagiEngine(0)
    try:
        k = np.zeros(4, dtype=np.int32)
        assert fresh._lib.magi_set_obs_model(fresh._h, 4, k.ctypes.data_as(ip), 0, None) == -5                   # before magi_set_problem
        assert fresh._lib.magi_get_obs_model(fresh._h, 4, k.ctypes.data_as(ip), 0, None) == -5
        with pytest.raises(MagiHipError):
            fresh.set_obs_model(None, None)
    finally:
        fresh.close()


def test_set_problem_resets_the_model_and_the_untransformed_data_are_kept():
    """After magi_set_problem the handle computes the reference's posterior again; a model set, changed and set again computes what a fresh
    handle under that model computes, to the bit (the handle keeps y itself, not g(y))."""
    c = OR.case("nuts_n41")
    pr, dense, (X0, s0, t0), w = OR.case_problem(c)
    eng = _case_engine(c)
    try:
        first = eng.logpost_grad(X0, s0, t0, 1.0, want_terms=True)
        eng.set_obs_model("sqrt", None)
        eng.set_obs_model(list(OR.LINKS_SEIR4), w)
        for a, b in zip(eng.logpost_grad(X0, s0, t0, 1.0, want_terms=True), first):
            np.testing.assert_array_equal(a, b)
        eng.set_problem(dense.mu, dense.N_ds, dense.obs_idx, dense.y, dense.beta, dense.LB, dense.drift)
        assert eng.obs_model()[0].tolist() == [0] * 4
        got = eng.logpost_grad(X0, s0, t0, 1.0)
        want = orc.logpost_grad(X0, s0, t0, 1.0, pr)
        assert abs(got[0] - want[0]) <= 1e-10 * abs(want[0])
        assert abs(got[0] - first[0]) > 1e-3 * abs(want[0])
    finally:
        eng.close()


# ---- the Python API ------------------------------------------------------------------------------------------------------------------------------

def _lv_model(data_seed=None):
    from magi_v2_amd.api import MAGI_v2
    from magi_v2_amd.drift_examples import lotka_volterra
    I, X_obs, _, W = OR.e2e_data(data_seed)
    model = MAGI_v2(4, I, X_obs, None, lotka_volterra)
    model.initial_fit(0, hparams={"phi1s": host.hparams_initial(X_obs)["phi1s"], "phi2s": np.full(2, OR.E2E["phi2"])})
    model.thetas_init = np.ones(4)          # (the start tests/test_obs_cpu.py holds to the knife-edge condition: obs_reference.e2e_twin)
    return model, X_obs, W


def _model_problem(model, LB):
    orc.DRIFTS["lotka_volterra"] = OR.e2e_oracle_drift(model.I)
    return orc.Problem(I=np.asarray(model.I).reshape(-1), mu=model.mu_ds, C_inv=np.asarray(model.C_d_invs), m=np.asarray(model.m_ds),
                       K_inv=np.asarray(model.K_d_invs), N_ds=model.N_ds.astype(float), obs_idx=np.asarray(model.not_nan_idxs),
                       y=np.asarray(model.y_tau_ds_observed), beta=float(model.beta), LB=LB, drift="lotka_volterra", P=4)


def test_predict_under_log_links_and_weights_equals_the_reference_on_multiplicative_data():
    """predict(obs_link="log", obs_weight=W) end to end on predator-prey data with 10 % multiplicative noise (N = 41, 200 + 200 transitions,
    depth <= 3, one chain): the leapfrog counts and the posterior means of theta are those of the CPU reference run on the model's own
    matrices with the same seed, to the draw-for-draw bars; the echoed specification and the link-scale sigma^2 defaults are host's."""
    e = OR.E2E
    model, X_obs, W = _lv_model()
    try:
        kw = dict(n_chains=1, seed=e["seed"], chain_ids=[0], stale_cache=False, max_tree_depth=e["max_tree_depth"])
        res = model.predict(e["results"], e["burnin"], obs_link="log", obs_weight=W, **kw)
        assert res["obs_link"] == ["log", "log"]
        np.testing.assert_array_equal(res["obs_weight"], W)
        links = host.obs_model_spec("log", 2)
        LB, start = host.link_sigma_defaults(links, X_obs, model.Xhat_init, W, host.sigma_sqs_lower_bound(model.Xhat_init),
                                             np.asarray(model.sigma_sqs_init, dtype=np.float64), False)
        gy = np.log(X_obs)
        np.testing.assert_array_equal(LB, [(0.01 * gy[:, d].std()) ** 2 for d in range(2)])
        r2 = (np.log(model.Xhat_init) - gy) ** 2
        np.testing.assert_array_equal(start, [np.sum(W[:, d] * r2[:, d]) / np.sum(W[:, d]) for d in range(2)])
        assert (start > LB).all() and (start < 0.1).all()          # (on the log's scale: ~ 0.1^2, the noise of the data)
        sig0, th0 = host.softplus_inverse_inits(start, np.asarray(model.thetas_init, dtype=np.float64), LB)
        got_LB, got_sig0, got_th0 = model._predict_prepare(None, obs_link="log", obs_weight=W)
        np.testing.assert_array_equal(got_LB, LB); np.testing.assert_array_equal(got_sig0, sig0); np.testing.assert_array_equal(got_th0, th0)
        lk, wt = model.engine.obs_model()
        assert lk.tolist() == [1, 1] and wt.tolist() == W.reshape(-1).tolist()
        np.testing.assert_array_equal(res["sigma_sqs_samps"], host.transform_samples(res["sample_results"][1], res["sample_results"][2], LB)[0])
        # the CPU reference on the model's own matrices
        pr = _model_problem(model, LB)
        th_ref, out = OR.e2e_reference(pr, np.asarray(model.Xhat_init, dtype=np.float64), sig0, th0, "log", W.reshape(-1))
        np.testing.assert_array_equal(res["kernel_results"]["leapfrogs_taken"], out[3]["leapfrogs"])
        mean = res["thetas_samps"].mean(axis=0)
        print("posterior mean of theta under log links and weights: device", mean.tolist(), "reference", th_ref.mean(axis=0).tolist(), "truth", e["truth"])
        np.testing.assert_allclose(mean, th_ref.mean(axis=0), rtol=U.BRANCH_TOL["th_pre"][0], atol=U.BRANCH_TOL["th_pre"][1])
        # summaries and trajectories work unchanged, on the natural scale
        traj = model.posterior_trajectories(res, return_draws=False)
        assert np.isfinite(traj["mean"]).all() and np.isfinite(res["X_samps"]).all()
        # recorded, not asserted: how far the identity-link posterior sits from it on this data
        plain = model.predict(e["results"], e["burnin"], **kw)
        assert "obs_link" not in plain and "obs_weight" not in plain
        print("posterior mean of theta under identity links:", plain["thetas_samps"].mean(axis=0).tolist(),
              "sd log", res["thetas_samps"].std(axis=0).tolist(), "sd identity", plain["thetas_samps"].std(axis=0).tolist())
        # a start state outside a link's domain at observed points
        keep = model.Xhat_init
        model.Xhat_init = np.array(keep, dtype=np.float64)
        model.Xhat_init[[3, 8], 1] = -0.5
        try:
            with pytest.raises(ValueError, match="component 1 .* at 2 observed point"):
                model.predict(4, 4, obs_link=["identity", "log"], **kw)
            assert model.predict(4, 4, obs_link=["log", "identity"], **kw)["obs_link"] == ["log", "identity"]
        finally:
            model.Xhat_init = keep
    finally:
        model.engine.close()


def test_predict_many_with_per_model_observation_models_equals_each_models_own_predict():
    from magi_v2_amd.api import predict_many
    models = [_lv_model(s) for s in (None, 13)]
    ms = [m for m, _, _ in models]
    links = [["log", "sqrt"], None]
    wts = [models[0][2], models[1][2]]
    kw = dict(n_chains=2, seed=3, stale_cache=False, max_tree_depth=4)
    try:
        many = predict_many(ms, 5, 5, obs_link=links, obs_weight=wts, **kw)
        for m, l, w, got in zip(ms, links, wts, many):
            own = m.predict(5, 5, obs_link=l, obs_weight=w, **kw)
            assert got["obs_link"] == own["obs_link"]
            for k in ("X_samps", "sigma_sqs_samps", "thetas_samps"):
                np.testing.assert_array_equal(got[k], own[k])
            np.testing.assert_array_equal(got["kernel_results"]["leapfrogs_taken"], own["kernel_results"]["leapfrogs_taken"])
        assert many[0]["obs_link"] == ["log", "sqrt"] and many[1]["obs_link"] == ["identity", "identity"]
        one = predict_many(ms, 5, 5, obs_link="log", **kw)
        assert [r["obs_link"] for r in one] == [["log", "log"]] * 2 and "obs_weight" not in one[0]
        np.testing.assert_array_equal(one[0]["thetas_samps"], ms[0].predict(5, 5, obs_link="log", **kw)["thetas_samps"])
    finally:
        for m in ms:
            m.engine.close()
