"""Time-dependent drifts on the GPU: an ``f_vec`` that uses ``t`` runs through the kernels compiled for it -- every streaming-kernel
family, the point phase, the three-phase kernels, the theta initialiser, the self-test, problem groups, the drop-in class -- and equals
the oracle, whose drift table takes a closure over the grid column (``tests/test_time_drift_cpu.py::oracle_drift_at``; Jacobians by
complex step with the times, independent of the sympy tracing).  The time of grid point i is what ``set_times`` was given -- the
reference passes ``self.I`` (magi_v2.py:155, 206, 335).  Tolerances are those of tests/test_user_drift_gpu.py and
tests/test_theta_init_gpu.py."""
import dataclasses
import re

import numpy as np
import pytest

from magi_v2_amd import drift, host, selftest
from magi_v2_amd.drift_examples import TIME_EXAMPLES, seir_seasonal
from magi_v2_amd.engine import MagiEngine, MagiHipError
from oracle import magi_oracle as orc
from tests.test_time_drift_cpu import fixture_data, oracle_drift_at

pytestmark = pytest.mark.gpu
NAMES = sorted(TIME_EXAMPLES)


def make_problem(name, band=None, shift=0.0, set_times=True):
    """tests/test_user_drift_gpu.py::make_problem on the fixtures of this feature.  The matrices are built on the grid I; the drift is
    evaluated at I + shift, on the device (set_times) and in the oracle (the closure).  Also registers ``name + "@0"``: the same drift with
    the times frozen at 0."""
    f_vec, D, P = TIME_EXAMPLES[name]
    I, X, X_obs, truth, phi2 = fixture_data(name)
    d = drift.resolve(f_vec, D, P)
    eng = MagiEngine(0, drift=d)
    Xi = host.linear_interpolate(X_obs)
    hp = host.hparams_initial(Xi)
    C_inv, m, K_inv = eng.build_matrices(I, hp["phi1s"], np.full(D, phi2), 2.01, bandsize=None)
    N_ds, beta, idx, y = host.observation_bookkeeping(X_obs, X_obs)
    Xhat = host.cubic_smoother(I, Xi)
    LB = host.sigma_sqs_lower_bound(Xhat)
    orc.DRIFTS[name] = (oracle_drift_at(f_vec, I + shift), D, P)
    orc.DRIFTS[name + "@0"] = (oracle_drift_at(f_vec, 0.0 * I), D, P)
    pr = orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=orc.band_part(C_inv, band), m=orc.band_part(m, band), K_inv=orc.band_part(K_inv, band),
                     N_ds=N_ds.astype(np.float64), obs_idx=idx, y=y, beta=float(beta), LB=LB, drift=name, P=P)
    eng.set_matrices(C_inv, m, K_inv, bandsize=band)
    if set_times:
        eng.set_times(I + shift)
        eng.set_problem(pr.mu, pr.N_ds, idx, y, beta, LB, d)
    return eng, pr, Xhat, hp, truth, d


def assert_logpost_equals_oracle(eng, pr, X, sp, tp, temp, fused, frozen_gap=None):
    L, gX, gs, gt = orc.logpost_grad(X, sp, tp, temp, pr)
    if frozen_gap is not None:
        # the condition that keeps this test honest, on the oracle alone: with the times frozen at 0 the value is another one
        L0 = orc.logpost_grad(X, sp, tp, temp, dataclasses.replace(pr, drift=pr.drift + "@0"))[0]
        frozen_gap.append(abs(L0 - L) / abs(L))
    out = eng.logpost_grad(X, sp, tp, temp, fused=fused)
    scale = np.abs(gX).max()
    assert abs(out[0] - L) <= 1e-9 * abs(L), (pr.drift, fused, out[0], L)
    np.testing.assert_allclose(out[1], gX, rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(out[2], gs, rtol=1e-8, atol=1e-9 * scale)
    np.testing.assert_allclose(out[3], gt, rtol=1e-8, atol=1e-9 * scale)


@pytest.mark.parametrize("name,band", [(n, None) for n in NAMES] + [("fhn_forced", 6)])
def test_log_posterior_and_gradient_match_oracle(name, band):
    """Three-phase and fused, two states x two temperatures.  A kernel that ignores t cannot pass: on the oracle alone the same states with
    the times frozen at 0 differ by at least 1e-2 relative in L."""
    eng, pr, Xhat, hp, truth, d = make_problem(name, band=band)
    rng = np.random.default_rng(5)
    D, P = Xhat.shape[1], len(truth)
    gaps = []
    for rep in range(2):
        X = Xhat + rng.normal(0, 1.0, Xhat.shape) * (0.05 * Xhat.std(axis=0))      # (5 % of each component's spread: the seasonal SEIR's states are ~0.1)
        sp, tp = rng.normal(-3, 0.5, D), rng.normal(0.3, 0.4, P)
        for temp in (1.0, 0.1316):
            for fused in (False, True):
                assert_logpost_equals_oracle(eng, pr, X, sp, tp, temp, fused, gaps)
    eng.close()
    print("relative change of L with the times frozen at 0:", name, band, min(gaps), max(gaps))
    assert min(gaps) >= 1e-2, (name, gaps)


@pytest.mark.parametrize("name", NAMES)
def test_batched_states_on_the_matrix_core_kernel(name, monkeypatch):
    """Five states per call with MAGI_STREAM_FAMILY=mc: k_stream_sep for the two separable drifts (their operand mirror holds basis
    functions of t), k_stream_mc for the infusion model.  Batched fused == batched three-phase == per-state oracle."""
    monkeypatch.setenv("MAGI_STREAM_FAMILY", "mc")
    eng, pr, Xhat, hp, truth, d = make_problem(name)
    assert eng.stream_kernel_name(5).startswith("k_stream_mc" if name == "mm_infusion" else "k_stream_sep")
    rng = np.random.default_rng(11)
    D, P, n = Xhat.shape[1], len(truth), 5
    X = Xhat[None] + rng.normal(0, 1.0, (n,) + Xhat.shape) * (0.05 * Xhat.std(axis=0))
    sp, tp = rng.normal(-3, 0.5, (n, D)), np.log(np.expm1(truth))[None] + rng.normal(0, 0.2, (n, P))
    a = eng.logpost_grad(X, sp, tp, 0.7)
    b = eng.logpost_grad(X, sp, tp, 0.7, fused=True)
    gaps = []
    for c in range(n):
        L, gX, gs, gt = orc.logpost_grad(X[c], sp[c], tp[c], 0.7, pr)
        L0 = orc.logpost_grad(X[c], sp[c], tp[c], 0.7, dataclasses.replace(pr, drift=name + "@0"))[0]
        gaps.append(abs(L0 - L) / abs(L))
        for out in (a, b):
            assert abs(out[0][c] - L) <= 1e-9 * abs(L)
            np.testing.assert_allclose(out[1][c], gX, rtol=0, atol=1e-9 * np.abs(gX).max())
            np.testing.assert_allclose(out[3][c], gt, rtol=1e-8, atol=1e-9 * np.abs(gX).max())
    eng.close()
    assert min(gaps) >= 1e-2, (name, gaps)


def test_the_handles_times_count_not_the_grid_of_the_matrices():
    eng, pr, Xhat, hp, truth, d = make_problem("seir_seasonal", shift=0.37)
    rng = np.random.default_rng(7)
    X = Xhat + rng.normal(0, 1.0, Xhat.shape) * (0.05 * Xhat.std(axis=0))
    sp, tp = rng.normal(-3, 0.5, 3), rng.normal(0.3, 0.4, 4)
    for fused in (False, True):
        assert_logpost_equals_oracle(eng, pr, X, sp, tp, 1.0, fused)
    # ... and they can be replaced after the problem was set: back on the grid itself
    L_shift = eng.logpost_grad(X, sp, tp, 1.0)[0]
    eng.set_times(pr.I)
    orc.DRIFTS["seir_seasonal"] = (oracle_drift_at(seir_seasonal, pr.I), 3, 4)
    for fused in (False, True):
        assert_logpost_equals_oracle(eng, pr, X, sp, tp, 1.0, fused)
    assert abs(eng.logpost_grad(X, sp, tp, 1.0)[0] - L_shift) > 1e-3 * abs(L_shift)
    # a wrong length, a non-finite entry
    with pytest.raises(MagiHipError, match="magi_set_times"):
        eng.set_times(pr.I[:-1])
    bad = pr.I.copy(); bad[3] = np.nan
    with pytest.raises(MagiHipError, match="finite"):
        eng.set_times(bad)
    for fused in (False, True):                                 # (the refused calls changed nothing)
        assert_logpost_equals_oracle(eng, pr, X, sp, tp, 1.0, fused)
    eng.close()


def test_set_problem_without_times_is_refused_and_names_the_call():
    eng, pr, Xhat, hp, truth, d = make_problem("fhn_forced", set_times=False)
    with pytest.raises(MagiHipError, match="magi_set_times") as e:
        eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, d)
    assert e.value.code == -5                                   # MAGI_E_STATE
    with pytest.raises(MagiHipError, match="magi_set_times"):
        eng.theta_init(d, Xhat, pr.mu, 5)
    eng.set_times(pr.I)
    eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, d)
    # matrices of another N forget the times
    I2 = np.linspace(0.0, 20.0, 31)
    eng.build_matrices(I2, hp["phi1s"], np.full(2, 1.5), 2.01, want_host=False)
    with pytest.raises(MagiHipError, match="magi_set_times"):
        eng.set_problem(pr.mu, pr.N_ds, np.zeros(0, dtype=np.int64), np.zeros(0), 1.0, pr.LB, d)
    eng.close()
    # a library whose drift ignores t takes times and ignores them; the base library too
    from magi_v2_amd.drift_examples import EXAMPLES
    from tests.util import engine_for, load_g4, problem_from_g4
    g = load_g4("seir4_N81")
    p4 = problem_from_g4(g, None)
    base = engine_for(p4, None)
    X, sp_, tp_ = g["state_X"][1], g["state_sig_pre"][1], g["state_th_pre"][1]
    before = base.logpost_grad(X, sp_, tp_, 1.0, fused=True)
    base.set_times(np.linspace(3.0, 9.0, 81))
    after = base.logpost_grad(X, sp_, tp_, 1.0, fused=True)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    base.close()
    # the engine refuses a library whose flag disagrees with the drift it is created for
    from magi_v2_amd import jit
    fhn = drift.resolve(*EXAMPLES["fhn"])
    with pytest.raises(ValueError, match="does not use t"):
        MagiEngine(0, drift=dataclasses.replace(fhn, time_dependent=True), _library=jit.library_for(fhn))


@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_deep_trees_match_oracle_draw_for_draw_in_every_kernel_family(name, chains, stream_family):
    """As test_traced_drift_deep_trees_match_oracle_in_every_kernel_family, started at the generating parameters."""
    eng, pr, Xhat, hp, truth, d = make_problem(name)
    th0 = truth.copy()
    sp0, tp0 = host.softplus_inverse_inits(hp["sigma_sqs"], th0, pr.LB)
    burnin, results, step0, depth = 4, 2, 2e-3, 6
    cfg = eng.default_cfg(num_results=results, num_burnin_steps=burnin, stale_cache=0, step_size=step0, max_tree_depth=depth)
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    ids = list(range(40, 40 + chains))
    eng.sampler_init(cfg, rep(Xhat), rep(sp0), rep(tp0), seed=515, chain_ids=ids)
    lf, _ = eng.sampler_run(burnin + results)
    Xs, sp, tp = eng.sampler_samples()
    dg = eng.sampler_diag()
    kernel = eng.stream_kernel_name(chains)
    eng.close()
    print(name, chains, stream_family, kernel, "leapfrogs", dg.leapfrogs_taken.tolist(), "accepted", int(dg.is_accepted.sum()))
    assert lf == dg.leapfrogs_taken.sum() and dg.leapfrogs_taken.max() >= 15 and dg.is_accepted.sum() >= chains
    for i in sorted({0, chains - 1}):
        trace = []
        oX, osp, otp, info, _ = orc.sample_chain(pr, Xhat, hp["sigma_sqs"], th0, results, burnin, seed=515, chain=ids[i], step_size=step0,
                                                 stale_cache=False, trace=trace, max_tree_depth=depth)
        np.testing.assert_array_equal(dg.leapfrogs_taken[i], [r.leapfrogs for _, r, _ in trace])
        np.testing.assert_array_equal(dg.is_accepted[i], [int(r.is_accepted) for _, r, _ in trace])
        np.testing.assert_allclose(dg.target_log_prob[i], [r.target_log_prob for _, r, _ in trace], rtol=1e-8)
        np.testing.assert_allclose(tp[i], otp, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(Xs[i], oX, rtol=0, atol=1e-8 * np.abs(oX).max())


def _seasonal_model(shift=0.0):
    import magi_v2
    I, X, X_obs, truth, phi2 = fixture_data("seir_seasonal")
    sd = np.nanstd(X, axis=0)
    m = magi_v2.MAGI_v2(D_thetas=4, ts_obs=I + shift, X_obs=X_obs, bandsize=None, f_vec=seir_seasonal)
    m.initial_fit(discretization=1, hparams={"phi2s": [phi2] * 3, "sigma_sqs": (0.05 * sd) ** 2 + 1e-8}, theta_init_iters=200)
    return m


def _oracle_problem_of(model, name):
    LB = orc.sigma_sqs_lower_bound(model.Xhat_init)
    orc.DRIFTS[name] = (oracle_drift_at(seir_seasonal, model.I), 3, 4)
    return orc.Problem(I=model.I[:, 0], mu=model.mu_ds, C_inv=np.asarray(model.C_d_invs), m=np.asarray(model.m_ds), K_inv=np.asarray(model.K_d_invs),
                       N_ds=model.N_ds.astype(float), obs_idx=model.not_nan_idxs, y=model.y_tau_ds_observed, beta=float(model.beta), LB=LB,
                       drift=name, P=4)


def test_through_the_class_from_constructor_to_results_and_onto_an_extended_grid():
    """The vignette's call sequence with a forced SEIR: MAGI_v2(...) -> initial_fit -> predict equals the oracle draw for draw; the theta
    initialiser (device branch: beta a is not linear in theta) equals the oracle's over the same closure; update_kernel_matrices onto a
    grid extended past T evaluates the forcing at the new times."""
    model = _seasonal_model()
    assert model.drift.time_dependent and model.mag_I == 81
    pr = _oracle_problem_of(model, "seir_seasonal_api")
    want, _ = orc.fit_thetas_init(model.X_interp_obs, model.mu_ds, np.asarray(model.m_ds), np.asarray(model.K_d_invs), "seir_seasonal_api", 4, num_iters=200)
    np.testing.assert_allclose(model.thetas_init, want, rtol=1e-8, atol=1e-10)
    orc.DRIFTS["seir_seasonal_api@0"] = (oracle_drift_at(seir_seasonal, 0.0 * model.I), 3, 4)
    frozen, _ = orc.fit_thetas_init(model.X_interp_obs, model.mu_ds, np.asarray(model.m_ds), np.asarray(model.K_d_invs), "seir_seasonal_api@0", 4, num_iters=200)
    assert np.abs(frozen - want).max() > 1e-3                  # (an initialiser that ignored t would land elsewhere)
    res = model.predict(num_results=3, num_burnin_steps=5, seed=99, stale_cache=False)
    trace = []
    oX, osp, otp, info, _ = orc.sample_chain(pr, model.Xhat_init, model.sigma_sqs_init, model.thetas_init, 3, 5, seed=99, stale_cache=False, trace=trace)
    np.testing.assert_array_equal(res["kernel_results"]["leapfrogs_taken"], [r.leapfrogs for _, r, _ in trace][5:])
    np.testing.assert_array_equal(res["kernel_results"]["is_accepted"], [int(r.is_accepted) for _, r, _ in trace][5:])
    np.testing.assert_allclose(res["kernel_results"]["target_log_prob"], [r.target_log_prob for _, r, _ in trace][5:], rtol=1e-8)
    _, oth = orc.transform_samples(osp, otp, pr.LB)
    np.testing.assert_allclose(res["thetas_samps"], oth, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["X_samps"], oX, rtol=0, atol=1e-8 * np.abs(oX).max())
    assert res["X_samps"].shape == (3, 81, 3) and res["thetas_samps"].shape == (3, 4)
    # forecasting: the grid extended past T = 4, the state extended by its last row
    I_new = np.concatenate([model.I[:, 0], model.I[-1, 0] + 0.05 * np.arange(1, 21)])
    model.update_kernel_matrices(I_new, model.phi1s, model.phi2s)
    Xext = np.concatenate([model.Xhat_init, np.repeat(model.Xhat_init[-1:], 20, axis=0)])
    model.Xhat_init = Xext
    lb, sp0, tp0 = model._predict_prepare(None)
    pr2 = _oracle_problem_of(model, "seir_seasonal_ext")
    pr2 = dataclasses.replace(pr2, LB=lb)
    rng = np.random.default_rng(8)
    X = Xext + rng.normal(0, 0.01, Xext.shape)
    L, gX, gs, gt = orc.logpost_grad(X, sp0, tp0, 1.0, pr2)
    for fused in (False, True):
        out = model.engine.logpost_grad(X, sp0, tp0, 1.0, fused=fused)
        assert abs(out[0] - L) <= 1e-9 * abs(L)
        np.testing.assert_allclose(out[1], gX, rtol=0, atol=1e-9 * np.abs(gX).max())
        np.testing.assert_allclose(out[3], gt, rtol=1e-8, atol=1e-9 * np.abs(gX).max())
    model.engine.close()


def test_predict_many_of_two_models_with_their_own_times_equals_predict_bit_for_bit():
    """Two seasonal SEIR models whose observation times differ by 0.5 (same N): one problem group, every member with its own times."""
    from magi_v2_amd import predict_many
    from magi_v2_amd.api import group_key
    from tests.test_group_gpu import _assert_results_equal
    models = [_seasonal_model(0.0), _seasonal_model(0.5)]
    kw = dict(n_chains=2, seed=2024, max_tree_depth=6, stale_cache=False)
    many = predict_many(models, 4, 4, **kw)
    assert group_key(models[0], 2) is not None and group_key(models[0], 2) == group_key(models[1], 2)
    singles = [m.predict(4, 4, **kw) for m in models]
    for r, s in zip(many, singles):
        _assert_results_equal(r, s)
    assert not np.array_equal(singles[0]["X_samps"], singles[1]["X_samps"])           # (the times differ: so do the draws)
    for m in models:
        m.engine.close()


@pytest.mark.parametrize("name", NAMES)
def test_selftest_passes_on_the_time_dependent_libraries(name):
    from magi_v2_amd import jit
    d = drift.resolve(*TIME_EXAMPLES[name])
    rep = selftest.run(jit.library_for(d), d, 0)
    print(rep.format())
    assert rep.ok and rep.drifts == [d.name]
    names = [c.name for c in rep.checks]
    assert names == ["drift.f", "drift.jt", "drift.runtime"] + (["drift.sep"] if name != "mm_infusion" else []) + ["families", "gradient", "sampler"]


def _wrong_seasonal(kind):
    """The seasonal SEIR header with the time frozen in f ("f": t_magi -> 0.0 in its body) or with the sign of the cosine term flipped
    in jt ("jt"); the host evaluators stay those of the trace."""
    d = drift.resolve(*TIME_EXAMPLES["seir_seasonal"])
    member = {"f": " void f(", "jt": " void jt("}[kind]
    head, body = d.header.split(member, 1)
    sig, body = body.split(" {\n", 1)
    body, tail = body.split("\n    }\n", 1)
    if kind == "f":
        new_body, n = body.replace("t_magi", "0.0"), body.count("t_magi")
    else:
        new_body, n = re.subn(r"cos\(", "-cos(", body, count=1)
    assert n >= 1 and new_body != body
    return dataclasses.replace(d, name=f"seir_seasonal_wrong_{kind}", header=head + member + sig + " {\n" + new_body + "\n    }\n" + tail)


@pytest.mark.parametrize("kind,fails", [("f", "drift.f"), ("jt", "drift.jt")])
def test_a_library_that_mishandles_the_time_is_refused(kind, fails, monkeypatch):
    monkeypatch.delenv("MAGI_SELFTEST", raising=False)
    bad = _wrong_seasonal(kind)
    with pytest.raises(selftest.MagiSelfTestError) as e:
        MagiEngine(0, drift=bad)
    print(e.value.report.format())
    failed = {c.name for c in e.value.report.failed()}
    assert fails in failed, failed
    if kind == "jt":
        assert "drift.f" not in failed
