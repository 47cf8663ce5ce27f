"""Supports of theta on the device (magi_set_theta_support) against tests/support_reference.py.

Tolerances are the project's own: ``tests.util.BRANCH_TOL`` / ``ENERGY_TOL`` for sampler runs, the 1e-9 bars of
tests/test_unobserved_gpu.py for the log posterior and its gradient, the bars of tests/test_summary_gpu.py for summaries; integer
diagnostics are compared exactly.  tests/test_support_cpu.py holds the reference and the case table on the CPU."""
import ctypes as C

import numpy as np
import pytest

from magi_v2_amd import host
from magi_v2_amd.engine import MagiEngine, MagiHipError
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import support_reference as S
from tests import util as U
from tests.test_metric_gpu import _KERNEL, _assert_chain, _cfg, _ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    """The traced drifts the cases register with the oracle (``orc.DRIFTS``) go when the module is done: other tests iterate over that table."""
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


def _engine(c, family="auto"):
    _, dense, _, d = S.case_problem(c) if isinstance(c, S.SupportCase) else M.case_problem(c)
    return U.engine_for(dense, c.band, drift=d, options={"stream_family": family})


def _states(c, n):
    return tuple(np.repeat(np.asarray(v)[None], n, axis=0) for v in S.case_init(c))


def _assert_logpost(eng, pr, kinds, bounds, X, sp, tp, where):
    """The 1e-9 bars of tests/test_unobserved_gpu.py::test_log_posterior_with_an_unobserved_component_matches_oracle, three-phase and fused."""
    L, gX, gs, gt = S.logpost_grad_supported(kinds, bounds)(X, sp, tp, 1.0, pr)
    for fused in (False, True):
        out = eng.logpost_grad(X, sp, tp, 1.0, fused=fused)
        print(f"{where} fused={fused}: logp rel {abs(out[0] - L) / abs(L):.2e}, gX {np.abs(out[1] - gX).max() / np.abs(gX).max():.2e}, "
              f"gth {np.abs(out[3] - gt).max() / np.abs(gX).max():.2e} of max|gX|")
        assert abs(out[0] - L) <= 1e-9 * abs(L), (where, fused)
        np.testing.assert_allclose(out[1], gX, rtol=0, atol=1e-9 * np.abs(gX).max(), err_msg=where)
        np.testing.assert_allclose(out[2], gs, rtol=1e-7, atol=1e-9 * np.abs(gX).max(), err_msg=where)
        np.testing.assert_allclose(out[3], gt, rtol=1e-7, atol=1e-9 * np.abs(gX).max(), err_msg=where)


def test_log_posterior_and_gradient_on_seir4_n41():
    c = S.case("nuts_n41")
    pr, dense, _, _ = M.case_problem(c)
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        k, b = eng.theta_support()
        assert k.tolist() == [host.THETA_REAL, host.THETA_LOWER, host.THETA_UPPER] and b.tolist() == [0.0, 0.5, 3.0]
        X0, s0, t0 = S.case_init(c)
        rng = np.random.default_rng(4)
        for tp in (t0, np.array([-1.7, 0.4, -0.8]), np.array([0.9, -2.0, 1.5])):
            _assert_logpost(eng, pr, k, b, X0 + 0.003 * rng.normal(size=X0.shape), s0, tp, f"seir4 N=41 th_pre={tp.tolist()}")
    finally:
        eng.close()


def test_log_posterior_and_gradient_on_a_structureless_fixture_of_two_blocks():
    from tests.test_structureless_cpu import fixture
    pr, X = fixture(129, "seir4")
    spec = [("upper", 9.0), "real", ("lower", 1.0)]
    kinds, bounds = host.theta_support(spec, 3)
    eng = U.engine_for(pr)
    try:
        eng.set_theta_support(spec)
        Xb, sp, tp = U.structureless_states(pr, X, 2, 3)
        tp = host.theta_pre_inits(host.transform_samples(sp, tp, pr.LB)[1], kinds, bounds)
        tp[1, 1] = -0.45                                        # a real entry at a negative pre
        for i in range(2):
            _assert_logpost(eng, pr, kinds, bounds, Xb[i], sp[i], tp[i], f"structureless seir4 N=129 state {i}")
    finally:
        eng.close()


def test_log_posterior_and_gradient_on_chain8_every_parameter_lane_and_kind():
    from tests import test_drift_edges_cpu as E
    spec = ["positive", "real", ("lower", 0.1), ("upper", 2.0), "real", ("upper", 1.5), ("lower", -1.0), "positive"]
    kinds, bounds = host.theta_support(spec, 8)
    with E.edge_drifts():
        pr, X = E.fixture("chain8")
        eng = U.engine_for(pr, drift=E.traced("chain8"))
        try:
            eng.set_theta_support(spec)
            Xb, sp, tp = U.structureless_states(pr, X, 2, 5)
            tp = host.theta_pre_inits(host.transform_samples(sp, tp, pr.LB)[1], kinds, bounds)
            tp[1, 4] = -0.3                                     # a real entry at a negative pre
            for i in range(2):
                _assert_logpost(eng, pr, kinds, bounds, Xb[i], sp[i], tp[i], f"chain8 N=129 state {i}")
        finally:
            eng.close()


@pytest.mark.parametrize("c,chains,family", [(c, n, f) for c in S.CASES for n, f in c.runs], ids=repr)
def test_sampler_matches_the_reference_draw_for_draw(c, chains, family):
    """The table of tests/support_reference.py: the N = 41 case (real, lower 0.5, upper 3.0 from theta = (-0.4, 1, 1); step 1e-2, depth <= 7,
    4 + 4 transitions, the two leading ones divergent) on k_stream<1>, <2>, k_stream_sep<8>, <16>; the stale cache; fixed-L HMC (L = 8);
    N = 161 under band 20; a non-separable traced drift on k_stream_mc; a time-dependent drift whose forcing amplitude is real and starts
    negative.  Chain ids 20 ..., the first and the last compared."""
    ids = _ids(chains)
    eng = _engine(c, family)
    try:
        name = eng.stream_kernel_name(chains)
        assert name.startswith(_KERNEL[(chains, family)]), name
        if family == "mc":
            assert name.startswith("k_stream_mc" if c.drift == "ptrans" else "k_stream_sep"), name
        eng.set_theta_support(c.spec)
        eng.sampler_init(_cfg(eng, c), *_states(c, chains), seed=c.seed, chain_ids=ids)
        lf, _ = eng.sampler_run(c.burnin + c.results)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert lf == d.leapfrogs_taken.sum()
    for i in sorted({0, chains - 1}):
        _assert_chain(f"{c.name} {name} chain {ids[i]}", i, d, samples, S.case_run(c, ids[i])[0], c.burnin)


def _run(c, chains, family, spec, set_it=True):
    eng = _engine(c, family)
    try:
        name = eng.stream_kernel_name(chains)
        if set_it:
            eng.set_theta_support(spec)
        init = M.case_problem(c)[2]
        eng.sampler_init(_cfg(eng, c), *[np.repeat(np.asarray(v)[None], chains, axis=0) for v in init], seed=c.seed, chain_ids=_ids(chains))
        eng.sampler_run(c.burnin + c.results)
        return name, eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()


def _assert_same_run(a, b):
    (_, sa, da), (_, sb, db) = a, b
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)
    for f in da.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(da, f), getattr(db, f), err_msg=f)


@pytest.mark.parametrize("case,chains,family", [("nuts_n41", 1, "auto"), ("nuts_n41", 2, "auto"), ("nuts_n41", 3, "mc"), ("nuts_ptrans_n41", 3, "mc")])
def test_all_positive_set_explicitly_is_the_support_never_set_bit_for_bit(case, chains, family):
    """Samples and every diagnostic, one kernel of each family (k_stream<1>, <2>, k_stream_sep, k_stream_mc); from theta = 1 as the metric cases."""
    c = M.case(case)
    P = M.case_problem(c)[0].P
    never = _run(c, chains, family, None, set_it=False)
    for spec in (["positive"] * P, None):
        _assert_same_run(never, _run(c, chains, family, spec))
    assert never[2].leapfrogs_taken.max() >= 31


@pytest.mark.parametrize("per", [1, 2])
def test_group_members_with_different_supports_equal_their_own_handles_bit_for_bit(per):
    """Two members of one shape, the supports of the N = 41 case and its mirror image, on k_stream_group<1> and <2>."""
    c = S.case("nuts_n41")
    specs = [c.spec, [("upper", 3.0), "real", ("lower", 0.5)]]
    th0 = [c.theta0, np.array([1.0, -0.4, 1.0])]
    X0, s0, _ = S.case_init(c)
    starts = [(X0, s0, host.theta_pre_inits(t, *host.theta_support(sp, 3))) for sp, t in zip(specs, th0)]
    rep = lambda st: [np.repeat(np.asarray(v)[None], per, axis=0) for v in st]
    ids = _ids(per)
    own = []
    for sp, st in zip(specs, starts):
        eng = _engine(c)
        try:
            eng.set_theta_support(sp)
            eng.sampler_init(_cfg(eng, c), *rep(st), seed=c.seed, chain_ids=ids)
            eng.sampler_run(c.burnin + c.results)
            own.append((eng.sampler_samples(), eng.sampler_diag(), eng.sampler_summary()))
        finally:
            eng.close()
    engs = [_engine(c) for _ in specs]
    try:
        for e, sp in zip(engs, specs):
            e.set_theta_support(sp)
        g = MagiEngine.group(engs)
        try:
            with pytest.raises(MagiHipError) as err:
                g.set_theta_support(c.spec)
            assert err.value.code == -5
            both = [np.concatenate([rep(st)[k] for st in starts]) for k in range(3)]
            g.sampler_init(_cfg(g, c), *both, seed=c.seed, chain_ids=ids + ids)
            g.sampler_run(c.burnin + c.results)
            samples, d = g.sampler_samples(), g.sampler_diag()
            sums = [g.sampler_summary(member=m) for m in range(2)]
        finally:
            g.close()
    finally:
        for e in engs:
            e.close()
    assert own[0][1].leapfrogs_taken.tolist() != own[1][1].leapfrogs_taken.tolist()
    for m in range(2):
        sl = slice(m * per, (m + 1) * per)
        for a, b in zip(samples, own[m][0]):
            np.testing.assert_array_equal(a[sl], b)
        for f in d.__dataclass_fields__:
            np.testing.assert_array_equal(getattr(d, f)[sl], getattr(own[m][1], f), err_msg=f)
        for stat in ("mean", "sd", "quantiles"):
            np.testing.assert_array_equal(sums[m]["thetas"][stat], own[m][2]["thetas"][stat])
        _assert_theta_summary(sums[m]["thetas"], host.transform_thetas(samples[2][sl], *host.theta_support(specs[m], 3)))


def _assert_theta_summary(got, th):
    """mean / sd / quantiles of the theta block against numpy on the transformed draws th [chains, draws, P], at the bars
    tests/test_summary_gpu.py holds the same statistics to."""
    from tests import summary_reference as sr
    probs = tuple(got.get("probs", (0.025, 0.5, 0.975)))
    ref = sr.summarize(np.asarray(th), probs)
    block = dict(got, probs=np.asarray(probs), n_nonfinite=ref["n_nonfinite"])
    assert block["mean"].shape == np.asarray(th).shape[2:]
    worst = sr.check_against(block, ref, sigma_theta=True)
    print("theta summary, worst error / bar:", worst)


def test_sampler_summary_reports_theta_on_the_natural_scale_of_its_support():
    c = S.case("nuts_n41")
    kinds, bounds = S.case_support(c.name)
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        eng.sampler_init(_cfg(eng, c, num_results=8, max_tree_depth=4), *_states(c, 2), seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(c.burnin + 8)
        _, _, tp = eng.sampler_samples()
        summ = eng.sampler_summary()
    finally:
        eng.close()
    th = host.transform_thetas(tp, kinds, bounds)
    assert (th[..., 1] > 0.5).all() and (th[..., 2] < 3.0).all()
    _assert_theta_summary(summ["thetas"], th)


def test_checkpoint_resumes_under_the_same_support_and_is_refused_under_another():
    c = S.case("nuts_n41")
    total = c.burnin + c.results
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        eng.sampler_init(_cfg(eng, c), *_states(c, 2), seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(3)
        ck = eng.sampler_checkpoint()
        eng.sampler_run(total - 3)
        whole = (eng.sampler_samples(), eng.sampler_diag())
    finally:
        eng.close()
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(total - 3)
        (sa, da), (sb, db) = whole, (eng.sampler_samples(), eng.sampler_diag())
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(da.leapfrogs_taken[:, 3:], db.leapfrogs_taken[:, 3:])
        np.testing.assert_array_equal(da.energy[:, 3:], db.energy[:, 3:])
        for other in (None, ["real", ("lower", 0.5), ("upper", 3.5)], ["real", ("lower", 0.5), "positive"]):
            eng.set_theta_support(other)
            with pytest.raises(MagiHipError) as err:
                eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=[20, 21])
            assert err.value.code == -1
    finally:
        eng.close()


def test_bad_arguments_are_rejected_and_leave_the_handle_as_it_was():
    c = S.case("nuts_n41")
    ip = C.POINTER(C.c_int32)
    good = _run_supported(c)
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        lib, h = eng._lib, eng._h
        call = lambda P, kinds, bounds: lib.magi_set_theta_support(
            h, P, None if kinds is None else np.asarray(kinds, dtype=np.int32).ctypes.data_as(ip),
            None if bounds is None else np.asarray(bounds, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        assert call(2, [3, 1], [0.0, 0.5]) == -1                       # P other than the problem's
        assert call(4, [3, 1, 2, 0], [0.0, 0.5, 3.0, 0.0]) == -1
        assert call(3, [3, 1, 4], [0.0, 0.5, 3.0]) == -1               # a kind out of range
        assert call(3, [-1, 1, 2], [0.0, 0.5, 3.0]) == -1
        assert call(3, [3, 1, 2], [0.0, np.inf, 3.0]) == -1            # a non-finite bound of a bounded entry
        assert call(3, [3, 1, 2], [0.0, 0.5, np.nan]) == -1
        assert call(3, [3, 1, 2], None) == -1
        assert call(3, [3, 1, 2], [np.nan, 0.5, 3.0]) == 0             # (the bound of a real entry is ignored ...)
        k, b = eng.theta_support()
        assert k.tolist() == [3, 1, 2] and b.tolist() == [0.0, 0.5, 3.0]          # (... and reported as 0)
        eng.sampler_init(_cfg(eng, c), *_states(c, 1), seed=c.seed, chain_ids=[20])
        eng.sampler_run(c.burnin + c.results)
        _assert_same_run(good, ("", eng.sampler_samples(), eng.sampler_diag()))
    finally:
        eng.close()
    fresh = MagiEngine(0)
    try:
        k = np.zeros(3, dtype=np.int32)
        assert fresh._lib.magi_set_theta_support(fresh._h, 3, k.ctypes.data_as(ip), None) == -5        # before magi_set_problem
        assert fresh._lib.magi_get_theta_support(fresh._h, 3, k.ctypes.data_as(ip), None) == -5
        with pytest.raises(MagiHipError):
            fresh.set_theta_support(["real"] * 3)
    finally:
        fresh.close()


def _run_supported(c):
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        eng.sampler_init(_cfg(eng, c), *_states(c, 1), seed=c.seed, chain_ids=[20])
        eng.sampler_run(c.burnin + c.results)
        return "", eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()


def test_set_problem_resets_the_support():
    c = S.case("nuts_n41")
    pr = M.case_problem(c)[1]
    eng = _engine(c)
    try:
        eng.set_theta_support(c.spec)
        eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, pr.drift)
        assert eng.theta_support()[0].tolist() == [0, 0, 0]
        X0, s0, t0 = M.case_problem(c)[2]
        got = eng.logpost_grad(X0, s0, t0, 1.0)
        want = orc.logpost_grad(X0, s0, t0, 1.0, pr)
        assert abs(got[0] - want[0]) <= 1e-9 * abs(want[0])
    finally:
        eng.close()


# ---- the Python API ---------------------------------------------------------------------------------------------------------------------------


def _oscillator_model(seed=3):
    from magi_v2_amd.api import MAGI_v2
    from magi_v2_amd.drift_examples import linear_oscillator
    I, X_obs, X_true = S.oscillator_data(seed=seed)
    model = MAGI_v2(3, I, X_obs, None, linear_oscillator)
    model.initial_fit(0, hparams={"phi1s": host.hparams_initial(X_obs)["phi1s"], "phi2s": np.array([1.5, 1.5])})
    return model, X_true


_KW = dict(n_chains=2, seed=3, stale_cache=False, max_tree_depth=5)
_ARRAYS = ("X_samps", "sigma_sqs_samps", "thetas_samps")


def test_predict_with_a_support_equals_the_engine_level_sequence_and_none_equals_all_positive():
    model, _ = _oscillator_model()
    try:
        res = model.predict(6, 6, summary=True, theta_support=S.OSC_SPEC, **_KW)
        assert res["theta_support"] == ["positive", "real", "real"]
        kinds, bounds = host.theta_support(S.OSC_SPEC, 3)
        np.testing.assert_array_equal(res["thetas_samps"], host.transform_thetas(res["sample_results"][2], kinds, bounds))
        _assert_theta_summary(res["summary"]["thetas"], res["thetas_samps"])
        # the engine-level sequence
        eng = model.engine
        LB, sig0, _ = model._predict_prepare(None)
        eng.set_theta_support(S.OSC_SPEC)
        th0 = host.theta_pre_inits(np.asarray(model.thetas_init, dtype=np.float64), kinds, bounds)
        rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None], 2, axis=0)
        cfg = eng.default_cfg(num_results=6, num_burnin_steps=6, stale_cache=0, anneal=1, max_tree_depth=5, step_size=0.1)
        eng.sampler_init(cfg, rep(model.Xhat_init), rep(sig0), rep(th0), seed=3)
        eng.sampler_run(12)
        Xs, sp, tp = eng.sampler_samples()
        np.testing.assert_array_equal(res["sample_results"][0], Xs)
        np.testing.assert_array_equal(res["sample_results"][2], tp)
        # keep_samples=False: the summary alone, the same numbers
        lean = model.predict(6, 6, summary=True, keep_samples=False, theta_support=S.OSC_SPEC, **_KW)
        assert lean["thetas_samps"] is None and lean["theta_support"] == res["theta_support"]
        for stat in ("mean", "sd", "quantiles"):
            np.testing.assert_array_equal(lean["summary"]["thetas"][stat], res["summary"]["thetas"][stat])
        # no argument == all-positive
        plain = model.predict(6, 6, **_KW)
        allpos = model.predict(6, 6, theta_support=["positive"] * 3, **_KW)
        assert "theta_support" not in plain and allpos["theta_support"] == ["positive"] * 3
        for k in _ARRAYS:
            np.testing.assert_array_equal(plain[k], allpos[k])
        for k in ("leapfrogs_taken", "energy", "target_log_prob"):
            np.testing.assert_array_equal(plain["kernel_results"][k], allpos["kernel_results"][k])
    finally:
        model.engine.close()


def test_predict_many_with_per_model_supports_equals_each_models_own_predict():
    from magi_v2_amd.api import predict_many
    models = [_oscillator_model(seed=s)[0] for s in (3, 4)]
    specs = [S.OSC_SPEC, ["positive", "real", ("upper", 0.0)]]
    try:
        many = predict_many(models, 5, 5, theta_support=specs, summary=True, **_KW)
        for m, sp, got in zip(models, specs, many):
            own = m.predict(5, 5, theta_support=sp, summary=True, **_KW)
            assert got["theta_support"] == own["theta_support"]
            for k in _ARRAYS:
                np.testing.assert_array_equal(got[k], own[k])
            np.testing.assert_array_equal(got["kernel_results"]["leapfrogs_taken"], own["kernel_results"]["leapfrogs_taken"])
            np.testing.assert_array_equal(got["summary"]["thetas"]["mean"], own["summary"]["thetas"]["mean"])
        assert (many[1]["thetas_samps"][..., 2] < 0.0).all()
        one = predict_many(models, 5, 5, theta_support=S.OSC_SPEC, **_KW)
        np.testing.assert_array_equal(one[0]["thetas_samps"], many[0]["thetas_samps"])
        assert one[1]["theta_support"] == ["positive", "real", "real"]
    finally:
        for m in models:
            m.engine.close()


def test_oscillator_end_to_end_recovers_its_signed_parameters():
    """x' = a y, y' = b x + c y with (a, b, c) = (1, -2, -0.3) through MAGI_v2: the bars tests/test_support_cpu.py fixes on the reference
    (every posterior mean within 0.25 |truth|, b and c negative, max |E[X] - X_true| < 0.1), all chains pooled."""
    model, X_true = _oscillator_model()
    try:
        res = model.predict(200, 200, n_chains=2, seed=3, stale_cache=False, max_tree_depth=8, theta_support=S.OSC_SPEC)
    finally:
        model.engine.close()
    print("theta_init", np.asarray(model.thetas_init).tolist(), "mean leapfrogs", float(res["kernel_results"]["leapfrogs_taken"].mean()))
    S.oscillator_bars(res["thetas_samps"], res["X_samps"], X_true)
