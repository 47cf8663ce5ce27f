"""Posterior summaries and convergence diagnostics on the GPU (include/magi_hip.h: magi_summarize, magi_sampler_summarize) against the
longdouble transcription of their definitions (tests/summary_reference.py) at the tolerances tests/test_summary_cpu.py derives: order
statistics bit-exact, quantiles 4 ulp, mean 1e-12 max|y|, sd / rhat / ess / mcse_mean rtol 1e-13 kappa + 1e-11; sigma / theta columns
1e-14 relative on the order statistics (the device's log / exp).  The shapes put C R on both sides of the LDS sort (2048 doubles) and M n
on both sides of the LDS series, with odd R, R = 4 and a partial 64-column tile (K = 11)."""
import os
import warnings

import numpy as np
import pytest

import summary_reference as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = os.path.join(GOLDEN, "seir_alpha_sweep.npz")
STATS = ("mean", "sd", "quantiles", "rhat", "ess", "mcse_mean")
RUN = dict(num_results=24, num_burnin_steps=6, max_tree_depth=6)


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


def _same_bits(a, b):
    for s in STATS:
        np.testing.assert_array_equal(np.asarray(a[s]).view(np.uint64), np.asarray(b[s]).view(np.uint64), err_msg=s)
    assert a["n_nonfinite"] == b["n_nonfinite"]


@pytest.mark.parametrize("C, R", sr.SHAPES)
def test_summarize_matches_the_reference_on_every_fixture_shape(eng, C, R):
    got = eng.summarize(sr.fixture(C, R), sr.PROBS)
    assert got["mean"].shape == (sr.K_FIXTURE,) and got["quantiles"].shape == (3, sr.K_FIXTURE)
    worst = sr.check_against(got, sr.fixture_reference(C, R))
    print(C, R, "worst error / bar:", worst)
    assert got["sd"][sr.COL_CONST] == 0.0 and got["mean"][sr.COL_CONST] == 0.75
    if R < 4:
        assert np.all(np.isnan(got["rhat"]))


@pytest.mark.parametrize("C, R", sr.SHAPES)
def test_order_statistics_are_bit_exact(eng, C, R):
    y = sr.fixture(C, R)
    S = C * R
    ranks = sorted(set(int(r) for r in np.linspace(0, S - 1, 16)))
    probs = [k / (S - 1) for k in ranks]
    keep = [i for i, (k, p) in enumerate(zip(ranks, probs)) if np.float64(S - 1) * np.float64(p) == k]      # (h lands on the rank itself: g = 0)
    assert len(keep) >= min(len(ranks), 4) and 0 in keep
    got = eng.summarize(y, probs)["quantiles"]
    for k in range(sr.K_FIXTURE):
        if k == sr.COL_NAN:
            assert np.all(np.isnan(got[:, k]))
            continue
        v = np.sort(y[:, :, k].reshape(-1))
        for i in keep:
            assert got[i, k] == v[ranks[i]], (k, ranks[i])
    assert probs[-1] == 1.0 and all(got[-1, k] == y[:, :, k].max() for k in range(sr.K_FIXTURE) if k != sr.COL_NAN)


@pytest.mark.parametrize("R", [513, 4097])                         # the LDS sort, the radix select
def test_order_statistics_at_the_edges_of_the_number_format(eng, R):
    big = np.finfo(np.float64).max
    y = np.zeros((1, R, 2))
    y[0, :, 0] = np.where(np.arange(R) % 2 == 0, -big, big)           # v[hi] - v[lo] overflows between the two halves
    y[0, ::3, 1] = -0.0                                               # zeros of both signs: the negative ones sort first on both paths
    got = eng.summarize(y, (0.0, 1.0 / (R - 1), 1.0))["quantiles"]
    assert np.float64(R - 1) * np.float64(1.0 / (R - 1)) == 1.0
    np.testing.assert_array_equal(got[:, 0], [-big, -big, big])
    assert np.all(got[:, 1] == 0.0)
    np.testing.assert_array_equal(np.signbit(got[:, 1]), [True, True, False])


def test_chunks_and_partial_tiles_do_not_change_a_bit(eng):
    base = sr.fixture(3, 257)
    reps = -(-200 // sr.K_FIXTURE)
    y = np.concatenate([base * (1.0 + 0.25 * j) for j in range(reps)], axis=2)[:, :, :200]
    y = np.ascontiguousarray(y).reshape(3, 257, 8, 25)                # (a trailing shape, K = 200)
    whole = eng.summarize(y)
    assert whole["rhat"].shape == (8, 25) and whole["quantiles"].shape == (3, 8, 25)
    eng.set_option("summary_chunk_cols", 48)                         # 200 = 4 x 48 + 8: five chunks, none a multiple of the 64-column tile
    try:
        chunked = eng.summarize(y)
    finally:
        eng.set_option("summary_chunk_cols", 0)
    _same_bits(whole, chunked)
    sr.check_against(whole, sr.summarize(y))


def test_non_finite_columns_are_nan_and_counted(eng):
    y = np.array(sr.fixture(2, 65)[:, :, :4])
    y[1, 64, 1] = np.inf
    y[0, 0, 3] = -np.inf
    y[0, 1, 3] = np.nan
    got = eng.summarize(y, (0.0, 0.5, 1.0))
    assert got["n_nonfinite"] == 2
    for s in STATS:
        a = np.asarray(got[s])
        assert np.all(np.isnan(a[..., [1, 3]])), s
        assert not np.any(np.isnan(a[..., [0, 2]])), s
    clean = eng.summarize(sr.fixture(2, 65)[:, :, [0, 2]], (0.0, 0.5, 1.0))
    for s in STATS:                                                   # a column does not depend on its neighbours
        np.testing.assert_array_equal(np.asarray(got[s])[..., [0, 2]], clean[s], err_msg=s)


def test_rejected_arguments_leave_the_handle_usable(eng):
    from magi_v2_amd.engine import MagiHipError, _dp
    y = np.ascontiguousarray(sr.fixture(1, 64)[:, :, :2])
    probs = np.array([0.5])
    out = np.empty(2)
    ptr = lambda a: a.ctypes.data_as(_dp)

    def raw(C=1, R=64, K=2, draws=y, n_q=1, pr=probs):
        return eng._lib.magi_summarize(eng._h, C, R, K, None if draws is None else ptr(draws), n_q, ptr(pr), 0, ptr(out), None, None, None, None, None, None)

    assert raw() == 0
    # (the sizes are checked before a draw is read: the oversized shapes never touch memory)
    for kw in (dict(C=0), dict(C=4097), dict(R=0), dict(R=(1 << 20) + 1), dict(C=8, R=1 << 20), dict(K=0), dict(K=(1 << 24) + 1), dict(n_q=17), dict(n_q=-1),
               dict(pr=np.array([1.5])), dict(pr=np.array([-0.1])), dict(pr=np.array([np.nan])), dict(draws=None)):
        assert raw(**kw) == -1, kw
    with pytest.raises(MagiHipError) as ei:
        eng.summarize(y, probs=(0.5, 2.0))
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        eng.summarize(np.zeros(5))
    assert raw() == 0 and out[0] == eng.summarize(y, probs)["mean"][0]


@pytest.mark.parametrize("C, R", [(64, 40), (4, 1000)])
def test_two_runs_give_the_same_bits(eng, C, R):
    _same_bits(eng.summarize(sr.fixture(C, R)), eng.summarize(sr.fixture(C, R)))


def test_max_lag_truncates_the_lag_loop(eng):
    y = sr.fixture(4, 1000)
    got = eng.summarize(y, max_lag=5)
    sr.check_against(got, sr.fixture_reference(4, 1000, 5))
    full = eng.summarize(y)
    assert got["ess"][3] > 2 * full["ess"][3]                        # phi = 0.99: three pairs instead of 250
    _same_bits(full, eng.summarize(y, max_lag=10 ** 6))
    _same_bits(full, eng.summarize(y, max_lag=-3))


# ---- the sampler's device-resident samples ------------------------------------------------------------------------------------------

def _datasets():
    from magi_v2_amd.sweep import alpha_sweep_datasets
    return alpha_sweep_datasets(SWEEP, 1)


def _member(pb, band=80):
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    e.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=band, want_host=False)
    e.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    return e


def _init(e, pbs, C, seed, ids=None, **over):
    rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
    X0, s0, t0 = [np.concatenate([rep(pb[k]) for pb in pbs]) for k in ("Xhat", "sig_pre0", "th_pre0")]
    e.sampler_init(e.default_cfg(**{**RUN, **over}), X0, s0, t0, seed=seed, chain_ids=ids)


@pytest.fixture(scope="module")
def members():
    ds = _datasets()[:2]
    engs = [_member(pb) for _, pb in ds]
    yield engs, [pb for _, pb in ds]
    for e in engs:
        e.close()


def _check_sampler_summary(got, X, sp, tp, LB):
    from magi_v2_amd import host
    sig, th = host.transform_samples(sp, tp, LB)
    worst = {}
    for name, draws, st in (("X", X, False), ("sigma_sqs", sig, True), ("thetas", th, True)):
        ref = sr.summarize(draws, tuple(got["probs"]))
        block = dict(got[name], probs=got["probs"], n_nonfinite=ref["n_nonfinite"])
        assert block["mean"].shape == draws.shape[2:]
        worst[name] = sr.check_against(block, ref, sigma_theta=st)
    assert got["n_nonfinite"] == 0
    return worst


@pytest.mark.parametrize("C", [1, 2, 3])
def test_sampler_summary_matches_the_reference_on_the_downloaded_samples(members, C):
    from magi_v2_amd.engine import MagiHipError
    e, pb = members[0][0], members[1][0]
    assert (e.N, e.D) == (161, 4)
    _init(e, [pb], C, seed=77 + C)
    e.sampler_run(7)
    with pytest.raises(MagiHipError) as ei:                           # the chains have not finished
        e.sampler_summary()
    assert ei.value.code == -5
    e.sampler_run(RUN["num_results"] + RUN["num_burnin_steps"])
    X, sp, tp = e.sampler_samples()
    got = e.sampler_summary(probs=(0.0, 0.025, 0.5, 0.975, 1.0))
    print(C, _check_sampler_summary(got, X, sp, tp, pb["LB"]))
    pooled = X.reshape(-1, 161, 4)
    np.testing.assert_array_equal(got["X"]["quantiles"][0], pooled.min(axis=0))      # order statistics of X: the stored bits
    np.testing.assert_array_equal(got["X"]["quantiles"][-1], pooled.max(axis=0))
    if C == 3:
        sub = e.sampler_summary(chains=range(1, 3))
        _check_sampler_summary(sub, X[1:3], sp[1:3], tp[1:3], pb["LB"])
        one = e.sampler_summary(chains=slice(2, 3))
        _check_sampler_summary(one, X[2:3], sp[2:3], tp[2:3], pb["LB"])
        for bad in (range(2, 4), [0, 2]):
            with pytest.raises((MagiHipError, ValueError)):
                e.sampler_summary(chains=bad)
    host_route = e.summarize(X)                                       # the same draws through magi_summarize: the same bits
    for s in STATS:
        np.testing.assert_array_equal(e.sampler_summary()["X"][s], host_route[s], err_msg=s)


def test_group_member_summary_equals_the_members_own_handle(members):
    from magi_v2_amd.engine import MagiGroup, MagiHipError
    engs, pbs = members
    C, seed = 2, 5
    g = MagiGroup(engs)
    try:
        _init(g, pbs, C, seed, ids=[0, 1, 0, 1])
        g.sampler_run(30)
        grouped = [g.sampler_summary(member=m) for m in range(2)]
        with pytest.raises(MagiHipError) as ei:                       # chains of two members are never pooled
            g.sampler_summary()
        assert ei.value.code == -1
        with pytest.raises(MagiHipError):
            g.sampler_summary(chains=range(1, 3))
        again = g.sampler_summary(chains=range(2, 4))
    finally:
        g.close()
    for m in range(2):
        _init(engs[m], [pbs[m]], C, seed, ids=[0, 1])
        engs[m].sampler_run(30)
        own = engs[m].sampler_summary()
        for b in ("X", "sigma_sqs", "thetas"):
            _same_bits(dict(grouped[m][b], n_nonfinite=0), dict(own[b], n_nonfinite=0))
    _same_bits(dict(again["thetas"], n_nonfinite=0), dict(grouped[1]["thetas"], n_nonfinite=0))
    assert not np.array_equal(grouped[0]["sigma_sqs"]["mean"], grouped[1]["sigma_sqs"]["mean"])


# ---- predict ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    from magi_v2_amd.api import MAGI_v2
    z = np.load(SWEEP)
    names = sorted(k for k in z.files if k.startswith("alpha="))
    out = []
    for k in names[:2]:
        rows = z[k]
        m = MAGI_v2(D_thetas=3, ts_obs=rows[:, 0], X_obs=np.clip(rows[:, 1:5], 0.0, None), bandsize=80, f_vec="seir4")
        m.initial_fit(discretization=1, hparam_iters=0, theta_init_iters=200)
        out.append(m)
    return out


def test_predict_with_summary_and_without_the_samples(models):
    from magi_v2_amd import predict_many
    from magi_v2_amd.api import MAGI_v2
    m = models[0]
    with pytest.raises(RuntimeError):
        MAGI_v2(D_thetas=3, ts_obs=m.ts_obs, X_obs=m.X_obs, bandsize=80, f_vec="seir4").posterior_summary()
    with pytest.raises(ValueError):
        m.predict(8, 6, keep_samples=False)
    kw = dict(n_chains=2, seed=11, max_tree_depth=6)
    plain = m.predict(8, 6, **kw)
    assert "summary" not in plain
    full = m.predict(8, 6, summary=True, **kw)
    assert set(full) == set(plain) | {"summary"}
    np.testing.assert_array_equal(full["X_samps"], plain["X_samps"])
    s = full["summary"]
    assert set(s) == {"X", "sigma_sqs", "thetas", "probs", "n_nonfinite"} and set(s["X"]) == set(STATS)
    ref = sr.summarize(full["X_samps"])
    sr.check_against(dict(s["X"], probs=s["probs"], n_nonfinite=0), ref)
    ref_th = sr.summarize(full["thetas_samps"])
    sr.check_against(dict(s["thetas"], probs=s["probs"], n_nonfinite=0), ref_th, sigma_theta=True)
    again = m.posterior_summary()
    _same_bits(dict(again["X"], n_nonfinite=0), dict(s["X"], n_nonfinite=0))
    lean = m.predict(8, 6, summary=True, keep_samples=False, **kw)
    with pytest.raises(ValueError, match="keep_samples=True"):
        m.posterior_trajectories(lean)
    assert set(lean) == set(full)
    assert lean["X_samps"] is None and lean["sigma_sqs_samps"] is None and lean["thetas_samps"] is None and lean["sample_results"] is None
    np.testing.assert_array_equal(lean["kernel_results"]["energy"], plain["kernel_results"]["energy"])
    for b in ("X", "sigma_sqs", "thetas"):
        _same_bits(dict(lean["summary"][b], n_nonfinite=0), dict(s[b], n_nonfinite=0))
    many = predict_many(models, 8, 6, summary=True, keep_samples=False, **kw)
    assert len(many) == 2 and many[1]["X_samps"] is None
    for b in ("X", "sigma_sqs", "thetas"):
        _same_bits(dict(many[0]["summary"][b], n_nonfinite=0), dict(s[b], n_nonfinite=0))
    own = models[1].predict(8, 6, summary=True, keep_samples=False, **kw)["summary"]
    for b in ("X", "sigma_sqs", "thetas"):
        _same_bits(dict(many[1]["summary"][b], n_nonfinite=0), dict(own[b], n_nonfinite=0))


def test_a_run_that_never_moves_warns_and_has_no_rhat(models):
    m = models[0]
    with pytest.warns(UserWarning, match="every X column"):
        # no burn-in, so no step-size adaptation: every transition of this step size is rejected
        r = m.predict(8, 0, summary=True, n_chains=2, seed=3, max_tree_depth=4, step_size=1e3)
    assert not np.any(r["kernel_results"]["is_accepted"])
    s = r["summary"]
    assert s["n_nonfinite"] == 0
    assert np.all(s["X"]["sd"] == 0.0) and np.all(np.isnan(s["X"]["rhat"])) and np.all(np.isnan(s["X"]["ess"]))
    np.testing.assert_allclose(s["X"]["mean"], r["X_samps"][0, 0], rtol=1e-15, atol=0)          # (a sum of 16 equal draws rounds)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.predict(8, 6, summary=True, n_chains=2, seed=11, max_tree_depth=6)
