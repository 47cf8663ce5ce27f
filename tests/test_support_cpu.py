"""Supports of theta: conditions on the reference (tests/support_reference.py) and on the host helpers alone -- no GPU.

What tests/test_support_gpu.py compares the device against is held here to the oracle (bit identity under all-positive supports), to its
own central differences, and to the sensitivity conditions of every sampler case: a device that ignored the supports, dropped the sign of
d theta / d pre of an upper-bounded parameter or kept the Jacobian term of a real one would change an integer diagnostic and move the
target by at least 1000 x its bar -- for every compared chain.  The last of the three is a small perturbation (one gradient entry moves by
1 - sg): where the table's rows run more than 4 + 3 transitions, or under another Philox seed than 808, that is why
(tests/support_reference.py: CASES)."""
import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import support_reference as S
from tests import util as U


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    """The traced drifts the cases register with the oracle (``orc.DRIFTS``) go when the module is done: other tests iterate over that table."""
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


def _random_states(pr, n, seed):
    rng = np.random.default_rng(seed)
    fx = M.seir_problem(41, None, 0.1)[0]
    return [(fx["Xhat_init"] + 0.05 * rng.normal(size=(pr.N, pr.D)), rng.normal(-2.0, 1.0, pr.D), rng.normal(0.0, 1.5, pr.P)) for _ in range(n)]


def test_all_positive_reference_is_the_oracle_bit_for_bit():
    pr = M.seir_problem(41, None, 0.1)[1]
    fn = S.logpost_grad_supported(*host.theta_support(None, pr.P))
    fn_lo = S.logpost_grad_supported(*host.theta_support([("lower", 0.0)] * pr.P, pr.P))
    for X, sp, tp in _random_states(pr, 6, 11):
        for temp in (1.0, 0.37):
            want = orc.logpost_grad(X, sp, tp, temp, pr)
            for f in (fn, fn_lo):
                got = f(X, sp, tp, temp, pr)
                for a, b in zip(got, want):
                    np.testing.assert_array_equal(a, b)


def test_mixed_support_gradient_agrees_with_central_differences_of_its_value():
    """real at a negative pre, upper, lower; 1e-8 relative (measured 3e-10 at N = 41)."""
    pr = M.seir_problem(41, None, 0.1)[1]
    kinds, bounds = host.theta_support(["real", ("upper", 3.0), ("lower", 0.5)], 3)
    fn = S.logpost_grad_supported(kinds, bounds)
    X, sp, _ = _random_states(pr, 1, 5)[0]
    tp = np.array([-0.4, 0.3, -0.2])
    _, _, _, gth = fn(X, sp, tp, 1.0, pr)
    h = 1e-5
    worst = 0.0
    for p in range(3):
        e = np.zeros(3); e[p] = h
        fd = (fn(X, sp, tp + e, 1.0, pr)[0] - fn(X, sp, tp - e, 1.0, pr)[0]) / (2 * h)
        worst = max(worst, abs(fd - gth[p]) / abs(gth[p]))
    print(f"theta-gradient vs central differences, worst relative difference {worst:.2e}")
    assert worst <= 1e-8


def test_theta_support_parses_and_rejects():
    k, b = host.theta_support(None, 3)
    assert k.tolist() == [0, 0, 0] and b.tolist() == [0.0, 0.0, 0.0] and k.dtype == np.int32
    k, b = host.theta_support(["positive", "real", ("lower", -1.5), ("upper", 2)], 4)
    assert k.tolist() == [host.THETA_POSITIVE, host.THETA_REAL, host.THETA_LOWER, host.THETA_UPPER]
    assert b.tolist() == [0.0, 0.0, -1.5, 2.0]
    assert host.theta_support_spec(k, b) == ["positive", "real", ("lower", -1.5), ("upper", 2.0)]
    for bad in (["positive"], ["positive", "real", "real", "real", "real"], "real", ["interval"] * 4, [("lower", np.inf)] + ["real"] * 3,
                [("upper", np.nan)] + ["real"] * 3, [("lower", 0.0, 1.0)] + ["real"] * 3, [("between", 0.0)] + ["real"] * 3, [3] * 4, [None] * 4,
                [("lower", "x")] + ["real"] * 3, 7):
        with pytest.raises(ValueError):
            host.theta_support(bad, 4)


def test_pre_inits_and_transform_round_trip_with_the_fallback_and_the_positive_bits():
    spec = ["positive", "real", ("lower", -1.5), ("upper", 2.0), "positive", ("lower", 1.0), ("upper", 0.0)]
    kinds, bounds = host.theta_support(spec, 7)
    th = np.array([0.7, -3.0, -1.0, 1.25, -0.2, 0.5, 0.3])          # the last three lie on the wrong side: positive, lower, upper
    pre = host.theta_pre_inits(th, kinds, bounds)
    assert pre[4] == -5.0 and pre[5] == -5.0 and pre[6] == -5.0 and pre[1] == -3.0
    back = host.transform_thetas(pre, kinds, bounds)
    np.testing.assert_allclose(back[:4], th[:4], rtol=1e-14, atol=0)
    sp5 = np.log(np.exp(-5.0) + 1.0)
    np.testing.assert_allclose(back[4:], [sp5, 1.0 + sp5, 0.0 - sp5], rtol=1e-15, atol=0)
    # positive: the values of softplus_inverse_inits / transform_samples, bit for bit
    rng = np.random.default_rng(2)
    thp = np.concatenate([rng.uniform(0.01, 8.0, 6), [-0.3, 0.0]])
    k0, b0 = host.theta_support(None, 8)
    LB = np.zeros(8)
    np.testing.assert_array_equal(host.theta_pre_inits(thp, k0, b0), host.softplus_inverse_inits(np.ones(8), thp, LB)[1])
    draws = rng.normal(0.0, 3.0, (2, 5, 8))
    np.testing.assert_array_equal(host.transform_thetas(draws, k0, b0), host.transform_samples(draws, draws, LB)[1])
    # a real parameter far out: no overflow leaks into it
    assert host.transform_thetas(np.array([800.0]), *host.theta_support(["real"], 1))[0] == 800.0


LEAPFROGS_N41 = {20: [2, 1, 63, 127, 127, 63, 127], 21: [3, 1, 63, 127, 127, 127, 127]}
LEAPFROGS_N41_IGNORED = {20: [2, 1, 63, 63, 127, 63, 127], 21: [3, 1, 63, 63, 63, 63, 63]}


def test_the_n41_case_is_the_one_the_table_was_chosen_for():
    c = S.case("nuts_n41")
    for ch in (20, 21):
        al = S.case_run(c, ch)[0][4]["all"]
        assert list(al["leapfrogs"][:7]) == LEAPFROGS_N41[ch]
        assert list(al["has_divergence"][:2]) == [True, True]
        assert list(S.case_run(c, ch, "ignored")[0][4]["all"]["leapfrogs"][:7]) == LEAPFROGS_N41_IGNORED[ch]


@pytest.mark.parametrize("c,ch", [(c, ch) for c in S.CASES for ch in c.chains()], ids=repr)
def test_every_compared_chain_would_show_a_wrong_support(c, ch):
    """Per compared chain of the GPU table, on the reference alone: (1) not every transition ends at the depth cap (NUTS); (2) a device that
    ignored the supports (all-positive on the same pre), (3) one that dropped the sign of d theta / d pre of an upper-bounded parameter and
    (4) one that kept 1 - sg as the Jacobian derivative of a real one would each change at least one integer diagnostic and move
    target_log_prob by >= 1000 x its bar."""
    al = S.case_run(c, ch)[0][4]["all"]
    if c.cfg.get("mode", 0) == 0:
        cap = (1 << c.cfg["max_tree_depth"]) - 1
        assert not all(lf == cap for lf in al["leapfrogs"]), list(al["leapfrogs"])
    missed = []
    for fault in S.FAULTS:
        fl = S.case_run(c, ch, fault)[0][4]["all"]
        ints = [f for _, f in M.INT_FIELDS if not np.array_equal(np.asarray(al[f]), np.asarray(fl[f]))]
        with np.errstate(invalid="ignore"):
            rel = np.nanmax(np.abs(np.asarray(fl["target_log_prob"]) - al["target_log_prob"]) / np.abs(al["target_log_prob"]))
        print(f"{c} chain {ch} {fault}: integer diagnostics that differ: {ints}; target_log_prob moves by {rel:.2e} relative "
              f"(bar {U.BRANCH_TOL['target_log_prob'][0]:.0e}); leapfrogs {list(map(int, al['leapfrogs']))} -> {list(map(int, fl['leapfrogs']))}")
        if not ints or not rel >= 1000.0 * U.BRANCH_TOL["target_log_prob"][0]:
            missed.append((fault, ints, float(rel)))
    assert not missed, missed


@pytest.fixture(scope="module")
def oscillator():
    return oscillator_reference()


_osc = {}


def oscillator_reference():
    """(orc.Problem, fixture, X_true) of the oscillator as MAGI_v2.initial_fit(0, hparams=...) sets it up: every point observed, phi1 from
    hparams_initial, phi2 = 1.5, theta_init from the reference's own initialiser.  The drift is registered with the oracle by the caller."""
    if not _osc:
        I, X_obs, X_true = S.oscillator_data()
        hp = orc.hparams_initial(X_obs)
        C_inv, m, K_inv = orc.build_all(I, hp["phi1s"], np.full(2, 1.5), 2.01, bandsize=None)
        Xhat = orc.cubic_smoother(I, X_obs)
        N_ds = np.full(2, float(len(I)))
        pr = orc.Problem(I=I, mu=X_obs.mean(axis=0), C_inv=C_inv, m=m, K_inv=K_inv, N_ds=N_ds, obs_idx=np.arange(X_obs.size), y=X_obs.reshape(-1),
                         beta=1.0, LB=orc.sigma_sqs_lower_bound(Xhat), drift="linear_oscillator", P=3)
        _osc["v"] = (pr, {"Xhat_init": Xhat, "sigma_sqs_init": hp["sigma_sqs"]}, X_true)
    return _osc["v"]


def test_oscillator_is_recovered_under_real_supports_on_the_reference(oscillator):
    """200 + 200 NUTS transitions, stale_cache off, depth <= 8, seed 3, chain 0, on the reference.  Fixes the bars the GPU end-to-end test
    re-uses (S.OSC_BARS): every posterior mean within 0.25 |truth|, b and c negative, max |E[X] - X_true| < 0.1."""
    pr, fx, X_true = oscillator
    orc.DRIFTS["linear_oscillator"] = (S.oscillator_drift, 2, 3)
    try:
        th_init = np.asarray(orc.fit_thetas_init(fx["Xhat_init"], pr.mu, pr.m, pr.K_inv, "linear_oscillator", 3)[0], dtype=np.float64)
        print("theta_init of the reference's initialiser:", th_init.tolist())
        kinds, bounds = host.theta_support(S.OSC_SPEC, 3)
        X0, s0, _ = orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(3), pr.LB)
        init = (X0, s0, host.theta_pre_inits(th_init, kinds, bounds))
        Xs, _, tp, info, _ = M.sample_chain(pr, None, None, None, 200, 200, seed=3, chain=0, initial=init, stale_cache=False, max_tree_depth=8,
                                            logpost_grad=S.logpost_grad_supported(kinds, bounds))
        print("mean leapfrogs", float(np.mean(info["leapfrogs"])))
        S.oscillator_bars(host.transform_thetas(tp, kinds, bounds), Xs, X_true)
    finally:
        del orc.DRIFTS["linear_oscillator"]
