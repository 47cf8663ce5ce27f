"""Priors on theta and sigma^2 and known noise variances: conditions on the reference (tests/prior_reference.py) and on the host helpers
alone -- no GPU.

What tests/test_prior_gpu.py compares the device against is held here to the oracle (bit identity when every prior is flat), to central
differences of its own value in longdouble, to the problem with the fixed variance as a constant, and to the sensitivity and knife-edge
conditions of every sampler case: a device with one of the named faults (prior_reference.FAULTS) would change an integer diagnostic or move
target_log_prob by at least 1000 x its bar, for every compared chain; and rounding the operator products in longdouble changes no integer."""
import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import prior_reference as PR
from tests import util as U


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    """The traced drifts the cases register with the oracle (``orc.DRIFTS``) go when the module is done: other tests iterate over that table."""
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


def _problem():
    fx, pr, _ = M.seir_problem(41, None, 0.1)
    return fx, pr


def _random_states(pr, n, seed):
    rng = np.random.default_rng(seed)
    fx = _problem()[0]
    return [(fx["Xhat_init"] + 0.05 * rng.normal(size=(pr.N, pr.D)), rng.normal(-2.0, 1.0, pr.D), rng.normal(0.0, 1.5, pr.P)) for _ in range(n)]


def test_all_flat_reference_is_the_oracle_bit_for_bit():
    pr = _problem()[1]
    fns = (PR.logpost_grad_prior(), PR.logpost_grad_prior(host.prior_spec(["flat"] * 4, 4, "sigma_sq"), host.prior_spec([None] * 3, 3, "theta")))
    for X, sp, tp in _random_states(pr, 6, 11):
        for temp in (1.0, 0.37):
            want = orc.logpost_grad(X, sp, tp, temp, pr)
            for f in fns:
                for a, b in zip(f(X, sp, tp, temp, pr), want):
                    np.testing.assert_array_equal(a, b)


# every kind on a sigma^2 entry; every kind on theta under every compatible support (normal: all four; the densities on (0, inf): positive and
# lower with lo >= 0)
_SIG_SETS = [[("normal", 0.1, 0.05), ("lognormal", -2.0, 0.7), ("gamma", 2.0, 8.0), ("invgamma", 3.0, 0.3)],
             [("invgamma", 2.0, 0.1), ("fixed", 0.2), "flat", ("normal", 0.2, 0.1)]]
_TH_SETS = [(["positive", "real", ("upper", 3.0)], [("normal", 1.0, 0.3)] * 3),
            ([("lower", 0.5), ("lower", 0.0), "positive"], [("normal", 1.0, 0.3), ("lognormal", 0.2, 0.5), ("gamma", 2.0, 1.5)]),
            (["positive", "positive", ("lower", 0.25)], [("lognormal", 0.0, 0.4), ("invgamma", 3.0, 2.0), ("invgamma", 2.0, 1.0)]),
            ([("lower", 1.0), "positive", ("lower", 0.0)], [("gamma", 3.0, 2.0), ("gamma", 1.5, 0.5), ("lognormal", -0.3, 0.8)])]


@pytest.mark.parametrize("sig_spec", _SIG_SETS, ids=("sig-all", "sig-fixed"))
@pytest.mark.parametrize("spec,th_spec", _TH_SETS, ids=("normal", "positive-a", "positive-b", "positive-c"))
def test_value_and_gradient_agree_with_central_differences_of_the_value_in_longdouble(sig_spec, spec, th_spec):
    """Parameter gradients against (L(pre + h) - L(pre - h)) / 2h of the value with the operator products in longdouble, h = 1e-6:
    1e-7 relative plus 1e-7 of the largest entry (truncation h^2 |L'''| / 6 and rounding eps_long |L| / h are both below that)."""
    pr = _problem()[1]
    sup = host.theta_support(spec, 3)
    sp_, tp_ = host.prior_spec(sig_spec, 4, "sigma_sq"), host.prior_spec(th_spec, 3, "theta", sup)
    fn, fl = PR.logpost_grad_prior(sp_, tp_, *sup), PR.logpost_grad_prior(sp_, tp_, *sup, long=True)
    X, sp, _ = _random_states(pr, 1, 5)[0]
    sp = np.array([-2.5, -1.5, -2.0, -3.0])
    tp = np.array([-0.4, 0.3, -0.2])
    for temp in (1.0, 0.6):
        L, _, gs, gt = fn(X, sp, tp, temp, pr)
        Ll = fl(X, sp, tp, temp, pr)[0]
        assert abs(L - Ll) <= 1e-10 * abs(L)
        h = 1e-6
        fd = np.zeros(7)
        for j in range(7):
            e = np.zeros(7); e[j] = h
            # (the value in longdouble: fl returns a float, so difference the two bracket sums before rounding)
            fd[j] = (fl(X, sp + e[:4], tp + e[4:], temp, pr)[0] - fl(X, sp - e[:4], tp - e[4:], temp, pr)[0]) / (2 * h)
        g = np.concatenate([gs, gt])
        worst = np.abs(fd - g) / (1e-7 * np.abs(g) + 1e-7 * np.abs(g).max())
        print(f"parameter gradients vs central differences, worst error / bar {worst.max():.2e}")
        assert worst.max() <= 1.0, (fd, g)


def test_a_fixed_variance_has_gradient_minus_pre_and_leaves_the_problem_with_that_constant():
    """sigma^2_1 fixed at c: its gradient is -beta_temp pre; every other gradient entry is that of the problem in which sigma^2_1 IS c
    (there: LB_1 = c - softplus(pre_1), no prior), and the value differs by the entry's own terms alone."""
    pr = _problem()[1]
    c = 0.2
    sp_ = host.prior_spec([None, ("fixed", c), None, None], 4, "sigma_sq")
    fn = PR.logpost_grad_prior(sp_, None)
    for X, sp, tp in _random_states(pr, 3, 7):
        for temp in (1.0, 0.37):
            L, gX, gs, gt = fn(X, sp, tp, temp, pr)
            assert gs[1] == -temp * sp[1] or abs(gs[1] + temp * sp[1]) <= 1e-15 * abs(sp[1])
            LB = pr.LB.copy()
            spl = np.log(1.0 + np.exp(sp[1]))
            LB[1] = c - spl
            twin = orc.Problem(I=pr.I, mu=pr.mu, C_inv=pr.C_inv, m=pr.m, K_inv=pr.K_inv, N_ds=pr.N_ds, obs_idx=pr.obs_idx, y=pr.y, beta=pr.beta, LB=LB,
                               drift=pr.drift, P=pr.P)
            L2, gX2, gs2, gt2 = orc.logpost_grad(X, sp, tp, temp, twin)
            np.testing.assert_allclose(gX, gX2, rtol=1e-12, atol=1e-12 * np.abs(gX2).max())
            np.testing.assert_allclose(gt, gt2, rtol=1e-12, atol=0)
            np.testing.assert_allclose(np.delete(gs, 1), np.delete(gs2, 1), rtol=1e-12, atol=0)
            assert abs((L - L2) - temp * (-0.5 * sp[1] ** 2 - (sp[1] - spl))) <= 1e-12 * abs(L)


def test_prior_specifications_parse_normalise_and_reject():
    k, a, b = host.prior_spec(None, 3, "theta")
    assert k.tolist() == [0, 0, 0] and a.tolist() == [0.0] * 3 and b.tolist() == [0.0] * 3 and k.dtype == np.int32
    spec = [None, "flat", ("normal", -1, 2), ("lognormal", 0.5, 1), ("gamma", 2, 3), ("invgamma", 3, 0.5), ("fixed", 0.25)]
    k, a, b = host.prior_spec(spec, 7, "sigma_sq")
    assert k.tolist() == [host.PRIOR_FLAT, host.PRIOR_FLAT, host.PRIOR_NORMAL, host.PRIOR_LOGNORMAL, host.PRIOR_GAMMA, host.PRIOR_INVGAMMA, host.PRIOR_FIXED]
    assert a.tolist() == [0.0, 0.0, -1.0, 0.5, 2.0, 3.0, 0.25] and b.tolist() == [0.0, 0.0, 2.0, 1.0, 3.0, 0.5, 0.0]
    assert host.prior_spec_echo(k, a, b) == ["flat", "flat", ("normal", -1.0, 2.0), ("lognormal", 0.5, 1.0), ("gamma", 2.0, 3.0), ("invgamma", 3.0, 0.5),
                                             ("fixed", 0.25)]
    ok = ["flat"] * 3
    bad = [["flat"], ["flat"] * 5, "flat", 7, [("uniform", 0.0, 1.0)] + ok, [3] + ok, [("normal", 0.0)] + ok, [("normal", 0.0, 1.0, 2.0)] + ok,
           [("fixed", 1.0, 2.0)] + ok, [("normal", "x", 1.0)] + ok,
           # parameters must be finite ...
           [("normal", np.nan, 1.0)] + ok, [("normal", 0.0, np.inf)] + ok, [("gamma", np.inf, 1.0)] + ok, [("fixed", np.nan)] + ok,
           # ... and in range: sd, shape, rate, scale, value > 0
           [("normal", 0.0, 0.0)] + ok, [("lognormal", 0.0, -1.0)] + ok, [("gamma", 0.0, 1.0)] + ok, [("gamma", 1.0, 0.0)] + ok,
           [("invgamma", -1.0, 1.0)] + ok, [("invgamma", 1.0, 0.0)] + ok, [("fixed", 0.0)] + ok, [("fixed", -0.1)] + ok]
    for spec in bad:
        with pytest.raises(ValueError):
            host.prior_spec(spec, 4, "sigma_sq")
    with pytest.raises(ValueError):
        host.prior_spec(ok + ["flat"], 4, "variance")
    # fixed is for sigma^2 entries only
    with pytest.raises(ValueError):
        host.prior_spec([("fixed", 0.5)] + ok, 4, "theta")
    # lognormal, gamma and invgamma on theta need a support inside (0, inf): positive, or lower with lo >= 0
    for name in ("lognormal", "gamma", "invgamma"):
        for sup in ("real", ("upper", 2.0), ("lower", -0.5)):
            with pytest.raises(ValueError):
                host.prior_spec([(name, 1.0, 1.0)], 1, "theta", host.theta_support([sup], 1))
        for sup in ("positive", ("lower", 0.0), ("lower", 1.5)):
            assert host.prior_spec([(name, 1.0, 1.0)], 1, "theta", host.theta_support([sup], 1))[0].tolist() == [host._PRIOR_NAMES[name]]
        assert host.prior_spec([("normal", -1.0, 1.0)], 1, "theta", host.theta_support(["real"], 1))[0].tolist() == [host.PRIOR_NORMAL]


def test_transform_samples_reports_a_fixed_variance_as_its_constant():
    rng = np.random.default_rng(3)
    sp, tp, LB = rng.normal(-3, 1, (2, 5, 3)), rng.normal(0, 1, (2, 5, 2)), np.array([1e-3, 2e-3, 3e-3])
    plain = host.transform_samples(sp, tp, LB)
    for a, b in zip(host.transform_samples(sp, tp, LB, host.prior_spec(None, 3, "sigma_sq")), plain):
        np.testing.assert_array_equal(a, b)
    sig, th = host.transform_samples(sp, tp, LB, host.prior_spec([None, ("fixed", 0.04), ("gamma", 2.0, 1.0)], 3, "sigma_sq"))
    assert (sig[..., 1] == 0.04).all()
    np.testing.assert_array_equal(sig[..., [0, 2]], plain[0][..., [0, 2]])
    np.testing.assert_array_equal(th, plain[1])


@pytest.mark.parametrize("c,ch", [(c, ch) for c in PR.CASES for ch in c.chains()] + [("warm-up", 20), ("warm-up", 21)], ids=repr)
def test_every_compared_chain_would_show_a_wrong_prior_and_sits_on_no_knife_edge(c, ch):
    """Per compared chain of the GPU table, on the reference alone: (1) not every transition ends at the depth cap (NUTS); (2) every fault of
    prior_reference.FAULTS changes at least one integer diagnostic or moves target_log_prob by >= 1000 x its bar; (3) with the operator
    products in longdouble the integer diagnostics are the same and the compared floats move by at most 1/100 of the device's bars (the
    criterion of tests/test_sampler_branches_cpu.py)."""
    if c == "warm-up":          # (the warm-up that adapts the metric, on the N = 41 case: prior_reference.WARM)
        c, run = PR.case("nuts_n41"), lambda c_, ch_, fault=None, long=False: PR.case_run(c_, ch_, fault, long, warm=True)
        cap = (1 << PR.WARM["max_tree_depth"]) - 1
    else:
        run, cap = PR.case_run, (1 << c.cfg.get("max_tree_depth", 0)) - 1
    ref = run(c, ch)[0]
    al = ref[4]["all"]
    if c.cfg.get("mode", 0) == 0:
        assert not all(lf == cap for lf in al["leapfrogs"]), list(al["leapfrogs"])
    missed = []
    for fault in PR.FAULTS:
        fl = run(c, ch, fault)[0][4]["all"]
        ints = [f for _, f in M.INT_FIELDS if not np.array_equal(np.asarray(al[f]), np.asarray(fl[f]))]
        with np.errstate(invalid="ignore"):
            rel = np.nanmax(np.abs(np.asarray(fl["target_log_prob"]) - al["target_log_prob"]) / np.abs(al["target_log_prob"]))
        print(f"{c} chain {ch} {fault}: integer diagnostics that differ: {ints}; target_log_prob moves by {rel:.2e} relative "
              f"(bar {U.BRANCH_TOL['target_log_prob'][0]:.0e}); leapfrogs {list(map(int, al['leapfrogs']))} -> {list(map(int, fl['leapfrogs']))}")
        if not ints and not rel >= 1000.0 * U.BRANCH_TOL["target_log_prob"][0]:
            missed.append((fault, ints, float(rel)))
    assert not missed, missed
    second = run(c, ch, long=True)[0]
    ll = second[4]["all"]
    for _, f in M.INT_FIELDS:
        np.testing.assert_array_equal(np.asarray(al[f]), np.asarray(ll[f]), err_msg=f)
    tol = dict(U.BRANCH_TOL, energy=U.ENERGY_TOL)
    worst = {}
    for k, u, v in [(k, np.asarray(al[k], dtype=np.float64), np.asarray(ll[k], dtype=np.float64)) for k in ("step_size", "log_accept_ratio", "target_log_prob", "energy")] \
            + [("X", ref[0], second[0]), ("sig_pre", ref[1], second[1]), ("th_pre", ref[2], second[2])]:
        rtol, atol = tol[k]
        np.testing.assert_array_equal(np.isfinite(u), np.isfinite(v), err_msg=k)
        fin = np.isfinite(u)
        if k == "X":
            atol = atol * np.abs(v).max()
        with np.errstate(invalid="ignore"):          # (-inf - -inf outside `fin`)
            d = np.abs(u - v)[fin] / (atol + rtol * np.abs(v)[fin])
        worst[k] = float(d.max()) if d.size else 0.0
    print(f"{c} chain {ch}: float64 vs longdouble operator products, fraction of the device tolerance:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-2, (k, v)


def test_an_informative_prior_moves_the_posterior_on_the_reference():
    """The N = 41 golden problem (SIRW), 200 + 200 NUTS transitions, seed 5, chain 0, depth <= 3, stale cache off: flat against a normal prior on
    theta_0 centred at 3.0 (sd 0.05), away from the flat posterior mean.  The mean of theta_0 moves towards 3.0 by more than 5 x the pooled
    MCSE of tests/summary_reference.py -- what tests/test_prior_gpu.py reproduces on the device is not vacuous."""
    from tests import summary_reference as sr
    flat, _ = PR.e2e_run(None)
    inf, _ = PR.e2e_run(PR.e2e_prior())
    j, m = PR.E2E["entry"], PR.e2e_prior()[PR.E2E["entry"]][1]
    mc = [float(sr.summarize(th[None], (0.5,))["mcse_mean"][j]) for th in (flat, inf)]
    pooled = float(np.hypot(*mc))
    moved = abs(flat[:, j].mean() - m) - abs(inf[:, j].mean() - m)
    print(f"theta_{j}: flat mean {flat[:, j].mean():.4f} (MCSE {mc[0]:.4f}), informative mean {inf[:, j].mean():.4f} (MCSE {mc[1]:.4f}), prior centre {m}; "
          f"moved towards it by {moved:.4f} = {moved / pooled:.1f} x the pooled MCSE {pooled:.4f}")
    assert abs(flat[:, j].mean() - m) > 1.0
    assert moved > 5.0 * pooled
