"""Observation model (log and square-root links, known weights): conditions on the reference (tests/obs_reference.py) and on the host helpers
alone -- no GPU.

What tests/test_obs_gpu.py compares the device against is held here to the oracle and to tests/prior_reference.py (bit identity under
identity links without weights), to central differences of its own value in longdouble, and -- on every fixture and sampler case the GPU
tests use -- to the conditioning and sensitivity conditions: float64 and longdouble operator products agree to 1/100 of the GPU bars, and a
device with one of the named faults (obs_reference.FAULTS) would move a compared quantity by at least 1000 x its bar, for every compared
state and chain."""
import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import obs_reference as OR
from tests import prior_reference as PR
from tests import util as U

BAR_THREE_PHASE, BAR_FUSED = 1e-10, 1e-9          # the GPU bars of the log posterior and its gradient (tests/test_obs_gpu.py)


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


def _seir():
    fx, pr, _ = M.seir_problem(41, None, 0.1)
    return fx, pr


def _random_states(pr, fx, n, seed):
    rng = np.random.default_rng(seed)
    return [(fx["Xhat_init"] + 0.05 * rng.normal(size=(pr.N, pr.D)), rng.normal(-2.0, 1.0, pr.D), rng.normal(0.0, 1.5, pr.P)) for _ in range(n)]


def test_identity_links_without_weights_are_the_oracle_and_the_prior_reference_bit_for_bit():
    fx, pr = _seir()
    sig = host.prior_spec([("invgamma", 3.0, 2e-4), ("fixed", 2.5e-4), None, ("lognormal", -8.0, 0.5)], 4, "sigma_sq")
    sup = host.theta_support(["real", ("lower", 0.5), ("upper", 3.0)], 3)
    th = host.prior_spec([("normal", -0.8, 0.05), ("lognormal", 0.5, 0.1), None], 3, "theta", sup)
    for X, sp, tp in _random_states(pr, fx, 4, 11):
        for temp in (1.0, 0.37):
            want = orc.logpost_grad(X, sp, tp, temp, pr)
            for f in (OR.logpost_grad_obs(), OR.logpost_grad_obs(np.zeros(4, dtype=np.int32), None), OR.logpost_grad_obs(fault="ignored", links=OR.LINKS_SEIR4)):
                for a, b in zip(f(X, sp, tp, temp, pr), want):
                    np.testing.assert_array_equal(a, b)
            want = PR.logpost_grad_prior(sig, th, *sup)(X, sp, tp, temp, pr)
            for a, b in zip(OR.logpost_grad_obs(None, None, sig, th, *sup)(X, sp, tp, temp, pr), want):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_agrees_with_central_differences_of_the_value_in_longdouble(weighted):
    """Every parameter entry and 24 entries of X (observed and unobserved, every component) against (L(q + h) - L(q - h)) / 2h of the value
    with the operator products in longdouble, h = 1e-6: 1e-6 relative plus 1e-7 of the block's largest entry (truncation h^2 |L'''| / 6
    -- the links' third derivatives at x ~ 0.1 are ~ 1e3 -- and rounding eps_long |L| / h are both below that)."""
    fx, pr, _, w = OR.obs_problem(41)
    fn = OR.logpost_grad_obs(OR.LINKS_SEIR4, w if weighted else None)
    fl = OR.logpost_grad_obs(OR.LINKS_SEIR4, w if weighted else None, long=True)
    X, sp, tp = fx["Xhat_init"], np.array([-2.5, -6.0, -5.0, -3.0]), np.array([1.0, -0.4, 0.3])
    rng = np.random.default_rng(4)
    entries = [(int(i), d) for d in range(4) for i in rng.choice(41, 6, replace=False)]
    for temp in (1.0, 0.6):
        L, gX, gs, gt = fn(X, sp, tp, temp, pr)
        assert np.isfinite(L) and abs(L - fl(X, sp, tp, temp, pr)[0]) <= 1e-12 * abs(L)
        h = 1e-6
        fd = np.zeros(7)
        for j in range(7):
            e = np.zeros(7); e[j] = h
            fd[j] = (fl(X, sp + e[:4], tp + e[4:], temp, pr)[0] - fl(X, sp - e[:4], tp - e[4:], temp, pr)[0]) / (2 * h)
        g = np.concatenate([gs, gt])
        worst = np.abs(fd - g) / (1e-6 * np.abs(g) + 1e-7 * np.abs(g).max())
        fdx = np.zeros(len(entries))
        for k, (i, d) in enumerate(entries):
            E = np.zeros_like(X); E[i, d] = h
            fdx[k] = (fl(X + E, sp, tp, temp, pr)[0] - fl(X - E, sp, tp, temp, pr)[0]) / (2 * h)
        gx = np.array([gX[i, d] for i, d in entries])
        worst_x = np.abs(fdx - gx) / (1e-6 * np.abs(gx) + 1e-7 * np.abs(gX).max())
        print(f"gradients vs central differences, worst error / bar: parameters {worst.max():.2e}, X {worst_x.max():.2e}")
        assert worst.max() <= 1.0 and worst_x.max() <= 1.0, (fd, g, fdx, gx)


@pytest.mark.parametrize("fx", OR.LOGPOST, ids=repr)
def test_every_logpost_fixture_is_well_conditioned_and_would_show_every_fault(fx):
    """Per fixture of the GPU table and per state of its largest batch: (1) float64 and longdouble operator products agree to 1/100 of the
    three-phase bar in every compared quantity (value, dX, dsigma, dtheta, t3, t4); (2) every fault of obs_reference.FAULTS moves at least
    one of them by >= 1000 x the fused bar -- "link_everywhere" through the negative unobserved entry every state carries."""
    with OR.fixture_drifts(fx):
        pr, w, (Xb, sp, tp), tb = OR.logpost_build(fx)
        assert (w != 1.0).sum() == len(w) // 2 and w.min() > 0.25 and w.max() < 4.0
        assert all(l in fx.links for l in (OR.LOG, OR.SQRT))
        if fx.unobserved is not None:
            assert pr.N_ds[fx.unobserved] == 0 and not (pr.obs_idx % pr.D == fx.unobserved).any()
        obs = np.zeros(pr.N * pr.D, dtype=bool); obs[pr.obs_idx] = True
        assert not obs.reshape(pr.N, pr.D)[fx.neg[0], fx.neg[1]] and (Xb[:, fx.neg[0], fx.neg[1]] < 0).all()
        lk = np.asarray(fx.links)[pr.obs_idx % pr.D]
        assert (Xb.reshape(len(Xb), -1)[:, pr.obs_idx][:, lk != OR.IDENTITY] > 0.04).all()          # observed linked entries: inside both domains
        missed = []
        for i in range(len(Xb)):
            ref = OR.reference_of(fx, i, 0.8)
            assert all(np.isfinite(v).all() for v in ref)
            worst = max(OR.figures(ref, OR.reference_of(fx, i, 0.8, long=True)).values())
            assert worst <= 1e-2 * BAR_THREE_PHASE, (i, worst)
            for fault in OR.FAULTS:
                moved = OR.figures(OR.reference_of(fx, i, 0.8, fault=fault), ref)
                if not max(moved.values()) >= 1000.0 * BAR_FUSED:
                    missed.append((i, fault, moved))
        assert not missed, missed


@pytest.mark.parametrize("c,ch", [(c, ch) for c in OR.CASES for ch in c.chains()], ids=repr)
def test_every_compared_chain_would_show_a_wrong_model_and_sits_on_no_knife_edge(c, ch):
    """Per compared chain of the GPU table, on the reference alone (the criteria of tests/test_prior_cpu.py): (1) not every transition ends
    at the depth cap (NUTS); (2) every fault changes an integer diagnostic or moves target_log_prob by >= 1000 x its bar
    ("link_everywhere" excepted: no entry of these runs is negative at an unobserved point -- the log-posterior fixtures hold it); (3) with
    the operator products in longdouble the integer diagnostics are the same and the compared floats move by <= 1/100 of the device's bars;
    (4) outside the domain case, every observed x of a linked component stays >= DOMAIN_MARGIN max|X| away from 0 over all evaluated states."""
    ref, _, record, _ = OR.case_run(c, ch)
    al = ref[4]["all"]
    cap = (1 << (OR.WARM["max_tree_depth"] if c.warm else c.cfg.get("max_tree_depth", 0))) - 1
    if c.cfg.get("mode", 0) == 0:
        assert not all(lf == cap for lf in al["leapfrogs"]), list(al["leapfrogs"])
    missed = []
    for fault in OR.FAULTS:
        if fault == "link_everywhere":
            continue
        fl = OR.case_run(c, ch, fault)[0][4]["all"]
        ints = [f for _, f in M.INT_FIELDS if not np.array_equal(np.asarray(al[f]), np.asarray(fl[f]))]
        with np.errstate(invalid="ignore"):
            rel = np.nanmax(np.abs(np.asarray(fl["target_log_prob"]) - al["target_log_prob"]) / np.abs(al["target_log_prob"]))
        print(f"{c} chain {ch} {fault}: integer diagnostics that differ: {ints}; target_log_prob moves by {rel:.2e} relative")
        if not ints and not rel >= 1000.0 * U.BRANCH_TOL["target_log_prob"][0]:
            missed.append((fault, ints, float(rel)))
    assert not missed, missed
    second = OR.case_run(c, ch, long=True)[0]
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
        with np.errstate(invalid="ignore"):
            d = np.abs(u - v)[fin] / (atol + rtol * np.abs(v)[fin])
        worst[k] = float(d.max()) if d.size else 0.0
    print(f"{c} chain {ch}: float64 vs longdouble operator products, fraction of the device tolerance:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-2, (k, v)
    rec = np.asarray(record)
    margin = np.nanmin(np.abs(rec[:, 0]) / rec[:, 1])
    print(f"{c} chain {ch}: smallest |observed x of a linked component| / max|X| over {len(rec)} evaluated states: {margin:.2e}")
    assert margin >= U.DOMAIN_MARGIN          # (a state outside a domain -- the blind first leaves from theta_0 = 1 -- is outside it by far more than rounding)


def test_the_domain_case_has_a_leaf_outside_a_links_domain_behind_an_accepted_proposal():
    """The oracle's census of chain 20: a NaN leaf in a sub-tree of depth >= 1 of a transition that ends accepted and divergent -- the
    proposal accepted before the leaf survives it -- and that leaf's state is outside the log link's domain at an observed point (x <= 0)
    while every operator product of it is finite; the run recovers (accepted transitions follow)."""
    c = OR.case("domain_n41")
    out, trace, record, events = OR.case_run(c, 20, census=True)
    run = U.DomainRun(out, trace, events, record, False)
    hits = [(k, it, d) for k, it, d in run.nan_leaves if d >= 1 and trace[k][1].is_accepted and trace[k][1].has_divergence]
    print("NaN leaves (transition, leaf, depth):", run.nan_leaves, "behind an accepted proposal:", hits, "census:", {k: v for k, v in events.items() if k[0] in ("nan", "div_accepted")})
    assert hits and events[("div_accepted",)] > 0
    for k, it, d in hits:
        assert run.outside(k), k          # some leaf of the transition holds an observed x <= 0 under its log link
    k_last = max(k for k, _, _ in run.nan_leaves)
    assert sum(int(r.is_accepted) for k, r, _ in trace if k > k_last) >= 1
    # the census run is the compared run
    np.testing.assert_array_equal(out[3]["leapfrogs"], OR.case_run(c, 20)[0][3]["leapfrogs"])


def test_link_specifications_parse_normalise_and_reject():
    assert host.obs_model_spec(None, 3).tolist() == [0, 0, 0] and host.obs_model_spec(None, 3).dtype == np.int32
    assert host.obs_model_spec("log", 3).tolist() == [1, 1, 1]
    assert host.obs_model_spec(["log", None, "sqrt", "identity", host.LINK_SQRT], 5).tolist() == [1, 0, 2, 0, 2]
    assert host.obs_model_spec_echo([1, 0, 2]) == ["log", "identity", "sqrt"]
    for bad in (["log"], ["log"] * 4, "logit", 7, ["log", "probit", None], [3, 0, 0], [True, None, None], [("log",), None, None]):
        with pytest.raises(ValueError):
            host.obs_model_spec(bad, 3)
    Xg = np.array([[1.0, np.nan], [np.nan, 0.0], [4.0, 9.0]])
    w = host.obs_weight_grid(np.array([[2.0, -1.0], [np.nan, 3.0], [0.5, 1.0]]), Xg)          # (entries at unobserved positions are ignored)
    assert w.tolist() == [[2.0, 1.0], [1.0, 3.0], [0.5, 1.0]] and host.obs_weight_grid(None, Xg) is None
    for bad in (np.ones((2, 2)), np.array([[0.0, 1], [1, 1], [1, 1]]), np.array([[1.0, 1], [1, np.inf], [1, 1]]), np.array([[1.0, 1], [1, 1], [-2.0, 1]])):
        with pytest.raises(ValueError):
            host.obs_weight_grid(bad, Xg)
    # data and start state against the links' domains: y = 0 is inside sqrt's and outside log's
    host.link_start_check([host.LINK_LOG, host.LINK_SQRT], Xg, np.array([[1.0, 1.0], [-5.0, 0.0], [3.0, 8.0]]))
    with pytest.raises(ValueError, match="component 1 has 1 observation"):
        host.link_start_check([host.LINK_LOG, host.LINK_LOG], Xg, np.ones((3, 2)))
    with pytest.raises(ValueError, match="Xhat_init of component 0 .* at 2 observed point"):
        host.link_start_check([host.LINK_LOG, host.LINK_SQRT], Xg, np.array([[0.0, 1.0], [1.0, 0.0], [-1.0, 8.0]]))
    with pytest.raises(ValueError, match="Xhat_init of component 1 .* at 1 observed point"):
        host.link_start_check([host.LINK_IDENTITY, host.LINK_SQRT], Xg, np.array([[-1.0, -1.0], [1.0, -1e-9], [-1.0, 8.0]]))


def test_sigma_defaults_live_on_the_links_scale():
    rng = np.random.default_rng(2)
    truth = np.stack([50.0 + 40.0 * np.sin(np.linspace(0, 3, 21)), 5.0 + np.linspace(0, 2, 21), np.linspace(1, 3, 21)], axis=1)
    Xg = truth * np.exp(0.1 * rng.standard_normal(truth.shape))
    Xg[1::2] = np.nan
    Xhat = truth.copy()
    links = np.array([host.LINK_LOG, host.LINK_IDENTITY, host.LINK_SQRT])
    LB0, s0 = host.sigma_sqs_lower_bound(Xhat), np.array([4.0, 0.3, 0.2])
    LB, start = host.link_sigma_defaults(links, Xg, Xhat, None, LB0, s0, False)
    seen = ~np.isnan(Xg[:, 0])
    assert LB[1] == LB0[1] and start[1] == s0[1]                                                # identity: the reference's values
    assert LB[0] == (0.01 * np.log(Xg[seen, 0]).std()) ** 2 and LB[2] == (0.01 * np.sqrt(Xg[seen, 2]).std()) ** 2
    assert start[0] == np.mean((np.log(Xhat[seen, 0]) - np.log(Xg[seen, 0])) ** 2) and 0.003 < start[0] < 0.03          # ~ 0.1^2, not 4.0
    w = np.where(seen[:, None], rng.uniform(0.5, 2.0, Xg.shape), 1.0)
    _, sw = host.link_sigma_defaults(links, Xg, Xhat, w, LB0, s0, False)
    r2 = (np.sqrt(Xhat[seen, 2]) - np.sqrt(Xg[seen, 2])) ** 2
    assert sw[2] == np.sum(w[seen, 2] * r2) / np.sum(w[seen, 2])
    # an explicit bound is taken as given; a mean square not above it, or fewer than two points inside the domain: (0.1 std g(y))^2
    LBg, sg = host.link_sigma_defaults(links, Xg, Xhat, None, np.array([1.0, 1.0, 1.0]), s0, True)
    assert LBg.tolist() == [1.0, 1.0, 1.0] and sg[0] == (0.1 * np.log(Xg[seen, 0]).std()) ** 2
    out = Xhat.copy(); out[2:, 0] = -1.0
    assert host.link_sigma_defaults(links, Xg, out, None, LB0, s0, False)[1][0] == (0.1 * np.log(Xg[seen, 0]).std()) ** 2


def test_the_end_to_end_chain_sits_on_no_knife_edge_and_the_link_moves_the_posterior():
    """The predator-prey data of the drop-in test on the oracle's own matrices: 200 + 200 transitions at depth <= 3 under log links and
    weights take the same leapfrogs with the operator products in longdouble and leave the posterior means of theta within 1/100 of the
    draw-for-draw bars; under identity links the chain is another one (the model is not vacuous on this data)."""
    pr, Xhat, s0, t0, w = OR.e2e_twin()
    th, out = OR.e2e_reference(pr, Xhat, s0, t0, OR.E2E["links"], w)
    th_l, out_l = OR.e2e_reference(pr, Xhat, s0, t0, OR.E2E["links"], w, long=True)
    np.testing.assert_array_equal(out[4]["all"]["leapfrogs"], out_l[4]["all"]["leapfrogs"])
    rtol, atol = U.BRANCH_TOL["th_pre"]
    frac = np.abs(th.mean(axis=0) - th_l.mean(axis=0)) / (atol + rtol * np.abs(th_l.mean(axis=0)))
    print("posterior means of theta under log links:", th.mean(axis=0).tolist(), "truth", OR.E2E["truth"], "; float64 vs longdouble, fraction of the bar:", frac.max())
    assert frac.max() <= 1e-2 and np.isfinite(th).all()
    assert np.isfinite(out[4]["all"]["target_log_prob"]).all() and np.mean(out[3]["is_accepted"]) > 0.8          # (the chain starts inside the domain and moves)
    th_i, out_i = OR.e2e_reference(pr, Xhat, s0, t0, None, None)
    moved = np.abs(th.mean(axis=0) - th_i.mean(axis=0)) / (atol + rtol * np.abs(th.mean(axis=0)))
    print("posterior means of theta under identity links (sigma^2 bounds and start as above):", th_i.mean(axis=0).tolist(), "; moved by", moved.max(), "x the bar")
    assert moved.max() >= 1000.0
