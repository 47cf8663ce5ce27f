"""The proof that the cases of tests/test_nonfinite_gpu.py see what they claim -- all of it on the CPU, with the oracle alone.

A leapfrog step that leaves the domain of a drift (a negative argument of ``sqrt`` or ``log``) gives a NaN log posterior, hence a NaN energy.
TFP, the oracle (``orc.nuts_one_step`` / ``orc.hmc_one_step``) and csrc/decide.h count such a leaf as energy -inf: it diverges, is never chosen and
ends its sub-tree and the transition.  The table ``tests.util.DOMAIN_CASES`` runs the two drifts of ``drift_examples.DOMAIN_EXAMPLES`` (a square-root
law, separable; a logarithmic one, not separable) from theta_0 = 1 at step sizes where that happens.  Here:

* CLAIMS: every claim of ``tests.util.DOMAIN_BRANCHES`` is made by a case and every case takes what it claims (census of chains 20 and 21, ordered
  by ``tests.util.Census``), within <= 12 transitions, <= 127 leapfrogs per transition, N = 41 (one case N = 161, two operator blocks, band 20);
* MARGIN: oracle and device agree on which leaf is outside the domain unless an argument of ``sqrt`` / ``log`` is within rounding of 0.  Over every
  state the oracle's drift is given in the compared chains, every such argument has |x| >= 1e-6 max|X| -- 100 x the device tolerance on X;
* ROBUSTNESS: every case runs a second time on another summation order of the log posterior (the C port does not carry traced drifts: the three
  operator products in ``np.longdouble``, local to this file): identical integer diagnostics, non-finite entries in the same places, every
  compared finite float within 1/100 of its device tolerance;
* SENSITIVITY: the NaN rule removed from (a copy of) the oracle's transition functions.  With a NaN energy comparing as "not divergent" the integer
  diagnostics of every case change.  With the energy merely left NaN, NUTS does NOT change: every comparison with NaN is false, so the leaf
  still diverges and is never chosen -- the rule matters where the device's ``fmin`` drops a NaN operand, the acceptance statistic
  exp(fmin(ediff, 0)) of fixed-L HMC, which is 1 instead of 0 without it; with that modelled the HMC cases change."""
import inspect

import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import util as U
from tests.test_sampler_branches_cpu import INT_FIELDS, _ints

CASES = U.DOMAIN_CASES
FLOATS = dict(U.BRANCH_TOL, energy=U.ENERGY_TOL)


def _runs(case, **kw):
    return {ch: U.domain_oracle_run(case, ch, **kw) for ch in U.BRANCH_CHAINS}


def _fields(run):
    col = lambda f: np.array([getattr(r, f) for _, r, _ in run.trace], dtype=np.float64)
    return {"step_size": np.array([s for _, _, s in run.trace]), "log_accept_ratio": col("log_accept_ratio"), "target_log_prob": col("target_log_prob"),
            "energy": col("energy"), "X": run.out[0], "sig_pre": run.out[1], "th_pre": run.out[2]}


def test_every_claim_is_made_by_a_case():
    claimed = {b for c in CASES for b in c.claims}
    assert claimed == set(U.DOMAIN_BRANCHES), set(U.DOMAIN_BRANCHES) ^ claimed
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.tag for c in CASES} == set(U.DOMAIN_TRUTH)                                          # both drifts
    assert sorted(c.N for c in CASES if c.N != 41) == [161]
    nine = [c for c in CASES if 9 in c.batches]                                                   # the 16-wide mirror: once per drift
    assert {c.tag for c in nine} == set(U.DOMAIN_TRUTH)
    for tag in U.DOMAIN_TRUTH:                                                                    # fixed-L HMC on both kernels
        assert any(c.tag == tag and "hmc_nan" in c.claims for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_takes_what_it_claims(case):
    runs = _runs(case)
    for ch, r in runs.items():
        print(case.name, ch, "leapfrogs", _ints(r.trace)["leapfrogs"], "NaN leaves (transition, leaf, depth)", r.nan_leaves, "ordinary", r.ordinary)
    assert case.claims
    for b in case.claims:
        assert U.DOMAIN_BRANCHES[b](case, runs), (case.name, b)
    for ch, r in runs.items():
        assert len(r.trace) <= 12 and max(x.leapfrogs for _, x, _ in r.trace) <= 127
        assert len(r.evals) == 1 + sum(x.leapfrogs for _, x, _ in r.trace)
        assert all(np.isfinite(a).all() for a in r.out[:3])                                       # every kept state is finite
        if "interior" not in case.claims and "hmc_nan" not in case.claims:
            assert r.events[("nan",)] > 0                                                         # both compared chains take NaN leaves
            for k in r.nan_transitions():
                assert r.trace[k][1].has_divergence and r.outside(k)                              # (the census and the recorded states agree)


def test_the_two_kinds_of_divergence_are_told_apart():
    """A NaN leaf is outside the domain (or follows such a state); an ordinary divergent leaf has a finite state inside it."""
    for case in CASES:
        if "hmc_nan" in case.claims:
            continue
        for r in _runs(case).values():
            leaves = {k: [] for k in range(len(r.trace))}
            for k, it, d in r.nan_leaves:
                leaves[k].append(True)
            for k, it, d in r.ordinary:
                leaves[k].append(False)
            for k, kinds in leaves.items():
                assert len(kinds) <= 1                                                            # (a divergent leaf ends the transition)
                if kinds:
                    last = r.first_eval[k] + r.trace[k][1].leapfrogs - 1
                    assert (not r.evals[last][0] > 0.0) == kinds[0], (case.name, k)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_no_leaf_is_within_rounding_of_the_edge_of_the_domain(case):
    worst = np.inf
    for r in _runs(case).values():
        for lo, big, near in r.evals:
            if np.isfinite(big):
                worst = min(worst, near / big)
    print(case.name, f"smallest |argument of sqrt / log| / max|X| over all evaluated states: {worst:.1e}")
    assert worst >= U.DOMAIN_MARGIN, (case.name, worst)


_long = {}


def _longdouble_logpost_grad(X, sig_pre, th_pre, beta_temp, pr):
    """orc.logpost_grad with the three operator products (and the sums over them) in np.longdouble: another summation order and precision."""
    if id(pr) not in _long:
        _long[id(pr)] = tuple(np.asarray(a, dtype=np.longdouble) for a in (pr.C_inv, pr.m, pr.K_inv))
    Ci, m, Ki = _long[id(pr)]
    T = lambda a: np.transpose(a, (0, 2, 1))
    D = pr.D
    sp_s = np.log(1.0 + np.exp(sig_pre))
    sigma_sqs = sp_s + pr.LB
    thetas = np.log(1.0 + np.exp(th_pre))
    sg_s, sg_t = 1.0 / (1.0 + np.exp(-sig_pre)), 1.0 / (1.0 + np.exp(-th_pre))
    lj_s, lj_t = np.sum(sig_pre - sp_s), np.sum(th_pre - np.log(1.0 + np.exp(th_pre)))
    xc = np.asarray((X - pr.mu).T[:, :, None], dtype=np.longdouble)
    Cx, CTx = Ci @ xc, T(Ci) @ xc
    t1 = np.sum(xc * Cx)
    f, J, Tm = orc.DRIFTS[pr.drift][0](X, thetas)
    r = np.asarray(f.T[:, :, None], dtype=np.longdouble) - m @ xc
    Kr, KTr = Ki @ r, T(Ki) @ r
    t2 = np.sum(r * Kr)
    g = (Kr + KTr)[:, :, 0]
    t3 = np.sum(pr.N_ds * np.log(2.0 * np.pi * sigma_sqs))
    cols = pr.obs_idx % D
    resid = X.reshape(-1)[pr.obs_idx] - pr.y
    t4 = np.sum(np.square(resid) * (1.0 / sigma_sqs)[cols])
    logp = float(beta_temp * (-0.5 * (((1.0 / pr.beta) * (t1 + t2)) + (t3 + t4)) + lj_s + lj_t))
    mTg = (T(m) @ g[:, :, None])[:, :, 0]
    d12 = ((Cx + CTx)[:, :, 0] - mTg + np.einsum("dn,nde->en", g, np.asarray(J, dtype=np.longdouble))).astype(np.float64)
    d4 = np.zeros(X.size)
    np.add.at(d4, pr.obs_idx, 2.0 * resid / sigma_sqs[cols])
    gX = beta_temp * (-0.5 * ((1.0 / pr.beta) * d12.T + d4.reshape(X.shape)))
    SS = np.zeros(D)
    np.add.at(SS, cols, np.square(resid))
    gsig = beta_temp * (-0.5 * (pr.N_ds / sigma_sqs - SS / sigma_sqs ** 2) * sg_s + (1.0 - sg_s))
    dth = np.einsum("dn,ndp->p", g, np.asarray(Tm, dtype=np.longdouble)).astype(np.float64)
    gth = beta_temp * (-0.5 * (1.0 / pr.beta) * dth * sg_t + (1.0 - sg_t))
    return logp, gX, gsig, gth


def test_the_longdouble_restatement_is_the_oracles_log_posterior():
    case = U.domain_case("sqrt_deep")
    fx, pr, _ = U.domain_problem(case)
    X0, s0, t0 = orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), pr.LB)
    with U.domain_drifts():
        a, b = orc.logpost_grad(X0, s0, t0, 0.7, pr), _longdouble_logpost_grad(X0, s0, t0, 0.7, pr)
    assert abs(a[0] - b[0]) <= 1e-10 * abs(a[0]) and a[0] != b[0]                                 # the same function, another rounding
    for u, v in zip(a[1:], b[1:]):
        np.testing.assert_allclose(v, u, rtol=0, atol=1e-10 * np.abs(a[1]).max())
    X1 = X0.copy()
    X1[7, 0] = -0.05                                                                              # one entry outside: NaN on both sides
    with np.errstate(all="ignore"), U.domain_drifts():
        assert np.isnan(orc.logpost_grad(X1, s0, t0, 0.7, pr)[0]) and np.isnan(_longdouble_logpost_grad(X1, s0, t0, 0.7, pr)[0])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_no_decision_of_the_case_sits_on_a_rounding_knife_edge(case):
    worst = {}
    with np.errstate(all="ignore"):
        second = _runs(case, logpost_grad=_longdouble_logpost_grad)
    for ch, a in _runs(case).items():
        b = second[ch]
        assert _ints(a.trace) == _ints(b.trace), (case.name, ch)
        assert a.nan_leaves == b.nan_leaves and a.ordinary == b.ordinary
        fa, fb = _fields(a), _fields(b)
        for k, (rtol, atol) in FLOATS.items():
            u, v = fa[k], fb[k]
            np.testing.assert_array_equal(np.isfinite(u), np.isfinite(v), err_msg=f"{case.name} {k}")
            np.testing.assert_array_equal(u[~np.isfinite(u)], v[~np.isfinite(v)], err_msg=f"{case.name} {k}")     # (-inf where -inf)
            fin = np.isfinite(u)
            if k == "X":
                atol = atol * np.abs(v).max()
            d = np.abs(u - v)[fin] / (atol + rtol * np.abs(v)[fin])
            worst[k] = max(worst.get(k, 0.0), float(d.max()) if d.size else 0.0)
    print(case.name, "float64 vs longdouble operator products, fraction of the device tolerance:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-2, (case.name, k, v)


# ---- sensitivity: the oracle without its NaN rule ------------------------------------------------------------------------------------
RULE = "if np.isnan(energy):"
BOUND = "not_divergent = bool(-ediff < max_energy_diff)"
HMC_STAT = "lar = min(ediff, 0.0) if np.isfinite(ediff) or ediff == -np.inf else -np.inf"


def _mutated(fn, swaps):
    """A copy of an oracle function with lines of its source replaced (each must occur exactly once), living in the oracle's namespace."""
    src = inspect.getsource(fn)
    for old, new in swaps:
        assert src.count(old) == 1, (fn.__name__, old)
        src = src.replace(old, new)
    ns = {}
    exec(compile(src, f"<{fn.__name__} without the NaN rule>", "exec"), vars(orc), ns)
    return ns[fn.__name__]


# NaN compares as "not divergent": the rule gone and the bound written the other way round, !(-ediff >= bound)
NOT_DIVERGENT = [(RULE, "if False:"), (BOUND, "not_divergent = not (-ediff >= max_energy_diff)")]
# the energy left NaN; in HMC the device's statistic exp(fmin(ediff, 0)) with C's fmin, which returns the operand that is not NaN
LEFT_NAN = [(RULE, "if False:")]
LEFT_NAN_HMC = LEFT_NAN + [(HMC_STAT, "lar = 0.0 if ediff != ediff else min(ediff, 0.0)")]


def _without_the_rule(case, monkeypatch, nuts_swaps, hmc_swaps):
    monkeypatch.setattr(orc, "nuts_one_step", _mutated(orc.nuts_one_step, nuts_swaps))
    monkeypatch.setattr(orc, "hmc_one_step", _mutated(orc.hmc_one_step, hmc_swaps))
    try:
        with np.errstate(all="ignore"):
            return U.domain_oracle_run(case, U.BRANCH_CHAINS[0], cache=False)
    finally:
        monkeypatch.undo()


def _same(a, b):
    return _ints(a.trace) == _ints(b.trace) and all(np.array_equal(u, v) for u, v in zip(a.out[:3], b.out[:3]))


NAN_CASES = [c for c in CASES if "interior" not in c.claims]


@pytest.mark.parametrize("case", NAN_CASES, ids=repr)
def test_a_device_on_which_nan_is_not_divergent_would_fail_the_case(case, monkeypatch):
    ref = U.domain_oracle_run(case, U.BRANCH_CHAINS[0])
    got = _without_the_rule(case, monkeypatch, NOT_DIVERGENT, NOT_DIVERGENT)
    assert orc.nuts_one_step.__module__ == orc.__name__ and _same(ref, U.domain_oracle_run(case, U.BRANCH_CHAINS[0], cache=False))
    print(case.name, {f: (_ints(ref.trace)[f], _ints(got.trace)[f]) for f in INT_FIELDS if _ints(ref.trace)[f] != _ints(got.trace)[f]})
    assert _ints(got.trace) != _ints(ref.trace)


@pytest.mark.parametrize("case", NAN_CASES, ids=repr)
def test_a_device_that_left_the_energy_nan(case, monkeypatch):
    """HMC: the acceptance statistic of a trajectory that ends outside the domain is 1 instead of 0, dual averaging moves the step size the other
    way and the chain is another one.  NUTS: nothing changes (module docstring) -- the leaf diverges through the comparison itself."""
    ref = U.domain_oracle_run(case, U.BRANCH_CHAINS[0])
    got = _without_the_rule(case, monkeypatch, LEFT_NAN, LEFT_NAN_HMC)
    if "hmc_nan" in case.claims:
        lar = lambda r: [x.log_accept_ratio for _, x, _ in r.trace]
        assert lar(got) != lar(ref) and not _same(ref, got)
    else:
        assert _same(ref, got)


def test_interior_member_never_sees_the_rule(monkeypatch):
    case = U.domain_case("sqrt_interior")
    assert _same(U.domain_oracle_run(case, U.BRANCH_CHAINS[0]), _without_the_rule(case, monkeypatch, NOT_DIVERGENT, NOT_DIVERGENT))
