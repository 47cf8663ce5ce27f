"""Conditions on tests/metric_reference.py alone (no GPU): the reference of the diagonal-metric sampler is the oracle where it must be, its
whitening is the textbook scheme, the cases of tests/test_metric_gpu.py would expose a device that mis-applies the metric, and the pieces
around it (warm-up windows, window sums, regularisation) are what they claim to be."""
import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M

INTS = ("leapfrogs", "depth", "is_accepted", "has_divergence", "reach_max_depth")


@pytest.mark.parametrize("name", ["nuts_n41", "nuts_n41_stale", "hmc_n41"])
def test_identity_metric_is_the_oracles_chain_bit_for_bit(name):
    """s = 1, no window: the loop of metric_reference.sample_chain is orc.sample_chain's, NUTS and fixed-L HMC, stale cache both ways."""
    c = M.case(name)
    fx, pr, _ = M.seir_problem(c.N, c.band, c.dt)
    kw = M.oracle_kwargs(c)
    want = orc.sample_chain(pr, fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), c.results, c.burnin, chain=20, **kw)
    dim = pr.N * pr.D + pr.D + pr.P
    for metric in (None, {0: np.ones(dim)}):
        got = M.sample_chain(pr, fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), c.results, c.burnin, chain=20, metric=metric, **kw)
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b)
        for k, v in want[3].items():
            np.testing.assert_array_equal(got[3][k], v, err_msg=k)
        assert got[4]["da"] == want[4]


def test_whitened_hmc_is_the_q_space_scheme():
    """Fixed-L HMC in q with p ~ N(0, M), K = p^T M^-1 p / 2, q += eps M^-1 p against the oracle's step on z = q / s: the same accept flags,
    states and energies at 1e-12 relative.  (HMC only: the tree sees momentum through dot products that whitening preserves, and a
    q-space NUTS would be a second copy of it.)"""
    c = M.case("hmc_n41")
    pr, _, init, _ = M.case_problem(c)
    fn_L = orc.make_fn_L(pr)
    s = M.case_metric(c, 20)
    fz = M.whitened_fn(fn_L, s)
    q = orc.pack(*init)
    L, gL = fn_L(q)
    flags = []
    for k in range(8):
        temp = orc.temperature(k, 0.1)
        res = orc.hmc_one_step(q / s, temp * L, temp * (s * gL), 2e-4, temp, fz, k, 20, 808, 8)
        acc, qn, energy, _, tgt = M.hmc_one_step_qspace(q, temp * L, temp * gL, 2e-4, temp, fn_L, k, 20, 808, 8, s)
        assert acc == res.is_accepted
        np.testing.assert_allclose(qn, s * res.q, rtol=1e-12, atol=1e-12 * np.abs(q).max())
        np.testing.assert_allclose([energy, tgt], [res.energy, res.target_log_prob], rtol=1e-12)
        flags.append(acc)
        if acc:
            q = s * res.q
            L, gL = fn_L(q)
    assert 0 < sum(flags) <= len(flags)


@pytest.mark.parametrize("c", M.CASES, ids=repr)
def test_a_device_that_mis_applies_the_metric_changes_an_integer_diagnostic(c):
    """Per compared chain of the case: ignoring s, applying it to the momentum update or to the position update only, s^2 for s, and
    s = 1 on the D + P parameter entries each change an integer diagnostic of at least one transition (leapfrogs or depth under NUTS;
    the accept flags under fixed-L HMC, whose leapfrog count is fixed); s (1 +- 1e-9) changes none: no case sits on a knife-edge."""
    pr = M.case_problem(c)[0]
    ND = pr.N * pr.D
    with M.oracle_drifts(c):
        for chain in c.chains():
            s = M.case_metric(c, chain)
            ones = np.ones_like(s)
            ints = lambda run: [list(np.asarray(run[0][4]["all"][f]).astype(int)) for f in INTS]
            want = ints(M.case_run(c, chain))
            sp = s.copy()
            sp[ND:] = 1.0
            wrong = {"ignored": None, "momentum update only": {0: (ones, s)}, "position update only": {0: (s, ones)}, "s^2 for s": {0: s * s},
                     "parameter entries skipped": {0: sp}}
            for what, table in wrong.items():
                got = ints(M.case_run(c, chain, table) if table is not None else M.case_run(c, chain, None))
                assert got != want, (c.name, chain, what)
            for f in (1.0 + 1e-9, 1.0 - 1e-9):
                assert ints(M.case_run(c, chain, {0: s * f})) == want, (c.name, chain, f)


def test_warmup_schedule_tiles_the_adaptation_with_doubling_windows():
    assert host.warmup_schedule(1000, 0) == []
    assert host.warmup_schedule(40, 32, 8, 4, 8) == [(0, 8, False), (8, 12, True), (12, 24, True), (24, 32, False)]
    for num_burnin, n_adapt in ((1000, 800), (500, 400), (250, 200), (200, 150), (100, 80), (40, 32), (25, 20), (1250, 1000)):
        sch = host.warmup_schedule(num_burnin, n_adapt)
        assert sch[0][0] == 0 and sch[-1][1] == n_adapt
        assert all(a[1] == b[0] for a, b in zip(sch, sch[1:])) and all(a < b for a, b, _ in sch)
        slow = [(a, b) for a, b, m in sch if m]
        assert slow and not sch[0][2] and not sch[-1][2]
        if n_adapt >= 150:
            assert sch[0] == (0, 75, False) and sch[-1] == (n_adapt - 50, n_adapt, False)
            sizes = [b - a for a, b in slow]
            assert sizes[0] == 25 or len(sizes) == 1
            assert all(y == 2 * x for x, y in zip(sizes[:-2], sizes[1:-1]))              # every window but the stretched last one doubles
            assert len(sizes) == 1 or sizes[-1] >= 2 * sizes[-2]
        else:
            assert sch == [(0, int(0.15 * n_adapt), False), (int(0.15 * n_adapt), n_adapt - int(0.1 * n_adapt), True), (n_adapt - int(0.1 * n_adapt), n_adapt, False)]
    assert host.warmup_schedule(1000, 800)[1:-1] == [(75, 100, True), (100, 150, True), (150, 250, True), (250, 750, True)]
    with pytest.raises(ValueError):
        host.warmup_schedule(10, 11)


def test_shifted_sums_and_the_relative_floor_against_numpy():
    """A window whose variances span eight orders of magnitude, far from the origin: the shifted sums give numpy.var(ddof=1) in longdouble
    to 1e-12 relative; the median and the regularised values are numpy's exactly."""
    rng = np.random.default_rng(5)
    n, dim = 100, 257
    sd = 10.0 ** rng.uniform(-5, -1, dim)
    assert sd.max() ** 2 / sd.min() ** 2 > 1e7
    q0 = rng.uniform(0.5, 3.0, dim)
    states = q0[None] + np.cumsum(sd[None] * rng.standard_normal((n, dim)), axis=0) / np.sqrt(n)
    S1, S2 = M.window_sums(states, q0)
    s, var, med = M.metric_from_sums(S1, S2, n)
    want = np.var(states.astype(np.longdouble), axis=0, ddof=1)
    assert var.max() / var.min() > 1e7
    np.testing.assert_allclose(var, want.astype(np.float64), rtol=1e-12, atol=0)
    naive = (np.sum(states * states, axis=0) - np.sum(states, axis=0) ** 2 / n) / (n - 1)
    assert np.max(np.abs(naive / want.astype(np.float64) - 1.0)) > 1e-9          # (without the shift the small variances are lost)
    assert med == np.median(var)
    np.testing.assert_array_equal(s * s, np.sqrt(n / (n + 5.0) * var + 5.0 / (n + 5.0) * 1e-3 * np.median(var)) ** 2)
    assert M.metric_from_sums(np.zeros(dim), np.zeros(dim), n)[0] is None          # a chain that never moved keeps its metric
    moved = var.copy(); moved[:3] = 0.0
    s0 = M.metric_from_sums(np.zeros(dim), moved * (n - 1), n)[0]
    np.testing.assert_array_equal(s0[:3], np.sqrt(5.0 / (n + 5.0) * 1e-3 * np.median(moved)))      # var = 0: the floor term alone
    assert M.restart_step_size(0.1, np.ones(dim), s) == 0.1 / s.min()


def test_one_adapted_window_cuts_the_leapfrogs_per_transition():
    """The claim the feature exists for, on the reference alone: tests/util.synthetic_seir_problem(41) (spacing 0.025), SEIR-4, oracle-built
    matrices with the initial hyper-parameters, theta_0 = the generating parameters, temperature 1, depth <= 10, seed 808.  One warm-up of 40
    identity transitions and a 40-draw window, shared by both continuations; then 40 more adaptation transitions and 30 measured ones --
    with the window's metric (restart rule, 40 adaptation steps left) and with the identity metric going on.

    Measured: 271.8 against 715.8 leapfrogs per transition (step sizes 0.21 and 1.7e-5), a ratio of 2.63; asserted: half of it, a
    seed-to-seed margin.  Larger phases measure more (50 / 50 / 50 / 30: 3.6; 100 / 100 / 100 / 100: 133 against 680, 5.1) and take over a minute."""
    W, Wm = 40, 30
    fx, pr, _ = M.seir_problem(41)
    init = orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.array([6.0, 0.6, 1.8]), pr.LB)
    kw = dict(seed=808, chain=0, initial=init, anneal=False, stale_cache=False, max_tree_depth=10, step_size=0.01, num_adaptation_steps=3 * W)
    with np.errstate(all="ignore"):
        adapted = M.sample_chain(pr, None, None, None, Wm, 3 * W, windows=[(W, 2 * W)], fork_at=2 * W, **kw)
        identity = M.sample_chain(pr, None, None, None, Wm, 3 * W, resume=adapted[4]["fork"], **kw)
    la, li = adapted[4]["all"]["leapfrogs"], identity[4]["all"]["leapfrogs"]
    np.testing.assert_array_equal(adapted[4]["all"]["step_size"][2 * W], adapted[4]["adapted"][0]["step_size"])
    assert identity[4]["s"] is None and adapted[4]["s"] is not None
    ratio = li[3 * W:].mean() / la[3 * W:].mean()
    print(f"leapfrogs per transition: identity {li[3 * W:].mean():.1f}, adapted {la[3 * W:].mean():.1f}, ratio {ratio:.2f}")
    assert ratio >= 2.63 / 2
