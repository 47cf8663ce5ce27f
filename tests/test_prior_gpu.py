"""Priors on theta and sigma^2 and known noise variances on the device (magi_set_prior) against tests/prior_reference.py.

Tolerances are the project's own: ``tests.util.BRANCH_TOL`` / ``ENERGY_TOL`` for sampler runs, the bars of tests/test_support_gpu.py for the
log posterior and its gradient (1e-9 max|g_X| absolute, 1e-7 relative on the parameter gradients), the bars of tests/test_summary_gpu.py for
summaries; integer diagnostics are compared exactly.  tests/test_prior_cpu.py holds the reference and the case table on the CPU."""
import ctypes as C

import numpy as np
import pytest

from magi_v2_amd import host
from magi_v2_amd.engine import MagiEngine, MagiHipError
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import prior_reference as PR
from tests import support_reference as S
from tests import util as U
from tests.test_metric_gpu import _assert_chain, _cfg, _ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_drift_table_left_as_found():
    """The traced drifts the cases register with the oracle (``orc.DRIFTS``) go when the module is done: other tests iterate over that table."""
    before = set(orc.DRIFTS)
    yield
    for name in set(orc.DRIFTS) - before:
        del orc.DRIFTS[name]


def _engine(c, family="auto"):
    _, dense, _, d = S.case_problem(c)
    return U.engine_for(dense, c.band, drift=d, options={"stream_family": family})


def _states(c, n):
    return tuple(np.repeat(np.asarray(v)[None], n, axis=0) for v in PR.case_init(c))


def _set(eng, c):
    eng.set_theta_support(c.spec)
    eng.set_prior(c.sig_prior, c.th_prior)


def _assert_logpost(eng, pr, sig_prior, th_prior, sup, X, sp, tp, where, temp=1.0):
    """Three-phase, fused and the sampler's own first evaluation against the reference at the bars of tests/test_support_gpu.py."""
    L, gX, gs, gt = PR.logpost_grad_prior(sig_prior, th_prior, *sup)(X, sp, tp, temp, pr)
    for fused in (False, True):
        out = eng.logpost_grad(X, sp, tp, temp, fused=fused)
        print(f"{where} fused={fused}: logp rel {abs(out[0] - L) / abs(L):.2e}, gX {np.abs(out[1] - gX).max() / np.abs(gX).max():.2e}, "
              f"gsig {np.abs(out[2] - gs).max() / np.abs(gX).max():.2e}, gth {np.abs(out[3] - gt).max() / np.abs(gX).max():.2e} of max|gX|")
        assert abs(out[0] - L) <= 1e-9 * abs(L), (where, fused)
        np.testing.assert_allclose(out[1], gX, rtol=0, atol=1e-9 * np.abs(gX).max(), err_msg=where)
        np.testing.assert_allclose(out[2], gs, rtol=1e-7, atol=1e-9 * np.abs(gX).max(), err_msg=where)
        np.testing.assert_allclose(out[3], gt, rtol=1e-7, atol=1e-9 * np.abs(gX).max(), err_msg=where)
    # the sampler: one fixed-L transition of one leapfrog at a step of 1e-14 -- its target is the log posterior of the start (the state
    # moves by ~1e-13, the value by less than 1e-9 |L| / 100), whether the transition is accepted or not
    L1 = PR.logpost_grad_prior(sig_prior, th_prior, *sup)(X, sp, tp, 1.0, pr)[0]
    cfg = eng.default_cfg(num_results=1, num_burnin_steps=0, mode=1, hmc_leapfrogs=1, step_size=1e-14, anneal=0, stale_cache=0)
    eng.sampler_init(cfg, X[None], sp[None], tp[None], seed=7)
    eng.sampler_run(1)
    got = eng.sampler_diag().target_log_prob[0, 0]
    print(f"{where} sampler: logp rel {abs(got - L1) / abs(L1):.2e}")
    assert abs(got - L1) <= 1e-9 * abs(L1), where


def _tables(pr, spec, sig_spec, th_spec):
    sup = host.theta_support(spec, pr.P)
    return sup, host.prior_spec(sig_spec, pr.D, "sigma_sq"), host.prior_spec(th_spec, pr.P, "theta", sup)


def test_log_posterior_and_gradient_on_the_golden_seir4_n81_and_sirw_n41():
    for tag, spec, sig_spec, th_spec in (
            ("seir4_N81", ["positive", ("lower", 0.0), ("upper", 9.0)], [("invgamma", 3.0, 1e-3), ("fixed", 4e-4), ("gamma", 2.0, 2e3), ("lognormal", -7.0, 1.0)],
             [("gamma", 3.0, 2.0), ("invgamma", 2.5, 1.0), ("normal", 2.0, 0.3)]),
            ("sirw_N41", None, [("normal", 1e-4, 5e-5), None, "flat", ("fixed", 2e-5)],
             [("lognormal", -1.0, 0.4), "flat", ("gamma", 1.5, 30.0), ("invgamma", 3.0, 0.2), ("normal", 0.02, 0.01)])):
        g = U.load_g4(tag)
        pr = U.problem_from_g4(g, None)
        sup, sp_, tp_ = _tables(pr, spec, sig_spec, th_spec)
        eng = U.engine_for(pr, None)
        try:
            eng.set_theta_support(spec)
            eng.set_prior(sig_spec, th_spec)
            (ks, a, b), (kt, at, bt) = eng.prior()
            assert ks.tolist() == sp_[0].tolist() and kt.tolist() == tp_[0].tolist() and a.tolist() == sp_[1].tolist() and bt.tolist() == tp_[2].tolist()
            for i in (0, 1):
                th = host.theta_pre_inits(host.transform_samples(g["state_sig_pre"][i], g["state_th_pre"][i], pr.LB)[1], *sup)
                _assert_logpost(eng, pr, sp_, tp_, sup, g["state_X"][i], g["state_sig_pre"][i], th, f"{tag} state {i}", temp=(1.0, 0.37)[i])
        finally:
            eng.close()


def test_log_posterior_and_gradient_on_a_structureless_fixture_of_two_blocks():
    from tests.test_structureless_cpu import fixture
    pr, X = fixture(129, "seir4")
    spec = [("upper", 9.0), "real", ("lower", 1.0)]
    sig_spec = [("gamma", 2.0, 10.0), ("fixed", 0.06), ("lognormal", -3.0, 0.7), ("invgamma", 4.0, 0.2)]
    th_spec = [("normal", 5.0, 1.0), ("normal", 0.0, 2.0), ("lognormal", 0.5, 0.5)]
    sup, sp_, tp_ = _tables(pr, spec, sig_spec, th_spec)
    eng = U.engine_for(pr)
    try:
        eng.set_theta_support(spec)
        eng.set_prior(sig_spec, th_spec)
        Xb, sp, tp = U.structureless_states(pr, X, 2, 3)
        tp = host.theta_pre_inits(host.transform_samples(sp, tp, pr.LB)[1], *sup)
        tp[1, 1] = -0.45                                        # a real entry at a negative pre
        for i in range(2):
            _assert_logpost(eng, pr, sp_, tp_, sup, Xb[i], sp[i], tp[i], f"structureless seir4 N=129 state {i}")
    finally:
        eng.close()


def test_log_posterior_and_gradient_of_eight_chains_every_parameter_lane_another_kind():
    """chain8: D = 8, P = 8 -- all sixteen parameter lanes carry a prior, every kind on both blocks, under every compatible support; the
    eight states go through the API as one batch of eight chains."""
    from tests import test_drift_edges_cpu as E
    spec = ["positive", "real", ("lower", 0.1), ("upper", 2.0), "real", ("upper", 1.5), ("lower", 0.0), "positive"]
    sig_spec = [("normal", 0.05, 0.02), ("lognormal", -3.0, 0.8), ("gamma", 2.0, 20.0), ("invgamma", 3.0, 0.1), ("fixed", 0.04), ("gamma", 1.5, 5.0), "flat",
                ("invgamma", 2.0, 0.05)]
    th_spec = [("lognormal", -0.5, 0.6), ("normal", 0.8, 0.5), ("gamma", 3.0, 4.0), ("normal", 0.9, 0.2), "flat", ("normal", 0.5, 0.4), ("invgamma", 3.0, 1.2),
               ("gamma", 2.0, 1.5)]
    with E.edge_drifts():
        pr, X = E.fixture("chain8")
        sup, sp_, tp_ = _tables(pr, spec, sig_spec, th_spec)
        eng = U.engine_for(pr, drift=E.traced("chain8"))
        try:
            eng.set_theta_support(spec)
            eng.set_prior(sig_spec, th_spec)
            Xb, sp, tp = U.structureless_states(pr, X, 8, 5)
            tp = host.theta_pre_inits(host.transform_samples(sp, tp, pr.LB)[1], *sup)
            tp[1, 4] = -0.3                                     # a real entry at a negative pre
            fn = PR.logpost_grad_prior(sp_, tp_, *sup)
            for fused in (False, True):
                out = eng.logpost_grad(Xb, sp, tp, 0.6, fused=fused)
                for i in range(8):
                    L, gX, gs, gt = fn(Xb[i], sp[i], tp[i], 0.6, pr)
                    assert abs(out[0][i] - L) <= 1e-9 * abs(L), (i, fused)
                    np.testing.assert_allclose(out[1][i], gX, rtol=0, atol=1e-9 * np.abs(gX).max())
                    np.testing.assert_allclose(out[2][i], gs, rtol=1e-7, atol=1e-9 * np.abs(gX).max())
                    np.testing.assert_allclose(out[3][i], gt, rtol=1e-7, atol=1e-9 * np.abs(gX).max())
            _assert_logpost(eng, pr, sp_, tp_, sup, Xb[3], sp[3], tp[3], "chain8 N=129 state 3")
        finally:
            eng.close()


@pytest.mark.parametrize("c,chains,family", [(c, n, f) for c in PR.CASES for n, f in c.runs], ids=repr)
def test_sampler_matches_the_reference_draw_for_draw(c, chains, family):
    """The table of tests/prior_reference.py, annealing on (the prior is tempered with the rest): every kind on a sigma^2 entry with one
    variance fixed, normal priors on a real and an upper-bounded parameter and a lognormal one on a lower-bounded; NUTS on k_stream<1>, <2>,
    k_stream_sep<8>, <16>, fixed-L HMC, N = 161 under band 20, a non-separable traced drift on k_stream_mc, a warm-up that adapts the metric.
    Chain ids 20 ..., the first and the last compared."""
    ids = _ids(chains)
    eng = _engine(c, family)
    try:
        name = eng.stream_kernel_name(chains)
        want = {1: "k_stream<1>", 2: "k_stream<2>"}.get(chains, "k_stream_mc" if c.drift == "ptrans" else "k_stream_sep")
        assert name.startswith(want), name
        if chains in (8, 9) and c.drift != "ptrans":
            assert ("16" in name) == (chains == 9), name
        _set(eng, c)
        eng.sampler_init(_cfg(eng, c), *_states(c, chains), seed=c.seed, chain_ids=ids)
        lf, _ = eng.sampler_run(c.burnin + c.results)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert lf == d.leapfrogs_taken.sum()
    for i in sorted({0, chains - 1}):
        _assert_chain(f"{c.name} {name} chain {ids[i]}", i, d, samples, PR.case_run(c, ids[i])[0], c.burnin)


@pytest.mark.parametrize("chains", [1, 2])
def test_warmup_that_adapts_the_metric_matches_the_reference_under_priors(chains):
    """sampler_warmup over warmup_schedule(40, 32, 8, 4, 8) on the N = 41 case under its priors (prior_reference.WARM): two windows become
    metrics, dual averaging restarts, then 13 more transitions, 5 of them results.  Every diagnostic of the 45 transitions and the results."""
    c, w = PR.case("nuts_n41"), PR.WARM
    ids = _ids(chains)
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.sampler_init(_cfg(eng, c, num_burnin_steps=w["burnin"], num_results=w["results"], max_tree_depth=w["max_tree_depth"]), *_states(c, chains),
                         seed=w["seed"], chain_ids=ids)
        _, _, windows = eng.sampler_warmup(host.warmup_schedule(*w["sched"]))
        eng.sampler_run(w["burnin"] + w["results"] - w["sched"][1])
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert [(x["start"], x["stop"]) for x in windows] == [(8, 12), (12, 24)]
    for i in sorted({0, chains - 1}):
        _assert_chain(f"warm-up chain {ids[i]}", i, d, samples, PR.warm_run(ids[i]), w["burnin"])


def _run(c, chains, family, how):
    """how: "never" (no call), "flat" (every entry flat explicitly), "none" (set_prior(None, None))."""
    eng = _engine(c, family)
    try:
        pr = M.case_problem(c)[0]
        if how == "flat":
            eng.set_prior(["flat"] * pr.D, [None] * pr.P)
        elif how == "none":
            eng.set_prior(None, None)
        init = M.case_problem(c)[2]
        eng.sampler_init(_cfg(eng, c), *[np.repeat(np.asarray(v)[None], chains, axis=0) for v in init], seed=c.seed, chain_ids=_ids(chains))
        eng.sampler_run(c.burnin + c.results)
        return eng.stream_kernel_name(chains), eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()


def _assert_same_run(a, b):
    (_, sa, da), (_, sb, db) = a, b
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)
    for f in da.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(da, f), getattr(db, f), err_msg=f)


@pytest.mark.parametrize("case,chains,family", [("nuts_n41", 1, "auto"), ("nuts_n41", 2, "auto"), ("nuts_n41", 3, "mc"), ("nuts_ptrans_n41", 3, "mc")])
def test_every_entry_flat_set_explicitly_is_the_prior_never_set_bit_for_bit(case, chains, family):
    """Samples and every diagnostic, one kernel of each family (k_stream<1>, <2>, k_stream_sep, k_stream_mc); the cases of the metric table."""
    c = M.case(case)
    never = _run(c, chains, family, "never")
    for how in ("flat", "none"):
        _assert_same_run(never, _run(c, chains, family, how))
    assert never[2].leapfrogs_taken.max() >= 31


@pytest.mark.parametrize("per", [1, 2])
def test_group_members_with_different_priors_equal_their_own_handles_bit_for_bit(per):
    """Two members of one shape on k_stream_group<1> and <2>: the priors of the N = 41 case, and others with another variance fixed."""
    c = PR.case("nuts_n41")
    priors = [(c.sig_prior, c.th_prior), ([("fixed", 3e-4), ("gamma", 2.0, 3e3), None, ("invgamma", 3.0, 3e-4)], [("normal", 0.0, 0.3), None, ("normal", 1.2, 0.1)])]
    start = _states(c, per)
    ids = _ids(per)
    own = []
    for sg, th in priors:
        eng = _engine(c)
        try:
            eng.set_theta_support(c.spec)
            eng.set_prior(sg, th)
            eng.sampler_init(_cfg(eng, c), *start, seed=c.seed, chain_ids=ids)
            eng.sampler_run(c.burnin + c.results)
            own.append((eng.sampler_samples(), eng.sampler_diag(), eng.sampler_summary()))
        finally:
            eng.close()
    engs = [_engine(c) for _ in priors]
    try:
        for e, (sg, th) in zip(engs, priors):
            e.set_theta_support(c.spec)
            e.set_prior(sg, th)
        g = MagiEngine.group(engs)
        try:
            with pytest.raises(MagiHipError) as err:
                g.set_prior(c.sig_prior, c.th_prior)
            assert err.value.code == -5
            both = [np.concatenate([v, v]) for v in start]
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
            np.testing.assert_array_equal(sums[m]["sigma_sqs"][stat], own[m][2]["sigma_sqs"][stat])
    assert sums[0]["sigma_sqs"]["mean"][1] == 2.5e-4 and sums[1]["sigma_sqs"]["mean"][0] == 3e-4


def _assert_sigma_summary(got, sig):
    """mean / sd / quantiles of the sigma^2 block against numpy on the transformed draws sig [chains, draws, D], at the bars
    tests/test_summary_gpu.py holds the same statistics to."""
    from tests import summary_reference as sr
    probs = tuple(got.get("probs", (0.025, 0.5, 0.975)))
    ref = sr.summarize(np.asarray(sig), probs)
    block = dict(got, probs=np.asarray(probs), n_nonfinite=ref["n_nonfinite"])
    worst = sr.check_against(block, ref, sigma_theta=True)
    print("sigma^2 summary, worst error / bar:", worst)


def test_sampler_summary_reports_a_fixed_variance_as_its_constant():
    c = PR.case("nuts_n41")
    _, sp_, _ = PR.case_tables(c.name)
    pr = S.case_problem(c)[0]
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.sampler_init(_cfg(eng, c, num_results=8, max_tree_depth=4), *_states(c, 2), seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(c.burnin + 8)
        _, sp, tp = eng.sampler_samples()
        summ = eng.sampler_summary()
    finally:
        eng.close()
    sig = host.transform_samples(sp, tp, pr.LB, sp_)[0]
    assert (sig[..., 1] == 2.5e-4).all() and np.ptp(sp[..., 1]) > 0.0          # (the constant, while its pre coordinate moves)
    assert summ["sigma_sqs"]["mean"][1] == 2.5e-4 and summ["sigma_sqs"]["quantiles"][:, 1].tolist() == [2.5e-4] * 3
    keep = [0, 2, 3]                                                            # (a constant column has no sd-relative bar: compared above, exactly)
    block = {k: (np.asarray(v)[..., keep] if isinstance(v, np.ndarray) and v.shape[-1:] == (4,) else v) for k, v in summ["sigma_sqs"].items()}
    _assert_sigma_summary(block, sig[..., keep])


def test_checkpoint_resumes_under_the_same_priors_and_is_refused_under_others():
    c = PR.case("nuts_n41")
    total = c.burnin + c.results
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.sampler_init(_cfg(eng, c), *_states(c, 2), seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(3)
        ck = eng.sampler_checkpoint()
        eng.sampler_run(total - 3)
        whole = (eng.sampler_samples(), eng.sampler_diag())
    finally:
        eng.close()
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=[20, 21])
        eng.sampler_run(total - 3)
        (sa, da), (sb, db) = whole, (eng.sampler_samples(), eng.sampler_diag())
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(da.leapfrogs_taken[:, 3:], db.leapfrogs_taken[:, 3:])
        np.testing.assert_array_equal(da.energy[:, 3:], db.energy[:, 3:])
        other_sig = list(c.sig_prior)
        other_sig[1] = ("fixed", 2.6e-4)
        for sg, th in ((None, None), (other_sig, c.th_prior), (c.sig_prior, [c.th_prior[0], c.th_prior[1], None])):
            eng.set_prior(sg, th)
            with pytest.raises(MagiHipError) as err:
                eng.sampler_resume(_cfg(eng, c), ck, seed=c.seed, chain_ids=[20, 21])
            assert err.value.code == -1
    finally:
        eng.close()


def _run_with_priors(c):
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.sampler_init(_cfg(eng, c), *_states(c, 1), seed=c.seed, chain_ids=[20])
        eng.sampler_run(c.burnin + c.results)
        return "", eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()


def test_bad_arguments_are_rejected_and_leave_the_handle_as_it_was():
    c = PR.case("nuts_n41")
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    good = _run_with_priors(c)
    (_, (ks, as_, bs), (kt, at, bt)) = PR.case_tables(c.name)
    K, A, B = np.concatenate([ks, kt]), np.concatenate([as_, at]), np.concatenate([bs, bt])
    eng = _engine(c)
    try:
        _set(eng, c)
        lib, h = eng._lib, eng._h
        arr = lambda v, t, p: None if v is None else np.asarray(v, dtype=t).ctypes.data_as(p)
        call = lambda n, k, a, b: lib.magi_set_prior(h, n, arr(k, np.int32, ip), arr(a, np.float64, dp), arr(b, np.float64, dp))
        def changed(j, k=None, a=None, b=None):
            kk, aa, bb = K.copy(), A.copy(), B.copy()
            if k is not None: kk[j] = k
            if a is not None: aa[j] = a
            if b is not None: bb[j] = b
            return call(7, kk, aa, bb)
        assert call(6, K[:6], A[:6], B[:6]) == -1 and call(8, np.append(K, 0), np.append(A, 0), np.append(B, 0)) == -1      # n other than D + P
        assert changed(0, k=6) == -1 and changed(0, k=-1) == -1                       # a kind out of range
        assert changed(0, a=np.nan) == -1 and changed(2, b=np.inf) == -1              # non-finite parameters
        assert call(7, K, None, B) == -1 and call(7, K, A, None) == -1                # missing parameters
        assert changed(0, b=0.0) == -1 and changed(0, a=-1.0) == -1                   # invgamma: scale, shape > 0
        assert changed(2, a=0.0) == -1 and changed(2, b=-2.0) == -1                   # gamma: shape, rate > 0
        assert changed(3, b=0.0) == -1 and changed(4, b=-0.05) == -1                  # lognormal, normal: sd > 0
        assert changed(1, a=0.0) == -1                                                # fixed: value > 0
        assert changed(4, k=host.PRIOR_FIXED, a=1.0) == -1                            # fixed on a theta entry
        for k in (host.PRIOR_LOGNORMAL, host.PRIOR_GAMMA, host.PRIOR_INVGAMMA):       # a density on (0, inf) on a real / an upper-bounded parameter
            assert changed(4, k=k, a=1.0, b=1.0) == -1 and changed(6, k=k, a=1.0, b=1.0) == -1
        # the support of parameter 1 (lower 0.5, lognormal prior) may not become real, upper or lower with a negative bound
        sup = lambda kinds, bounds: lib.magi_set_theta_support(h, 3, arr(kinds, np.int32, ip), arr(bounds, np.float64, dp))
        assert sup([3, 3, 2], [0.0, 0.0, 3.0]) == -1 and sup([3, 2, 2], [0.0, 5.0, 3.0]) == -1 and sup([3, 1, 2], [0.0, -0.1, 3.0]) == -1
        (gks, ga, gb), (gkt, gat, gbt) = eng.prior()
        assert gks.tolist() == ks.tolist() and gkt.tolist() == kt.tolist() and ga.tolist() == as_.tolist() and gbt.tolist() == bt.tolist()
        assert eng.theta_support()[0].tolist() == [3, 1, 2]
        with pytest.raises(ValueError):
            eng.set_prior(c.sig_prior, [("gamma", 1.0, 1.0), None, None])             # (the host refuses the same: theta 0 is real)
        eng.sampler_init(_cfg(eng, c), *_states(c, 1), seed=c.seed, chain_ids=[20])
        eng.sampler_run(c.burnin + c.results)
        _assert_same_run(good, ("", eng.sampler_samples(), eng.sampler_diag()))
    finally:
        eng.close()
    fresh = MagiEngine(0)
    try:
        k = np.zeros(7, dtype=np.int32)
        assert fresh._lib.magi_set_prior(fresh._h, 7, k.ctypes.data_as(ip), None, None) == -5        # before magi_set_problem
        assert fresh._lib.magi_get_prior(fresh._h, 7, k.ctypes.data_as(ip), None, None) == -5
        with pytest.raises(MagiHipError):
            fresh.set_prior(None, None)
    finally:
        fresh.close()


def test_set_problem_resets_the_priors():
    c = PR.case("nuts_n41")
    pr = M.case_problem(c)[1]
    eng = _engine(c)
    try:
        _set(eng, c)
        eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, pr.drift)
        (ks, _, _), (kt, _, _) = eng.prior()
        assert ks.tolist() == [0] * 4 and kt.tolist() == [0] * 3
        X0, s0, t0 = M.case_problem(c)[2]
        got = eng.logpost_grad(X0, s0, t0, 1.0)
        want = orc.logpost_grad(X0, s0, t0, 1.0, pr)
        assert abs(got[0] - want[0]) <= 1e-9 * abs(want[0])
    finally:
        eng.close()


# ---- the Python API ---------------------------------------------------------------------------------------------------------------------------

_KW = dict(n_chains=2, seed=3, stale_cache=False, max_tree_depth=5)
_ARRAYS = ("X_samps", "sigma_sqs_samps", "thetas_samps")
_TH_PRIOR = [("lognormal", 0.0, 0.5), ("normal", -2.0, 0.5), None]
_SIG_PRIOR = [("fixed", 0.0025), ("invgamma", 3.0, 0.005)]


def _oscillator_model(seed=3):
    from tests.test_support_gpu import _oscillator_model as model
    return model(seed)[0]


def test_predict_with_priors_equals_the_engine_level_sequence():
    model = _oscillator_model()
    try:
        res = model.predict(6, 6, summary=True, theta_support=S.OSC_SPEC, theta_prior=_TH_PRIOR, sigma_sq_prior=_SIG_PRIOR, **_KW)
        assert res["theta_prior"] == [("lognormal", 0.0, 0.5), ("normal", -2.0, 0.5), "flat"]
        assert res["sigma_sq_prior"] == [("fixed", 0.0025), ("invgamma", 3.0, 0.005)]
        assert (res["sigma_sqs_samps"][..., 0] == 0.0025).all() and res["summary"]["sigma_sqs"]["mean"][0] == 0.0025
        # the engine-level sequence: the problem, the support, then the priors; the fixed variance's pre starts at 0
        eng = model.engine
        kinds, bounds = host.theta_support(S.OSC_SPEC, 3)
        LB, sig0, _ = model._predict_prepare(None)
        eng.set_theta_support(S.OSC_SPEC)
        eng.set_prior(_SIG_PRIOR, _TH_PRIOR)
        sig0 = np.array([0.0, sig0[1]])
        th0 = host.theta_pre_inits(np.asarray(model.thetas_init, dtype=np.float64), kinds, bounds)
        rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None], 2, axis=0)
        cfg = eng.default_cfg(num_results=6, num_burnin_steps=6, stale_cache=0, anneal=1, max_tree_depth=5, step_size=0.1)
        eng.sampler_init(cfg, rep(model.Xhat_init), rep(sig0), rep(th0), seed=3)
        eng.sampler_run(12)
        Xs, sp, tp = eng.sampler_samples()
        for k, want in enumerate((Xs, sp, tp)):
            np.testing.assert_array_equal(res["sample_results"][k], want)
        np.testing.assert_array_equal(res["sigma_sqs_samps"], host.transform_samples(sp, tp, LB, host.prior_spec(_SIG_PRIOR, 2, "sigma_sq"))[0])
        # posterior_trajectories works unchanged on the results
        traj = model.posterior_trajectories(res, return_draws=False)
        assert np.isfinite(traj["mean"]).all()
        # no argument == every entry flat
        plain = model.predict(6, 6, **_KW)
        flat = model.predict(6, 6, theta_prior=[None] * 3, sigma_sq_prior=["flat"] * 2, **_KW)
        assert "theta_prior" not in plain and flat["theta_prior"] == ["flat"] * 3 and flat["sigma_sq_prior"] == ["flat"] * 2
        for k in _ARRAYS:
            np.testing.assert_array_equal(plain[k], flat[k])
        for k in ("leapfrogs_taken", "energy", "target_log_prob"):
            np.testing.assert_array_equal(plain["kernel_results"][k], flat["kernel_results"][k])
    finally:
        model.engine.close()


def test_predict_many_with_per_model_priors_equals_each_models_own_predict():
    from magi_v2_amd.api import predict_many
    models = [_oscillator_model(seed=s) for s in (3, 4)]
    th = [_TH_PRIOR, [("gamma", 2.0, 2.0), None, ("normal", -0.3, 0.1)]]
    sg = [_SIG_PRIOR, None]
    try:
        many = predict_many(models, 5, 5, theta_support=S.OSC_SPEC, theta_prior=th, sigma_sq_prior=sg, summary=True, **_KW)
        for m, t, s, got in zip(models, th, sg, many):
            own = m.predict(5, 5, theta_support=S.OSC_SPEC, theta_prior=t, sigma_sq_prior=s, summary=True, **_KW)
            assert got["theta_prior"] == own["theta_prior"] and got.get("sigma_sq_prior") == own.get("sigma_sq_prior")
            for k in _ARRAYS:
                np.testing.assert_array_equal(got[k], own[k])
            np.testing.assert_array_equal(got["kernel_results"]["leapfrogs_taken"], own["kernel_results"]["leapfrogs_taken"])
            np.testing.assert_array_equal(got["summary"]["sigma_sqs"]["mean"], own["summary"]["sigma_sqs"]["mean"])
        assert (many[0]["sigma_sqs_samps"][..., 0] == 0.0025).all() and "sigma_sq_prior" not in many[1]
        one = predict_many(models, 5, 5, theta_support=S.OSC_SPEC, theta_prior=_TH_PRIOR, sigma_sq_prior=_SIG_PRIOR, **_KW)
        np.testing.assert_array_equal(one[0]["thetas_samps"], many[0]["thetas_samps"])
        assert one[1]["theta_prior"] == many[0]["theta_prior"]
    finally:
        for m in models:
            m.engine.close()


def test_the_informative_prior_moves_the_posterior_as_on_the_reference():
    """The end-to-end case of tests/test_prior_cpu.py on the device: the same seed and chain, the same leapfrog counts and the posterior
    means of theta within the sampler's bars on theta_pre -- the shift the CPU test shows on the reference is the device's too."""
    g, pr = PR.e2e_problem()
    e = PR.E2E
    means = []
    for spec in (None, PR.e2e_prior()):
        th_ref, out = PR.e2e_run(spec)
        eng = U.engine_for(pr, None)
        try:
            eng.set_prior(None, spec)
            X0, s0, t0 = orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), pr.LB)
            cfg = eng.default_cfg(num_results=e["results"], num_burnin_steps=e["burnin"], stale_cache=0, max_tree_depth=e["max_tree_depth"])
            eng.sampler_init(cfg, X0[None], s0[None], t0[None], seed=e["seed"], chain_ids=[e["chain"]])
            eng.sampler_run(e["results"] + e["burnin"])
            samples, d = eng.sampler_samples(), eng.sampler_diag()
        finally:
            eng.close()
        np.testing.assert_array_equal(d.leapfrogs_taken[0], out[4]["all"]["leapfrogs"])
        mean = np.log(1.0 + np.exp(samples[2][0])).mean(axis=0)
        print("posterior mean of theta, device", mean.tolist(), "reference", th_ref.mean(axis=0).tolist())
        np.testing.assert_allclose(mean, th_ref.mean(axis=0), rtol=U.BRANCH_TOL["th_pre"][0], atol=U.BRANCH_TOL["th_pre"][1])
        means.append(mean[e["entry"]])
    assert abs(means[1] - 3.0) < abs(means[0] - 3.0)
