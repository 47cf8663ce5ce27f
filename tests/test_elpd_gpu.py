"""Pointwise log-likelihood, WAIC and PSIS-LOO on the GPU (include/magi_hip.h: magi_elpd, magi_sampler_elpd) against the longdouble
transcription of their definitions (tests/elpd_reference.py) at the bars tests/test_elpd_cpu.py derives.  Crafted log-likelihood arrays go
through magi_elpd: both sides read the same bits, so every order decision (who is in the tail, where the cutoff lies) is exact.  On sampler
draws the device's log-likelihood (loglik_out) is held to the longdouble one formed from the downloaded draws at its own bar, and the six
statistics to the reference applied to that same device log-likelihood -- again the same bits on both sides, so no near-tie of two ratios
can be ordered differently by the two; and on every such fixture the independently formed log-likelihood shows that no two distinct ratios at
a cutoff or inside a tail are closer than 1000 x what its bar could move (elpd_reference.tail_margin), so the decisions were never open."""
import dataclasses
import types

import numpy as np
import pytest

import elpd_reference as er
from oracle import magi_oracle as orc
from tests.util import engine_for, load_g4, problem_from_g4

pytestmark = pytest.mark.gpu

POINT = er.OUTPUTS


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


def _same_bits(a, b, outputs=POINT):
    for s in outputs:
        np.testing.assert_array_equal(np.asarray(a["pointwise"][s]).view(np.uint64), np.asarray(b["pointwise"][s]).view(np.uint64), err_msg=s)
    assert a["n_nonfinite"] == b["n_nonfinite"]


def _got(res):
    return dict(res["pointwise"], n_nonfinite=res["n_nonfinite"])


# ---- magi_elpd on crafted log-likelihood arrays ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,R", er.SHAPES)
def test_elpd_matches_the_reference_on_every_crafted_shape(eng, C, R):
    big = C * R > 5000                                             # (the bound of the LDS stage: every column, a full 2048-slot tail)
    y, ref = er.crafted(C, R), er.crafted_reference(C, R)
    res = eng.elpd(y)
    worst = er.check_against(_got(res), ref)
    print(C * R, "worst error / bar:", {s: f"{v:.3f}" for s, v in worst.items()}, "khat", np.round(res["pointwise"]["khat"], 3).tolist())
    assert res["n_nonfinite"] == 2 and res["obs_index"] is None and res["n_obs"] == y.shape[2]
    _same_bits(res, eng.elpd(y))                                   # bit-identical from run to run
    if not big:
        for cols in (1, 3):                                        # and whatever the chunking
            eng.set_option("summary_chunk_cols", cols)
            try:
                _same_bits(res, eng.elpd(y))
            finally:
                eng.set_option("summary_chunk_cols", 0)
        kh = res["pointwise"]["khat"]
        assert res["n_khat_bad"] == int((kh > 0.7).sum())


def test_past_the_bound_of_the_tail_sort_loo_is_refused_and_waic_served(eng):
    from magi_v2_amd.engine import MagiHipError
    S = er.LOO_MAX_S + 1
    y = np.ascontiguousarray(er.crafted(1, S)[:, :, [0, 6]])
    with pytest.raises(MagiHipError, match="C R <= 466033") as ei:
        eng.elpd(y)
    assert ei.value.code == -1
    res = eng.elpd(y, loo=False)
    assert res["pointwise"]["elpd_loo"] is None and res["pointwise"]["khat"] is None and res["elpd_loo"] is None and res["n_khat_bad"] is None
    ref = er.elpd(y)
    print(er.check_against(_got(res), ref, outputs=("lpd", "p_waic", "elpd_waic")))
    assert res["n_nonfinite"] == 1 and np.isnan(res["pointwise"]["lpd"][1])


def test_contract_of_magi_elpd(eng):
    """NULL outputs are skipped; bad arguments give MAGI_E_BADARG with the texts of the header."""
    import ctypes as C
    y = np.ascontiguousarray(er.crafted(2, 50))
    K = y.shape[2]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    kh, lpd = np.empty(K), np.empty(K)
    full = eng.elpd(y)

    def raw(c=2, r=50, k=K, data=y, outs=(None, None, None, None, None, None)):
        return eng._lib.magi_elpd(eng._h, c, r, k, None if data is None else ptr(data), *[None if o is None else ptr(o) for o in outs], None)

    assert raw(outs=(None, None, None, None, None, kh)) == 0
    np.testing.assert_array_equal(kh.view(np.uint64), full["pointwise"]["khat"].view(np.uint64))
    assert raw(outs=(lpd, None, None, None, None, None)) == 0
    np.testing.assert_array_equal(lpd.view(np.uint64), full["pointwise"]["lpd"].view(np.uint64))
    assert raw() == 0
    for kw, text in ((dict(c=0), "1 <= C <= 4096 chains"), (dict(r=0), "1 <= R <= 2^20 draws per chain"), (dict(c=4096, r=2048), "C R exceeds 2^22"),
                     (dict(k=0), "1 <= K <= 2^24 columns"), (dict(data=None), "loglik is NULL")):
        assert raw(**kw) == -1
        assert text in eng._lib.magi_last_error(eng._h).decode(), kw
    with pytest.raises(ValueError):
        eng.elpd(np.zeros((4, 5)))
    one = eng.elpd(np.full((1, 1, 1), -2.0))                     # S = 1: lpd = l, no variance
    assert one["pointwise"]["lpd"][0] == -2.0 and np.isnan(one["pointwise"]["p_waic"][0]) and np.isinf(one["pointwise"]["khat"][0])
    assert one["pointwise"]["elpd_loo"][0] == -2.0


# ---- magi_sampler_elpd ---------------------------------------------------------------------------------------------------------------------------

RUN = dict(num_results=50, num_burnin_steps=50, max_tree_depth=3)
# Philox seeds of the sampler fixtures: for each, the first from the stated start on at which no two distinct ratios at a cutoff or inside a
# tail come closer than 1000 x what the log-likelihood bar could move (_check_sampler asserts it on the reference's own log-likelihood)
SEEDS = {"sirw": {1: 41, 2: 41, 3: 41}, "links": 21, "structureless": 5, "banded": 6}          # (42 and 43, tried first for 2 and 3 chains, leave margins of 520 - 530)


def _grid(pr, vals, fill):
    """[N][D] array with ``vals`` at the problem's observed entries (obs_idx is in the host layout i D + d)."""
    g = np.full(pr.N * pr.D, fill, dtype=np.float64)
    g[np.asarray(pr.obs_idx)] = vals
    return g.reshape(pr.N, pr.D)


def _run(e, pr, X0, s0, t0, C, seed, **over):
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], C, axis=0)
    e.sampler_init(e.default_cfg(**{**RUN, **over}), rep(X0), rep(s0), rep(t0), seed=seed)
    R = {**RUN, **over}
    return R["num_results"] + R["num_burnin_steps"]


def _check_sampler(e, pr, links=None, weights=None, fixed=None, chains=None, LB=None):
    """sampler_elpd of the finished run against the reference; returns the result."""
    X, sp, tp = e.sampler_samples()
    sl = slice(None) if chains is None else slice(chains[0], chains[-1] + 1)
    res = e.sampler_elpd(chains=chains, loglik=True)
    y_grid = _grid(pr, pr.y, np.nan)
    w_grid = None if weights is None else _grid(pr, weights, 1.0)
    ref_ll, idx, cond = er.loglik(X[sl], sp[sl], y_grid, pr.LB if LB is None else LB, links, w_grid, fixed)
    assert res["obs_index"].tolist() == idx.tolist() and res["n_obs"] == len(idx) == len(pr.obs_idx)
    e_flat = res["obs_index"][:, 1] * pr.N + res["obs_index"][:, 0]
    assert np.all(np.diff(e_flat) > 0)                              # ascending in d N + i: the non-NaN entries of yobs
    worst_ll = er.check_loglik(res["loglik"], ref_ll, cond)
    # the order decisions (cutoff, tail) rest on the device's l here: the independently formed l leaves them no room to differ
    K = ref_ll.shape[2]
    margin = er.tail_margin(ref_ll.astype(np.float64).reshape(-1, K), er.loglik_bar(ref_ll, cond).reshape(-1, K))
    print("smallest gap of two distinct ratios at the cutoff or inside a tail / what the log-likelihood bar could move:", margin)
    assert margin >= 1000.0
    ref = er.elpd(res["loglik"])
    worst = er.check_against(_got(res), ref)
    print("log-likelihood error / bar:", worst_ll, "; statistics:", {s: f"{v:.3f}" for s, v in worst.items()}, "; khat > 0.7:", res["n_khat_bad"])
    _same_bits(res, e.elpd(res["loglik"]))                        # the host route on the same log-likelihood: the same bits
    return res


@pytest.fixture(scope="module")
def sirw():
    g = load_g4("sirw_N41")
    pr = problem_from_g4(g, None)
    e = engine_for(pr, None)
    yield e, pr, orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), pr.LB)
    e.close()


@pytest.mark.parametrize("C", [1, 2, 3])
def test_sampler_elpd_matches_the_reference_on_the_golden_sirw_problem(sirw, C):
    """1, 2 and 3 chains: both kernel families leave samples."""
    from magi_v2_amd.engine import MagiHipError
    e, pr, (X0, s0, t0) = sirw
    total = _run(e, pr, X0, s0, t0, C, seed=SEEDS["sirw"][C])
    e.sampler_run(7)
    with pytest.raises(MagiHipError) as ei:                           # the chains have not finished
        e.sampler_elpd()
    assert ei.value.code == -5 and "transitions" in str(ei.value)
    e.sampler_run(total)
    res = _check_sampler(e, pr)
    assert res["n_nonfinite"] == 0 and np.isfinite(res["elpd_loo"]) and np.isfinite(res["se_elpd_waic"])
    _same_bits(res, e.sampler_elpd())                               # bit-identical from run to run
    e.set_option("summary_chunk_cols", 7)
    try:
        _same_bits(res, e.sampler_elpd())
    finally:
        e.set_option("summary_chunk_cols", 0)
    if C == 3:
        sub = _check_sampler(e, pr, chains=range(1, 3))             # 2 of the 3 chains (equal to the host route on their l: inside)
        np.testing.assert_array_equal(sub["loglik"], res["loglik"][1:3])
        for bad in (range(2, 4), [0, 2]):
            with pytest.raises((MagiHipError, ValueError)):
                e.sampler_elpd(chains=bad)


def test_sampler_elpd_contract(sirw):
    import ctypes as C
    e, pr, (X0, s0, t0) = sirw
    e.sampler_run(_run(e, pr, X0, s0, t0, 2, seed=9, num_results=12, num_burnin_steps=8))
    full = e.sampler_elpd()
    n = C.c_int32(0)
    dp = C.POINTER(C.c_double)
    args = [None] * 6 + [None, C.byref(n), None, None]
    assert e._lib.magi_sampler_elpd(e._h, 0, 2, *args) == 0 and n.value == len(pr.obs_idx)
    kh = np.empty(n.value)
    args[5] = kh.ctypes.data_as(dp)
    assert e._lib.magi_sampler_elpd(e._h, 0, 2, *args) == 0
    np.testing.assert_array_equal(kh.view(np.uint64), full["pointwise"]["khat"].view(np.uint64))
    assert e._lib.magi_sampler_elpd(e._h, 1, 2, *args) == -1
    assert "must lie inside the sampler's 2" in e._lib.magi_last_error(e._h).decode()
    assert e._lib.magi_sampler_elpd(e._h, 0, 0, *args) == -1
    waic = e.sampler_elpd(loo=False)
    _same_bits(waic, full, outputs=("lpd", "p_waic", "elpd_waic"))
    assert waic["pointwise"]["khat"] is None


def test_sampler_elpd_under_links_weights_a_fixed_variance_and_masked_observations(sirw):
    """SIRW N = 41 with a component without observations, NaN-masked entries in another, log and sqrt links with weights 1 / 2 / 4, a
    fixed sigma^2, a lower-bounded theta and a non-default LB."""
    _, base, _ = sirw
    g = load_g4("sirw_N41")
    rng = np.random.default_rng(3)
    D, N = base.D, base.N
    comp, row = np.asarray(base.obs_idx) % D, np.asarray(base.obs_idx) // D
    keep = (comp != 3) & ~((comp == 1) & (row % 3 == 0))              # component 3 unobserved; a third of component 1 masked
    y = np.abs(np.asarray(base.y)) + 0.05                             # inside the domains of log and sqrt
    N_ds = np.array([(keep & (comp == d)).sum() for d in range(D)], dtype=np.float64)
    LB = np.array([2e-4, 5e-4, 1e-4, 3e-4])
    pr = dataclasses.replace(base, obs_idx=np.asarray(base.obs_idx)[keep], y=y[keep], N_ds=N_ds, LB=LB)
    links, w = [1, 2, 0, 0], rng.choice([1.0, 2.0, 4.0], size=int(keep.sum()))
    e = engine_for(pr, None)
    try:
        e.set_theta_support(["positive", ("lower", 0.1), "positive", "real", "positive"])
        e.set_prior([None, ("fixed", 4e-3), None, None], None)
        e.set_obs_model(["log", "sqrt", "identity", "identity"], w)
        X0 = np.clip(np.asarray(g["Xhat_init"], dtype=np.float64), 0.02, None)
        s0 = np.log(np.expm1(np.full(D, 0.05) - LB))
        s0[1] = 0.0
        e.sampler_run(_run(e, pr, X0, s0, np.zeros(pr.P), 2, seed=SEEDS["links"]))
        res = _check_sampler(e, pr, links=links, weights=w, fixed={1: 4e-3}, LB=LB)
        assert set(res["obs_index"][:, 1].tolist()) == {0, 1, 2} and res["n_obs"] == int(keep.sum())
    finally:
        e.close()


def test_sampler_elpd_on_a_structureless_n129_and_a_banded_n161_problem():
    from tests.util import structureless_problem
    from tests.test_summary_gpu import _datasets, _member
    pr, X = structureless_problem(129, "seir4", 11, spd=True)
    comp, row = np.asarray(pr.obs_idx) % pr.D, np.asarray(pr.obs_idx) // pr.D
    keep = (comp != 2) & ~((comp == 0) & (row % 8 == 0))             # component 2 without observations, NaN-masked entries in component 0
    pr = dataclasses.replace(pr, obs_idx=np.asarray(pr.obs_idx)[keep], y=np.asarray(pr.y)[keep],
                             N_ds=np.array([(keep & (comp == d)).sum() for d in range(pr.D)], dtype=np.float64))
    e = engine_for(pr, None)
    try:
        s0 = np.full(pr.D, -3.0)
        e.sampler_run(_run(e, pr, X, s0, np.log(np.expm1(np.array([6.0, 0.6, 1.8]))), 2, seed=SEEDS["structureless"], num_results=30, num_burnin_steps=10))
        res = _check_sampler(e, pr)
        assert set(res["obs_index"][:, 1].tolist()) == {0, 1, 3} and res["n_obs"] == int(keep.sum()) < 260
    finally:
        e.close()
    _, pb = _datasets()[0]
    e = _member(pb, band=80)
    try:
        assert (e.N, e.D) == (161, 4)
        pr = types.SimpleNamespace(N=161, D=4, obs_idx=np.asarray(pb["idx"]), y=np.asarray(pb["y"]), LB=np.asarray(pb["LB"]))
        e.sampler_run(_run(e, pr, pb["Xhat"], pb["sig_pre0"], pb["th_pre0"], 3, seed=SEEDS["banded"], num_results=24, num_burnin_steps=6, max_tree_depth=6))
        _check_sampler(e, pr)
    finally:
        e.close()


def test_group_member_elpd_equals_the_members_own_handle(sirw):
    """Two members with different observation models: each member's elpd is its own handle's, bit for bit; a chain range spanning both
    members is refused."""
    from magi_v2_amd.engine import MagiGroup, MagiHipError
    _, base, (X0, s0, t0) = sirw
    pr = dataclasses.replace(base, y=np.abs(np.asarray(base.y)) + 0.05)
    rng = np.random.default_rng(8)
    w = rng.choice([1.0, 2.0, 4.0], size=len(pr.obs_idx))
    engs = [engine_for(pr, None), engine_for(pr, None)]
    X0 = np.clip(X0, 0.02, None)
    sg = np.log(np.expm1(np.full(pr.D, 0.05) - pr.LB))
    try:
        engs[0].set_obs_model(["log", "identity", "sqrt", "identity"], w)
        engs[1].set_obs_model(None, w[::-1].copy())
        C, seed = 2, 5
        rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], 2 * C, axis=0)
        grp = MagiGroup(engs)
        try:
            grp.sampler_init(grp.default_cfg(**RUN), rep(X0), rep(sg), rep(t0), seed=seed, chain_ids=[0, 1, 0, 1])
            grp.sampler_run(100)
            grouped = [grp.sampler_elpd(member=m, loglik=True) for m in range(2)]
            with pytest.raises(MagiHipError) as ei:
                grp.sampler_elpd()
            assert ei.value.code == -1 and "more than one member" in str(ei.value)
            with pytest.raises(MagiHipError):
                grp.sampler_elpd(chains=range(1, 3))
        finally:
            grp.close()
        for m in range(2):
            engs[m].sampler_init(engs[m].default_cfg(**RUN), rep(X0)[:C], rep(sg)[:C], rep(t0)[:C], seed=seed, chain_ids=[0, 1])
            engs[m].sampler_run(100)
            own = engs[m].sampler_elpd(loglik=True)
            _same_bits(grouped[m], own)
            np.testing.assert_array_equal(grouped[m]["loglik"], own["loglik"])
            np.testing.assert_array_equal(grouped[m]["obs_index"], own["obs_index"])
        assert not np.array_equal(grouped[0]["pointwise"]["lpd"], grouped[1]["pointwise"]["lpd"])
    finally:
        for e in engs:
            e.close()


# ---- the Python API ------------------------------------------------------------------------------------------------------------------------------

def test_predict_with_elpd_end_to_end_on_predator_prey_data():
    """obs_reference.E2E (log links + weights, its seed): predict(elpd=True) against the reference applied to the CPU reference chain's
    draws.  The two chains agree draw for draw to tests.util.BRANCH_TOL, not to the bit, so the log-likelihood is held to its bar plus
    what those tolerances become through dl/dx and dl/dsig_pre, and all six statistics to their bars plus what that allowance becomes in
    them (closed-form for lpd, p_waic, elpd_waic; measured on the reference for the PSIS outputs); the six statistics are also held to
    their bars alone on the device's own log-likelihood.  Then the same data under identity links through
    compare_elpd on the scale of the data: recorded, not asserted in sign."""
    from magi_v2_amd import host
    from tests import obs_reference as OR
    from tests import util as U
    from tests.test_obs_gpu import _lv_model, _model_problem
    e = OR.E2E
    model, X_obs, W = _lv_model()
    try:
        kw = dict(n_chains=1, seed=e["seed"], chain_ids=[0], stale_cache=False, max_tree_depth=e["max_tree_depth"])
        res = model.predict(e["results"], e["burnin"], obs_link="log", obs_weight=W, elpd=True, **kw)
        el = res["elpd"]
        assert el["scale"] == "data" and el["n_obs"] == X_obs.size and el["n_nonfinite"] == 0
        link = model.posterior_elpd(scale="link", loglik=True)
        shift = -np.log(X_obs[link["obs_index"][:, 0], link["obs_index"][:, 1]])
        for s in ("lpd", "elpd_waic", "elpd_loo"):
            np.testing.assert_array_equal(el["pointwise"][s], link["pointwise"][s] + shift)
        np.testing.assert_array_equal(el["pointwise"]["khat"], link["pointwise"]["khat"])
        ref = er.elpd(link["loglik"])
        print("statistics, worst error / bar:", er.check_against(dict(link["pointwise"], n_nonfinite=0), ref))
        # the CPU reference chain on the model's own matrices
        links = host.obs_model_spec("log", 2)
        LB, start = host.link_sigma_defaults(links, X_obs, model.Xhat_init, W, host.sigma_sqs_lower_bound(model.Xhat_init),
                                             np.asarray(model.sigma_sqs_init, dtype=np.float64), False)
        sig0, th0 = host.softplus_inverse_inits(start, np.asarray(model.thetas_init, dtype=np.float64), LB)
        _, out = OR.e2e_reference(_model_problem(model, LB), np.asarray(model.Xhat_init, dtype=np.float64), sig0, th0, "log", W.reshape(-1))
        oX, osp = np.asarray(out[0])[None], np.asarray(out[1])[None]
        ref_ll, idx, cond = er.loglik(oX, osp, X_obs, LB, links, W)
        assert idx.tolist() == link["obs_index"].tolist()
        # |dl/dx| = w |g(x) - g(y)| / (x sigma^2) under the log link, |dl/dpre| <= (1 + w (g(x) - g(y))^2 / sigma^2) / 2 (d sigma^2 / d pre <= sigma^2 ... <= 1)
        s2 = (np.log1p(np.exp(osp)) + LB)[:, :, idx[:, 1]]
        xs = oX[:, :, idx[:, 0], idx[:, 1]]
        wv = W[idx[:, 0], idx[:, 1]]
        df = np.abs(np.log(xs) - np.log(X_obs[idx[:, 0], idx[:, 1]]))
        dx = U.BRANCH_TOL["X"][1] * np.abs(oX).max()
        dpre = U.BRANCH_TOL["sig_pre"][0] * np.abs(osp)[:, :, idx[:, 1]] + U.BRANCH_TOL["sig_pre"][1]
        allow = er.loglik_bar(ref_ll, cond) + wv * df / (xs * s2) * dx + 0.5 * (1.0 + wv * df * df / s2) / s2 * dpre
        err = np.abs(link["loglik"] - ref_ll.astype(np.float64))
        print("log-likelihood against the CPU reference chain's, worst error / allowance:", float((err / allow).max()))
        assert np.all(err <= allow)
        # the six statistics against the reference applied to the CPU reference chain's log-likelihood.  a = the largest |dl| of an
        # observation's column that the draw tolerances permit.  lpd: a smooth maximum, |d lpd| <= a.  p_waic = var(l): the centred
        # perturbation is at most 2 a, so |d var| <= 2 (2 a) sd sqrt(S / (S - 1)) + (2 a)^2 S / (S - 1).  elpd_waic: their sum.
        ll_o = ref_ll.astype(np.float64)
        ref_o = er.elpd(ll_o)
        S = ll_o.shape[0] * ll_o.shape[1]
        a = allow.max(axis=(0, 1))
        scale = np.maximum(1.0, np.abs(ll_o).max(axis=(0, 1)))
        sd = np.sqrt(ref_o["p_waic"].astype(np.float64))
        tol = {"lpd": a + er.BAR["lpd"] * scale,
               "p_waic": 4.0 * a * sd * np.sqrt(S / (S - 1.0)) + 4.0 * a * a * S / (S - 1.0) + er.BAR["p_waic"] * scale}
        tol["elpd_waic"] = tol["lpd"] + tol["p_waic"]
        # khat, elpd_loo, p_loo are continuous in l (order statistics are; draws that swap ranks do so at equal l) but have no closed-form
        # Lipschitz bound: their sensitivity is measured on the reference -- the largest move under 8 random sign patterns of the
        # per-entry allowance -- and the tolerance is 10 x that plus the output's bar.  Derived before the device is looked at.
        base, rng, sens = er.elpd(ll_o, dtype=np.float64), np.random.default_rng(0), {s: 0.0 for s in ("elpd_loo", "p_loo", "khat")}
        for _ in range(8):
            moved = er.elpd(ll_o + rng.choice([-1.0, 1.0], size=ll_o.shape) * allow, dtype=np.float64)
            for s in sens:
                sens[s] = np.maximum(sens[s], np.abs(moved[s] - base[s]))
        for s in sens:
            assert np.all(np.isfinite(sens[s]))
            tol[s] = 10.0 * sens[s] + er.BAR[s] * scale
        worst = {}
        for s in POINT:
            err = np.abs(link["pointwise"][s] - ref_o[s].astype(np.float64))
            worst[s] = float((err / tol[s]).max())
            assert np.all(err <= tol[s]), (s, worst[s])
        print("against the CPU reference chain, worst error / tolerance:", worst, "; largest tolerance:", {s: float(np.max(tol[s])) for s in POINT})
        print("elpd_loo: device", el["elpd_loo"], "se", el["se_elpd_loo"], "; reference chain (link scale)", float(ref_o["elpd_loo"].sum()), "device (link scale)", link["elpd_loo"])
        # keep_samples=False with elpd=True
        lean = model.predict(e["results"], e["burnin"], obs_link="log", obs_weight=W, elpd=True, keep_samples=False, **kw)
        assert lean["X_samps"] is None and "summary" not in lean
        for s in POINT:
            np.testing.assert_array_equal(lean["elpd"]["pointwise"][s], el["pointwise"][s])
        # the same data under identity links, compared on the scale of the data
        plain = model.predict(e["results"], e["burnin"], elpd=True, **kw)["elpd"]
        rows = host.compare_elpd({"log links": el, "identity": plain})
        print("compare_elpd (scale = data):", [(r["name"], round(r["elpd"], 3), round(r["elpd_diff"], 3), round(r["se_diff"], 3), r["n_khat_bad"]) for r in rows])
        assert rows[0]["elpd_diff"] == 0.0 and rows[1]["elpd_diff"] <= 0.0 and np.isfinite(rows[1]["se_diff"])
        with pytest.raises(ValueError, match="scale"):
            model.posterior_elpd(scale="natural")
    finally:
        model.engine.close()


def test_predict_many_with_elpd_on_two_n41_models():
    from magi_v2_amd.api import MAGI_v2, predict_many
    from magi_v2_amd.drift_examples import lotka_volterra
    from tests.test_obs_gpu import _lv_model
    models = [_lv_model(s) for s in (None, 13)]
    ms = [m for m, _, _ in models]
    kw = dict(n_chains=2, seed=3, stale_cache=False, max_tree_depth=3)
    try:
        with pytest.raises(RuntimeError):
            MAGI_v2(4, ms[0].ts_obs, ms[0].X_obs, None, lotka_volterra).posterior_elpd()
        with pytest.raises(ValueError, match="elpd=True"):
            predict_many(ms, 6, 6, keep_samples=False, **kw)
        many = predict_many(ms, 12, 8, obs_link=[["log", "sqrt"], None], elpd=True, keep_samples=False, **kw)
        for m, lk, got in zip(ms, (["log", "sqrt"], None), many):
            own = m.predict(12, 8, obs_link=lk, elpd=True, **kw)["elpd"]
            assert got["X_samps"] is None and got["elpd"]["scale"] == "data"
            for s in POINT:
                np.testing.assert_array_equal(got["elpd"]["pointwise"][s], own["pointwise"][s])
            assert got["elpd"]["elpd_loo"] == own["elpd_loo"] and got["elpd"]["n_obs"] == 82
    finally:
        for m in ms:
            m.engine.close()
