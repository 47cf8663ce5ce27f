"""Posterior predictive checks on the GPU (include/magi_hip.h: magi_ppc, magi_sampler_ppc) against the longdouble restatement of their
definitions (tests/ppc_reference.py) at the bars tests/test_ppc_cpu.py derives.  The noise is Philox on both sides, so replicates are
compared draw for draw; p-values and excluded draws are compared exactly (the CPU test shows no fixture decides one on a rounding
edge, and the sampler fixtures assert the same margin on the reference before they compare).  The sampler route is held to magi_ppc on the
downloaded draws bit for bit, with the sigma^2 the kernel formed (sigma_sq_out)."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import ppc_reference as pr
from oracle import magi_oracle as orc
from tests.util import engine_for, load_g4, problem_from_g4

pytestmark = pytest.mark.gpu

ARRAYS = ("y_rep", "mean", "sd", "quantiles", "pit", "T_obs", "T_rep", "n_T_excluded", "pit_ks")
FULL = dict(probs=pr.PROBS, return_draws=True, discrepancies=True)


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b, names=ARRAYS):
    for s in names:
        if s in a or s in b:
            np.testing.assert_array_equal(_bits(a[s]), _bits(b[s]), err_msg=s)
    for s in a["pvalues"]:
        np.testing.assert_array_equal(_bits(a["pvalues"][s]), _bits(b["pvalues"][s]), err_msg=s)
    assert a["n_nonfinite"] == b["n_nonfinite"]


def _got(res):
    """The engine's dictionary under the reference's names."""
    out = {s: res[s] for s in pr.COMPARED if s in res}
    out.update(pval=np.stack([res["pvalues"][s] for s in pr.STATS], axis=1), n_T_excluded=res["n_T_excluded"], n_nonfinite=res["n_nonfinite"])
    return out


def _chunked(e, call):
    e.set_option("summary_chunk_cols", 7)
    try:
        return call()
    finally:
        e.set_option("summary_chunk_cols", 0)


# ---- magi_ppc on crafted shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_,R,K,domain", pr.FIXTURES)
def test_ppc_matches_the_reference_on_every_crafted_shape(eng, C_, R, K, domain):
    f = pr.crafted(C_, R, K, domain)
    ref = pr.crafted_reference(C_, R, K, domain)
    call = lambda: eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **pr.args_of(f), **FULL)
    res = call()
    worst = pr.check_against(_got(res), ref)
    print((C_, R, K, domain), "worst error / bar:", {s: f"{v:.3f}" for s, v in worst.items()}, "p-values", {s: np.round(v, 3).tolist() for s, v in res["pvalues"].items()})
    assert res["n_T_excluded"].tolist() == f["n_excluded"].tolist() and res["n_obs"] == K and res["obs_index"] is None
    _same_bits(res, call())                                        # bit-identical from run to run
    _same_bits(res, _chunked(eng, call))                           # and whatever the chunking: the accumulators of T persist across chunks
    summ = eng.summarize(res["y_rep"], probs=pr.PROBS)             # mean, sd, quantiles: the statistics of magi_summarize, to the bit
    for s in ("mean", "sd", "quantiles"):
        np.testing.assert_array_equal(_bits(res[s]), _bits(summ[s]), err_msg=s)
    assert res["n_nonfinite"] == summ["n_nonfinite"]
    lean = eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **pr.args_of(f), probs=pr.PROBS)      # outputs left out change nothing of the others
    assert "y_rep" not in lean and "T_obs" not in lean
    _same_bits(res, lean, names=("mean", "sd", "quantiles", "pit", "n_T_excluded"))


def test_chain_ids_select_the_noise_and_null_means_0_to_c(eng):
    f = pr.crafted(3, 67, 63)
    kw = {**pr.args_of(f), **FULL}
    assert f["chain_ids"] is None
    base = eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **kw)
    _same_bits(base, eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **{**kw, "chain_ids": [0, 1, 2]}))
    other = eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **{**kw, "chain_ids": list(pr.CHAIN_IDS)})
    assert not np.any(other["T_rep"][:, :, 0] == base["T_rep"][:, :, 0])      # (not y_rep: sqrt replicates clamped at 0 are equal under any noise)
    assert np.mean(other["y_rep"] == base["y_rep"]) < 0.2
    pr.check_against(_got(other), pr.ppc(f["x"], sigma_sq=f["sigma_sq"], **{**pr.args_of(f), "chain_ids": pr.CHAIN_IDS}))
    # a chain keeps its noise wherever it stands in the call: chains 1, 2 of the three alone
    sub = eng.ppc(f["x"][1:], sigma_sq=f["sigma_sq"][1:], **{**kw, "chain_ids": [1, 2]})
    np.testing.assert_array_equal(_bits(sub["y_rep"]), _bits(base["y_rep"][1:]))
    np.testing.assert_array_equal(_bits(sub["T_rep"]), _bits(base["T_rep"][1:]))


def test_contract_of_magi_ppc(eng):
    """Every MAGI_E_BADARG case of the header returns its code with the handle usable afterwards; every output is optional."""
    f = pr.crafted(2, 33, 63)
    Cn, R, K, D = 2, 33, 63, 3
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    P = lambda a, t=dp: None if a is None else a.ctypes.data_as(t)
    x, s2 = np.ascontiguousarray(f["x"]), np.ascontiguousarray(f["sigma_sq"])
    comp, link = np.ascontiguousarray(f["comp"], dtype=np.int32), np.ascontiguousarray(f["link"], dtype=np.int32)
    w, y, ev = np.array(f["weight"]), np.array(f["y"]), np.full(K, 1e-4)
    probs = np.array(pr.PROBS)
    pit = np.empty(K)

    def raw(c=Cn, r=R, k=K, d=D, x=x, comp=comp, s2=s2, link=link, w=w, y=y, ev=ev, n_q=3, probs=probs, pit=None):
        return eng._lib.magi_ppc(eng._h, c, r, k, d, P(x), P(comp, ip), P(s2), P(link, ip), P(w), P(y), P(ev), 5, None, n_q, P(probs),
                                 None, None, None, None, P(pit), None, None, None, None, None)

    def bad(a, i, v):
        b = np.array(a)
        b.reshape(-1)[i] = v
        return b

    assert raw() == 0
    cases = [(dict(c=0), "1 <= C <= 4096 chains"), (dict(r=0), "1 <= R <= 2^20 draws per chain"), (dict(c=4096, r=2048), "C R exceeds 2^22"),
             (dict(k=0), "1 <= K <= 2^24 columns"), (dict(k=(1 << 24) + 1), "1 <= K <= 2^24 columns"), (dict(d=0), "components"), (dict(d=9), "components"),
             (dict(comp=bad(comp, 4, 3)), "comp[4]"), (dict(comp=bad(comp, 0, -1)), "comp[0]"), (dict(link=bad(link, 1, 3)), "link[1]"),
             (dict(w=bad(w, 2, 0.0)), "weight[2]"), (dict(w=bad(w, 2, np.inf)), "weight[2]"), (dict(s2=bad(s2, 7, -1.0)), "sigma_sq[7]"),
             (dict(s2=bad(s2, 7, np.nan)), "sigma_sq[7]"), (dict(ev=bad(ev, 3, -1e-9)), "extra_var[3]"), (dict(ev=bad(ev, 3, np.nan)), "extra_var[3]"),
             (dict(y=bad(y, 0, -1.0)), "y[0]"), (dict(y=bad(y, 1, 0.0)), "y[1]"), (dict(n_q=17), "n_q"), (dict(probs=np.array([0.1, 1.5, 0.2])), "probs[1]"), (dict(probs=None), "probs is NULL"),
             (dict(x=None), "NULL"), (dict(comp=None), "NULL"), (dict(s2=None), "NULL")]
    for kw, text in cases:
        assert raw(**kw) == -1, kw
        assert text in eng._lib.magi_last_error(eng._h).decode(), (kw, eng._lib.magi_last_error(eng._h).decode())
    assert raw(pit=pit) == 0                                       # the handle is usable, and one output alone is served
    full = eng.ppc(f["x"], sigma_sq=f["sigma_sq"], **{**pr.args_of(f), "extra_var": ev, "seed": 5, "chain_ids": None})
    np.testing.assert_array_equal(_bits(pit), _bits(full["pit"]))
    with pytest.raises(ValueError):
        eng.ppc(f["x"][0], f["comp"], f["sigma_sq"])


# ---- magi_sampler_ppc -----------------------------------------------------------------------------------------------------------------------------

RUN = dict(num_results=50, num_burnin_steps=50, max_tree_depth=3)
NOISE_SEED = 77
SIGMA_ULP = 32.0          # sigma^2 = softplus(pre) + LB against longdouble: one rounding of 1 + e^pre is an ABSOLUTE error 2^-53 (1 + e^pre) of sigma^2


def _grid(p, vals, fill):
    g = np.full(p.N * p.D, fill, dtype=np.float64)
    g[np.asarray(p.obs_idx)] = vals
    return g.reshape(p.N, p.D)


def _run(e, X0, s0, t0, Cn, seed, ids=None, **over):
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], Cn, axis=0)
    e.sampler_init(e.default_cfg(**{**RUN, **over}), rep(X0), rep(s0), rep(t0), seed=seed, chain_ids=ids)
    R = {**RUN, **over}
    return R["num_results"] + R["num_burnin_steps"]


def _check_sampler(e, p, links=None, weights=None, fixed=None, chains=None, LB=None, ids=None):
    """sampler_ppc of the finished run: bit for bit magi_ppc fed with the downloaded samples, sigma^2 and obs_index; within the bars of
    the reference.  Returns the result."""
    X, sp, _ = e.sampler_samples()
    sl = slice(None) if chains is None else slice(chains[0], chains[-1] + 1)
    X, sp = X[sl], sp[sl]
    res = e.sampler_ppc(chains=chains, seed=NOISE_SEED, sigma_sq=True, **FULL)
    i, d = res["obs_index"][:, 0], res["obs_index"][:, 1]
    e_flat = d * p.N + i
    assert np.all(np.diff(e_flat) > 0) and res["n_obs"] == len(p.obs_idx)            # ascending in d N + i: the non-NaN entries of yobs
    assert sorted((i * p.D + d).tolist()) == sorted(np.asarray(p.obs_idx).tolist())
    LBv = np.asarray(p.LB if LB is None else LB, dtype=np.float64)
    s2_ref = pr.sigma_sq_of(sp, LBv, fixed, dtype=np.longdouble)
    tol = SIGMA_ULP * 2.0 ** -53 * (1.0 + np.exp(sp) + LBv)
    assert np.all(np.abs(res["sigma_sq"].astype(np.longdouble) - s2_ref).astype(np.float64) <= tol)
    for dd, c in (fixed or {}).items():
        assert np.all(res["sigma_sq"][:, :, dd] == c)
    x = np.ascontiguousarray(X[:, :, i, d])
    y = _grid(p, p.y, np.nan)[i, d]
    w = None if weights is None else _grid(p, weights, 1.0)[i, d]
    cid = np.arange(e.n_chains)[sl] if ids is None else np.asarray(ids)[sl]
    kw = dict(comp=d, link=links, weight=w, y=y, seed=NOISE_SEED, chain_ids=cid)
    _same_bits(res, e.ppc(x, sigma_sq=res["sigma_sq"], **kw, **FULL))
    ref = pr.ppc(x, sigma_sq=res["sigma_sq"], **kw)
    margin = pr.knife_edge(ref) / max(pr.BAR["T_obs"], pr.BAR["T_rep"])
    assert margin >= 1000.0, margin                                 # no p-value is decided on a rounding edge: compared exactly below
    worst = pr.check_against(_got(res), ref)
    print("worst error / bar:", {s: f"{v:.3f}" for s, v in worst.items()}, "; smallest |T_rep - T_obs| in bars:", margin, "; pit_ks", res["pit_ks"].tolist())
    return res


@pytest.fixture(scope="module")
def sirw():
    g = load_g4("sirw_N41")
    p = problem_from_g4(g, None)
    e = engine_for(p, None)
    yield e, p, orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(p.P), p.LB)
    e.close()


@pytest.mark.parametrize("Cn", [1, 2, 3])
def test_sampler_ppc_equals_ppc_of_the_downloaded_draws_on_the_golden_sirw_problem(sirw, Cn):
    from magi_v2_amd.engine import MagiHipError
    e, p, (X0, s0, t0) = sirw
    total = _run(e, X0, s0, t0, Cn, seed=41)
    e.sampler_run(7)
    with pytest.raises(MagiHipError) as ei:                           # inside a paused run: refused, and the run goes on as if never asked
        e.sampler_ppc(seed=NOISE_SEED)
    assert ei.value.code == -5 and "transitions" in str(ei.value)
    e.sampler_run(total)
    res = _check_sampler(e, p)
    assert res["n_nonfinite"] == 0 and res["n_T_excluded"].tolist() == [0] * p.D
    again = lambda: e.sampler_ppc(seed=NOISE_SEED, sigma_sq=True, **FULL)
    _same_bits(res, again())
    _same_bits(res, _chunked(e, again))
    assert not np.any(e.sampler_ppc(seed=NOISE_SEED + 1, return_draws=True)["y_rep"] == res["y_rep"])
    if Cn == 2:                                                       # the paused call left no trace: an uninterrupted run gives the same bits
        e.sampler_run(_run(e, X0, s0, t0, Cn, seed=41))
        _same_bits(res, again())
    if Cn == 3:
        sub = _check_sampler(e, p, chains=range(1, 3))                # a chain keeps its noise however the chains are selected
        np.testing.assert_array_equal(_bits(sub["y_rep"]), _bits(res["y_rep"][1:3]))
        for bad in (range(2, 4), [0, 2]):
            with pytest.raises((MagiHipError, ValueError)):
                e.sampler_ppc(chains=bad)


def test_sampler_ppc_contract(sirw):
    from magi_v2_amd.engine import MagiHipError
    e, p, (X0, s0, t0) = sirw
    fresh = engine_for(p, None)
    try:
        with pytest.raises(MagiHipError) as ei:                       # no sampler yet
            fresh.sampler_ppc()
        assert ei.value.code == -5
    finally:
        fresh.close()
    e.sampler_run(_run(e, X0, s0, t0, 2, seed=9, num_results=12, num_burnin_steps=8))
    full = e.sampler_ppc(seed=3)
    n = C.c_int32(0)
    dp = C.POINTER(C.c_double)
    probs = np.array(pr.PROBS)
    call = lambda c0, ns, nq, pit, cnt: e._lib.magi_sampler_ppc(e._h, c0, ns, 3, nq, probs.ctypes.data_as(dp), None, None, None, None,
                                                                None if pit is None else pit.ctypes.data_as(dp), None, None, None, None, None,
                                                                None, None if cnt is None else C.byref(cnt), None)
    assert call(0, 2, 3, None, n) == 0 and n.value == len(p.obs_idx)      # the call that returns only the count
    pit = np.empty(n.value)
    assert call(0, 2, 3, pit, None) == 0
    np.testing.assert_array_equal(_bits(pit), _bits(full["pit"]))
    for args, text in (((1, 2, 3, pit, None), "must lie inside the sampler's 2"), ((0, 0, 3, pit, None), "must lie inside"), ((0, 2, 17, pit, None), "n_q")):
        assert call(*args) == -1
        assert text in e._lib.magi_last_error(e._h).decode(), args
    _same_bits(full, e.sampler_ppc(seed=3))                           # usable afterwards, unchanged
    s2 = e.sampler_ppc(seed=3, sigma_sq=True)["sigma_sq"]
    np.testing.assert_array_equal(_bits(e.sampler_sigma_sq()), _bits(s2))      # sigma_sq_out asked for alone: the same numbers
    np.testing.assert_array_equal(_bits(e.sampler_sigma_sq(chains=range(1, 2))), _bits(s2[1:2]))


def test_sampler_ppc_under_links_weights_a_fixed_variance_and_masked_observations(sirw):
    """SIRW N = 41 with a component without observations, NaN-masked entries in another, log and sqrt links with weights 1 / 2 / 4, a
    fixed sigma^2, a lower-bounded theta and a non-default LB (the setting of tests/test_elpd_gpu.py)."""
    _, base, _ = sirw
    g = load_g4("sirw_N41")
    rng = np.random.default_rng(3)
    D = base.D
    comp, row = np.asarray(base.obs_idx) % D, np.asarray(base.obs_idx) // D
    keep = (comp != 3) & ~((comp == 1) & (row % 3 == 0))
    y = np.abs(np.asarray(base.y)) + 0.05
    N_ds = np.array([(keep & (comp == d)).sum() for d in range(D)], dtype=np.float64)
    LB = np.array([2e-4, 5e-4, 1e-4, 3e-4])
    p = dataclasses.replace(base, obs_idx=np.asarray(base.obs_idx)[keep], y=y[keep], N_ds=N_ds, LB=LB)
    links, w = [1, 2, 0, 0], rng.choice([1.0, 2.0, 4.0], size=int(keep.sum()))
    e = engine_for(p, None)
    try:
        e.set_theta_support(["positive", ("lower", 0.1), "positive", "real", "positive"])
        e.set_prior([None, ("fixed", 4e-3), None, None], None)
        e.set_obs_model(["log", "sqrt", "identity", "identity"], w)
        X0 = np.clip(np.asarray(g["Xhat_init"], dtype=np.float64), 0.02, None)
        s0 = np.log(np.expm1(np.full(D, 0.05) - LB))
        s0[1] = 0.0
        e.sampler_run(_run(e, X0, s0, np.zeros(p.P), 2, seed=21))
        res = _check_sampler(e, p, links=links, weights=w, fixed={1: 4e-3}, LB=LB)
        assert set(res["obs_index"][:, 1].tolist()) == {0, 1, 2} and res["n_obs"] == int(keep.sum())
        assert np.all(np.isnan(res["pvalues"]["chi2"][3])) and np.all(np.isfinite(res["pvalues"]["chi2"][:3]))
    finally:
        e.close()


def test_sampler_ppc_on_the_banded_n161_problem():
    from tests.test_summary_gpu import _datasets, _member
    _, pb = _datasets()[0]
    e = _member(pb, band=80)
    try:
        assert (e.N, e.D) == (161, 4)
        p = types.SimpleNamespace(N=161, D=4, obs_idx=np.asarray(pb["idx"]), y=np.asarray(pb["y"]), LB=np.asarray(pb["LB"]))
        e.sampler_run(_run(e, pb["Xhat"], pb["sig_pre0"], pb["th_pre0"], 3, seed=6, num_results=24, num_burnin_steps=6, max_tree_depth=6))
        _check_sampler(e, p)
    finally:
        e.close()


def test_group_member_ppc_equals_the_members_own_handle(sirw):
    """Two members with different observation models: each member's check is its own handle's, bit for bit."""
    from magi_v2_amd.engine import MagiGroup, MagiHipError
    _, base, (X0, s0, t0) = sirw
    p = dataclasses.replace(base, y=np.abs(np.asarray(base.y)) + 0.05)
    rng = np.random.default_rng(8)
    w = rng.choice([1.0, 2.0, 4.0], size=len(p.obs_idx))
    engs = [engine_for(p, None), engine_for(p, None)]
    X0 = np.clip(X0, 0.02, None)
    sg = np.log(np.expm1(np.full(p.D, 0.05) - p.LB))
    try:
        engs[0].set_obs_model(["log", "identity", "sqrt", "identity"], w)
        engs[1].set_obs_model(None, w[::-1].copy())
        Cn, seed = 2, 5
        rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], 2 * Cn, axis=0)
        grp = MagiGroup(engs)
        try:
            grp.sampler_init(grp.default_cfg(**RUN), rep(X0), rep(sg), rep(t0), seed=seed, chain_ids=[0, 1, 0, 1])
            grp.sampler_run(100)
            grouped = [grp.sampler_ppc(member=m, seed=NOISE_SEED, sigma_sq=True, **FULL) for m in range(2)]
            with pytest.raises(MagiHipError) as ei:
                grp.sampler_ppc()
            assert ei.value.code == -1 and "more than one member" in str(ei.value)
        finally:
            grp.close()
        for m in range(2):
            engs[m].sampler_init(engs[m].default_cfg(**RUN), rep(X0)[:Cn], rep(sg)[:Cn], rep(t0)[:Cn], seed=seed, chain_ids=[0, 1])
            engs[m].sampler_run(100)
            own = engs[m].sampler_ppc(seed=NOISE_SEED, sigma_sq=True, **FULL)
            _same_bits(grouped[m], own)
            np.testing.assert_array_equal(_bits(grouped[m]["sigma_sq"]), _bits(own["sigma_sq"]))
            np.testing.assert_array_equal(grouped[m]["obs_index"], own["obs_index"])
        assert not np.array_equal(grouped[0]["pit"], grouped[1]["pit"])
    finally:
        for e in engs:
            e.close()


# ---- the Python API ---------------------------------------------------------------------------------------------------------------------------------

PARENT_KEYS = {"phi1s", "phi2s", "Xhat_init", "sigma_sqs_init", "thetas_init", "I", "X_samps", "sigma_sqs_samps", "thetas_samps", "kernel_results",
               "sample_results", "minutes_elapsed"}


def _equal_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if k != "minutes_elapsed":
                _equal_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _equal_tree(u, v, f"{path}[{i}]")
    elif a is None:
        assert b is None, path
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=path)


def test_predict_and_predict_many_with_ppc_and_posterior_predictive_at_new_times():
    from magi_v2_amd.api import MAGI_v2, predict_many
    from magi_v2_amd.drift_examples import lotka_volterra
    from tests.test_obs_gpu import _lv_model
    models = [_lv_model(s) for s in (None, 13)]
    ms = [m for m, _, _ in models]
    kw = dict(n_chains=2, seed=3, stale_cache=False, max_tree_depth=3)
    try:
        with pytest.raises(RuntimeError):
            MAGI_v2(4, ms[0].ts_obs, ms[0].X_obs, None, lotka_volterra).posterior_predictive()
        with pytest.raises(ValueError, match="ppc=True"):
            ms[0].predict(6, 6, keep_samples=False, **kw)
        m, eng = ms[0], ms[0].engine
        plain = m.predict(12, 8, obs_link=["log", "sqrt"], **kw)
        assert set(plain) == PARENT_KEYS | {"obs_link"}               # without ppc: the dictionary it returned before
        res = m.predict(12, 8, obs_link=["log", "sqrt"], ppc=True, **kw)
        assert set(res) == set(plain) | {"ppc"}
        _equal_tree({k: v for k, v in res.items() if k != "ppc"}, plain)      # and the same arrays under the same seed
        own = eng.sampler_ppc(seed=3)
        _same_bits(res["ppc"], own)
        np.testing.assert_array_equal(res["ppc"]["obs_index"], own["obs_index"])
        assert res["ppc"]["n_obs"] == 82 and set(res["ppc"]["pvalues"]) == {"chi2", "mean", "maxabs", "acf1"} and res["ppc"]["pit_ks"].shape == (2,)
        _same_bits(m.posterior_predictive(), own)                     # None: the seed of the last predict
        assert not np.array_equal(m.posterior_predictive(seed=4)["mean"], own["mean"])
        # held-out measurements at times between the grid points: the reference applied to posterior_at's draws and their cond_var
        rng = np.random.default_rng(2)
        I = np.asarray(m.I).reshape(-1)
        t_new = np.concatenate([0.5 * (I[3:9] + I[4:10]), [I[5]]])
        y_new = np.abs(1.0 + 0.3 * rng.standard_normal((t_new.shape[0], 2)))
        y_new[2, 1] = np.nan
        at = m.posterior_predictive(t_new, y_new, seed=11, return_draws=True)
        gp = eng.sampler_gp_predict(m.I, m.phi1s, m.phi2s, t_new, derivative=False, return_draws=True)
        np.testing.assert_array_equal(gp["X_draws"], m.posterior_at(t_new, derivative=False, return_draws=True)["X_draws"])
        T = t_new.shape[0]
        x = np.ascontiguousarray(gp["X_draws"].transpose(0, 1, 3, 2)).reshape(2, 12, 2 * T)
        ref = pr.ppc(x, np.repeat([0, 1], T), eng.sampler_sigma_sq(), link=[1, 2], y=y_new.T.reshape(-1), extra_var=gp["cond_var"].T.reshape(-1), seed=11)
        got = {s: at[s] for s in ("y_rep", "pit", "mean", "sd", "quantiles")}
        got.update(pval=np.stack([at["pvalues"][s] for s in pr.STATS], axis=1), n_T_excluded=at["n_T_excluded"], n_nonfinite=at["n_nonfinite"])
        print("at new times, worst error / bar:", pr.check_against(got, ref, names=tuple(got)[:5]))
        assert at["obs_index"].tolist() == [[mm, d] for d in range(2) for mm in range(T)] and np.isnan(at["pit"][T + 2])
        # keep_samples=False: nothing of the check needs the draws on the host
        lean = m.predict(12, 8, obs_link=["log", "sqrt"], ppc=True, keep_samples=False, **kw)
        assert lean["X_samps"] is None
        _same_bits(lean["ppc"], own)
        _same_bits(m.posterior_predictive(t_new, y_new, seed=11, return_draws=True), at)
        # predict_many serves each member from its chain range
        with pytest.raises(ValueError, match="ppc=True"):
            predict_many(ms, 6, 6, keep_samples=False, **kw)
        many = predict_many(ms, 12, 8, obs_link=[["log", "sqrt"], None], ppc=True, keep_samples=False, **kw)
        for mm, lk, got in zip(ms, (["log", "sqrt"], None), many):
            one = mm.predict(12, 8, obs_link=lk, ppc=True, **kw)["ppc"]
            assert got["X_samps"] is None
            _same_bits(got["ppc"], one)
            np.testing.assert_array_equal(got["ppc"]["obs_index"], one["obs_index"])
        _same_bits(many[0]["ppc"], own)
    finally:
        for mm in ms:
            mm.engine.close()
