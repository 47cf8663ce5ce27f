"""The diagonal metric on the device against tests/metric_reference.py: the oracle's own NUTS / HMC transition driven in whitened space.

Tolerances are ``tests.util.BRANCH_TOL`` / ``ENERGY_TOL``, the bars the sampler is held to under the identity metric; integer diagnostics
are compared exactly.  tests/test_metric_cpu.py shows on the reference alone that a device which ignored the metric, applied it to one of
its two updates only, took s^2 for s or skipped the D + P parameter entries would change them in every case of the table, and that no
case sits on a rounding knife-edge."""
import ctypes as C

import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import util as U

pytestmark = pytest.mark.gpu


def _engine(c, family="auto", pr=None):
    _, dense, _, d = M.case_problem(c)
    return U.engine_for(dense if pr is None else pr, c.band, drift=d, options={"stream_family": family})


def _cfg(eng, c, **over):
    kw = dict(num_results=c.results, num_burnin_steps=c.burnin)
    kw.update(c.cfg)
    kw.update(over)
    return eng.default_cfg(**kw)


def _states(c, n):
    init = M.case_problem(c)[2]
    return tuple(np.repeat(np.asarray(v)[None], n, axis=0) for v in init)


def _inv_mass(c, ids):
    pr = M.case_problem(c)[0]
    parts = [M.unpack_inv_mass(M.case_metric(c, ch), pr.N, pr.D, pr.P) for ch in ids]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def _assert_chain(where, i, d, samples, ref, burnin, upto=None):
    """Chain i of the device (diagnostics d over all transitions, samples = (X, sig_pre, th_pre) behind the burn-in) is the reference's."""
    oX, osp, otp, _, extra = ref
    al = extra["all"]
    T = len(al["leapfrogs"]) if upto is None else upto
    for name, field in M.INT_FIELDS:
        np.testing.assert_array_equal(getattr(d, name)[i][:T], np.asarray(al[field][:T]).astype(np.int64), err_msg=f"{where}: {name}")
    tol = U.BRANCH_TOL
    np.testing.assert_allclose(d.beta_temp[i][:T], al["beta_temp"][:T], rtol=1e-15, atol=0, err_msg=where)
    np.testing.assert_allclose(d.step_size[i][:T], al["step_size"][:T], rtol=tol["step_size"][0], atol=tol["step_size"][1], err_msg=f"{where}: step_size")
    lar = al["log_accept_ratio"][:T]
    fin = np.isfinite(lar)
    np.testing.assert_array_equal(np.isfinite(d.log_accept_ratio[i][:T]), fin, err_msg=where)
    np.testing.assert_allclose(d.log_accept_ratio[i][:T][fin], lar[fin], rtol=tol["log_accept_ratio"][0], atol=tol["log_accept_ratio"][1], err_msg=f"{where}: log_accept_ratio")
    np.testing.assert_allclose(d.target_log_prob[i][:T], al["target_log_prob"][:T], rtol=tol["target_log_prob"][0], atol=tol["target_log_prob"][1], err_msg=f"{where}: target")
    np.testing.assert_allclose(d.energy[i][:T], al["energy"][:T], rtol=U.ENERGY_TOL[0], atol=U.ENERGY_TOL[1], err_msg=f"{where}: energy")
    R = T - burnin
    if samples is not None and R > 0:
        Xs, sp, tp = samples
        np.testing.assert_allclose(Xs[i][:R], oX[:R], rtol=0, atol=tol["X"][1] * np.abs(oX[:R]).max(), err_msg=f"{where}: X")
        np.testing.assert_allclose(sp[i][:R], osp[:R], rtol=tol["sig_pre"][0], atol=tol["sig_pre"][1], err_msg=f"{where}: sig_pre")
        np.testing.assert_allclose(tp[i][:R], otp[:R], rtol=tol["th_pre"][0], atol=tol["th_pre"][1], err_msg=f"{where}: th_pre")


def _ids(n):
    return list(range(20, 20 + n))


_KERNEL = {(1, "auto"): "k_stream<1>", (2, "auto"): "k_stream<2>", (3, "mc"): "k_stream_", (9, "mc"): "k_stream_"}


@pytest.mark.parametrize("c,chains,family", [(c, n, f) for c in M.CASES for n, f in c.runs], ids=repr)
def test_fixed_metric_matches_the_whitened_oracle_draw_for_draw(c, chains, family):
    """s log-uniform in [0.3, 3] per entry, parameter entries included, another draw per chain; NUTS (step 2e-3, depth <= 6, 4 + 3
    transitions, stale cache both ways) and fixed-L HMC (L = 8) on SEIR-4 at N = 41 (one operator block, three point workgroups) and N = 161
    under band 20, on k_stream<1>, <2>, k_stream_sep<8>, <16>; a non-separable traced drift on k_stream_mc; chain8 (eight component lanes)."""
    ids = _ids(chains)
    eng = _engine(c, family)
    try:
        name = eng.stream_kernel_name(chains)
        assert name.startswith(_KERNEL[(chains, family)]), name
        if family == "mc":
            assert name.startswith("k_stream_mc" if c.drift == "ptrans" else "k_stream_sep"), name
        eng.sampler_init(_cfg(eng, c), *_states(c, chains), seed=c.seed, chain_ids=ids)
        eng.sampler_set_metric(*_inv_mass(c, ids))
        got = eng.sampler_metric()
        lf, _ = eng.sampler_run(c.burnin + c.results)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    for a, b in zip(got, _inv_mass(c, ids)):
        np.testing.assert_allclose(a, b, rtol=4e-16, atol=0)          # (sqrt, then a square: one rounding each)
    assert lf == d.leapfrogs_taken.sum()
    with M.oracle_drifts(c):
        for i in sorted({0, chains - 1}):
            _assert_chain(f"{c.name} {name} chain {ids[i]}", i, d, samples, M.case_run(c, ids[i])[0], c.burnin)


@pytest.mark.parametrize("chains,family", [(1, "auto"), (3, "auto"), (3, "mc")])
def test_all_ones_metric_is_the_identity_metric_bit_for_bit(chains, family):
    c = M.case("nuts_n41")
    ids = _ids(chains)
    runs = []
    for ones in (False, True):
        eng = _engine(c, family)
        try:
            eng.sampler_init(_cfg(eng, c), *_states(c, chains), seed=c.seed, chain_ids=ids)
            if ones:
                pr = M.case_problem(c)[0]
                eng.sampler_set_metric(np.ones((chains, pr.N, pr.D)), np.ones((chains, pr.D)), np.ones((chains, pr.P)))
            eng.sampler_run(c.burnin + c.results)
            runs.append((eng.sampler_samples(), eng.sampler_diag()))
        finally:
            eng.close()
    (sa, da), (sb, db) = runs
    for a, b in zip(sa, sb):
        np.testing.assert_array_equal(a, b)
    for f in da.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(da, f), getattr(db, f), err_msg=f)
    assert da.leapfrogs_taken.max() >= 31


def test_metric_set_between_runs_governs_the_next_transition_and_null_goes_back():
    """run(3), set_metric, run(4), set_metric(None), run(3): the reference switching at transitions 3 and 7."""
    c = M.case("nuts_n41")
    eng = _engine(c)
    try:
        eng.sampler_init(_cfg(eng, c, num_results=6), *_states(c, 1), seed=c.seed, chain_ids=[20])
        eng.sampler_run(3)
        eng.sampler_set_metric(*_inv_mass(c, [20]))
        eng.sampler_run(4)
        eng.sampler_set_metric()
        for a in eng.sampler_metric():
            np.testing.assert_array_equal(a, 1.0)
        eng.sampler_run(3)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    pr, _, init, _ = M.case_problem(c)
    ref = M.sample_chain(pr, None, None, None, 6, c.burnin, chain=20, initial=init, metric={3: M.case_metric(c, 20), 7: None}, **M.oracle_kwargs(c))
    _assert_chain("switch", 0, d, samples, ref, c.burnin)
    ident = M.sample_chain(pr, None, None, None, 6, c.burnin, chain=20, initial=init, **M.oracle_kwargs(c))
    assert np.abs(ref[0] - ident[0]).max() > 1e-3 * np.abs(ident[0]).max()          # (the switch is not a no-op at these tolerances)


# The adaptation tests cap the trees at depth 2 (3 leapfrogs).  A metric is made of variances over 4 to 12 states and the restart divides by the
# smallest standard deviation, so the comparison amplifies the device-vs-oracle difference of the states by |X| / spread, and trajectories of
# 63 leapfrogs amplify it again.  Measured on the CPU (numpy oracle vs the C port's summation order, chains 20-22, the two scenarios below):
# step sizes differ by <= 1.7e-11 at depth 2, <= 2.8e-10 at depth 3 and up to 5.1e-9 at depth 4, against BRANCH_TOL's 1e-9; at depth 6 the
# device left the reference by 1e-8 .. 1e-5.  What these tests hold -- window sums, formula, step-size rule, restart -- does not depend on the depth.
_SHALLOW = 2
_WIN = dict(num_burnin_steps=0, num_results=18, num_adaptation_steps=18, max_tree_depth=_SHALLOW)


def test_window_sums_and_adaptation_match_the_reference_formula():
    """num_burnin_steps = 0: every state is a sample.  Window over transitions 2 .. 13; the metric after the adaptation against the reference's
    formula on the DOWNLOADED states at 1e-12; step_size_out and the step sizes of the transitions behind it against the reference, restart
    included; a wrong n is rejected and leaves the window open."""
    from magi_v2_amd.engine import MagiHipError
    c = M.case("nuts_n41")
    pr, _, init, _ = M.case_problem(c)
    chains, ids = 2, [20, 21]
    eng = _engine(c)
    try:
        eng.sampler_init(_cfg(eng, c, **_WIN), *_states(c, chains), seed=c.seed, chain_ids=ids)
        eng.sampler_run(2)
        eng.sampler_metric_window(True)
        eng.sampler_run(12)
        eps_old = eng.sampler_state()[3]
        for bad in (11, 13):
            with pytest.raises(MagiHipError) as e:
                eng.sampler_adapt_metric(bad, restart_adapt_steps=3)
            assert e.value.code == -1
        ss, kept = eng.sampler_adapt_metric(12, restart_adapt_steps=3)
        mX, ms, mt = eng.sampler_metric()
        eng.sampler_run(4)
        (Xs, sp, tp), d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert kept == 0
    for i, ch in enumerate(ids):
        q = np.stack([orc.pack(Xs[i][k], sp[i][k], tp[i][k]) for k in range(14)])
        S1, S2 = M.window_sums(q[2:14], q[1])
        s, var, med = M.metric_from_sums(S1, S2, 12)
        got = M.pack_metric(mX[i], ms[i], mt[i])
        print(f"chain {ch}: metric vs the formula on the downloaded states, worst relative difference {np.max(np.abs(got / s - 1.0)):.2e}; var spans {var.min():.2e} .. {var.max():.2e}")
        np.testing.assert_allclose(got * got, s * s, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ss[i], M.restart_step_size(eps_old[i], np.ones_like(s), got), rtol=1e-14, atol=0)
        ref = M.sample_chain(pr, None, None, None, 18, 0, chain=ch, initial=init, num_adaptation_steps=18, windows=[(2, 14)], restart={14: 3},
                             **dict(M.oracle_kwargs(c), max_tree_depth=_SHALLOW))
        al = ref[4]["all"]
        print(f"chain {ch}: step sizes behind the restart, device / reference - 1: {(d.step_size[i][14:] / al['step_size'][14:] - 1.0).tolist()}")
        np.testing.assert_array_equal(d.leapfrogs_taken[i], al["leapfrogs"])
        np.testing.assert_allclose(ss[i], ref[4]["adapted"][0]["step_size"], rtol=U.BRANCH_TOL["step_size"][0])
        np.testing.assert_allclose(d.step_size[i], al["step_size"], rtol=U.BRANCH_TOL["step_size"][0], atol=0)


@pytest.mark.parametrize("family", ["auto", "mc"])
def test_window_metric_equals_the_formula_with_deep_trees(family):
    """Depth 6, three chains whose transitions end many slots apart (k_stream<2> pairs with a ragged last pair / k_stream_sep), the window
    split over two runs so that chains wait idle in the middle of it: the metric equals the formula on the downloaded states at 1e-12
    relative.  No reference trajectory is involved, so nothing amplifies."""
    c = M.case("nuts_n41")
    chains, ids = 3, [20, 21, 22]
    eng = _engine(c, family)
    try:
        eng.sampler_init(_cfg(eng, c, num_burnin_steps=0, num_results=15, num_adaptation_steps=15), *_states(c, chains), seed=c.seed, chain_ids=ids)
        eng.sampler_run(2)
        eng.sampler_metric_window(True)
        eng.sampler_run(5)
        eng.sampler_run(7)
        _, kept = eng.sampler_adapt_metric(12)
        mX, ms, mt = eng.sampler_metric()
        eng.sampler_run(1)
        (Xs, sp, tp), d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    assert kept == 0
    lf = d.leapfrogs_taken[:, 2:14]
    assert lf.max() >= 31 and np.any(lf[0] != lf[1]) and np.any(lf[1] != lf[2])
    for i in range(chains):
        q = np.stack([orc.pack(Xs[i][k], sp[i][k], tp[i][k]) for k in range(14)])
        s, var, med = M.metric_from_sums(*M.window_sums(q[2:14], q[1]), 12)
        got = M.pack_metric(mX[i], ms[i], mt[i])
        np.testing.assert_allclose(got * got, s * s, rtol=1e-12, atol=0, err_msg=f"chain {ids[i]}")


_WARM = dict(num_burnin_steps=40, num_results=5, max_tree_depth=_SHALLOW)
_SCHED = (40, 32, 8, 4, 8)


def _warm_run(eng, c, chains, ids, pause=False, depth=_SHALLOW):
    eng.sampler_init(_cfg(eng, c, **dict(_WARM, max_tree_depth=depth)), *_states(c, chains), seed=c.seed, chain_ids=ids)
    sched = host.warmup_schedule(*_SCHED)
    _, _, windows = eng.sampler_warmup(sched)
    if pause:
        return windows
    eng.sampler_run(45 - _SCHED[1])
    return windows, eng.sampler_samples(), eng.sampler_diag(), eng.sampler_metric()


def _warm_reference(c, chain):
    pr, _, init, _ = M.case_problem(c)
    wins = [(a, b) for a, b, adapt in host.warmup_schedule(*_SCHED) if adapt]
    return M.sample_chain(pr, None, None, None, 5, 40, chain=chain, initial=init, windows=wins, **dict(M.oracle_kwargs(c), max_tree_depth=_SHALLOW))


@pytest.mark.parametrize("chains,family", [(1, "auto"), (3, "mc")])
def test_whole_warmup_matches_the_reference(chains, family):
    """sampler_warmup over warmup_schedule(40, 32, 8, 4, 8) -- windows [8, 12) and [12, 24) become metrics, dual averaging restarts with
    20 and 8 steps left -- then 13 more transitions, 5 of them results.  Every diagnostic of the 45 transitions and the results."""
    c = M.case("nuts_n41")
    assert host.warmup_schedule(*_SCHED) == [(0, 8, False), (8, 12, True), (12, 24, True), (24, 32, False)]
    ids = _ids(chains)
    eng = _engine(c, family)
    try:
        windows, samples, d, metric = _warm_run(eng, c, chains, ids)
    finally:
        eng.close()
    assert [(w["start"], w["stop"], w["unchanged"]) for w in windows] == [(8, 12, 0), (12, 24, 0)]
    for i in sorted({0, chains - 1}):
        ref = _warm_reference(c, ids[i])
        s = M.pack_metric(metric[0][i], metric[1][i], metric[2][i])
        print(f"chain {ids[i]}: final metric, device / reference - 1: {np.max(np.abs(s / ref[4]['s'] - 1.0)):.2e}; leapfrogs {d.leapfrogs_taken[i].tolist()}")
        _assert_chain(f"warm-up chain {ids[i]}", i, d, samples, ref, 40)


@pytest.mark.parametrize("depth", [_SHALLOW, 6])
def test_a_chain_does_not_depend_on_the_batch_it_is_adapted_in(depth):
    """stream_family = mc: chain id 21 alone and as the middle chain of three, warm-up and adapted metric included, bit for bit.  At depth 6
    the chains of the batch end their transitions many slots apart and wait idle for each other at the end of every run: the window sums
    take each chain's state exactly once per transition whatever the others do."""
    c = M.case("nuts_n41")
    out = []
    for ids in ([21], [20, 21, 22]):
        eng = _engine(c, "mc")
        try:
            out.append((ids.index(21),) + _warm_run(eng, c, len(ids), ids, depth=depth)[1:])
        finally:
            eng.close()
    (i, sa, da, ma), (j, sb, db, mb) = out
    for a, b in zip(sa + ma, sb + mb):
        np.testing.assert_array_equal(a[i], b[j])
    for f in da.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(da, f)[i], getattr(db, f)[j], err_msg=f)
    assert not np.all(ma[0][i] == 1.0)
    if depth == 6:
        lf = db.leapfrogs_taken
        assert lf.max() >= 31 and np.any(lf[0] != lf[1]) and np.any(lf[1] != lf[2])          # (the batch does not run in lockstep)


def test_group_members_under_a_fixed_metric_equal_handles_of_their_own(monkeypatch):
    import dataclasses
    from magi_v2_amd.engine import MagiGroup
    monkeypatch.delenv("MAGI_STREAM_FAMILY", raising=False)
    c = M.case("nuts_n41")
    _, dense, _, _ = M.case_problem(c)
    prs = [dense, dataclasses.replace(dense, y=dense.y * 1.02, K_inv=dense.K_inv * 1.05)]
    ids = [20, 21]
    mass = _inv_mass(c, ids)
    solo = []
    engs = [U.engine_for(p, c.band) for p in prs]
    try:
        for e in engs:
            e.sampler_init(_cfg(e, c), *_states(c, 2), seed=c.seed, chain_ids=ids)
            e.sampler_set_metric(*mass)
            e.sampler_run(c.burnin + c.results)
            solo.append((e.sampler_samples(), e.sampler_diag()))
        grp = MagiGroup(engs)
        try:
            grp.sampler_init(_cfg(grp, c), *_states(c, 4), seed=c.seed, chain_ids=ids * 2)
            grp.sampler_set_metric(*(np.concatenate([m, m]) for m in mass))
            for a, m in zip(grp.sampler_metric(), mass):
                np.testing.assert_allclose(a, np.concatenate([m, m]), rtol=4e-16)
            grp.sampler_run(c.burnin + c.results)
            gs, gd = grp.sampler_samples(), grp.sampler_diag()
        finally:
            grp.close()
    finally:
        for e in engs:
            e.close()
    for m, (ss, sd) in enumerate(solo):
        for a, b in zip(gs, ss):
            np.testing.assert_array_equal(a[2 * m: 2 * m + 2], b)
        for f in sd.__dataclass_fields__:
            np.testing.assert_array_equal(getattr(gd, f)[2 * m: 2 * m + 2], getattr(sd, f), err_msg=f)
    assert not np.array_equal(solo[0][0][0], solo[1][0][0])


def test_resume_after_warmup_in_a_fresh_handle_is_bit_for_bit():
    """Pause behind the warm-up; resume as include/magi_hip.h documents: init with num_adaptation_steps = the value in force (the last
    restart's: 32 - 24), then set_metric, then set_checkpoint."""
    c = M.case("nuts_n41")
    ids = [20, 21]
    eng = _engine(c)
    try:
        _warm_run(eng, c, 2, ids, pause=True)
        ck, metric = eng.sampler_checkpoint(), eng.sampler_metric()
        eng.sampler_run(13)
        want = (eng.sampler_samples(), eng.sampler_diag())
    finally:
        eng.close()
    eng = _engine(c)
    try:
        eng.sampler_resume(_cfg(eng, c, num_adaptation_steps=8, **_WARM), ck, seed=c.seed, chain_ids=ids, metric=metric)
        for a, b in zip(eng.sampler_metric(), metric):
            np.testing.assert_array_equal(a, b)
        eng.sampler_run(13)
        got = (eng.sampler_samples(), eng.sampler_diag())
    finally:
        eng.close()
    for a, b in zip(got[0], want[0]):
        np.testing.assert_array_equal(a, b)
    for f in want[1].__dataclass_fields__:
        np.testing.assert_array_equal(getattr(got[1], f)[:, 32:], getattr(want[1], f)[:, 32:], err_msg=f)


def test_bad_arguments_are_rejected_and_leave_the_sampler_as_it_was():
    from magi_v2_amd.engine import MagiHipError
    c = M.case("nuts_n41")
    pr = M.case_problem(c)[0]
    ids = [20]
    mass = _inv_mass(c, ids)
    eng = _engine(c)
    try:
        p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))       # (before init the wrappers have no shapes: the C ABI itself)
        buf = [m.copy() for m in mass]
        lib, h = eng._lib, eng._h
        assert lib.magi_sampler_set_metric(h, p(mass[0]), p(mass[1]), p(mass[2])) == -5
        assert lib.magi_sampler_get_metric(h, p(buf[0]), p(buf[1]), p(buf[2])) == -5
        assert lib.magi_sampler_metric_window(h, 1) == -5
        assert lib.magi_sampler_adapt_metric(h, 4, 5.0, 1e-3, -1, None) == -5
        eng.sampler_init(_cfg(eng, c), *_states(c, 1), seed=c.seed, chain_ids=ids)
        eng.sampler_set_metric(*mass)
        for bad in (0.0, -1.0, np.nan, np.inf):
            for k, e_idx in ((0, (0, 17, 2)), (1, (0, 1)), (2, (0, pr.P - 1))):
                arrs = [m.copy() for m in mass]
                arrs[k][e_idx] = bad
                with pytest.raises(MagiHipError) as e:
                    eng.sampler_set_metric(*arrs)
                assert e.value.code == -1
        with pytest.raises(MagiHipError) as e:
            eng.sampler_adapt_metric(4)                      # no window open
        assert e.value.code == -5
        eng.sampler_metric_window(True)
        eng.sampler_run(1)
        with pytest.raises(MagiHipError) as e:
            eng.sampler_adapt_metric(1)                      # n < 2
        assert e.value.code == -1
        eng.sampler_metric_window(False)
        for a, b in zip(eng.sampler_metric(), mass):
            np.testing.assert_allclose(a, b, rtol=4e-16)
        eng.sampler_run(c.burnin + c.results - 1)
        samples, d = eng.sampler_samples(), eng.sampler_diag()
    finally:
        eng.close()
    _assert_chain("after the rejections", 0, d, samples, M.case_run(c, 20)[0], c.burnin)


def test_predict_with_adapt_metric_is_the_engine_level_warmup():
    """MAGI_v2.predict(adapt_metric=True) on the vignette's thinned SEIR rows: results["metric"] and the draws equal the engine-level run of
    the same schedule bit for bit; without the option the dictionary is the reference's."""
    import os
    import magi_v2
    from tests.test_api_gpu import vignette_f_vec
    g = np.load(os.path.join(U.GOLDEN, "g3_pipeline.npz"))
    model = magi_v2.MAGI_v2(D_thetas=3, ts_obs=g["seir3_ts_obs"], X_obs=g["seir3_X_obs"], bandsize=80, f_vec=vignette_f_vec)
    model.initial_fit(discretization=1, verbose=False, hparam_iters=0)
    kw = dict(num_results=4, num_burnin_steps=40, seed=7, n_chains=2, max_tree_depth=4)
    res = model.predict(adapt_metric=True, **kw)
    sched = host.warmup_schedule(40, 32)
    assert sched == [(0, 4, False), (4, 29, True), (29, 32, False)]
    met = res["metric"]
    assert set(met) == {"inv_mass_X", "inv_mass_sigma_pre", "inv_mass_theta_pre", "windows"}
    assert met["inv_mass_X"].shape == (2, 161, 3) and met["inv_mass_sigma_pre"].shape == (2, 3) and met["inv_mass_theta_pre"].shape == (2, 3)
    assert [(w["start"], w["stop"], w["unchanged"]) for w in met["windows"]] == [(4, 29, 0)]
    assert met["inv_mass_X"].max() / met["inv_mass_X"].min() > 10.0
    eng = model.engine
    LB = orc.sigma_sqs_lower_bound(model.Xhat_init)
    sig0, th0 = host.softplus_inverse_inits(np.asarray(model.sigma_sqs_init, dtype=np.float64), np.asarray(model.thetas_init, dtype=np.float64), LB)
    rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None], 2, axis=0)
    cfg = eng.default_cfg(num_results=4, num_burnin_steps=40, stale_cache=1, anneal=1, max_tree_depth=4, step_size=0.1)
    eng.sampler_init(cfg, rep(model.Xhat_init), rep(sig0), rep(th0), seed=7)
    _, _, windows = eng.sampler_warmup(sched)
    eng.sampler_run(44 - 32)
    for a, b in zip(eng.sampler_metric(), (met["inv_mass_X"], met["inv_mass_sigma_pre"], met["inv_mass_theta_pre"])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(windows[0]["step_size"], met["windows"][0]["step_size"])
    for a, b in zip(eng.sampler_samples(), res["sample_results"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.sampler_diag().leapfrogs_taken[:, 40:], res["kernel_results"]["leapfrogs_taken"])
    plain = model.predict(**kw)
    assert "metric" not in plain and plain["X_samps"].shape == res["X_samps"].shape
    assert not np.array_equal(plain["X_samps"], res["X_samps"])
