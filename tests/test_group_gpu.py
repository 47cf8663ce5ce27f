"""Problem groups on the GPU (include/magi_hip.h: magi_group_create): one sampler over the chains of several alpha-sweep datasets (N = 161,
b = 80) reproduces every member's own handle bit for bit -- samples and every diagnostic -- whatever the chains per member, the order of
the members and the pauses; the rejections leave the members usable; predict_many and SweepRunner sample through groups and equal the
per-model / per-handle paths."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = os.path.join(GOLDEN, "seir_alpha_sweep.npz")
RUN = dict(num_results=6, num_burnin_steps=6, max_tree_depth=6)
DIAG = ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence", "reach_max_depth", "is_accepted",
        "energy", "target_log_prob", "beta_temp")


def _datasets(discretization=1):
    from magi_v2_amd.sweep import alpha_sweep_datasets
    return alpha_sweep_datasets(SWEEP, discretization)


def _member(pb, band=80):
    from magi_v2_amd.engine import MagiEngine
    eng = MagiEngine(0)
    eng.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=band, want_host=False)
    eng.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    return eng


def _states(pbs, C):
    rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
    return [np.concatenate([rep(pb[k]) for pb in pbs]) for k in ("Xhat", "sig_pre0", "th_pre0")]


def _ids(m, C):
    return list(range(C)) if m % 2 == 0 else [1000 + 37 * m + c for c in range(C)]     # (ids repeat across members)


def _run(eng, pbs, C, ids, seed, steps=(12,)):
    X0, s0, t0 = _states(pbs, C)
    eng.sampler_init(eng.default_cfg(**RUN), X0, s0, t0, seed=seed, chain_ids=ids)
    for n in steps:
        eng.sampler_run(n)
    return eng.sampler_samples(), eng.sampler_diag()


def _assert_same(got, ref, sl=slice(None)):
    (gs, gd), (rs, rd) = got, ref
    for a, b in zip(gs, rs):
        np.testing.assert_array_equal(a[sl], b)
    for k in DIAG:
        np.testing.assert_array_equal(getattr(gd, k)[sl], getattr(rd, k), err_msg=k)


@pytest.fixture(scope="module")
def members():
    ds = _datasets()[:4]
    engs = [_member(pb) for _, pb in ds]
    yield engs, [pb for _, pb in ds]
    for e in engs:
        e.close()


@pytest.mark.parametrize("G, C", [(4, 1), (4, 2), (4, 3), (4, 8), (1, 2)])
def test_group_equals_its_members_own_handles_bit_for_bit(members, G, C):
    from magi_v2_amd.engine import MagiGroup
    engs, pbs = members[0][:G], members[1][:G]
    seed = 4242 + C
    g = MagiGroup(engs)
    try:
        assert g.stream_kernel_name(G * C) == ("k_stream_group<2>" if C % 2 == 0 else "k_stream_group<1>")
        got = _run(g, pbs, C, [i for m in range(G) for i in _ids(m, C)], seed)
    finally:
        g.close()
    for m in range(G):
        assert engs[m].stream_kernel_name(C).startswith("k_stream<")
        _assert_same(got, _run(engs[m], [pbs[m]], C, _ids(m, C), seed), slice(m * C, (m + 1) * C))


def test_group_members_in_permuted_order_keep_their_own_chains(members):
    from magi_v2_amd.engine import MagiGroup
    engs, pbs = members
    order, C, seed = [2, 0, 3, 1], 2, 99
    g = MagiGroup([engs[k] for k in order])
    try:
        got = _run(g, [pbs[k] for k in order], C, [i for k in order for i in _ids(k, C)], seed)
    finally:
        g.close()
    for j, k in enumerate(order):
        _assert_same(got, _run(engs[k], [pbs[k]], C, _ids(k, C), seed), slice(j * C, (j + 1) * C))


def test_group_pause_and_resume_equals_one_run(members):
    from magi_v2_amd.engine import MagiGroup
    engs, pbs = members
    g = MagiGroup(engs)
    try:
        ids = [i for m in range(4) for i in _ids(m, 2)]
        whole = _run(g, pbs, 2, ids, 7, steps=(12,))
        split = _run(g, pbs, 2, ids, 7, steps=(6, 6))
        assert list(g.sampler_steps_done()) == [12] * 8
    finally:
        g.close()
    _assert_same(split, whole)


def test_group_rejections_raise_and_leave_the_members_usable(members):
    from magi_v2_amd.engine import MagiEngine, MagiGroup, MagiHipError
    engs, pbs = members
    wide = _member(_datasets(2)[0][1])                     # N = 321
    narrow = _member(pbs[0], band=40)
    try:
        assert wide.N == 321
        with pytest.raises(MagiHipError, match="shape: N = 321"):
            MagiGroup([engs[0], wide])
        with pytest.raises(MagiHipError, match="shape: band = 40"):
            MagiGroup([engs[0], narrow])
        bare = MagiEngine(0)
        try:
            with pytest.raises(MagiHipError, match="no problem set"):
                MagiGroup([engs[0], bare])
        finally:
            bare.close()
        g = MagiGroup(engs[:2])
        try:
            assert engs[0].stream_kernel_name(17).startswith("k_stream_sep")
            with pytest.raises(MagiHipError, match="matrix-core"):              # the per-handle rule sends 17 chains to k_stream_sep
                _run(g, pbs[:2], 17, None, 1)
            X0, s0, t0 = _states(pbs[:2], 2)
            with pytest.raises(MagiHipError, match="not a positive multiple"):
                g.sampler_init(g.default_cfg(**RUN), X0[:3], s0[:3], t0[:3], seed=1)
            with pytest.raises(MagiHipError, match="problem group"):
                g.set_matrices(np.eye(161)[None].repeat(4, 0), np.eye(161)[None].repeat(4, 0), np.eye(161)[None].repeat(4, 0))
            with pytest.raises(MagiHipError, match="problem group"):
                g.logpost_grad(X0[0], s0[0], t0[0])
            with pytest.raises(MagiHipError, match="problem group"):
                g.set_problem(pbs[0]["mu"], pbs[0]["N_ds"], pbs[0]["idx"], pbs[0]["y"], pbs[0]["beta"], pbs[0]["LB"], "seir4")
            got = _run(g, pbs[:2], 2, [0, 1, 0, 1], 5)                           # the group itself still samples
            with pytest.raises(MagiHipError, match="problem group"):
                g.sampler_checkpoint()
            with pytest.raises(MagiHipError, match="problem group"):
                g.sampler_resume(g.default_cfg(**RUN), {"X": X0, "sig_pre": s0, "th_pre": t0, "scalars": np.zeros((4, 16))}, seed=5)
        finally:
            g.close()
        # the members: their own samplers and log posteriors as before
        _assert_same(got, _run(engs[1], [pbs[1]], 2, [0, 1], 5), slice(2, 4))
        assert np.isfinite(engs[0].logpost_grad(X0[0], s0[0], t0[0])[0])
    finally:
        wide.close()
        narrow.close()


def _models():
    from magi_v2_amd.api import MAGI_v2
    z = np.load(SWEEP)
    names = sorted(k for k in z.files if k.startswith("alpha="))
    out = []
    for k, disc in zip(names[:4], (1, 1, 1, 2)):
        rows = z[k]
        m = MAGI_v2(D_thetas=3, ts_obs=rows[:, 0], X_obs=np.clip(rows[:, 1:5], 0.0, None), bandsize=80, f_vec="seir4")
        m.initial_fit(discretization=disc, hparam_iters=0, theta_init_iters=500)
        out.append(m)
    return out


def _assert_results_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "minutes_elapsed":
            continue
        if k == "kernel_results":
            assert a[k].keys() == b[k].keys()
            for kk in a[k]:
                np.testing.assert_array_equal(a[k][kk], b[k][kk], err_msg=kk)
        elif k == "sample_results":
            for x, y in zip(a[k], b[k]):
                np.testing.assert_array_equal(x, y)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_predict_many_equals_sequential_predict():
    from magi_v2_amd import predict_many
    models = _models()
    assert [m.mag_I for m in models] == [161, 161, 161, 321]
    kw = dict(n_chains=2, seed=2024, max_tree_depth=6)
    many = predict_many(models, 6, 6, **kw)
    assert len(many) == 4
    for m, r in zip(models, many):
        _assert_results_equal(r, m.predict(6, 6, **kw))
        assert r["X_samps"].shape == (2, 6, m.mag_I, 4)


def test_sweep_runner_grouped_equals_per_handle_unit_for_unit():
    from magi_v2_amd.sweep import SweepRunner
    ds = _datasets()[:3]
    out = []
    for grouped in (True, False):
        run = SweepRunner(0, ds, 4, 0, 1, bandsize=80, grouped=grouped)
        try:
            assert (run.group is not None) == grouped and len(run.engines) == 3
            run.init(31, **RUN)
            lf = run.run(6) + run.run(6)
            flat, ids = run.samples()
            out.append((flat, ids, lf))
        finally:
            run.close()
    (fa, ia, la), (fb, ib, lb) = out
    assert ia == ib == list(range(12))
    assert la == lb > 0
    np.testing.assert_array_equal(fa, fb)
