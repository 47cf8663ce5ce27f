"""Rank-normalised R-hat, bulk and tail ESS on the GPU (include/magi_hip.h: magi_rank_diagnostics, magi_sampler_rank_diagnostics) against
the longdouble transcription of their definitions (tests/rank_reference.py) at the bars tests/test_rank_cpu.py derives: ranks bit-exact,
z and z_folded within Z_BAR U max(1, |z|), the three diagnostics within rtol_spread(kappa) of their series plus the effect of a z error
of that size.  The shapes put C R on both sides of the LDS sort (RANK_LDS keys) and beyond twice that at no power of two, with odd R,
R = 4 and a partial 64-column tile (K = 16).  The statistics are held to summary.hip's own kernels bit for bit through the z the call
returns, and the sampler route to the host route on the downloaded samples."""
import os
import warnings

import numpy as np
import pytest

import rank_reference as rr
import summary_reference as sr
from oracle import magi_oracle as orc
from tests.util import engine_for, load_g4, problem_from_g4

pytestmark = pytest.mark.gpu

DIAG = ("rhat_rank", "ess_bulk", "ess_tail")
SERIES = ("rank", "z", "z_folded")
BLOCKS = ("X", "sigma_sqs", "thetas")
RUN = dict(num_results=24, num_burnin_steps=6, max_tree_depth=3)
RUN161 = dict(num_results=24, num_burnin_steps=6, max_tree_depth=6)


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b, names=DIAG):
    for s in names:
        np.testing.assert_array_equal(_bits(a[s]), _bits(b[s]), err_msg=s)


_DEVICE = {}


def _device(eng, C, R):
    """The device's result on fixture(C, R) with the series, computed once per shape."""
    if (C, R) not in _DEVICE:
        _DEVICE[C, R] = eng.rank_diagnostics(rr.fixture(C, R), max_lag=rr.lag_for(C, R), return_z=True)
    return _DEVICE[C, R]


# ---- magi_rank_diagnostics on the fixture -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C, R", rr.SHAPES)
def test_matches_the_reference_on_every_fixture_shape(eng, C, R):
    got = _device(eng, C, R)
    assert got["rhat_rank"].shape == (rr.K_FIXTURE,) and got["z"].shape == (C, R, rr.K_FIXTURE)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # (W = 0 in a series of a handful of draws: rhat = inf on both sides)
        worst = rr.check_against(got, rr.fixture_reference(C, R), rr.fixture_bars(C, R))
    print(C, R, "worst error / bar:", worst, "; z bar in U:", rr.Z_BAR)
    assert got["n_nonfinite"] == 1
    if R < 4:
        assert all(np.all(np.isnan(got[s])) for s in DIAG)


@pytest.mark.parametrize("C, R", rr.SHAPES)
def test_the_statistics_are_the_summary_kernels_on_the_returned_scores(eng, C, R):
    got = _device(eng, C, R)
    lag = rr.lag_for(C, R)
    sz, sf = eng.summarize(got["z"], (), max_lag=lag), eng.summarize(got["z_folded"], (), max_lag=lag)
    # (a series without a split R-hat has no ESS here; summarize reports tau at its floor for split chains that are all one constant)
    np.testing.assert_array_equal(_bits(got["ess_bulk"]), _bits(np.where(np.isnan(sz["rhat"]), np.nan, sz["ess"])))
    legs = np.where(np.isnan(sz["rhat"]) | np.isnan(sf["rhat"]), np.nan, np.maximum(sz["rhat"], sf["rhat"]))
    np.testing.assert_array_equal(_bits(got["rhat_rank"]), _bits(legs))
    ok = [k for k in range(rr.K_FIXTURE) if k not in (sr.COL_NAN, sr.COL_CONST)]
    if R >= 4 and C * R >= 100:
        assert np.all(np.isfinite(got["ess_bulk"][ok])) and np.all(np.isfinite(got["rhat_rank"][ok]))


def test_ranks_do_not_change_under_an_increasing_map(eng):
    C, R = 4, 1000
    y = rr.fixture(C, R)
    keep = [k for k in (0, 1, 2, 4, 5, 6, rr.COL_SCALE, rr.COL_CAUCHY)
            if all(np.unique(f(y[:, :, k])).shape[0] == np.unique(y[:, :, k]).shape[0] and np.all(np.isfinite(f(y[:, :, k])))
                   for f in (lambda v: 2.0 * v + 1.0, lambda v: v ** 3))]
    assert len(keep) >= 4                                             # (the maps create no ties and no overflow there)
    base = eng.rank_diagnostics(y[:, :, keep], return_z=True)
    for f in (lambda v: 2.0 * v + 1.0, lambda v: v ** 3):
        got = eng.rank_diagnostics(f(y[:, :, keep]), return_z=True)
        _same_bits(base, got, ("rank", "z", "ess_bulk"))
        np.testing.assert_array_equal(_bits(eng.summarize(got["z"], ())["rhat"]), _bits(eng.summarize(base["z"], ())["rhat"]))      # the bulk leg


def test_negation_mirrors_the_ranks_and_keeps_the_folded_scores(eng):
    C, R = 3, 257                                                     # S odd: the median is an order statistic, -med that of -y exactly
    y = rr.fixture(C, R)
    ok = [k for k in range(rr.K_FIXTURE) if k != sr.COL_NAN]
    a, b = _device(eng, C, R), eng.rank_diagnostics(-y, return_z=True)
    np.testing.assert_array_equal(b["rank"][:, :, ok], C * R + 1 - a["rank"][:, :, ok])
    np.testing.assert_array_equal(_bits(b["z_folded"][:, :, ok]), _bits(a["z_folded"][:, :, ok]))
    np.testing.assert_array_equal(_bits(eng.summarize(b["z_folded"], ())["rhat"][ok]), _bits(eng.summarize(a["z_folded"], ())["rhat"][ok]))
    assert np.all(np.isnan(b["rank"][:, :, sr.COL_NAN]))


def test_ties_share_a_rank_and_a_tied_top_has_no_tail_ess(eng):
    for C, R in ((2, 65), (1, rr.RANK_LDS + 1)):
        got, y = _device(eng, C, R), rr.fixture(C, R)
        pm0 = y[:, :, rr.COL_PM0]
        zero = pm0 == 0.0
        assert np.any(np.signbit(pm0[zero])) and not np.all(np.signbit(pm0[zero]))
        below = np.count_nonzero(pm0 < 0.0)
        assert np.all(got["rank"][:, :, rr.COL_PM0][zero] == below + (np.count_nonzero(zero) + 1) / 2)
        assert np.isnan(got["ess_tail"][rr.COL_TOP]) and np.isfinite(got["ess_bulk"][rr.COL_TOP]) and np.isfinite(got["rhat_rank"][rr.COL_TOP])
        top = y[:, :, rr.COL_TOP]
        assert len(set(got["rank"][:, :, rr.COL_TOP][top == top.max()].tolist())) == 1


def test_chunks_and_partial_tiles_do_not_change_a_bit(eng):
    base = rr.fixture(3, 257)
    reps = -(-200 // rr.K_FIXTURE)
    y = np.concatenate([base * (1.0 + 0.25 * j) for j in range(reps)], axis=2)[:, :, :200]
    y = np.ascontiguousarray(y).reshape(3, 257, 8, 25)                # (a trailing shape, K = 200)
    whole = eng.rank_diagnostics(y, return_z=True)
    assert whole["rhat_rank"].shape == (8, 25) and whole["z_folded"].shape == y.shape
    eng.set_option("summary_chunk_cols", 48)                         # 200 = 4 x 48 + 8: five chunks, none a multiple of the 64-column tile
    try:
        chunked = eng.rank_diagnostics(y, return_z=True)
    finally:
        eng.set_option("summary_chunk_cols", 0)
    _same_bits(whole, chunked, DIAG + SERIES)
    assert whole["n_nonfinite"] == chunked["n_nonfinite"] == sum(1 for k in range(200) if k % rr.K_FIXTURE == sr.COL_NAN)
    first = _device(eng, 3, 257)                                      # a column does not depend on its neighbours (x 1.0: the fixture itself)
    flat = {s: whole[s].reshape(-1)[:rr.K_FIXTURE] for s in DIAG}
    _same_bits(flat, first)


def test_two_runs_give_the_same_bits_and_outputs_are_optional(eng):
    from magi_v2_amd.engine import _dp
    C, R = 1, rr.RANK_LDS + 1
    a = _device(eng, C, R)
    b = eng.rank_diagnostics(rr.fixture(C, R), max_lag=rr.lag_for(C, R), return_z=True)
    _same_bits(a, b, DIAG + SERIES)
    lean = eng.rank_diagnostics(rr.fixture(C, R), max_lag=rr.lag_for(C, R))
    assert set(lean) == set(DIAG) | {"n_nonfinite"}
    _same_bits(a, lean)
    y = np.ascontiguousarray(rr.fixture(2, 65))
    tail = np.empty(rr.K_FIXTURE)
    rc = eng._lib.magi_rank_diagnostics(eng._h, 2, 65, rr.K_FIXTURE, y.ctypes.data_as(_dp), 0, 0.05, None, None, tail.ctypes.data_as(_dp), None, None, None, None)
    assert rc == 0
    np.testing.assert_array_equal(_bits(tail), _bits(_device(eng, 2, 65)["ess_tail"]))
    other = eng.rank_diagnostics(rr.fixture(2, 65), tail_prob=0.25)
    assert not np.array_equal(_bits(other["ess_tail"]), _bits(tail))
    _same_bits(other, _device(eng, 2, 65), ("rhat_rank", "ess_bulk"))


def test_the_largest_column_sorts_exactly(eng):
    """C R = 2^22, the limit: every stride of the large sort, global and LDS.  Ranks against numpy's sort; the scores against scipy's ndtri
    at its own error plus the device's bar."""
    from scipy.special import ndtri
    S = 1 << 22
    rng = np.random.default_rng(22)
    y = np.rint(rng.standard_normal(S) * 2.0 ** 18) * 2.0 ** -18     # (rounded: a few thousand ties)
    y[::1000] = np.where(np.arange(0, S, 1000) % 2000 == 0, -0.0, 0.0)
    got = eng.rank_diagnostics(y.reshape(4, S // 4, 1), max_lag=8, return_z=True)
    rank = rr.rankdata(y)
    assert np.unique(rank).shape[0] < S - 1000
    np.testing.assert_array_equal(got["rank"].reshape(-1), rank)
    z = ndtri(rr.fractions(rank, S))
    err = np.abs(got["z"].reshape(-1) - z) / (rr.U * np.maximum(1.0, np.abs(z)))
    print("2^22 draws: z against ndtri, worst in U max(1, |z|):", float(err.max()))
    assert err.max() <= rr.Z_BAR + rr.Z_ERR_NDTRI
    assert 0.9 < got["ess_bulk"][0] / S < 1.1 and abs(got["rhat_rank"][0] - 1) < 1e-3 and got["n_nonfinite"] == 0


def test_non_finite_columns_are_nan_and_counted(eng):
    y = np.array(rr.fixture(2, 65)[:, :, :4])
    y[1, 64, 1] = np.inf
    y[0, 0, 3] = -np.inf
    y[0, 1, 3] = np.nan
    got = eng.rank_diagnostics(y, return_z=True)
    assert got["n_nonfinite"] == 2
    for s in DIAG + SERIES:
        assert np.all(np.isnan(got[s][..., [1, 3]])), s
        assert not np.any(np.isnan(got[s][..., [0, 2]])), s
    clean = _device(eng, 2, 65)
    for s in DIAG + SERIES:
        np.testing.assert_array_equal(_bits(got[s][..., [0, 2]]), _bits(clean[s][..., [0, 2]]), err_msg=s)


def test_rejected_arguments_leave_the_handle_usable(eng):
    from magi_v2_amd.engine import MagiHipError, _dp
    y = np.ascontiguousarray(rr.fixture(2, 65)[:, :, :2])
    out = np.empty(2)
    ptr = lambda a: a.ctypes.data_as(_dp)

    def raw(C=2, R=65, K=2, draws=y, tail_prob=0.05):
        return eng._lib.magi_rank_diagnostics(eng._h, C, R, K, None if draws is None else ptr(draws), 0, tail_prob, None, ptr(out), None, None, None, None, None)

    assert raw() == 0
    good = out.copy()
    # (the sizes are checked before a draw is read: the oversized shapes never touch memory)
    for kw in (dict(tail_prob=0.0), dict(tail_prob=0.6), dict(tail_prob=np.nan), dict(tail_prob=-0.1), dict(tail_prob=np.inf), dict(C=8, R=1 << 20),
               dict(C=0), dict(C=4097), dict(R=(1 << 20) + 1), dict(K=0), dict(K=(1 << 24) + 1), dict(draws=None)):
        assert raw(**kw) == -1, kw
        assert raw() == 0 and np.array_equal(_bits(out), _bits(good)), kw
    assert raw(tail_prob=0.5) == 0
    for bad in (0.0, 0.6, float("nan")):
        with pytest.raises(MagiHipError) as ei:
            eng.rank_diagnostics(y, tail_prob=bad)
        assert ei.value.code == -1 and "tail_prob" in str(ei.value)
    with pytest.raises(ValueError):
        eng.rank_diagnostics(np.zeros(5))
    _same_bits(eng.rank_diagnostics(y), {s: _device(eng, 2, 65)[s][:2] for s in DIAG})


# ---- the sampler's device-resident samples ------------------------------------------------------------------------------------------

def _init(e, X0, s0, t0, Cn, seed, ids=None, **over):
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], Cn, axis=0)
    cfg = {**RUN, **over}
    e.sampler_init(e.default_cfg(**cfg), rep(X0), rep(s0), rep(t0), seed=seed, chain_ids=ids)
    return cfg["num_results"] + cfg["num_burnin_steps"]


def _folded_leg_candidates(e, draws, host):
    """For an even S the two middle draws of a column lie equally far from the median, and whether their folded values tie is decided in
    the last place of the median (include/magi_hip.h): their folded ranks are (1.5, 1.5), (1, 2) or (2, 1), every other folded rank is
    the same.  Per column the folded legs the definition admits for draws that differ from ``draws`` in their last places only: the
    host route's own, and -- where the middle pair is two untied values -- summarize's rhat of its z_folded with the pair's two scores
    set to each of the three patterns; the scores of the ranks 1, 2 and 1.5 are the device's own, from a probe column.  [n][K] float64."""
    C, R = draws.shape[:2]
    S = C * R
    flat, zf = draws.reshape(S, -1), host["z_folded"].reshape(S, -1)
    probe = np.stack([np.arange(S, dtype=np.float64), np.maximum(np.arange(S, dtype=np.float64), 1.0)], axis=-1)
    pz = e.rank_diagnostics(probe.reshape(C, R, 2), return_z=True)["z"].reshape(S, 2)
    z1, z2, z15 = pz[0, 0], pz[1, 0], pz[0, 1]
    assert z1 < z15 < z2 and pz[1, 1] == z15
    cands = [zf, zf.copy(), zf.copy(), zf.copy()]
    for k in range(flat.shape[1]):
        order = np.argsort(flat[:, k], kind="stable")
        v = flat[order, k]
        m = S // 2
        if S >= 4 and v[m - 2] < v[m - 1] < v[m] < v[m + 1]:
            for c, (a, b) in zip(cands[1:], ((z15, z15), (z1, z2), (z2, z1))):
                c[order[m - 1], k], c[order[m], k] = a, b
    return np.stack([e.summarize(c.reshape(draws.shape), ())["rhat"].reshape(-1) for c in cands])


def _check_sampler(e, res, X, sig, th):
    """sampler_rank_diagnostics ``res`` against rank_diagnostics of the downloaded samples on the natural scale.  X: the stored bits on both
    routes, bit for bit.  sigma^2 / theta: the host's softplus differs from the device's in the last places, which moves no rank of y and no
    comparison against an order statistic -- the scores of y, so ess_bulk, and the indicators, so ess_tail, are the same bits.  The folded
    leg sees the natural scale itself (the bounds, the supports, a fixed variance): bit for bit when C R is odd; when it is even, bit for
    bit one of the outcomes that _folded_leg_candidates derives from the one decision that is open to those last places."""
    host_X = e.rank_diagnostics(X, return_z=True)
    _same_bits(res["X"], host_X)
    assert res["X"]["rhat_rank"].shape == X.shape[2:]
    S = X.shape[0] * X.shape[1]
    for name, draws in (("sigma_sqs", sig), ("thetas", th)):
        draws = np.ascontiguousarray(draws)
        host = e.rank_diagnostics(draws, return_z=True)
        assert res[name]["ess_bulk"].shape == draws.shape[2:]
        _same_bits(res[name], host, ("ess_bulk", "ess_tail"))
        if S % 2:
            _same_bits(res[name], host, ("rhat_rank",))
            continue
        bulk = e.summarize(host["z"], ())["rhat"].reshape(-1)
        folded = _folded_leg_candidates(e, draws, host)
        admitted = np.where(np.isnan(bulk) | np.isnan(folded), np.nan, np.maximum(bulk, folded))
        np.testing.assert_array_equal(_bits(admitted[0]), _bits(host["rhat_rank"].reshape(-1)))
        g = res[name]["rhat_rank"].reshape(-1)
        hit = (_bits(admitted) == _bits(g)[None, :]).any(axis=0)
        assert np.all(hit), (name, g, admitted)
    assert res["n_nonfinite"] == 0


@pytest.fixture(scope="module")
def sirw():
    g = load_g4("sirw_N41")
    p = problem_from_g4(g, None)
    e = engine_for(p, None)
    yield e, p, orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(p.P), p.LB)
    e.close()


@pytest.mark.parametrize("Cn", [1, 2, 3, 9])
def test_sampler_route_equals_the_host_route_on_the_golden_sirw_problem(sirw, Cn, stream_family):
    _, p, state = sirw
    e = engine_for(p, None)                                           # (created under the family's environment)
    try:
        _sampler_route_case(e, p, state, Cn)
    finally:
        e.close()


def _sampler_route_case(e, p, state, Cn):
    from magi_v2_amd import host
    from magi_v2_amd.engine import MagiHipError
    X0, s0, t0 = state
    total = _init(e, X0, s0, t0, Cn, seed=60 + Cn)
    e.sampler_run(7)
    with pytest.raises(MagiHipError) as ei:                           # the chains have not finished
        e.sampler_rank_diagnostics()
    assert ei.value.code == -5 and "transitions" in str(ei.value)
    e.sampler_run(total)
    X, sp, tp = e.sampler_samples()
    sig, th = host.transform_samples(sp, tp, p.LB)
    res = e.sampler_rank_diagnostics()
    _check_sampler(e, res, X, sig, th)
    for b in BLOCKS:
        _same_bits(res[b], e.sampler_rank_diagnostics()[b])
    if Cn == 3:
        sub = e.sampler_rank_diagnostics(chains=range(1, 3))
        _check_sampler(e, sub, X[1:3], sig[1:3], th[1:3])
        assert not np.array_equal(_bits(sub["X"]["ess_bulk"]), _bits(res["X"]["ess_bulk"]))
        for bad in (range(2, 4), [0, 2]):
            with pytest.raises((MagiHipError, ValueError)):
                e.sampler_rank_diagnostics(chains=bad)
        with pytest.raises(MagiHipError) as ei:
            e.sampler_rank_diagnostics(tail_prob=0.6)
        assert ei.value.code == -1
        _same_bits(res["X"], e.sampler_rank_diagnostics()["X"])       # usable afterwards, unchanged


def test_an_odd_number_of_draws_is_bit_for_bit_on_every_block(sirw):
    from magi_v2_amd import host
    e, p, (X0, s0, t0) = sirw
    e.sampler_run(_init(e, X0, s0, t0, 3, seed=5, num_results=25))
    X, sp, tp = e.sampler_samples()
    assert X.shape[0] * X.shape[1] == 75
    _check_sampler(e, e.sampler_rank_diagnostics(), X, *host.transform_samples(sp, tp, p.LB))


def test_a_call_inside_a_paused_run_leaves_no_trace(sirw, eng):
    from magi_v2_amd.engine import MagiHipError
    e, p, (X0, s0, t0) = sirw
    total = _init(e, X0, s0, t0, 2, seed=41)
    e.sampler_run(total)
    plain = (e.sampler_samples(), e.sampler_summary(), e.sampler_rank_diagnostics())
    _init(e, X0, s0, t0, 2, seed=41)
    e.sampler_run(11)
    y = rr.fixture(2, 65)
    inside = e.rank_diagnostics(y, return_z=True)                     # on the sampling handle itself, between two sampler_run calls
    _same_bits(inside, _device(eng, 2, 65), DIAG + SERIES)
    with pytest.raises(MagiHipError) as ei:                           # the sampler route is refused there, and touches nothing either
        e.sampler_rank_diagnostics()
    assert ei.value.code == -5
    e.sampler_run(total)
    for a, b in zip(plain[0], e.sampler_samples()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    again = e.sampler_summary()
    for b in BLOCKS:
        for s in ("mean", "sd", "quantiles", "rhat", "ess", "mcse_mean"):
            np.testing.assert_array_equal(_bits(plain[1][b][s]), _bits(again[b][s]), err_msg=s)
        _same_bits(plain[2][b], e.sampler_rank_diagnostics()[b])


def test_sampler_route_under_a_mixed_theta_support_and_a_fixed_variance(sirw):
    from magi_v2_amd import host
    _, p, (X0, s0, t0) = sirw
    spec = ["positive", ("lower", 0.1), "positive", "real", "positive"]
    e = engine_for(p, None)
    try:
        e.set_theta_support(spec)
        e.set_prior([None, ("fixed", 4e-3), None, None], None)
        s0 = np.array(s0, dtype=np.float64)
        s0[1] = 0.0
        kinds, bounds = host.theta_support(spec, p.P)
        for Cn, over in ((3, dict(num_results=25)), (2, {})):         # C R odd: every block bit for bit; even: the folded leg as derived
            e.sampler_run(_init(e, X0, s0, np.zeros(p.P), Cn, seed=21, **over))
            X, sp, tp = e.sampler_samples()
            sig = host.transform_samples(sp, tp, p.LB)[0]
            sig[:, :, 1] = 4e-3
            res = e.sampler_rank_diagnostics()
            _check_sampler(e, res, X, sig, host.transform_thetas(tp, kinds, bounds))
        assert all(np.isnan(res["sigma_sqs"][s][1]) for s in DIAG)    # the known variance: a constant column
        assert all(np.all(np.isfinite(np.delete(res["sigma_sqs"][s], 1))) for s in ("rhat_rank", "ess_bulk"))
        assert np.all(np.isfinite(res["thetas"]["ess_bulk"]))
    finally:
        e.close()


@pytest.fixture(scope="module")
def members():
    from magi_v2_amd.engine import MagiEngine
    from magi_v2_amd.sweep import alpha_sweep_datasets
    ds = alpha_sweep_datasets(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seir_alpha_sweep.npz"), 1)[:2]
    engs = []
    for _, pb in ds:
        e = MagiEngine(0)
        e.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=80, want_host=False)
        e.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
        engs.append(e)
    yield engs, [pb for _, pb in ds]
    for e in engs:
        e.close()


def _init161(e, pbs, C, seed, ids=None, **over):
    rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
    X0, s0, t0 = [np.concatenate([rep(pb[k]) for pb in pbs]) for k in ("Xhat", "sig_pre0", "th_pre0")]
    e.sampler_init(e.default_cfg(**{**RUN161, **over}), X0, s0, t0, seed=seed, chain_ids=ids)


def test_sampler_route_on_the_banded_n161_problem(members):
    from magi_v2_amd import host
    e, pb = members[0][0], members[1][0]
    assert (e.N, e.D) == (161, 4)
    _init161(e, [pb], 3, seed=80)
    e.sampler_run(30)
    X, sp, tp = e.sampler_samples()
    res = e.sampler_rank_diagnostics()
    _check_sampler(e, res, X, *host.transform_samples(sp, tp, pb["LB"]))
    # (24 draws behind 6 of burn-in: where a chain sits at a column's extreme for five draws the tail indicator is constant, and NaN is the answer)
    assert res["X"]["ess_tail"].shape == (161, 4) and np.all(np.isfinite(res["X"]["ess_bulk"])) and np.any(np.isfinite(res["X"]["ess_tail"]))
    _init161(e, [pb], 3, seed=81, num_results=25)                     # C R = 75, odd: sigma^2 and theta bit for bit too
    e.sampler_run(31)
    X, sp, tp = e.sampler_samples()
    _check_sampler(e, e.sampler_rank_diagnostics(), X, *host.transform_samples(sp, tp, pb["LB"]))


def test_group_member_equals_the_members_own_handle(members):
    from magi_v2_amd.engine import MagiGroup, MagiHipError
    engs, pbs = members
    C, seed = 2, 5
    g = MagiGroup(engs)
    try:
        _init161(g, pbs, C, seed, ids=[0, 1, 0, 1])
        g.sampler_run(30)
        grouped = [g.sampler_rank_diagnostics(member=m) for m in range(2)]
        with pytest.raises(MagiHipError) as ei:                       # chains of two members are never pooled
            g.sampler_rank_diagnostics()
        assert ei.value.code == -1 and "more than one member" in str(ei.value)
        with pytest.raises(MagiHipError):
            g.sampler_rank_diagnostics(chains=range(1, 3))
        again = g.sampler_rank_diagnostics(chains=range(2, 4))
    finally:
        g.close()
    for m in range(2):
        _init161(engs[m], [pbs[m]], C, seed, ids=[0, 1])
        engs[m].sampler_run(30)
        own = engs[m].sampler_rank_diagnostics()
        for b in BLOCKS:
            _same_bits(grouped[m][b], own[b])
    _same_bits(again["thetas"], grouped[1]["thetas"])
    assert not np.array_equal(_bits(grouped[0]["sigma_sqs"]["ess_bulk"]), _bits(grouped[1]["sigma_sqs"]["ess_bulk"]))


# ---- predict ------------------------------------------------------------------------------------------------------------------------

def test_predict_posterior_summary_and_predict_many_carry_the_diagnostics_on_request():
    from magi_v2_amd import predict_many
    from magi_v2_amd.api import MAGI_v2
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seir_alpha_sweep.npz"))
    models = []
    for k in sorted(k for k in z.files if k.startswith("alpha="))[:2]:
        rows = z[k]
        m = MAGI_v2(D_thetas=3, ts_obs=rows[:, 0], X_obs=np.clip(rows[:, 1:5], 0.0, None), bandsize=80, f_vec="seir4")
        m.initial_fit(discretization=1, hparam_iters=0, theta_init_iters=200)
        models.append(m)
    m = models[0]
    kw = dict(n_chains=2, seed=11, max_tree_depth=6)
    stats = {"mean", "sd", "quantiles", "rhat", "ess", "mcse_mean"}
    with pytest.raises(ValueError, match="summary=True"):
        m.predict(8, 6, rank_diagnostics=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # not asked for: no warning of theirs, and today's keys exactly
        plain = m.predict(8, 6, summary=True, **kw)
        today = m.posterior_summary()
    assert set(today) == set(plain["summary"]) == {"X", "sigma_sqs", "thetas", "probs", "n_nonfinite"}
    assert all(set(today[b]) == set(plain["summary"][b]) == stats for b in BLOCKS)
    ranked = m.posterior_summary(rank=True)
    assert all(set(ranked[b]) == stats | set(DIAG) for b in BLOCKS) and ranked["X"]["ess_tail"].shape == ranked["X"]["mean"].shape
    direct = m.engine.sampler_rank_diagnostics()
    for b in BLOCKS:
        _same_bits(ranked[b], direct[b])
        for s in stats:
            np.testing.assert_array_equal(_bits(ranked[b][s]), _bits(today[b][s]), err_msg=s)
    with pytest.warns(UserWarning, match="rank diagnostics: columns beyond the thresholds"):      # 16 draws: every ESS is under 100 per chain
        lean = m.predict(8, 6, summary=True, rank_diagnostics=True, keep_samples=False, **kw)
    assert lean["X_samps"] is None and set(lean["summary"]) == set(today)
    for b in BLOCKS:
        _same_bits(lean["summary"][b], ranked[b])
    with pytest.warns(UserWarning, match="rank diagnostics"):
        many = predict_many(models, 8, 6, summary=True, rank_diagnostics=True, keep_samples=False, **kw)
    for b in BLOCKS:
        _same_bits(many[0]["summary"][b], ranked[b])
    with pytest.warns(UserWarning, match="rank diagnostics"):
        own = models[1].predict(8, 6, summary=True, rank_diagnostics=True, keep_samples=False, **kw)["summary"]
    for b in BLOCKS:
        _same_bits(many[1]["summary"][b], own[b])
    assert set(predict_many(models, 8, 6, summary=True, keep_samples=False, **kw)[0]["summary"]["X"]) == stats
