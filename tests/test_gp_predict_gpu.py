"""GP conditioning of trajectory draws on the GPU (include/magi_hip.h: magi_matern_cross, magi_gp_predict, magi_sampler_gp_predict;
MAGI_v2.posterior_at) against tests/gp_reference.py at the bars tests/test_gp_predict_cpu.py proves sufficient and sharp.

The product reference is fed the device's own cross blocks (magi_matern_cross) and the device's own C^-1 (get_dense): the product tests
see product rounding only, and the Matern kernel is judged separately, against the oracle's accurate columns at the 2e-14 of
tests/test_build_gpu.py."""
import os

import numpy as np
import pytest

from tests import gp_reference as gpr
from tests.util import shuffled_grid, structureless_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = os.path.join(GOLDEN, "seir_alpha_sweep.npz")
STATS = ("mean", "sd", "quantiles", "rhat", "ess", "mcse_mean")
PHI1, PHI2, MU = np.array([0.7, 0.2]), np.array([0.3, 0.15]), np.array([0.35, -0.2])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


# ---- the cross blocks -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [63, 64, 65, 200])
def test_matern_cross_of_the_grid_is_matern_blocks_bit_for_bit(eng, N):
    Is, perm = shuffled_grid(N, 5)
    for I in (Is, Is[perm]):
        Kap, pK, _ = eng.matern_blocks(I, 0.7, 0.3, 2.01)
        Ks, pKs = eng.matern_cross(I, I, 0.7, 0.3, 2.01)
        _same(Ks, Kap, "Kappa")
        _same(pKs, pK, "p_Kappa")
        assert np.array_equal(np.diag(Ks), np.full(N, 0.7)) and np.array_equal(np.diag(pKs), np.zeros(N))


@pytest.mark.parametrize("nu", [2.01, 1.5, 2.5, 3.2])
@pytest.mark.parametrize("T, N", [(1, 129), (127, 300), (130, 65)])
def test_cross_blocks_match_the_oracle(eng, nu, T, N):
    Is, perm = shuffled_grid(N, 7)
    I = Is[perm]
    full, _ = gpr.new_times(I)
    t_new = {1: I[57:58], 127: full[:127], 130: full}[T]              # (1: a coincident time; 130: three of them at the end)
    for phi1, phi2 in ((0.7, 0.3), (0.2, 0.15)):
        Ks, pKs = eng.matern_cross(t_new, I, phi1, phi2, nu)
        rK, rP = gpr.cross_blocks(I, t_new, phi1, phi2, nu)
        eK, eP = relmax(Ks, rK), relmax(pKs, rP)
        print(nu, T, N, phi1, phi2, "Ks", eK, "pKs", eP)
        assert Ks.shape == (T, N) and eK < 2e-14 and eP < 2e-14
        same = t_new[:, None] == I[None, :]
        assert T == 127 or same.sum() >= (1 if T == 1 else 3)          # (a uniform time may fall on a grid time too: the same branch)
        assert np.all(Ks[same] == phi1) and np.all(pKs[same] == 0.0)


def test_cross_blocks_at_large_lags_are_finite_and_far_entries_exactly_zero(eng):
    I = np.linspace(0.0, 100.0, 129)
    t_new = np.array([0.0, 0.013, 50.3, 100.0, 137.0])
    Ks, pKs = eng.matern_cross(t_new, I, 0.05, 0.08, 2.01)
    assert np.isfinite(Ks).all() and np.isfinite(pKs).all()
    assert Ks[0, 0] == 0.05 and Ks[3, -1] == 0.05 and Ks[1, 0] > 0.0
    assert Ks[0, -1] == 0.0 and Ks[1, -1] == 0.0 and pKs[0, -1] == 0.0 and np.all(Ks[4, :64] == 0.0)


# ---- magi_gp_predict ------------------------------------------------------------------------------------------------------------------

class Built:
    """An engine with dense matrices of D = 2 components on the shuffled grid of N points, the device's cross blocks for the 130 test
    times, the device's C^-1, and S = 130 draws."""

    def __init__(self, N, structureless=False):
        from magi_v2_amd.engine import MagiEngine
        Is, perm = shuffled_grid(N, 7)
        self.N, self.I = N, Is[perm]
        self.e = MagiEngine(0)
        if structureless:              # non-symmetric i.i.d. matrices through magi_set_matrices (D = 4)
            pr, _ = structureless_problem(N, "seir4", 21)
            self.e.set_matrices(pr.C_inv, pr.m, pr.K_inv)
            self.phi1, self.phi2, self.mu = np.array([0.7, 0.2, 0.4, 1.3]), np.array([0.3, 0.15, 0.5, 0.2]), np.array([0.35, -0.2, 0.0, 1.5])
        else:
            self.e.build_matrices(self.I, PHI1, PHI2, 2.01, want_host=False)
            self.phi1, self.phi2, self.mu = PHI1, PHI2, MU
        self.D = len(self.phi1)
        self.C_inv, self.m, _ = self.e.get_dense()
        self.t_new, self.grid_idx = gpr.new_times(self.I)
        self.X = gpr.smooth_draws(self.I, 130, self.D, self.mu, seed=11)
        self._ref = {}

    def times(self, T):
        return {1: self.t_new[64:65], 127: self.t_new[:127], 130: self.t_new}[T]

    def reference(self, S, T):
        """(longdouble reference, bars) from the device's own cross blocks and C^-1, computed once per shape"""
        if (S, T) not in self._ref:
            blocks = [self.e.matern_cross(self.times(T), self.I, self.phi1[d], self.phi2[d]) for d in range(self.D)]
            Ks, pKs = np.stack([b[0] for b in blocks]), np.stack([b[1] for b in blocks])
            args = (Ks, pKs, self.C_inv, self.X[:S], self.mu, self.phi1, self.phi2)
            self._ref[(S, T)] = (gpr.predict(*args), gpr.bars(*args), args)
        return self._ref[(S, T)]

    def run(self, S, T, **kw):
        return self.e.gp_predict(self.I, self.phi1, self.phi2, self.mu, self.times(T), self.X[:S], **kw)


_built = {}


def built(N, structureless=False):
    if (N, structureless) not in _built:
        _built[(N, structureless)] = Built(N, structureless)
    return _built[(N, structureless)]


def teardown_module(module):
    for b in _built.values():
        b.e.close()
    _built.clear()


KEYS = ("x_new", "dx_new", "cond_var", "dcond_var")
SHAPES = [(1, 130), (3, 127), (130, 1), (130, 130)]
# the tile edges of the transpose to the host layout (64 x 64 tiles over S draws x nc = rows D columns): S around one and two tiles, with
# gp_chunk_rows 3 and 33 (nc = 6 and 66, below and just above a tile) among the chunkings below
EDGE_SHAPES = [(63, 130), (64, 130), (65, 130), (129, 130)]


def _check_against_reference(b, S, T):
    got = b.run(S, T)
    ref, bars, _ = b.reference(S, T)
    assert got["x_new"].shape == (S, T, b.D) and got["cond_var"].shape == (T, b.D)
    worst = {}
    for k, r, bar in zip(KEYS, ref, bars):
        r = np.maximum(r, 0.0) if k.endswith("var") else r           # (the device clamps the variances at 0)
        worst[k] = float((np.abs(got[k] - r) / bar).max())
    print(b.N, S, T, "worst error / bar:", worst)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert (got["cond_var"] >= 0.0).all() and (got["dcond_var"] >= 0.0).all()
    return got


@pytest.mark.parametrize("S, T", SHAPES + EDGE_SHAPES)
@pytest.mark.parametrize("N", [129, 300])
def test_gp_predict_on_built_matrices_is_within_the_bars_and_independent_of_chunks_and_runs(N, S, T):
    b = built(N)
    got = _check_against_reference(b, S, T)
    try:
        for rows in (1, 3, 33, 64, 129):
            b.e.set_option("gp_chunk_rows", rows)
            chunked = b.run(S, T)
            for k in KEYS:
                _same(chunked[k], got[k], f"{k} with gp_chunk_rows = {rows}")
    finally:
        b.e.set_option("gp_chunk_rows", 0)
    again = b.run(S, T)
    for k in KEYS:
        _same(again[k], got[k], f"{k} on a second run")
    only_x = b.run(S, T, derivative=False)                            # (the derivative planes left out: the values do not move)
    _same(only_x["x_new"], got["x_new"])
    _same(only_x["cond_var"], got["cond_var"])
    assert only_x["dx_new"] is None


@pytest.mark.parametrize("S, T", SHAPES)
@pytest.mark.parametrize("N", [129, 300])
def test_gp_predict_uses_a_non_symmetric_c_inv_as_stored(N, S, T):
    b = built(N, structureless=True)
    assert b.D == 4 and np.abs(b.C_inv - np.transpose(b.C_inv, (0, 2, 1))).max() > 0.1 * np.abs(b.C_inv).max()
    got = _check_against_reference(b, S, T)
    ref, bars, args = b.reference(S, T)
    flipped = gpr.predict(args[0], args[1], np.transpose(b.C_inv, (0, 2, 1)), *args[3:])
    moved = float((np.abs(flipped[0] - ref[0]) / bars[0]).max())
    print("the transposed C^-1 lies", moved, "bars away")
    assert moved >= 1000.0
    try:
        b.e.set_option("gp_chunk_rows", 64)
        chunked = b.run(S, T)
    finally:
        b.e.set_option("gp_chunk_rows", 0)
    for k in KEYS:
        _same(chunked[k], got[k], k)


@pytest.mark.parametrize("N", [129, 300])
def test_rows_at_exact_grid_times_reproduce_the_draw_and_m_times_the_centred_draw(N):
    b = built(N)
    S = 5
    got = b.run(S, 130)
    rows = np.arange(127, 130)
    V = np.ascontiguousarray(np.transpose(b.X[:S] - b.mu, (2, 1, 0)))        # [D, N, S]
    mx = b.e.dense_apply("m", V)                                             # m_d (x_d - mu_d) per draw
    for d in range(b.D):
        Kap, _, _ = b.e.matern_blocks(b.I, b.phi1[d], b.phi2[d], 2.01)
        bound = 100.0 * np.linalg.cond(Kap) * U * np.abs(b.X[:S, :, d]).max()
        ex = np.abs(got["x_new"][:, rows, d] - b.X[:S, b.grid_idx, d]).max()
        ed = np.abs(got["dx_new"][:, rows, d] - mx[d][b.grid_idx, :].T).max()
        print(N, d, "|x_new - x|", ex, "bound", bound, "|dx_new - m (x - mu)|", ed, "bound", bound * np.abs(b.m[d]).max())
        assert ex <= bound and ed <= bound * np.abs(b.m[d]).max()
    far = b.e.gp_predict(b.I, b.phi1, b.phi2, b.mu, [b.I.min() - 50.0, b.I.max() + 50.0], b.X[:S])
    np.testing.assert_allclose(far["x_new"], np.broadcast_to(b.mu, (S, 2, b.D)), rtol=0, atol=1e-12)     # the mean reverts to mu,
    np.testing.assert_allclose(far["cond_var"], np.broadcast_to(b.phi1, (2, b.D)), rtol=1e-12)           # the variance to phi1


# ---- the sampler's device-resident samples ----------------------------------------------------------------------------------------------

RUN = dict(num_results=12, num_burnin_steps=10, max_tree_depth=3)


def _member(pb, band=80):
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    e.build_matrices(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], 2.01, bandsize=band, want_host=False)
    e.set_problem(pb["mu"], pb["N_ds"], pb["idx"], pb["y"], pb["beta"], pb["LB"], "seir4")
    return e


def _init(e, pbs, C, seed, ids=None):
    rep = lambda v: np.repeat(np.asarray(v)[None], C, axis=0)
    X0, s0, t0 = [np.concatenate([rep(pb[k]) for pb in pbs]) for k in ("Xhat", "sig_pre0", "th_pre0")]
    e.sampler_init(e.default_cfg(**RUN), X0, s0, t0, seed=seed, chain_ids=ids)


@pytest.fixture(scope="module")
def members():
    from magi_v2_amd.sweep import alpha_sweep_datasets
    ds = alpha_sweep_datasets(SWEEP, 1)[:2]
    engs = [_member(pb) for _, pb in ds]
    yield engs, [pb for _, pb in ds]
    for e in engs:
        e.close()


def _at(e, pb, t_new, **kw):
    return e.sampler_gp_predict(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], t_new, **kw)


def _check_sampler_route(e, own, pb, t_new, X, **sel):
    """magi_sampler_gp_predict on the resident samples of the selected chains == magi_gp_predict (on the handle ``own`` that holds the
    matrices) and magi_summarize on the downloaded draws X [C, R, N, D], bit for bit"""
    C, R, N, D = X.shape
    got = _at(e, pb, t_new, probs=(0.0, 0.025, 0.5, 0.975, 1.0), return_draws=True, **sel)
    host = own.gp_predict(pb["I"], pb["hp"]["phi1s"], pb["hp"]["phi2s"], pb["mu"], t_new, X.reshape(C * R, N, D))
    T = len(t_new)
    assert got["X_draws"].shape == (C, R, T, D) and got["X"]["quantiles"].shape == (5, T, D)
    _same(got["X_draws"].reshape(C * R, T, D), host["x_new"], "x_new")
    _same(got["dX_draws"].reshape(C * R, T, D), host["dx_new"], "dx_new")
    _same(got["cond_var"], host["cond_var"])
    _same(got["dcond_var"], host["dcond_var"])
    for block, draws in (("X", "X_draws"), ("dX", "dX_draws")):
        ref = own.summarize(got[draws], got["probs"])
        for s in STATS:
            _same(got[block][s], ref[s], f"{block} {s}")
    assert got["n_nonfinite"] == 0
    lean = _at(e, pb, t_new, probs=(0.0, 0.025, 0.5, 0.975, 1.0), **sel)         # (without the draws: the same summaries)
    for s in STATS:
        _same(lean["X"][s], got["X"][s], s)
    return got


def test_sampler_gp_predict_equals_the_host_route_bit_for_bit(members):
    from magi_v2_amd.engine import MagiHipError
    e, pb = members[0][0], members[1][0]
    assert (e.N, e.D) == (161, 4)
    t_new, _ = gpr.new_times(pb["I"])
    _init(e, [pb], 3, seed=31)
    e.sampler_run(5)
    with pytest.raises(MagiHipError) as ei:                           # the chains have not finished
        _at(e, pb, t_new)
    assert ei.value.code == -5
    e.sampler_run(RUN["num_results"] + RUN["num_burnin_steps"])
    X, _, _ = e.sampler_samples()
    whole = _check_sampler_route(e, e, pb, t_new, X)
    _check_sampler_route(e, e, pb, t_new, X[1:3], chains=range(1, 3))
    _check_sampler_route(e, e, pb, t_new, X[2:3], chains=slice(2, 3))
    for bad in (range(2, 4), [0, 2]):
        with pytest.raises((MagiHipError, ValueError)):
            _at(e, pb, t_new, chains=bad)
    try:
        e.set_option("gp_chunk_rows", 7)
        chunked = _at(e, pb, t_new, probs=(0.0, 0.025, 0.5, 0.975, 1.0))
    finally:
        e.set_option("gp_chunk_rows", 0)
    for block in ("X", "dX"):
        for s in STATS:
            _same(chunked[block][s], whole[block][s], f"{block} {s} in chunks of 7 rows")


def test_group_member_route_uses_the_members_own_matrices_and_rejects_a_range_across_members(members):
    from magi_v2_amd.engine import MagiGroup, MagiHipError
    engs, pbs = members
    t_new, _ = gpr.new_times(pbs[0]["I"])
    g = MagiGroup(engs)
    try:
        _init(g, pbs, 2, 5, ids=[0, 1, 0, 1])
        g.sampler_run(RUN["num_results"] + RUN["num_burnin_steps"])
        X, _, _ = g.sampler_samples()
        grouped = [_check_sampler_route(g, engs[m], pbs[m], t_new, X[2 * m:2 * m + 2], member=m) for m in range(2)]
        _check_sampler_route(g, engs[1], pbs[1], t_new, X[3:4], chains=range(3, 4))          # a range inside one member
        for bad in (dict(), dict(chains=range(1, 3))):                                       # ranges across the members
            with pytest.raises(MagiHipError) as ei:
                _at(g, pbs[0], t_new, **bad)
            assert ei.value.code == -1
    finally:
        g.close()
    assert not np.array_equal(grouped[0]["X"]["mean"], grouped[1]["X"]["mean"])
    for m in range(2):                                                                       # the member's own handle: the same bits
        _init(engs[m], [pbs[m]], 2, 5, ids=[0, 1])
        engs[m].sampler_run(RUN["num_results"] + RUN["num_burnin_steps"])
        own = _at(engs[m], pbs[m], t_new, probs=(0.0, 0.025, 0.5, 0.975, 1.0))
        for s in STATS:
            _same(own["X"][s], grouped[m]["X"][s], s)


# ---- MAGI_v2.posterior_at -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    from magi_v2_amd.api import MAGI_v2
    z = np.load(SWEEP)
    names = sorted(k for k in z.files if k.startswith("alpha="))
    out = []
    for k in names[:2]:
        rows = z[k]
        m = MAGI_v2(D_thetas=3, ts_obs=rows[:, 0], X_obs=np.clip(rows[:, 1:5], 0.0, None), bandsize=80, f_vec="seir4")
        m.initial_fit(discretization=1, hparam_iters=0, theta_init_iters=200)
        out.append(m)
    return out


def test_posterior_at(models):
    from magi_v2_amd import predict_many
    from magi_v2_amd.api import MAGI_v2
    m = models[0]
    with pytest.raises(RuntimeError):
        MAGI_v2(D_thetas=3, ts_obs=m.ts_obs, X_obs=m.X_obs, bandsize=80, f_vec="seir4").posterior_at([0.5])
    kw = dict(n_chains=2, seed=11, max_tree_depth=3)
    full = m.predict(12, 10, summary=True, **kw)
    I = np.asarray(m.I).reshape(-1)
    t_new, _ = gpr.new_times(I)
    T, D = len(t_new), m.D
    at = m.posterior_at(t_new, return_draws=True)
    assert set(at) == {"t", "X", "dX", "cond_sd", "dcond_sd", "pred_sd", "probs", "n_nonfinite", "X_draws", "dX_draws"}
    assert set(at["X"]) == set(STATS) == set(at["dX"])
    assert at["X"]["mean"].shape == (T, D) and at["dX"]["quantiles"].shape == (3, T, D) and at["cond_sd"].shape == (T, D)
    assert at["X_draws"].shape == (2, 12, T, D) and at["dX_draws"].shape == (2, 12, T, D) and at["n_nonfinite"] == 0
    # pred_sd = sqrt(sd^2 + cond_var) with cond_sd = sqrt(cond_var): squaring the root again moves cond_var by an ulp or two
    np.testing.assert_allclose(at["pred_sd"], np.sqrt(at["X"]["sd"] ** 2 + at["cond_sd"] ** 2), rtol=8 * U, atol=0)
    assert (at["pred_sd"] >= at["X"]["sd"]).all() and (at["pred_sd"] >= at["cond_sd"]).all()
    _same(at["X"]["mean"], m.engine.summarize(at["X_draws"])["mean"])
    plain = m.posterior_at(t_new, derivative=False, probs=(0.1, 0.9))
    assert "dX" not in plain and "X_draws" not in plain and plain["X"]["quantiles"].shape == (2, T, D)
    _same(plain["X"]["mean"], at["X"]["mean"])
    # the grid itself: the posterior mean of X on the grid, to the bound of exact grid times
    on_grid = m.posterior_at(I)
    for d in range(D):
        Kap, _, _ = m.engine.matern_blocks(I, m.phi1s[d], m.phi2s[d], 2.01)
        bound = 100.0 * np.linalg.cond(Kap) * U * np.abs(full["X_samps"][..., d]).max()
        err = np.abs(on_grid["X"]["mean"][:, d] - full["summary"]["X"]["mean"][:, d]).max()
        print(d, "posterior_at(I) against posterior_summary:", err, "bound", bound)
        assert err <= bound
    # legal without the samples on the host, and the same bits
    lean = m.predict(12, 10, summary=True, keep_samples=False, **kw)
    assert lean["X_samps"] is None
    again = m.posterior_at(t_new)
    for s in STATS:
        _same(again["X"][s], at["X"][s], s)
        _same(again["dX"][s], at["dX"][s], s)
    # predict_many: a grouped model's through the group's handle and its member index
    many = predict_many(models, 12, 10, keep_samples=False, posterior_at=t_new, **kw)
    assert many[0]["X_samps"] is None and "summary" not in many[0]
    for s in STATS:
        _same(many[0]["posterior_at"]["X"][s], at["X"][s], s)
    _same(many[0]["posterior_at"]["pred_sd"], at["pred_sd"])
    models[1].predict(12, 10, **kw)
    own = models[1].posterior_at(t_new)
    for s in STATS:
        _same(many[1]["posterior_at"]["dX"][s], own["dX"][s], s)


# ---- rejected arguments ---------------------------------------------------------------------------------------------------------------

def test_rejected_arguments_leave_the_handle_usable(members):
    from magi_v2_amd.engine import MagiEngine, _dp
    import ctypes as C
    b = built(129)
    e, lib = b.e, b.e._lib
    p = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_dp)
    N, D, S, T = b.N, b.D, 3, 4
    keep = dict(I=b.I.copy(), phi1=b.phi1.copy(), phi2=b.phi2.copy(), mu=b.mu.copy(), t=b.t_new[:T].copy(), X=np.ascontiguousarray(b.X[:S]))
    x_new, cv, Ks = np.empty((S, T, D)), np.empty((T, D)), np.empty((T, N))
    nan = lambda a, i=0: np.concatenate([a[:i], [np.nan], a[i + 1:]])
    inf = lambda a, i=0: np.concatenate([a[:i], [np.inf], a[i + 1:]])

    def predict(N=N, D=D, nu=2.01, T=T, S=S, out=x_new, **over):
        a = {**keep, **over}
        return lib.magi_gp_predict(e._h, p(a["I"]), N, D, p(a["phi1"]), p(a["phi2"]), nu, p(a["mu"]), T, p(a["t"]), S, p(a["X"]), p(out), None, p(cv), None)

    def cross(T=T, N=N, phi1=0.7, phi2=0.3, nu=2.01, **over):
        a = {**keep, **over}
        return lib.magi_matern_cross(e._h, p(a["t"]), T, p(a["I"]), N, phi1, phi2, nu, p(Ks), None)

    assert predict() == 0 and cross() == 0
    first = x_new.copy()
    # (the sizes are checked before a draw is read: the oversized shapes never touch memory)
    for kw in (dict(T=0), dict(T=(1 << 16) + 1), dict(S=0), dict(S=(1 << 20) + 1), dict(S=1 << 20, T=300), dict(N=1), dict(D=0), dict(D=99),
               dict(I=None), dict(phi1=None), dict(phi2=None), dict(mu=None), dict(t=None), dict(X=None),
               dict(t=nan(keep["t"], 2)), dict(t=inf(keep["t"])), dict(I=nan(keep["I"], 100)), dict(I=inf(keep["I"], 5)), dict(mu=nan(keep["mu"], 1)),
               dict(phi1=np.array([0.7, 0.0])), dict(phi2=np.array([-0.3, 0.15])), dict(phi1=nan(keep["phi1"])), dict(nu=1.0), dict(nu=float("nan"))):
        assert predict(**kw) == -1, kw
        assert predict() == 0, kw                                     # the next call succeeds,
    _same(x_new, first)                                               # with the same bits
    for kw in (dict(T=0), dict(T=(1 << 16) + 1), dict(N=0), dict(t=None), dict(I=None), dict(t=nan(keep["t"])), dict(I=inf(keep["I"], 7)),
               dict(phi1=0.0), dict(phi2=-1.0), dict(nu=1.0)):
        assert cross(**kw) == -1, kw
        assert cross() == 0, kw
    assert lib.magi_gp_predict(e._h, p(keep["I"][:100]), 100, D, p(keep["phi1"]), p(keep["phi2"]), 2.01, p(keep["mu"]), T, p(keep["t"]), S, p(keep["X"]),
                               p(x_new), None, None, None) == -5      # no resident matrices of this N
    fresh = MagiEngine(0)
    try:
        assert lib.magi_gp_predict(fresh._h, p(keep["I"]), N, D, p(keep["phi1"]), p(keep["phi2"]), 2.01, p(keep["mu"]), T, p(keep["t"]), S, p(keep["X"]),
                                   p(x_new), None, None, None) == -5  # no resident matrices at all
        assert fresh._lib.magi_matern_cross(fresh._h, p(keep["t"]), T, p(keep["I"]), N, 0.7, 0.3, 2.01, p(Ks), None) == 0      # needs none
    finally:
        fresh.close()
    assert predict() == 0
    _same(x_new, first)
    with pytest.raises(Exception):
        e.set_option("gp_chunk_rows", (1 << 16) + 1)
    with pytest.raises(Exception):
        e.set_option("gp_chunk_rows", -1)

    # the sampler's call: its own preconditions, then the same checks
    s, pb = members[0][0], members[1][0]
    mean = np.empty((T, 4))
    nf = C.c_int32(0)
    sk = dict(I=np.asarray(pb["I"], dtype=np.float64).copy(), phi1=np.asarray(pb["hp"]["phi1s"], dtype=np.float64).copy(),
              phi2=np.asarray(pb["hp"]["phi2s"], dtype=np.float64).copy(), t=keep["t"].copy(), probs=np.array([0.5]))

    def sampler(chain0=0, n_sel=2, nu=2.01, T=T, n_q=1, **over):
        a = {**sk, **over}
        return s._lib.magi_sampler_gp_predict(s._h, chain0, n_sel, p(a["I"]), p(a["phi1"]), p(a["phi2"]), nu, T, p(a["t"]), n_q, p(a["probs"]), 0,
                                              None, None, None, None, p(mean), *([None] * 11), C.byref(nf))

    _init(s, [pb], 2, seed=9)
    assert sampler() == -5                                            # the chains have not finished
    s.sampler_run(RUN["num_results"] + RUN["num_burnin_steps"])
    assert sampler() == 0
    first_mean = mean.copy()
    for kw in (dict(chain0=-1), dict(chain0=1, n_sel=2), dict(n_sel=0), dict(T=0), dict(T=(1 << 16) + 1), dict(I=None), dict(phi1=None), dict(phi2=None),
               dict(t=None), dict(t=nan(sk["t"])), dict(I=inf(sk["I"], 3)), dict(phi1=np.array([0.7, 0.2, -1.0, 0.3])), dict(nu=0.5),
               dict(n_q=17), dict(n_q=-1), dict(probs=np.array([1.5])), dict(probs=np.array([np.nan])), dict(probs=None)):
        assert sampler(**kw) == -1, kw
        assert sampler() == 0, kw
    _same(mean, first_mean)
