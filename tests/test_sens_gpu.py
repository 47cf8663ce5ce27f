"""Forward sensitivities and Fisher information on the GPU (include/magi_hip.h: magi_ode_sensitivities, magi_sampler_sensitivities;
csrc/sens.hip; MagiEngine.ode_sensitivities / sampler_sensitivities, MAGI_v2.posterior_sensitivities) against the complex-step truth of
tests/sens_reference.py, which uses the drift callable alone and no Jacobian code.

Bar: 1e-11 of a column's max |sens| over draws, times and components.  tests/test_sens_cpu.py shows on the CPU that the two independent
truths and their float64 / longdouble runs agree within 1/100 of it on every case used here, and that every wrong scheme -- a df/dtheta
term missing at a stage, J_x^T, a stale stage increment, a Jacobian at the wrong stage time -- moves a column by >= 1000 bars.
Fisher information: 8 n_obs 2^-52 sqrt(F_aa F_bb) against the numpy restatement on the downloaded device sensitivities.

Measured on an MI355X, worst column of the 257-draw batch as a fraction of its bar, substeps 4 / substeps 1:
    seir3 1.4e-04            sirw 1.5e-04             fhn 9.0e-04              lotka_volterra 5.8e-04 / 3.0e-04
    seir_seasonal 1.4e-04 / 8.1e-05                   chain8 1.3e-04 / 8.6e-05 sqrt_outflow 1.6e-04
The trajectories were bit-equal to ode_solve's on every case (the test asks for ode_solve's bar and equal status).
mean / sd against numpy on the downloaded draws: <= 1.8e-02 of the summation-order bound; fim 1.5e-03, fim_mean 1.3e-03 of their bar."""
import ctypes as C
import dataclasses
import warnings

import numpy as np
import pytest

from magi_v2_amd import drift as drift_mod
from magi_v2_amd import host
from magi_v2_amd.engine import MagiEngine, MagiGroup, MagiHipError, _ptr
from tests import ode_reference as R
from tests import sens_reference as SR
from tests.util import engine_for, load_g4, problem_from_g4

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65)               # lane, wave and workgroup edges: the leading draws of the 257-draw batch
KEYS = ("trajectories", "sens", "sens_mean", "sens_sd", "status")
FIM_KEYS = ("fim", "fim_mean")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, keys, msg=""):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{msg} {k}")


@pytest.fixture(scope="module")
def engines():
    """name -> (engine, what to pass as ``drift``): the base library for the compiled-in drifts, the traced drift's own library otherwise."""
    made = {}

    def get(name):
        key = "base" if name in R.BUILTIN else name
        if key not in made:
            d = None if name in R.BUILTIN else drift_mod.resolve(*R.TRACED[name])
            made[key] = (MagiEngine(0) if d is None else MagiEngine(0, drift=d), d)
        eng, d = made[key]
        return eng, (name if d is None else d)

    yield get
    for eng, _ in made.values():
        eng.close()


def sens(engines, name, x0, th, t, substeps=4, **kw):
    eng, d = engines(name)
    return eng.ode_sensitivities(x0, th, t, substeps=substeps, drift=d, **kw)


@pytest.fixture(scope="module")
def full(engines):
    """The 257-draw, all-column device result of a case at a sub-step count, computed once and shared: treat it as read-only."""
    made = {}

    def get(name, substeps=4):
        if (name, substeps) not in made:
            case = R.CASES[name]
            x0, th = R.draws(case)
            made[name, substeps] = sens(engines, name, x0, th, case.t, substeps)
        return made[name, substeps]

    return get


@pytest.mark.parametrize("drift,substeps", [(d, 4) for d in R.CASES] + [(d, 1) for d in R.SUBSTEPS_1_CASES])
def test_parity_with_the_complex_step_truth_and_with_ode_solve(engines, full, drift, substeps):
    """257 draws, all P + D columns: every column within its bar of truth (a); the trajectories within ode_solve's bar of ode_solve's,
    with equal status."""
    case = R.CASES[drift]
    out = full(drift, substeps)
    want = SR.reference(drift, substeps, "complex", "float64")
    Q = case.P + case.D
    assert out["sens"].shape == (R.BATCH, len(case.t), case.D, Q) and out["n_failed"] == 0 and list(out["cols"]) == list(range(Q))
    b = SR.bars(out["sens"], want)
    eng, d = engines(drift)
    x0, th = R.draws(case)
    solved = eng.ode_solve(x0, th, case.t, substeps=substeps, drift=d)
    tb = float(np.abs(out["trajectories"] - solved["trajectories"]).max() / (R.BAR * np.abs(solved["trajectories"]).max()))
    same = np.array_equal(_bits(out["trajectories"]), _bits(solved["trajectories"]))
    print(f"sens parity {drift} substeps={substeps}: worst column {b.max():.2e} of its bar; trajectories vs ode_solve {tb:.2e} of the bar, "
          f"bit-equal: {same}")
    assert b.max() <= 1.0, (drift, substeps, b)
    assert tb <= 1.0
    np.testing.assert_array_equal(out["status"], solved["status"])
    eye = np.zeros((case.D, Q))
    eye[:, case.P:] = np.eye(case.D)
    np.testing.assert_array_equal(out["sens"][:, 0], np.broadcast_to(eye, (R.BATCH,) + eye.shape))       # output 0: s(t_0)


@pytest.mark.parametrize("drift", ("sirw", "seir_seasonal", "chain8"))
def test_a_draw_and_a_column_have_the_same_bits_in_any_launch_shape(engines, full, drift):
    """The leading S = 1, 63, 64, 65 draws, the columns [P + D - 1, 0] and [P] alone, and a repeated call give the bits of the 257-draw,
    all-column call."""
    case = R.CASES[drift]
    x0, th = R.draws(case)
    big = full(drift)
    for S in SIZES:
        out = sens(engines, drift, x0[:S], th[:S], case.t)
        for k in ("trajectories", "sens", "status"):
            np.testing.assert_array_equal(_bits(out[k]), _bits(big[k][:S]), err_msg=f"S={S} {k}")
    Q = case.P + case.D
    for cols in ([Q - 1, 0], [case.P]):
        out = sens(engines, drift, x0, th, case.t, wrt=cols)
        assert out["sens"].shape[-1] == len(cols)
        np.testing.assert_array_equal(_bits(out["sens"]), _bits(big["sens"][..., cols]), err_msg=str(cols))
        np.testing.assert_array_equal(_bits(out["sens_mean"]), _bits(big["sens_mean"][..., cols]))
        np.testing.assert_array_equal(_bits(out["trajectories"]), _bits(big["trajectories"]))
    _same(sens(engines, drift, x0, th, case.t), big, KEYS, "repeat")
    bare = sens(engines, drift, x0, th, case.t, return_draws=False)
    assert bare["sens"] is None and bare["trajectories"] is None
    _same(bare, big, ("sens_mean", "sens_sd", "status"), "without draws")


@pytest.mark.parametrize("drift", ("seir3", "sqrt_outflow"))
def test_relative_is_the_unscaled_result_times_the_draws_own_value(engines, full, drift):
    case = R.CASES[drift]
    x0, th = R.draws(case)
    out = sens(engines, drift, x0, th, case.t, relative=True)
    scale = np.concatenate([th, x0], axis=1)                  # [S, Q]: theta_q, then the x0 components
    np.testing.assert_array_equal(_bits(out["sens"]), _bits(full(drift)["sens"] * scale[:, None, None, :]))
    np.testing.assert_array_equal(_bits(out["trajectories"]), _bits(full(drift)["trajectories"]))


def _all_obs(T, D, S, link=None):
    return {"j": np.repeat(np.arange(T), D), "comp": np.tile(np.arange(D), T), "sigma_sq": np.full((S, D), 1e-4), "weight": None, "link": link}


def test_failed_draws_are_marked_and_left_out_of_every_mean(engines):
    """The five sqrt_outflow draws of ode_reference.status_inputs: status (16, 18, 13, 23, 0); the survivor has the bits it has alone and is
    alone in the means; the Fisher information of the failed draws is NaN and they are counted."""
    x0, th = R.status_inputs()
    T, D = len(R.STATUS_T), 2
    out = sens(engines, "sqrt_outflow", x0, th, R.STATUS_T, R.STATUS_SUBSTEPS, obs=_all_obs(T, D, 5))
    assert tuple(out["status"]) == R.STATUS_WANT and out["n_failed"] == 4 and out["n_fim_excluded"] == 4
    alone = sens(engines, "sqrt_outflow", x0[4:], th[4:], R.STATUS_T, R.STATUS_SUBSTEPS, obs=_all_obs(T, D, 1))
    for k in ("trajectories", "sens", "fim"):
        np.testing.assert_array_equal(_bits(out[k][4]), _bits(alone[k][0]), err_msg=k)
    want = SR.complex_step(R.callable_for("sqrt_outflow"), x0[4:], th[4:], R.STATUS_T, R.STATUS_SUBSTEPS)
    assert SR.bars(alone["sens"], want).max() <= 1.0
    np.testing.assert_array_equal(_bits(out["sens_mean"]), _bits(out["sens"][4]))
    np.testing.assert_array_equal(_bits(out["fim_mean"]), _bits(out["fim"][4]))
    assert np.isnan(out["sens_sd"]).all() and np.isnan(out["fim"][:4]).all() and np.isfinite(out["fim"][4]).all()
    x0b, thb = R.status_inputs(True)
    two = sens(engines, "sqrt_outflow", x0b, thb, R.STATUS_T, R.STATUS_SUBSTEPS, obs=_all_obs(T, D, 6))
    assert tuple(two["status"]) == R.STATUS_WANT + (0,) and two["n_failed"] == 4 and two["n_fim_excluded"] == 4
    assert np.isfinite(two["sens_mean"]).all() and np.isfinite(two["sens_sd"]).all() and np.isfinite(two["fim_mean"]).all()
    np.testing.assert_array_equal(_bits(two["sens"][:5]), _bits(out["sens"]))
    none = sens(engines, "sqrt_outflow", x0[:4], th[:4], R.STATUS_T, R.STATUS_SUBSTEPS, obs=_all_obs(T, D, 4))
    assert none["n_failed"] == 4 and none["n_fim_excluded"] == 4 and np.isnan(none["sens_mean"]).all() and np.isnan(none["fim_mean"]).all()


@pytest.mark.parametrize("drift,S", [("chain8", 257), ("sirw", 65), ("sqrt_outflow", 6)])
def test_mean_and_sd_are_numpy_on_the_downloaded_draws(engines, drift, S):
    """Against numpy (ddof = 1) on the device's own sensitivities restricted to status 0, within the summation-order bound
    4 S 2^-53 max |sens| of tests/test_ode_gpu.py, per column."""
    if drift == "sqrt_outflow":
        (x0, th), t, sub = R.status_inputs(True), R.STATUS_T, R.STATUS_SUBSTEPS
    else:
        case = R.CASES[drift]
        (x0, th), t, sub = R.draws(case, S), case.t, 4
    out = sens(engines, drift, x0, th, t, sub)
    ok = out["status"] == 0
    z = out["sens"][ok]
    bound = 4.0 * S * 2.0 ** -53 * np.abs(z).max(axis=(0, 1, 2))
    em = np.abs(out["sens_mean"] - z.mean(axis=0)).max(axis=(0, 1))
    es = np.abs(out["sens_sd"] - z.std(axis=0, ddof=1)).max(axis=(0, 1))
    print(f"sens stats {drift} S={S} ({int(ok.sum())} finite): mean {(em / bound).max():.2e}, sd {(es / bound).max():.2e} of the summation-order bound")
    assert (em <= bound).all() and (es <= bound).all()


def test_fisher_information_is_the_numpy_restatement_on_the_device_sensitivities(engines):
    """sirw, 65 draws, 164 observations, a log and a sqrt link, weights and a variance per draw: fim against the restatement on the
    downloaded sensitivities, symmetric bit for bit; fim_mean against numpy; no observations, no Fisher information and the same sens."""
    fs = SR.fisher_setup()
    o = fs["obs"]
    n_obs = len(o["j"])
    assert n_obs == 164
    out = sens(engines, SR.FIM_CASE, fs["x0"], fs["theta"], fs["t"], obs=o)
    assert out["n_failed"] == 0 and out["n_fim_excluded"] == 0 and out["fim"].shape == (SR.FIM_S, 9, 9)
    want = SR.fisher(out["sens"], out["trajectories"], o["j"], o["comp"], o["weight"], o["sigma_sq"], o["link"])
    bar = SR.fisher_bar(want, n_obs)
    e = float((np.abs(out["fim"] - want) / bar).max())
    np.testing.assert_array_equal(_bits(out["fim"]), _bits(out["fim"].transpose(0, 2, 1)))
    em = float((np.abs(out["fim_mean"] - out["fim"].mean(axis=0)) / SR.fisher_bar(out["fim_mean"], n_obs)).max())
    print(f"fisher: fim {e:.2e}, fim_mean {em:.2e} of the bar")
    assert e <= 1.0 and em <= 1.0
    for v in SR.FIM_VARIANTS:                                # the bar tells the restatement from every wrong one
        wrong = SR.fisher(out["sens"], out["trajectories"], o["j"], o["comp"], o["weight"], o["sigma_sq"], o["link"], variant=v)
        assert float((np.abs(out["fim"] - wrong) / bar).max()) >= 1e3, v
    rep = host.fisher_report(out["fim_mean"], SR.names(R.CASES[SR.FIM_CASE]), collinearity_warn=np.inf)
    assert np.isfinite(rep["eigenvalues"]).all() and rep["eigenvalues"][-1] > 0
    plain = sens(engines, SR.FIM_CASE, fs["x0"], fs["theta"], fs["t"])
    assert "fim" not in plain and "fim_mean" not in plain
    _same(plain, out, KEYS, "n_obs = 0")
    empty = sens(engines, SR.FIM_CASE, fs["x0"], fs["theta"], fs["t"], obs={**o, "j": o["j"][:0], "comp": o["comp"][:0], "weight": None})
    assert "fim" not in empty
    _same(empty, out, KEYS, "an empty list")
    # relative: the Fisher information of the log parameters is formed from the scaled sensitivities
    rel = sens(engines, SR.FIM_CASE, fs["x0"], fs["theta"], fs["t"], obs=o, relative=True)
    wr = SR.fisher(rel["sens"], rel["trajectories"], o["j"], o["comp"], o["weight"], o["sigma_sq"], o["link"])
    assert float((np.abs(rel["fim"] - wr) / SR.fisher_bar(wr, n_obs)).max()) <= 1.0


def test_rejected_arguments_raise_and_leave_the_handle_usable(engines, full):
    eng, _ = engines("seir3")
    case = R.CASES["seir3"]
    x0, th = R.draws(case, 5)
    t = case.t
    T = len(t)
    good_obs = _all_obs(T, 3, 5)

    def call(**kw):
        obs = kw.pop("obs", None)
        return eng.ode_sensitivities(kw.get("x0", x0), kw.get("th", th), kw.get("t", t), substeps=kw.get("substeps", 4), drift=kw.get("drift", "seir3"),
                                     wrt=kw.get("wrt"), obs=obs)

    big = (1 << 20) + 1
    bad = [("S <= 2\\^20", dict(x0=np.empty((0, 3)), th=np.empty((0, 3)))),
           ("S <= 2\\^20", dict(x0=np.zeros((big, 3)), th=np.zeros((big, 3)))),
           ("T <= 2\\^16", dict(t=t[:1])),
           ("substeps <= 1024", dict(substeps=0)),
           ("substeps <= 1024", dict(substeps=1025)),
           ("exceeds 2\\^28", dict(x0=np.zeros((1 << 12, 3)), th=np.zeros((1 << 12, 3)), t=np.arange(float(1 << 13)))),      # 2^12 2^13 3 6 > 2^28 >= 2^12 2^13 3
           ("drift expects P=3", dict(th=np.ones((5, 4)))),
           ("not strictly increasing at index 3", dict(t=np.array([0.0, 0.1, 0.2, 0.2, 0.3]))),
           ("t_out\\[2\\] is not finite", dict(t=np.array([0.0, 0.1, np.nan, 0.3]))),
           ("n_col <= P \\+ D", dict(wrt=[])),
           ("n_col <= P \\+ D", dict(wrt=[0, 1, 2, 3, 4, 5, 0])),
           ("cols\\[1\\] is outside", dict(wrt=[0, 6])),
           ("cols\\[0\\] is outside", dict(wrt=[-1])),
           ("cols\\[2\\] repeats cols\\[0\\]", dict(wrt=[4, 1, 4])),
           ("obs_j\\[1\\] is outside", dict(obs={**good_obs, "j": np.array([0, T]), "comp": np.array([0, 0])})),
           ("obs_j\\[0\\] is outside", dict(obs={**good_obs, "j": np.array([-1]), "comp": np.array([0])})),
           ("obs_comp\\[0\\] is outside", dict(obs={**good_obs, "j": np.array([1]), "comp": np.array([3])})),
           ("obs_weight\\[2\\] is not a finite number > 0", dict(obs={**good_obs, "weight": np.r_[1.0, 1.0, 0.0, np.ones(3 * T - 3)]})),
           ("obs_weight\\[0\\] is not a finite number > 0", dict(obs={**good_obs, "weight": np.r_[np.inf, np.ones(3 * T - 1)]})),
           ("sigma_sq\\[4\\] is not a finite number > 0", dict(obs={**good_obs, "sigma_sq": np.r_[np.ones(4), -1.0, np.ones(10)].reshape(5, 3)})),
           ("sigma_sq\\[0\\] is not a finite number > 0", dict(obs={**good_obs, "sigma_sq": np.r_[np.nan, np.ones(14)].reshape(5, 3)})),
           ("link\\[1\\] = 3 is none of", dict(obs={**good_obs, "link": [0, 3, 0]})),
           ("sigma_sq is NULL", dict(obs={**good_obs, "sigma_sq": None}))]
    for msg, kw in bad:
        with pytest.raises(MagiHipError, match=msg) as e:
            call(**kw)
        assert e.value.code == -1, msg
    ip = C.POINTER(C.c_int32)
    cols = np.arange(6, dtype=np.int32)
    raw = lambda x0p, thp, tp, cp: eng._lib.magi_ode_sensitivities(eng._h, 0, 3, 5, x0p, thp, T, tp, 4, 6, cp, 0, 0, None, None, None, None, None,
                                                                   None, None, None, None, None, None, None, None, None)
    for k in range(4):                                        # a null x0, theta, t_out or cols
        ptrs = [_ptr(x0), _ptr(th), _ptr(t), cols.ctypes.data_as(ip)]
        ptrs[k] = None
        with pytest.raises(MagiHipError, match="null pointer|cols is NULL"):
            eng._check(raw(*ptrs))
    with pytest.raises(MagiHipError, match="unknown drift id"):
        eng._check(eng._lib.magi_ode_sensitivities(eng._h, 3, 3, 5, _ptr(x0), _ptr(th), T, _ptr(t), 4, 6, cols.ctypes.data_as(ip), 0, 0, *([None] * 14)))
    eng._check(raw(_ptr(x0), _ptr(th), _ptr(t), cols.ctypes.data_as(ip)))          # every output pointer is optional
    out = call(obs=good_obs)
    np.testing.assert_array_equal(_bits(out["sens"]), _bits(full("seir3")["sens"][:5]))
    assert out["n_fim_excluded"] == 0 and np.isfinite(out["fim_mean"]).all()


# ---- the sampler route ---------------------------------------------------------------------------------------------------------------------

RUN = dict(num_results=20, num_burnin_steps=20, max_tree_depth=3)
LINKS = ["log", "identity", "identity", "identity"]
SUPPORT = ["positive", ("lower", 0.1), "positive", "real", "positive"]
FIXED = 4e-3


def _model(e, w):
    e.set_theta_support(SUPPORT)
    e.set_prior([None, ("fixed", FIXED), None, None], None)
    e.set_obs_model(LINKS, w)


def _start(e, X0, s0, P, Cn, seed, ids=None):
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], Cn, axis=0)
    e.sampler_init(e.default_cfg(**RUN), rep(X0), rep(s0), rep(np.zeros(P)), seed=seed, chain_ids=ids)
    return RUN["num_results"] + RUN["num_burnin_steps"]


@pytest.fixture(scope="module")
def sirw():
    """The golden SIRW N = 41 problem with positive data (a log link on component 0), weights 1 / 2 / 4, a lower-bounded and a real theta and
    a fixed sigma^2: (engine, problem, weights, X0, sig_pre0)."""
    g = load_g4("sirw_N41")
    base = problem_from_g4(g, None)
    p = dataclasses.replace(base, y=np.abs(np.asarray(base.y)) + 0.05)
    w = np.random.default_rng(8).choice([1.0, 2.0, 4.0], size=len(p.obs_idx))
    e = engine_for(p, None)
    _model(e, w)
    X0 = np.clip(np.asarray(g["Xhat_init"], dtype=np.float64), 0.02, None)
    s0 = np.log(np.expm1(np.full(p.D, 0.05) - p.LB))
    yield e, p, w, X0, s0
    e.close()


def _direct(e, p, w, r, t_out, grid_out, **kw):
    """ode_sensitivities on the draws the sampler route used, with the observation list counted independently in numpy."""
    idx = np.asarray(p.obs_idx)                              # host layout i D + d, aligned with the weights
    i, d = idx // p.D, idx % p.D
    use = grid_out[i] >= 0
    order = np.argsort((d * p.N + i)[use], kind="stable")
    i, d, ww = i[use][order], d[use][order], w[use][order]
    assert r["n_obs_used"] == int(use.sum())
    np.testing.assert_array_equal(r["obs_index"], np.stack([i, d], axis=1))
    obs = {"j": grid_out[i], "comp": d, "weight": ww, "sigma_sq": r["sigma_sq"], "link": LINKS}
    return e.ode_sensitivities(r["x0"], r["theta"], t_out, obs=obs, drift="sirw", **kw)


def test_sampler_route_equals_ode_sensitivities_on_the_downloaded_draws(sirw):
    e, p, w, X0, s0 = sirw
    I = np.asarray(p.I, dtype=np.float64).reshape(-1)
    lp0 = e.logpost_grad(X0, s0, np.zeros(p.P))
    total = _start(e, X0, s0, p.P, 2, seed=31)
    e.sampler_run(7)
    with pytest.raises(MagiHipError) as ei:                  # inside a paused run: refused, and the run goes on as if never asked
        e.sampler_sensitivities(I)
    assert ei.value.code == -5 and "transitions" in str(ei.value)
    e.sampler_run(total)
    X, sp, tp = e.sampler_samples()
    s2 = e.sampler_ppc(sigma_sq=True)["sigma_sq"]
    kinds, bounds = e.theta_support()
    th_host = host.transform_thetas(tp, kinds, bounds)
    dt = I[1] - I[0]
    first = None
    for start, thin, past in ((0, 1, 0), (7, 3, 5), (0, 3, 0), (7, 1, 5)):
        t_out = np.concatenate([I[start:], I[-1] + dt * np.arange(1, past + 1)])
        grid_out = np.where(np.arange(p.N) >= start, np.arange(p.N) - start, -1).astype(np.int32)
        r = e.sampler_sensitivities(t_out, grid_out, start_index=start, thin=thin)
        S = 2 * len(range(0, RUN["num_results"], thin))
        assert r["sens"].shape == (S, len(t_out), p.D, p.P + p.D) and r["n_failed"] == 0
        np.testing.assert_array_equal(_bits(r["x0"]), _bits(X[:, ::thin, start, :].reshape(S, p.D)))
        np.testing.assert_array_equal(_bits(r["sigma_sq"]), _bits(s2[:, ::thin].reshape(S, p.D)))
        assert (r["sigma_sq"][:, 1] == FIXED).all()
        np.testing.assert_allclose(r["theta"], th_host[:, ::thin].reshape(S, p.P), rtol=1e-14, atol=1e-15)
        direct = _direct(e, p, w, r, t_out, grid_out)
        _same(r, direct, KEYS + FIM_KEYS, f"start {start} thin {thin}")
        assert r["n_fim_excluded"] == direct["n_fim_excluded"] == 0 and np.isfinite(r["fim_mean"]).all()
        if first is None:
            first = r
    # columns, relative and the statistics alone
    cols = [p.P + 1, 2]
    grid_out = np.arange(p.N, dtype=np.int32)
    r = e.sampler_sensitivities(I, grid_out, wrt=cols, relative=True)
    _same(r, _direct(e, p, w, r, I, grid_out, wrt=cols, relative=True), KEYS + FIM_KEYS, "columns, relative")
    bare = e.sampler_sensitivities(I, grid_out, return_draws=False)
    assert bare["sens"] is None and bare["fim"] is None
    _same(bare, first, ("sens_mean", "sens_sd", "status", "fim_mean"), "without draws")
    none = e.sampler_sensitivities(I, None)
    assert none["n_obs_used"] == 0 and "fim" not in none
    _same(none, first, KEYS, "no observations")
    some = np.where(np.arange(p.N) % 2 == 0, np.arange(p.N), -1).astype(np.int32)          # every second grid point
    r = e.sampler_sensitivities(I, some)
    _same(r, _direct(e, p, w, r, I, some), KEYS + FIM_KEYS, "every second grid point")
    # the call left no trace: the samples stand, an uninterrupted run of the same seed gives the same bits, and so does the log posterior
    np.testing.assert_array_equal(_bits(e.sampler_samples()[0]), _bits(X))
    e.sampler_run(_start(e, X0, s0, p.P, 2, seed=31))
    np.testing.assert_array_equal(_bits(e.sampler_samples()[0]), _bits(X))
    _same(e.sampler_sensitivities(I, np.arange(p.N, dtype=np.int32)), first, KEYS + FIM_KEYS, "after a second run")
    # rejected arguments
    for kw, text in ((dict(thin=0), "thin >= 1"), (dict(start_index=p.N), "start_index"), (dict(start_index=-1), "start_index"),
                     (dict(grid_out=np.full(p.N, len(I), dtype=np.int32)), "grid_out\\[0\\] is outside"), (dict(chains=range(1, 3)), "must lie inside"),
                     (dict(wrt=[0, 0]), "repeats"), (dict(substeps=0), "substeps")):
        args = {"t_out": I, "grid_out": None, **kw}
        with pytest.raises(MagiHipError, match=text) as ei:
            e.sampler_sensitivities(**args)
        assert ei.value.code == -1, text
    one = e.sampler_sensitivities(I, np.arange(p.N, dtype=np.int32), chains=range(1, 2))
    np.testing.assert_array_equal(_bits(one["sens"]), _bits(first["sens"][RUN["num_results"]:]))
    lp1 = e.logpost_grad(X0, s0, np.zeros(p.P))
    for a, b in zip(lp0, lp1):
        np.testing.assert_array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))
    fresh = engine_for(p, None)
    try:
        with pytest.raises(MagiHipError) as ei:               # no sampler yet
            fresh.sampler_sensitivities(I)
        assert ei.value.code == -5
    finally:
        fresh.close()


def test_group_member_sensitivities_equal_the_members_own_handle(sirw):
    """Two members with different weights: a member's range gives its own handle's bits; a range across two members is refused."""
    _, p, w, X0, s0 = sirw
    I = np.asarray(p.I, dtype=np.float64).reshape(-1)
    grid_out = np.arange(p.N, dtype=np.int32)
    engs = [engine_for(p, None), engine_for(p, None)]
    try:
        _model(engs[0], w)
        _model(engs[1], w[::-1].copy())
        Cn, seed = 2, 5
        grp = MagiGroup(engs)
        try:
            total = _start(grp, X0, s0, p.P, 2 * Cn, seed, ids=[0, 1, 0, 1])
            grp.sampler_run(total)
            grouped = [grp.sampler_sensitivities(I, grid_out, member=m, thin=2) for m in range(2)]
            for bad in (None, range(1, 3)):
                with pytest.raises(MagiHipError) as ei:
                    grp.sampler_sensitivities(I, grid_out, chains=bad)
                assert ei.value.code == -1 and "more than one member" in str(ei.value)
        finally:
            grp.close()
        for m in range(2):
            engs[m].sampler_run(_start(engs[m], X0, s0, p.P, Cn, seed, ids=[0, 1]))
            own = engs[m].sampler_sensitivities(I, grid_out, thin=2)
            _same(grouped[m], own, KEYS + FIM_KEYS + ("x0", "theta", "sigma_sq"), f"member {m}")
            np.testing.assert_array_equal(grouped[m]["obs_index"], own["obs_index"])
        assert not np.array_equal(grouped[0]["fim_mean"], grouped[1]["fim_mean"])
    finally:
        for e in engs:
            e.close()


# ---- the Python API ----------------------------------------------------------------------------------------------------------------------

def test_posterior_sensitivities_through_the_drop_in():
    """The vignette's SEIR-3 data, 20 + 20 transitions on two chains: the documented keys and shapes, names theta then x0, a finite
    sd_ratio, ``wrt``; the same bits after a predict that kept no samples; the engine's route on the same handle bit for bit."""
    import os
    import magi_v2
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g3_pipeline.npz"))
    model = magi_v2.MAGI_v2(D_thetas=3, ts_obs=g["seir3_ts_obs"], X_obs=g["seir3_X_obs"], bandsize=80, f_vec="seir3")
    try:
        model.initial_fit(discretization=1, hparam_iters=0)
        with pytest.raises(RuntimeError, match="run predict first"):
            model.posterior_sensitivities()
        model.predict(num_results=20, num_burnin_steps=20, seed=5, n_chains=2)
        I = np.asarray(model.I).reshape(-1)
        T, D, P = len(I), 3, 3
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # (a collinearity warning is the report's to give, not this test's subject)
            out = model.posterior_sensitivities()
            draws = model.posterior_sensitivities(return_draws=True, thin=2)
            th_only = model.posterior_sensitivities(wrt=("theta",))
            late = model.posterior_sensitivities(start_index=40, fisher=False)
            model.predict(num_results=20, num_burnin_steps=20, seed=5, n_chains=2, summary=True, keep_samples=False)
            again = model.posterior_sensitivities()
        assert {"t", "names", "sens", "fim_mean", "report", "status", "n_failed", "n_fim_excluded", "n_obs_used"} <= set(out)
        assert out["names"] == ["theta[0]", "theta[1]", "theta[2]", "x0[0]", "x0[1]", "x0[2]"]
        np.testing.assert_array_equal(out["t"], I)
        assert out["sens"]["mean"].shape == (T, D, P + D) == out["sens"]["sd"].shape and "draws" not in out["sens"]
        assert out["fim_mean"].shape == (P + D, P + D) and out["status"].shape == (40,) and out["n_failed"] == 0 and out["n_fim_excluded"] == 0
        assert out["n_obs_used"] == int(np.isfinite(g["seir3_X_obs"]).sum())
        rep = out["report"]
        assert rep["names"] == out["names"] and np.isfinite(rep["sd_ratio"]).all() and np.isfinite(rep["crlb_sd"]).all()
        assert draws["sens"]["draws"].shape == (20, T, D, P + D)
        assert th_only["names"] == out["names"][:P] and th_only["sens"]["mean"].shape == (T, D, P) and th_only["fim_mean"].shape == (P, P)
        np.testing.assert_array_equal(_bits(th_only["sens"]["mean"]), _bits(out["sens"]["mean"][..., :P]))
        np.testing.assert_array_equal(_bits(th_only["fim_mean"]), _bits(out["fim_mean"][:P, :P]))
        assert late["t"][0] == I[40] and late["sens"]["mean"].shape == (T - 40, D, P + D) and late["fim_mean"] is None and late["report"] is None
        np.testing.assert_array_equal(_bits(again["sens"]["mean"]), _bits(out["sens"]["mean"]))
        np.testing.assert_array_equal(_bits(again["fim_mean"]), _bits(out["fim_mean"]))
        eng = model.engine.sampler_sensitivities(I, np.arange(T, dtype=np.int32))
        np.testing.assert_array_equal(_bits(eng["sens_mean"]), _bits(out["sens"]["mean"]))
        want = SR.complex_step(R.callable_for("seir3"), eng["x0"], eng["theta"], I, 4)
        assert SR.bars(eng["sens"], want).max() <= 1.0
    finally:
        model.engine.close()
