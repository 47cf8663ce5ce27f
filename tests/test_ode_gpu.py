"""The device ODE solver (magi_ode_solve, csrc/ode.hip; MagiEngine.ode_solve, MAGI_v2.posterior_trajectories) against the CPU restatement
of its scheme (tests/ode_reference.py).

Bar: 1e-11 max|x| of the case.  tests/test_ode_cpu.py shows on the CPU that float64 and longdouble runs of the scheme differ by <= 1/100 of
it on every case used here and that every wrong scheme -- a k4 weight off by 1e-6, middle stages at the wrong time, a dropped sub-step,
Euler -- moves its case by >= 1000 bars.

Measured on an MI355X, worst |device - float64 reference| over S = 1 .. 257 and both grids, as a fraction of the bar (1 to 2 ulp of the
largest entry in most cases), substeps 4 / substeps 1:
    seir3 2.8e-05            sirw 4.1e-05             fhn 5.0e-04              lotka_volterra 2.2e-04 / 1.2e-04
    seir_seasonal 4.2e-05 / 4.2e-05                   chain8 2.0e-05 / 2.0e-05 sqrt_outflow 2.9e-05
    non-uniform grid (lotka_volterra, 65 draws) 1.0e-04; the drop-in's 20 and 40 SEIR-3 draws on 161 points 1.4e-05, 2.6e-05
Order ratios e(1)/e(2), e(2)/e(4) against longdouble with 64 sub-steps, device | float64 reference:
    lotka_volterra 15.9835, 15.9994 | 15.9835, 15.9994       seir_seasonal 18.3651, 17.2030 | 18.3651, 17.2030
mean / sd against numpy on the downloaded draws: <= 1.3e-02 of the summation-order bound."""
import os
import warnings

import numpy as np
import pytest

from magi_v2_amd import drift as drift_mod
from magi_v2_amd.engine import MagiEngine, MagiHipError
from tests import ode_reference as R
from tests.test_ode_cpu import order_errors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (1, 63, 64, 65, 129, 257)     # lane, wave and workgroup edges; with T D = 6 (seir3, T = 2) and 66 (sqrt_outflow's grid) also the transpose's tile edges


@pytest.fixture(scope="module")
def engines():
    """name -> (engine, what to pass as ``drift``): the base library for the compiled-in drifts, the traced drift's own library otherwise.
    One handle per library for the whole module."""
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


def solve(engines, name, x0, th, t, substeps=4, **kw):
    eng, d = engines(name)
    return eng.ode_solve(x0, th, t, substeps=substeps, drift=d, **kw)


def bars(got, want):
    """max |got - want| in bars of the case (1e-11 max|want|)."""
    return float(np.abs(got - want).max() / (R.BAR * np.abs(want).max()))


@pytest.mark.parametrize("drift,substeps", [(d, 4) for d in R.CASES] + [(d, 1) for d in R.SUBSTEPS_1_CASES])
def test_scheme_parity_at_the_lane_wave_and_workgroup_edges(engines, drift, substeps):
    """S = 1, 63, 64, 65, 129, 257 draws on T = 2 and on the case's grid: every draw finite and within the bar of the float64 reference."""
    case = R.CASES[drift]
    want, wstatus = R.reference(drift, substeps)
    assert (wstatus == 0).all()
    x0, th = R.draws(case)
    worst = 0.0
    for S in SIZES:
        for T in (2, len(case.t)):
            out = solve(engines, drift, x0[:S], th[:S], case.t[:T], substeps)
            assert out["trajectories"].shape == (S, T, case.D) and out["n_failed"] == 0 and (out["status"] == 0).all(), (S, T, out["status"])
            np.testing.assert_array_equal(out["trajectories"][:, 0], x0[:S])
            e = np.abs(out["trajectories"] - want[:S, :T]).max() / (R.BAR * np.abs(want).max())
            worst = max(worst, float(e))
    print(f"ode parity {drift} substeps={substeps}: worst {worst:.2e} of the bar")
    assert worst <= 1.0, (drift, substeps, worst)


def test_scheme_parity_on_a_non_uniform_grid(engines):
    case = R.CASES["lotka_volterra"]
    t = np.concatenate([[0.0], np.cumsum(0.05 + 0.4 * np.random.default_rng(3).uniform(size=24) ** 2)])
    x0, th = R.draws(case, 65)
    want, _ = R.rk4(R.callable_for("lotka_volterra"), x0, th, t, 4)
    out = solve(engines, "lotka_volterra", x0, th, t)
    e = bars(out["trajectories"], want)
    print(f"ode parity lotka_volterra, non-uniform grid of {len(t)} points, h {np.diff(t).min():.3f} .. {np.diff(t).max():.3f}: {e:.2e} of the bar")
    assert (out["status"] == 0).all() and e <= 1.0


@pytest.mark.parametrize("drift", ("lotka_volterra", "seir_seasonal"))
def test_order_ratios_equal_the_reference_ratios(engines, drift):
    """Errors against longdouble with 64 sub-steps at 1, 2, 4 sub-steps: the device's two successive ratios are the float64 reference's
    within 1 % of each (the reference's, not 16: the leading error term is not alone at these steps)."""
    S = 9
    case = R.CASES[drift]
    x0, th = R.draws(case, S)
    _, want = order_errors(drift, lambda s: R.reference(drift, s, "float64", S)[0], S)
    _, got = order_errors(drift, lambda s: solve(engines, drift, x0, th, case.t, s)["trajectories"], S)
    print(f"ode order {drift}: device ratios {got[0]:.4f}, {got[1]:.4f}; float64 reference {want[0]:.4f}, {want[1]:.4f}")
    for g, w in zip(got, want):
        assert abs(g / w - 1.0) <= 0.01, (drift, got, want)


@pytest.mark.parametrize("drift", ("seir_seasonal", "chain8"))
def test_a_draw_has_the_same_bits_alone_and_in_any_batch_and_calls_repeat(engines, drift):
    case = R.CASES[drift]
    x0, th = R.draws(case)
    runs = {S: solve(engines, drift, x0[:S], th[:S], case.t) for S in (65, 257)}
    for s in (0, 37, 63, 64):
        alone = solve(engines, drift, x0[s:s + 1], th[s:s + 1], case.t)["trajectories"][0]
        for S, out in runs.items():
            np.testing.assert_array_equal(out["trajectories"][s], alone, err_msg=f"draw {s} in a batch of {S}")
    again = solve(engines, drift, x0, th, case.t)
    for key in ("trajectories", "mean", "sd", "status"):
        np.testing.assert_array_equal(again[key], runs[257][key], err_msg=key)
    assert np.isfinite(again["mean"]).all() and np.isfinite(again["sd"]).all()


def test_status_marks_the_draws_that_leave_the_domain_and_spares_the_others(engines):
    """The five sqrt_outflow draws of the CPU test in one batch: status (16, 18, 13, 23, 0), the survivor within the bar and alone in the
    mean; sd needs two."""
    x0, th = R.status_inputs()
    want, wstatus = R.rk4(R.callable_for("sqrt_outflow"), x0, th, R.STATUS_T, R.STATUS_SUBSTEPS)
    assert tuple(wstatus) == R.STATUS_WANT
    out = solve(engines, "sqrt_outflow", x0, th, R.STATUS_T, R.STATUS_SUBSTEPS)
    assert tuple(out["status"]) == R.STATUS_WANT and out["n_failed"] == 4
    e = bars(out["trajectories"][4], want[4])
    print(f"ode status case: surviving draw {e:.2e} of the bar")
    assert e <= 1.0
    for s, st in enumerate(R.STATUS_WANT[:4]):          # finite up to the exit, not after it; the stored values are the arithmetic's
        assert np.isfinite(out["trajectories"][s, :st]).all() and not np.isfinite(out["trajectories"][s, st]).all()
        assert bars(out["trajectories"][s, :st], want[s, :st]) <= 1.0
    np.testing.assert_array_equal(out["mean"], out["trajectories"][4])
    assert np.isnan(out["sd"]).all()
    x0b, thb = R.status_inputs(True)
    two = solve(engines, "sqrt_outflow", x0b, thb, R.STATUS_T, R.STATUS_SUBSTEPS)
    assert tuple(two["status"]) == R.STATUS_WANT + (0,) and two["n_failed"] == 4
    assert np.isfinite(two["mean"]).all() and np.isfinite(two["sd"]).all() and (two["sd"][1:] > 0).all()
    np.testing.assert_array_equal(two["trajectories"][:5], out["trajectories"])
    none = solve(engines, "sqrt_outflow", x0[:4], th[:4], R.STATUS_T, R.STATUS_SUBSTEPS)          # no draw qualifies
    assert none["n_failed"] == 4 and np.isnan(none["mean"]).all() and np.isnan(none["sd"]).all()


def test_posterior_trajectories_warns_about_failed_draws():
    import magi_v2
    from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES
    x0, th = R.status_inputs()
    model = magi_v2.MAGI_v2(D_thetas=3, ts_obs=R.STATUS_T, X_obs=np.zeros((len(R.STATUS_T), 2)), bandsize=None, f_vec=DOMAIN_EXAMPLES["sqrt_outflow"][0])
    res = {"I": R.STATUS_T.reshape(-1, 1), "X_samps": np.repeat(x0[:, None, :], len(R.STATUS_T), axis=1), "thetas_samps": th}
    try:
        with pytest.warns(UserWarning, match="4 of 5 trajectories") as rec:
            out = model.posterior_trajectories(res, substeps=R.STATUS_SUBSTEPS)
        assert len(rec) == 1
        assert tuple(out["status"]) == R.STATUS_WANT and out["n_failed"] == 4
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            model.posterior_trajectories({**res, "X_samps": res["X_samps"][4:], "thetas_samps": th[4:]}, substeps=R.STATUS_SUBSTEPS)
    finally:
        model.engine.close()


@pytest.mark.parametrize("drift,S", [("chain8", 257), ("sirw", 65), ("sqrt_outflow", 6)])
def test_mean_and_sd_are_numpy_on_the_downloaded_draws(engines, drift, S):
    """Against numpy (ddof = 1) on the device's own trajectories restricted to status 0, within the summation-order bound
    4 S 2^-53 max|trajectory|; without the draws the same bits."""
    if drift == "sqrt_outflow":
        (x0, th), t, sub = R.status_inputs(True), R.STATUS_T, R.STATUS_SUBSTEPS
    else:
        case = R.CASES[drift]
        (x0, th), t, sub = R.draws(case, S), case.t, 4
    out = solve(engines, drift, x0, th, t, sub)
    ok = out["status"] == 0
    tr = out["trajectories"][ok]
    bound = 4.0 * S * 2.0 ** -53 * np.abs(tr).max()
    em, es = np.abs(out["mean"] - tr.mean(axis=0)).max(), np.abs(out["sd"] - tr.std(axis=0, ddof=1)).max()
    print(f"ode stats {drift} S={S} ({int(ok.sum())} finite): mean {em / bound:.2e}, sd {es / bound:.2e} of the summation-order bound")
    assert em <= bound and es <= bound
    bare = solve(engines, drift, x0, th, t, sub, return_draws=False)
    assert bare["trajectories"] is None
    for key in ("mean", "sd", "status"):
        np.testing.assert_array_equal(bare[key], out[key], err_msg=key)
    assert bare["n_failed"] == out["n_failed"]


@pytest.fixture(scope="module")
def fitted():
    import magi_v2
    g = np.load(os.path.join(GOLDEN, "g3_pipeline.npz"))
    model = magi_v2.MAGI_v2(D_thetas=3, ts_obs=g["seir3_ts_obs"], X_obs=g["seir3_X_obs"], bandsize=80, f_vec="seir3")
    model.initial_fit(discretization=1, hparam_iters=0)
    yield model
    model.engine.close()


@pytest.mark.parametrize("n_chains", (1, 2))
def test_posterior_trajectories_through_the_drop_in(fitted, n_chains):
    """The vignette's SEIR-3 data (81 rows, 161 grid points), 20 + 20 transitions: the method is engine.ode_solve on the same samples to the
    bit and the CPU reference within the bar; thinning and a forecasting grid leave the shared draws and outputs to the bit."""
    model = fitted
    res = model.predict(num_results=20, num_burnin_steps=20, seed=5, n_chains=n_chains)
    I = res["I"].reshape(-1)
    T, D = len(I), 3
    lead = (20,) if n_chains == 1 else (2, 20)
    out = model.posterior_trajectories(res)
    assert out["trajectories"].shape == lead + (T, D) and out["status"].shape == lead and out["mean"].shape == (T, D) == out["sd"].shape
    np.testing.assert_array_equal(out["t"], I)
    assert out["n_failed"] == 0 and (out["status"] == 0).all()
    x0, th = res["X_samps"][..., 0, :].reshape(-1, D), res["thetas_samps"].reshape(-1, 3)
    direct = model.engine.ode_solve(x0, th, I, drift="seir3")
    np.testing.assert_array_equal(out["trajectories"].reshape(-1, T, D), direct["trajectories"])
    for key in ("mean", "sd"):
        np.testing.assert_array_equal(out[key], direct[key], err_msg=key)
    want, _ = R.rk4(R.callable_for("seir3"), x0, th, I, 4)
    e = bars(direct["trajectories"], want)
    print(f"ode drop-in n_chains={n_chains}: {e:.2e} of the bar")
    assert e <= 1.0
    # thin = 2: every second draw of every chain
    thin = model.posterior_trajectories(res, thin=2)
    assert thin["trajectories"].shape == lead[:-1] + (10, T, D)
    np.testing.assert_array_equal(thin["trajectories"], out["trajectories"][..., ::2, :, :])
    # a later start, without the draws
    late = model.posterior_trajectories(res, start_index=40, substeps=2, return_draws=False)
    assert late["trajectories"] is None and late["mean"].shape == (T - 40, D) and late["t"][0] == I[40]
    # forecasting: 25 % past I[-1]
    dt = I[1] - I[0]
    grid = np.concatenate([I, I[-1] + dt * np.arange(1, (T - 1) // 4 + 1)])
    fc = model.posterior_trajectories(res, t_out=grid)
    assert fc["trajectories"].shape == lead + (len(grid), D) and np.isfinite(fc["trajectories"]).all()
    np.testing.assert_array_equal(fc["trajectories"][..., :T, :], out["trajectories"])
    np.testing.assert_array_equal(fc["mean"][:T], out["mean"])
    with pytest.raises(AssertionError, match="start at"):
        model.posterior_trajectories(res, t_out=grid[1:])


def test_rejected_arguments_raise_and_leave_the_handle_usable(engines):
    """Every check is made on the host before anything is allocated or launched."""
    eng, _ = engines("seir3")
    case = R.CASES["seir3"]
    x0, th = R.draws(case, 5)
    t = case.t
    ok = lambda **kw: eng.ode_solve(kw.get("x0", x0), kw.get("th", th), kw.get("t", t), substeps=kw.get("substeps", 4), drift=kw.get("drift", "seir3"))
    big = (1 << 20) + 1
    bad = [("S <= 2\\^20", dict(x0=np.empty((0, 3)), th=np.empty((0, 3)))),
           ("S <= 2\\^20", dict(x0=np.zeros((big, 3)), th=np.zeros((big, 3)))),
           ("T <= 2\\^16", dict(t=t[:1])),
           ("T <= 2\\^16", dict(t=np.arange((1 << 16) + 1.0))),
           ("substeps <= 1024", dict(substeps=0)),
           ("substeps <= 1024", dict(substeps=1025)),
           ("exceeds 2\\^28", dict(x0=np.zeros((1 << 14, 3)), th=np.zeros((1 << 14, 3)), t=np.arange(float(1 << 16)))),
           ("drift expects P=3", dict(th=np.ones((5, 4)))),
           ("drift expects P=5", dict(drift="sirw", x0=np.ones((5, 4)))),
           ("not strictly increasing at index 3", dict(t=np.array([0.0, 0.1, 0.2, 0.2, 0.3]))),
           ("not strictly increasing at index 1", dict(t=t[::-1])),
           ("t_out\\[2\\] is not finite", dict(t=np.array([0.0, 0.1, np.nan, 0.3]))),
           ("t_out\\[1\\] is not finite", dict(t=np.array([0.0, np.inf])))]
    for msg, kw in bad:
        with pytest.raises(MagiHipError, match=msg) as e:
            ok(**kw)
        assert e.value.code == -1, msg
    from magi_v2_amd.engine import _ptr
    for k in range(3):                                   # a null x0, theta or t_out
        ptrs = [_ptr(x0), _ptr(th), _ptr(t)]
        ptrs[k] = None
        with pytest.raises(MagiHipError, match="null pointer"):
            eng._check(eng._lib.magi_ode_solve(eng._h, 0, 3, 5, ptrs[0], ptrs[1], len(t), ptrs[2], 4, None, None, None, None, None))
    with pytest.raises(MagiHipError, match="unknown drift id"):
        eng._check(eng._lib.magi_ode_solve(eng._h, 3, 3, 5, _ptr(x0), _ptr(th), len(t), _ptr(t), 4, None, None, None, None, None))
    # every output pointer is optional
    eng._check(eng._lib.magi_ode_solve(eng._h, 0, 3, 5, _ptr(x0), _ptr(th), len(t), _ptr(t), 4, None, None, None, None, None))
    out = ok()
    assert bars(out["trajectories"], R.reference("seir3", 4)[0][:5]) <= 1.0 and out["n_failed"] == 0
