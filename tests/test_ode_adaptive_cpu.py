"""The conditions tests/test_ode_adaptive_gpu.py rests on, shown on the CPU with the numpy restatement of the error-controlled integrators
(tests/ode_adaptive_reference.py):

1. truth       the float64 reference against scipy (Radau with the analytic Jacobian on the stiff cases, DOP853 on the others; rtol 1e-12,
               atol 1e-14) is finite on every draw.  Worst |reference - truth| / (atol + rtol |truth|) over the first TRUTH_DRAWS draws:
                   robertson ros23 1e-4: 0.11, 1e-6: 0.65     van_der_pol dopri5 1e-9: 2.1, ros23 1e-4: 240     forced_relaxation ros23 1e-6: 0.67
                   seir3 0.55 / 170   sirw 0.34 / 69   lotka_volterra 1.8 / 240   seir_seasonal 0.39 / 130   chain8 0.0031 / 16   logistic1 0.28 / 43
                   (dopri5 / ros23 at 1e-6: the order-2 pair controls its local error, its global error on a non-stiff problem is one to two
                   hundred tolerances -- ros23 is for the stiff draws)
2. no knife    float64 and longdouble take the same decision at every trial step of every draw of every run, and every trial step has
               |errn - 1| >= 1000 times its own float64-versus-longdouble difference in errn: a perturbation a thousand times the rounding of
               float64 flips no decision.  (Trial by trial, not the least |errn - 1| of a run against the largest difference of the run:
               that largest difference belongs to the rejected first steps, whose errn is 1e6 to 1e8 and differs by 2.0 (robertson 1e-4) or
               224 (1e-6) in absolute terms -- no tolerance or seed brings it under 1e-3 of anything, and it says nothing about a decision
               at errn = 1.  Both figures are printed.)
               Van der Pol under DOPRI5 runs at rtol 1e-9 on the draws of seed 985, not at 1e-6 on seed 0: ode_adaptive_reference.RUN_SEEDS
               says why (least ratio there 1.27e3).
3. variants    every wrong variant changes a step count or moves the trajectories by > 1000 device bars on at least one run.
4. need        classical RK4 with 1024 sub-steps per interval -- the most magi_ode_solve takes -- is non-finite on Robertson.
5. df/dt       the emitted time derivative of the time-dependent examples is a longdouble central difference of the callable."""
import numpy as np
import pytest

from magi_v2_amd import drift as drift_mod
from magi_v2_amd.drift_examples import EXAMPLES, STIFF_EXAMPLES, TIME_EXAMPLES
from tests import ode_adaptive_reference as R
from tests import ode_reference as R0

TRUTH_DRAWS = 3


def _truth(name, x0, th, t_out, stiff):
    from scipy.integrate import solve_ivp
    m = R.model(name)
    one = lambda a: np.asarray(a, dtype=np.float64)[None]
    f = lambda t, y: m.f(one(t), one(y), one(th))[0]
    jac = lambda t, y: m.jac(one(t), one(y), one(th))[0]
    kw = dict(method="Radau", jac=jac) if stiff else dict(method="DOP853")
    sol = solve_ivp(f, (t_out[0], t_out[-1]), x0, t_eval=t_out, rtol=1e-12, atol=1e-14, **kw)
    assert sol.success, (name, sol.message)
    return sol.y.T


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_the_reference_is_finite_on_every_draw_and_near_the_truth(run):
    name, method, rtol = run
    case = R.CASES[name]
    ref = R.reference(name, method, rtol)
    assert (ref["reason"] == 0).all() and (ref["status"] == 0).all() and np.isfinite(ref["trajectories"]).all()
    x0, th = R.run_draws(run, TRUTH_DRAWS)
    worst = 0.0
    for s in range(TRUTH_DRAWS):
        truth = _truth(name, x0[s], th[s], case.t, stiff=run in R.STIFF_RUNS)
        worst = max(worst, float((np.abs(ref["trajectories"][s] - truth) / (R.ATOL + rtol * np.abs(truth))).max()))
    print(f"ode adaptive truth {R.run_id(run)}: {worst:.2g} of atol + rtol |x|; steps of draw 0: {ref['n_accepted'][0]} + {ref['n_rejected'][0]}")
    assert np.isfinite(worst)


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_no_decision_sits_on_a_knife_edge(run):
    name, method, rtol = run
    a, b = R.reference(name, method, rtol, "float64", R.BATCH, None, True), R.reference(name, method, rtol, "longdouble", R.BATCH, None, True)
    for key in ("n_accepted", "n_rejected", "reason", "status"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert len(a["record"]) == len(b["record"])
    edge, diff, near, ratio = np.inf, 0.0, 0.0, np.inf
    for (sa, ea, oka), (sb, eb, okb) in zip(a["record"], b["record"]):
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(oka, okb)
        np.testing.assert_array_equal(ea[oka] <= 1, eb[okb] <= 1)
        if oka.any():
            e, d = ea[oka], np.abs(ea[oka] - eb[okb]).astype(np.float64)
            edge, diff = min(edge, float(np.abs(e - 1).min())), max(diff, float(d.max()))
            near = max(near, float(d[e < 2].max(initial=0.0)))
            with np.errstate(divide="ignore"):
                ratio = min(ratio, float((np.abs(e - 1) / d).min()))
    dist = R0.distance(a["trajectories"], b["trajectories"])
    print(f"ode adaptive knife edge {R.run_id(run)}: min |errn - 1| {edge:.2e}; float64 vs longdouble errn: {diff:.2e} over all trials, {near:.2e} over "
          f"those with errn < 2; least |errn - 1| / difference of one trial {ratio:.3g}; trajectories {dist:.2e} (bar {R.bar(name, method, rtol):.2e})")
    assert ratio >= 1000.0, (ratio, edge, diff)


# (case, method, rtol, draws): small batches, and the whole batch where a variant shows on a few draws only (e32 off by 1e-6 moves a step
# count of one draw in 257 of van_der_pol and nothing else by a thousand bars)
VARIANT_RUNS = (("forced_relaxation", "ros23", 1e-6, 5), ("robertson", "ros23", 1e-4, 5), ("lotka_volterra", "dopri5", 1e-6, 5),
                ("van_der_pol", "dopri5", 1e-9, 5), ("seir_seasonal", "ros23", 1e-6, 5), ("van_der_pol", "ros23", 1e-4, R.BATCH))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_shows(variant):
    shown = []
    for name, method, rtol, S in VARIANT_RUNS:
        good, bad = R.reference(name, method, rtol, "float64", S), R.reference(name, method, rtol, "float64", S, variant)
        counts = any((good[k] != bad[k]).any() for k in ("n_accepted", "n_rejected", "reason", "status"))
        with np.errstate(invalid="ignore"):
            move = np.nan_to_num(np.abs(bad["trajectories"] - good["trajectories"]), nan=np.inf).max() / np.abs(good["trajectories"]).max()
        if counts or move > 1000.0 * R.bar(name, method, rtol):
            shown.append((name, method, counts, float(move / R.bar(name, method, rtol))))
    print(f"ode adaptive variant {variant}: shows on {shown}")
    assert shown, variant


def test_rk4_at_the_most_substeps_is_non_finite_on_robertson():
    case = R.CASES["robertson"]
    m = R.model("robertson")
    f = lambda s, y, th: m.f(np.full(y.shape[0], s, dtype=y.dtype), y, th)
    for substeps in (4, 64, 1024):
        traj, status = R0.rk4(f, case.x0[None], case.theta[None], case.t, substeps)
        assert status[0] != 0 and not np.isfinite(traj).all(), substeps
    ref = R.reference("robertson", "ros23", 1e-4)
    assert ref["status"][0] == 0 and ref["n_accepted"][0] + ref["n_rejected"][0] < 1024


@pytest.mark.parametrize("name", sorted(TIME_EXAMPLES) + ["forced_relaxation"])
def test_emitted_time_derivative_is_a_central_difference_of_the_callable(name):
    """Step 1e-5 in longdouble: truncation h^2 / 6 |f'''| <= 2e-10 |df/dt| for these forcings (frequencies <= pi), rounding 1e-14 |f|."""
    f_vec, D, P = {**TIME_EXAMPLES, **STIFF_EXAMPLES}[name]
    d = drift_mod.resolve(f_vec, D, P)
    assert d.time_dependent and "user_drift_ft" in d.header and "void ft(" in d.header
    rng = np.random.default_rng(11)
    n = 16
    X, th, t = rng.uniform(0.1, 0.9, (n, D)), rng.uniform(0.3, 1.7, P), rng.uniform(0.0, 5.0, n)
    got = d.ft_np(t, X, th)
    ld = np.longdouble
    h = ld(1e-5)
    call = lambda tt: np.asarray(f_vec(tt[:, None], X.astype(ld), th.astype(ld)), dtype=ld)
    want = (call(t.astype(ld) + h) - call(t.astype(ld) - h)) / (2 * h)
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"ode adaptive df/dt {name}: {e:.2e} of max |df/dt|")
    assert np.abs(want).max() > 0 and e <= 1e-8


def test_a_drift_without_t_carries_no_time_derivative():
    d = drift_mod.resolve(*EXAMPLES["lotka_volterra"])
    assert not d.time_dependent and d.ft_np is None and "ft(" not in d.header
    assert all("ft(" not in drift_mod.resolve(*STIFF_EXAMPLES[k]).header for k in ("robertson", "van_der_pol"))
