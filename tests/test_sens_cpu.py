"""The conditions the device bars of tests/test_sens_gpu.py rest on, shown on the CPU truths alone (tests/sens_reference.py), the pure-numpy
``host.fisher_report``, and the build facts of the new unit.  No library call is made.

The device differs from the float64 run of the variational scheme by FMA contraction, the order of a row's dot product and a few ulp in
the transcendentals: the same kind of difference as float64 against longdouble.  The bar, 1e-11 of a column's max |sens|, must sit >= 100 x
above that rounding distance -- and above the distance between the two independent truths -- and >= 1000 x below the shift of every
fault it is meant to catch."""
import os
import warnings

import numpy as np
import pytest

from magi_v2_amd import host
from tests import ode_reference as R
from tests import sens_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = [(d, 4) for d in R.CASES] + [(d, 1) for d in R.SUBSTEPS_1_CASES]
S_VAR = 9            # draws per case for the wrong variants (the nominal one and eight perturbed): the shifts are per draw


@pytest.mark.parametrize("drift,substeps", PARITY)
def test_the_two_truths_and_both_precisions_agree_within_a_hundredth_of_the_bar(drift, substeps):
    """The full 257-draw batch: (b) in float64 against (b) in longdouble, (a) against (b) in longdouble, and the float64 complex step the
    GPU test compares with against (b) in longdouble."""
    b64, bld = SR.reference(drift, substeps, "augmented", "float64"), SR.reference(drift, substeps, "augmented", "longdouble")
    a64, ald = SR.reference(drift, substeps, "complex", "float64"), SR.reference(drift, substeps, "complex", "longdouble")
    assert np.isfinite(b64).all() and np.isfinite(a64).all()
    gaps = {"float64 vs longdouble (b)": SR.bars(b64, bld).max(), "(a) vs (b), longdouble": SR.bars(ald, bld).max(),
            "(a) float64 vs (b) longdouble": SR.bars(a64, bld).max()}
    print(f"{drift} substeps={substeps}: " + ", ".join(f"{k} {v:.1e} bars" for k, v in gaps.items()))
    for k, v in gaps.items():
        assert v <= 0.01, (drift, substeps, k, v)


@pytest.mark.parametrize("drift", sorted(R.CASES))
def test_every_case_has_a_jacobian_that_is_not_symmetric(drift):
    """So that J_x^T in place of J_x is a different scheme on every case."""
    case = R.CASES[drift]
    J, _ = SR.jacobians(drift)(0.3, case.x0[None], case.theta[None])
    assert np.abs(J[0] - J[0].T).max() >= 1e-3 * np.abs(J[0]).max(), J[0]


@pytest.mark.parametrize("variant", SR.VARIANTS)
@pytest.mark.parametrize("drift", sorted(R.CASES))
def test_every_wrong_scheme_moves_a_column_by_a_thousand_bars(drift, variant):
    """The df/dtheta term missing at the last stage, J_x^T, stage sensitivities built with a stale increment, and -- for the
    time-dependent case -- the middle stages' Jacobians taken at time s."""
    right = SR.reference(drift, 4, "augmented", "float64", S_VAR)
    wrong = SR.reference(drift, 4, "augmented", "float64", S_VAR, variant)
    if variant == "mid_jac_time_at_s" and not R.CASES[drift].time_dependent:
        np.testing.assert_array_equal(wrong, right)             # an autonomous Jacobian never reads the time: the variant IS the scheme
        return
    shift = SR.bars(wrong, right)
    print(f"{drift} {variant}: worst column {shift.max():.1e} bars, least {shift.min():.1e}")
    assert shift.max() >= 1e3, (drift, variant, shift)
    if variant == "dtheta_missing_last":                        # the x0 columns have no such term
        np.testing.assert_array_equal(wrong[..., R.CASES[drift].P:], right[..., R.CASES[drift].P:])


def test_the_jacobians_of_truth_b_are_those_of_jac_np():
    for drift in ("sirw", "seir_seasonal", "sqrt_outflow"):
        case = R.CASES[drift]
        d = SR.drift_for(drift)
        X = np.tile(case.x0, (3, 1)) * np.array([[1.0], [1.1], [0.9]])
        J, Tm = SR.jacobians(drift)(0.7, X, np.tile(case.theta, (3, 1)))
        Jw, Tw = d.jac_np(X, case.theta, np.full(3, 0.7) if case.time_dependent else None)
        np.testing.assert_allclose(J, Jw, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(Tm, Tw, rtol=1e-14, atol=1e-15)


def _fisher_inputs():
    fs = SR.fisher_setup()
    sens, traj = SR.augmented(SR.FIM_CASE, fs["x0"], fs["theta"], fs["t"], 4)
    o = fs["obs"]
    return sens, traj, (o["j"], o["comp"], o["weight"], o["sigma_sq"], o["link"])


def test_fisher_restatement_against_longdouble_and_its_wrong_variants():
    """The float64 restatement in the stated order is within 1/100 of the bar of the longdouble one on the same inputs; g' dropped, sigma in
    place of sigma^2 and the weights dropped each move an entry by >= 1000 bars."""
    sens, traj, obs = _fisher_inputs()
    n_obs = len(obs[0])
    assert n_obs == 164
    F, Fl = SR.fisher(sens, traj, *obs), SR.fisher(sens, traj, *obs, dtype=np.longdouble)
    bar = SR.fisher_bar(Fl, n_obs)
    assert np.isfinite(F).all() and (bar > 0).all()
    gap = float((np.abs(F - Fl) / bar).max())
    print(f"fisher float64 vs longdouble: {gap:.1e} bars")
    assert gap <= 0.01
    np.testing.assert_array_equal(F, F.transpose(0, 2, 1))
    for v in SR.FIM_VARIANTS:
        shift = float((np.abs(SR.fisher(sens, traj, *obs, variant=v) - F) / bar).max())
        print(f"fisher {v}: {shift:.1e} bars")
        assert shift >= 1e3, (v, shift)


def test_fisher_report_on_a_diagonal_matrix():
    F = np.diag([4.0, 25.0, 0.01])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep = host.fisher_report(F, ["a", "b", "c"], post_sd=[0.25, 0.2, 20.0])
    np.testing.assert_allclose(rep["crlb_sd"], 1.0 / np.sqrt(np.diag(F)), rtol=1e-15)
    assert rep["collinearity_index"] == pytest.approx(1.0, abs=1e-12) and rep["positive_definite"]
    np.testing.assert_allclose(rep["eigenvalues"], [0.01, 4.0, 25.0], rtol=1e-15)
    assert rep["condition_number"] == pytest.approx(2500.0)
    assert rep["weakest_direction"][0] == ("c", 1.0)
    np.testing.assert_allclose(rep["sd_ratio"], [0.5, 1.0, 2.0], rtol=1e-14)
    np.testing.assert_allclose(rep["eigenvectors"] @ np.diag(rep["eigenvalues"]) @ rep["eigenvectors"].T, F, atol=1e-13)


def test_fisher_report_on_an_exactly_collinear_pair():
    """Sensitivity columns u, 2 u and an independent w: F has the null direction (2, -1, 0) / sqrt 5."""
    rng = np.random.default_rng(4)
    u, w = rng.normal(size=50), rng.normal(size=50)
    A = np.stack([u, 2.0 * u, w], axis=1)
    F = A.T @ A
    with pytest.warns(UserWarning, match="collinearity index") as rec:
        rep = host.fisher_report(F, ["beta", "gamma", "x0[1]"], post_sd=np.ones(3))
    assert len(rec) == 1 and "beta" in str(rec[0].message) and "gamma" in str(rec[0].message) and "x0[1]" not in str(rec[0].message)
    assert rep["collinearity_index"] > 15.0 and not rep["positive_definite"]
    assert np.isnan(rep["crlb_sd"]).all() and np.isnan(rep["sd_ratio"]).all()
    lead = dict(rep["weakest_direction"])
    assert [n for n, _ in rep["weakest_direction"]][:2] == ["beta", "gamma"]
    np.testing.assert_allclose([lead["beta"], lead["gamma"], lead["x0[1]"]], np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0), atol=1e-7)
    # nearly collinear but well conditioned enough to invert: a finite bound, and a warning only past the threshold
    F2 = F + np.diag([0.0, 1e-3 * F[1, 1], 0.0])
    with pytest.warns(UserWarning, match="collinearity index"):
        rep2 = host.fisher_report(F2, ["beta", "gamma", "x0[1]"])
    assert np.isfinite(rep2["crlb_sd"]).all() and 15.0 < rep2["collinearity_index"] < 1e3 and rep2["sd_ratio"] is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host.fisher_report(F2, ["beta", "gamma", "x0[1]"], collinearity_warn=1e3)
        nan = host.fisher_report(np.full((2, 2), np.nan), ["a", "b"])
    assert np.isnan(nan["crlb_sd"]).all() and np.isnan(nan["collinearity_index"])
    with pytest.raises(ValueError):
        host.fisher_report(F, ["a", "b"])


def test_the_unit_is_built_per_drift_and_its_symbols_are_bound():
    from magi_v2_amd import build, engine, jit
    assert os.path.join(build.CSRC, "sens.hip") in build.sources() and "sens.hip" not in jit._DRIFT_FREE
    for sym, n_args in (("magi_ode_sensitivities", 27), ("magi_sampler_sensitivities", 26)):
        assert sym in engine.exported_symbols() and len(engine._SYMBOLS[sym][1]) == n_args
    with open(os.path.join(ROOT, "include", "magi_hip.h")) as fh:
        text = fh.read()
    assert "int magi_ode_sensitivities(" in text and "int magi_sampler_sensitivities(" in text
