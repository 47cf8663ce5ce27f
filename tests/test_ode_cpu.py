"""The conditions the device bar of tests/test_ode_gpu.py rests on, shown on the CPU reference alone (tests/ode_reference.py), and the
build facts of the new unit.  No library call is made.

The device differs from the float64 numpy run of the same scheme by FMA contraction and a few ulp in the transcendentals: the same kind of
difference as float64 against longdouble.  The bar, 1e-11 max|x| of the case, must sit >= 100 x above that rounding distance and >= 1000 x
below the shift of every fault it is meant to catch."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import ode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_CPU = 9            # draws per case here (the nominal one and eight perturbed): the conditions are per draw


def _ref(drift, substeps, dtype="float64", variant=None):
    return R.reference(drift, substeps, dtype, S_CPU, variant)[0]


PARITY = [(d, 4) for d in R.CASES] + [(d, 1) for d in R.SUBSTEPS_1_CASES]


@pytest.mark.parametrize("drift,substeps", PARITY)
def test_float64_is_within_a_hundredth_of_the_bar_of_longdouble(drift, substeps):
    d = R.distance(_ref(drift, substeps), _ref(drift, substeps, "longdouble"))
    print(f"{drift} substeps={substeps}: float64 vs longdouble {d:.2e} of max|x| = {d / R.BAR:.1e} bars")
    assert np.isfinite(_ref(drift, substeps)).all()
    assert d <= R.BAR / 100.0, (drift, substeps, d)


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("drift", sorted(R.CASES))
def test_every_wrong_scheme_moves_its_case_by_a_thousand_bars(drift, variant):
    """A k4 weight off by 1e-6, the middle stages' time taken at s (time-dependent case), a dropped last sub-step, Euler."""
    if variant == "mid_time_at_s" and not R.CASES[drift].time_dependent:
        # an autonomous drift never reads the time: the variant IS the scheme, and must be bit-equal to it
        np.testing.assert_array_equal(_ref(drift, 4, variant=variant), _ref(drift, 4))
        return
    shift = R.distance(_ref(drift, 4, variant=variant), _ref(drift, 4))
    print(f"{drift} {variant}: shift {shift:.2e} of max|x| = {shift / R.BAR:.1e} bars")
    assert shift >= 1e3 * R.BAR, (drift, variant, shift)


@pytest.mark.parametrize("drift", ("lotka_volterra", "seir_seasonal"))
def test_order_ratios_are_measurable_within_a_percent(drift):
    """Errors against longdouble with 64 sub-steps at 1, 2, 4 sub-steps: the smallest is >= 1000 bars, so a device within the bar has the
    reference's two ratios within 2e-3 of each (the GPU test asks 1 %)."""
    e, ratios = order_errors(drift, lambda s: _ref(drift, s))
    print(f"{drift}: errors {e}, ratios {ratios}")
    assert min(e) >= 1e3 * R.BAR
    assert all(10.0 < r < 25.0 for r in ratios)


def order_errors(drift, run, S=S_CPU):
    truth = R.reference(drift, 64, "longdouble", S)[0]
    e = [R.distance(run(s), truth) for s in (1, 2, 4)]
    return e, (e[0] / e[1], e[1] / e[2])


@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_status_case_leaves_the_domain_where_stated_and_far_from_its_edge(dtype):
    """sqrt_outflow from (0.25, 0.1) with theta = (a, 0.5, 0.3), 33 points on [0, 2], two sub-steps: a = 1.0, 0.9, 1.3, 0.7, 0.2 give
    status 16, 18, 13, 23, 0 in both precisions, and every argument a sqrt sees at a finite stage is >= 1e-6 from 0 -- no draw's exit
    hangs on rounding."""
    x0, th = R.status_inputs()
    seen = []
    traj, status = R.rk4(R.callable_for("sqrt_outflow"), x0, th, R.STATUS_T, R.STATUS_SUBSTEPS, dtype=dtype, on_stage=lambda y: seen.append(np.array(y[:, 0], dtype=np.float64)))
    assert tuple(status) == R.STATUS_WANT
    args = np.concatenate(seen)
    margin = np.abs(args[np.isfinite(args)]).min()
    print(f"{np.dtype(dtype).name}: status {tuple(status)}, smallest |argument of sqrt| {margin:.2e}")
    assert margin >= 1e-6
    for k, st in enumerate(R.STATUS_WANT[:4]):          # the status is the index of the first non-finite output
        assert np.isfinite(traj[k, :st]).all() and not np.isfinite(traj[k, st]).all()
    assert np.isfinite(traj[4]).all()
    # a second survivor for the sd of the GPU test
    _, s2 = R.rk4(R.callable_for("sqrt_outflow"), *R.status_inputs(True), R.STATUS_T, R.STATUS_SUBSTEPS, dtype=dtype)
    assert tuple(s2) == R.STATUS_WANT + (0,)


def test_reference_restates_the_package_host_loop():
    """ode_reference.rk4 in float64 is drift_examples.rk4 to the bit on a non-uniform grid, time-dependent drift included."""
    from magi_v2_amd.drift_examples import TIME_EXAMPLES, rk4
    case = R.CASES["seir_seasonal"]
    grid = np.array([0.0, 0.1, 0.25, 0.3, 0.7, 1.0])
    _, want = rk4(TIME_EXAMPLES["seir_seasonal"][0], case.x0, case.theta, None, None, substeps=3, grid=grid)
    got, status = R.rk4(R.callable_for("seir_seasonal"), case.x0[None], case.theta[None], grid, 3)
    assert status[0] == 0
    np.testing.assert_allclose(got[0], want, rtol=4e-16, atol=0)          # (numpy's vector and scalar cos may differ in the last bit)


def test_ode_unit_is_built_declared_and_bound():
    from magi_v2_amd import api, build, engine, jit
    assert os.path.join(build.CSRC, "ode.hip") in build.sources()
    assert "ode.hip" not in jit._DRIFT_FREE
    hdr = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    assert re.search(r"int magi_ode_solve\(magi_handle\* h, int drift_id, int P, int S,\s*const double\* x0, const double\* theta,\s*"
                     r"int T, const double\* t_out, int substeps,\s*double\* traj, double\* mean, double\* sd, int\* status, int\* n_failed\);", hdr)
    assert "magi_ode_solve" in engine.exported_symbols() and len(engine._SYMBOLS["magi_ode_solve"][1]) == 14
    assert hasattr(engine.MagiEngine, "ode_solve") and hasattr(api.MAGI_v2, "posterior_trajectories")
    if shutil.which(build.hipcc()) is None:
        pytest.skip("no hipcc")
    build.build_lib(verbose=False)
    assert hasattr(engine.load_library(), "magi_ode_solve")


def test_ode_unit_compiles_clean_without_scratch_or_spills():
    """The EXEC-prologue guard passes, and tools/resource_usage.py shows every kernel of the call in the base library -- k_ode_rk4 for the
    three compiled-in drifts in ode.hip; k_ode_stats and k_transpose in summary.hip, the drift-free unit a traced drift's library reuses --
    with 0 spilled registers and 0 scratch."""
    from magi_v2_amd import build, isa_check, jit
    if shutil.which(build.hipcc()) is None:
        pytest.skip("no hipcc")
    build.build_lib(verbose=False)
    assert "summary.hip" in jit._DRIFT_FREE
    rows = []
    for unit, prefixes in (("ode.hip", ("k_ode_",)), ("summary.hip", ("k_ode_", "k_transpose"))):
        isa = build.isa_path(os.path.join(build.OBJDIR, unit + ".o"))
        assert os.path.exists(isa) and isa_check.check_file(isa) == []
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), unit], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        rows += [[c.strip() for c in line.split("|")] for line in r.stdout.splitlines() if line.startswith(prefixes)]
    assert sorted(row[0].split("(")[0] for row in rows) == ["k_ode_rk4<0>", "k_ode_rk4<1>", "k_ode_rk4<2>", "k_ode_stats", "k_transpose"], rows
    for name, vgprs, vspill, sspill, scratch, occ, lds in rows:
        assert (vspill, sspill, scratch) == ("0", "0", "0"), (name, vspill, sspill, scratch)
