"""Time-dependent drifts, everything that needs no GPU: an ``f_vec`` that uses its first argument is traced (``Drift.time_dependent``),
its host evaluators take the times of the rows, its header carries ``TDEP`` and the time ``t_magi`` in every drift member, and the
library compiled for it reports itself time-dependent.  The reference passes its grid ``self.I`` as ``t`` (magi_v2.py:155, 206, 335);
the three examples are ``drift_examples.TIME_EXAMPLES``.  Also here: the fixtures the GPU tests of the same feature run on."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from magi_v2_amd import drift, host, jit
from magi_v2_amd.drift_examples import EXAMPLES, TIME_EXAMPLES, rk4, seir_seasonal
from magi_v2_amd.engine import exported_symbols

N_GRID = 41
# name -> (generating parameters, initial state, T)
FIXTURES = {"seir_seasonal": (np.array([6.0, 0.6, 1.8, 0.4]), [0.02, 0.01, 0.0], 4.0),
            "fhn_forced": (np.array([0.2, 0.2, 3.0, 0.5]), [-1.0, 1.0], 20.0),
            "mm_infusion": (np.array([2.0, 1.5, 0.5, 0.4]), [0.1, 0.0], 12.0)}


def fixture_grid(name):
    """Uniform, except for the forced FitzHugh-Nagumo system: T (0.6 u + 0.4 u^2) -- times that no index and spacing reconstruct."""
    T = FIXTURES[name][2]
    u = np.linspace(0.0, 1.0, N_GRID)
    return T * (0.6 * u + 0.4 * u ** 2) if name == "fhn_forced" else T * u


def fixture_data(name):
    """(I[N], X_true[N, D], X_obs[N, D], truth[P], phi2): RK4 (20 sub-steps, the drift evaluated at the current time) on the fixture's grid,
    noise N(0, (0.05 std_d)^2) from default_rng(0), every second row unobserved."""
    f_vec = TIME_EXAMPLES[name][0]
    truth, x0, T = FIXTURES[name]
    I = fixture_grid(name)
    _, X = rk4(f_vec, x0, truth, T, N_GRID, substeps=20, grid=I)
    rng = np.random.default_rng(0)
    X_obs = X + rng.normal(0.0, 1.0, X.shape) * (0.05 * X.std(axis=0))
    X_obs[1::2] = np.nan
    return I, X, X_obs, truth, (0.5 if T <= 5 else 1.5)


def complex_step_jacobians_at(f_vec, t, X, th):
    """tests/test_drift_cpu.py::complex_step_jacobians with the times of the rows (t[n, 1]) passed to the callable."""
    n, D = X.shape
    P = len(th)
    h = 1e-30
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    J = np.zeros((n, D, D)); T = np.zeros((n, D, P))
    for k in range(D):
        Xc = X.astype(complex); Xc[:, k] += 1j * h
        J[:, :, k] = np.imag(f_vec(t, Xc, th.astype(complex))) / h
    for p in range(P):
        tc = th.astype(complex); tc[p] += 1j * h
        T[:, :, p] = np.imag(f_vec(t, X.astype(complex), tc)) / h
    return J, T


def oracle_drift_at(f_vec, times):
    """An entry of the oracle's drift table, ``fn(X, th) -> (f, J, T)``, that evaluates ``f_vec`` at the times ``times`` (one per row of
    X): a closure over the grid column, Jacobians by complex step WITH the times."""
    tcol = np.asarray(times, dtype=np.float64).reshape(-1, 1).copy()

    def fn(X, th):
        X, th = np.asarray(X, dtype=np.float64), np.asarray(th, dtype=np.float64)
        J, T = complex_step_jacobians_at(f_vec, tcol, X, th)
        return np.asarray(f_vec(tcol, X, th), dtype=np.float64), J, T
    return fn


def test_a_drift_that_uses_t_is_traced_and_its_evaluators_take_the_times():
    for name, (f_vec, D, P) in TIME_EXAMPLES.items():
        d = drift.resolve(f_vec, D, P)
        assert d.time_dependent and not d.is_builtin and (d.D, d.P) == (D, P), name
        rng = np.random.default_rng(1)
        X, th, t = rng.uniform(-1.5, 1.5, (11, D)), rng.uniform(0.3, 2.5, P), rng.uniform(0.0, 20.0, (11, 1))
        np.testing.assert_allclose(d.f_np(t, X, th), f_vec(t, X, th), rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(d.f_np(t[:, 0], X, th), f_vec(t, X, th), rtol=1e-14, atol=1e-15)       # [N] as well as [N, 1]
        Jc, Tc = complex_step_jacobians_at(f_vec, t, X, th)
        for tt in (t, t[:, 0]):
            J, T = d.jac_np(X, th, tt)
            np.testing.assert_allclose(J, Jc, rtol=1e-13, atol=1e-14)
            np.testing.assert_allclose(T, Tc, rtol=1e-13, atol=1e-14)
        with pytest.raises(ValueError, match=r"\bt\b"):
            d.jac_np(X, th)
        # (the drift really depends on t: frozen at 0 it is another function)
        assert np.abs(d.f_np(t, X, th) - d.f_np(np.zeros_like(t), X, th)).max() > 1e-3
    for name, (f_vec, D, P) in EXAMPLES.items():
        d = drift.resolve(f_vec, D, P)
        assert not d.time_dependent, name
        X, th = np.random.default_rng(2).uniform(0.1, 1.0, (5, D)), np.full(P, 0.7)
        J0, T0 = d.jac_np(X, th)
        J1, T1 = d.jac_np(X, th, np.linspace(0, 1, 5))              # t is ignored: every existing caller keeps working
        np.testing.assert_array_equal(J0, J1); np.testing.assert_array_equal(T0, T1)
    # the plain call of trace_drift still traces an autonomous drift only
    with pytest.raises(NotImplementedError, match="explicit use of t"):
        drift.trace_drift(seir_seasonal, 3, 4)
    assert drift.trace_drift(seir_seasonal, 3, 4, allow_time=True).time_dependent


def _nbasis(header, D):
    m = re.search(r"static constexpr int nbasis\(int d\) \{ return (.*?); \}", header)
    expr = m.group(1)
    out = []
    for d in range(D):
        out.append(int(eval(expr.replace("?", " and ").replace(":", " or "), {"d": d})))       # "d == 0 ? 3 : d == 1 ? 2 : 1"
    return tuple(out)


def test_separable_form_treats_t_as_part_of_x_and_headers_carry_tdep():
    want = {"seir_seasonal": (3, 2, 1), "fhn_forced": (2, 3), "mm_infusion": None}
    for name, (f_vec, D, P) in TIME_EXAMPLES.items():
        h = drift.resolve(f_vec, D, P).header
        assert "static constexpr bool TDEP = true;" in h, name
        assert "t_magi" in h
        if want[name] is None:
            assert "static constexpr bool SEP = false;" in h, name
        else:
            assert "static constexpr bool SEP = true;" in h, name
            assert _nbasis(h, D) == want[name], (name, _nbasis(h, D))
        # every member that evaluates the drift takes the time; coefs(theta) does not
        for member in ("void f(", "double f1(", "void jt(") + (("void basis(",) if want[name] else ()):
            sig = h.split(member, 1)[1].split(" {\n", 1)[0]
            assert "const double t_magi" in sig, (name, member, sig)
        assert "t_magi" not in h.split("void coefs(", 1)[1].split("{", 1)[0]
    # seasonal SEIR, component 0: th2 (-x0) + th0 (x1 S) + th0 th3 (x1 S cos(pi t)) -- one basis function carries the cosine
    h = drift.resolve(*TIME_EXAMPLES["seir_seasonal"]).header
    basis = h.split("void basis(", 1)[1].split("\n    }\n", 1)[0]
    assert len(re.findall(r"^\s*ph\[0\]\[\d\] = .*cos\(", basis, flags=re.M)) == 1
    # forced FitzHugh-Nagumo: a basis function of t alone
    h = drift.resolve(*TIME_EXAMPLES["fhn_forced"]).header
    basis = h.split("void basis(", 1)[1].split("\n    }\n", 1)[0]
    assert re.search(r"^\s*ph\[0\]\[1\] = cos\(0\.8\d*\*t_magi\);$", basis, flags=re.M), basis
    for name, (f_vec, D, P) in EXAMPLES.items():
        h = drift.resolve(f_vec, D, P).header
        assert "TDEP = true" not in h and "static constexpr bool TDEP = false;" in h, name


@pytest.mark.parametrize("name", sorted(TIME_EXAMPLES))
def test_time_dependent_library_builds_clean_for_gfx950_and_says_what_it_is(name, tmp_path):
    """hipcc cross-compiles the kernels for the drift (no GPU needed); the library exports every name of include/magi_hip.h and
    magi_user_drift_time_dependent() is 1 (0 in the base library).  Its streaming and point kernels spill no vector register and reserve
    no scratch, and pass the EXEC-prologue guard."""
    from magi_v2_amd import build, isa_check
    f_vec, D, P = TIME_EXAMPLES[name]
    d = drift.resolve(f_vec, D, P)
    path = jit.library_for(d)
    lib = ctypes.CDLL(path)
    for sym in exported_symbols():
        assert hasattr(lib, sym), sym
    for sym in ("magi_set_times", "magi_user_drift_time_dependent", "magi_drift_probe_at"):
        assert sym in exported_symbols()
    Dc, Pc = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.magi_user_drift_info(ctypes.byref(Dc), ctypes.byref(Pc)) == 1 and (Dc.value, Pc.value) == (D, P)
    assert lib.magi_user_drift_time_dependent() == 1
    base = ctypes.CDLL(os.path.join(os.path.dirname(jit.__file__), "libmagi_hip.so"))
    assert base.magi_user_drift_time_dependent() == 0
    auto = ctypes.CDLL(jit.library_for(drift.resolve(*EXAMPLES["fhn"])))
    assert auto.magi_user_drift_time_dependent() == 0
    # resource usage and ISA of the units that hold the stream and point kernels, compiled for THIS drift's header
    hdr = os.path.join(os.path.dirname(path), "user_drift.h")
    assert os.path.exists(hdr)
    seen = 0
    for unit in ("leap.hip", "leap_group.hip"):
        src = os.path.join(build.CSRC, unit)
        obj = str(tmp_path / (unit + ".o"))
        r = subprocess.run(build.compile_command(src, jit.drift_flags(d, hdr) + ["-Rpass-analysis=kernel-resource-usage"]) +
                           ["-c", src, "-o", obj, "--save-temps=obj"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        assert isa_check.check_file(build.isa_path(obj)) == [], unit
        for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
            kname = b.split(" [")[0]
            if "k_stream" not in kname and "k_point" not in kname and "k_mirror" not in kname:
                continue
            seen += 1
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, kname
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, kname
    assert seen >= 6, seen               # k_stream<1>, <2>, a matrix-core kernel, k_point, the two group twins, ...


def test_gradient_matching_objective_of_a_time_dependent_drift_has_the_right_gradients():
    """magi_v2.py:196-216 with E of the seasonal SEIR never observed: the drift is evaluated at the grid times (the Jacobians at the
    interior ones), the analytic gradients equal central differences of the loss (the bounds of the autonomous twin of this test)."""
    from magi_v2_amd.api import MAGI_v2
    I, X, X_obs, truth, _ = fixture_data("seir_seasonal")
    X_obs = X_obs.copy()
    X_obs[:, 0] = np.nan
    m = MAGI_v2(D_thetas=4, ts_obs=I, X_obs=X_obs, bandsize=None, f_vec=seir_seasonal)
    assert m.drift.time_dependent
    m.I, Xd = host.discretize(m.ts_obs, m.X_obs, 1)
    m.mag_I = m.I.shape[0]
    rng = np.random.default_rng(3)
    Xs = host.cubic_smoother(m.I, host.linear_interpolate(Xd[:, m.observed_indicators]))
    Xu, th = rng.normal(0.05, 0.02, (m.mag_I, 1)), rng.uniform(0.5, 3, 4)
    loss, gX, gth = m.gradient_matching_loss_and_grads(Xs, Xu, th)

    def ref(Xu_, th_):                   # the loss restated: drift at the grid times against centred differences
        Xf = np.concatenate([Xs, Xu_], axis=1)[:, m.proper_order]
        f = seir_seasonal(m.I, Xf, th_)
        r = f[1:-1] - (Xf[2:] - Xf[:-2]) / (2.0 * (m.I[1, 0] - m.I[0, 0]))
        return float((r ** 2).sum())
    assert abs(loss - ref(Xu, th)) <= 1e-12 * abs(loss)
    frozen = float(((seir_seasonal(0.0 * m.I, np.concatenate([Xs, Xu], axis=1)[:, m.proper_order], th)[1:-1] -
                     (np.concatenate([Xs, Xu], axis=1)[:, m.proper_order][2:] - np.concatenate([Xs, Xu], axis=1)[:, m.proper_order][:-2]) /
                     (2.0 * (m.I[1, 0] - m.I[0, 0]))) ** 2).sum())
    assert abs(frozen - loss) > 1e-3 * abs(loss)            # (the times matter in this loss)
    for p in range(4):
        e = np.zeros(4); e[p] = 1e-6
        assert abs((ref(Xu, th + e) - ref(Xu, th - e)) / 2e-6 - gth[p]) <= 1e-6 * max(1.0, abs(gth[p]))
    for i in (0, 1, 40, m.mag_I - 2, m.mag_I - 1):
        E = np.zeros_like(Xu); E[i, 0] = 1e-6
        assert abs((ref(Xu + E, th) - ref(Xu - E, th)) / 2e-6 - gX[i, 0]) <= 1e-5 * max(1.0, abs(gX[i, 0]))


def test_fixture_integrator_passes_the_time_and_leaves_autonomous_trajectories_alone():
    f_vec, D, P = EXAMPLES["fhn"]
    I, X = rk4(f_vec, [-1.0, 1.0], np.array([0.2, 0.2, 3.0]), 20.0, 41)
    seen = []

    def spy(t, Xv, th):
        seen.append(float(np.asarray(t).reshape(-1)[0]))
        return f_vec(t, Xv, th)
    I2, X2 = rk4(spy, [-1.0, 1.0], np.array([0.2, 0.2, 3.0]), 20.0, 41)
    np.testing.assert_array_equal(X, X2)
    assert seen[0] == 0.0 and abs(max(seen) - 20.0) < 1e-9 and np.all(np.diff(seen[::4]) > 0)
    # a grid of its own
    g = fixture_grid("fhn_forced")
    I3, X3 = rk4(TIME_EXAMPLES["fhn_forced"][0], [-1.0, 1.0], FIXTURES["fhn_forced"][0], 20.0, 41, grid=g)
    np.testing.assert_array_equal(I3, g)
    assert X3.shape == (41, 2) and np.isfinite(X3).all()
