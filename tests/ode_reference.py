"""CPU truth for the device ODE solver (magi_ode_solve; tests/test_ode_cpu.py, tests/test_ode_gpu.py): the scheme of
``magi_v2_amd.drift_examples.rk4`` restated in numpy for a batch of draws, in float64 or longdouble, with the deliberately wrong schemes
the CPU test holds the device bar against.  A helper module: product code never imports it.

Scheme: h = (t[j+1] - t[j]) / substeps; sub-step k starts at s = t[j] + k h; stages at s, s + h/2, s + h/2, s + h;
x += h/6 (k1 + 2 k2 + 2 k3 + k4).  status[s]: 0, or j + 1 for the first interval [t[j], t[j+1]] whose output has a non-finite component (the index of that output; a
non-finite x0 gives 1)."""
import functools

import numpy as np

from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES, EDGE_EXAMPLES, EXAMPLES, TIME_EXAMPLES
from oracle import magi_oracle as orc

BAR = 1e-11                      # device tolerance, as a fraction of max|x| of the case
VARIANTS = ("k4_weight", "mid_time_at_s", "drop_last_substep", "euler")
TRACED = {**EXAMPLES, **TIME_EXAMPLES, **DOMAIN_EXAMPLES, **EDGE_EXAMPLES}
BUILTIN = ("seir3", "sirw")      # compiled into the base library; their CPU callables are the oracle's


class Case:
    def __init__(self, drift, x0, theta, t_end, n, time_dependent=False):
        self.drift, self.x0, self.theta = drift, np.asarray(x0, dtype=np.float64), np.asarray(theta, dtype=np.float64)
        self.t = np.linspace(0.0, t_end, n)
        self.time_dependent = time_dependent
        self.D, self.P = len(self.x0), len(self.theta)

    def __repr__(self):
        return self.drift


CASES = {c.drift: c for c in (
    Case("seir3", (0.1, 0.05, 0.0), (6.0, 0.6, 1.8), 4.0, 41),
    Case("sirw", (0.9, 0.05, 0.02, 0.03), (2.0, 0.5, 0.3, 1.0, 0.2), 10.0, 41),
    Case("fhn", (-1.0, 1.0), (0.2, 0.2, 3.0), 20.0, 41),
    Case("lotka_volterra", (1.0, 0.5), (1.0, 1.0, 1.0, 1.0), 10.0, 41),
    Case("seir_seasonal", (0.1, 0.05, 0.0), (6.0, 0.6, 1.8, 0.3), 4.0, 41, time_dependent=True),
    Case("chain8", (0.3,) * 8, (0.5, 0.4, 0.6, 0.7, 0.5, 0.6, 0.4, 0.8), 4.0, 33),
    Case("sqrt_outflow", (0.25, 0.1), (0.2, 0.5, 0.3), 2.0, 33),
)}
SUBSTEPS_1_CASES = ("lotka_volterra", "seir_seasonal", "chain8")          # (FitzHugh-Nagumo at one sub-step: float64 vs longdouble up to 9e-13)
BATCH = 257                                                              # lane, wave and workgroup edges: S = 1, 63, 64, 65, 257 are its leading draws

# the status case: sqrt_outflow leaves its domain sooner or later according to theta_0
STATUS_X0, STATUS_A, STATUS_WANT = (0.25, 0.1), (1.0, 0.9, 1.3, 0.7, 0.2), (16, 18, 13, 23, 0)
STATUS_T, STATUS_SUBSTEPS = np.linspace(0.0, 2.0, 33), 2


def status_inputs(extra_survivor=False):
    a = list(STATUS_A) + ([0.25] if extra_survivor else [])
    return np.tile(np.asarray(STATUS_X0), (len(a), 1)), np.array([[v, 0.5, 0.3] for v in a])


def callable_for(drift):
    """f(t scalar, X[S, D], TH[S, P]) -> [S, D] in the dtype of its arguments: the oracle's drift function for a compiled-in drift, the
    ``drift_examples`` callable for a traced one (draw s is row s of all three)."""
    if drift in BUILTIN:
        fn = orc.DRIFTS[drift][0]
        return lambda t, X, TH: fn(X, TH.T)[0]
    f_vec = TRACED[drift][0]
    return lambda t, X, TH: f_vec(np.full((X.shape[0], 1), t, dtype=X.dtype), X, TH.T[:, :, None])


def draws(case, S=BATCH, seed=0):
    """(x0[S, D], theta[S, P]): draw 0 is the case's nominal input, the others i.i.d. perturbations of it by <= 5 %; the first draws of
    a larger batch are the draws of a smaller one."""
    u = np.random.default_rng([seed, case.D, case.P]).uniform(-1.0, 1.0, (S, case.D + case.P))      # (row s is the same for every S)
    x0 = case.x0[None] * (1.0 + 0.05 * u[:, :case.D])
    th = case.theta[None] * (1.0 + 0.05 * u[:, case.D:])
    x0[0], th[0] = case.x0, case.theta
    return x0, th


def rk4(f, x0, theta, t_out, substeps, dtype=np.float64, variant=None, on_stage=None):
    """(trajectories[S, T, D], status[S]) in ``dtype``.  ``variant``: None, or one of VARIANTS -- a k4 weight times (1 + 1e-6); the two
    middle stages evaluated at time s; the last sub-step of every interval dropped; explicit Euler.  ``on_stage(y[S, D])`` sees every
    state the drift is evaluated at."""
    assert variant is None or variant in VARIANTS, variant
    x = np.array(x0, dtype=dtype)
    th = np.array(theta, dtype=dtype)
    t = np.asarray(t_out, dtype=np.float64).astype(dtype)
    out = [x.copy()]
    w4 = dtype(1.0) + (dtype(1e-6) if variant == "k4_weight" else dtype(0.0))

    def F(s, y):
        if on_stage is not None:
            on_stage(y)
        return np.asarray(f(s, y, th), dtype=dtype)

    with np.errstate(all="ignore"):
        for j in range(len(t) - 1):
            h = (t[j + 1] - t[j]) / substeps
            for k in range(substeps - 1 if variant == "drop_last_substep" else substeps):
                s = t[j] + k * h
                if variant == "euler":
                    x = x + h * F(s, x)
                    continue
                sm = s if variant == "mid_time_at_s" else s + 0.5 * h
                k1 = F(s, x); k2 = F(sm, x + 0.5 * h * k1); k3 = F(sm, x + 0.5 * h * k2); k4 = F(s + h, x + h * k3)
                x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + w4 * k4)
            out.append(x.copy())
    traj = np.stack(out, axis=1)
    bad = ~np.isfinite(traj).all(axis=2)                                 # [S, T]
    status = np.where(bad.any(axis=1), np.maximum(bad.argmax(axis=1), 1), 0).astype(np.int32)
    return traj, status


@functools.lru_cache(maxsize=None)
def reference(drift, substeps, dtype_name="float64", S=BATCH, variant=None):
    """(trajectories, status) of the case's batch on its own grid, computed once per session and shared: treat it as read-only.  The
    outputs on a grid cut after T' points are its first T' (the steps of an interval depend on that interval alone)."""
    case = CASES[drift]
    x0, th = draws(case, S)
    traj, status = rk4(callable_for(drift), x0, th, case.t, substeps, dtype=getattr(np, dtype_name), variant=variant)
    traj.setflags(write=False)
    status.setflags(write=False)
    return traj, status


def distance(a, b):
    """max |a - b| as a fraction of max |b|, over finite entries of b."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / np.abs(b).max())
