"""CPU truths for the device sensitivities (magi_ode_sensitivities; tests/test_sens_cpu.py, tests/test_sens_gpu.py), on the cases, draws and
RK4 restatement of tests/ode_reference.py (imported unchanged).  A helper module: product code never imports it.

Two independent truths of sens[s, j, d, q] = d x_d(t_j) / d (theta_q or x0 component q - P) of the DISCRETE map ``ode_reference.rk4``:
  (a) ``complex_step``: ``ode_reference.rk4`` run in complex arithmetic with an imaginary perturbation of 1e-30 on one theta or x0 entry;
      the derivative is the imaginary part / 1e-30, exact to rounding.  It uses the drift CALLABLE alone, no Jacobian code at all, so
      the device is held to the callable and not to the trace its Jacobians come from.
  (b) ``augmented``: the variational equations beside the state on the same stages, with the Jacobians of ``Drift.exprs`` -- the sympy
      derivatives ``Drift.jac_np`` evaluates -- lambdified without jac_np's float64 casts and with a theta per draw, so that the scheme
      runs in float64 or longdouble.  It comes with the deliberately wrong schemes the CPU test holds the bar against.
Bar: ``ode_reference.BAR`` (1e-11) times the column's max |sens| over draws, times and components: columns have different units.

The Fisher information F[s, a, b] = sum_k ((w_k / sigma_sq[s, d_k]) g'(x)^2) sens_a sens_b is restated in the order the header states
(``fisher``), with its own wrong variants."""
import functools
import warnings

import numpy as np

from magi_v2_amd import drift as drift_mod
from tests import ode_reference as R

BAR = R.BAR
STEP = 1e-30                         # the complex step: x + i STEP never rounds into the real part
VARIANTS = ("dtheta_missing_last", "jac_transposed", "stale_increment", "mid_jac_time_at_s")
FIM_VARIANTS = ("no_gprime", "sigma_not_squared", "no_weights")
LINKS = {"identity": 0, "log": 1, "sqrt": 2}


def drift_for(name):
    case = R.CASES[name]
    return drift_mod.resolve(name if name in R.BUILTIN else R.TRACED[name][0], case.D, case.P)


def names(case):
    return [f"theta[{p}]" for p in range(case.P)] + [f"x0[{d}]" for d in range(case.D)]


def complex_step(f, x0, theta, t_out, substeps, cols=None, dtype=np.complex128):
    """(a): sens[S, T, D, Q] in the real dtype that belongs to ``dtype``; one complex run of ``ode_reference.rk4`` per column."""
    x0, theta = np.asarray(x0), np.asarray(theta)
    P, D = theta.shape[1], x0.shape[1]
    cols = range(P + D) if cols is None else cols
    out = []
    for q in cols:
        xc, tc = np.array(x0, dtype=dtype), np.array(theta, dtype=dtype)
        if q < P:
            tc[:, q] += dtype(1j * STEP)
        else:
            xc[:, q - P] += dtype(1j * STEP)
        with warnings.catch_warnings():                      # (the oracle's callables also fill real Jacobian arrays nobody reads here)
            warnings.simplefilter("ignore", getattr(np, "exceptions", np).ComplexWarning)
            traj, _ = R.rk4(f, xc, tc, t_out, substeps, dtype=dtype)
        out.append(traj.imag / STEP)
    return np.stack(out, axis=3)


@functools.lru_cache(maxsize=None)
def jacobians(name):
    """(J, T)(t scalar, X[S, D], TH[S, P]) -> [S, D, D], [S, D, P] in the dtype of X: d f_d / d x_k and d f_d / d theta_p of the drift's
    sympy trace (``Drift.exprs``), one theta per row."""
    import sympy as sp
    case = R.CASES[name]
    D, P = case.D, case.P
    exprs = drift_for(name).exprs
    xs, ths, tsym = sp.symbols(f"x0:{D}", real=True), sp.symbols(f"th0:{P}", real=True), sp.Symbol("t_magi", real=True)
    args = [tsym] + list(xs) + list(ths)
    j_l = sp.lambdify(args, [sp.diff(exprs[d], xs[k]) for d in range(D) for k in range(D)], modules="numpy")
    t_l = sp.lambdify(args, [sp.diff(exprs[d], ths[p]) for d in range(D) for p in range(P)], modules="numpy")

    def ev(t, X, TH):
        S = X.shape[0]
        a = [np.full(S, t, dtype=X.dtype)] + [X[:, k] for k in range(D)] + [TH[:, p] for p in range(P)]
        full = lambda vals, n: np.stack([np.broadcast_to(np.asarray(v, dtype=X.dtype), (S,)) for v in vals], axis=1).reshape(S, D, n)
        return full(j_l(*a), D), full(t_l(*a), P)

    return ev


def augmented(name, x0, theta, t_out, substeps, dtype=np.float64, variant=None):
    """(b): (sens[S, T, D, P + D], trajectories[S, T, D]) in ``dtype``.  ``variant``: None, or one of VARIANTS -- the df/dtheta term
    missing at the last stage; J_x^T in place of J_x; the third and fourth stage sensitivities built with the increment of the stage
    before the right one (l1 for l2, l2 for l3); the two middle stages' Jacobians taken at time s (time-dependent drifts)."""
    assert variant is None or variant in VARIANTS, variant
    f, jac = R.callable_for(name), jacobians(name)
    x = np.array(x0, dtype=dtype)
    th = np.array(theta, dtype=dtype)
    t = np.asarray(t_out, dtype=np.float64).astype(dtype)
    S, D = x.shape
    P = th.shape[1]
    Q = P + D
    Z = np.zeros((S, D, Q), dtype=dtype)
    for e in range(D):
        Z[:, e, P + e] = 1.0
    xs, zs = [x.copy()], [Z.copy()]

    def L(s, y, W, with_theta=True):
        J, Tm = jac(s, y, th)
        if variant == "jac_transposed":
            J = J.transpose(0, 2, 1)
        out = (J[:, :, :, None] * W[:, None, :, :]).sum(axis=2)
        if with_theta:
            out[:, :, :P] += Tm
        return out

    with np.errstate(all="ignore"):
        for j in range(len(t) - 1):
            h = (t[j + 1] - t[j]) / substeps
            for k in range(substeps):
                s = t[j] + k * h
                sm = s + 0.5 * h
                smj = s if variant == "mid_jac_time_at_s" else sm
                F = lambda tt, y: np.asarray(f(tt, y, th), dtype=dtype)
                k1, l1 = F(s, x), L(s, x, Z)
                y2 = x + 0.5 * h * k1
                k2, l2 = F(sm, y2), L(smj, y2, Z + 0.5 * h * l1)
                y3 = x + 0.5 * h * k2
                k3, l3 = F(sm, y3), L(smj, y3, Z + 0.5 * h * (l1 if variant == "stale_increment" else l2))
                y4 = x + h * k3
                k4, l4 = F(s + h, y4), L(s + h, y4, Z + h * (l2 if variant == "stale_increment" else l3), with_theta=variant != "dtheta_missing_last")
                x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
                Z = Z + h / 6.0 * (l1 + 2 * l2 + 2 * l3 + l4)
            xs.append(x.copy())
            zs.append(Z.copy())
    return np.stack(zs, axis=1), np.stack(xs, axis=1)


@functools.lru_cache(maxsize=None)
def reference(name, substeps, kind="complex", dtype_name="float64", S=R.BATCH, variant=None):
    """sens[S, T, D, P + D] of the case's batch on its own grid, computed once per session and shared: treat it as read-only.
    kind "complex": truth (a); "augmented": truth (b) (``variant`` applies to it alone)."""
    case = R.CASES[name]
    x0, th = R.draws(case, S)
    if kind == "complex":
        assert variant is None
        out = complex_step(R.callable_for(name), x0, th, case.t, substeps, dtype={"float64": np.complex128, "longdouble": np.clongdouble}[dtype_name])
    else:
        out = augmented(name, x0, th, case.t, substeps, dtype=getattr(np, dtype_name), variant=variant)[0]
    out.setflags(write=False)
    return out


def column_scale(want):
    """max |sens| of every column over draws, times and components, [Q]."""
    return np.abs(np.asarray(want, dtype=np.longdouble)).max(axis=(0, 1, 2))


def bars(got, want):
    """Per column: max |got - want| in bars of that column (1e-11 of its max |want|), [Q] float64."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return (np.abs(got - want).max(axis=(0, 1, 2)) / (BAR * column_scale(want))).astype(np.float64)


def link_derivative(link, x):
    return 1.0 / x if link == 1 else 0.5 / np.sqrt(x) if link == 2 else np.ones_like(x)


def fisher(sens, traj, obs_j, obs_comp, weight, sigma_sq, link, dtype=np.float64, variant=None):
    """F[S, Q, Q] from sens[S, T, D, Q] and traj[S, T, D] in the order the header states: k ascending, cf = (w_k / sigma_sq[s, d_k]) *
    (g' * g'), F += (cf * sens_a) * sens_b.  ``variant``: None or one of FIM_VARIANTS -- g' dropped; sigma in place of sigma^2; the
    weights dropped."""
    assert variant is None or variant in FIM_VARIANTS, variant
    sens, traj, sig = np.asarray(sens, dtype=dtype), np.asarray(traj, dtype=dtype), np.asarray(sigma_sq, dtype=dtype)
    S, _, D, Q = sens.shape
    w = np.ones(len(obs_j), dtype=dtype) if weight is None or variant == "no_weights" else np.asarray(weight, dtype=dtype)
    link = [0] * D if link is None else [LINKS.get(v, v) for v in link]
    F = np.zeros((S, Q, Q), dtype=dtype)
    with np.errstate(all="ignore"):
        for k, (j, d) in enumerate(zip(obs_j, obs_comp)):
            gp = np.ones(S, dtype=dtype) if variant == "no_gprime" else link_derivative(link[d], traj[:, j, d])
            var = np.sqrt(sig[:, d]) if variant == "sigma_not_squared" else sig[:, d]
            cf = (w[k] / var) * (gp * gp)
            F += (cf[:, None] * sens[:, j, d, :])[:, :, None] * sens[:, j, d, None, :]
    a, b = np.triu_indices(Q, 1)
    F[:, b, a] = F[:, a, b]                                   # computed for a <= b as (cf s_a) s_b, and mirrored
    return F


def fisher_bar(F, n_obs):
    """8 n_obs 2^-52 sqrt(F_aa F_bb) per entry, [S, Q, Q]: n_obs terms of a few roundings each; Cauchy-Schwarz bounds sum |terms|."""
    dg = np.sqrt(np.abs(np.diagonal(np.asarray(F, dtype=np.float64), axis1=-2, axis2=-1)))
    return 8.0 * n_obs * 2.0 ** -52 * dg[..., :, None] * dg[..., None, :]


FIM_CASE, FIM_S = "sirw", 65
FIM_LINK = ("identity", "log", "sqrt", "identity")


def fisher_setup():
    """The Fisher-information case of both test files: sirw, 65 draws, every (time, component) of its grid observed (164 entries, time-major),
    a log link on component 1 and sqrt on component 2 (the states stay positive), weights in [0.5, 2) and a variance per draw and
    component in [1e-4, 4e-4).  Returns dict(x0, theta, t, obs=dict(j, comp, weight, sigma_sq, link))."""
    case = R.CASES[FIM_CASE]
    x0, th = R.draws(case, FIM_S)
    T, D = len(case.t), case.D
    rng = np.random.default_rng(21)
    j, comp = np.repeat(np.arange(T), D).astype(np.int32), np.tile(np.arange(D), T).astype(np.int32)
    return {"x0": x0, "theta": th, "t": case.t,
            "obs": {"j": j, "comp": comp, "weight": rng.uniform(0.5, 2.0, T * D), "sigma_sq": rng.uniform(1e-4, 4e-4, (FIM_S, D)), "link": FIM_LINK}}
