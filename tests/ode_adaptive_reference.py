"""CPU truth for the error-controlled ODE integrators (magi_ode_solve_adaptive; tests/test_ode_adaptive_cpu.py, tests/test_ode_adaptive_gpu.py):
both methods and the controller of include/magi_hip.h restated in numpy for a batch of draws, in float64 or longdouble, every draw with its
own time, step and interval, and the deliberately wrong variants the CPU test holds the device bar against.  A helper module: product code
never imports it.

The drift is the case's callable (tests/ode_reference.py); J = df/dx and T = df/dt are sympy derivatives of the traced expressions evaluated
per draw (tests/test_ode_adaptive_cpu.py holds T against a central difference of the callable, the J transposed variant shows what J
carries).  The linear solves are a Gaussian elimination with partial pivoting written here (lu_factor, lu_solve).

Draws: the +-5 % perturbations of tests/ode_reference.py (draw 0 is the nominal input; a zero component of x0 stays zero), BATCH = 257 of
them: the leading 1, 63, 64, 65 are the smaller batches."""
import functools

import numpy as np

from magi_v2_amd import drift as drift_mod
from magi_v2_amd.drift_examples import STIFF_EXAMPLES
from oracle import magi_oracle as orc
from tests import ode_reference as R0

BATCH = R0.BATCH
BUILTIN = R0.BUILTIN
TRACED = {**R0.TRACED, **STIFF_EXAMPLES}
METHODS = ("dopri5", "ros23")
ORDER_Q = {"dopri5": 5, "ros23": 3}
REASONS = {"none": 0, "nonfinite": 1, "budget": 2, "underflow": 3}
ATOL, MAX_STEPS = 1e-9, 100000
FLOOR = 1e-13                      # of max|x|: the least bar, about 450 ulp of the largest entry
VARIANTS = ("drop_T", "e32", "b_weight", "wrong_q", "reject_grows", "no_clip", "J_transposed")

Case = R0.Case
CASES = {c.drift: c for c in (
    Case("robertson", (1.0, 0.0, 0.0), (0.04, 3e7, 1e4), 40.0, 41),
    Case("van_der_pol", (2.0, 0.0), (50.0,), 100.0, 41),
    Case("forced_relaxation", (1.5, 0.0), (1000.0, 2.0), 5.0, 41, time_dependent=True),
    R0.CASES["seir3"], R0.CASES["sirw"], R0.CASES["lotka_volterra"], R0.CASES["seir_seasonal"], R0.CASES["chain8"],
    Case("logistic1", (0.1,), (1.5, 2.0), 6.0, 33),
)}
# (case, method, rtol): the table of the issue, then both methods at 1e-6 on the non-stiff cases
RUNS = (("robertson", "ros23", 1e-4), ("robertson", "ros23", 1e-6), ("van_der_pol", "dopri5", 1e-9), ("van_der_pol", "ros23", 1e-4),
        ("forced_relaxation", "ros23", 1e-6)) + tuple((c, m, 1e-6) for c in ("seir3", "sirw", "lotka_volterra", "seir_seasonal", "chain8", "logistic1")
                                                      for m in METHODS)
STIFF_RUNS = RUNS[:5]
# Van der Pol under DOPRI5 is the one run whose tolerance and draws are not the issue's first choice (1e-6, seed 0).  An explicit method
# steps at its stability limit on this limit cycle: errn hovers about 1 for thousands of steps and carries their rounding (float64 and
# longdouble differ by about 1e-6 in it), so that at 1e-6 the two disagree on the step counts of 106 of the 257 draws, and at every
# tolerance from 1e-1 to 1e-8 on 3 to 199.  From 1e-9 on the steps are partly accuracy-limited and about 5 draws of a batch still sit
# within 1000 differences of errn = 1.  The issue's remedy for such a run is another tolerance or seed, not a smaller factor: 1e-9, and
# the first seed from 0 upward on which every draw passes tests/test_ode_adaptive_cpu.py: 985.  About one batch of 257 in 500 has no
# such draw; the run shows that the device follows the reference where the reference is well defined, not that DOPRI5 suits this system.
RUN_SEEDS = {("van_der_pol", "dopri5", 1e-9): 985}


def run_id(run):
    return f"{run[0]}-{run[1]}-{run[2]:g}"


def draws(case, S=BATCH, seed=0):
    return R0.draws(case, S, seed)


def run_draws(run, S=BATCH):
    """The draws of a run of RUNS: its case's, from the run's seed."""
    return R0.draws(CASES[run[0]], S, RUN_SEEDS.get(tuple(run), 0))


class Model:
    """f, J and T of one drift for a batch: f(t[n], X[n, D], TH[n, P]) -> [n, D] in the dtype of X; jac -> [n, D, D] with [s, i, k] =
    df_i/dx_k; ft -> [n, D]."""

    def __init__(self, name):
        import sympy as sp
        self.name = name
        if name in BUILTIN:
            d = drift_mod.builtin_drift(name)
            fn = orc.DRIFTS[name][0]
            self.f = lambda t, X, TH: np.asarray(fn(X, TH.T)[0], dtype=X.dtype)
        else:
            d = drift_mod.resolve(*TRACED[name])
            f_vec = TRACED[name][0]
            self.f = lambda t, X, TH: np.asarray(f_vec(t[:, None], X, TH.T[:, :, None]), dtype=X.dtype)
        self.D, self.P, self.time_dependent = d.D, d.P, bool(d.time_dependent)
        xs, ths, ts = sp.symbols(f"x0:{d.D}", real=True), sp.symbols(f"th0:{d.P}", real=True), sp.Symbol("t_magi", real=True)
        args = [ts] + list(xs) + list(ths)
        self._j = sp.lambdify(args, [sp.diff(e, x) for e in d.exprs for x in xs], modules="numpy")
        self._t = sp.lambdify(args, [sp.diff(e, ts) for e in d.exprs], modules="numpy")

    def _cols(self, fn, t, X, TH):
        a = [t] + [X[:, k] for k in range(self.D)] + [TH[:, k] for k in range(self.P)]
        return np.stack([np.broadcast_to(np.asarray(v, dtype=X.dtype), t.shape) for v in fn(*a)], axis=1)

    def jac(self, t, X, TH):
        return self._cols(self._j, t, X, TH).reshape(-1, self.D, self.D)

    def ft(self, t, X, TH):
        return self._cols(self._t, t, X, TH)


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(name)


def lu_factor(W):
    """Gaussian elimination with partial pivoting (the first row of largest |entry|) of a batch W[n, D, D]: (factors, pivots[n, D], ok[n]);
    multipliers stay at the rows they had when they were formed, lu_solve replays the exchanges.  ok: every pivot finite and not 0."""
    W = W.copy()
    n, D, _ = W.shape
    r = np.arange(n)
    piv = np.zeros((n, D), dtype=np.int64)
    ok = np.ones(n, dtype=bool)
    for k in range(D):
        p = k + np.argmax(np.abs(W[:, k:, k]), axis=1)
        piv[:, k] = p
        top = W[r, k, k:].copy()
        W[r, k, k:] = W[r, p, k:]
        W[r, p, k:] = top
        pv = W[:, k, k]
        ok &= (pv != 0) & np.isfinite(pv)
        l = W[:, k + 1:, k] / pv[:, None]
        W[:, k + 1:, k] = l
        W[:, k + 1:, k + 1:] = W[:, k + 1:, k + 1:] - l[:, :, None] * W[:, None, k, k + 1:]
    return W, piv, ok


def lu_solve(fac, b):
    W, piv, _ = fac
    b = b.copy()
    n, D = b.shape
    r = np.arange(n)
    for k in range(D):
        p = piv[:, k]
        top = b[:, k].copy()
        b[:, k] = b[r, p]
        b[r, p] = top
        b[:, k + 1:] = b[:, k + 1:] - W[:, k + 1:, k] * b[:, k:k + 1]
    for k in range(D - 1, -1, -1):
        s = b[:, k]
        for c in range(k + 1, D):
            s = s - W[:, k, c] * b[:, c]
        b[:, k] = s / W[:, k, k]
    return b


def _dopri5(m, dt, x, th, k1, t, ht, tn, variant):
    q = lambda a, b: dt(a) / dt(b)
    H = ht[:, None]
    k2 = m.f(t + q(1, 5) * ht, x + H * (q(1, 5) * k1), th)
    k3 = m.f(t + q(3, 10) * ht, x + H * (q(3, 40) * k1 + q(9, 40) * k2), th)
    k4 = m.f(t + q(4, 5) * ht, x + H * (q(44, 45) * k1 + q(-56, 15) * k2 + q(32, 9) * k3), th)
    k5 = m.f(t + q(8, 9) * ht, x + H * (q(19372, 6561) * k1 + q(-25360, 2187) * k2 + q(64448, 6561) * k3 + q(-212, 729) * k4), th)
    k6 = m.f(tn, x + H * (q(9017, 3168) * k1 + q(-355, 33) * k2 + q(46732, 5247) * k3 + q(49, 176) * k4 + q(-5103, 18656) * k5), th)
    b6 = q(11, 84) * (dt(1) + dt(1e-6)) if variant == "b_weight" else q(11, 84)
    xn = x + H * (q(35, 384) * k1 + q(500, 1113) * k3 + q(125, 192) * k4 + q(-2187, 6784) * k5 + b6 * k6)
    k7 = m.f(tn, xn, th)
    err = H * (q(71, 57600) * k1 + q(-71, 16695) * k3 + q(71, 1920) * k4 + q(-17253, 339200) * k5 + q(22, 525) * k6 + q(-1, 40) * k7)
    return xn, k7, err, np.ones(len(t), dtype=bool)


def _ros23(m, dt, x, th, F0, t, ht, tn, variant):
    r2 = np.sqrt(dt(2))
    d, e32 = dt(1) / (dt(2) + r2), dt(6) + r2 + (dt(1e-6) if variant == "e32" else dt(0))
    hd = ht * d
    J = m.jac(t, x, th)
    if variant == "J_transposed":
        J = J.transpose(0, 2, 1)
    fac = lu_factor(np.eye(m.D, dtype=dt)[None] - hd[:, None, None] * J)
    Tv = m.ft(t, x, th) if m.time_dependent and variant != "drop_T" else np.zeros_like(x)
    H, HD = ht[:, None], hd[:, None]
    k1 = lu_solve(fac, F0 + HD * Tv)
    F1 = m.f(t + dt(0.5) * ht, x + (dt(0.5) * H) * k1, th)
    k2 = lu_solve(fac, F1 - k1) + k1
    xn = x + H * k2
    F2 = m.f(tn, xn, th)
    k3 = lu_solve(fac, ((F2 - e32 * (k2 - F1)) - dt(2) * (k1 - F0)) + HD * Tv)
    err = (H / dt(6)) * ((k1 - dt(2) * k2) + k3)
    return xn, F2, err, fac[2]


def solve(name, x0, theta, t_out, method, rtol, atol=ATOL, h0=0.0, max_steps=MAX_STEPS, dtype=np.float64, variant=None, record=None):
    """dict(trajectories [S, T, D] in ``dtype``, status, reason, n_accepted, n_rejected [S]).  ``variant``: None or one of VARIANTS -- the
    T term dropped; e32 off by 1e-6; the weight b6 times (1 + 1e-6); the exponent 1 / (q - 1); the step accepted after a rejection allowed
    to grow; steps not clipped to the output times (an output is the state of the first step that ends at or behind it); J transposed.
    ``record``: a list that receives (draws[n], errn[n], finite[n]) of every round of trial steps."""
    assert method in METHODS and (variant is None or variant in VARIANTS), (method, variant)
    m, dt = model(name), dtype
    x, th = np.array(x0, dtype=dt), np.array(theta, dtype=dt)
    ts = np.asarray(t_out, dtype=np.float64).astype(dt)
    S, T = x.shape[0], len(ts)
    out = np.full((S, T, m.D), np.nan, dtype=dt)
    out[:, 0] = x
    rtol, atol = dt(rtol), dt(atol)
    t = np.full(S, ts[0], dtype=dt)
    h = np.full(S, dt(h0) if h0 > 0 else ts[1] - ts[0], dtype=dt)
    j, na, nr = (np.zeros(S, dtype=np.int64) for _ in range(3))
    fin = np.isfinite(x).all(axis=1)
    st, rs = np.where(fin, 0, 1), np.where(fin, 0, 1)
    rejected = np.zeros(S, dtype=bool)
    q = ORDER_Q[method] - (1 if variant == "wrong_q" else 0)
    expo = dt(-1) / dt(q)
    trial = _dopri5 if method == "dopri5" else _ros23
    with np.errstate(all="ignore"):
        F0 = m.f(t, x, th)
        active = fin.copy()
        while active.any():
            a = np.nonzero(active)[0]
            tend = ts[j[a] + 1]
            rem = tend - t[a]
            clip = (rem - h[a] < 16.0 * np.spacing(np.abs(tend).astype(np.float64))) if variant != "no_clip" else np.zeros(len(a), dtype=bool)
            ht = np.where(clip, rem, h[a])
            budget = na[a] + nr[a] >= max_steps
            under = ~budget & (ht < 16.0 * np.spacing(np.abs(t[a]).astype(np.float64)))
            for mask, why in ((budget, 2), (under, 3)):
                rs[a[mask]], st[a[mask]], active[a[mask]] = why, j[a[mask]] + 1, False
            go = ~(budget | under)
            a, tend, clip, ht = a[go], tend[go], clip[go], ht[go]
            if len(a) == 0:
                continue
            tn = np.where(clip, tend, t[a] + ht)
            xn, Fn, err, ok = trial(m, dt, x[a], th[a], F0[a], t[a], ht, tn, variant)
            r = np.abs(err) / (atol + rtol * np.maximum(np.abs(x[a]), np.abs(xn)))
            ok = ok & np.isfinite(r).all(axis=1) & np.isfinite(xn).all(axis=1)
            errn = np.fmax(np.fmax.reduce(r, axis=1), dt(0))
            if record is not None:
                record.append((a.copy(), errn.copy(), ok.copy()))
            fac = np.where(errn == 0, dt(5), np.minimum(dt(5), np.maximum(dt(0.2), dt(0.9) * errn ** expo)))
            acc = ok & (errn <= 1)
            rej = ok & ~acc
            # a non-finite trial or a singular W
            b = a[~ok]
            nr[b] += 1
            h[b] = ht[~ok] * dt(0.2)
            rejected[b] = True
            # rejected: the step shrinks
            b = a[rej]
            nr[b] += 1
            h[b] = ht[rej] * np.minimum(fac[rej], dt(1))
            rejected[b] = True
            # accepted
            b = a[acc]
            na[b] += 1
            fa = fac[acc] if variant == "reject_grows" else np.where(rejected[b], np.minimum(fac[acc], dt(1)), fac[acc])
            hn = ht[acc] * fa
            h[b] = np.where(clip[acc], np.maximum(h[b], hn), hn)
            rejected[b] = False
            t[b], x[b], F0[b] = tn[acc], xn[acc], Fn[acc]
            if variant == "no_clip":
                for s in b:
                    while j[s] + 1 < T and t[s] >= ts[j[s] + 1]:
                        j[s] += 1
                        out[s, j[s]] = x[s]
            else:
                c = b[clip[acc]]
                j[c] += 1
                out[c, j[c]] = x[c]
            active[b[j[b] + 1 >= T]] = False
    return {"trajectories": out, "status": st.astype(np.int32), "reason": rs.astype(np.int32), "n_accepted": na.astype(np.int32),
            "n_rejected": nr.astype(np.int32)}


@functools.lru_cache(maxsize=None)
def reference(name, method, rtol, dtype_name="float64", S=BATCH, variant=None, with_record=False):
    """The case's batch on its own grid, computed once per session and shared: treat it as read-only.  A draw's steps do not depend on
    the batch it is in: the reference of the first S' draws is the first S' rows."""
    case = CASES[name]
    x0, th = run_draws((name, method, rtol), S)
    record = [] if with_record else None
    out = solve(name, x0, th, case.t, method, rtol, dtype=getattr(np, dtype_name), variant=variant, record=record)
    for v in out.values():
        v.setflags(write=False)
    out["record"] = record
    return out


def bar(name, method, rtol):
    """The device bar of a run, as a fraction of max|x|: 64 times the float64-versus-longdouble distance of this reference on it (the
    rule of tests/test_elpd_gpu.py), at least FLOOR."""
    a, b = reference(name, method, rtol)["trajectories"], reference(name, method, rtol, "longdouble")["trajectories"]
    return max(64.0 * R0.distance(a, b), FLOOR)


def bars(got, name, method, rtol, rows=slice(None)):
    """max |got - float64 reference| over the draws ``rows``, in bars of the run."""
    want = reference(name, method, rtol)["trajectories"]
    return float(np.abs(got - want[rows]).max() / (bar(name, method, rtol) * np.abs(want).max()))
