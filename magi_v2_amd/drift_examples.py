"""Classic MAGI benchmark systems written the way a user of the reference writes ``f_vec`` (numpy in place of
tf.*): used by the tests of the generic-drift path and pre-built by ``__graft_entry__.build()``.  ``EXAMPLES`` ignore their first
argument; ``TIME_EXAMPLES`` are forced systems that use it; ``DOMAIN_EXAMPLES`` are defined on part of the state space only (a square root, a logarithm);
``EDGE_EXAMPLES`` sit at the documented shape limits (D = 1, 7, 8; P = 8) and at the edges of what the tracer prints and separates;
``SIGNED_EXAMPLES`` have parameters that are negative at the truth (supports of theta: ``predict(theta_support=...)``)."""
import numpy as np


def fitzhugh_nagumo(t, X, thetas):
    """FitzHugh-Nagumo: V' = c (V - V^3/3 + R),  R' = -(V - a + b R) / c;  theta = (a, b, c)."""
    V, R = X[:, 0:1], X[:, 1:2]
    a, b, c = thetas[0], thetas[1], thetas[2]
    return np.concatenate([c * (V - V ** 3 / 3.0 + R), -(V - a + b * R) / c], axis=1)


def lotka_volterra(t, X, thetas):
    """Predator-prey: x' = a x - b x y,  y' = d x y - c y;  theta = (a, b, c, d)."""
    x, y = X[:, 0:1], X[:, 1:2]
    return np.concatenate([thetas[0] * x - thetas[1] * x * y, thetas[3] * x * y - thetas[2] * y], axis=1)


def protein_transduction(t, X, thetas):
    """Protein signalling transduction (5 components S, dS, R, RS, Rpp; 6 parameters) -- the third benchmark of the MAGI paper."""
    S, dS, R, RS, Rpp = (X[:, k:k + 1] for k in range(5))
    k1, k2, k3, k4, V, Km = (thetas[k] for k in range(6))
    return np.concatenate([-k1 * S - k2 * S * R + k3 * RS,
                           k1 * S,
                           -k2 * S * R + k3 * RS + V * Rpp / (Km + Rpp),
                           k2 * S * R - k3 * RS - k4 * RS,
                           k4 * RS - V * Rpp / (Km + Rpp)], axis=1)


def competition_7(t, X, thetas):
    """Two-species competition with self-limitation and immigration: 7 parameters (exercises builds with more than 6)."""
    x, y = X[:, 0:1], X[:, 1:2]
    a, b, c, d, e, f, g = (thetas[k] for k in range(7))
    return np.concatenate([a * x - b * x * y - e * x ** 2, d * x * y - c * y - f * y ** 2 + g * x], axis=1)


EXAMPLES = {"fhn": (fitzhugh_nagumo, 2, 3), "lotka_volterra": (lotka_volterra, 2, 4), "ptrans": (protein_transduction, 5, 6),
            "competition7": (competition_7, 2, 7)}


def seir_seasonal(t, X, thetas):
    """SEIR with seasonal transmission (E, I, R; S = 1 - E - I - R implicit): beta(t) = beta (1 + a cos(pi t));  theta = (beta, gamma, sigma, a)."""
    E, I, R = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    S = 1.0 - E - I - R
    beta, gamma, sigma, a = (thetas[k] for k in range(4))
    return np.concatenate([beta * (1.0 + a * np.cos(np.pi * t)) * S * I - sigma * E, sigma * E - gamma * I, gamma * I], axis=1)


def fhn_forced(t, X, thetas):
    """Periodically driven FitzHugh-Nagumo: V' = c (V - V^3/3 + R) + A cos(0.8 t),  R' = -(V - a + b R) / c;  theta = (a, b, c, A)."""
    V, R = X[:, 0:1], X[:, 1:2]
    a, b, c, A = (thetas[k] for k in range(4))
    return np.concatenate([c * (V - V ** 3 / 3.0 + R) + A * np.cos(0.8 * t), -(V - a + b * R) / c], axis=1)


def mm_infusion(t, X, thetas):
    """Two compartments with a decaying infusion and saturable elimination:
    x' = th0 e^{-0.3 t} - th1 x / (th2 + x) - th3 (x - y),  y' = th3 (x - y)."""
    x, y = X[:, 0:1], X[:, 1:2]
    return np.concatenate([thetas[0] * np.exp(-0.3 * t) - thetas[1] * x / (thetas[2] + x) - thetas[3] * (x - y), thetas[3] * (x - y)], axis=1)


TIME_EXAMPLES = {"seir_seasonal": (seir_seasonal, 3, 4), "fhn_forced": (fhn_forced, 2, 4), "mm_infusion": (mm_infusion, 2, 4)}


def sqrt_outflow(t, X, thetas):
    """Torricelli outflow from one tank into a second, leaky one: x' = -a sqrt(x),  y' = b sqrt(x) - c y;  theta = (a, b, c).
    Defined for x >= 0 only.  Separable: coefficients a, b, c on the basis sqrt(x), y."""
    x, y = X[:, 0:1], X[:, 1:2]
    a, b, c = thetas[0], thetas[1], thetas[2]
    return np.concatenate([-a * np.sqrt(x), b * np.sqrt(x) - c * y], axis=1)


def gompertz_predation(t, X, thetas):
    """Gompertz growth under predation: x' = a x log(K / x) - b x y,  y' = c x - b y;  theta = (a, K, b, c).
    Defined for x > 0 only.  Not separable: log(K / x) mixes the state with the parameter K."""
    x, y = X[:, 0:1], X[:, 1:2]
    a, K, b, c = thetas[0], thetas[1], thetas[2], thetas[3]
    return np.concatenate([a * x * np.log(K / x) - b * x * y, c * x - b * y], axis=1)


# drifts with a limited domain: a leapfrog step that leaves it gives a NaN energy (tests/test_nonfinite_*.py)
DOMAIN_EXAMPLES = {"sqrt_outflow": (sqrt_outflow, 2, 3), "gompertz": (gompertz_predation, 2, 4)}


def logistic_1(t, X, thetas):
    """Logistic growth, ONE component: x' = r x (1 - x / K);  theta = (r, K).  Separable: coefficients r, r / K on the basis x, x^2."""
    x = X[:, 0:1]
    return thetas[0] * x * (1.0 - x / thetas[1])


def chain_8(t, X, thetas):
    """Linear cascade of eight compartments with a constant source and a saturating last link, 8 parameters:
    x0' = th0 - th1 x0,  xk' = thk x(k-1) - th(k+1) xk (k = 1..5),  x6' = th6 x5 - th7 x6 / (1 + x7^2),  x7' = th7 x6 / (1 + x7^2) - th1 x7.
    Separable: two basis functions per component, the source's a constant."""
    x = [X[:, k:k + 1] for k in range(8)]
    th = [thetas[k] for k in range(8)]
    link = th[7] * x[6] / (1.0 + x[7] ** 2)
    return np.concatenate([th[0] - th[1] * x[0]] + [th[k] * x[k - 1] - th[k + 1] * x[k] for k in range(1, 6)]
                          + [th[6] * x[5] - link, link - th[1] * x[7]], axis=1)


def cascade_7(t, X, thetas):
    """Seven-compartment cascade whose last link is Michaelis-Menten with its constant a parameter, 8 parameters:
    x0' = th0 - th1 x0,  xk' = thk x(k-1) - th(k+1) xk (k = 1..4),  x5' = th5 x4 - th6 x5 / (th7 + x5),  x6' = th6 x5 / (th7 + x5) - th1 x6.
    Not separable (th7 + x5 mixes the state with a parameter)."""
    x = [X[:, k:k + 1] for k in range(7)]
    th = [thetas[k] for k in range(8)]
    mm = th[6] * x[5] / (th[7] + x[5])
    return np.concatenate([th[0] - th[1] * x[0]] + [th[k] * x[k - 1] - th[k + 1] * x[k] for k in range(1, 5)]
                          + [th[5] * x[4] - mm, mm - th[1] * x[6]], axis=1)


def hill_powers(t, X, thetas):
    """A Hill term with its exponent a parameter beside powers of every kind the printer knows:
    x' = V y^n / (K^n + y^n) - d x^2.5 - 0.3 x^5 + pi / 10,  y' = d 2^x - V x^(1/3) y - 0.02 / y^6;  theta = (V, n, K, d).
    Defined for x, y > 0.  Not separable."""
    x, y = X[:, 0:1], X[:, 1:2]
    V, n, K, d = thetas[0], thetas[1], thetas[2], thetas[3]
    return np.concatenate([V * y ** n / (K ** n + y ** n) - d * x ** 2.5 - 0.3 * x ** 5 + np.pi / 10.0,
                           d * 2 ** x - V * x ** (1.0 / 3.0) * y - 0.02 * y ** -6], axis=1)


def mixed_3(t, X, thetas):
    """Three components that between them hold every shape of separable term:
    x' = a e^-x - b sin y + c tanh(x y) - e log(1 + x^2)                                  (four transcendental basis functions),
    y' = p - y + 2 p q x - p q x y + z^2 / 3 - (x / 7)^2 + 0.1 / (1 + y^2)                 (a constant term, a parameter-free group, a merged pair),
    z' = 0;  theta = (p, q, a, b, c, e)."""
    x, y, z = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    p, q, a, b, c, e = (thetas[k] for k in range(6))
    return np.concatenate([a * np.exp(-x) - b * np.sin(y) + c * np.tanh(x * y) - e * np.log(1.0 + x ** 2),
                           p - y + 2.0 * p * q * x - p * q * x * y + np.square(z) / 3 - (x / 7) ** 2 + 0.1 * np.reciprocal(1.0 + y ** 2),
                           0.0 * x], axis=1)


def five_terms(t, X, thetas):
    """A component with five separable terms (one more than the separable kernels carry): x' = a x + b y + c x y + d x^2 + e y^2,  y' = -a y."""
    x, y = X[:, 0:1], X[:, 1:2]
    a, b, c, d, e = (thetas[k] for k in range(5))
    return np.concatenate([a * x + b * y + c * x * y + d * x ** 2 + e * y ** 2, -a * y], axis=1)


# the documented shape limits (D = 1, 7, 8; P = 8) and the printer's and the separator's vocabulary (tests/test_drift_edges_*.py)
EDGE_EXAMPLES = {"logistic1": (logistic_1, 1, 2), "chain8": (chain_8, 8, 8), "cascade7": (cascade_7, 7, 8), "hill_pow": (hill_powers, 2, 4),
                 "mixed3": (mixed_3, 3, 6)}
# traced on the CPU only: no library is built for it
EDGE_TRACE_ONLY = {"five_term": (five_terms, 2, 5)}


def linear_oscillator(t, X, thetas):
    """Damped linear oscillator: x' = a y,  y' = b x + c y;  theta = (a, b, c).  A restoring force (b < 0) and a damping (c < 0): parameters
    the reference's positivity rule cannot reach -- sampled with ``predict(theta_support=["positive", "real", "real"])``."""
    x, y = X[:, 0:1], X[:, 1:2]
    return np.concatenate([thetas[0] * y, thetas[1] * x + thetas[2] * y], axis=1)


# systems with parameters of either sign (tests/test_support_*.py)
SIGNED_EXAMPLES = {"linear_oscillator": (linear_oscillator, 2, 3)}


def robertson(t, X, thetas):
    """Robertson's chemical kinetics: a' = -k1 a + k3 b c,  b' = k1 a - k3 b c - k2 b^2,  c' = k2 b^2;  theta = (k1, k2, k3), classically
    (0.04, 3e7, 1e4) from (1, 0, 0).  Stiff: rates nine orders of magnitude apart."""
    a, b, c = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    k1, k2, k3 = thetas[0], thetas[1], thetas[2]
    return np.concatenate([-k1 * a + k3 * b * c, k1 * a - k3 * b * c - k2 * b ** 2, k2 * b ** 2], axis=1)


def van_der_pol(t, X, thetas):
    """Van der Pol oscillator: x' = y,  y' = mu (1 - x^2) y - x;  theta = (mu,).  A relaxation oscillator, stiff for large mu."""
    x, y = X[:, 0:1], X[:, 1:2]
    return np.concatenate([y, thetas[0] * (1.0 - x ** 2) * y - x], axis=1)


def forced_relaxation(t, X, thetas):
    """Fast relaxation onto a slow forcing, with the forcing's phase as a second component: x' = -k (x - cos(w t)),  p' = w;
    theta = (k, w).  Time-dependent; stiff for large k."""
    x = X[:, 0:1]
    k, w = thetas[0], thetas[1]
    return np.concatenate([-k * (x - np.cos(w * t)), w + 0.0 * x], axis=1)


# stiff systems (adaptive integrators of csrc/ode_adaptive.hip: MagiEngine.ode_solve(method="ros23" / "dopri5"); tests/test_ode_adaptive_*.py)
STIFF_EXAMPLES = {"robertson": (robertson, 3, 3), "van_der_pol": (van_der_pol, 2, 1), "forced_relaxation": (forced_relaxation, 2, 2)}


def rk4(f_vec, x0, thetas, T, n, substeps=20, grid=None):
    """Reference trajectory on a uniform grid of n points over [0, T], or on ``grid`` (increasing times, its first the start): test data
    only.  The drift is given the current time."""
    x = np.asarray(x0, dtype=np.float64)
    out = [x.copy()]
    ts = np.linspace(0.0, T, n) if grid is None else np.asarray(grid, dtype=np.float64).reshape(-1)
    f = lambda s, v: f_vec(np.array([[s]]), v[None], thetas)[0]
    for i in range(len(ts) - 1):
        h = T / (n - 1) / substeps if grid is None else (ts[i + 1] - ts[i]) / substeps
        for j in range(substeps):
            s = ts[i] + j * h
            k1 = f(s, x); k2 = f(s + 0.5 * h, x + 0.5 * h * k1); k3 = f(s + 0.5 * h, x + 0.5 * h * k2); k4 = f(s + h, x + h * k3)
            x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        out.append(x.copy())
    return ts, np.array(out)
