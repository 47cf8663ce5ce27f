"""GP conditioning of trajectory draws restated in numpy (tests only): what include/magi_hip.h defines for magi_matern_cross,
magi_gp_predict and magi_sampler_gp_predict, and the derived bars the tests hold the device to.

Per component, with Ks = k(t_new, I), pKs = d k / d t* (t_new, I), C^-1 an ARGUMENT (used as given: rows of Ks times columns of C^-1):
    W = Ks C^-1,  Wd = pKs C^-1
    x_new  = mu + W (x - mu),        dx_new   = Wd (x - mu)
    var    = phi1 - sum_k W Ks,      dvar     = nu phi1 / (phi2^2 (nu - 1)) - sum_k Wd pKs          (UNclamped here; the device clamps at 0)
The device forms x_new as sum_k W x + mu (1 - sum_k W): the difference to the form above is rounding of the second inner product on
|W| |x| instead of |W| |x - mu|, far inside the bar below, which is dominated by its first product (|Ks| |C^-1| is orders of magnitude
above |W|: C^-1 = Kappa^-1 has entries of the size of cond(Kappa)).

The bar is the entry-wise forward bound of two chained inner products of length N in float64 (unit round-off 2^-53), with c = 8:
    bar_x[s, m]  = c (N + 4) 2^-53 [(|Ks| |C^-1|) |x - mu|][m, s] + c 2^-53 |mu|            (dx: pKs for Ks, no mu term)
    bar_var[m]   = c (N + 4) 2^-53 (sum_k (|Ks| |C^-1|)[m, k] |Ks[m, k]| + phi1)            (dvar: pKs and diag_pp)
computed in longdouble from the same inputs."""
import numpy as np

from oracle import magi_oracle as orc

U = 2.0 ** -53
C_BAR = 8.0


def diag_pp(phi1, phi2, nu=2.01):
    return nu * phi1 / (phi2 ** 2 * (nu - 1.0))


def cross_blocks(I, t_new, phi1, phi2, nu=2.01):
    """(Ks, pKs), each [T, N]: the oracle's accurate Matern columns on the concatenated grid [I, t_new], rows N.., columns 0..N.  The oracle
    marks its diagonal by INDEX and gives 0 where two different indices hold the same time: entries with t_new[m] == I[j] are set to the
    coincident values (phi1, 0)."""
    I, t_new = np.asarray(I, dtype=np.float64).reshape(-1), np.asarray(t_new, dtype=np.float64).reshape(-1)
    N = I.shape[0]
    Kap, pK, _ = orc.matern_block_columns_accurate(np.concatenate([I, t_new]), np.arange(N), phi1, phi2, nu)
    Ks, pKs = Kap[N:].copy(), pK[N:].copy()
    same = t_new[:, None] == I[None, :]
    Ks[same] = phi1
    pKs[same] = 0.0
    return Ks, pKs


def predict_component(Ks, pKs, C_inv, X, mu, phi1, dpp, dtype=np.longdouble):
    """One component: X [S, N] -> (x_new [S, T], dx_new [S, T], var [T], dvar [T]), every product in ``dtype``."""
    Ks, pKs, C_inv, X = (np.asarray(a, dtype=dtype) for a in (Ks, pKs, C_inv, X))
    mu = dtype(mu)
    W, Wd = Ks @ C_inv, pKs @ C_inv
    xc = (X - mu).T                                      # [N, S]
    return (mu + (W @ xc).T, (Wd @ xc).T, dtype(phi1) - (W * Ks).sum(axis=1), dtype(dpp) - (Wd * pKs).sum(axis=1))


def bars_component(Ks, pKs, C_inv, X, mu, phi1, dpp):
    """The bars of predict_component's four outputs, same shapes, in longdouble."""
    L = np.longdouble
    aK, aP, aC = np.abs(np.asarray(Ks, dtype=L)), np.abs(np.asarray(pKs, dtype=L)), np.abs(np.asarray(C_inv, dtype=L))
    N = aC.shape[0]
    f = L(C_BAR) * (N + 4) * L(U)
    G, Gd = aK @ aC, aP @ aC
    axc = np.abs(np.asarray(X, dtype=L) - L(mu)).T
    return (f * (G @ axc).T + L(C_BAR) * L(U) * abs(L(mu)), f * (Gd @ axc).T, f * ((G * aK).sum(axis=1) + L(phi1)), f * ((Gd * aP).sum(axis=1) + L(dpp)))


def _stack(parts):
    """per-component tuples of ([S, T], [S, T], [T], [T]) -> ([S, T, D], [S, T, D], [T, D], [T, D])"""
    return tuple(np.stack([p[i] for p in parts], axis=-1) for i in range(4))


def predict(Ks, pKs, C_inv, X, mu, phi1s, phi2s, nu=2.01, dtype=np.longdouble):
    """All components: Ks, pKs [D, T, N], C_inv [D, N, N], X [S, N, D] -> (x_new, dx_new [S, T, D], var, dvar [T, D]) in ``dtype``."""
    D = len(phi1s)
    return _stack([predict_component(Ks[d], pKs[d], C_inv[d], X[:, :, d], mu[d], phi1s[d], diag_pp(phi1s[d], phi2s[d], nu), dtype) for d in range(D)])


def bars(Ks, pKs, C_inv, X, mu, phi1s, phi2s, nu=2.01):
    D = len(phi1s)
    return _stack([bars_component(Ks[d], pKs[d], C_inv[d], X[:, :, d], mu[d], phi1s[d], diag_pp(phi1s[d], phi2s[d], nu)) for d in range(D)])


def new_times(I, n_uniform=127, grid_points=(0, 57, -1)):
    """The T = n_uniform + 3 times of the tests: n_uniform uniform in [min I - 0.1, max I + 0.1], then three exact grid times (entries of
    I by index, so they coincide with grid times bit for bit); (t_new, the indices into I of the last three)."""
    I = np.asarray(I, dtype=np.float64).reshape(-1)
    idx = [int(np.arange(len(I))[g]) for g in grid_points]
    return np.concatenate([np.linspace(I.min() - 0.1, I.max() + 0.1, n_uniform), I[idx]]), idx


def smooth_draws(I, S, D, mu, seed):
    """S smooth-plus-noise draws [S, N, D] around mu: one sinusoid per (draw, component) in the time, plus 1 % i.i.d. noise."""
    I = np.asarray(I, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(seed)
    amp, w, ph = rng.uniform(0.2, 0.5, (S, 1, D)), rng.uniform(0.5, 2.0, (S, 1, D)), rng.uniform(0.0, 2.0 * np.pi, (S, 1, D))
    return np.asarray(mu)[None, None, :] + amp * np.sin(w * I[None, :, None] + ph) + 0.01 * rng.standard_normal((S, len(I), D))
