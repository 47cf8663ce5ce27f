"""Host-side (numpy) pieces of the reference's pipeline that surround the GPU hot path.

These are O(N*D) preprocessing steps that run once per fit plus
the state transforms at the predict() boundary.  Each function cites the reference lines it
mirrors (relative to the reference tree).  Nothing here evaluates the log posterior, builds
kernel matrices or samples -- those exist only as HIP kernels (magi_v2_amd/csrc).
"""
from __future__ import annotations

import warnings
from typing import Callable, Dict, Optional, Tuple

import numpy as np
from scipy.interpolate import splev, splrep

# --------------------------------------------------------------------------------------------
# grid / interpolation / smoothing
# --------------------------------------------------------------------------------------------


def discretize(ts_obs: np.ndarray, X_obs: np.ndarray, discretization: int):
    """magi_v2.py:475-498 -- 2^k - 1 evenly spaced points between consecutive observations."""
    ts_obs = np.asarray(ts_obs, dtype=np.float64).flatten()
    assert ts_obs.shape[0] == X_obs.shape[0], \
        "Please make sure there are equal numbers of observations in ts_obs and X_obs."
    N, D = X_obs.shape
    stride = 2 ** discretization
    n_grid = stride * (N - 1) + 1
    I = np.full((n_grid,), np.nan)
    I[::stride] = ts_obs
    pos = np.arange(n_grid)
    known = ~np.isnan(I)
    I = np.interp(x=pos, xp=pos[known], fp=I[known]).reshape(-1, 1)
    X_grid = np.full((n_grid, D), np.nan)
    X_grid[::stride] = X_obs
    return I, X_grid


def linear_interpolate(X_partial: np.ndarray) -> np.ndarray:
    """magi_v2.py:509-527 -- per-column linear fill of NaNs (all-NaN columns stay NaN)."""
    out = X_partial.copy()
    pos = np.arange(X_partial.shape[0])
    for d in range(X_partial.shape[1]):
        missing = np.isnan(X_partial[:, d])
        if missing.any():
            out[:, d] = np.interp(x=pos, xp=pos[~missing], fp=X_partial[~missing, d])
    return out


def cubic_smoother(I: np.ndarray, X_filled: np.ndarray) -> np.ndarray:
    """magi_v2.py:695-770.  The reference cross-validates the knot count and then fits with the
    loop variable left over from that search, i.e. always len(I)//10 interior knots
    (magi_v2.py:747-757); the CV therefore has no effect on the result and is not repeated."""
    t = np.asarray(I, dtype=np.float64).flatten()
    if t.shape[0] < 10:
        return X_filled
    n_knots = t.shape[0] // 10
    knots = np.linspace(t[0], t[-1], n_knots + 2)[1:-1] if n_knots > 0 else np.array([])
    return np.stack([splev(t, splrep(t, X_filled[:, d], t=knots, s=0)) for d in range(X_filled.shape[1])], axis=1)


# --------------------------------------------------------------------------------------------
# hyper-parameter starting values
# --------------------------------------------------------------------------------------------


def fourier_phi2_prior(x: np.ndarray) -> Tuple[float, float]:
    """magi_v2.py:552-556 -- spectral-centroid prior mean / sd for the Matern length scale."""
    power = np.abs(np.fft.fft(x))
    power = power[1:(len(power) - 1) // 2 + 1] ** 2
    k = np.linspace(1, len(power), len(power))
    mean = 0.5 / (np.sum(k * power) / np.sum(power))
    return mean, (1 - mean) / 3


def hparams_initial(X_filled: np.ndarray) -> Dict[str, np.ndarray]:
    """The values the reference initialises its hyper-parameter fit with (magi_v2.py:631-639):
    phi1 = var, phi2 = Fourier prior mean, sigma^2 = (0.1 std)^2."""
    sd = X_filled.std(axis=0)
    return {"phi1s": sd ** 2,
            "phi2s": np.array([fourier_phi2_prior(X_filled[:, d])[0] for d in range(X_filled.shape[1])]),
            "sigma_sqs": (sd * 0.1) ** 2}


# --------------------------------------------------------------------------------------------
# predict() boundary
# --------------------------------------------------------------------------------------------


def sigma_sqs_lower_bound(Xhat_init: np.ndarray) -> np.ndarray:
    """magi_v2.py:299-300."""
    return (Xhat_init.std(axis=0) * 0.01) ** 2


def softplus_inverse_inits(sigma_sqs_init, thetas_init, LB):
    """magi_v2.py:374-380 (with the -5.0 fallback)."""
    sig_pre = np.full_like(sigma_sqs_init, -5.0)
    ok = sigma_sqs_init > LB
    sig_pre[ok] = np.log(np.exp((sigma_sqs_init - LB)[ok]) - 1.0)
    th_pre = np.full_like(thetas_init, -5.0)
    ok = thetas_init > 0.0
    th_pre[ok] = np.log(np.exp(thetas_init[ok]) - 1.0)
    return sig_pre, th_pre


def transform_samples(sig_pre, th_pre, LB, sigma_sq_prior=None):
    """magi_v2.py:418-419.  ``sigma_sq_prior``: None or the (kinds, a, b) of ``prior_spec(..., "sigma_sq")`` -- a component whose noise variance is
    fixed reports that constant, whatever its ``pre`` coordinate is."""
    sig = np.log(np.exp(sig_pre) + 1.0) + LB
    if sigma_sq_prior is not None:
        kinds, a, _ = sigma_sq_prior
        sig = np.where(np.asarray(kinds) == PRIOR_FIXED, np.asarray(a, dtype=np.float64), sig)
    return sig, np.log(np.exp(th_pre) + 1.0)


# supports of the ODE parameters (include/magi_hip.h: magi_set_theta_support).  The codes are the header's MAGI_THETA_*.
THETA_POSITIVE, THETA_LOWER, THETA_UPPER, THETA_REAL = 0, 1, 2, 3


def theta_support(spec, P: int):
    """Normalises a support specification for P parameters into (kinds int32[P], bounds float64[P]).  ``spec`` is None (every
    parameter positive: the reference's rule, magi_v2.py:303-306, 319) or P entries out of "positive", "real", ("lower", lo),
    ("upper", hi) with finite bounds; anything else raises ValueError.  The bound of a positive or real entry is 0."""
    P = int(P)
    kinds, bounds = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    if spec is None:
        return kinds, bounds
    if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__"):
        raise ValueError(f"theta_support: expected None or a sequence of {P} entries, got {spec!r}")
    if len(spec) != P:
        raise ValueError(f"theta_support: {len(spec)} entries for {P} parameters")
    for p, e in enumerate(spec):
        if isinstance(e, str):
            if e == "positive":
                continue
            if e == "real":
                kinds[p] = THETA_REAL
                continue
            raise ValueError(f"theta_support[{p}]: {e!r} is none of 'positive', 'real', ('lower', lo), ('upper', hi)")
        if isinstance(e, (tuple, list)) and len(e) == 2 and e[0] in ("lower", "upper"):
            try:
                b = float(e[1])
            except (TypeError, ValueError):
                raise ValueError(f"theta_support[{p}]: the bound {e[1]!r} is not a number") from None
            if not np.isfinite(b):
                raise ValueError(f"theta_support[{p}]: the bound {b} is not finite")
            kinds[p] = THETA_LOWER if e[0] == "lower" else THETA_UPPER
            bounds[p] = b
            continue
        raise ValueError(f"theta_support[{p}]: {e!r} is none of 'positive', 'real', ('lower', lo), ('upper', hi)")
    return kinds, bounds


def theta_support_spec(kinds, bounds):
    """The normalised specification (a list of "positive", "real", ("lower", lo), ("upper", hi)) of (kinds, bounds)."""
    names = {THETA_POSITIVE: "positive", THETA_REAL: "real"}
    return [names[int(k)] if int(k) in names else ("lower" if int(k) == THETA_LOWER else "upper", float(b)) for k, b in zip(kinds, bounds)]


def theta_pre_inits(thetas_init, kinds, bounds):
    """theta_pre of the starting values under the supports: theta itself for a real parameter, the softplus inverse of the distance to
    the bound for a bounded one -- with the reference's -5.0 fallback (magi_v2.py:374-380) when the value lies on the wrong side of the
    bound -- and for a positive one exactly what softplus_inverse_inits gives."""
    th = np.asarray(thetas_init, dtype=np.float64)
    kinds, bounds = np.asarray(kinds), np.asarray(bounds, dtype=np.float64)
    # the distance to the bound (theta itself for a positive parameter: th - 0.0 is th bit for bit)
    dist = np.where(kinds == THETA_UPPER, bounds - th, np.where(kinds == THETA_LOWER, th - bounds, th))
    ok = dist > 0.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pre = np.where(ok, np.log(np.exp(np.where(ok, dist, 1.0)) - 1.0), -5.0)
    return np.where(kinds == THETA_REAL, th, pre)


def transform_thetas(th_pre, kinds, bounds):
    """theta on the natural scale from theta_pre[..., P] under the supports (for a positive parameter: transform_samples)."""
    th_pre = np.asarray(th_pre, dtype=np.float64)
    kinds, bounds = np.asarray(kinds), np.asarray(bounds, dtype=np.float64)
    with np.errstate(over="ignore"):
        sp = np.log(np.exp(th_pre) + 1.0)
    out = np.where(kinds == THETA_LOWER, bounds + sp, np.where(kinds == THETA_UPPER, bounds - sp, sp))
    return np.where(kinds == THETA_REAL, th_pre, out)


# priors of the parameter entries (include/magi_hip.h: magi_set_prior).  The codes are the header's MAGI_PRIOR_*.
PRIOR_FLAT, PRIOR_NORMAL, PRIOR_LOGNORMAL, PRIOR_GAMMA, PRIOR_INVGAMMA, PRIOR_FIXED = 0, 1, 2, 3, 4, 5
_PRIOR_NAMES = {"normal": PRIOR_NORMAL, "lognormal": PRIOR_LOGNORMAL, "gamma": PRIOR_GAMMA, "invgamma": PRIOR_INVGAMMA}
_PRIOR_POSITIVE = (PRIOR_LOGNORMAL, PRIOR_GAMMA, PRIOR_INVGAMMA)          # densities on (0, inf)


def prior_spec(spec, n: int, which: str, support=None):
    """Normalises a prior specification for the n entries of one block into (kinds int32[n], a float64[n], b float64[n]).  ``which`` is
    "sigma_sq" or "theta".  ``spec`` is None (every prior flat, the reference's posterior) or n entries out of None / "flat",
    ("normal", m, s), ("lognormal", m, s), ("gamma", k, r), ("invgamma", a, b) and, for sigma_sq only, ("fixed", c): all parameters finite;
    s, k, r, a, b, c > 0.  ``support`` (theta only): the (kinds, bounds) of ``theta_support`` -- lognormal, gamma and invgamma need a
    support inside (0, inf): positive, or lower with lo >= 0.  Anything else raises ValueError.  b of a fixed entry is 0."""
    if which not in ("sigma_sq", "theta"):
        raise ValueError(f"prior_spec: which = {which!r} is neither 'sigma_sq' nor 'theta'")
    n = int(n)
    name = which + "_prior"
    kinds, a, b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    if spec is None:
        return kinds, a, b
    if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__"):
        raise ValueError(f"{name}: expected None or a sequence of {n} entries, got {spec!r}")
    if len(spec) != n:
        raise ValueError(f"{name}: {len(spec)} entries for {n} parameters")
    known = "None, 'flat', ('normal', m, s), ('lognormal', m, s), ('gamma', k, r), ('invgamma', a, b)" + (", ('fixed', c)" if which == "sigma_sq" else "")
    for j, e in enumerate(spec):
        if e is None or (isinstance(e, str) and e == "flat"):
            continue
        if not isinstance(e, (tuple, list)) or len(e) < 1 or not isinstance(e[0], str):
            raise ValueError(f"{name}[{j}]: {e!r} is none of {known}")
        if e[0] == "fixed":
            if which != "sigma_sq":
                raise ValueError(f"{name}[{j}]: 'fixed' is for noise variances only (a constant in f_vec states a fixed parameter)")
            want = 1
        elif e[0] in _PRIOR_NAMES:
            want = 2
        else:
            raise ValueError(f"{name}[{j}]: {e!r} is none of {known}")
        if len(e) != 1 + want:
            raise ValueError(f"{name}[{j}]: {e[0]!r} takes {want} parameter(s), got {len(e) - 1}")
        try:
            v = [float(x) for x in e[1:]]
        except (TypeError, ValueError):
            raise ValueError(f"{name}[{j}]: the parameters of {e!r} are not numbers") from None
        if not all(np.isfinite(v)):
            raise ValueError(f"{name}[{j}]: the parameters of {e!r} are not finite")
        k = PRIOR_FIXED if e[0] == "fixed" else _PRIOR_NAMES[e[0]]
        if not v[-1] > 0.0 or (k in (PRIOR_GAMMA, PRIOR_INVGAMMA) and not v[0] > 0.0):
            raise ValueError(f"{name}[{j}]: sd, shape, rate, scale and a fixed value must be > 0, got {e!r}")
        if which == "theta" and k in _PRIOR_POSITIVE and support is not None:
            sk, sb = int(np.asarray(support[0])[j]), float(np.asarray(support[1])[j])
            if not (sk == THETA_POSITIVE or (sk == THETA_LOWER and sb >= 0.0)):
                raise ValueError(f"{name}[{j}]: a {e[0]} prior needs a support inside (0, inf): 'positive', or ('lower', lo) with lo >= 0")
        kinds[j], a[j], b[j] = k, v[0], (0.0 if k == PRIOR_FIXED else v[1])
    return kinds, a, b


def prior_spec_echo(kinds, a, b):
    """The normalised specification (a list of "flat", ("normal", m, s), ..., ("fixed", c)) of (kinds, a, b)."""
    names = {v: k for k, v in _PRIOR_NAMES.items()}
    return ["flat" if int(k) == PRIOR_FLAT else ("fixed", float(x)) if int(k) == PRIOR_FIXED else (names[int(k)], float(x), float(y))
            for k, x, y in zip(kinds, a, b)]


# observation model (include/magi_hip.h: magi_set_obs_model).  The codes are the header's MAGI_LINK_*.
LINK_IDENTITY, LINK_LOG, LINK_SQRT = 0, 1, 2
_LINK_NAMES = {"identity": LINK_IDENTITY, "log": LINK_LOG, "sqrt": LINK_SQRT}


def obs_model_spec(link, D: int):
    """Normalises a link specification into codes int32[D]: None (every link the identity, the reference's model), one of "identity",
    "log", "sqrt" for all D components, or one such name (or None, or a LINK_* code) per component.  Anything else raises ValueError."""
    D = int(D)
    links = np.zeros(D, dtype=np.int32)
    if link is None:
        return links
    if isinstance(link, str):
        link = [link] * D
    if isinstance(link, bytes) or not hasattr(link, "__len__"):
        raise ValueError(f"obs_link: expected None, a link name or a sequence of {D} entries, got {link!r}")
    if len(link) != D:
        raise ValueError(f"obs_link: {len(link)} entries for {D} components")
    for d, e in enumerate(link):
        if e is None:
            continue
        if isinstance(e, str) and e in _LINK_NAMES:
            links[d] = _LINK_NAMES[e]
        elif isinstance(e, (int, np.integer)) and not isinstance(e, bool) and int(e) in _LINK_NAMES.values():
            links[d] = int(e)
        else:
            raise ValueError(f"obs_link[{d}]: {e!r} is none of None, 'identity', 'log', 'sqrt'")
    return links


def obs_model_spec_echo(links):
    """The normalised specification (a list of "identity" / "log" / "sqrt") of link codes."""
    names = {v: k for k, v in _LINK_NAMES.items()}
    return [names[int(k)] for k in links]


def link_apply(link: int, v):
    """g(v) of one link code, elementwise (NaN outside the link's domain; -inf for log 0)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(v) if int(link) == LINK_LOG else np.sqrt(v) if int(link) == LINK_SQRT else v.copy()


def link_domain(link: int, v):
    """Whether v lies in the domain of the link: log v > 0, sqrt v >= 0, identity anything finite or not."""
    v = np.asarray(v, dtype=np.float64)
    return v > 0.0 if int(link) == LINK_LOG else v >= 0.0 if int(link) == LINK_SQRT else np.ones(v.shape, dtype=bool)


def obs_weight_grid(obs_weight, X_grid: np.ndarray):
    """``obs_weight`` (shaped like the observed data on the grid, [n_points, D]) as float64 with 1 at unobserved positions, whose entries
    are ignored; every weight at an observed position must be finite and > 0.  None stays None."""
    if obs_weight is None:
        return None
    w = np.asarray(obs_weight, dtype=np.float64)
    if w.shape != X_grid.shape:
        raise ValueError(f"obs_weight: shape {w.shape}, the observed data on the grid have shape {X_grid.shape}")
    seen = ~np.isnan(X_grid)
    if not np.all(np.isfinite(w[seen]) & (w[seen] > 0.0)):
        raise ValueError("obs_weight: every weight of an observed point must be a finite number > 0")
    return np.where(seen, w, 1.0)


def link_start_check(links, X_grid: np.ndarray, Xhat_init: np.ndarray):
    """Raises ValueError when the data or the start state leave a link's domain at an observed point: a chain started there starts at NaN."""
    for d, k in enumerate(links):
        seen = ~np.isnan(X_grid[:, d])
        bad_y = int((~link_domain(k, X_grid[seen, d])).sum())
        if bad_y:
            raise ValueError(f"obs_link: component {d} has {bad_y} observation(s) outside the domain of its {obs_model_spec_echo([k])[0]} link")
        bad = int((~link_domain(k, np.asarray(Xhat_init)[seen, d])).sum())
        if bad:
            raise ValueError(f"obs_link: Xhat_init of component {d} is outside the domain of its {obs_model_spec_echo([k])[0]} link at {bad} observed point(s): "
                             "the chain would start at a non-finite log posterior")


def link_sigma_defaults(links, X_grid: np.ndarray, Xhat_init: np.ndarray, weight_grid, LB, sigma_sqs_init, LB_given: bool):
    """sigma^2 lives on the link's scale, where the natural-scale defaults are wrong by orders of magnitude.  For every component with a link
    other than the identity: the lower bound becomes (0.01 std(g(y_d)))^2 unless ``LB_given``, and the starting value the weighted mean square
    of g(Xhat_init) - g(y) over the observed points where Xhat_init lies in the link's domain -- or (0.1 std(g(y_d)))^2 when fewer than two
    such points exist or the mean square is not above the bound.  Identity components keep ``LB`` and ``sigma_sqs_init``.
    Returns (LB, sigma_sqs_start)."""
    LB = np.array(LB, dtype=np.float64)
    start = np.array(sigma_sqs_init, dtype=np.float64)
    for d, k in enumerate(links):
        if int(k) == LINK_IDENTITY:
            continue
        seen = ~np.isnan(X_grid[:, d])
        gy = link_apply(k, X_grid[seen, d])
        sd = gy.std() if gy.size else 0.0
        if not LB_given:
            LB[d] = (0.01 * sd) ** 2
        xs = np.asarray(Xhat_init, dtype=np.float64)[seen, d]
        ok = link_domain(k, xs) & np.isfinite(link_apply(k, xs))
        w = np.ones(gy.shape) if weight_grid is None else np.asarray(weight_grid)[seen, d]
        ms = -1.0
        if int(ok.sum()) >= 2:
            ms = float(np.sum(w[ok] * (link_apply(k, xs[ok]) - gy[ok]) ** 2) / np.sum(w[ok]))
        start[d] = ms if ms > LB[d] else (0.1 * sd) ** 2
    return LB, start


def observation_bookkeeping(X_obs: np.ndarray, X_grid: np.ndarray):
    """magi_v2.py:53, 89, 96-100: N_ds, beta, flat indices and values of the non-NaN grid entries."""
    N_ds = (~np.isnan(X_obs)).sum(axis=0)
    n_grid, D = X_grid.shape
    beta = (D * n_grid) / N_ds.sum()
    idx = np.where(~np.isnan(X_grid).flatten())[0]
    return N_ds, beta, idx, X_grid.reshape(-1)[idx]


# --------------------------------------------------------------------------------------------
# pointwise log-likelihood, WAIC, PSIS-LOO: the host side (the statistics themselves are the device's, csrc/elpd.hip)
# --------------------------------------------------------------------------------------------

ELPD_POINTWISE = ("lpd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "khat")       # the order of the six outputs in include/magi_hip.h
ELPD_TOTALS = ("elpd_waic", "elpd_loo", "p_waic", "p_loo")
KHAT_BAD = 0.7
ELPD_LOO_MAX_DRAWS = 466033          # pooled draws per observation up to which the device serves PSIS-LOO (include/magi_hip.h: magi_elpd)


def elpd_result(pointwise, obs_index=None, n_nonfinite=0, loglik=None, shift=None, scale="link"):
    """The dictionary ``MagiEngine.elpd`` / ``sampler_elpd`` / ``MAGI_v2.posterior_elpd`` return, from the device's pointwise arrays
    (``pointwise``: name -> [n] for the names of ELPD_POINTWISE; an entry may be None when it was not asked for).  ``shift`` [n]: a
    per-observation constant added to lpd, elpd_waic and elpd_loo (``elpd_jacobian``).  Holds ``pointwise`` (the arrays), ``obs_index``
    ([n, 2] pairs (i, d): grid point, component; None for a plain log-likelihood array), ``n_obs``, ``n_nonfinite``, ``scale``, the totals
    ``elpd_waic``, ``elpd_loo``, ``p_waic``, ``p_loo`` -- sums over the observations -- each with its standard error ``se_<name>`` =
    sqrt(n var_i) (ddof = 1), ``n_khat_bad`` (observations with khat > 0.7: their elpd_loo is not reliable) and, when given, ``loglik``."""
    point = {}
    for s in ELPD_POINTWISE:
        v = pointwise.get(s)
        if v is None:
            point[s] = None
            continue
        v = np.array(v, dtype=np.float64)
        if shift is not None and s in ("lpd", "elpd_waic", "elpd_loo"):
            v = v + np.asarray(shift, dtype=np.float64)
        point[s] = v
    n = int(next(v.shape[0] for v in point.values() if v is not None))
    out = {"pointwise": point, "obs_index": None if obs_index is None else np.asarray(obs_index, dtype=np.int64).reshape(-1, 2),
           "n_obs": n, "n_nonfinite": int(n_nonfinite), "scale": scale}
    for s in ELPD_TOTALS:
        v = point[s]
        if v is None:
            out[s] = out["se_" + s] = None
            continue
        out[s] = float(v.sum())
        out["se_" + s] = float(np.sqrt(n * v.var(ddof=1))) if n >= 2 else float("nan")
    out["n_khat_bad"] = None if point["khat"] is None else int((point["khat"] > KHAT_BAD).sum())
    if loglik is not None:
        out["loglik"] = loglik
    return out


def elpd_wants_loo(n_draws: int, loo=None) -> bool:
    """Whether PSIS-LOO is computed beside WAIC for ``n_draws`` pooled draws per observation: ``loo`` as given, or -- None -- whenever the
    device serves it (n_draws <= ELPD_LOO_MAX_DRAWS); past that bound one warning says that lpd and WAIC alone are returned, so that a
    finished sampling run is not lost to the refusal."""
    if loo is not None:
        return bool(loo)
    if int(n_draws) <= ELPD_LOO_MAX_DRAWS:
        return True
    warnings.warn(f"elpd: {int(n_draws)} pooled draws per observation exceed the {ELPD_LOO_MAX_DRAWS} up to which PSIS-LOO is computed on the device; "
                  "returning lpd and WAIC only (elpd_loo, p_loo and khat are None)", stacklevel=3)
    return False


def elpd_jacobian(links, X_grid: np.ndarray, obs_index):
    """log|g_d'(y)| of every observation (i, d) of ``obs_index`` [n, 2], y = X_grid[i, d]: what carries a log density on the link's scale
    to the scale of the data -- 0 for the identity, -log y for log, -log(2 sqrt(y)) for sqrt.  A datum 0 under a sqrt link has no finite
    constant: ValueError naming the component and the count."""
    X_grid = np.asarray(X_grid, dtype=np.float64)
    obs_index = np.asarray(obs_index, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(obs_index.shape[0])
    for d, k in enumerate(np.zeros(X_grid.shape[1], dtype=np.int32) if links is None else links):
        sel = obs_index[:, 1] == d
        y = X_grid[obs_index[sel, 0], d]
        if int(k) == LINK_LOG:
            out[sel] = -np.log(y)
        elif int(k) == LINK_SQRT:
            zeros = int((y == 0.0).sum())
            if zeros:
                raise ValueError(f"scale='data': component {d} has {zeros} observation(s) equal to 0 under its sqrt link, where log|g'(y)| is not finite; "
                                 "use scale='link'")
            out[sel] = -np.log(2.0 * np.sqrt(y))
    return out


def compare_elpd(models, kind="loo"):
    """Models of the SAME observations compared by their expected log predictive density: ``models`` {name: the dictionary of
    ``posterior_elpd`` / ``sampler_elpd`` / ``elpd``}, ``kind`` "loo" or "waic".  Returns one row per model, best first: dict(name, elpd, se,
    p, elpd_diff (to the best model, <= 0), se_diff = sqrt(n var_i(pointwise difference)) (ddof = 1; 0 for the best), n_khat_bad).  Raises
    ValueError when the models' ``obs_index`` (or numbers of observations) or scales differ: sums over different data do not compare."""
    if kind not in ("loo", "waic"):
        raise ValueError(f"kind: 'loo' or 'waic', got {kind!r}")
    if not models:
        raise ValueError("compare_elpd: no model")
    key, pkey = "elpd_" + kind, "p_" + kind
    names = list(models)
    first = models[names[0]]
    for nm in names:
        r = models[nm]
        if r["pointwise"][key] is None:
            raise ValueError(f"compare_elpd: model {nm!r} holds no {key}")
        a, b = r["obs_index"], first["obs_index"]
        if r["n_obs"] != first["n_obs"] or (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
            raise ValueError(f"compare_elpd: model {nm!r} and model {names[0]!r} differ in obs_index: they were not fitted to the same observations")
        if r.get("scale") != first.get("scale"):
            raise ValueError(f"compare_elpd: model {nm!r} is on scale {r.get('scale')!r}, model {names[0]!r} on {first.get('scale')!r}")
    order = sorted(names, key=lambda nm: -models[nm][key] if np.isfinite(models[nm][key]) else np.inf)
    best = models[order[0]]
    n = best["n_obs"]
    rows = []
    for nm in order:
        r = models[nm]
        diff = r["pointwise"][key] - best["pointwise"][key]
        se_diff = 0.0 if r is best else (float(np.sqrt(n * diff.var(ddof=1))) if n >= 2 else float("nan"))
        rows.append({"name": nm, "elpd": r[key], "se": r["se_" + key], "p": r[pkey], "elpd_diff": 0.0 if r is best else float(diff.sum()),
                     "se_diff": se_diff, "n_khat_bad": r["n_khat_bad"] if kind == "loo" else None})
    return rows


# --------------------------------------------------------------------------------------------
# posterior predictive checks: the host side (replicates, PIT and discrepancies are the device's, csrc/ppc.hip)
# --------------------------------------------------------------------------------------------

PPC_STATS = ("chi2", "mean", "maxabs", "acf1")       # the order of T[0..3] in include/magi_hip.h


def pit_ks(pit, comp, D):
    """Kolmogorov distance of the PIT values from the uniform distribution, per component: sup_t |F_n(t) - t| over the finite ``pit`` of
    the columns with ``comp == d`` -- max_i max(i / n - p_(i), p_(i) - (i - 1) / n) over the sorted values.  NaN for a component without
    one.  Against a calibrated model it stays below about 1.95 / sqrt(n) (alpha = 0.001), PIT values of one fit being nearly independent."""
    pit, comp = np.asarray(pit, dtype=np.float64).reshape(-1), np.asarray(comp, dtype=np.int64).reshape(-1)
    out = np.full(int(D), np.nan)
    for d in range(int(D)):
        p = np.sort(pit[(comp == d) & np.isfinite(pit)])
        n = p.shape[0]
        if n:
            i = np.arange(1, n + 1, dtype=np.float64)
            out[d] = float(max(np.max(i / n - p), np.max(p - (i - 1.0) / n)))
    return out


def ppc_result(comp, D, mean, sd, quantiles, pit, pval, n_T_excluded, n_nonfinite=0, obs_index=None, probs=None, y_rep=None, T_obs=None,
               T_rep=None):
    """The dictionary ``MagiEngine.ppc`` / ``sampler_ppc`` / ``MAGI_v2.posterior_predictive`` return, from the device's arrays
    (include/magi_hip.h: magi_ppc).  ``comp`` [K]: the component of every column.  Holds ``obs_index`` ([K, 2] pairs (grid point,
    component), None for plain columns), ``comp``, ``n_obs`` (= K), ``y_rep`` [chains, draws, K] when given, then ``mean``, ``sd`` [K],
    ``quantiles`` [n_q, K] with their ``probs``, ``pit`` [K], ``pvalues`` {chi2, mean, maxabs, acf1}: each [D], the posterior predictive
    p-value of that discrepancy per component, ``T_obs`` / ``T_rep`` [chains, draws, D, 4] when given, ``n_T_excluded`` [D],
    ``n_nonfinite`` and ``pit_ks`` [D], the Kolmogorov distance of each component's PIT values from uniform (``pit_ks``)."""
    comp = np.asarray(comp, dtype=np.int64).reshape(-1)
    D = int(D)
    pval = np.asarray(pval, dtype=np.float64).reshape(D, len(PPC_STATS))
    out = {"obs_index": None if obs_index is None else np.asarray(obs_index, dtype=np.int64).reshape(-1, 2), "comp": comp, "n_obs": int(comp.shape[0])}
    if y_rep is not None:
        out["y_rep"] = y_rep
    pit = np.asarray(pit, dtype=np.float64).reshape(-1)
    out.update(mean=mean, sd=sd, quantiles=quantiles, probs=probs, pit=pit,
               pvalues={s: pval[:, t].copy() for t, s in enumerate(PPC_STATS)})
    if T_obs is not None:
        out["T_obs"] = T_obs
    if T_rep is not None:
        out["T_rep"] = T_rep
    out.update(n_T_excluded=np.asarray(n_T_excluded, dtype=np.int64).reshape(D), n_nonfinite=int(n_nonfinite), pit_ks=pit_ks(pit, comp, D))
    return out


# --------------------------------------------------------------------------------------------
# rank-normalised diagnostics: the host side (the diagnostics themselves are the device's, csrc/rank.hip)
# --------------------------------------------------------------------------------------------
RANK_KEYS = ("rhat_rank", "ess_bulk", "ess_tail")
RANK_BLOCKS = ("X", "sigma_sqs", "thetas")
RHAT_RANK_MAX = 1.01              # the thresholds of Vehtari et al. (2021): rhat_rank above 1.01,
ESS_PER_CHAIN_MIN = 100.0         # a bulk or tail ESS under 100 per chain


def merge_rank_diagnostics(summary, rank):
    """Adds the three keys of every block of ``rank`` (MagiEngine.sampler_rank_diagnostics) to the same block of ``summary``
    (MagiEngine.sampler_summary), in place; returns ``summary``."""
    for b in RANK_BLOCKS:
        for k in RANK_KEYS:
            summary[b][k] = rank[b][k]
    return summary


def rank_diagnostics_flags(summary, n_chains: int):
    """Per block of a summary that carries the rank diagnostics: the number of columns with rhat_rank > 1.01, ess_bulk < 100 n_chains and
    ess_tail < 100 n_chains (a NaN diagnostic -- a constant column, fewer than four draws -- is not counted)."""
    need = ESS_PER_CHAIN_MIN * n_chains
    with np.errstate(invalid="ignore"):
        return {b: {"rhat_rank": int(np.sum(np.asarray(summary[b]["rhat_rank"]) > RHAT_RANK_MAX)),
                    "ess_bulk": int(np.sum(np.asarray(summary[b]["ess_bulk"]) < need)),
                    "ess_tail": int(np.sum(np.asarray(summary[b]["ess_tail"]) < need))} for b in RANK_BLOCKS}


def warn_rank_diagnostics(summary, n_chains: int):
    """One warning that names, per block, how many columns miss a threshold; none when every column passes.  Called only where the
    rank diagnostics were asked for.  Returns the counts of ``rank_diagnostics_flags``."""
    flags = rank_diagnostics_flags(summary, n_chains)
    parts = [f"{b}: {f['rhat_rank']} with rhat_rank > {RHAT_RANK_MAX}, {f['ess_bulk']} with ess_bulk and {f['ess_tail']} with ess_tail < "
             f"{ESS_PER_CHAIN_MIN * n_chains:g}" for b, f in flags.items() if any(f.values())]
    if parts:
        import warnings
        warnings.warn("rank diagnostics: columns beyond the thresholds of Vehtari et al. (2021) -- " + "; ".join(parts)
                      + " (run longer chains, or more of them)")
    return flags


def fisher_report(fim_mean, names, post_sd=None, collinearity_warn=15.0):
    """What a Fisher information matrix F [Q, Q] (MagiEngine.ode_sensitivities' ``fim_mean``) says about the parameters ``names``: pure
    numpy.  Returns dict(
      names;
      eigenvalues [Q] ascending and eigenvectors [Q, Q] (column i belongs to eigenvalue i) of the symmetrised F;
      condition_number  lambda_max / lambda_min, inf when lambda_min <= 0;
      positive_definite  lambda_min > Q eps lambda_max;
      crlb_sd [Q]  sqrt(diag(F^-1)), the Cramer-Rao bound on an unbiased estimate's sd; NaN when F is not numerically positive definite;
      collinearity_index  gamma = 1 / sqrt(lambda_min of F scaled to unit diagonal) (Brun, Reichert & Kuensch 2001, who treat 10-15 as the
                   critical range): 1 for orthogonal sensitivities, inf when the scaled lambda_min <= 0 or a diagonal entry is not > 0;
      weakest_direction  [(name, loading), ...] of the eigenvector of lambda_min, largest |loading| first, signed so that the first is > 0:
                   the combination of parameters the observations determine least;
      sd_ratio [Q]  post_sd / crlb_sd (None without ``post_sd``): well below 1 where a posterior is narrower than the data alone allow).
    One warning, naming the weakest direction, when gamma exceeds ``collinearity_warn``.  A non-finite F gives NaN throughout and no
    warning."""
    F = np.array(fim_mean, dtype=np.float64)
    names = [str(n) for n in names]
    Q = len(names)
    if F.shape != (Q, Q):
        raise ValueError(f"expected a [{Q}, {Q}] matrix for {Q} names, got {F.shape}")
    nan_q = np.full(Q, np.nan)
    post_sd = None if post_sd is None else np.asarray(post_sd, dtype=np.float64).reshape(-1)
    if post_sd is not None and post_sd.shape[0] != Q:
        raise ValueError(f"expected {Q} posterior sds, got {post_sd.shape[0]}")
    if not np.isfinite(F).all():
        return {"names": names, "eigenvalues": nan_q, "eigenvectors": np.full((Q, Q), np.nan), "condition_number": np.nan, "positive_definite": False,
                "crlb_sd": nan_q.copy(), "collinearity_index": np.nan, "weakest_direction": [], "sd_ratio": None if post_sd is None else nan_q.copy()}
    F = 0.5 * (F + F.T)
    lam, vec = np.linalg.eigh(F)
    eps = np.finfo(np.float64).eps
    pd = bool(lam[0] > Q * eps * lam[-1]) and bool(lam[-1] > 0.0)
    cond = float(lam[-1] / lam[0]) if lam[0] > 0.0 else np.inf
    crlb = np.sqrt(np.diag(np.linalg.inv(F))) if pd else nan_q.copy()
    dg = np.diag(F)
    if (dg > 0.0).all():
        sc = 1.0 / np.sqrt(dg)
        lmin = np.linalg.eigvalsh(F * sc[:, None] * sc[None, :])[0]
        gamma = float(1.0 / np.sqrt(lmin)) if lmin > 0.0 else np.inf
    else:
        gamma = np.inf
    v = vec[:, 0]
    order = np.argsort(-np.abs(v), kind="stable")
    v = v * (1.0 if v[order[0]] >= 0.0 else -1.0)
    weakest = [(names[i], float(v[i])) for i in order]
    if gamma > collinearity_warn:
        shown = ", ".join(f"{l:+.3g} {n}" for n, l in weakest if abs(l) >= 0.05)
        warnings.warn(f"Fisher information: collinearity index {gamma:.3g} exceeds {collinearity_warn:g}: the observations hardly determine the "
                      f"direction {shown}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = None if post_sd is None else post_sd / crlb
    return {"names": names, "eigenvalues": lam, "eigenvectors": vec, "condition_number": cond, "positive_definite": pd, "crlb_sd": crlb,
            "collinearity_index": gamma, "weakest_direction": weakest, "sd_ratio": ratio}


# --------------------------------------------------------------------------------------------
# drifts
# --------------------------------------------------------------------------------------------


def _np_seir3(t, X, th):
    S = 1.0 - X.sum(axis=1, keepdims=True)
    E, I_ = X[:, 0:1], X[:, 1:2]
    return np.concatenate([th[0] * S * I_ - th[2] * E, th[2] * E - th[1] * I_, th[1] * I_], axis=1)


def _np_seir4(t, X, th):
    S, E, I_ = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    return np.concatenate([-th[0] * S * I_, th[0] * S * I_ - th[2] * E, th[2] * E - th[1] * I_, th[1] * I_], axis=1)


def _np_sirw(t, X, th):
    S, I_, R, W = (X[:, k:k + 1] for k in range(4))
    inf, wane, boost = th[0] * S * I_, th[4] * W, th[3] * I_ * W
    return np.concatenate([wane - inf, inf - th[1] * I_, th[1] * I_ - th[2] * R + boost, th[2] * R - boost - wane], axis=1)


NUMPY_DRIFTS: Dict[str, Callable] = {"seir3": _np_seir3, "seir4": _np_seir4, "sirw": _np_sirw}


def resolve_drift(f_vec, D: int, P: int) -> str:
    """Name of the drift ``f_vec`` resolves to (magi_v2.py:33, 73): a compiled-in one ("seir3", "seir4", "sirw")
    when the callable agrees with it numerically, else the name of the traced user drift (drift.resolve)."""
    from . import drift
    return drift.resolve(f_vec, D, P).name


# --------------------------------------------------------------------------------------------
# warm-up windows of the diagonal-metric adaptation (MAGI_v2.predict(adapt_metric=True))
# --------------------------------------------------------------------------------------------


def warmup_schedule(num_burnin: int, n_adapt: int, init_buffer: int = 75, base_window: int = 25, term_buffer: int = 50):
    """Stan's windowed warm-up over the adaptation transitions [0, n_adapt) of a burn-in of ``num_burnin``: a fast initial buffer (step
    size only), slow windows whose states become the metric at their end -- the first ``base_window`` long, each next one twice as long,
    the last one stretched to the terminal buffer when the one after it would not fit -- and a fast terminal buffer.  When the three
    do not fit into n_adapt (with the defaults: n_adapt < 150) they become 15 % / 75 % / 10 % of it; a slow part too short for a
    variance (fewer than 2 transitions) leaves one fast window.  Returns [(start, stop, adapt_metric_at_stop)], tiling [0, n_adapt);
    empty for n_adapt = 0.  A pure function."""
    num_burnin, n_adapt = int(num_burnin), int(n_adapt)
    init_buffer, base_window, term_buffer = int(init_buffer), int(base_window), int(term_buffer)
    if not 0 <= n_adapt <= num_burnin:
        raise ValueError(f"need 0 <= n_adapt <= num_burnin, got {n_adapt}, {num_burnin}")
    if init_buffer < 0 or base_window < 1 or term_buffer < 0:
        raise ValueError("need init_buffer >= 0, base_window >= 1, term_buffer >= 0")
    if n_adapt == 0:
        return []
    if init_buffer + base_window + term_buffer > n_adapt:
        init_buffer, term_buffer = int(0.15 * n_adapt), int(0.1 * n_adapt)
        base_window = n_adapt - init_buffer - term_buffer
    if base_window < 2:
        return [(0, n_adapt, False)]
    out = [(0, init_buffer, False)] if init_buffer else []
    start, size, end_slow = init_buffer, base_window, n_adapt - term_buffer
    while start < end_slow:
        stop = start + size
        if stop + 2 * size > end_slow:          # the next (doubled) window would not fit: this one runs to the terminal buffer
            stop = end_slow
        out.append((start, stop, True))
        start, size = stop, 2 * size
    if term_buffer:
        out.append((end_slow, n_adapt, False))
    return out


# --------------------------------------------------------------------------------------------
# synthetic SEIR grids (BASELINE.json configs 2, 3, 5)
# --------------------------------------------------------------------------------------------


def synthetic_seir(N: int, seed: int = 0, dt: float = 0.025, alpha: float = 0.05):
    """SEIR-4 truth by RK4 (beta=6, gamma=.6, sigma=1.8, x0=(.99,.01,0,0) -- the generator of the
    reference's data/*.csv), uniform grid of spacing dt, observations at even grid indices with
    noise N(0, (alpha * range_d)^2) drawn from PCG64(seed), clipped at 0 as the vignette does.
    Returns (I[N], X_obs[N,4] with NaN at unobserved rows, truth[N,4], theta_true)."""
    th = np.array([6.0, 0.6, 1.8])

    def f(x):
        S, E, I_, _ = x
        return np.array([-th[0] * S * I_, th[0] * S * I_ - th[2] * E, th[2] * E - th[1] * I_, th[1] * I_])

    sub = 25
    h = dt / sub
    x = np.array([0.99, 0.01, 0.0, 0.0])
    truth = np.zeros((N, 4))
    truth[0] = x
    for i in range(1, N):
        for _ in range(sub):
            k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
            x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        truth[i] = x
    rng = np.random.Generator(np.random.PCG64(seed))
    span = truth.max(axis=0) - truth.min(axis=0)
    X_obs = np.full((N, 4), np.nan)
    rows = np.arange(0, N, 2)
    X_obs[rows] = truth[rows] + rng.normal(size=(len(rows), 4)) * (alpha * span)
    X_obs[X_obs < 0.0] = 0.0
    return np.arange(N) * dt, X_obs, truth, th
