"""CPU truth for the device's pointwise log-likelihood, WAIC and PSIS-LOO (magi_elpd, magi_sampler_elpd; tests/test_elpd_cpu.py,
tests/test_elpd_gpu.py): the definitions of include/magi_hip.h transcribed in numpy, in float64 or longdouble, with the deliberately wrong
definitions the CPU test holds the device bars against.  A helper module: product code never imports it.

Per column l[s], s = c R + r over S = C R pooled draws:
  lpd = logsumexp_s l - log S;  p_waic = var_s l (ddof 1, NaN when S < 2);  elpd_waic = lpd - p_waic.
  PSIS (Vehtari, Gelman, Gabry 2017, r_eff = 1): r_s = -l_s - max_s(-l_s), formed in float64 as the device forms it (a -0.0 counts as
  +0.0); M = min(S // 5, ceil(3 sqrt(S))); the draws ordered ascending by (r, s) -- a stable argsort -- the tail the last M, the cutoff the
  r of the draw just below.  M < 5 or a tied tail: no smoothing, khat = +inf.  Else x_j = exp(r_tail,j) - exp(cutoff) and the
  Zhang-Stephens fit: m = 30 + floor(sqrt(M)); theta_j = 1/x_M + (1 - sqrt(m / (j - 1/2))) / (3 x_[floor(M/4 + 1/2)]); k_j = mean
  log1p(-theta_j x); l_j = M (log(-theta_j / k_j) - k_j - 1); w_j = 1 / sum_i exp(l_i - l_j); theta = sum theta_j w_j; k = mean log1p(-theta x);
  sigma = -k / theta; khat = (k M + 5) / (M + 10).  khat finite: the tail draw of rank j gets log(exp(cutoff) + sigma / khat expm1(-khat
  log1p(-(j - 1/2) / M))) (khat = 0: exp(cutoff) - sigma log1p(..) inside the log).  All log weights capped at 0.
  elpd_loo = logsumexp(l + lw) - logsumexp(lw);  p_loo = lpd - elpd_loo.
A column with a non-finite l: every output NaN, counted in n_nonfinite."""
import functools
import math

import numpy as np

OUTPUTS = ("lpd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "khat")
U = 2.0 ** -53
LOO_MAX_S = 466033          # the device sorts a tail of at most 2048 draws in LDS: ceil(3 sqrt(S)) <= 2048

# ---- the bars of the device comparison (derived in tests/test_elpd_cpu.py from the float64 / longdouble distance of this reference alone;
#      DESIGN.md 4.5) ----------------------------------------------------------------------------------------------------------------------
# One rule per output: |device - longdouble| <= BAR[out] * scale, scale = max(1, max_s |l_s|) of the column -- every output is a difference
# of sums of numbers of that size.  khat has its own: the Zhang-Stephens weights exponentiate M times a mean of logs.
# Each constant is MARGIN x the largest float64 / longdouble distance over the fixture table (in units of the scale), and at least
# FLOOR_ULP ulp of the scale: the device's log / exp and its summation order differ from numpy's by rounding errors of the same size.
MARGIN = 64.0
FLOOR_ULP = 16.0
BAR = {"lpd": 6e-14, "p_waic": 2e-14, "elpd_waic": 6e-14, "elpd_loo": 1.5e-13, "p_loo": 1.5e-13, "khat": 1.5e-13}
LL_ULP = 32.0            # pointwise log-likelihood from draws, see loglik_bar: softplus (exp, log, two adds), the link, log(2 pi sigma^2 / w), the quadratic term -- about 12 roundings

FAULTS = ("ddof0", "lpd_no_logS", "tail_ceil_fifth", "cutoff_in_tail", "ties_desc_index", "khat_no_prior", "quantile_j", "no_cap", "no_normalise")
LL_FAULTS = ("sigma_no_LB", "fixed_ignored", "weight_not_in_quadratic", "weight_not_in_log", "link_ignored", "nan_counted", "X_as_ND")


def tail_length(S, fault=None):
    if fault == "tail_ceil_fifth":
        return -(-S // 5)
    t = math.isqrt(9 * S)
    return min(S // 5, t if t * t == 9 * S else t + 1)


def log_ratios(l64):
    """float64, as the device forms them."""
    r = -l64
    r = r - r.max()
    return np.where(r == 0.0, 0.0, r)


def tail_order(r, fault=None):
    """Indices of the draws ascending by (r, s); ``ties_desc_index``: by (r, -s)."""
    if fault == "ties_desc_index":
        n = r.shape[0]
        return (n - 1 - np.argsort(r[::-1], kind="stable"))
    return np.argsort(r, kind="stable")


def gpd_fit(x, dtype, fault=None):
    """x ascending, >= 0 -> (khat, sigma)."""
    M = x.shape[0]
    m = 30 + math.isqrt(M)
    j = np.arange(1, m + 1).astype(dtype)
    xq = x[(M + 2) // 4 - 1]
    with np.errstate(all="ignore"):
        th = dtype(1) / x[-1] + (dtype(1) - np.sqrt(dtype(m) / (j - dtype(0.5)))) / (dtype(3) * xq)
        k = np.log1p(-th[:, None] * x[None, :]).sum(axis=1) / dtype(M)
        l = dtype(M) * (np.log(-th / k) - k - dtype(1))
        w = dtype(1) / np.exp(l[None, :] - l[:, None]).sum(axis=1)
        t = (th * w).sum()
        k = np.log1p(-t * x).sum() / dtype(M)
        s = -k / t
        kh = k if fault == "khat_no_prior" else (k * dtype(M) + dtype(5)) / dtype(M + 10)
    return kh, s


def column(l, dtype=np.longdouble, fault=None):
    """One column l[S] (float64 bits) -> dict of OUTPUTS plus nonfinite, M, scale and the conditioning of the order decision: ``gap`` = the
    smallest relative distance of two distinct neighbouring r among cutoff + tail (None without smoothing)."""
    l64 = np.asarray(l, dtype=np.float64).reshape(-1)
    S = l64.shape[0]
    nan = dtype(np.nan)
    out = {k: nan for k in OUTPUTS}
    out.update(nonfinite=False, M=tail_length(S, fault), gap=None, scale=None, smoothed=False)
    if not np.all(np.isfinite(l64)):
        out["nonfinite"] = True
        return out
    ll = l64.astype(dtype)
    out["scale"] = max(1.0, float(np.abs(l64).max()))
    mx = ll.max()
    lpd = mx + np.log(np.exp(ll - mx).sum())
    if fault != "lpd_no_logS":
        lpd = lpd - np.log(dtype(S))
    mu = ll.sum() / dtype(S)
    if S >= 2:
        out["p_waic"] = ((ll - mu) ** 2).sum() / dtype(S if fault == "ddof0" else S - 1)
    out["lpd"] = lpd
    out["elpd_waic"] = lpd - out["p_waic"]
    r64 = log_ratios(l64)
    nl = -ll
    r = nl - nl.max()                                     # (the same ratios in dtype; the ORDER is that of the float64 ones)
    r = np.where(r == 0, dtype(0), r)
    M = out["M"]
    lw = r.copy()
    kh = dtype(np.inf)
    if M >= 5:
        o = tail_order(r64, fault)
        tail = o[S - M:]
        cut = r[o[S - M]] if fault == "cutoff_in_tail" else r[o[S - M - 1]]
        rt = r[tail]
        if r64[tail].max() > r64[tail].min():
            seq = np.concatenate([[r64[o[S - M - 1]]], r64[tail]])
            d = np.diff(seq)
            rel = d[d > 0] / np.maximum(np.abs(seq[1:]), np.abs(seq[:-1]))[d > 0]
            out["gap"] = float(rel.min()) if rel.size else None
            ec = np.exp(cut)
            x = np.exp(rt) - ec
            kh, s = gpd_fit(x, dtype, fault)
            if np.isfinite(kh):
                out["smoothed"] = True
                jj = np.arange(1, M + 1).astype(dtype)
                p = (jj if fault == "quantile_j" else jj - dtype(0.5)) / dtype(M)
                with np.errstate(all="ignore"):
                    lp = np.log1p(-p)
                    q = s / kh * np.expm1(-kh * lp) if kh != 0 else -s * lp
                    lw[tail] = np.log(ec + q)
    if fault != "no_cap":
        lw = np.minimum(lw, dtype(0))
    a = ll + lw
    A, B = a.max(), lw.max()
    with np.errstate(all="ignore"):
        el = A + np.log(np.exp(a - A).sum())
        if fault != "no_normalise":
            el = el - (B + np.log(np.exp(lw - B).sum()))
    out["khat"] = kh
    out["elpd_loo"] = el
    out["p_loo"] = lpd - el
    return out


def elpd(loglik, dtype=np.longdouble, fault=None):
    """loglik [C][R][K] -> dict of arrays [K] of OUTPUTS, n_nonfinite, ``columns`` (the per-column dicts)."""
    loglik = np.asarray(loglik, dtype=np.float64)
    K = loglik.shape[2]
    flat = loglik.reshape(-1, K)
    cols = [column(flat[:, k], dtype, fault) for k in range(K)]
    out = {s: np.array([c[s] for c in cols], dtype=dtype) for s in OUTPUTS}
    out["n_nonfinite"] = sum(c["nonfinite"] for c in cols)
    out["columns"] = cols
    return out


def check_against(got, ref, outputs=OUTPUTS):
    """The device's pointwise arrays ``got`` (name -> [K]) against ``ref`` (``elpd`` above, longdouble) at BAR; NaN and +-inf must agree
    exactly.  Returns the worst error as a fraction of its bar, per output."""
    worst = {}
    for k, c in enumerate(ref["columns"]):
        for s in outputs:
            g, r = np.asarray(got[s])[k], ref[s][k]
            if not np.isfinite(r):
                assert (np.isnan(g) and np.isnan(r)) or g == r, (s, k, g, r)
                continue
            bar = max(BAR[s], FLOOR_ULP * 2 * U) * c["scale"]
            err = float(abs(np.longdouble(g) - r))
            worst[s] = max(worst.get(s, 0.0), err / bar)
            assert err <= bar, (s, k, float(g), float(r), err, bar)
    if "n_nonfinite" in got:
        assert got["n_nonfinite"] == ref["n_nonfinite"]
    return worst


# ---- crafted log-likelihood arrays --------------------------------------------------------------------------------------------------------

SHAPES = ((1, 24), (1, 25), (2, 50), (2, 1024), (1, 2049), (5, 1000), (1, LOO_MAX_S))          # C x R
COLUMNS = ("light", "z2", "heavy", "constant", "tied_tail", "straddle", "nan", "neg_inf", "zeros", "shifted")
K_CRAFTED = len(COLUMNS)


def half_normal_grid(S, rng):
    """S half-normal quantiles (i + 1/2) / S in a random order: no two alike, and neighbours in the upper tail a known distance apart --
    1 / (2 S phi(a)) -- so that no two ratios of a tail come closer than the CPU test's 1e-6 relative, whatever S is."""
    from scipy.special import ndtri
    return ndtri(0.5 + (rng.permutation(S) + 0.5) / (2.0 * S))


@functools.lru_cache(maxsize=None)
def crafted(C, R):
    """[C][R][K_CRAFTED] log-likelihoods, read-only, each column a function of a half_normal_grid a: a light tail (khat < 0.5), ratios
    proportional to exp(a^2 / 2) (khat about 1), a heavy tail (khat > 3), a constant column, a column whose whole tail is tied, ties
    straddling the cutoff (the index order decides who is in the tail), a column with one NaN, one with -inf, a column with -0.0 / +0.0
    pairs, and a column shifted to |l| of about 40."""
    S = C * R
    rng = np.random.default_rng(1000 * C + R)
    M = tail_length(S)
    y = np.empty((S, K_CRAFTED))
    a = np.stack([half_normal_grid(S, rng) for _ in range(K_CRAFTED)], axis=1)
    y[:, 0] = -0.5 * (0.3 * a[:, 0]) ** 2 - 1.0
    y[:, 1] = -0.5 * a[:, 1] ** 2 - 0.9
    y[:, 2] = -0.5 * (2.5 * a[:, 2]) ** 2
    y[:, 3] = -1.25
    # the whole tail tied: the M + 2 smallest l equal
    t = -a[:, 4] - 0.1
    o = np.argsort(t)
    t[o[:M + 2]] = t[o[M + 1]]
    y[:, 4] = t
    # ties straddling the cutoff: the draws of rank M - 1, M, M + 1 from below share one value -- two inside the tail, one below it
    t = -1.5 * a[:, 5] - 0.2
    o = np.argsort(t)
    if M >= 2:
        t[o[M - 2]] = t[o[M - 1]] = t[o[M]]
    y[:, 5] = t
    y[:, 6] = -0.5 * a[:, 6] ** 2
    y[S // 3, 6] = np.nan
    y[:, 7] = -0.5 * a[:, 7] ** 2
    y[(2 * S) // 3, 7] = -np.inf
    t = -a[:, 8]
    t[0::7] = 0.0
    t[3::7] = -0.0
    y[:, 8] = t
    y[:, 9] = 40.0 - 0.5 * a[:, 9] ** 2
    y = y.reshape(C, R, K_CRAFTED)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def crafted_reference(C, R, long=True):
    return elpd(crafted(C, R), np.longdouble if long else np.float64)


# ---- the log-likelihood of sampler draws ---------------------------------------------------------------------------------------------------

def link_g(link, v, dtype):
    v = np.asarray(v, dtype=dtype)
    with np.errstate(all="ignore"):
        return np.log(v) if int(link) == 1 else np.sqrt(v) if int(link) == 2 else v


def loglik(X, sig_pre, y_grid, LB, links=None, weights=None, fixed=None, dtype=np.longdouble, fault=None):
    """The log-likelihood [C][R][n_obs] of the draws X [C][R][N][D] (host layout), sig_pre [C][R][D] under the data y_grid [N][D] (the raw
    observations, NaN where there is none), LB [D], link codes [D] (None: identity), weights [N][D] (None: 1), fixed {d: constant}.
    Returns (loglik, obs_index [n_obs][2] = (i, d) ascending in d N + i, cond [C][R][n_obs]: the conditioning term of loglik_bar)."""
    X = np.asarray(X, dtype=np.float64)
    C, R, N, D = X.shape
    y_grid = np.asarray(y_grid, dtype=np.float64)
    links = np.zeros(D, dtype=int) if links is None else np.asarray(links)
    W = np.ones((N, D)) if weights is None else np.asarray(weights, dtype=np.float64)
    sp = np.asarray(sig_pre, dtype=np.float64).astype(dtype)
    seen = ~np.isnan(y_grid)
    if fault == "nan_counted":
        seen = np.ones_like(seen)
    cols, conds, idx = [], [], []
    pi = np.arccos(dtype(-1))
    Xs = X.reshape(C, R, D, N)                            # (the fault X_as_ND: the block indexed in the other of its two layouts)
    for d in range(D):
        s2 = np.log(dtype(1) + np.exp(sp[:, :, d]))
        if fault != "sigma_no_LB":
            s2 = s2 + dtype(LB[d])
        is_fixed = bool(fixed) and d in fixed and fault != "fixed_ignored"
        if is_fixed:
            s2 = np.full_like(s2, dtype(fixed[d]))
        lk = 0 if fault == "link_ignored" else links[d]
        for i in np.nonzero(seen[:, d])[0]:
            x = Xs[:, :, d, i] if fault == "X_as_ND" else X[:, :, i, d]
            w = dtype(W[i, d])
            wq = dtype(1) if fault == "weight_not_in_quadratic" else w
            wl = dtype(1) if fault == "weight_not_in_log" else w
            with np.errstate(all="ignore"):
                gy, gx = link_g(lk, y_grid[i, d], dtype), link_g(lk, x, dtype)
                df = gx - gy
                cols.append(-dtype(0.5) * (np.log(dtype(2) * pi * s2 / wl) + wq * df * df / s2))
                conds.append(wq * np.abs(df) * (np.abs(gx) + np.abs(gy)) / s2 + (0 if is_fixed else dtype(0.5) * (1 + wq * df * df / s2) / s2))
            idx.append((i, d))
    ll = np.stack(cols, axis=-1) if cols else np.empty((C, R, 0), dtype=dtype)
    cond = np.stack(conds, axis=-1) if conds else np.empty((C, R, 0), dtype=dtype)
    return ll, np.asarray(idx, dtype=np.int64).reshape(-1, 2), cond


def loglik_bar(ref, cond):
    """LL_ULP roundings of max(1, |l|) + w |g(x) - g(y)| (|g(x)| + |g(y)|) / sigma^2 + (1 + w (g(x) - g(y))^2 / sigma^2) / (2 sigma^2).  The
    second term is what one rounding of g(x) or g(y) becomes in the quadratic term (the residual cancels; the divide by sigma^2
    amplifies); the third what one rounding of 1 + e^pre inside softplus = log(1 + e^pre) -- an absolute error u of sigma^2, the
    definition's own formula -- becomes in l (absent under a fixed variance)."""
    return LL_ULP * 2 * U * (np.maximum(1.0, np.abs(ref).astype(np.float64)) + np.asarray(cond, dtype=np.float64))


def tail_margin(ll, bar):
    """How far the order decisions of PSIS on the log-likelihood ll [S][K] (float64) are from what an error of ``bar`` [S][K] per entry
    could change: over the columns that smooth, the smallest distance of two DISTINCT neighbouring ratios among the cutoff and the tail,
    divided by twice the column's largest bar (a ratio carries the error of its own l and of the maximum).  Draws a chain repeats are
    equal on both sides and do not count.  inf when no column smooths."""
    ll, bar = np.asarray(ll, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    S, K = ll.shape
    M = tail_length(S)
    worst = np.inf
    if M < 5:
        return worst
    for k in range(K):
        if not np.all(np.isfinite(ll[:, k])):
            continue
        r = log_ratios(ll[:, k])
        seq = r[tail_order(r)[S - M - 1:]]
        d = np.diff(seq)
        if seq[-1] > seq[1] and np.any(d > 0):
            worst = min(worst, float(d[d > 0].min() / (2.0 * bar[:, k].max())))
    return worst


def check_loglik(got, ref, cond):
    """The device's log-likelihood ``got`` against ``ref`` (longdouble) at loglik_bar; non-finite entries must agree."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    err = np.abs(got[fin].astype(np.longdouble) - ref[fin]).astype(np.float64)
    worst = float((err / loglik_bar(ref[fin], cond[fin])).max()) if err.size else 0.0
    assert worst <= 1.0, worst
    return worst
