"""CPU truth for the device summaries (magi_summarize, magi_sampler_summarize; tests/test_summary_cpu.py, tests/test_summary_gpu.py): the
definitions of include/magi_hip.h transcribed in numpy, in float64 or longdouble, with the deliberately wrong definitions the CPU test
holds the device tolerances against.  A helper module: product code never imports it.

Per column y[c][r] (C chains, R draws), S = C R pooled draws:
  order statistics v = sort(pooled); quantile at p: h = (S - 1) p (float64, as the device forms it), lo = floor(h), g = h - lo,
  q = v[lo] + g (v[min(lo + 1, S - 1)] - v[lo]).  mean; sd with ddof = 1 (NaN when S < 2).
  Split R-hat: n = R // 2, M = 2 C; split chain 2c = rows [0, n) of chain c, 2c + 1 = rows [R - n, R).  W = mean_m s2_m (ddof = 1),
  B/n = var_m(ybar_m, ddof = 1), var+ = (n - 1)/n W + B/n, rhat = sqrt(var+ / W).
  ESS: acov_m(t) = 1/n sum_{i < n - t} (y_i - ybar_m)(y_{i+t} - ybar_m); rho_0 = 1, rho_t = 1 - (W - mean_m acov_m(t)) / var+ for
  1 <= t <= L = min(n - 1, max_lag) (max_lag <= 0: n - 1); P_k = rho_{2k} + rho_{2k+1} for 2k + 1 <= L; K* = first k with P_k < 0 (else the
  number of pairs); for k = 1 .. K* - 1 in turn P_k = min(P_k, P_{k-1}); tau = max(-1 + 2 sum_{k < K*} P_k, 1 / log10(M n));
  ess = M n / tau; mcse_mean = sd / sqrt(ess).
  rhat, ess, mcse_mean are NaN when R < 4.  Constant column (v[0] == v[-1]): sd = 0, rhat = ess = mcse_mean = NaN.  A non-finite draw:
  every statistic NaN, the column counts in n_nonfinite."""
import functools

import numpy as np

SHAPES = ((1, 4), (1, 5), (1, 64), (2, 65), (3, 257), (9, 130), (64, 40), (4, 1000))
PHIS = (0.0, 0.5, 0.9, 0.99, -0.5, -0.9, 0.3)
PROBS = (0.025, 0.5, 0.975)
K_FIXTURE = len(PHIS) + 4
COL_OFFSET, COL_TIGHT, COL_CONST, COL_NAN = len(PHIS), len(PHIS) + 1, len(PHIS) + 2, len(PHIS) + 3
VARIANTS = ("lag_divisor_n_minus_t", "no_split")
U = 2.0 ** -53


def rtol_spread(kappa):
    """sd, rhat, ess, mcse_mean: the first-order error is the mean's rounding relative to the spread, u kappa (kappa = max|y| / sd)."""
    return 1e-13 * kappa + 1e-11


@functools.lru_cache(maxsize=None)
def fixture(C, R):
    """[C][R][K_FIXTURE] draws: AR(1) columns 3 + x 10^(j-3) for the PHIS (stationary start), then chains offset from one another, a
    1e3 + 1e-3 noise column, a constant column and a column with one NaN.  Read-only."""
    rng = np.random.default_rng(100 * C + R)
    y = np.empty((C, R, K_FIXTURE))
    for j, phi in enumerate(PHIS):
        e = rng.standard_normal((C, R))
        x = np.empty((C, R))
        x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
        for r in range(1, R):
            x[:, r] = phi * x[:, r - 1] + e[:, r]
        y[:, :, j] = 3.0 + x * 10.0 ** (j - 3)
    y[:, :, COL_OFFSET] = rng.standard_normal((C, R)) + 3.0 * np.arange(C)[:, None] + np.where(np.arange(R) < R // 2, 0.0, 2.0)[None, :] * (C == 1)
    y[:, :, COL_TIGHT] = 1e3 + 1e-3 * rng.standard_normal((C, R))
    y[:, :, COL_CONST] = 0.75
    y[:, :, COL_NAN] = rng.standard_normal((C, R))
    y[C // 2, R // 3, COL_NAN] = np.nan
    y.setflags(write=False)
    return y


def quantiles(v, probs, dtype):
    """v: sorted pooled draws of one column."""
    S = v.shape[0]
    out = np.empty(len(probs), dtype=dtype)
    for q, p in enumerate(probs):
        h = np.float64(S - 1) * np.float64(p)
        lo = int(np.floor(h))
        g = dtype(h - lo)
        hi = min(lo + 1, S - 1)
        out[q] = v[lo] if g == 0 else v[lo] + g * (v[hi] - v[lo])          # (g = 0: the order statistic itself, also where v[hi] - v[lo] overflows)
    return out


def column(y, probs=PROBS, max_lag=0, dtype=np.longdouble, variant=None):
    """One column y[C][R] -> dict(mean, sd, quantiles, rhat, ess, mcse_mean, order (the sorted pooled draws, float64), nonfinite, and the
    conditioning of the decision the result rests on: kstar, min_abs_P (over k <= K*), tau_gap (|tau - floor|), tau_at_floor (tau is the
    floor 1 / log10(M n)), kappa)."""
    assert variant is None or variant in VARIANTS
    y64 = np.asarray(y, dtype=np.float64)
    C, R = y64.shape
    S = C * R
    nan = dtype(np.nan)
    out = dict(mean=nan, sd=nan, quantiles=np.full(len(probs), np.nan, dtype=dtype), rhat=nan, ess=nan, mcse_mean=nan, order=None,
               nonfinite=False, kstar=None, min_abs_P=None, tau_gap=None, tau_at_floor=None, kappa=None)
    if not np.all(np.isfinite(y64)):
        out["nonfinite"] = True
        return out
    yy = y64.astype(dtype)
    v = np.sort(yy.reshape(-1))
    out["order"] = np.sort(y64.reshape(-1))
    out["quantiles"] = quantiles(v, probs, dtype)
    mu = yy.sum() / dtype(S)
    out["mean"] = mu
    constant = v[0] == v[-1]
    if S >= 2:
        out["sd"] = dtype(0.0) if constant else np.sqrt(((yy - mu) ** 2).sum() / dtype(S - 1))
    if R < 4 or constant:
        return out
    out["kappa"] = float(np.abs(yy).max() / out["sd"])
    if variant == "no_split":
        n, M = R, C
        z = yy
    else:
        n, M = R // 2, 2 * C
        z = np.empty((M, n), dtype=dtype)
        z[0::2] = yy[:, :n]
        z[1::2] = yy[:, R - n:]
    ybar = z.sum(axis=1) / dtype(n)
    zc = z - ybar[:, None]
    s2 = (zc ** 2).sum(axis=1) / dtype(n - 1)
    W = s2.sum() / dtype(M)
    Bn = ((ybar - ybar.sum() / dtype(M)) ** 2).sum() / dtype(M - 1) if M > 1 else dtype(0.0)
    varp = dtype(n - 1) / dtype(n) * W + Bn
    out["rhat"] = np.sqrt(varp / W)
    L = n - 1 if max_lag <= 0 else min(n - 1, max_lag)

    def rho(t):
        if t == 0:
            return dtype(1.0)
        div = dtype(n - t) if variant == "lag_divisor_n_minus_t" else dtype(n)
        acov = (zc[:, :n - t] * zc[:, t:]).sum(axis=1) / div
        return dtype(1.0) - (W - acov.sum() / dtype(M)) / varp

    P = [rho(2 * k) + rho(2 * k + 1) for k in range((L + 1) // 2)]
    kstar = next((k for k, p in enumerate(P) if p < 0), len(P))
    total, prev = dtype(0.0), None
    for k in range(kstar):
        prev = P[k] if k == 0 else min(P[k], prev)
        total += prev
    floor_ = dtype(1.0) / np.log10(dtype(M * n))
    tau_raw = dtype(-1.0) + dtype(2.0) * total
    tau = max(tau_raw, floor_)
    out["ess"] = dtype(M * n) / tau
    out["mcse_mean"] = out["sd"] / np.sqrt(out["ess"])
    out["kstar"] = kstar
    out["min_abs_P"] = float(min(abs(p) for p in P[:kstar + 1])) if P else np.inf
    out["tau_gap"] = float(abs(tau_raw - floor_))
    out["tau_at_floor"] = bool(tau_raw <= floor_)
    return out


def summarize(draws, probs=PROBS, max_lag=0, dtype=np.longdouble, variant=None):
    """draws [C][R] + shape -> dict of arrays of that shape (quantiles: [len(probs)] + shape), n_nonfinite, and ``columns``: the per-column
    dicts of ``column`` in C order."""
    draws = np.asarray(draws, dtype=np.float64)
    C, R, shape = draws.shape[0], draws.shape[1], draws.shape[2:]
    flat = draws.reshape(C, R, -1)
    cols = [column(flat[:, :, k], probs, max_lag, dtype, variant) for k in range(flat.shape[2])]
    out = {s: np.array([c[s] for c in cols], dtype=dtype).reshape(shape) for s in ("mean", "sd", "rhat", "ess", "mcse_mean")}
    out["quantiles"] = np.stack([c["quantiles"] for c in cols], axis=-1).astype(dtype).reshape((len(probs),) + tuple(shape))
    out["n_nonfinite"] = sum(c["nonfinite"] for c in cols)
    out["columns"] = cols
    return out


@functools.lru_cache(maxsize=None)
def fixture_reference(C, R, max_lag=0):
    """The longdouble summary of fixture(C, R): computed once, shared, read-only."""
    return summarize(fixture(C, R), PROBS, max_lag)


def check_against(got, ref, sigma_theta=False):
    """The device result ``got`` (MagiEngine.summarize's dict) against ``ref`` (summarize above, longdouble) at the derived tolerances:
    mean 1e-12 max|y|; sd, rhat, ess, mcse_mean rtol 1e-13 kappa + 1e-11; quantiles 4 ulp of max(|v_lo|, |v_hi|) (``sigma_theta``: the
    columns went through the device's softplus, 1e-14 relative on the order statistics on top).  Returns the worst error as a fraction of
    its bar, per statistic."""
    worst = {}
    cols = ref["columns"]
    flat = lambda a: np.asarray(a).reshape(-1)
    gq, rq = np.asarray(got["quantiles"]).reshape(len(got["probs"]), -1), np.asarray(ref["quantiles"]).reshape(len(got["probs"]), -1)
    for k, c in enumerate(cols):
        if c["nonfinite"] or c["order"] is None:
            for s in ("mean", "sd", "rhat", "ess", "mcse_mean"):
                assert np.isnan(flat(got[s])[k]), (s, k)
            assert np.all(np.isnan(gq[:, k])), k
            continue
        v = c["order"]
        S = v.shape[0]
        amax = np.abs(v).max()
        bar = 1e-12 * amax
        err = abs(np.longdouble(flat(got["mean"])[k]) - flat(ref["mean"])[k])
        worst["mean"] = max(worst.get("mean", 0.0), float(err / bar) if bar > 0 else float(err))
        assert err <= bar, ("mean", k, float(err), bar)
        for q, p in enumerate(got["probs"]):
            h = np.float64(S - 1) * np.float64(p)
            lo = int(np.floor(h))
            hi = min(lo + 1, S - 1)
            scale = max(abs(v[lo]), abs(v[hi]))
            bar = 4.0 * np.spacing(scale) + (1e-14 * scale if sigma_theta else 0.0)
            err = abs(np.longdouble(gq[q, k]) - rq[q, k])
            worst["quantiles"] = max(worst.get("quantiles", 0.0), float(err / bar) if bar > 0 else float(err))
            assert err <= bar, ("quantile", k, p, float(err), bar)
        for s in ("sd", "rhat", "ess", "mcse_mean"):
            r, g = flat(ref[s])[k], flat(got[s])[k]
            if np.isnan(r):
                assert np.isnan(g), (s, k, g)
                continue
            if s == "sd" and r == 0:
                assert g == 0.0, (s, k, g)               # a constant column: exactly 0
                continue
            rt = rtol_spread(c["kappa"] if c["kappa"] is not None else float(amax / r))
            err = abs(np.longdouble(g) - r) / abs(r)
            worst[s] = max(worst.get(s, 0.0), float(err / rt))
            assert err <= rt, (s, k, float(err), rt)
    assert got["n_nonfinite"] == ref["n_nonfinite"]
    return worst
