"""CPU truth for the rank-normalised diagnostics (magi_rank_diagnostics, magi_sampler_rank_diagnostics; tests/test_rank_cpu.py,
tests/test_rank_gpu.py): the definitions of include/magi_hip.h transcribed in numpy, in float64 or longdouble, with the deliberately
wrong definitions the CPU test holds the device tolerances against.  A helper module: product code never imports it.

Per column y[c][r] (C chains, R draws), S = C R pooled draws, v = sort(pooled):
  rank[s] = #(y < y[s]) + (#(y == y[s]) + 1) / 2 (1-based average rank; == ties -0.0 with +0.0), pooled also for odd R;
  z[s] = Phi^-1((rank[s] - 3/8) / (S + 1/4)) -- the fraction formed in float64, as the device forms it; Phi^-1 from mpmath at 50 digits in
  the longdouble transcription (rounded to float64 for the statistics: they are statistics of float64 series), scipy's ndtri in float64;
  zf = the same transform of f = |y - med| in float64, med = summary_reference's quantile at 0.5 in float64 (g is 0 or 1/2: every operation
  of it is the device's, fused or not);
  I_p[s] = 1 if y[s] <= v[floor((S - 1) p)] else 0, p = tail_prob and 1 - tail_prob (float64);
  ess_bulk = ess(z); rhat_rank = max(rhat(z), rhat(zf)), NaN if either is; ess_tail = min(ess(I_lo), ess(I_hi)), NaN if either is --
  rhat and ess those of summary_reference.column (the section 4.4 split, truncation, max_lag and floor).
  A series whose split chains are all one constant (an odd R drops the middle draw, which may be the only one that differs) has neither.
  A non-finite draw: everything NaN, the column counts in n_nonfinite."""
import functools

import numpy as np

import summary_reference as sr

RANK_LDS = 8192                   # csrc/rank.hip: keys a workgroup sorts in LDS (tests/test_rank_cpu.py compares it with the source)
TAIL_PROB = 0.05
U = 2.0 ** -53

# z: the worst error of scipy.special.ndtri against mpmath over the rank fractions of every fixture shape, in units of U max(1, |z|), as
# tests/test_rank_cpu.py measures it again, and the device's bar: 4 x that (its erf / erfc / log are other implementations, a few ulp apart)
Z_ERR_NDTRI = 7.0
Z_BAR = 4.0 * Z_ERR_NDTRI

K_BASE = sr.K_FIXTURE
COL_TIED, COL_PM0, COL_CAUCHY, COL_SCALE, COL_TOP = K_BASE, K_BASE + 1, K_BASE + 2, K_BASE + 3, K_BASE + 4
K_FIXTURE = K_BASE + 5
# C R on both sides of the LDS sort's capacity, and one beyond twice that which is no power of two; odd R, R = 4, several chains
SHAPES = ((1, 4), (1, 5), (2, 65), (3, 257), (4, 1000), (1, RANK_LDS - 1), (2, RANK_LDS // 2), (1, RANK_LDS + 1), (3, 5500))
VARIANTS = ("ordinal_ranks", "fraction_r_over_S_plus_1", "no_folding", "lower_tail_only", "fmin_over_nan_leg", "ties_by_key")
SERIES = ("z", "zf", "lo", "hi")
# per fixture column a seed offset: change a column's entry when one of its truncation decisions sits on a rounding edge
SEED_OFFSET = {COL_TIED: 0, COL_PM0: 0, COL_CAUCHY: 1, COL_SCALE: 0, COL_TOP: 0}


def lag_for(C, R):
    """The max_lag a shape runs with: all lags up to (4, 1000), 64 beyond (the longdouble reference stays within seconds)."""
    return 0 if C * R <= 4000 else 64


@functools.lru_cache(maxsize=None)
def fixture(C, R):
    """[C][R][K_FIXTURE] draws: summary_reference.fixture's eleven columns, then a heavily tied column (AR(1) rounded to 0 .. 9), a column
    whose only ties are -0.0 against +0.0, a Cauchy column, chains of equal mean and scales 1 : 3 (one chain: its halves), and a column whose
    top tenth is one tied value.  Read-only."""
    y = np.empty((C, R, K_FIXTURE))
    y[:, :, :K_BASE] = sr.fixture(C, R)
    rng = lambda col: np.random.default_rng(7000 + 100 * C + R + 100003 * (col - K_BASE) + 1000003 * SEED_OFFSET[col])
    g = rng(COL_TIED)
    e = g.standard_normal((C, R))
    x = np.empty((C, R))
    x[:, 0] = e[:, 0] / np.sqrt(0.75)
    for r in range(1, R):
        x[:, r] = 0.5 * x[:, r - 1] + e[:, r]
    y[:, :, COL_TIED] = np.clip(np.rint(4.5 + 1.5 * x), 0.0, 9.0)
    g = rng(COL_PM0)
    x = g.standard_normal((C, R))
    zero = g.random((C, R)) < 0.3
    zero.reshape(-1)[:2] = True                                       # (both signs also at S = 4)
    sign = g.random((C, R)) < 0.5
    sign.reshape(-1)[:2] = (True, False)
    y[:, :, COL_PM0] = np.where(zero, np.where(sign, -0.0, 0.0), x)
    y[:, :, COL_CAUCHY] = rng(COL_CAUCHY).standard_cauchy((C, R))
    scale = np.where(np.arange(C) % 2 == 0, 1.0, 3.0)[:, None] * np.ones((1, R))
    if C == 1:
        scale = np.where(np.arange(R) < R // 2, 1.0, 3.0)[None, :]
    y[:, :, COL_SCALE] = 2.0 + scale * rng(COL_SCALE).standard_normal((C, R))
    x = rng(COL_TOP).standard_normal((C, R))
    S = C * R
    y[:, :, COL_TOP] = np.minimum(x, np.sort(x.reshape(-1))[int(np.floor(0.9 * (S - 1)))])
    y.setflags(write=False)
    return y


# ---- the definitions ----------------------------------------------------------------------------------------------------------------

def rankdata(y, variant=None):
    """1-based average ranks of the flat float64 array y (scipy.stats.rankdata(method="average"): == ties -0.0 with +0.0)."""
    y = np.asarray(y, dtype=np.float64)
    if variant == "ordinal_ranks":
        r = np.empty(y.shape[0])
        r[np.argsort(y, kind="stable")] = np.arange(1, y.shape[0] + 1)
        return r
    if variant == "ties_by_key":                                      # the order of the sort's keys: -0.0 before +0.0
        b = y.view(np.uint64)
        y = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    v = np.sort(y)
    return 0.5 * (np.searchsorted(v, y, "left") + np.searchsorted(v, y, "right") + 1)


def fractions(rank, S, variant=None):
    """The argument of Phi^-1 in float64, as the device forms it."""
    if variant == "fraction_r_over_S_plus_1":
        return np.asarray(rank, dtype=np.float64) / np.float64(S + 1)
    return (np.asarray(rank, dtype=np.float64) - np.float64(0.375)) / (np.float64(S) + np.float64(0.25))


_PHI_INV = {}                     # lower-tail fraction (a float) -> Phi^-1 of exactly that float64, as a longdouble


def phi_inv_exact(p):
    """Phi^-1 of the float64 array p (0 < p < 1), each entry taken as the exact number it is: two Newton steps on erfc at 50 digits from
    scipy's ndtri, rounded to longdouble.  Cached; p > 1/2 goes through 1 - p (exact in float64)."""
    import mpmath as mp
    from scipy.special import ndtri
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(-1)
    low = np.where(flat <= 0.5, flat, 1.0 - flat)
    uniq = np.unique(low)
    need = [v for v in uniq.tolist() if v not in _PHI_INV]
    if need:
        with mp.workdps(50):
            r2, c = mp.sqrt(2), 1 / mp.sqrt(2 * mp.pi)
            for v, x0 in zip(need, ndtri(np.array(need)).tolist()):
                x, pm = mp.mpf(x0), mp.mpf(v)
                for _ in range(2):
                    x -= (mp.erfc(-x / r2) / 2 - pm) / (c * mp.exp(-x * x / 2))
                _PHI_INV[v] = np.longdouble(mp.nstr(x, 30))
    vals = np.array([_PHI_INV[v] for v in uniq.tolist()], dtype=np.longdouble)
    out = vals[np.searchsorted(uniq, low)]
    return np.where(flat <= 0.5, out, -out).reshape(p.shape)


def z_scores(y, dtype, variant=None):
    """(rank, z as float64, z as dtype) of the flat array y."""
    from scipy.special import ndtri
    rank = rankdata(y, variant)
    p = fractions(rank, y.shape[0], variant)
    zz = ndtri(p) if dtype is np.float64 else phi_inv_exact(p)
    return rank, np.asarray(zz, dtype=np.float64), zz


def column(y, max_lag=0, tail_prob=TAIL_PROB, dtype=np.longdouble, variant=None):
    """One column y[C][R] -> dict(nonfinite, rank, rank_f (of the folded draws), z, zf (float64 [C][R]), z_exact, zf_exact (dtype), rhat_rank, ess_bulk, ess_tail (dtype),
    legs: per series of SERIES the dict of summary_reference.column -- rhat, ess and the conditioning of its truncation decision)."""
    assert variant is None or variant in VARIANTS
    y = np.asarray(y, dtype=np.float64)
    C, R = y.shape
    S = C * R
    nan = dtype(np.nan)
    out = dict(nonfinite=False, rank=np.full((C, R), np.nan), z=np.full((C, R), np.nan), zf=np.full((C, R), np.nan), z_exact=None, zf_exact=None,
               rhat_rank=nan, ess_bulk=nan, ess_tail=nan, legs=None)
    if not np.all(np.isfinite(y)):
        out["nonfinite"] = True
        return out
    flat = y.reshape(-1)
    v = np.sort(flat)
    rank, z, z_exact = z_scores(flat, dtype, variant)
    med = sr.quantiles(v, (0.5,), np.float64)[0]
    rank_f, zf, zf_exact = z_scores(np.abs(flat - med), dtype, variant)
    ind = lambda p: (flat <= v[int(np.floor(np.float64(S - 1) * np.float64(p)))]).astype(np.float64)
    series = dict(z=z, zf=zf, lo=ind(np.float64(tail_prob)), hi=ind(np.float64(1.0) - np.float64(tail_prob)))
    legs = {name: sr.column(a.reshape(C, R), (), max_lag, dtype) for name, a in series.items()}
    out.update(rank=rank.reshape(C, R), rank_f=rank_f.reshape(C, R), z=z.reshape(C, R), zf=zf.reshape(C, R), z_exact=z_exact.reshape(C, R), zf_exact=zf_exact.reshape(C, R), legs=legs)
    # a series without a split R-hat has no ESS: the constant series, and split chains that are all one constant (W = var+ = 0)
    ess_of = lambda leg: nan if np.isnan(leg["rhat"]) else leg["ess"]
    out["ess_bulk"] = ess_of(legs["z"])
    a, b = legs["z"]["rhat"], legs["zf"]["rhat"]
    out["rhat_rank"] = a if variant == "no_folding" else nan if (np.isnan(a) or np.isnan(b)) else max(a, b)
    lo, hi = ess_of(legs["lo"]), ess_of(legs["hi"])
    if variant == "lower_tail_only":
        out["ess_tail"] = lo
    elif variant == "fmin_over_nan_leg":
        out["ess_tail"] = np.fmin(lo, hi)
    else:
        out["ess_tail"] = nan if (np.isnan(lo) or np.isnan(hi)) else min(lo, hi)
    return out


def diagnostics(draws, max_lag=0, tail_prob=TAIL_PROB, dtype=np.longdouble, variant=None):
    """draws [C][R] + shape -> dict(rhat_rank, ess_bulk, ess_tail of that shape; rank, z, z_folded of the shape of draws; n_nonfinite;
    columns: the per-column dicts of ``column`` in C order)."""
    draws = np.asarray(draws, dtype=np.float64)
    C, R, shape = draws.shape[0], draws.shape[1], draws.shape[2:]
    flat = draws.reshape(C, R, -1)
    cols = [column(flat[:, :, k], max_lag, tail_prob, dtype, variant) for k in range(flat.shape[2])]
    out = {s: np.array([c[s] for c in cols], dtype=dtype).reshape(shape) for s in ("rhat_rank", "ess_bulk", "ess_tail")}
    for name, key in (("rank", "rank"), ("z", "z"), ("z_folded", "zf")):
        out[name] = np.stack([c[key] for c in cols], axis=-1).reshape(draws.shape)
    out["n_nonfinite"] = sum(c["nonfinite"] for c in cols)
    out["columns"] = cols
    return out


@functools.lru_cache(maxsize=None)
def fixture_reference(C, R):
    """The longdouble diagnostics of fixture(C, R) at lag_for(C, R): computed once, shared, read-only."""
    return diagnostics(fixture(C, R), lag_for(C, R))


# ---- tolerances ---------------------------------------------------------------------------------------------------------------------

def z_error(got, exact):
    """The worst error of the float64 scores ``got`` against ``exact`` (longdouble) in units of U max(1, |z|)."""
    exact = np.asarray(exact, dtype=np.longdouble)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - exact) / (U * np.maximum(1.0, np.abs(exact)))
    return float(err.max())


def perturbation_effect(zs, C, R, max_lag):
    """The first-order effect on (rhat, ess) of a z error of the size of the device's bar: the largest relative change under three sign
    patterns of z (1 +- Z_BAR U max(1, |z|) / |z|) -- two random ones and one that alternates along the chain."""
    base = sr.column(zs.reshape(C, R), (), max_lag)
    worst = [0.0, 0.0]
    signs = [np.random.default_rng(s).choice([-1.0, 1.0], size=zs.shape) for s in (0, 1)] + [np.where(np.arange(zs.shape[0]) % 2 == 0, 1.0, -1.0)]
    for sg in signs:
        c = sr.column((zs + sg * Z_BAR * U * np.maximum(1.0, np.abs(zs))).reshape(C, R), (), max_lag)
        for i, s in enumerate(("rhat", "ess")):
            if np.isfinite(base[s]) and np.isfinite(c[s]):
                worst[i] = max(worst[i], float(abs(c[s] - base[s]) / abs(base[s])))
    return worst


@functools.lru_cache(maxsize=None)
def fixture_bars(C, R):
    """Per fixture column the relative bars (rhat_rank, ess_bulk, ess_tail) of the device against fixture_reference(C, R), or None for
    a column without diagnostics: summary_reference.rtol_spread(kappa) of the series a leg is a statistic of, plus -- for the statistics
    of z and zf -- the effect of a z error of the size of Z_BAR; the indicators are exact."""
    bars = []
    for c in fixture_reference(C, R)["columns"]:
        legs = c["legs"]
        if legs is None or legs["z"]["kappa"] is None:
            bars.append(None)
            continue
        lag = lag_for(C, R)
        leg_bar = {}
        for name in ("z", "zf"):
            if legs[name]["kappa"] is None:
                leg_bar[name] = (np.nan, np.nan)
                continue
            dr, de = perturbation_effect(c[name].reshape(-1), C, R, lag)
            rt = sr.rtol_spread(legs[name]["kappa"])
            leg_bar[name] = (rt + dr, rt + de)
        tail = [sr.rtol_spread(legs[name]["kappa"]) for name in ("lo", "hi") if legs[name]["kappa"] is not None]
        bars.append(dict(rhat_rank=float(np.nanmax([leg_bar["z"][0], leg_bar["zf"][0]])), ess_bulk=leg_bar["z"][1],
                         ess_tail=max(tail) if tail else np.nan))
    return bars


def check_against(got, ref, bars):
    """The device result ``got`` (MagiEngine.rank_diagnostics(return_z=True)'s dict, K columns flat) against ``ref`` (diagnostics above,
    longdouble) at ``bars`` (fixture_bars): ranks bit-exact, z and z_folded within Z_BAR U max(1, |z|), the three diagnostics within
    their relative bars, the NaN pattern and n_nonfinite equal.  Returns the worst error as a fraction of its bar, per quantity."""
    worst = {}
    C, R = got["rank"].shape[:2]
    g3 = lambda a: np.asarray(a).reshape(C, R, -1)
    for k, c in enumerate(ref["columns"]):
        rank, z, zf = g3(got["rank"])[:, :, k], g3(got["z"])[:, :, k], g3(got["z_folded"])[:, :, k]
        if c["nonfinite"]:
            assert np.all(np.isnan(rank)) and np.all(np.isnan(z)) and np.all(np.isnan(zf)), k
        else:
            np.testing.assert_array_equal(rank, c["rank"], err_msg=f"rank of column {k}")
            for name, a, exact in (("z", z, c["z_exact"]), ("z_folded", zf, c["zf_exact"])):
                e = z_error(a, exact) / Z_BAR
                worst[name] = max(worst.get(name, 0.0), e)
                assert e <= 1.0, (name, k, e * Z_BAR, Z_BAR)
        for s in ("rhat_rank", "ess_bulk", "ess_tail"):
            r, g = c[s], np.asarray(got[s]).reshape(-1)[k]
            if not np.isfinite(r):                                    # (NaN: no diagnostic; inf: split chains that are constant and differ, W = 0)
                assert np.isnan(g) if np.isnan(r) else g == r, (s, k, g)
                continue
            err = float(abs(np.longdouble(g) - r) / abs(r)) / bars[k][s]
            worst[s] = max(worst.get(s, 0.0), err)
            assert err <= 1.0, (s, k, float(g), float(r), err * bars[k][s], bars[k][s])
    assert got["n_nonfinite"] == ref["n_nonfinite"]
    return worst
