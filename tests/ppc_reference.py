"""CPU truth for the device's posterior predictive checks (magi_ppc, magi_sampler_ppc; tests/test_ppc_cpu.py, tests/test_ppc_gpu.py): the
definitions of include/magi_hip.h restated in numpy, in float64 or longdouble, with the deliberately wrong definitions the CPU test holds
the device bars against, and the fixture tables both test files use.  A helper module: product code never imports it.

Draw s = c R + r of S = C R; column k of component comp[k]; link g_d (0 identity, 1 log, 2 sqrt), weight w_k, variance sigma^2_d(s) on the
link's scale, datum y_k (NaN: none).  One Philox4x32-10 block per (s, k): philox4x32(k, r, chain_id[c], STREAM_PPC, seed) -> u1, u2 ->
rad = sqrt(-2 log u1), ang = 2 pi u2, z0 = rad cos ang, z1 = rad sin ang (the oracle's generator, imported unchanged).
  x_lat = x + sqrt(extra_var) z1;  gy_rep = g(x_lat) + sqrt(sigma^2 / w) z0;  y_rep = g^-1(gy_rep) (identity; exp; max(., 0)^2), NaN where
  g(x_lat) is not finite;  u_obs = (g(y) - g(x_lat)) sqrt(w / sigma^2);  pit_k = mean_s 1/2 erfc(-u_obs / sqrt 2) (NaN: no datum, or a
  non-finite term).  Per (s, d), over the columns of d with a datum, ascending, for u = u_obs and for u = z0:
  T = (sum u^2, sum u / n, max |u|, sum_j u_j u_(j+1) / sum u^2 (n < 2: NaN));  pval[d][t] = #{T_rep >= T_obs} / #{both finite};
  n_T_excluded[d] = #{s: a defined T of (s, d) is not finite}."""
import functools

import numpy as np

from oracle.magi_oracle import _u01, philox4x32

STREAM_PPC = 5
STATS = ("chi2", "mean", "maxabs", "acf1")
COMPARED = ("y_rep", "pit", "T_obs", "T_rep", "mean", "sd", "quantiles")
PROBS = (0.025, 0.5, 0.975)

# ---- the bars of the device comparison --------------------------------------------------------------------------------------------------
# |device - longdouble| <= BAR[q] * scale, with the scale the reference states per entry (``ppc`` below: what one rounding of an input of
# that entry becomes in it).  Each constant is 100 x the largest float64 / longdouble distance of this reference, in units of the scale,
# over the whole fixture table FIXTURES; tests/test_ppc_cpu.py recomputes them and asserts that these constants are those numbers rounded
# up (by at most a quarter).
# A DEVIATION from the issue's wording, which asks for "100 x the largest float64-against-longdouble difference" and names no unit: the
# differences are taken, and the bars applied, relative to that per-entry scale (>= 1: max(1, |y_rep|) max(1, |gy_rep|) for a replicate and
# its column statistics; 1 for pit; for T the count n, the largest |u| and the conditioning of u -- (|g(x)| + |g(y)|) sqrt(w / sigma^2) + |u|
# for u_obs, 8 max(1, rad) for z0 -- combined as first-order error propagation gives them, see the end of ``ppc``).  The formulas are chosen by
# hand from that reasoning, not fitted to the device; where the scale is 1 the bar is the literal absolute one.
MARGIN = 100.0
BAR = {"y_rep": 8.5e-14, "pit": 1.1e-13, "T_obs": 9.6e-15, "T_rep": 1.3e-14, "mean": 2.9e-14, "sd": 1.3e-14, "quantiles": 3.5e-14}

FAULTS = ("weights_ignored", "weights_not_under_root", "sigma_natural_scale", "no_inverse_link", "sqrt_not_clamped", "z1_for_z0", "r_ignored",
          "chain_ignored", "k_r_swapped", "stream_momentum", "extra_var_ignored", "acf1_centred", "fixed_ignored", "nan_y_counted", "pit_from_ranks")

# ---- calibration (tests/test_ppc_cpu.py): seeds at which the REFERENCE alone meets the condition of the issue -- data generated from the
# model itself, n_obs = 400 over two components, S = 512: pit_ks < 1.95 / sqrt(n) per component and every p-value inside [0.01, 0.99]; a
# sinusoidal misfit of two noise sd gives an acf1 p-value below 0.01.  data_seed draws the data and the posterior draws, noise_seed is the
# Philox seed of the replicates.
CALIBRATION = {"data_seed": 11, "noise_seed": 2024, "C": 2, "R": 256, "n_per_component": 200, "period": 50.0, "misfit_sd": 2.0}


def erfc(x, dtype=np.longdouble):
    """erfc in ``dtype`` without a library: |x| < 2 by the all-positive series erf x = 2 / sqrt(pi) e^(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!,
    beyond it by the continued fraction e^(-x^2) / (sqrt(pi) (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))), 120 levels."""
    if dtype == np.float64:
        from scipy.special import erfc as erfc64
        return erfc64(np.asarray(x, dtype=np.float64))
    x = np.asarray(x, dtype=dtype)
    a = np.abs(x)
    pi = np.arccos(dtype(-1))
    out = np.full(x.shape, dtype(np.nan))
    with np.errstate(all="ignore"):
        small = a < 2
        xs = np.where(small, a, dtype(0))
        term = xs.copy()
        acc = xs.copy()
        for n in range(1, 90):
            term = term * (dtype(2) * xs * xs) / dtype(2 * n + 1)
            acc = acc + term
        erf_s = dtype(2) / np.sqrt(pi) * np.exp(-xs * xs) * acc
        xl = np.where(small, dtype(2), a)
        t = xl.copy()
        for k in range(120, 0, -1):
            t = xl + dtype(k) / dtype(2) / t
        erfc_l = np.exp(-xl * xl) / (np.sqrt(pi) * t)
        pos = np.where(small, dtype(1) - erf_s, erfc_l)
        out = np.where(x >= 0, pos, dtype(2) - pos)
    return np.where(np.isnan(x), dtype(np.nan), out)


def link_g(link, v):
    with np.errstate(all="ignore"):
        return np.log(v) if int(link) == 1 else np.sqrt(v) if int(link) == 2 else v + 0


def sigma_sq_of(sig_pre, LB, fixed=None, dtype=np.float64, fault=None):
    """sigma^2 [.., D] of sig_pre [.., D]: softplus + LB[d], or the constant of a fixed component (``fixed`` {d: c})."""
    sp = np.asarray(sig_pre, dtype=np.float64).astype(dtype)
    s2 = np.log(dtype(1) + np.exp(sp)) + np.asarray(LB, dtype=np.float64).astype(dtype)
    if fixed and fault != "fixed_ignored":
        for d, c in fixed.items():
            s2[..., d] = dtype(c)
    return s2


def noise(C, R, K, seed, chain_ids=None, dtype=np.longdouble, fault=None):
    """(z0, z1, rad) [C R][K]."""
    S = C * R
    ids = np.arange(C) if chain_ids is None else np.asarray(chain_ids)
    k = np.arange(K, dtype=np.uint64)[None, :]
    r = (np.arange(S) % R).astype(np.uint64)[:, None]
    cid = (np.asarray(ids, dtype=np.int64)[np.arange(S) // R] & 0xFFFFFFFF).astype(np.uint64)[:, None]
    if fault == "r_ignored":
        r = np.zeros_like(r)
    if fault == "chain_ignored":
        cid = np.zeros_like(cid)
    if fault == "k_r_swapped":
        k, r = r, k
    r0, r1, r2, r3 = philox4x32(k, r, cid, 0 if fault == "stream_momentum" else STREAM_PPC, int(seed))
    u1, u2 = _u01(r0, r1).astype(dtype), _u01(r2, r3).astype(dtype)
    pi = np.arccos(dtype(-1))
    rad = np.sqrt(dtype(-2) * np.log(u1))
    ang = dtype(2) * pi * u2
    z0, z1 = rad * np.cos(ang), rad * np.sin(ang)
    if fault == "z1_for_z0":
        z0, z1 = z1, z0
    return z0, z1, rad


def discrepancies(u, cols, dtype, centred=False):
    """u [S][K], cols: the column indices of one component, ascending -> T [S][4]."""
    S = u.shape[0]
    n = len(cols)
    T = np.full((S, 4), dtype(np.nan))
    if n == 0:
        return T
    v = u[:, cols]
    with np.errstate(all="ignore"):
        T[:, 0] = (v * v).sum(axis=1)
        T[:, 1] = v.sum(axis=1) / dtype(n)
        T[:, 2] = np.abs(v).max(axis=1)
        if n >= 2:
            c = v - v.mean(axis=1, keepdims=True) if centred else v
            T[:, 3] = (c[:, :-1] * c[:, 1:]).sum(axis=1) / (c * c).sum(axis=1)
    return T


def quantiles(col, probs, dtype):
    """numpy's "linear" method on the column's float64 order, in dtype."""
    v = np.sort(col)
    S = v.shape[0]
    out = []
    for p in probs:
        hq = (S - 1) * float(p)
        lo = min(max(int(np.floor(hq)), 0), S - 1)
        g = dtype(hq - lo)
        hi = min(lo + 1, S - 1)
        out.append(v[lo] if g == 0 else v[lo] + g * (v[hi] - v[lo]))
    return out


def ppc(x, comp, sigma_sq, link=None, weight=None, y=None, extra_var=None, seed=0, chain_ids=None, probs=PROBS, dtype=np.longdouble, fault=None):
    """x [C][R][K], sigma_sq [C][R][D] (float64 bits) -> dict of y_rep [S][K], pit [K], T_obs, T_rep [S][D][4], pval [D][4], n_T_excluded [D],
    mean, sd [K], quantiles [n_q][K], n_nonfinite, u_obs, z0, and ``scale`` {name: array}: the size of one rounding's effect per entry."""
    x = np.asarray(x, dtype=np.float64)
    C, R, K = x.shape
    S = C * R
    s2a = np.asarray(sigma_sq, dtype=np.float64).reshape(S, -1).astype(dtype)
    D = s2a.shape[1]
    comp = np.asarray(comp, dtype=np.int64)
    links = np.zeros(D, dtype=int) if link is None else np.asarray(link)
    w = np.ones(K) if weight is None or fault == "weights_ignored" else np.asarray(weight, dtype=np.float64)
    w = w.astype(dtype)
    yv = np.full(K, np.nan) if y is None else np.asarray(y, dtype=np.float64)
    has = ~np.isnan(yv)
    z0, z1, rad = noise(C, R, K, seed, chain_ids, dtype, fault)
    xl = x.reshape(S, K).astype(dtype)
    if extra_var is not None and fault != "extra_var_ignored":
        xl = xl + np.sqrt(np.asarray(extra_var, dtype=np.float64).astype(dtype))[None, :] * z1
    y_rep = np.empty((S, K), dtype=dtype)
    u_obs = np.empty((S, K), dtype=dtype)
    gyr = np.empty((S, K), dtype=dtype)
    cond_u = np.empty((S, K), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            d, lk = comp[k], links[comp[k]]
            s2 = s2a[:, d]
            gx = link_g(lk, xl[:, k])
            gy = link_g(lk, dtype(yv[k]))
            if fault == "weights_not_under_root":
                sdv, isd = np.sqrt(s2) / w[k], w[k] / np.sqrt(s2)
            else:
                sdv, isd = np.sqrt(s2 / w[k]), np.sqrt(w[k] / s2)
            gr = link_g(lk, xl[:, k] + sdv * z0[:, k]) if fault == "sigma_natural_scale" else gx + sdv * z0[:, k]
            if fault == "no_inverse_link" or lk == 0:
                yr = gr + 0
            elif lk == 1:
                yr = np.exp(gr)
            else:
                t = gr if fault == "sqrt_not_clamped" else np.maximum(gr, dtype(0))
                yr = t * t
            yr = np.where(np.isfinite(gx), yr, dtype(np.nan))
            y_rep[:, k], gyr[:, k] = yr, gr
            u_obs[:, k] = (gy - gx) * isd
            cond_u[:, k] = (np.abs(u_obs[:, k]) + (np.abs(gx) + np.abs(gy)) * isd).astype(np.float64)
    # per column
    pit = np.full(K, dtype(np.nan))
    with np.errstate(all="ignore"):
        for k in np.nonzero(has)[0]:
            if fault == "pit_from_ranks":
                pit[k] = dtype((y_rep[:, k].astype(np.float64) <= yv[k]).mean())
            elif np.all(np.isfinite(u_obs[:, k].astype(np.float64))):
                pit[k] = (dtype(0.5) * erfc(-u_obs[:, k] / np.sqrt(dtype(2)), dtype)).sum() / dtype(S)
    mean = np.full(K, dtype(np.nan))
    sd = np.full(K, dtype(np.nan))
    quant = np.full((len(probs), K), dtype(np.nan))
    n_nonfinite = 0
    y64 = y_rep.astype(np.float64)
    for k in range(K):
        if not np.all(np.isfinite(y64[:, k])):
            n_nonfinite += 1
            continue
        mean[k] = y_rep[:, k].sum() / dtype(S)
        if S >= 2:
            sd[k] = np.sqrt(((y_rep[:, k] - mean[k]) ** 2).sum() / dtype(S - 1))
        quant[:, k] = quantiles(y_rep[:, k], probs, dtype)
    # per draw and component
    T_obs = np.full((S, D, 4), dtype(np.nan))
    T_rep = np.full((S, D, 4), dtype(np.nan))
    sc_obs = np.ones((S, D, 4))
    sc_rep = np.ones((S, D, 4))
    pval = np.full((D, 4), np.nan)
    n_excl = np.zeros(D, dtype=np.int64)
    for d in range(D):
        cols = np.nonzero((comp == d) & (has | (fault == "nan_y_counted")))[0]
        n = len(cols)
        if n == 0:
            continue
        T_obs[:, d] = discrepancies(u_obs, cols, dtype, fault == "acf1_centred")
        T_rep[:, d] = discrepancies(z0, cols, dtype, fault == "acf1_centred")
        for T, sc, cn, a in ((T_obs, sc_obs, cond_u[:, cols].max(axis=1), np.abs(u_obs[:, cols]).astype(np.float64).max(axis=1)),
                             (T_rep, sc_rep, 8.0 * np.maximum(1.0, rad[:, cols].astype(np.float64).max(axis=1)),
                              np.abs(z0[:, cols]).astype(np.float64).max(axis=1))):
            with np.errstate(all="ignore"):
                cn = np.maximum(1.0, cn)
                a = np.maximum(1.0, a)
                t0, t3 = T[:, d, 0].astype(np.float64), T[:, d, 3].astype(np.float64)
                sc[:, d, 0] = n * a * cn
                sc[:, d, 1] = cn
                sc[:, d, 2] = cn
                sc[:, d, 3] = np.maximum(1.0, n * a * cn * (1.0 + np.abs(t3)) / t0)
        to, tr = T_obs[:, d].astype(np.float64), T_rep[:, d].astype(np.float64)
        defined = 4 if n >= 2 else 3
        both = np.isfinite(to) & np.isfinite(tr)
        for t in range(4):
            if both[:, t].any():
                pval[d, t] = float((tr[both[:, t], t] >= to[both[:, t], t]).sum()) / float(both[:, t].sum())
        n_excl[d] = int((~both[:, :defined]).any(axis=1).sum())
    sy = np.maximum(1.0, np.abs(y64)) * np.maximum(1.0, np.abs(gyr.astype(np.float64)))
    sy = np.where(np.isfinite(sy), sy, 1.0)
    scol = sy.max(axis=0)
    return {"y_rep": y_rep, "pit": pit, "T_obs": T_obs, "T_rep": T_rep, "pval": pval, "n_T_excluded": n_excl, "mean": mean, "sd": sd,
            "quantiles": quant, "n_nonfinite": n_nonfinite, "u_obs": u_obs, "z0": z0,
            "scale": {"y_rep": sy, "pit": np.ones(K), "T_obs": sc_obs, "T_rep": sc_rep, "mean": scol, "sd": scol, "quantiles": np.broadcast_to(scol, quant.shape)}}


def distance(got, ref, names=COMPARED):
    """Per compared quantity the largest |got - ref| / scale over the entries finite in ref; inf where the two differ in which entries are
    finite.  ``got``: name -> array (float64 or longdouble), ``ref``: ``ppc`` above."""
    out = {}
    for q in names:
        g, r = np.asarray(got[q]).reshape(np.asarray(ref[q]).shape), np.asarray(ref[q])
        fin = np.isfinite(r.astype(np.float64))
        if not np.array_equal(np.isfinite(g.astype(np.float64)), fin):
            out[q] = np.inf
            continue
        err = np.abs(g[fin].astype(np.longdouble) - r[fin].astype(np.longdouble)).astype(np.float64)
        out[q] = float((err / np.asarray(ref["scale"][q])[fin]).max()) if err.size else 0.0
    return out


def check_against(got, ref, names=COMPARED):
    """The device's arrays against ``ref`` (longdouble) at BAR; non-finite entries must coincide, pval and n_T_excluded agree exactly.
    Returns the worst error as a fraction of its bar, per quantity."""
    worst = {q: v / BAR[q] for q, v in distance(got, ref, names).items()}
    for q, v in worst.items():
        assert v <= 1.0, (q, v)
    if "pval" in got:
        np.testing.assert_array_equal(np.asarray(got["pval"], dtype=np.float64), ref["pval"])
    if "n_T_excluded" in got:
        np.testing.assert_array_equal(np.asarray(got["n_T_excluded"], dtype=np.int64), ref["n_T_excluded"])
    if "n_nonfinite" in got:
        assert int(got["n_nonfinite"]) == ref["n_nonfinite"]
    return worst


def knife_edge(ref):
    """The smallest |T_rep - T_obs| / (scale_obs + scale_rep) over the draws where both are finite: in units of a bar of 1."""
    to, tr = ref["T_obs"].astype(np.float64), ref["T_rep"].astype(np.float64)
    both = np.isfinite(to) & np.isfinite(tr)
    if not both.any():
        return np.inf
    return float((np.abs(tr - to)[both] / (ref["scale"]["T_obs"] + ref["scale"]["T_rep"])[both]).min())


# ---- the GPU fixture table -----------------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1), (1, 5), (2, 33), (3, 67))            # C x R: S below, at (66: a full tile and two rows) and above a 64-row tile
KS = (1, 63, 65, 130)
CHAIN_IDS = (7, 2, 5)
LB = (2e-4, 5e-4, 1e-4)
DOMAIN_DRAWS = (3, 40)                                  # pooled draws of the domain case with x <= 0 under the log link (column DOMAIN_COLUMN)
DOMAIN_COLUMN = 5
DOMAIN = (2, 33, 65)
FIXTURES = tuple((C, R, K, False) for C, R in SHAPES for K in KS) + (DOMAIN + (True,),)
SEED = 20240611


@functools.lru_cache(maxsize=None)
def crafted(C, R, K, domain=False):
    """One fixture, read-only arrays: dict(x [C][R][K], comp, sig_pre, sigma_sq [C][R][3], link, weight, y, extra_var (None on every
    second fixture), chain_ids (CHAIN_IDS[:C] on every third, else None), fixed, seed, n_excluded [3]).  D = 3: component 1 owns no
    column, component 2 a single datum (and, K >= 3, a column without one), component 0 the rest with every seventh datum missing;
    links rotate through the three; weights 1 / 2 / 4; every fifth column has a small state, so that sqrt replicates go negative (no extra
    variance there, nor at every fourth column: the latent state stays inside the links' domains except in the domain case)."""
    i = SHAPES.index((C, R)) * len(KS) + KS.index(K)
    rng = np.random.default_rng(7000 + 100 * i + (1 if domain else 0))
    S = C * R
    comp = np.zeros(K, dtype=np.int32)
    if K >= 2:
        comp[K // 2] = 2
    if K >= 3:
        comp[K // 2 + 1] = 2
    rot = [(1, 2, 0), (2, 0, 1), (0, 1, 2)][i % 3]
    link = np.array([1, 0, rot[2]] if domain else [rot[0], rot[1], rot[2]], dtype=np.int32)
    truth = 0.8 + 0.5 * np.sin(np.arange(K) / 6.0) + 0.3 * rng.random(K)
    truth[0::5] = 0.02 + 0.02 * rng.random(len(truth[0::5]))
    x = truth[None, :] * np.exp(0.05 * rng.standard_normal((S, K)))
    sig_pre = np.log(np.expm1(0.02 + 0.03 * rng.random((S, 3))))
    fixed = {0: 0.015} if i % 4 == 1 else None
    sigma_sq = sigma_sq_of(sig_pre, LB, fixed)
    weight = rng.choice([1.0, 2.0, 4.0], size=K)
    y = truth * np.exp(0.1 * rng.standard_normal(K))
    y[3::7] = np.nan
    if K >= 3:
        y[K // 2 + 1] = np.nan
        y[K // 2] = truth[K // 2]
    extra_var = None if (i % 2 == 1 or domain) else np.where((np.arange(K) % 4 == 0) | (np.arange(K) % 5 == 0), 0.0, 1e-3 * rng.random(K))
    n_excl = np.zeros(3, dtype=np.int64)
    if domain:
        x[DOMAIN_DRAWS[0], DOMAIN_COLUMN] = -0.5
        x[DOMAIN_DRAWS[1], DOMAIN_COLUMN] = 0.0
        n_excl[0] = len(DOMAIN_DRAWS)
    out = dict(x=x.reshape(C, R, K), comp=comp, sig_pre=sig_pre.reshape(C, R, 3), sigma_sq=sigma_sq.reshape(C, R, 3), link=link, weight=weight, y=y,
               extra_var=extra_var, chain_ids=np.array(CHAIN_IDS[:C], dtype=np.int64) if i % 3 == 0 else None, fixed=fixed, seed=SEED + i,
               n_excluded=n_excl)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def args_of(f):
    """The keyword arguments of ``ppc`` (and of MagiEngine.ppc) for fixture f."""
    return dict(comp=f["comp"], link=f["link"], weight=f["weight"], y=f["y"], extra_var=f["extra_var"], seed=f["seed"], chain_ids=f["chain_ids"])


@functools.lru_cache(maxsize=None)
def crafted_reference(C, R, K, domain=False, long=True, fault=None):
    f = crafted(C, R, K, domain)
    s2 = f["sigma_sq"] if fault != "fixed_ignored" else sigma_sq_of(f["sig_pre"], LB, f["fixed"], fault=fault)
    return ppc(f["x"], sigma_sq=s2, dtype=np.longdouble if long else np.float64, fault=fault, **args_of(f))


# ---- calibration data ----------------------------------------------------------------------------------------------------------------------

def calibration_data(misfit=False):
    """Data generated from the model itself (CALIBRATION): two components, identity and log links, truth on a smooth curve, the posterior
    draws scattered a twentieth of a noise sd around it; ``misfit`` adds misfit_sd noise sd of a sinusoid on the link's scale."""
    c = CALIBRATION
    rng = np.random.default_rng(c["data_seed"])
    n, S = c["n_per_component"], c["C"] * c["R"]
    K = 2 * n
    comp = np.repeat([0, 1], n).astype(np.int32)
    link = np.array([0, 1], dtype=np.int32)
    s2 = np.array([0.04, 0.01])
    weight = rng.choice([1.0, 2.0, 4.0], size=K)
    t = np.arange(K) % n
    truth = 1.5 + np.sin(t / 15.0) * 0.5
    sdk = np.sqrt(s2[comp] / weight)
    g = np.where(comp == 1, np.log(truth), truth)
    gy = g + sdk * rng.standard_normal(K)
    if misfit:
        gy = gy + c["misfit_sd"] * sdk * np.sin(2.0 * np.pi * t / c["period"])
    y = np.where(comp == 1, np.exp(gy), gy)
    gx = g[None, :] + 0.05 * sdk[None, :] * rng.standard_normal((S, K))
    x = np.where(comp[None, :] == 1, np.exp(gx), gx)
    sigma_sq = s2[None, :] * np.exp(0.05 * rng.standard_normal((S, 2)))
    return dict(x=x.reshape(c["C"], c["R"], K), comp=comp, sigma_sq=sigma_sq.reshape(c["C"], c["R"], 2), link=link, weight=weight, y=y,
                seed=c["noise_seed"])
