"""Drop-in for the Python surface of the reference's ``magi_v2.MAGI_v2`` (magi_v2.py:20-462).

Same constructor, methods, public attributes and results dictionary; the hot path -- kernel
matrices, log posterior + gradient, NUTS -- runs in libmagi_hip.so on an MI355X.  There is no
CPU implementation of that path in this package: without the library or a GPU the methods raise.

What differs from the reference, deliberately:
  * ``f_vec`` is a built-in drift name or a numpy-compatible callable (TensorFlow is not a dependency).  A
    callable that equals a compiled-in drift uses the hand-written kernels; any other one is traced with
    sympy and the kernels are compiled for it (drift.py, jit.py; D <= 8, P <= 8).  It may use ``t``: the time of grid
    point ``i`` is ``self.I[i]``, as in the reference.
  * hyper-parameters are fitted on the GPU (``magi_fit_hparams``: the reference's GP marginal
    likelihood + priors + Adam, magi_v2.py:538-691, restated -- TFP itself is not available, so this
    step is parity-unpinned); ``hparams=`` / ``hparam_iters=0`` bypass it.
  * ``predict`` takes keyword-only extras (n_chains, seed, ...); defaults reproduce the reference.
"""
from __future__ import annotations

import time
from typing import Callable, Optional, Sequence, Union

import numpy as np

from . import drift as _drift
from . import host
from .engine import DEFAULT_PROBS, DRIFT_SHAPES, MagiEngine, MagiGroup


def _fresh_seed() -> int:
    """A 64-bit seed from the operating system's entropy (predict's seed when none is given)."""
    return int(np.random.SeedSequence().generate_state(2, dtype=np.uint32).astype(np.uint64) @ np.array([1, 1 << 32], dtype=np.uint64))


def _warn_if_stuck(summary):
    """predict(summary=True): one warning when every X column is constant -- no post-burn-in transition moved (with the
    reference-faithful ``stale_cache=True`` a run can return ``num_results`` copies of one state).  Returns ``summary``."""
    if np.all(summary["X"]["sd"] == 0.0):
        import warnings
        warnings.warn("predict: every X column of the posterior sample is constant -- no post-burn-in transition was accepted; "
                      "rhat, ess and mcse_mean are NaN (try stale_cache=False, a smaller step_size or a longer burn-in)")
    return summary


def logarithmic_temperature_schedule(step, min_temp: float = 0.1):
    """magi_v2.py:833-835."""
    return np.maximum(1.0 / np.log(np.asarray(step, dtype=np.float64) + 2.0), min_temp)


def _band(A: np.ndarray, b: Optional[int]) -> np.ndarray:
    if b is None:
        return A
    n = A.shape[-1]
    i = np.arange(n)
    return A * (np.abs(i[:, None] - i[None, :]) <= b)


def _digest(a) -> bytes:
    """Full-content hash of a host matrix stack (an in-place edit anywhere is seen)."""
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.blake2b(a.view(np.uint8).reshape(-1).data, digest_size=16).digest() + repr(a.shape).encode()


class MAGI_v2:
    """MAnifold-constrained Gaussian-process Inference on an MI355X (interface of magi_v2.py:20-73)."""

    def __init__(self, D_thetas: int, ts_obs: np.ndarray, X_obs: np.ndarray, bandsize: Union[int, None],
                 f_vec: Union[str, Callable], device: int = 0):
        self.D_thetas = D_thetas
        self.BANDSIZE = bandsize
        self.ts_obs = ts_obs
        self.X_obs = X_obs
        self.N, self.D = self.X_obs.shape

        # observed vs completely unobserved components (magi_v2.py:45-50)
        self.observed_indicators = (~np.isnan(X_obs)).mean(axis=0) > 0
        self.observed_components = np.arange(self.D)[self.observed_indicators]
        self.D_observed = len(self.observed_components)
        self.unobserved_components = np.setdiff1d(np.arange(self.D), self.observed_components)
        self.D_unobserved = len(self.unobserved_components)
        self.proper_order = np.argsort(np.concatenate([self.observed_components, self.unobserved_components]))
        self.N_ds = (~np.isnan(self.X_obs)).sum(axis=0)                       # magi_v2.py:53

        self.I, self.X_obs_discret = None, None
        self.beta, self.mag_I = None, None
        self.not_nan_idxs, self.not_nan_cols = None, None
        self.y_tau_ds_observed = None
        self.X_interp_obs, self.X_interp_unobs = None, None

        self.phi1s = np.full((self.D,), np.nan)
        self.phi2s = np.full((self.D,), np.nan)
        self.sigma_sqs_init = np.full((self.D,), np.nan)
        self.Xhat_init, self.thetas_init = None, None
        self.mu_ds = np.full((self.D,), np.nan)
        # C_d_invs / m_ds / K_d_invs (magi_v2.py:117-119): the authoritative copies live on the GPU; the attributes are
        # properties that download on first read and upload again only if the caller assigned or edited them
        self._host_mats = [None, None, None]
        self._host_digests = [None, None, None]
        self._assigned = [False, False, False]
        self._dev_valid = False          # the handle's dense stacks hold the current matrices
        self._band_applied = False       # magi_v2.py:271-274 has run (host copies are masked; the device masks when packing)
        self._packed_for = None          # bandsize the device operands were last packed with

        self.f_vec = f_vec
        self.drift = _drift.resolve(f_vec, self.D, D_thetas)       # built-in, or traced + JIT-compiled (drift.py, jit.py)
        self._device = device
        self._engine: Optional[MagiEngine] = None

    # ------------------------------------------------------------------------------------------
    @property
    def engine(self) -> MagiEngine:
        if self._engine is None:
            self._engine = MagiEngine(self._device, drift=self.drift)      # raises without libmagi_hip.so / GPU
        return self._engine

    # -- matrices: device-resident, lazily mirrored on the host ----------------------------------------------------
    def _materialise(self):
        if self._dev_valid and any(m is None for m in self._host_mats):
            got = self.engine.get_dense(self.BANDSIZE if self._band_applied else None)
            for k in range(3):
                if self._host_mats[k] is None:
                    self._host_mats[k] = got[k]
                    self._host_digests[k] = _digest(got[k])

    def _get_mat(self, k):
        self._materialise()
        return self._host_mats[k]

    def _set_mat(self, k, value):
        self._host_mats[k] = value
        self._assigned[k] = value is not None
        self._host_digests[k] = None

    C_d_invs = property(lambda self: self._get_mat(0), lambda self, v: self._set_mat(0, v))
    m_ds = property(lambda self: self._get_mat(1), lambda self, v: self._set_mat(1, v))
    K_d_invs = property(lambda self: self._get_mat(2), lambda self, v: self._set_mat(2, v))

    def _host_overrides(self) -> bool:
        """True when the caller assigned one of the three attributes or edited a downloaded copy in place."""
        return any(self._assigned) or any(m is not None and d is not None and _digest(m) != d
                                          for m, d in zip(self._host_mats, self._host_digests))

    def _build(self, comps: Sequence[int], phi1s, phi2s):
        """Eqn. 6 matrices for the listed components on the GPU (magi_v2.py:122-128, 262-268, 447-451): built into the
        handle's dense stacks, no host copy."""
        self.engine.build_dense(self.I, self.D, list(comps), phi1s, phi2s, 2.01)
        self._dev_valid = True
        self._host_mats, self._host_digests, self._assigned = [None] * 3, [None] * 3, [False] * 3
        self._packed_for = None

    def _apply_band(self):
        """magi_v2.py:271-274 / 459-462: the device applies the mask when it packs; host copies that exist are masked here."""
        self._band_applied = True
        if self.BANDSIZE is not None:
            for k in range(3):
                if self._host_mats[k] is not None:
                    keep = self._assigned[k]
                    self._host_mats[k] = _band(np.asarray(self._host_mats[k]), self.BANDSIZE)
                    self._assigned[k] = keep
                    if not keep:
                        self._host_digests[k] = _digest(self._host_mats[k])
        self._packed_for = None

    def _sync_matrices(self):
        if self._host_overrides() or not self._dev_valid:
            self._materialise()                    # (the ones the caller did not touch)
            assert all(m is not None for m in self._host_mats), "C_d_invs, m_ds and K_d_invs must be set (run initial_fit first)."
            mats = [np.asarray(m, dtype=np.float64) for m in self._host_mats]
            self.engine.set_matrices(*mats, bandsize=self.BANDSIZE)
            self._dev_valid = True
            self._assigned = [False] * 3
            self._host_digests = [_digest(m) for m in self._host_mats]
            self._packed_for = ("band", self.BANDSIZE)
        elif self._packed_for != ("band", self.BANDSIZE):
            self.engine.pack_resident(self.BANDSIZE)
            self._packed_for = ("band", self.BANDSIZE)

    def _dense_apply(self, which: str, V, transpose=False):
        """A_d V[d] (or A_d^T V[d]) with the current dense matrices: on the GPU while they are device-resident, with the
        caller's arrays once those were overwritten."""
        if self._dev_valid and not self._host_overrides():
            return self.engine.dense_apply(which, V, transpose)
        A = np.asarray({"C_inv": self.C_d_invs, "m": self.m_ds, "K_inv": self.K_d_invs}[which])
        V = np.asarray(V, dtype=np.float64)
        sub = "dji" if transpose else "dij"
        return np.einsum(f"{sub},dj->di", A, V) if V.ndim == 2 else np.einsum(f"{sub},djp->dip", A, V)

    # ------------------------------------------------------------------------------------------
    def _fit_kernel_hparams(self, I, X_filled, verbose=False, num_iters: int = 1000):
        """magi_v2.py:538-691 on the GPU (magi_fit_hparams): Adam x num_iters on the GP marginal likelihood +
        the reference's Fourier-informed priors, starting from its initial values."""
        pri = [host.fourier_phi2_prior(X_filled[:, d]) for d in range(X_filled.shape[1])]
        init = host.hparams_initial(X_filled)
        if verbose:
            print(f"Fitting hparams for {X_filled.shape[1]} components on the GPU ({num_iters} Adam steps) ...")
        return self.engine.fit_hparams(I, X_filled, X_filled.mean(axis=0), [p[0] for p in pri], [p[1] for p in pri],
                                       init["sigma_sqs"], init["phi1s"], init["phi2s"], init["sigma_sqs"], num_iters=num_iters)

    def initial_fit(self, discretization: int, verbose=False, hparams: Optional[dict] = None,
                    theta_init_iters: int = 10000, hparam_iters: int = 1000, hparam_fit_on: str = "grid",
                    init_seed: int = 0):
        """magi_v2.py:82-277.  Hyper-parameters are fitted as in the reference (1000 Adam steps on the
        linearly interpolated discretisation grid, magi_v2.py:105-106) unless ``hparams`` carries phi1s /
        phi2s / sigma_sqs for the observed components, or ``hparam_iters=0`` keeps the reference's starting
        values.  ``hparam_fit_on="observed"`` is a documented deviation: it fits on the observation times only.
        The inserted grid points are exact linear interpolants, which a GP marginal likelihood can only explain
        with a short length scale and near-zero noise; on the vignette data that optimum (phi2 ~ 0.1,
        sigma ~ 0.002) ruins the parameter recovery, while the fit on the observed rows lands at the true noise level
        (theta ~ (3.9, 0.47, 1.66) against the truth (6, 0.6, 1.8); with phi2 = 0.5 and that noise level
        (5.9, 0.56, 1.76)) -- see DESIGN.md section 8 and examples/vignette_seir.py.  Components that are never
        observed are initialised as in magi_v2.py:182-268; ``init_seed`` seeds the reference's unseeded start."""
        self.I, self.X_obs_discret = host.discretize(self.ts_obs, self.X_obs, discretization)
        self.mag_I = self.I.shape[0]
        N_ds, self.beta, idx, y = host.observation_bookkeeping(self.X_obs, self.X_obs_discret)
        self.not_nan_idxs = idx
        self.not_nan_cols = idx % self.D
        self.y_tau_ds_observed = y

        self.X_interp_obs = host.linear_interpolate(self.X_obs_discret[:, self.observed_indicators])
        if hparams is not None:
            hp = dict(host.hparams_initial(self.X_interp_obs))
            hp.update({k: np.asarray(v, dtype=np.float64) for k, v in hparams.items()})
        elif hparam_iters > 0 and hparam_fit_on == "observed":
            X_rows = host.linear_interpolate(self.X_obs[:, self.observed_indicators])
            hp = self._fit_kernel_hparams(np.asarray(self.ts_obs, dtype=np.float64), X_rows, verbose=verbose, num_iters=hparam_iters)
        elif hparam_iters > 0:
            if hparam_fit_on != "grid":
                raise ValueError("hparam_fit_on must be 'grid' (reference) or 'observed'")
            hp = self._fit_kernel_hparams(self.I, self.X_interp_obs, verbose=verbose, num_iters=hparam_iters)
        else:
            hp = dict(host.hparams_initial(self.X_interp_obs))
        self.phi1s[self.observed_indicators] = hp["phi1s"]
        self.phi2s[self.observed_indicators] = hp["phi2s"]
        self.sigma_sqs_init[self.observed_indicators] = hp["sigma_sqs"]
        self.Xhat_init = self.X_obs_discret.copy()
        self.Xhat_init[:, self.observed_indicators] = self.X_interp_obs
        self.mu_ds[self.observed_indicators] = self.X_interp_obs.mean(axis=0)

        self._band_applied = False
        self._build(self.observed_components, hp["phi1s"], hp["phi2s"])        # (components not built yet are zero matrices, magi_v2.py:117-119)

        if np.all(self.observed_indicators):
            self.thetas_init = self._fit_thetas_init(theta_init_iters)
        else:
            # magi_v2.py:182-268: (X_unobs, theta) jointly by finite-difference gradient matching with the observed
            # components fixed at their smoothed values, then hyper-parameters + matrices of the unobserved components
            self.X_interp_unobs, self.thetas_init = self._fit_unobserved(theta_init_iters, init_seed)
            if hparams is not None and "phi1s_unobs" in hparams:
                hpu = {"phi1s": np.asarray(hparams["phi1s_unobs"], dtype=np.float64),
                       "phi2s": np.asarray(hparams["phi2s_unobs"], dtype=np.float64),
                       "sigma_sqs": np.asarray(hparams["sigma_sqs_unobs"], dtype=np.float64)}
            elif hparam_iters > 0:
                hpu = self._fit_kernel_hparams(self.I, self.X_interp_unobs, verbose=verbose, num_iters=hparam_iters)
            else:
                hpu = dict(host.hparams_initial(self.X_interp_unobs))
            self.phi1s[self.unobserved_components] = hpu["phi1s"]
            self.phi2s[self.unobserved_components] = hpu["phi2s"]
            self.sigma_sqs_init[self.unobserved_components] = hpu["sigma_sqs"]
            self.Xhat_init[:, self.unobserved_components] = self.X_interp_unobs
            self.mu_ds[self.unobserved_components] = self.X_interp_unobs.mean(axis=0)
            self.engine.build_dense(self.I, self.D, list(self.unobserved_components), hpu["phi1s"], hpu["phi2s"], 2.01)
            self._packed_for = None

        self._apply_band()
        self.Xhat_init = host.cubic_smoother(self.I, self.Xhat_init)

    def _fit_thetas_init(self, iters: int) -> np.ndarray:
        """magi_v2.py:133-179: Adam(lr=.01) from theta = 1 on the t2 term, *including* the
        reference's reshape (magi_v2.py:155-156 reinterprets the [N, D] drift as [D, N] instead of
        transposing it).  Drifts that are linear in theta make the objective the quadratic
        theta^T A theta - 2 b^T theta + c, and Adam iterates on (A, b) exactly; otherwise every step evaluates
        the traced drift and its theta-Jacobian."""
        P, D, n = self.D_thetas, self.D, self.mag_I
        f_np, jac_np = self.drift.f_np, self.drift.jac_np
        Xc = (self.Xhat_init - self.mu_ds).T                                     # [D, n]
        bvec = self._dense_apply("m", Xc)                                        # m_d x_c   (the N x N products run on the GPU)
        rng = np.random.default_rng(0)
        probe = rng.uniform(0.3, 2.0, size=P)
        cols = [f_np(self.I, self.Xhat_init, np.eye(P)[p]) for p in range(P)]
        linear = (np.abs(f_np(self.I, self.Xhat_init, np.zeros(P))).max() == 0.0 and
                  np.allclose(f_np(self.I, self.Xhat_init, probe), sum(probe[p] * cols[p] for p in range(P)), rtol=1e-12, atol=1e-14))
        if linear:
            F = np.stack([c.reshape(D, n) for c in cols], axis=-1)               # [D, n, P]   (the reshape quirk)
            KF = self._dense_apply("K_inv", F)
            KTF = self._dense_apply("K_inv", F, transpose=True)
            A = np.einsum("dip,diq->pq", F, KF)
            g0 = np.einsum("dip,di->p", KF + KTF, bvec)                          # gradient offset
            grad_fn = lambda th: (A + A.T) @ th - g0
        elif self._dev_valid and not self._host_overrides():
            # the general branch stays on the GPU: drift values, theta-Jacobian, (K^-1 + K^-T) r and the Adam update of every step in one
            # captured graph, the host waits once (csrc/thetainit.hip); 10 000 steps at N = 161: a fraction of a second
            if self.drift.time_dependent:
                self.engine.set_times(self.I)
            return self.engine.theta_init(self.drift, self.Xhat_init, self.mu_ds, iters)
        else:
            def grad_fn(th):
                fv = f_np(self.I, self.Xhat_init, th).reshape(D, n)              # the reshape quirk
                _, T = jac_np(self.Xhat_init, th, self.I)                        # [n, D, P]
                Tq = np.stack([T[:, :, p].reshape(D, n) for p in range(P)], axis=-1)   # same reshape as the drift
                r = fv - bvec
                g = self._dense_apply("K_inv", r) + self._dense_apply("K_inv", r, transpose=True)      # (K^-1 + K^-T) r on the GPU
                return np.einsum("dip,di->p", Tq, g)
        theta = np.ones(P)
        m = np.zeros(P); v = np.zeros(P)
        b1, b2, lr, eps = 0.9, 0.999, 0.01, 1e-7
        for t in range(1, iters + 1):
            grad = grad_fn(theta)
            m = b1 * m + (1 - b1) * grad
            v = b2 * v + (1 - b2) * grad * grad
            alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            theta = theta - alpha * m / (np.sqrt(v) + eps)
        return theta

    def gradient_matching_loss_and_grads(self, X_obs_smoothed, X_unobs, thetas):
        """Objective of magi_v2.py:196-216 and its gradients w.r.t. (X_unobs, thetas): the L2 mismatch between the
        drift and the centred finite differences of the state on the interior grid points."""
        I = self.I
        X_full = np.concatenate([X_obs_smoothed, X_unobs], axis=1)[:, self.proper_order]
        f = self.drift.f_np(I, X_full, thetas)
        h2 = 2.0 * (I[1, 0] - I[0, 0])
        r = f[1:-1] - (X_full[2:] - X_full[:-2]) / h2                            # [n-2, D]
        J, T = self.drift.jac_np(X_full[1:-1], thetas, I[1:-1])                  # [n-2, D, D], [n-2, D, P]
        gX = np.zeros_like(X_full)
        gX[1:-1] += 2.0 * np.einsum("nd,ndk->nk", r, J)
        gX[2:] -= 2.0 * r / h2
        gX[:-2] += 2.0 * r / h2
        gth = 2.0 * np.einsum("nd,ndp->p", r, T)
        return float((r ** 2).sum()), gX[:, self.unobserved_components], gth

    def _fit_unobserved(self, iters: int, seed: int):
        """magi_v2.py:182-247: Adam(lr=.01) x ``iters`` on (X_unobs, theta) jointly.  The reference draws the
        starting X_unobs from an unseeded numpy normal (magi_v2.py:223); here the generator is seeded."""
        Xs = host.cubic_smoother(self.I, self.X_interp_obs)
        mu0 = self.X_interp_obs.mean()
        sd0 = (self.X_interp_obs.std(axis=0) ** 2).mean() ** 0.5
        rng = np.random.Generator(np.random.PCG64(seed))
        Xu = rng.normal(loc=mu0, scale=sd0, size=(self.mag_I, self.D_unobserved))
        th = np.ones(self.D_thetas)
        mX, vX, mt, vt = np.zeros_like(Xu), np.zeros_like(Xu), np.zeros_like(th), np.zeros_like(th)
        b1, b2, lr, eps = 0.9, 0.999, 0.01, 1e-7
        for t in range(1, iters + 1):
            _, gX, gt = self.gradient_matching_loss_and_grads(Xs, Xu, th)
            alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            mX = b1 * mX + (1 - b1) * gX; vX = b2 * vX + (1 - b2) * gX * gX
            mt = b1 * mt + (1 - b1) * gt; vt = b2 * vt + (1 - b2) * gt * gt
            Xu = Xu - alpha * mX / (np.sqrt(vX) + eps)
            th = th - alpha * mt / (np.sqrt(vt) + eps)
        return Xu, th

    # ------------------------------------------------------------------------------------------
    def predict(self, num_results: int = 1000, num_burnin_steps: int = 1000, sigma_sqs_LB=None, verbose=False, *,
                n_chains: int = 1, seed: Optional[int] = None, chain_ids: Optional[Sequence[int]] = None,
                stale_cache: bool = True, anneal: bool = True, max_tree_depth: int = 10, step_size: float = 0.1,
                family_chains: Optional[int] = None, summary: bool = False, keep_samples: bool = True, adapt_metric: bool = False,
                theta_support=None, theta_prior=None, sigma_sq_prior=None, obs_link=None, obs_weight=None, elpd: bool = False, ppc: bool = False,
                rank_diagnostics: bool = False):
        """magi_v2.py:286-425.  Returns the reference's results dictionary; with n_chains > 1 every
        sample array gains a leading chain axis.  ``family_chains``: in a job sharded over GPUs, the largest per-GPU share
        (shard.family_chains_for) -- every rank then samples with the same kernel family whatever its own share.
        ``summary=True`` adds ``results["summary"]``: the posterior summaries and convergence diagnostics of all chains pooled, computed
        on the GPU from the device-resident samples (``posterior_summary``, which also takes other ``probs`` / ``max_lag``).  ``keep_samples=False`` (only with ``summary=True``) skips
        the download of the draws: ``X_samps``, ``sigma_sqs_samps``, ``thetas_samps`` and ``sample_results`` are then None.
        ``rank_diagnostics=True`` (with ``summary=True``): each block of the summary gains ``rhat_rank``, ``ess_bulk`` and ``ess_tail``, the
        rank-normalised diagnostics of ``posterior_summary(rank=True)``, and one warning names the columns beyond their thresholds.
        ``adapt_metric=True`` (the reference, like TFP's NoUTurnSampler, has the identity metric only): a per-chain diagonal mass matrix is
        adapted during the ``int(0.8 * num_burnin_steps)`` adaptation transitions over Stan's windows (``host.warmup_schedule``), dual
        averaging restarting after each window; ``results["metric"]`` = dict(inv_mass_X, inv_mass_sigma_pre, inv_mass_theta_pre: the
        metric the results were drawn with, leading chain axis as the samples; windows: per adapted window start, stop, the step sizes
        after it and the number of chains it left unchanged).
        ``theta_support`` (the reference constrains every ODE parameter to be positive, and None keeps that): one entry per parameter out
        of "positive", "real", ("lower", lo), ("upper", hi) -- theta = softplus(pre), pre, lo + softplus(pre), hi - softplus(pre).  The
        sampler works on ``pre`` as before; ``thetas_samps`` and ``summary["thetas"]`` are on the natural scale under the supports,
        ``sample_results[2]`` stays ``pre``, and ``results["theta_support"]`` echoes the normalised specification.
        ``theta_prior`` / ``sigma_sq_prior`` (the reference has a flat prior on every parameter and noise variance, and None keeps that):
        one entry per parameter / component out of None or "flat", ("normal", m, s), ("lognormal", m, s), ("gamma", k, r),
        ("invgamma", a, b) -- unnormalised densities on the natural scale (theta under its support, sigma^2), tempered with the posterior --
        and for a noise variance also ("fixed", c): that sigma^2 is the known constant c, ``sigma_sqs_samps`` and the summaries report c, and
        its ``pre`` coordinate (started at 0) is an independent standard normal.  lognormal, gamma and invgamma on a parameter need a support
        inside (0, inf).  ``results["theta_prior"]`` / ``results["sigma_sq_prior"]`` echo the normalised specifications when given.
        ``obs_link`` / ``obs_weight`` (the reference observes y = x + N(0, sigma^2_d), and None keeps that): ``obs_link`` is one of "identity",
        "log" (multiplicative error; data > 0), "sqrt" (counts; data >= 0) for all components or one per component -- Gaussian error on
        g(y), sigma^2 the variance on that scale; ``obs_weight`` is shaped like the observed data on the grid, [n_points, D], a known weight
        > 0 per observation (the mean of n replicates: n; entries at unobserved positions are ignored).  ``X_samps``, the summaries and
        ``posterior_trajectories`` stay on the natural scale.  For a linked component the default ``sigma_sqs_LB`` is (0.01 std(g(y_d)))^2 and
        the chain starts from a sigma^2 on the link's scale (host.link_sigma_defaults); an explicit ``sigma_sqs_LB`` is taken as given.
        ``Xhat_init`` outside a link's domain at an observed point raises ValueError.  ``results["obs_link"]`` / ``results["obs_weight"]`` echo
        the normalised specification when given.
        ``elpd=True`` adds ``results["elpd"]``: the pointwise log predictive density of the observations, WAIC and PSIS-LOO with the
        Pareto-khat diagnostic, computed on the GPU from the device-resident samples (``posterior_elpd``, on the scale of the data) -- what
        ``host.compare_elpd`` compares two models of the same data by.  Legal with ``keep_samples=False``.
        ``ppc=True`` adds ``results["ppc"]``: the posterior predictive check of the fitted observations -- replicated data, PIT values and
        discrepancy p-values, computed on the GPU from the device-resident samples (``posterior_predictive``, its noise seeded with this
        call's ``seed``).  Legal with ``keep_samples=False``.
        Many datasets on one GPU: ``predict_many``."""
        if not keep_samples and not (summary or elpd or ppc):
            raise ValueError("keep_samples=False needs summary=True, elpd=True or ppc=True: the call would return nothing of the posterior")
        if rank_diagnostics and not summary:
            raise ValueError("rank_diagnostics=True adds its keys to results['summary']: it needs summary=True")
        sigma_sqs_LB, sig_pre0, th_pre0 = self._predict_prepare(sigma_sqs_LB, family_chains, theta_support, theta_prior, sigma_sq_prior, obs_link, obs_weight)
        eng = self.engine
        if seed is None:                 # the reference calls sample_chain unseeded (magi_v2.py:389-395)
            seed = _fresh_seed()
        cfg = eng.default_cfg(num_results=num_results, num_burnin_steps=num_burnin_steps, stale_cache=int(stale_cache),
                              anneal=int(anneal), max_tree_depth=max_tree_depth, step_size=step_size)
        rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None], n_chains, axis=0)
        if verbose:
            print("Starting NUTS posterior sampling ...")
        start = time.time()
        eng.sampler_init(cfg, rep(self.Xhat_init), rep(sig_pre0), rep(th_pre0), seed=seed, chain_ids=chain_ids)
        if adapt_metric:
            n_adapt = int(0.8 * num_burnin_steps)
            _, _, windows = eng.sampler_warmup(host.warmup_schedule(num_burnin_steps, n_adapt))
            eng.sampler_run(num_results + num_burnin_steps - n_adapt)
        else:
            eng.sampler_run(num_results + num_burnin_steps)
        self._predicted = True
        self._predict_seed = seed
        X_samps, sig_pre, th_pre = eng.sampler_samples() if keep_samples else (None, None, None)
        end = time.time()
        minutes = np.round((end - start) / 60, 2)
        if verbose:
            print(f"Finished sampling in {minutes} minutes.")
        results = self._predict_results(X_samps, sig_pre, th_pre, eng.sampler_diag(), sigma_sqs_LB, seed, n_chains, num_burnin_steps, minutes)
        if adapt_metric:
            sq = (lambda a: a[0]) if n_chains == 1 else (lambda a: a)
            mX, ms, mt = eng.sampler_metric()
            results["metric"] = {"inv_mass_X": sq(mX), "inv_mass_sigma_pre": sq(ms), "inv_mass_theta_pre": sq(mt), "windows": windows}
        if summary:
            results["summary"] = _warn_if_stuck(self.posterior_summary(rank=rank_diagnostics))
            if rank_diagnostics:
                host.warn_rank_diagnostics(results["summary"], n_chains)
        if elpd:
            results["elpd"] = self.posterior_elpd()
        if ppc:
            results["ppc"] = self.posterior_predictive(seed=seed)
        return results

    def posterior_summary(self, probs=DEFAULT_PROBS, max_lag: int = 0, rank: bool = False, tail_prob: float = 0.05):
        """Posterior summaries and convergence diagnostics of the last ``predict``, all its chains pooled, computed on the GPU from the
        samples the sampler left there (MagiEngine.sampler_summary): dict(X, sigma_sqs, thetas, probs, n_nonfinite), where X [N, D],
        sigma_sqs [D] and thetas [P] each hold mean, sd (ddof = 1), quantiles [len(probs), ...], rhat (split), ess and mcse_mean.  What the
        reference's notebooks compute on the host as ``X_samps.mean(axis=0)`` and ``np.quantile(X_samps, [0.025, 0.975], axis=0)``.
        ``rank=True`` adds to each of the three blocks ``rhat_rank``, ``ess_bulk`` and ``ess_tail``: the rank-normalised split R-hat, bulk
        ESS and tail ESS (at ``tail_prob``) of Vehtari et al. (2021), what Stan, ``posterior`` and ArviZ print
        (MagiEngine.sampler_rank_diagnostics; include/magi_hip.h has the definitions).  Without it the dictionary is as before."""
        if not getattr(self, "_predicted", False):
            raise RuntimeError("posterior_summary summarises the samples of the last predict: run predict first")
        out = self.engine.sampler_summary(probs=probs, max_lag=max_lag)
        if rank:
            host.merge_rank_diagnostics(out, self.engine.sampler_rank_diagnostics(max_lag=max_lag, tail_prob=tail_prob))
        return out

    @staticmethod
    def _posterior_at_result(r, derivative, return_draws):
        """The dictionary ``posterior_at`` returns, from MagiEngine.sampler_gp_predict's."""
        out = {"t": r["t"], "X": r["X"], "cond_sd": np.sqrt(r["cond_var"]), "pred_sd": np.sqrt(r["X"]["sd"] ** 2 + r["cond_var"]),
               "probs": r["probs"], "n_nonfinite": r["n_nonfinite"]}
        if derivative:
            out.update(dX=r["dX"], dcond_sd=np.sqrt(r["dcond_var"]))
        if return_draws:
            out["X_draws"] = r["X_draws"]
            if derivative:
                out["dX_draws"] = r["dX_draws"]
        return out

    def posterior_at(self, t_new, probs=DEFAULT_PROBS, max_lag: int = 0, derivative: bool = True, return_draws: bool = False):
        """The inferred trajectory of the last ``predict`` at the times ``t_new`` [T], which need not be grid points: a smooth band between
        them, the state at a held-out measurement's time, the derivative x'(t) that MAGI matches to f(x, theta), a short extrapolation
        under the GP alone.  Under MAGI's model x_d(t*) given a draw's x_d(I) is Gaussian with mean mu_d + k_d(t*, I) C_d^-1 (x_d(I) - mu_d)
        and a variance that does not depend on the draw (include/magi_hip.h: magi_sampler_gp_predict); the call conditions every
        device-resident draw on the GPU, all chains pooled, and nothing but the results crosses to the host -- legal after
        ``keep_samples=False``.  It uses the model's current grid ``I`` and the ``phi1s`` / ``phi2s`` the resident matrices were built
        with; a user who overwrote ``C_d_invs`` gets their own matrix (as stored, neither symmetrised nor transposed), with phi as the
        model holds them in the cross blocks and the prior variances.
        Returns dict(t [T]; X: mean, sd, rhat, ess, mcse_mean [T, D] and quantiles [len(probs), T, D] of the CONDITIONAL MEANS over the
        draws; cond_sd [T, D], the sd of x(t*) about its conditional mean; pred_sd = sqrt(sd^2 + cond_sd^2), the predictive sd of x(t*);
        probs; n_nonfinite; with ``derivative`` dX and dcond_sd, the same for x'(t*); with ``return_draws`` X_draws (and dX_draws)
        [chains, draws, T, D], the conditional means per draw: a draw of x(t*) itself is X_draws + cond_sd * z, z ~ N(0, 1)).  Outside
        [min I, max I] the mean reverts to ``mu_ds`` and cond_sd to sqrt(phi1)."""
        if not getattr(self, "_predicted", False):
            raise RuntimeError("posterior_at conditions the samples of the last predict: run predict first")
        r = self.engine.sampler_gp_predict(self.I, self.phi1s, self.phi2s, t_new, nu=2.01, probs=probs, max_lag=max_lag, derivative=derivative,
                                           return_draws=return_draws)
        return self._posterior_at_result(r, derivative, return_draws)

    def posterior_predictive(self, t_new=None, y_new=None, probs=DEFAULT_PROBS, seed: Optional[int] = None, return_draws: bool = False):
        """Could the model have produced the data?  The posterior predictive check of the last ``predict``, all its chains pooled, computed
        on the GPU (include/magi_hip.h: magi_ppc).  Without ``t_new`` the fitted observations are checked against replicates
        drawn from the device-resident samples under the model's links, weights and fixed variances (MagiEngine.sampler_ppc): no draw
        crosses to the host, legal after ``keep_samples=False``.  Returns the dictionary of ``host.ppc_result``: ``obs_index`` [(grid
        point, component)], per observation ``mean``, ``sd``, ``quantiles`` [len(probs), n_obs] of the replicated data y_rep on the data's
        scale (the predictive band of the OBSERVATIONS, noise included) and ``pit`` (uniform under a calibrated model), ``pvalues`` {chi2,
        mean, maxabs, acf1: [D]}, the posterior predictive p-values of four discrepancies of the standardised residuals per component
        (near 0 or 1: the data are not like the replicates in that respect), ``pit_ks`` [D], ``n_T_excluded``, ``n_nonfinite``;
        ``return_draws`` adds ``y_rep`` [chains, draws, n_obs].
        ``t_new`` [T] (times that need not be grid points) gives the predictive band of observations THERE, and with ``y_new`` [T, D] (NaN:
        none) the PIT and p-values of held-out measurements: the draws are conditioned to ``t_new`` on the GPU (``posterior_at``'s
        conditional means and their variance) and checked with that variance added to the latent state (MagiEngine.ppc with extra_var =
        cond_var), links the model's, weight 1.  One column per (time, component), component-major; ``obs_index`` then holds (index into
        t_new, component).  This route moves the conditioned draws x_new through the host.
        ``seed``: the Philox seed of the replicates' noise, a stream of its own; None: the seed of the last ``predict``."""
        if not getattr(self, "_predicted", False):
            raise RuntimeError("posterior_predictive checks the samples of the last predict: run predict first")
        eng = self.engine
        seed = getattr(self, "_predict_seed", 0) if seed is None else seed
        if t_new is None:
            if y_new is not None:
                raise ValueError("y_new are held-out measurements at the times t_new: give t_new")
            return eng.sampler_ppc(seed=seed, probs=probs, return_draws=return_draws)
        return self._ppc_at(eng, t_new, y_new, probs, seed, return_draws)

    def _ppc_at(self, eng, t_new, y_new, probs, seed, return_draws):
        """posterior_predictive at new times: the conditioned draws of all chains and their cond_var into MagiEngine.ppc."""
        t_new = np.asarray(t_new, dtype=np.float64).reshape(-1)
        T, D = t_new.shape[0], self.D
        r = eng.sampler_gp_predict(self.I, self.phi1s, self.phi2s, t_new, nu=2.01, probs=(), derivative=False, return_draws=True)
        xd = r["X_draws"]                                                   # [chains, draws, T, D]
        x = np.ascontiguousarray(xd.transpose(0, 1, 3, 2)).reshape(xd.shape[0], xd.shape[1], D * T)
        y = None
        if y_new is not None:
            y = np.asarray(y_new, dtype=np.float64)
            if y.shape != (T, D):
                raise ValueError(f"y_new: expected shape {(T, D)}, got {y.shape}")
            y = np.ascontiguousarray(y.T).reshape(-1)
        out = eng.ppc(x, np.repeat(np.arange(D), T), eng.sampler_sigma_sq(), link=getattr(self, "_obs_link", None), y=y,
                      extra_var=np.ascontiguousarray(r["cond_var"].T).reshape(-1), seed=seed, chain_ids=eng._chain_ids, probs=probs,
                      return_draws=return_draws)
        out["obs_index"] = np.stack([np.tile(np.arange(T), D), np.repeat(np.arange(D), T)], axis=1)
        out["t"] = t_new
        return out

    def posterior_elpd(self, scale: str = "data", loglik: bool = False, loo: Optional[bool] = None):
        """Pointwise log predictive density, WAIC and PSIS-LOO of the last ``predict``, all its chains pooled, computed on the GPU from the
        samples the sampler left there (MagiEngine.sampler_elpd; definitions in include/magi_hip.h).  The likelihood of an observation is
        Gaussian on its link's scale; ``scale="data"`` (default) adds the constant log|g_d'(y)| per observation -- -log y under a log
        link, -log(2 sqrt(y)) under sqrt, 0 under the identity -- to lpd, elpd_waic and elpd_loo, so that models with different links
        compare on the scale of the data (a datum 0 under a sqrt link: ValueError); ``scale="link"`` adds nothing.  Returns the dictionary
        of ``host.elpd_result``: ``pointwise`` (lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat), ``obs_index`` [(grid point, component)],
        the totals elpd_waic, elpd_loo, p_waic, p_loo with ``se_<name>``, ``n_khat_bad`` (khat > 0.7), ``n_nonfinite``; ``loglik=True`` adds
        the log-likelihood [chains, draws, n_obs] (on the link's scale).  ``loo``: None computes PSIS-LOO whenever the device serves it -- up
        to 466033 pooled draws -- and past that warns and returns lpd and WAIC alone (``host.elpd_wants_loo``); False skips it; True insists
        (MagiHipError past the bound)."""
        if not getattr(self, "_predicted", False):
            raise RuntimeError("posterior_elpd works on the samples of the last predict: run predict first")
        if scale not in ("data", "link"):
            raise ValueError(f"scale: 'data' or 'link', got {scale!r}")
        eng = self.engine
        want = host.elpd_wants_loo(eng.n_chains * eng._cfg.num_results, loo)
        return self._elpd_on_scale(eng.sampler_elpd(loglik=loglik, loo=want), scale)

    def _elpd_on_scale(self, res, scale):
        """``res`` (MagiEngine.sampler_elpd: the link's scale) on ``scale``, under the links of the last ``_predict_prepare``."""
        if scale not in ("data", "link"):
            raise ValueError(f"scale: 'data' or 'link', got {scale!r}")
        shift = None
        if scale == "data":
            shift = host.elpd_jacobian(getattr(self, "_obs_link", None), np.asarray(self.X_obs_discret, dtype=np.float64), res["obs_index"])
        return host.elpd_result(res["pointwise"], res["obs_index"], res["n_nonfinite"], loglik=res.get("loglik"), shift=shift, scale=scale)

    def _predict_prepare(self, sigma_sqs_LB, family_chains=None, theta_support=None, theta_prior=None, sigma_sq_prior=None,
                         obs_link=None, obs_weight=None):
        """predict's set-up up to the sampler: matrices on the device, the problem, the parameters' supports, the priors and then the
        observation model set; returns (sigma_sqs_LB, sig_pre0, th_pre0)."""
        assert ~np.any(np.isnan(self.Xhat_init)), "Please make sure Xhat_init does not have NaNs."
        assert ~np.any(np.isnan(self.sigma_sqs_init)), "Please make sure sigma_sqs_init does not have NaNs."
        assert ~np.any(np.isnan(self.thetas_init)), "Please make sure thetas_init does not have NaNs."

        LB_given = sigma_sqs_LB is not None
        if sigma_sqs_LB is None:
            sigma_sqs_LB = host.sigma_sqs_lower_bound(self.Xhat_init)
        sigma_sqs_LB = np.asarray(sigma_sqs_LB, dtype=np.float64)
        sigma_sqs_start = np.asarray(self.sigma_sqs_init, dtype=np.float64)
        self._obs_link = self._obs_weight = None
        if obs_link is not None or obs_weight is not None:          # (checked before the engine is touched)
            Xg = np.asarray(self.X_obs_discret, dtype=np.float64)
            self._obs_link = host.obs_model_spec(obs_link, Xg.shape[1])
            self._obs_weight = host.obs_weight_grid(obs_weight, Xg)
            host.link_start_check(self._obs_link, Xg, self.Xhat_init)
            sigma_sqs_LB, sigma_sqs_start = host.link_sigma_defaults(self._obs_link, Xg, self.Xhat_init, self._obs_weight, sigma_sqs_LB,
                                                                     sigma_sqs_start, LB_given)
        eng = self.engine
        self._sync_matrices()
        if family_chains is not None:
            eng.set_option("family_chains", int(family_chains))
        if self.drift.time_dependent:          # (after the matrices, which fix N; an updated grid -- update_kernel_matrices -- is followed here)
            eng.set_times(self.I)
        eng.set_problem(self.mu_ds, self.N_ds.astype(np.float64), np.asarray(self.not_nan_idxs),
                        np.asarray(self.y_tau_ds_observed), float(self.beta), sigma_sqs_LB, self.drift)
        sig_pre0, th_pre0 = host.softplus_inverse_inits(sigma_sqs_start, np.asarray(self.thetas_init, dtype=np.float64), sigma_sqs_LB)
        self._theta_support = None                   # (set_problem has reset the engine's supports to all-positive)
        if theta_support is not None:
            self._theta_support = host.theta_support(theta_support, self.drift.P)
            eng.set_theta_support(theta_support)
            th_pre0 = host.theta_pre_inits(np.asarray(self.thetas_init, dtype=np.float64), *self._theta_support)
        self._theta_prior = self._sigma_sq_prior = None          # (set_problem has reset the engine's priors to flat)
        if theta_prior is not None or sigma_sq_prior is not None:
            if theta_prior is not None:
                self._theta_prior = host.prior_spec(theta_prior, self.drift.P, "theta", self._theta_support or host.theta_support(None, self.drift.P))
            if sigma_sq_prior is not None:
                self._sigma_sq_prior = host.prior_spec(sigma_sq_prior, len(sig_pre0), "sigma_sq")
                sig_pre0 = np.where(self._sigma_sq_prior[0] == host.PRIOR_FIXED, 0.0, sig_pre0)      # (a fixed variance: pre ~ N(0, 1), started at 0)
            eng.set_prior(sigma_sq_prior, theta_prior)
        if self._obs_link is not None:               # (set_problem has reset the engine's observation model to the reference's)
            w = None if self._obs_weight is None else self._obs_weight.reshape(-1)[np.asarray(self.not_nan_idxs)]
            eng.set_obs_model(None if obs_link is None else self._obs_link, w)
        return sigma_sqs_LB, sig_pre0, th_pre0

    def _predict_results(self, X_samps, sig_pre, th_pre, diag, sigma_sqs_LB, seed, n_chains, num_burnin_steps, minutes):
        """predict's results dictionary from the chains' samples [n_chains, results, ...] and diagnostics."""
        kept = X_samps is not None                   # (predict(keep_samples=False): no draw was downloaded)
        sig_prior, th_prior = getattr(self, "_sigma_sq_prior", None), getattr(self, "_theta_prior", None)
        sig_samps, th_samps = host.transform_samples(sig_pre, th_pre, sigma_sqs_LB, sig_prior) if kept else (None, None)
        support = getattr(self, "_theta_support", None)
        if kept and support is not None:
            th_samps = host.transform_thetas(th_pre, *support)
        sq = (lambda a: None if a is None else a[0]) if n_chains == 1 else (lambda a: a)
        B = num_burnin_steps
        kernel_results = {k: sq(getattr(diag, k)[:, B:]) for k in
                          ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence",
                           "reach_max_depth", "is_accepted", "target_log_prob", "energy", "beta_temp")}
        kernel_results["seed"] = seed
        extra = {} if support is None else {"theta_support": host.theta_support_spec(*support)}
        if th_prior is not None:
            extra["theta_prior"] = host.prior_spec_echo(*th_prior)
        if sig_prior is not None:
            extra["sigma_sq_prior"] = host.prior_spec_echo(*sig_prior)
        if getattr(self, "_obs_link", None) is not None:
            extra["obs_link"] = host.obs_model_spec_echo(self._obs_link)
            if self._obs_weight is not None:
                extra["obs_weight"] = self._obs_weight
        return {**extra, "phi1s": self.phi1s, "phi2s": self.phi2s,
                "Xhat_init": self.Xhat_init,
                "sigma_sqs_init": self.sigma_sqs_init,
                "thetas_init": self.thetas_init,
                "I": self.I,
                "X_samps": sq(X_samps),
                "sigma_sqs_samps": sq(sig_samps),
                "thetas_samps": sq(th_samps),
                "kernel_results": kernel_results,
                "sample_results": [sq(X_samps), sq(sig_pre), sq(th_pre)] if kept else None,
                "minutes_elapsed": minutes}

    # ------------------------------------------------------------------------------------------
    def posterior_trajectories(self, results, t_out=None, start_index: int = 0, substeps: int = 4, thin: int = 1, return_draws: bool = True,
                               method: str = "rk4", rtol: float = 1e-6, atol: float = 1e-9, h0: float = 0.0, max_steps: int = 100000):
        """The ODE solved on the GPU with every kept posterior draw (MagiEngine.ode_solve: classical RK4, ``substeps`` steps per output
        interval, the device's own drift code): draw k starts at ``results["X_samps"][..., k, start_index, :]`` with
        ``results["thetas_samps"][..., k, :]``; ``thin`` keeps every thin-th draw.  ``t_out``: the output times, default
        ``I[start_index:]``; any increasing grid whose first entry is ``I[start_index]`` will do, and one that runs past ``I[-1]``
        forecasts.  Returns dict(t [T], trajectories [draws, T, D] or None without ``return_draws``, mean [T, D], sd [T, D] (ddof = 1,
        over the draws whose trajectory stayed finite), status [draws] (0, or the index of the first non-finite output), n_failed).  With
        a leading chain axis in ``results`` (n_chains > 1) trajectories and status keep it; mean and sd are over all chains' draws.
        ``method="dopri5"`` or ``"ros23"`` (stiff systems) integrates with error control instead, to ``rtol`` and ``atol`` (``h0``,
        ``max_steps``: MagiEngine.ode_solve); the result then also has reason, n_accepted and n_rejected per draw, shaped like status."""
        if results.get("X_samps") is None or results.get("thetas_samps") is None:
            raise ValueError("posterior_trajectories needs the draws: predict with keep_samples=True")
        I = np.asarray(results["I"], dtype=np.float64).reshape(-1)
        X, th = np.asarray(results["X_samps"], dtype=np.float64), np.asarray(results["thetas_samps"], dtype=np.float64)
        X0 = X[..., ::thin, start_index, :]
        th = th[..., ::thin, :]
        kept = X0.shape[:-1]                                  # lead + (draws,)
        t = I[start_index:] if t_out is None else np.asarray(t_out, dtype=np.float64).reshape(-1)
        assert t[0] == I[start_index], "t_out must start at I[start_index]"
        adaptive = {} if method == "rk4" else dict(method=method, rtol=rtol, atol=atol, h0=h0, max_steps=max_steps)
        out = self.engine.ode_solve(X0.reshape(-1, self.D), th.reshape(-1, self.D_thetas), t, substeps=substeps, return_draws=return_draws,
                                    drift=self.drift, **adaptive)
        if out["n_failed"] > 0:
            import warnings
            why = ""
            if adaptive:
                counts = np.bincount(out["reason"], minlength=4)
                why = ": " + ", ".join(f"{int(counts[r])} {self.engine.ODE_REASONS[r]}" for r in (1, 2, 3) if counts[r])
            warnings.warn(f"posterior_trajectories: {out['n_failed']} of {out['status'].shape[0]} trajectories left the finite range "
                          f"(status > 0{why}); mean and sd are over the others")
        traj = out["trajectories"]
        res = {"t": t, "trajectories": None if traj is None else traj.reshape(kept + traj.shape[1:]), "mean": out["mean"], "sd": out["sd"],
               "status": out["status"].reshape(kept), "n_failed": out["n_failed"]}
        for key in ("reason", "n_accepted", "n_rejected") if adaptive else ():
            res[key] = out[key].reshape(kept)
        return res

    def posterior_sensitivities(self, t_out=None, start_index: int = 0, substeps: int = 4, thin: int = 1, wrt=("theta", "x0"),
                                relative: bool = False, fisher: bool = True, return_draws: bool = False):
        """Which parameters do the data determine, and through which states and times?  Forward sensitivities of the fitted ODE for every
        draw of the last ``predict`` (all chains pooled, every ``thin``-th), and the Fisher information of the fitted observations,
        computed on the GPU from the device-resident samples (MagiEngine.sampler_sensitivities; include/magi_hip.h has the scheme): legal
        after ``keep_samples=False``.  Draw k starts at its X at grid row ``start_index`` with its theta and is integrated with the RK4
        of ``posterior_trajectories``; the sensitivities are the exact derivatives of that discrete solution.  ``t_out``: default
        ``I[start_index:]``; the observations used are those at grid points whose time is exactly an entry of ``t_out``.  ``wrt``: "theta"
        and / or "x0", in that order of columns.  ``relative``: sensitivities to the log parameters.
        Returns dict(t [T], names [Q] (theta names, then x0 names), sens: dict(mean, sd [T, D, Q] over the draws whose trajectory stayed
        finite, plus draws [S, T, D, Q] with ``return_draws``), fim_mean [Q, Q] and report (``host.fisher_report`` with post_sd = the
        posterior sd of theta and of X[start_index] from ``posterior_summary``, divided by |posterior mean| under ``relative``) -- both None
        without ``fisher`` or when no observation is used -- status [S], n_failed, n_fim_excluded, n_obs_used)."""
        if not getattr(self, "_predicted", False):
            raise RuntimeError("posterior_sensitivities works from the samples of the last predict: run predict first")
        wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
        if not wrt or any(w not in ("theta", "x0") for w in wrt) or len(set(wrt)) != len(wrt):
            raise ValueError(f"wrt: some of ('theta', 'x0'), got {wrt}")
        P, D = self.D_thetas, self.D
        cols = ([p for p in range(P)] if "theta" in wrt else []) + ([P + d for d in range(D)] if "x0" in wrt else [])
        names = [f"theta[{p}]" for p in range(P)] + [f"x0[{d}]" for d in range(D)]
        I = np.asarray(self.I, dtype=np.float64).reshape(-1)
        t = I[start_index:] if t_out is None else np.asarray(t_out, dtype=np.float64).reshape(-1)
        assert t[0] == I[start_index], "t_out must start at I[start_index]"
        where = {float(v): j for j, v in enumerate(t)}
        grid_out = np.array([where.get(float(v), -1) for v in I], dtype=np.int32) if fisher else None
        r = self.engine.sampler_sensitivities(t, grid_out, start_index=start_index, thin=thin, substeps=substeps, wrt=cols, relative=relative,
                                              return_draws=return_draws)
        if r["n_failed"] > 0:
            import warnings
            warnings.warn(f"posterior_sensitivities: {r['n_failed']} of {r['status'].shape[0]} trajectories left the finite range (status > 0); "
                          "means, sds and the Fisher information are over the others")
        out = {"t": t, "names": [names[c] for c in cols], "sens": {"mean": r["sens_mean"], "sd": r["sens_sd"]}, "fim_mean": None, "report": None,
               "status": r["status"], "n_failed": r["n_failed"], "n_fim_excluded": r.get("n_fim_excluded", 0), "n_obs_used": r["n_obs_used"]}
        if return_draws:
            out["sens"]["draws"] = r["sens"]
        if fisher and r["n_obs_used"] > 0:
            summ = self.engine.sampler_summary(probs=())
            sd = np.concatenate([summ["thetas"]["sd"], summ["X"]["sd"][start_index]])
            if relative:                                     # the sd of log(parameter), to first order
                sd = sd / np.abs(np.concatenate([summ["thetas"]["mean"], summ["X"]["mean"][start_index]]))
            out["fim_mean"] = r["fim_mean"]
            out["report"] = host.fisher_report(r["fim_mean"], out["names"], post_sd=sd[cols])
        return out

    def update_kernel_matrices(self, I_new, phi1s_new, phi2s_new):
        """magi_v2.py:433-462: new grid + hyper-parameters -> rebuild every component's matrices."""
        self.I = np.asarray(I_new, dtype=np.float64).reshape(-1, 1)
        self.phi1s, self.phi2s = np.array(phi1s_new, dtype=np.float64), np.array(phi2s_new, dtype=np.float64)
        self.mag_I = self.I.shape[0]
        self.beta = (self.D * self.mag_I) / self.N_ds.sum()
        self._band_applied = False
        self._build(range(self.D), self.phi1s, self.phi2s)
        self._apply_band()

    # reference helper names kept for callers that reach into them
    def _discretize(self, ts_obs, X_obs, discretization):
        return host.discretize(ts_obs, X_obs, discretization)

    def _linear_interpolate(self, X_partial):
        return host.linear_interpolate(X_partial)

    def cv_cubic_smoother(self, I, X_filled):
        return host.cubic_smoother(I, X_filled)


# ------------------------------------------------------------------------------------------
# many datasets on one GPU
# ------------------------------------------------------------------------------------------
def group_key(model, n_chains: int):
    """What decides whether ``model`` (its problem set: MAGI_v2._predict_prepare) can share a problem group (include/magi_hip.h:
    magi_group_create) with another: its engine's library and device and the problem's shape -- grid points, components, parameters,
    drift, band.  None when it cannot join any group: its own rule would stream ``n_chains`` chains on a matrix-core kernel."""
    eng = model.engine
    if not eng.stream_kernel_name(n_chains).startswith("k_stream<"):
        return None
    return (id(eng._lib), eng.device, model.mag_I, model.D, model.D_thetas, getattr(model.drift, "name", str(model.drift)), model.BANDSIZE)


def partition_for_groups(keys):
    """Index lists, in the order of first appearance: the models of one key (not None) together, every other model alone.  A key met once
    is alone too (a group of one gains nothing over the model's own predict)."""
    by_key, order = {}, []
    for k, key in enumerate(keys):
        if key is None:
            order.append([k])
        elif key in by_key:
            by_key[key].append(k)
        else:
            by_key[key] = [k]
            order.append(by_key[key])
    return [g for grp in order for g in ([grp] if len(grp) > 1 else [[i] for i in grp])]


def predict_many(models: Sequence[MAGI_v2], num_results: int = 1000, num_burnin_steps: int = 1000, sigma_sqs_LB=None, verbose=False, *,
                 n_chains: int = 1, seed: Optional[int] = None, chain_ids: Optional[Sequence[Sequence[int]]] = None,
                 stale_cache: bool = True, anneal: bool = True, max_tree_depth: int = 10, step_size: float = 0.1,
                 summary: bool = False, keep_samples: bool = True, theta_support=None, theta_prior=None, sigma_sq_prior=None,
                 obs_link=None, obs_weight=None, elpd: bool = False, posterior_at=None, ppc: bool = False, rank_diagnostics: bool = False):
    """``predict`` for several models (after their ``initial_fit``) at once.  Models of one library, device and problem shape are sampled
    as one problem group on their GPU -- one captured graph, one kernel pair per leapfrog slot for all their chains -- and the others by
    their own ``predict``.  ``sigma_sqs_LB``: None (each model's default) or one entry per model; ``chain_ids``: None (0 .. n_chains - 1
    for every model, as predict) or one id list per model.  Returns one results dictionary per model, in order: element k equals
    ``models[k].predict(<same arguments>, seed=<the seed used>)`` array for array, bit for bit; ``minutes_elapsed`` is the group's.
    ``summary`` / ``keep_samples`` as in ``predict``: a grouped model's summary pools that model's chains alone.  ``theta_support``: None, one
    specification for all models (entries "positive", "real", ("lower", lo), ("upper", hi), as in ``predict``) or one per model (each None
    or such a specification); the members of one group may differ.  ``theta_prior`` / ``sigma_sq_prior``: likewise None, one specification
    for all models (entries None, "flat", ("normal", m, s), ... as in ``predict``) or one per model.  ``obs_link`` / ``obs_weight``: likewise
    None, one specification for all models (a link name, or one name per component; one weight array) or one per model (a list of such
    specifications / of arrays or None); the members of one group may differ.  ``elpd`` as in ``predict``: one ``results["elpd"]`` per
    model, a grouped model's from its own chains and observation model.  ``posterior_at``: None, or times t_new [T]: adds
    ``results["posterior_at"]`` = that model's ``MAGI_v2.posterior_at(t_new)`` (a grouped model's through the group's handle and its
    member index, from its own chains, matrices and mu); legal with ``keep_samples=False``.  ``ppc`` as in ``predict``: one
    ``results["ppc"]`` per model, a grouped model's from its own chain range and observation model.  ``rank_diagnostics`` as in ``predict``
    (with ``summary=True``): a grouped model's from its own chains."""
    if not keep_samples and not (summary or elpd or ppc or posterior_at is not None):
        raise ValueError("keep_samples=False needs summary=True, elpd=True, ppc=True or posterior_at: the call would return nothing of the posterior")
    if rank_diagnostics and not summary:
        raise ValueError("rank_diagnostics=True adds its keys to results['summary']: it needs summary=True")
    models = list(models)
    n = len(models)
    lbs = [None] * n if sigma_sqs_LB is None else list(sigma_sqs_LB)
    ids = [None] * n if chain_ids is None else [None if c is None else list(c) for c in chain_ids]
    is_entry = lambda e: isinstance(e, str) or (isinstance(e, (tuple, list)) and len(e) == 2 and e[0] in ("lower", "upper"))
    if theta_support is None:
        sups = [None] * n
    elif len(theta_support) > 0 and all(is_entry(e) for e in theta_support):       # one specification for all
        sups = [list(theta_support)] * n
    else:
        sups = list(theta_support)
    def per_model(spec):
        # one prior specification for all models: every entry is None, "flat" or a (name, numbers...) tuple; else one per model
        is_prior = lambda e: e is None or (isinstance(e, str) and e == "flat") or (
            isinstance(e, (tuple, list)) and len(e) >= 2 and e[0] in ("normal", "lognormal", "gamma", "invgamma", "fixed"))
        if spec is None:
            return [None] * n
        if len(spec) > 0 and all(is_prior(e) for e in spec) and not all(e is None for e in spec):
            return [list(spec)] * n
        return list(spec)
    tpri, spri = per_model(theta_prior), per_model(sigma_sq_prior)
    # one link specification for all models: a name, or a sequence of names / None / codes; one per model: a list whose entries are such specifications
    one_link = lambda e: e is None or isinstance(e, (str, int, np.integer))
    if obs_link is None or isinstance(obs_link, str) or (len(obs_link) > 0 and all(one_link(e) for e in obs_link) and not all(e is None for e in obs_link)):
        olnk = [obs_link] * n
    else:
        olnk = list(obs_link)
    owts = [obs_weight] * n if obs_weight is None or isinstance(obs_weight, np.ndarray) else list(obs_weight)      # (one array for all, or a list with one array or None per model)
    if len(lbs) != n or len(ids) != n or len(sups) != n or len(tpri) != n or len(spri) != n or len(olnk) != n or len(owts) != n:
        raise ValueError("sigma_sqs_LB, chain_ids and per-model theta_support, theta_prior, sigma_sq_prior, obs_link and obs_weight take one entry per model")
    if seed is None:
        seed = _fresh_seed()
    kw = dict(n_chains=n_chains, seed=seed, stale_cache=stale_cache, anneal=anneal, max_tree_depth=max_tree_depth, step_size=step_size)
    prep = [m._predict_prepare(lb, None, sp, tp, sq, ol, ow) for m, lb, sp, tp, sq, ol, ow in zip(models, lbs, sups, tpri, spri, olnk, owts)]
    out = [None] * n
    for grp in partition_for_groups([group_key(m, n_chains) for m in models]):
        if len(grp) == 1:
            k = grp[0]
            only_at = not (keep_samples or summary or elpd or ppc)          # (predict wants a reason of its own to drop the draws)
            out[k] = models[k].predict(num_results, num_burnin_steps, lbs[k], verbose, chain_ids=ids[k], summary=summary or only_at, keep_samples=keep_samples,
                                        theta_support=sups[k], theta_prior=tpri[k], sigma_sq_prior=spri[k], obs_link=olnk[k], obs_weight=owts[k], elpd=elpd, ppc=ppc,
                                        rank_diagnostics=rank_diagnostics, **kw)
            if only_at:
                del out[k]["summary"]
            if posterior_at is not None:
                out[k]["posterior_at"] = models[k].posterior_at(posterior_at)
            continue
        g = MagiGroup([models[k].engine for k in grp])
        try:
            cfg = g.default_cfg(num_results=num_results, num_burnin_steps=num_burnin_steps, stale_cache=int(stale_cache),
                                anneal=int(anneal), max_tree_depth=max_tree_depth, step_size=step_size)
            rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[None], n_chains, axis=0)
            X0 = np.concatenate([rep(models[k].Xhat_init) for k in grp])
            s0 = np.concatenate([rep(prep[k][1]) for k in grp])
            t0 = np.concatenate([rep(prep[k][2]) for k in grp])
            gids = np.concatenate([np.arange(n_chains) if ids[k] is None else np.asarray(ids[k]) for k in grp]).astype(np.int64)
            if verbose:
                print(f"Starting NUTS posterior sampling of {len(grp)} models as one group ...")
            start = time.time()
            g.sampler_init(cfg, X0, s0, t0, seed=seed, chain_ids=gids)
            g.sampler_run(num_results + num_burnin_steps)
            X_samps, sig_pre, th_pre = g.sampler_samples() if keep_samples else (None, None, None)
            minutes = np.round((time.time() - start) / 60, 2)
            if verbose:
                print(f"Finished sampling in {minutes} minutes.")
            diag = g.sampler_diag()
            summaries = [g.sampler_summary(member=j) for j in range(len(grp))] if summary else None
            if rank_diagnostics:
                for j in range(len(grp)):
                    host.merge_rank_diagnostics(summaries[j], g.sampler_rank_diagnostics(member=j))
            elpds = [g.sampler_elpd(member=j, loo=host.elpd_wants_loo(n_chains * num_results))
                     for j in range(len(grp))] if elpd else None
            ppcs = [g.sampler_ppc(member=j, seed=seed) for j in range(len(grp))] if ppc else None
            ats = [g.sampler_gp_predict(models[k].I, models[k].phi1s, models[k].phi2s, posterior_at, member=j)
                   for j, k in enumerate(grp)] if posterior_at is not None else None
        finally:
            g.close()
        for j, k in enumerate(grp):
            sl = slice(j * n_chains, (j + 1) * n_chains)
            dk = type(diag)(*[getattr(diag, f)[sl] for f in diag.__dataclass_fields__])
            part = (X_samps[sl], sig_pre[sl], th_pre[sl]) if keep_samples else (None, None, None)
            out[k] = models[k]._predict_results(*part, dk, prep[k][0], seed, n_chains, num_burnin_steps, minutes)
            if summary:
                out[k]["summary"] = _warn_if_stuck(summaries[j])
                if rank_diagnostics:
                    host.warn_rank_diagnostics(summaries[j], n_chains)
            if elpd:
                out[k]["elpd"] = models[k]._elpd_on_scale(elpds[j], "data")
            if ppc:
                out[k]["ppc"] = ppcs[j]
            if posterior_at is not None:
                out[k]["posterior_at"] = MAGI_v2._posterior_at_result(ats[j], True, False)
    return out
