"""ctypes binding of libmagi_hip.so (include/magi_hip.h) -- the only compute path of the package.

There is deliberately no CPU fallback: if the shared library or a GPU is missing every entry point
raises.  numpy arrays in, numpy arrays out; layouts follow the reference ([N, D] trajectories).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .host import ELPD_POINTWISE, elpd_result, obs_model_spec, ppc_result, prior_spec, theta_support

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmagi_hip.so")

DRIFT_IDS = {"seir3": 0, "seir4": 1, "sirw": 2}
DRIFT_SHAPES = {"seir3": (3, 3), "seir4": (4, 3), "sirw": (4, 5)}   # name -> (D, P)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


class MagiHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmagi_hip error {code}: {msg}")
        self.code = code


class SamplerCfg(C.Structure):
    """Mirror of ``magi_sampler_cfg``; defaults = the reference's (magi_v2.py:357-366)."""
    _fields_ = [("num_results", C.c_int32), ("num_burnin_steps", C.c_int32), ("num_adaptation_steps", C.c_int32),
                ("max_tree_depth", C.c_int32), ("mode", C.c_int32), ("hmc_leapfrogs", C.c_int32),
                ("anneal", C.c_int32), ("stale_cache", C.c_int32), ("step_size", C.c_double),
                ("target_accept_prob", C.c_double), ("max_energy_diff", C.c_double), ("min_temp", C.c_double)]


_SYMBOLS = {
    "magi_create": (C.c_void_p, [C.c_int]),
    "magi_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "magi_destroy": (None, [C.c_void_p]),
    "magi_last_error": (C.c_char_p, [C.c_void_p]),
    "magi_version": (C.c_char_p, []),
    "magi_user_drift_info": (C.c_int, [_ip, _ip]),
    "magi_user_drift_time_dependent": (C.c_int, []),
    "magi_build_matrices": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp]),
    "magi_matern_blocks": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp]),
    "magi_fit_hparams": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_double,
                                   C.c_double, _dp, _dp, _dp, _dp]),
    "magi_set_matrices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]),
    "magi_theta_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double, _dp, _dp]),
    "magi_build_dense": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, C.c_double]),
    "magi_pack_resident": (C.c_int, [C.c_void_p, C.c_int]),
    "magi_get_dense": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "magi_dense_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "magi_set_problem": (C.c_int, [C.c_void_p, _dp, _dp, _lp, _dp, C.c_int64, C.c_double, _dp, C.c_int, C.c_int]),
    "magi_set_times": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "magi_set_theta_support": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp]),
    "magi_get_theta_support": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp]),
    "magi_set_prior": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp]),
    "magi_get_prior": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp]),
    "magi_set_obs_model": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int64, _dp]),
    "magi_get_obs_model": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int64, _dp]),
    "magi_logpost_grad": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp]),
    "magi_logpost_grad_fused": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp]),
    "magi_sampler_cfg_default": (None, [C.POINTER(SamplerCfg)]),
    "magi_sampler_init": (C.c_int, [C.c_void_p, C.POINTER(SamplerCfg), C.c_int, _dp, _dp, _dp, C.c_uint64, _lp]),
    "magi_sampler_run": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp]),
    "magi_sampler_steps_done": (C.c_int, [C.c_void_p, _lp]),
    "magi_sampler_get_samples": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "magi_sampler_get_diag": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _dp, _dp, _dp]),
    "magi_sampler_get_state": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "magi_sample": (C.c_int, [C.c_void_p, C.POINTER(SamplerCfg), C.c_int, _dp, _dp, _dp, C.c_uint64, _lp, _dp, _dp, _dp]),
    "magi_sampler_get_checkpoint": (C.c_int, [C.c_void_p, _dp]),
    "magi_sampler_set_checkpoint": (C.c_int, [C.c_void_p, _dp]),
    "magi_sampler_set_metric": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "magi_sampler_get_metric": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "magi_sampler_metric_window": (C.c_int, [C.c_void_p, C.c_int]),
    "magi_sampler_adapt_metric": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, _dp]),
    "magi_sampler_run_stats": (C.c_int, [C.c_void_p, _lp, _lp]),
    "magi_sampler_profile": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _lp]),
    "magi_time_gradient": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "magi_gradient_bytes": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "magi_tile_formats": (C.c_int, [C.c_void_p, C.c_int, _lp, _lp, _dp]),
    "magi_stream_carriers": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "magi_stream_carrier_tasks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "magi_stream_kernel_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    "magi_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "magi_debug_par": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "magi_build_profile": (C.c_int, [C.c_void_p, _dp, _dp, _lp]),
    "magi_drift_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "magi_drift_probe_at": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "magi_ode_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _ip, _ip]),
    "magi_ode_solve_adaptive": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_double,
                                          C.c_int, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip]),
    "magi_ode_sensitivities": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, _ip, C.c_int, C.c_int, _ip, _ip, _dp, _dp,
                                         _ip, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]),
    "magi_sampler_sensitivities": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip, C.c_int, _ip, C.c_int,
                                             _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _dp, _dp, _dp]),
    "magi_summarize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int] + [_dp] * 6 + [_ip]),
    "magi_sampler_summarize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int] + [_dp] * 18 + [_ip]),
    "magi_rank_diagnostics": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double] + [_dp] * 6 + [_ip]),
    "magi_sampler_rank_diagnostics": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double] + [_dp] * 9 + [_ip]),
    "magi_matern_cross": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp]),
    "magi_gp_predict": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, _dp, C.c_double, _dp, C.c_int, _dp, C.c_int, _dp] + [_dp] * 4),
    "magi_sampler_gp_predict": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, _dp, C.c_int, _dp, C.c_int]
                                + [_dp] * 16 + [_ip]),
    "magi_gp_profile": (C.c_int, [C.c_void_p, _dp]),
    "magi_elpd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp] + [_dp] * 6 + [_ip]),
    "magi_sampler_elpd": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [_dp] * 6 + [_ip, _ip, _dp, _ip]),
    "magi_ppc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _dp, _ip, _dp, _dp, _dp, C.c_uint64, _lp, C.c_int, _dp]
                 + [_dp] * 8 + [_ip, _ip]),
    "magi_sampler_ppc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, _dp] + [_dp] * 8 + [_ip, _ip, _ip, _ip, _dp]),
}

SUMMARY_STATS = ("mean", "sd", "quantiles", "rhat", "ess", "mcse_mean")       # the order of the six outputs in include/magi_hip.h
DEFAULT_PROBS = (0.025, 0.5, 0.975)
RANK_STATS = ("rhat_rank", "ess_bulk", "ess_tail")       # the order of the three outputs of magi_rank_diagnostics, and of its optional series
RANK_SERIES = ("rank", "z", "z_folded")


def _summary_arrays(shape, n_q):
    """The six output arrays of one block of columns of shape ``shape`` (quantiles: [n_q] + shape)."""
    return [np.empty((n_q,) + tuple(shape)) if s == "quantiles" else np.empty(shape) for s in SUMMARY_STATS]

_libs = {}


def load_library(path: Optional[str] = None):
    """dlopen libmagi_hip.so (or a drift-specialised build of it, magi_v2_amd.jit) and declare every symbol of
    include/magi_hip.h.  Raises if absent."""
    p = os.path.abspath(path or os.environ.get("MAGI_HIP_LIB") or LIB_PATH)      # MAGI_HIP_LIB: A/B builds in one session
    if p in _libs:
        return _libs[p]
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `python -m magi_v2_amd.build` (hipcc, gfx950); "
                          "magi_v2_amd has no CPU fallback")
    lib = C.CDLL(p)
    for name, (res, args) in _SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _libs[p] = lib
    return lib


def exported_symbols():
    return sorted(_SYMBOLS)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


@dataclass
class SamplerDiag:
    step_size: np.ndarray
    log_accept_ratio: np.ndarray
    leapfrogs_taken: np.ndarray
    tree_depth: np.ndarray
    has_divergence: np.ndarray
    reach_max_depth: np.ndarray
    is_accepted: np.ndarray
    target_log_prob: np.ndarray
    energy: np.ndarray
    beta_temp: np.ndarray


class MagiEngine:
    """One handle = one GPU.  Not thread-safe; different engines may be used from different threads."""

    def __init__(self, device_id: int = 0, drift=None, _library: Optional[str] = None):
        """``drift``: a magi_v2_amd.drift.Drift traced from a user f_vec -> the engine runs the library that
        magi_v2_amd.jit compiles for it; None / a built-in -> the base library.  A drift-specialised library passes its self-test
        (magi_v2_amd.selftest: verdict cached beside the file) before its first handle exists; a library that fails raises
        MagiSelfTestError and is not used.  (``_library``: the self-test's own handles, on the file under test.)"""
        self.user_drift = None
        user = drift is not None and not getattr(drift, "is_builtin", True)
        if _library is not None:
            self._lib = load_library(_library)
        elif user:
            from . import jit, selftest
            path = jit.library_for(drift)
            selftest.ensure(path, drift, int(device_id))
            self._lib = load_library(path)
        else:
            self._lib = load_library()
        if user:
            self.user_drift = drift
            if bool(self._lib.magi_user_drift_time_dependent()) != bool(getattr(drift, "time_dependent", False)):
                raise ValueError(f"library {self._lib._name} was built for a drift that "
                                 f"{'uses' if self._lib.magi_user_drift_time_dependent() else 'does not use'} t; drift '{drift.name}' "
                                 f"{'does' if drift.time_dependent else 'does not'}")
        self._h = self._lib.magi_create(int(device_id))
        if not self._h:
            raise MagiHipError(-2, self._lib.magi_last_error(None).decode())
        self.device = int(device_id)
        self.N = self.D = self.P = None
        self.n_chains = 0
        self._cfg = None
        self._problem_drift = None
        self._n_obs = 0

    # -- plumbing -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.magi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise MagiHipError(rc, self._lib.magi_last_error(self._h).decode())

    @staticmethod
    def version():
        return load_library().magi_version().decode()

    _FAMILIES = {"auto": 0, "mc": 1, "valu": 2}

    def set_option(self, name, value):
        """Tuning / test switch of this handle (include/magi_hip.h: magi_set_option); stream_family also takes "auto" / "mc" / "valu"."""
        if name == "stream_family" and isinstance(value, str):
            value = self._FAMILIES[value]
        self._check(self._lib.magi_set_option(self._h, name.encode(), int(value)))

    def drift_probe(self, drift, X, th, g=None, path=0, t=None):
        """This library's drift code by itself at the points X[n, D] (magi_drift_probe): (f[n, D], c[n, D], t[n, P]) with c_k = sum_d g_d
        df_d/dx_k and t_p = sum_d g_d df_d/dtheta_p through path 0 (DriftT::f / jt) or 1 (the runtime-switch entries); (f, None, None)
        through path 2 (the separable members; MagiHipError when the drift has none) or 3 (DriftT::f1).  ``th``: the parameters as the
        drift sees them.  ``drift``: built-in name, or the Drift this engine was created for.  ``t``: the time of every point, [n]
        (magi_drift_probe_at); None: all at time 0."""
        if isinstance(drift, str):
            (D, P), drift_id = DRIFT_SHAPES[drift], DRIFT_IDS[drift]
        else:
            D, P, drift_id = drift.D, drift.P, drift.device_id
        X = _f64(X)
        n = X.shape[0]
        X, th = _f64(X, (n, D)), _f64(th, (P,))
        deriv = int(path) in (0, 1)
        g = _f64(np.zeros((n, D)) if g is None else g, (n, D)) if deriv else None
        f = np.empty((n, D))
        c, tt = (np.empty((n, D)), np.empty((n, P))) if deriv else (None, None)
        if t is None:
            self._check(self._lib.magi_drift_probe(self._h, drift_id, P, int(path), n, _ptr(X), _ptr(th), _ptr(g), _ptr(f), _ptr(c), _ptr(tt)))
        else:
            times = _f64(np.asarray(t, dtype=np.float64).reshape(-1), (n,))
            self._check(self._lib.magi_drift_probe_at(self._h, drift_id, P, int(path), n, _ptr(X), _ptr(th), _ptr(g), _ptr(f), _ptr(c), _ptr(tt), _ptr(times)))
        return f, c, tt

    ODE_METHODS = {"rk4": 0, "dopri5": 1, "ros23": 2}          # (1, 2: MAGI_ODE_DOPRI5, MAGI_ODE_ROS23 of include/magi_hip.h)
    ODE_REASONS = ("none", "non-finite state", "step budget", "step underflow")

    def ode_solve(self, x0, theta, t_out, substeps=4, return_draws=True, drift=None, method="rk4", rtol=1e-6, atol=1e-9, h0=0.0, max_steps=100000):
        """This library's drift integrated on the device for S draws at once (magi_ode_solve): draw s starts at x0[s] ([S, D]) with the
        parameters theta[s] ([S, P], natural scale) and is reported at the increasing times t_out[T] (output 0 is x0).  Classical RK4,
        ``substeps`` steps per output interval: the scheme of drift_examples.rk4.  Returns dict(trajectories [S, T, D] or None without
        ``return_draws``, mean [T, D], sd [T, D] (ddof = 1) over the draws with status 0, status [S] (0, or the index of the first
        non-finite output; 1 for a non-finite x0), n_failed).  ``drift``: built-in name or Drift; None: the Drift this engine was created for, else the drift
        of the last set_problem.
        ``method``: "rk4" (the above; the arguments behind it are not used), or an error-controlled integrator (magi_ode_solve_adaptive,
        the controller is stated in include/magi_hip.h): "dopri5", Dormand-Prince 5(4), or "ros23", the Rosenbrock 2(3) pair of ode23s for
        stiff systems, with relative and absolute tolerances ``rtol``, ``atol``, first step ``h0`` (0: the first output interval) and at
        most ``max_steps`` accepted + rejected steps per draw (``substeps`` is not used).  The result then also holds reason [S]
        (index into ODE_REASONS: a draw that ran out of steps or whose step underflowed has status j + 1 of the interval it did not
        complete and NaN from there on), n_accepted [S] and n_rejected [S]."""
        if method not in self.ODE_METHODS:
            raise ValueError(f"unknown method {method!r}; one of {sorted(self.ODE_METHODS)}")
        if drift is None:
            drift = self.user_drift if self.user_drift is not None else getattr(self, "_problem_drift", None)
            if drift is None:
                raise ValueError("ode_solve on the base library needs drift= (a built-in name) or a problem set before")
        if isinstance(drift, str):
            D, drift_id = DRIFT_SHAPES[drift][0], DRIFT_IDS[drift]
        else:
            D, drift_id = drift.D, drift.device_id
        x0, theta = _f64(x0), _f64(theta)
        S = x0.shape[0]
        x0 = _f64(x0, (S, D))
        if theta.ndim != 2 or theta.shape[0] != S:
            raise ValueError(f"expected theta of shape ({S}, P), got {theta.shape}")
        P = theta.shape[1]                                   # (a wrong P is the library's to refuse)
        t_out = _f64(np.asarray(t_out, dtype=np.float64).reshape(-1))
        T = t_out.shape[0]
        traj = np.empty((S, T, D)) if return_draws else None
        mean, sd = np.empty((T, D)), np.empty((T, D))
        status, nf = np.zeros(max(S, 1), dtype=np.int32), C.c_int32(0)
        if method != "rk4":
            reason, n_acc, n_rej = (np.zeros(max(S, 1), dtype=np.int32) for _ in range(3))
            self._check(self._lib.magi_ode_solve_adaptive(self._h, drift_id, P, S, _ptr(x0), _ptr(theta), T, _ptr(t_out), self.ODE_METHODS[method],
                                                          float(rtol), float(atol), float(h0), int(max_steps), _ptr(traj), _ptr(mean), _ptr(sd),
                                                          status.ctypes.data_as(_ip), reason.ctypes.data_as(_ip), n_acc.ctypes.data_as(_ip),
                                                          n_rej.ctypes.data_as(_ip), C.byref(nf)))
            return {"trajectories": traj, "mean": mean, "sd": sd, "status": status[:S], "n_failed": int(nf.value), "reason": reason[:S],
                    "n_accepted": n_acc[:S], "n_rejected": n_rej[:S]}
        self._check(self._lib.magi_ode_solve(self._h, drift_id, P, S, _ptr(x0), _ptr(theta), T, _ptr(t_out), int(substeps), _ptr(traj),
                                             _ptr(mean), _ptr(sd), status.ctypes.data_as(_ip), C.byref(nf)))
        return {"trajectories": traj, "mean": mean, "sd": sd, "status": status[:S], "n_failed": int(nf.value)}

    LINKS = {"identity": 0, "log": 1, "sqrt": 2}          # (MAGI_LINK_* of include/magi_hip.h)

    def ode_sensitivities(self, x0, theta, t_out, substeps=4, wrt=None, relative=False, obs=None, return_draws=True, drift=None):
        """Forward sensitivities of ``ode_solve``'s RK4 trajectories on the device (magi_ode_sensitivities; the scheme and the fixed orders
        are stated in include/magi_hip.h): the exact derivative of the discrete map, for S draws at once.  x0 [S, D], theta [S, P], t_out,
        substeps and drift as in ``ode_solve``.  ``wrt``: the columns, distinct indices in [0, P + D) -- q < P is theta_q, q >= P is
        component q - P of x0; None: all P + D in that order.  ``relative``: every sensitivity times the draw's own theta_q or x0
        component (the sensitivity to the log parameter).  ``obs``: None, or a dict(j [n] output indices, comp [n] components,
        sigma_sq [S, D] the draws' variances on the link's scale, weight [n] or None, link [D] of "identity" / "log" / "sqrt" (or
        MAGI_LINK_* codes) or None) -- the observations whose Fisher information F[s] = sum_k w_k / sigma_sq g'(x)^2 s_a s_b is formed per
        draw.  Returns dict(trajectories [S, T, D] and sens [S, T, D, Q] (None without ``return_draws``), sens_mean, sens_sd [T, D, Q] over
        the draws with status 0, status [S], n_failed, cols [Q]; with ``obs`` also fim [S, Q, Q] (None without ``return_draws``),
        fim_mean [Q, Q] over the draws whose F is finite and whose status is 0, n_fim_excluded)."""
        if drift is None:
            drift = self.user_drift if self.user_drift is not None else getattr(self, "_problem_drift", None)
            if drift is None:
                raise ValueError("ode_sensitivities on the base library needs drift= (a built-in name) or a problem set before")
        if isinstance(drift, str):
            D, drift_id = DRIFT_SHAPES[drift][0], DRIFT_IDS[drift]
        else:
            D, drift_id = drift.D, drift.device_id
        x0, theta = _f64(x0), _f64(theta)
        S = x0.shape[0]
        x0 = _f64(x0, (S, D))
        if theta.ndim != 2 or theta.shape[0] != S:
            raise ValueError(f"expected theta of shape ({S}, P), got {theta.shape}")
        P = theta.shape[1]                                   # (a wrong P is the library's to refuse)
        t_out = _f64(np.asarray(t_out, dtype=np.float64).reshape(-1))
        T = t_out.shape[0]
        cols = np.ascontiguousarray(np.arange(P + D) if wrt is None else np.asarray(wrt).reshape(-1), dtype=np.int32)
        Q = cols.shape[0]
        i32 = lambda a: None if a is None else a.ctypes.data_as(_ip)
        n_obs, oj, oc, ow, sig, link = 0, None, None, None, None, None
        if obs is not None:
            oj = np.ascontiguousarray(np.asarray(obs["j"]).reshape(-1), dtype=np.int32)
            oc = np.ascontiguousarray(np.asarray(obs["comp"]).reshape(-1), dtype=np.int32)
            n_obs = oj.shape[0]
            if oc.shape[0] != n_obs:
                raise ValueError(f"obs: {n_obs} output indices for {oc.shape[0]} components")
            ow = None if obs.get("weight") is None else _f64(np.asarray(obs["weight"], dtype=np.float64).reshape(-1), (n_obs,))
            sig = None if obs.get("sigma_sq") is None else _f64(obs["sigma_sq"], (S, D))
            if obs.get("link") is not None:
                link = np.ascontiguousarray([self.LINKS.get(v, v) if isinstance(v, str) else int(v) for v in obs["link"]], dtype=np.int32)
                if link.shape[0] != D:
                    raise ValueError(f"obs: expected {D} links, got {link.shape[0]}")
        fisher = n_obs > 0
        traj = np.empty((S, T, D)) if return_draws else None
        sens = np.empty((S, T, D, Q)) if return_draws else None
        mean, sd = np.empty((T, D, Q)), np.empty((T, D, Q))
        fim = np.empty((S, Q, Q)) if (fisher and return_draws) else None
        fim_mean = np.empty((Q, Q)) if fisher else None
        status, nf, nex = np.zeros(max(S, 1), dtype=np.int32), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.magi_ode_sensitivities(self._h, drift_id, P, S, _ptr(x0), _ptr(theta), T, _ptr(t_out), int(substeps), Q, i32(cols),
                                                     int(bool(relative)), n_obs, i32(oj), i32(oc), _ptr(ow), _ptr(sig), i32(link), _ptr(traj),
                                                     _ptr(sens), _ptr(mean), _ptr(sd), _ptr(fim), _ptr(fim_mean), i32(status), C.byref(nf),
                                                     C.byref(nex) if fisher else None))
        out = {"trajectories": traj, "sens": sens, "sens_mean": mean, "sens_sd": sd, "status": status[:S], "n_failed": int(nf.value), "cols": cols}
        if fisher:
            out.update(fim=fim, fim_mean=fim_mean, n_fim_excluded=int(nex.value))
        return out

    def sampler_sensitivities(self, t_out, grid_out=None, start_index=0, chains=None, member=None, thin=1, substeps=4, wrt=None, relative=False,
                              return_draws=True):
        """``ode_sensitivities`` of the finished sampler run's draws, computed from the device-resident samples (magi_sampler_sensitivities):
        no draw is copied to the host first, so it also serves a run whose samples were never downloaded.  Draw s starts at its X at grid
        row ``start_index`` with its theta on the natural scale and is reported at ``t_out``; every ``thin``-th result of each chain.
        ``grid_out`` [N]: the index in ``t_out`` of grid point i, or -1 -- the observed entries with grid_out >= 0 are the observations of
        the Fisher information, under the handle's (a group member's own) links, weights, LB and fixed variances; None: none.
        ``chains`` / ``member`` as in ``sampler_summary``; ``wrt`` / ``relative`` as in ``ode_sensitivities``.  Returns its dictionary
        (fim, fim_mean, n_fim_excluded only when an observation is used) plus n_obs_used, obs_index [n_obs_used, 2] = (grid point i,
        component d) ascending in d N + i, and x0 [S, D], theta [S, P], sigma_sq [S, D]: the draws as the device formed them, chain-major."""
        chain0, n_sel = self._chain_range(chains, member)
        R = self._cfg.num_results if self._cfg is not None else 0
        thin = int(thin)
        S = n_sel * (-(-R // thin) if thin >= 1 else 0)
        D, P = self.D, self.P
        t_out = _f64(np.asarray(t_out, dtype=np.float64).reshape(-1))
        T = t_out.shape[0]
        cols = np.ascontiguousarray(np.arange(P + D) if wrt is None else np.asarray(wrt).reshape(-1), dtype=np.int32)
        Q = cols.shape[0]
        i32 = lambda a: None if a is None else a.ctypes.data_as(_ip)
        go = None
        if grid_out is not None:
            go = np.ascontiguousarray(np.asarray(grid_out).reshape(-1), dtype=np.int32)
            if go.shape[0] != self.N:
                raise ValueError(f"grid_out: expected {self.N} entries, got {go.shape[0]}")
        idx = np.zeros(max(self.N * D, 1), dtype=np.int32)
        traj = np.empty((S, T, D)) if return_draws else None
        sens = np.empty((S, T, D, Q)) if return_draws else None
        mean, sd = np.empty((T, D, Q)), np.empty((T, D, Q))
        fim = np.full((S, Q, Q), np.nan) if return_draws else None
        fim_mean = np.full((Q, Q), np.nan)
        x0, th, s2 = np.empty((S, D)), np.empty((S, P)), np.empty((S, D))
        status = np.zeros(max(S, 1), dtype=np.int32)
        nf, nex, n_obs = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.magi_sampler_sensitivities(self._h, chain0, n_sel, thin, int(start_index), T, _ptr(t_out), int(substeps), i32(go), Q, i32(cols),
                                                         int(bool(relative)), _ptr(traj), _ptr(sens), _ptr(mean), _ptr(sd), _ptr(fim), _ptr(fim_mean),
                                                         i32(status), C.byref(nf), C.byref(nex), C.byref(n_obs), i32(idx), _ptr(x0), _ptr(th), _ptr(s2)))
        K = int(n_obs.value)
        e = idx[:K].astype(np.int64)
        out = {"trajectories": traj, "sens": sens, "sens_mean": mean, "sens_sd": sd, "status": status[:S], "n_failed": int(nf.value), "cols": cols,
               "n_obs_used": K, "obs_index": np.stack([e % self.N, e // self.N], axis=1), "x0": x0, "theta": th, "sigma_sq": s2}
        if K:
            out.update(fim=fim, fim_mean=fim_mean, n_fim_excluded=int(nex.value))
        return out

    @staticmethod
    def _probs(probs):
        probs = _f64(np.asarray(probs, dtype=np.float64).reshape(-1))
        return probs, probs.shape[0]

    def summarize(self, draws, probs=DEFAULT_PROBS, max_lag=0):
        """Posterior summaries and convergence diagnostics of ``draws`` [C chains, R draws, ...] on the device (magi_summarize; the
        definitions are in include/magi_hip.h): dict(mean, sd (ddof = 1), rhat (split), ess, mcse_mean -- each of the trailing shape --
        quantiles [len(probs), ...] (numpy's "linear" method on the pooled draws), probs, n_nonfinite (columns with a non-finite draw:
        all their statistics are NaN)).  ``max_lag``: the largest autocorrelation lag of the ESS, <= 0: all."""
        draws = _f64(draws)
        if draws.ndim < 2:
            raise ValueError(f"expected draws of shape (chains, draws, ...), got {draws.shape}")
        n_c, n_r, shape = draws.shape[0], draws.shape[1], draws.shape[2:]
        K = int(np.prod(shape, dtype=np.int64))
        probs, n_q = self._probs(probs)
        outs = _summary_arrays(shape, n_q)
        nf = C.c_int32(0)
        self._check(self._lib.magi_summarize(self._h, n_c, n_r, K, _ptr(draws), n_q, _ptr(probs), int(max_lag), *[_ptr(o) for o in outs], C.byref(nf)))
        out = dict(zip(SUMMARY_STATS, outs))
        out.update(probs=probs, n_nonfinite=int(nf.value))
        return out

    def _chain_range(self, chains, member):
        """(chain0, n_sel) of ``chains`` (None: all; a contiguous run of chain indices, or a slice) or of ``member`` of a MagiGroup."""
        if member is not None:
            if chains is not None:
                raise ValueError("give chains or member, not both")
            if not getattr(self, "members", None):
                raise ValueError("member= selects a member of a MagiGroup; this engine is not a group")
            per = self.n_chains // len(self.members)
            chain0, n_sel = int(member) * per, per
        elif chains is None:
            chain0, n_sel = 0, self.n_chains
        else:
            idx = np.arange(self.n_chains)[chains] if isinstance(chains, slice) else np.asarray(list(chains), dtype=np.int64)
            if idx.size == 0 or np.any(np.diff(idx) != 1):
                raise ValueError("chains must be a contiguous, increasing run of chain indices")
            chain0, n_sel = int(idx[0]), int(idx.size)
        return chain0, n_sel

    def sampler_summary(self, chains=None, probs=DEFAULT_PROBS, max_lag=0, member=None):
        """Summaries of the finished sampler run, computed on the device-resident samples (magi_sampler_summarize): no draw is copied to the
        host.  Returns dict(X, sigma_sqs, thetas, probs, n_nonfinite); X, sigma_sqs (= softplus(sig_pre) + LB) and thetas
        (= softplus(th_pre); under ``set_theta_support`` the natural scale of each parameter's support, a group member's own) each a dict as
        ``summarize`` returns, of shapes [N, D], [D] and [P].  ``chains``: None (all) or a contiguous
        run of chain indices (a range, or (first, count) as a slice) pooled into one summary.  ``member`` (a MagiGroup): the chains of
        that member -- a group's members sample different posteriors and are never pooled."""
        chain0, n_sel = self._chain_range(chains, member)
        probs, n_q = self._probs(probs)
        blocks = {"X": _summary_arrays((self.N, self.D), n_q), "sigma_sqs": _summary_arrays((self.D,), n_q),
                  "thetas": _summary_arrays((self.P,), n_q)}
        nf = C.c_int32(0)
        self._check(self._lib.magi_sampler_summarize(self._h, chain0, n_sel, n_q, _ptr(probs), int(max_lag),
                                                     *[_ptr(o) for b in ("X", "sigma_sqs", "thetas") for o in blocks[b]], C.byref(nf)))
        out = {b: dict(zip(SUMMARY_STATS, arrs)) for b, arrs in blocks.items()}
        out.update(probs=probs, n_nonfinite=int(nf.value))
        return out

    def rank_diagnostics(self, draws, max_lag=0, tail_prob=0.05, return_z=False):
        """Rank-normalised split R-hat, bulk ESS and tail ESS (Vehtari et al. 2021) of ``draws`` [C chains, R draws, ...] on the device
        (magi_rank_diagnostics; the definitions are in include/magi_hip.h): dict(rhat_rank, ess_bulk, ess_tail -- each of the trailing
        shape --, n_nonfinite).  ``tail_prob`` in (0, 0.5]: the tail ESS is that of the lower and upper ``tail_prob`` quantile indicators.
        ``return_z=True`` adds rank, z and z_folded, each of the shape of ``draws``: the pooled average ranks and the normal scores the
        diagnostics are the ``summarize`` rhat / ess of (for rank plots)."""
        draws = _f64(draws)
        if draws.ndim < 2:
            raise ValueError(f"expected draws of shape (chains, draws, ...), got {draws.shape}")
        n_c, n_r, shape = draws.shape[0], draws.shape[1], draws.shape[2:]
        K = int(np.prod(shape, dtype=np.int64))
        outs = [np.empty(shape) for _ in RANK_STATS]
        series = [np.empty(draws.shape) if return_z else None for _ in RANK_SERIES]
        nf = C.c_int32(0)
        self._check(self._lib.magi_rank_diagnostics(self._h, n_c, n_r, K, _ptr(draws), int(max_lag), float(tail_prob), *[_ptr(o) for o in outs],
                                                    *[None if a is None else _ptr(a) for a in series], C.byref(nf)))
        out = dict(zip(RANK_STATS, outs))
        if return_z:
            out.update(zip(RANK_SERIES, series))
        out["n_nonfinite"] = int(nf.value)
        return out

    def sampler_rank_diagnostics(self, chains=None, member=None, max_lag=0, tail_prob=0.05):
        """``rank_diagnostics`` of the finished sampler run, computed on the device-resident samples (magi_sampler_rank_diagnostics): no
        draw is copied to the host.  Returns dict(X, sigma_sqs, thetas, n_nonfinite); the three blocks, on the natural scale as in
        ``sampler_summary``, each dict(rhat_rank, ess_bulk, ess_tail) of shapes [N, D], [D] and [P].  ``chains`` / ``member`` as in
        ``sampler_summary``."""
        chain0, n_sel = self._chain_range(chains, member)
        blocks = {b: [np.empty(shape) for _ in RANK_STATS] for b, shape in (("X", (self.N, self.D)), ("sigma_sqs", (self.D,)), ("thetas", (self.P,)))}
        nf = C.c_int32(0)
        self._check(self._lib.magi_sampler_rank_diagnostics(self._h, chain0, n_sel, int(max_lag), float(tail_prob),
                                                            *[_ptr(o) for b in ("X", "sigma_sqs", "thetas") for o in blocks[b]], C.byref(nf)))
        out = {b: dict(zip(RANK_STATS, arrs)) for b, arrs in blocks.items()}
        out["n_nonfinite"] = int(nf.value)
        return out

    def matern_cross(self, t_new, I, phi1, phi2, nu=2.01):
        """Matern cross blocks of the times ``t_new`` [T] against the grid times ``I`` [N] (magi_matern_cross): (Ks, pKs), each [T, N],
        Ks[m, j] = k(t_new[m], I[j]) and pKs its derivative in the first argument; with ``t_new = I`` the Kappa and p_Kappa of
        ``matern_blocks`` bit for bit."""
        t_new, I = _f64(np.asarray(t_new, dtype=np.float64).reshape(-1)), _f64(np.asarray(I, dtype=np.float64).reshape(-1))
        T, N = t_new.shape[0], I.shape[0]
        Ks, pKs = np.empty((T, N)), np.empty((T, N))
        self._check(self._lib.magi_matern_cross(self._h, _ptr(t_new), T, _ptr(I), N, float(phi1), float(phi2), float(nu), _ptr(Ks), _ptr(pKs)))
        return Ks, pKs

    def gp_predict(self, I, phi1s, phi2s, mu, t_new, X, nu=2.01, derivative=True):
        """The draws ``X`` [S, N, D] of the trajectory on the grid ``I`` conditioned to the times ``t_new`` [T] against the resident dense
        C_inv (magi_gp_predict; the definitions are in include/magi_hip.h): dict(x_new [S, T, D], the conditional means; cond_var [T, D],
        their conditional variance; with ``derivative`` dx_new and dcond_var, the same for x'(t))."""
        I = _f64(np.asarray(I, dtype=np.float64).reshape(-1))
        t_new = _f64(np.asarray(t_new, dtype=np.float64).reshape(-1))
        N, T = I.shape[0], t_new.shape[0]
        phi1s = _f64(np.asarray(phi1s, dtype=np.float64).reshape(-1))
        D = phi1s.shape[0]
        phi2s, mu = _f64(np.asarray(phi2s, dtype=np.float64).reshape(-1), (D,)), _f64(np.asarray(mu, dtype=np.float64).reshape(-1), (D,))
        X = _f64(X)
        S = X.shape[0]
        X = _f64(X, (S, N, D))
        out = {"x_new": np.empty((S, T, D)), "cond_var": np.empty((T, D)),
               "dx_new": np.empty((S, T, D)) if derivative else None, "dcond_var": np.empty((T, D)) if derivative else None}
        self._check(self._lib.magi_gp_predict(self._h, _ptr(I), N, D, _ptr(phi1s), _ptr(phi2s), float(nu), _ptr(mu), T, _ptr(t_new), S, _ptr(X),
                                              _ptr(out["x_new"]), _ptr(out["dx_new"]), _ptr(out["cond_var"]), _ptr(out["dcond_var"])))
        return out

    def sampler_gp_predict(self, I, phi1s, phi2s, t_new, chains=None, member=None, nu=2.01, probs=DEFAULT_PROBS, max_lag=0, derivative=True,
                           return_draws=False):
        """The finished sampler run's trajectory draws conditioned to the times ``t_new`` [T], computed on the device-resident samples
        (magi_sampler_gp_predict): no draw is copied to the host.  ``I``, ``phi1s``, ``phi2s``, ``nu``: the grid and hyper-parameters the
        resident C_inv was built with.  Returns dict(t, X, dX, cond_var, dcond_var, probs, n_nonfinite): X a dict as ``summarize`` returns
        over the conditional means x_new, of shape [T, D]; cond_var [T, D] their conditional variance; dX / dcond_var the same for x'(t)
        (None without ``derivative``).  ``return_draws`` adds X_draws (and dX_draws) [chains, draws, T, D].  ``chains`` / ``member`` as in
        ``sampler_summary``; a member's matrices and mu are its own."""
        chain0, n_sel = self._chain_range(chains, member)
        I = _f64(np.asarray(I, dtype=np.float64).reshape(-1), (self.N,))
        t_new = _f64(np.asarray(t_new, dtype=np.float64).reshape(-1))
        T, D = t_new.shape[0], self.D
        phi1s, phi2s = _f64(np.asarray(phi1s, dtype=np.float64).reshape(-1), (D,)), _f64(np.asarray(phi2s, dtype=np.float64).reshape(-1), (D,))
        probs, n_q = self._probs(probs)
        R = self._cfg.num_results if self._cfg is not None else 0
        xs = _summary_arrays((T, D), n_q)
        dxs = _summary_arrays((T, D), n_q) if derivative else [None] * 6
        cv, dcv = np.empty((T, D)), (np.empty((T, D)) if derivative else None)
        xd = np.empty((n_sel, R, T, D)) if return_draws else None
        dxd = np.empty((n_sel, R, T, D)) if return_draws and derivative else None
        nf = C.c_int32(0)
        self._check(self._lib.magi_sampler_gp_predict(self._h, chain0, n_sel, _ptr(I), _ptr(phi1s), _ptr(phi2s), float(nu), T, _ptr(t_new), n_q,
                                                      _ptr(probs), int(max_lag), _ptr(xd), _ptr(dxd), _ptr(cv), _ptr(dcv),
                                                      *[_ptr(a) for a in xs + dxs], C.byref(nf)))
        out = {"t": t_new, "X": dict(zip(SUMMARY_STATS, xs)), "dX": dict(zip(SUMMARY_STATS, dxs)) if derivative else None,
               "cond_var": cv, "dcond_var": dcv, "probs": probs, "n_nonfinite": int(nf.value)}
        if return_draws:
            out["X_draws"] = xd
            if derivative:
                out["dX_draws"] = dxd
        return out

    def gp_profile(self):
        """Device time (ms) of the stages of the last gp_predict / sampler_gp_predict under ``set_option("gp_profile", 1)`` (magi_gp_profile)."""
        ms = np.zeros(5)
        self._check(self._lib.magi_gp_profile(self._h, _ptr(ms)))
        return dict(zip(("cross_blocks", "weights", "application_gemm", "application_epilogue", "statistics"), ms.tolist()))

    def _elpd_outputs(self, n, loo):
        return {s: (np.empty(n) if (loo or s in ("lpd", "p_waic", "elpd_waic")) else None) for s in ELPD_POINTWISE}

    def elpd(self, loglik, loo=True):
        """WAIC and PSIS-LOO of a log-likelihood array ``loglik`` [C chains, R draws, K observations] on the device (magi_elpd; the
        definitions are in include/magi_hip.h): a sharded job's gathered log-likelihoods, or any other model's.  Returns the dictionary
        of ``host.elpd_result``: ``pointwise`` (lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat, each [K]), the totals with their standard
        errors, ``n_khat_bad``, ``n_nonfinite`` (columns with a non-finite entry: all their outputs are NaN).  ``loo=False`` leaves the
        three PSIS outputs out (None) -- the only way past C R = 466033, the bound of the device's tail sort."""
        loglik = _f64(loglik)
        if loglik.ndim != 3:
            raise ValueError(f"expected loglik of shape (chains, draws, observations), got {loglik.shape}")
        n_c, n_r, K = loglik.shape
        outs = self._elpd_outputs(K, loo)
        nf = C.c_int32(0)
        self._check(self._lib.magi_elpd(self._h, n_c, n_r, K, _ptr(loglik), *[_ptr(outs[s]) for s in ELPD_POINTWISE], C.byref(nf)))
        return elpd_result(outs, None, nf.value)

    def sampler_elpd(self, chains=None, member=None, loglik=False, loo=True):
        """Pointwise log-likelihood, WAIC and PSIS-LOO of the finished sampler run, computed on the device-resident samples
        (magi_sampler_elpd): no draw is copied to the host.  One entry per observation, in the order of ``obs_index`` [n_obs, 2] = (grid
        point i, component d), ascending in d N + i; the log-likelihood is the untempered observation density under the handle's (a
        group member's own) links, weights, LB and fixed variances, on the LINK's scale.  ``chains`` / ``member`` as in
        ``sampler_summary``.  ``loglik=True`` adds ``loglik`` [chains, draws, n_obs], the log-likelihood itself.  ``loo`` as in ``elpd``.
        Returns the dictionary of ``host.elpd_result``."""
        chain0, n_sel = self._chain_range(chains, member)
        group = getattr(self, "members", None)
        cap = (group[chain0 // (self.n_chains // len(group))] if group else self)._n_obs      # observations given to set_problem: n_obs is at most that
        outs = self._elpd_outputs(cap, loo)
        idx = np.zeros(max(cap, 1), dtype=np.int32)
        ll = np.empty(n_sel * self._cfg.num_results * cap) if loglik and self._cfg is not None else None
        n_obs, nf = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.magi_sampler_elpd(self._h, chain0, n_sel, *[_ptr(outs[s]) for s in ELPD_POINTWISE], idx.ctypes.data_as(_ip),
                                                C.byref(n_obs), _ptr(ll), C.byref(nf)))
        n = int(n_obs.value)
        outs = {s: (None if v is None else v[:n].copy()) for s, v in outs.items()}
        if ll is not None:
            ll = ll[:n_sel * self._cfg.num_results * n].reshape(n_sel, self._cfg.num_results, n)
        e = idx[:n].astype(np.int64)
        return elpd_result(outs, np.stack([e % self.N, e // self.N], axis=1), nf.value, loglik=ll)

    @staticmethod
    def _ppc_outputs(S, K, D, n_q, y_rep, discrepancies):
        return {"y_rep": np.empty((S, K)) if y_rep else None, "mean": np.empty(K), "sd": np.empty(K), "quant": np.empty((n_q, K)), "pit": np.empty(K),
                "T_obs": np.empty((S, D, 4)) if discrepancies else None, "T_rep": np.empty((S, D, 4)) if discrepancies else None,
                "pval": np.empty((D, 4)), "excl": np.zeros(D, dtype=np.int32)}

    @staticmethod
    def _ppc_pointers(o):
        return [_ptr(o[s]) for s in ("y_rep", "mean", "sd", "quant", "pit", "T_obs", "T_rep", "pval")] + [o["excl"].ctypes.data_as(_ip)]

    def ppc(self, x, comp, sigma_sq, link=None, weight=None, y=None, extra_var=None, seed=0, chain_ids=None, probs=DEFAULT_PROBS,
            return_draws=False, discrepancies=False):
        """Posterior predictive check of ``x`` [C chains, R draws, K columns], the latent state at K observation points, on the device
        (magi_ppc; the definitions are in include/magi_hip.h): column k belongs to component ``comp[k]`` of D = sigma_sq.shape[-1],
        ``sigma_sq`` [C, R, D] is the draws' noise variance on the link's scale, ``link`` [D] codes or names (None: identity), ``weight``,
        ``y`` (NaN: no datum, a pure prediction) and ``extra_var`` (a latent variance added per column, e.g. the GP's cond_var) are [K] or
        None.  ``seed`` and ``chain_ids`` [C] (None: 0 .. C - 1) select the Philox noise.  Any draws serve: those of ``gp_predict``, or the
        ODE solutions of ``posterior_trajectories`` at the observation times.  Returns the dictionary of ``host.ppc_result``;
        ``return_draws`` adds ``y_rep`` [C, R, K], ``discrepancies`` adds ``T_obs`` and ``T_rep`` [C, R, D, 4]."""
        x, sigma_sq = _f64(x), _f64(sigma_sq)
        if x.ndim != 3 or sigma_sq.ndim != 3 or sigma_sq.shape[:2] != x.shape[:2]:
            raise ValueError(f"expected x (chains, draws, columns) and sigma_sq (chains, draws, components), got {x.shape} and {sigma_sq.shape}")
        n_c, n_r, K = x.shape
        D = sigma_sq.shape[2]
        comp = np.ascontiguousarray(np.asarray(comp).reshape(-1), dtype=np.int32)
        if comp.shape[0] != K:
            raise ValueError(f"comp: expected {K} entries, got {comp.shape[0]}")
        lk = None if link is None else np.ascontiguousarray(obs_model_spec(link, D), dtype=np.int32)
        opt = lambda a: None if a is None else _f64(np.asarray(a, dtype=np.float64).reshape(-1), (K,))
        weight, y, extra_var = opt(weight), opt(y), opt(extra_var)
        ids = None if chain_ids is None else np.ascontiguousarray(np.asarray(chain_ids).reshape(-1), dtype=np.int64)
        if ids is not None and ids.shape[0] != n_c:
            raise ValueError(f"chain_ids: expected {n_c} entries, got {ids.shape[0]}")
        probs, n_q = self._probs(probs)
        o = self._ppc_outputs(n_c * n_r, K, D, n_q, return_draws, discrepancies)
        nf = C.c_int32(0)
        self._check(self._lib.magi_ppc(self._h, n_c, n_r, K, D, _ptr(x), comp.ctypes.data_as(_ip), _ptr(sigma_sq),
                                       None if lk is None else lk.ctypes.data_as(_ip), _ptr(weight), _ptr(y), _ptr(extra_var), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                       None if ids is None else ids.ctypes.data_as(_lp), n_q, _ptr(probs), *self._ppc_pointers(o), C.byref(nf)))
        shape = lambda a, *s: None if a is None else a.reshape(n_c, n_r, *s)
        return ppc_result(comp, D, o["mean"], o["sd"], o["quant"], o["pit"], o["pval"], o["excl"], nf.value, probs=probs,
                          y_rep=shape(o["y_rep"], K), T_obs=shape(o["T_obs"], D, 4), T_rep=shape(o["T_rep"], D, 4))

    def sampler_ppc(self, chains=None, member=None, seed=0, probs=DEFAULT_PROBS, return_draws=False, discrepancies=False, sigma_sq=False):
        """Posterior predictive check of the fitted observations of the finished sampler run, computed on the device-resident samples
        (magi_sampler_ppc): no draw is copied to the host.  One column per observation, in the order of ``obs_index`` [n_obs, 2] = (grid
        point i, component d), ascending in d N + i, under the handle's (a group member's own) links, weights, LB and fixed variances.
        ``chains`` / ``member`` as in ``sampler_summary``; ``seed`` selects the Philox noise (a stream of its own: the sampler's draws are
        not touched).  Returns the dictionary of ``host.ppc_result``; ``return_draws`` adds ``y_rep`` [chains, draws, n_obs],
        ``discrepancies`` ``T_obs`` / ``T_rep`` [chains, draws, D, 4], ``sigma_sq`` the draws' ``sigma_sq`` [chains, draws, D] as the kernel
        formed them."""
        chain0, n_sel = self._chain_range(chains, member)
        group = getattr(self, "members", None)
        cap = (group[chain0 // (self.n_chains // len(group))] if group else self)._n_obs      # observations given to set_problem: n_obs is at most that
        R = self._cfg.num_results if self._cfg is not None else 0
        D = self.D
        probs, n_q = self._probs(probs)
        idx = np.zeros(max(cap, 1), dtype=np.int32)
        n_obs, nf = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.magi_sampler_ppc(self._h, chain0, n_sel, int(seed) & 0xFFFFFFFFFFFFFFFF, n_q, _ptr(probs), *([None] * 10), idx.ctypes.data_as(_ip),
                                               C.byref(n_obs), None))
        K = int(n_obs.value)
        e = idx[:K].astype(np.int64)
        o = self._ppc_outputs(n_sel * R, K, D, n_q, return_draws, discrepancies)
        s2 = np.empty((n_sel, R, D)) if sigma_sq else None
        if K:
            self._check(self._lib.magi_sampler_ppc(self._h, chain0, n_sel, int(seed) & 0xFFFFFFFFFFFFFFFF, n_q, _ptr(probs), *self._ppc_pointers(o), C.byref(nf), None,
                                                   None, _ptr(s2)))
        else:
            o["pval"][:] = np.nan
        shape = lambda a, *s: None if a is None else a.reshape(n_sel, R, *s)
        out = ppc_result(e // self.N, D, o["mean"], o["sd"], o["quant"], o["pit"], o["pval"], o["excl"], nf.value,
                         obs_index=np.stack([e % self.N, e // self.N], axis=1), probs=probs, y_rep=shape(o["y_rep"], K),
                         T_obs=shape(o["T_obs"], D, 4), T_rep=shape(o["T_rep"], D, 4))
        if sigma_sq:
            out["sigma_sq"] = s2
        return out

    def sampler_sigma_sq(self, chains=None, member=None):
        """The noise variances sigma_sq [chains, draws, D] of the finished sampler run's draws as the device forms them (softplus(sig_pre)
        + LB, or a fixed variance's constant; magi_sampler_ppc's sigma_sq_out): what ``ppc`` takes beside draws derived from the run's."""
        chain0, n_sel = self._chain_range(chains, member)
        s2 = np.empty((n_sel, self._cfg.num_results if self._cfg is not None else 0, self.D))
        self._check(self._lib.magi_sampler_ppc(self._h, chain0, n_sel, 0, 0, None, *([None] * 12), _ptr(s2)))      # asked for alone: nothing else is computed
        return s2

    def selftest(self, drift=None, force=False):
        """Self-test of the library this engine runs (magi_v2_amd.selftest.ensure: cached verdict, or a run on handles of its own);
        returns the Report, raises MagiSelfTestError.  The base library is tested for ``drift`` (a built-in name) or, None, all three."""
        from . import selftest
        return selftest.ensure(self._lib._name, self.user_drift if self.user_drift is not None else drift, self.device, force=force)

    def stream_kernel_name(self, n_chains=1):
        buf = C.create_string_buffer(64)
        self._check(self._lib.magi_stream_kernel_name(self._h, int(n_chains), buf, 64))
        return buf.value.decode()

    # -- matrices -------------------------------------------------------------------------------
    def build_matrices(self, I, phi1s, phi2s, nu=2.01, bandsize=None, want_host=True):
        """magi_v2.py:774-823 + :126-128 + :271-274 on the GPU for all components."""
        I = _f64(np.asarray(I).reshape(-1))
        phi1s, phi2s = _f64(phi1s), _f64(phi2s)
        N, D = I.shape[0], phi1s.shape[0]
        b = -1 if bandsize is None else int(bandsize)
        outs = [np.empty((D, N, N)) for _ in range(3)] if want_host else [None, None, None]
        self._check(self._lib.magi_build_matrices(self._h, _ptr(I), N, D, _ptr(phi1s), _ptr(phi2s), float(nu), b,
                                                  *[_ptr(o) for o in outs]))
        self.N, self.D = N, D
        return tuple(outs) if want_host else None

    def build_dense(self, I, D, comps, phi1s, phi2s, nu=2.01):
        """Matrices of the listed components into the device-resident dense stacks of a D-component problem (no host copy,
        no packing): magi_v2.py:122-128 / 262-268 / 447-451."""
        I = _f64(np.asarray(I).reshape(-1))
        comps = np.ascontiguousarray(comps, dtype=np.int32)
        phi1s, phi2s = _f64(phi1s, comps.shape), _f64(phi2s, comps.shape)
        self._check(self._lib.magi_build_dense(self._h, _ptr(I), I.shape[0], int(D), comps.shape[0], comps.ctypes.data_as(_ip),
                                               _ptr(phi1s), _ptr(phi2s), float(nu)))
        self.N, self.D = I.shape[0], int(D)

    def pack_resident(self, bandsize=None):
        """Band mask (magi_v2.py:271-274) + packing of the resident dense stacks."""
        self._check(self._lib.magi_pack_resident(self._h, -1 if bandsize is None else int(bandsize)))

    def get_dense(self, bandsize=None):
        """Host copies (C_inv, m, K_inv), each [D, N, N], of the resident stacks with the band mask applied."""
        outs = [np.empty((self.D, self.N, self.N)) for _ in range(3)]
        self._check(self._lib.magi_get_dense(self._h, -1 if bandsize is None else int(bandsize), *[_ptr(o) for o in outs]))
        return tuple(outs)

    def dense_apply(self, which, V, transpose=False):
        """Y[d] = A_d V[d] (or A_d^T V[d]) for the resident stack ``which`` in ("C_inv", "m", "K_inv"); V [D, N] or [D, N, nv]."""
        V = _f64(V)
        vec = V.ndim == 2
        V3 = V[:, :, None] if vec else V
        V3 = _f64(V3, (self.D, self.N, V3.shape[2]))
        Y = np.empty_like(V3)
        self._check(self._lib.magi_dense_apply(self._h, ("C_inv", "m", "K_inv").index(which), int(bool(transpose)), V3.shape[2], _ptr(V3), _ptr(Y)))
        return Y[:, :, 0] if vec else Y

    def fit_hparams(self, I, X_filled, mu, mu_phi2, sd_phi2, sigma_sq_loc, phi1_init, phi2_init, sigma_sq_init, nu=2.01,
                    num_iters=1000, learning_rate=0.01, jitter=1e-6, want_trace=False):
        """magi_v2.py:538-691 on the GPU; returns dict(phi1s, phi2s, sigma_sqs[, loss])."""
        I = _f64(np.asarray(I).reshape(-1))
        X = _f64(X_filled)
        N, D = X.shape
        phi1, phi2, sig = _f64(phi1_init, (D,)).copy(), _f64(phi2_init, (D,)).copy(), _f64(sigma_sq_init, (D,)).copy()
        trace = np.zeros(max(num_iters, 1)) if want_trace else None
        self._check(self._lib.magi_fit_hparams(self._h, _ptr(I), N, D, _ptr(X), _ptr(_f64(mu, (D,))), _ptr(_f64(mu_phi2, (D,))),
                                               _ptr(_f64(sd_phi2, (D,))), _ptr(_f64(sigma_sq_loc, (D,))), float(nu), int(num_iters),
                                               float(learning_rate), float(jitter), _ptr(phi1), _ptr(phi2), _ptr(sig), _ptr(trace)))
        out = {"phi1s": phi1, "phi2s": phi2, "sigma_sqs": sig}
        if want_trace:
            out["loss"] = trace[:num_iters]
        return out

    def theta_init(self, drift, Xhat, mu, num_iters=10000, learning_rate=0.01, theta0=None, want_trace=False):
        """magi_v2.py:133-179 on the GPU (magi_theta_init): the whole Adam loop on the device-resident UNbanded matrices, any drift
        this library carries (``drift``: built-in name or the traced Drift the engine was created for).  Returns theta[P] (, losses)."""
        if isinstance(drift, str):
            P, drift_id = DRIFT_SHAPES[drift][1], DRIFT_IDS[drift]
        else:
            P, drift_id = drift.P, drift.device_id
        Xhat = _f64(Xhat, (self.N, self.D))
        th = np.ones(P) if theta0 is None else _f64(theta0, (P,)).copy()
        trace = np.zeros(max(num_iters, 1)) if want_trace else None
        self._check(self._lib.magi_theta_init(self._h, drift_id, P, _ptr(Xhat), _ptr(_f64(mu, (self.D,))), int(num_iters), float(learning_rate),
                                              _ptr(th), _ptr(trace)))
        return (th, trace[:num_iters]) if want_trace else th

    def matern_blocks(self, I, phi1, phi2, nu=2.01):
        I = _f64(np.asarray(I).reshape(-1))
        N = I.shape[0]
        outs = [np.empty((N, N)) for _ in range(3)]
        self._check(self._lib.magi_matern_blocks(self._h, _ptr(I), N, float(phi1), float(phi2), float(nu),
                                                 *[_ptr(o) for o in outs]))
        return tuple(outs)

    def set_matrices(self, C_inv, m, K_inv, bandsize=None):
        C_inv = _f64(C_inv)
        D, N, _ = C_inv.shape
        m, K_inv = _f64(m, (D, N, N)), _f64(K_inv, (D, N, N))
        b = -1 if bandsize is None else int(bandsize)
        self._check(self._lib.magi_set_matrices(self._h, N, D, b, _ptr(C_inv), _ptr(m), _ptr(K_inv)))
        self.N, self.D = N, D

    # -- problem --------------------------------------------------------------------------------
    def set_times(self, I):
        """The times of the grid points ([N] or [N, 1]; magi_set_times), after the matrices: what a drift that uses ``t`` is evaluated at --
        the reference passes its grid ``self.I``.  Required before ``set_problem`` / ``theta_init`` for such a drift, harmless otherwise."""
        I = _f64(np.asarray(I, dtype=np.float64).reshape(-1))
        self._check(self._lib.magi_set_times(self._h, _ptr(I), I.shape[0]))

    def set_problem(self, mu, N_ds, obs_idx, y, beta, LB, drift):
        """``drift``: built-in name, or the Drift this engine was created for."""
        D = self.D
        if not isinstance(drift, str):
            if self.user_drift is None and not drift.is_builtin:
                raise ValueError("engine was not created for this user drift: MagiEngine(device, drift=...)")
            P, drift_id = drift.P, drift.device_id
        else:
            P, drift_id = DRIFT_SHAPES[drift][1], DRIFT_IDS[drift]
        mu, N_ds, LB = _f64(mu, (D,)), _f64(N_ds, (D,)), _f64(LB, (D,))
        obs_idx = np.ascontiguousarray(obs_idx, dtype=np.int64)
        y = _f64(y, obs_idx.shape)
        self._check(self._lib.magi_set_problem(self._h, _ptr(mu), _ptr(N_ds), obs_idx.ctypes.data_as(_lp), _ptr(y),
                                               obs_idx.shape[0], float(beta), _ptr(LB), drift_id, P))
        self.P = P
        self._n_obs = int(obs_idx.shape[0])
        self._problem_drift = drift

    def set_theta_support(self, spec):
        """The support of every ODE parameter (magi_set_theta_support), after ``set_problem`` -- which resets it to all-positive: None, or
        P entries out of "positive", "real", ("lower", lo), ("upper", hi) (host.theta_support).  It governs ``logpost_grad``, the next
        ``sampler_init`` and the theta block of ``sampler_summary``; theta_pre stays theta_pre everywhere."""
        if self.P is None:
            raise MagiHipError(-5, "set_theta_support: set the problem first (magi_set_problem)")
        kinds, bounds = theta_support(spec, self.P)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        self._check(self._lib.magi_set_theta_support(self._h, int(self.P), None if spec is None else kinds.ctypes.data_as(_ip), _ptr(bounds)))

    def theta_support(self):
        """The supports in force as (kinds int32[P], bounds float64[P]) (magi_get_theta_support; host.theta_support_spec names them)."""
        if self.P is None:
            raise MagiHipError(-5, "theta_support: set the problem first (magi_set_problem)")
        kinds, bounds = np.zeros(self.P, dtype=np.int32), np.zeros(self.P)
        self._check(self._lib.magi_get_theta_support(self._h, int(self.P), kinds.ctypes.data_as(_ip), _ptr(bounds)))
        return kinds, bounds

    def set_prior(self, sigma_sq_prior=None, theta_prior=None):
        """Priors on the noise variances and the ODE parameters (magi_set_prior), after ``set_problem`` -- which resets them to flat -- and
        after ``set_theta_support``: each None (flat) or one entry per component / parameter out of None / "flat", ("normal", m, s),
        ("lognormal", m, s), ("gamma", k, r), ("invgamma", a, b) and, for a noise variance, ("fixed", c) (host.prior_spec).  They act on the
        natural scale and govern ``logpost_grad``, the next ``sampler_init`` and the sigma^2 block of ``sampler_summary`` (a fixed variance
        reports its constant)."""
        if self.P is None:
            raise MagiHipError(-5, "set_prior: set the problem first (magi_set_problem)")
        ks, as_, bs = prior_spec(sigma_sq_prior, self.D, "sigma_sq")
        kt, at, bt = prior_spec(theta_prior, self.P, "theta", self.theta_support())
        kinds = np.ascontiguousarray(np.concatenate([ks, kt]), dtype=np.int32)
        a, b = np.ascontiguousarray(np.concatenate([as_, at])), np.ascontiguousarray(np.concatenate([bs, bt]))
        flat = sigma_sq_prior is None and theta_prior is None
        self._check(self._lib.magi_set_prior(self._h, int(self.D + self.P), None if flat else kinds.ctypes.data_as(_ip), _ptr(a), _ptr(b)))

    def prior(self):
        """The priors in force as ((kinds int32[D], a[D], b[D]) of sigma^2, (kinds int32[P], a[P], b[P]) of theta) (magi_get_prior;
        host.prior_spec_echo names them)."""
        if self.P is None:
            raise MagiHipError(-5, "prior: set the problem first (magi_set_problem)")
        n, D = int(self.D + self.P), int(self.D)
        kinds, a, b = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
        self._check(self._lib.magi_get_prior(self._h, n, kinds.ctypes.data_as(_ip), _ptr(a), _ptr(b)))
        return (kinds[:D], a[:D], b[:D]), (kinds[D:], a[D:], b[D:])

    def set_obs_model(self, link=None, weight=None):
        """The observation model (magi_set_obs_model), after ``set_problem`` -- which resets it to the reference's: ``link`` None, one of
        "identity", "log", "sqrt" for all components or one per component (host.obs_model_spec); ``weight`` None or one known weight > 0 per
        observation, in the order of ``set_problem``'s ``obs_idx``.  Gaussian error on the link's scale, sigma^2 the variance there:
        t4 = sum_d (1 / sigma^2_d) sum_k w_k (g_d(x_k) - g_d(y_k))^2.  It governs ``logpost_grad`` and the next ``sampler_init``; samples and
        summaries stay on the natural scale.  Both None: back to the default."""
        if self.P is None:
            raise MagiHipError(-5, "set_obs_model: set the problem first (magi_set_problem)")
        links = np.ascontiguousarray(obs_model_spec(link, self.D), dtype=np.int32)
        w = None if weight is None else _f64(np.asarray(weight, dtype=np.float64).reshape(-1))
        n_obs = self._n_obs if w is None else int(w.shape[0])
        self._check(self._lib.magi_set_obs_model(self._h, int(self.D), None if link is None else links.ctypes.data_as(_ip), n_obs, None if w is None else _ptr(w)))

    def obs_model(self):
        """The observation model in force as (links int32[D], weights float64[n_obs]) (magi_get_obs_model; host.obs_model_spec_echo names
        the links; the weights are 1 when none were given)."""
        if self.P is None:
            raise MagiHipError(-5, "obs_model: set the problem first (magi_set_problem)")
        links, w = np.zeros(self.D, dtype=np.int32), np.ones(self._n_obs)
        self._check(self._lib.magi_get_obs_model(self._h, int(self.D), links.ctypes.data_as(_ip), self._n_obs, _ptr(w)))
        return links, w

    def _states(self, X, sig_pre, th_pre):
        X = _f64(X)
        if X.ndim == 2:
            X, sig_pre, th_pre = X[None], np.asarray(sig_pre)[None], np.asarray(th_pre)[None]
        n = X.shape[0]
        X = _f64(X, (n, self.N, self.D))
        return n, X, _f64(sig_pre, (n, self.D)), _f64(th_pre, (n, self.P))

    def logpost_grad(self, X, sig_pre, th_pre, beta_temp=1.0, want_terms=False, fused=False):
        """unnormalized_log_prob (magi_v2.py:308-348) + gradient for one state or a batch of states.
        fused=True evaluates it through the sampler's single-phase kernels instead."""
        single = np.asarray(X).ndim == 2
        n, X, sp, tp = self._states(X, sig_pre, th_pre)
        logp, gX = np.empty(n), np.empty((n, self.N, self.D))
        gs, gt, terms = np.empty((n, self.D)), np.empty((n, self.P)), np.empty((n, 4))
        fn = self._lib.magi_logpost_grad_fused if fused else self._lib.magi_logpost_grad
        self._check(fn(self._h, n, _ptr(X), _ptr(sp), _ptr(tp), float(beta_temp), _ptr(logp),
                       _ptr(gX), _ptr(gs), _ptr(gt), _ptr(terms)))
        out = (logp[0], gX[0], gs[0], gt[0]) if single else (logp, gX, gs, gt)
        if want_terms:
            out = out + ((terms[0] if single else terms),)
        return out

    # -- sampler --------------------------------------------------------------------------------
    def default_cfg(self, **kw) -> SamplerCfg:
        cfg = SamplerCfg()
        self._lib.magi_sampler_cfg_default(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown sampler option {k}")
            setattr(cfg, k, v)
        return cfg

    def sampler_init(self, cfg: SamplerCfg, X0, sig_pre0, th_pre0, seed: int, chain_ids: Optional[Sequence[int]] = None):
        n, X, sp, tp = self._states(X0, sig_pre0, th_pre0)
        ids = None
        if chain_ids is not None:
            ids = np.ascontiguousarray(chain_ids, dtype=np.int64)
            if ids.shape != (n,):
                raise ValueError("chain_ids must have one entry per chain")
        self._check(self._lib.magi_sampler_init(self._h, C.byref(cfg), n, _ptr(X), _ptr(sp), _ptr(tp),
                                                C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                                None if ids is None else ids.ctypes.data_as(_lp)))
        self.n_chains = n
        self._cfg = cfg
        self._chain_ids = np.arange(n, dtype=np.int64) if ids is None else ids.copy()      # the chains' Philox ids (sampler_sigma_sq / ppc of derived draws)

    def sampler_run(self, n_steps: int):
        """Advance all chains by n_steps transitions; returns (leapfrogs taken, device ms)."""
        lf = C.c_int64(0)
        ms = C.c_double(0.0)
        self._check(self._lib.magi_sampler_run(self._h, int(n_steps), C.byref(lf), C.byref(ms)))
        return lf.value, ms.value

    def sampler_steps_done(self):
        out = np.zeros(self.n_chains, dtype=np.int64)
        self._check(self._lib.magi_sampler_steps_done(self._h, out.ctypes.data_as(_lp)))
        return out

    def sampler_samples(self):
        n, R = self.n_chains, self._cfg.num_results
        X = np.empty((n, R, self.N, self.D))
        sp, tp = np.empty((n, R, self.D)), np.empty((n, R, self.P))
        self._check(self._lib.magi_sampler_get_samples(self._h, _ptr(X), _ptr(sp), _ptr(tp)))
        return X, sp, tp

    def sampler_diag(self) -> SamplerDiag:
        n, T = self.n_chains, self._cfg.num_results + self._cfg.num_burnin_steps
        f = lambda: np.zeros((n, T))
        i = lambda: np.zeros((n, T), dtype=np.int32)
        d = SamplerDiag(f(), f(), i(), i(), i(), i(), i(), f(), f(), f())
        ip = lambda a: a.ctypes.data_as(_ip)
        self._check(self._lib.magi_sampler_get_diag(self._h, _ptr(d.step_size), _ptr(d.log_accept_ratio),
                                                    ip(d.leapfrogs_taken), ip(d.tree_depth), ip(d.has_divergence),
                                                    ip(d.reach_max_depth), ip(d.is_accepted), _ptr(d.target_log_prob),
                                                    _ptr(d.energy), _ptr(d.beta_temp)))
        return d

    def sampler_state(self):
        n = self.n_chains
        X, sp, tp = np.empty((n, self.N, self.D)), np.empty((n, self.D)), np.empty((n, self.P))
        ss, bc = np.empty(n), np.empty(n)
        self._check(self._lib.magi_sampler_get_state(self._h, _ptr(X), _ptr(sp), _ptr(tp), _ptr(ss), _ptr(bc)))
        return X, sp, tp, ss, bc

    CKPT_SCALARS = 16

    def sampler_checkpoint(self):
        """Everything needed to resume the chains at the transition boundary they stand at (between two sampler_run calls):
        dict(X, sig_pre, th_pre, scalars).  See include/magi_hip.h (magi_sampler_get_checkpoint)."""
        X, sp, tp, _, _ = self.sampler_state()
        sc = np.zeros((self.n_chains, self.CKPT_SCALARS))
        self._check(self._lib.magi_sampler_get_checkpoint(self._h, _ptr(sc)))
        return {"X": X, "sig_pre": sp, "th_pre": tp, "scalars": sc}

    def sampler_resume(self, cfg: SamplerCfg, ckpt, seed: int, chain_ids: Optional[Sequence[int]] = None, metric=None):
        """sampler_init at the checkpointed states + the checkpoint's scalars: the next sampler_run continues the run.  A checkpoint does
        not carry the metric: ``metric`` = what sampler_metric() returned when it was taken (and ``cfg.num_adaptation_steps`` the value
        in force then: after a sampler_warmup, the ``n_adapt - stop`` of its last adapted window)."""
        self.sampler_init(cfg, ckpt["X"], ckpt["sig_pre"], ckpt["th_pre"], seed, chain_ids)
        if metric is not None:
            self.sampler_set_metric(*metric)
        sc = _f64(ckpt["scalars"], (self.n_chains, self.CKPT_SCALARS))
        self._check(self._lib.magi_sampler_set_checkpoint(self._h, _ptr(sc)))

    # -- diagonal metric (include/magi_hip.h: magi_sampler_set_metric ...) ---------------------------
    def sampler_set_metric(self, inv_mass_X=None, inv_mass_sig=None, inv_mass_th=None):
        """Per-chain diagonal inverse mass in the layouts of sampler_init ([n, N, D], [n, D], [n, P]; one chain may drop the leading
        axis); no argument: back to the identity metric.  Governs the next transition from its first half step."""
        given = [a is not None for a in (inv_mass_X, inv_mass_sig, inv_mass_th)]
        if not any(given):
            self._check(self._lib.magi_sampler_set_metric(self._h, None, None, None))
            return
        if not all(given):
            raise ValueError("give all three inverse-mass arrays, or none for the identity metric")
        n, X, sp, tp = self._states(inv_mass_X, inv_mass_sig, inv_mass_th)
        if n != self.n_chains:
            raise ValueError(f"the sampler has {self.n_chains} chains, the metric {n}")
        self._check(self._lib.magi_sampler_set_metric(self._h, _ptr(X), _ptr(sp), _ptr(tp)))

    def sampler_metric(self):
        """(inv_mass_X [n, N, D], inv_mass_sig [n, D], inv_mass_th [n, P]) in force; ones under the identity metric."""
        n = self.n_chains
        X, sp, tp = np.empty((n, self.N, self.D)), np.empty((n, self.D)), np.empty((n, self.P))
        self._check(self._lib.magi_sampler_get_metric(self._h, _ptr(X), _ptr(sp), _ptr(tp)))
        return X, sp, tp

    def sampler_metric_window(self, on=True):
        """Open (shift := the chains' current states, sums := 0) or close the window whose states sampler_adapt_metric turns into a metric."""
        self._check(self._lib.magi_sampler_metric_window(self._h, 1 if on else 0))

    def sampler_adapt_metric(self, n, kappa=5.0, rel_floor=1e-3, restart_adapt_steps=-1):
        """The open window of n transitions -> every chain's metric (regularised sample variances; the floor is rel_floor x the chain's
        median variance); restart_adapt_steps >= 0 restarts dual averaging at the rescaled step with that many adaptation steps left.
        Returns (step sizes [n_chains] after the call, number of chains whose metric was left unchanged)."""
        ss = np.empty(self.n_chains)
        rc = self._lib.magi_sampler_adapt_metric(self._h, int(n), float(kappa), float(rel_floor), int(restart_adapt_steps), _ptr(ss))
        if rc < 0:
            self._check(rc)
        return ss, rc

    def sampler_warmup(self, schedule, n_adapt=None, kappa=5.0, rel_floor=1e-3):
        """Run the transitions of ``schedule`` = [(start, stop, adapt_metric_at_stop)] (magi_v2_amd.host.warmup_schedule; contiguous, from
        the transition the chains stand at): a window with adapt_metric_at_stop set is accumulated on the device and turned into the
        metric at its end, dual averaging restarting with ``n_adapt - stop`` adaptation steps left.  ``n_adapt``: the sampler's adaptation
        steps, by default the schedule's end (warmup_schedule tiles [0, n_adapt)).  Returns (leapfrogs, device ms,
        [per adapted window: dict(start, stop, step_size, unchanged)])."""
        schedule = list(schedule)
        if n_adapt is None:
            n_adapt = schedule[-1][1] if schedule else 0
        lf = ms = 0
        windows = []
        for start, stop, adapt in schedule:
            if stop <= start:
                raise ValueError(f"empty window [{start}, {stop})")
            if adapt:
                self.sampler_metric_window(True)
            a, b = self.sampler_run(stop - start)
            lf, ms = lf + a, ms + b
            if adapt:
                ss, kept = self.sampler_adapt_metric(stop - start, kappa, rel_floor, restart_adapt_steps=max(int(n_adapt) - stop, 0))
                windows.append({"start": int(start), "stop": int(stop), "step_size": ss, "unchanged": int(kept)})
        return lf, ms, windows

    def sampler_run_stats(self):
        """(leapfrog slots issued, graph launches) of the last sampler_run."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.magi_sampler_run_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sampler_profile(self, n_slots=512):
        """Mean in-sampler device time (us) per launch of the streaming kernel and of k_point over n_slots slots launched with
        per-kernel HIP events; returns (stream_us, point_us, leapfrogs).  The sampler must be re-initialised afterwards."""
        a, b, lf = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        self._check(self._lib.magi_sampler_profile(self._h, int(n_slots), C.byref(a), C.byref(b), C.byref(lf)))
        return a.value, b.value, lf.value

    # -- instrumentation ------------------------------------------------------------------------
    def time_gradient(self, n_chains=1, reps=50):
        total = C.c_double(0.0)
        ph = np.zeros(8)
        self._check(self._lib.magi_time_gradient(self._h, int(n_chains), int(reps), C.byref(total), _ptr(ph)))
        return total.value, ph

    BUILD_CLASSES = ("matern", "diag_chol_inv", "potrf_panel", "potrf_trailing_syrk", "trtri", "TtT", "m_K_products",
                     "single_phase_operators", "potrf_wall")

    def build_profile(self):
        """Per-class (flops, ms, calls) of the last build_matrices run with set_option("build_profile", 1); the last row, "potrf_wall", is
        filled by every build: its two Cholesky factorisations as a whole (look-ahead included when the build was not profiled)."""
        f, ms = np.zeros(16), np.zeros(16)
        calls = np.zeros(16, dtype=np.int64)
        n = self._lib.magi_build_profile(self._h, _ptr(f), _ptr(ms), calls.ctypes.data_as(_lp))
        return {self.BUILD_CLASSES[i]: (f[i], ms[i], int(calls[i])) for i in range(n)}

    def debug_par(self, chain=0):
        out = np.zeros(64)
        self._check(self._lib.magi_debug_par(self._h, int(chain), _ptr(out)))
        return out

    def gradient_bytes(self, n_chains=1):
        b = np.zeros(8)
        self._check(self._lib.magi_gradient_bytes(self._h, int(n_chains), _ptr(b)))
        return b

    def tile_formats(self, n_chains=1):
        """(operator blocks, blocks of them with an fp32 copy, operator bytes a launch of the streaming kernel of ``n_chains`` reads) of
        the current pack -- option ``tile_demote`` (include/magi_hip.h: magi_tile_formats)."""
        nb, nd, by = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.magi_tile_formats(self._h, int(n_chains), C.byref(nb), C.byref(nd), C.byref(by)))
        return int(nb.value), int(nd.value), float(by.value)

    def stream_carriers(self):
        """The carrier workgroups of the current pack -- option ``stream_carriers`` (include/magi_hip.h: magi_stream_carriers): a dict of
        ``on`` (whether the VALU streaming kernels launch them), ``units`` (64-KB units of every carrier) and ``tasks`` ([carriers, 3] block
        indices, -1 = an empty slot)."""
        on, n = C.c_int(0), C.c_int(0)
        self._check(self._lib.magi_stream_carriers(self._h, C.byref(on), C.byref(n), None, 0))
        units = np.zeros(max(n.value, 1), dtype=np.intc)
        tasks = np.full(3 * max(n.value, 1), -1, dtype=np.intc)
        ip = C.POINTER(C.c_int)
        self._check(self._lib.magi_stream_carriers(self._h, None, None, units.ctypes.data_as(ip), n.value))
        self._check(self._lib.magi_stream_carrier_tasks(self._h, tasks.ctypes.data_as(ip), 3 * n.value))
        return {"on": bool(on.value), "units": units[:n.value].copy(), "tasks": tasks[:3 * n.value].reshape(-1, 3).copy()}

    @staticmethod
    def group(engines):
        """A MagiGroup over ``engines`` (see there)."""
        return MagiGroup(engines)


class MagiGroup(MagiEngine):
    """One sampler over the chains of several problems of one shape on one GPU (include/magi_hip.h: magi_group_create): one captured
    graph, one [stream, point] kernel pair per leapfrog slot for all of them, one host thread.

    ``members``: MagiEngines of one loaded library and one device, each with its matrices and its problem set.  The chains are
    problem-major, C per member: ``sampler_init`` takes G * C states and chain ids (ids may repeat across members), and the chains of member
    m reproduce ``members[m].sampler_init(cfg, <its C states>, seed, <its C ids>)`` bit for bit.  The sampler_* methods work as on an
    engine; the calls that need matrices of their own raise.  The group keeps its members alive; a member changed after ``sampler_init``
    takes effect at the next ``sampler_init``."""

    def __init__(self, engines):
        engines = list(engines)
        if not engines:
            raise ValueError("a group needs at least one member")
        lib, dev = engines[0]._lib, engines[0].device
        for k, e in enumerate(engines):
            if isinstance(e, MagiGroup) or not getattr(e, "_h", None):
                raise ValueError(f"group member {k} is a group or a closed engine")
            if e._lib is not lib:
                raise ValueError(f"group member {k} runs another library than member 0 (its drift differs): group engines of one library only")
            if e.device != dev:
                raise ValueError(f"group member {k} is on device {e.device}, member 0 on {dev}")
        self._lib = lib
        self.user_drift = engines[0].user_drift
        self.device = dev
        self.members = engines
        self._h = None
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        out = C.c_void_p()
        rc = lib.magi_group_create(arr, len(engines), C.byref(out))
        if rc != 0:
            raise MagiHipError(rc, lib.magi_last_error(None).decode())
        self._h = out.value
        self.N, self.D, self.P = engines[0].N, engines[0].D, engines[0].P
        self._n_obs = engines[0]._n_obs
        self.n_chains = 0
        self._cfg = None
