"""Self-test of a freshly built library before its first use.

A library that magi_v2_amd.jit compiles for a traced f_vec is a binary no test has ever seen: its own generated header, its own register
allocation.  ``run`` checks such a file (or the base library) against itself and against the expressions it was generated from, with no
oracle and no file input:

* ``drift.f`` / ``drift.jt`` / ``drift.runtime`` / ``drift.sep``: the device drift code by itself (magi_drift_probe, csrc/selftest.hip) against the
  host evaluators ``f_np`` / ``jac_np`` of the same trace;
* ``families``: the reference-order three-phase log posterior and gradient against the sampler's single-phase form in every streaming
  kernel family the drift and shape can run;
* ``gradient``: the analytic gradient against central differences of the log posterior's own values;
* ``sampler``: short fixed-L HMC and NUTS runs whose reported ``target_log_prob`` is recomputed at the returned states.

It is a consistency check of the binary, not parity with the reference (that is what tests/ and oracle/ do for the base library and the
example drifts).  ``ensure`` remembers the verdict beside the library (``<library>.selftest.json``) and refuses a library that failed;
MagiEngine calls it for every drift-specialised library before the first handle.

    python -m magi_v2_amd.selftest [--lib PATH] [--drift NAME] [--device K] [--force]
"""
from __future__ import annotations

import fcntl
import hashlib
import json
import logging
import os
import sys
import time
from dataclasses import asdict, dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

VERSION = 1                     # part of a cached verdict's key: raise it when a check, a tolerance or the synthetic problem changes
N_GRID = 161                    # two operator blocks of 128 points
N_PROBE = 256
TOL_DRIFT = (1e-12, 1e-14)      # relative to the largest magnitude of the point's output vector, + absolute (drift.resolve's pair)
TOL_FAMILIES = 1e-9             # tests/test_fused_gpu.py
TOL_GRADIENT = (1e-4, 1e-6)     # tests/test_fullsize_gpu.py: |fd - an| <= 1e-4 max(|an|, |fd|) + 1e-6, h = 1e-4
TOL_SAMPLER = 1e-9
# The sampler check's first step sizes.  Dual averaging cannot be switched off: with num_adaptation_steps = 0 the first transition runs at
# the configured step and every later one at the averaged step, 10 e^0.45 = 15.7 x as large after an accepted first transition.  At
# N = 161 (dense) C^-1 has entries of 1e7, so leapfrog is stable below about 6e-4: 1.25e-5 puts the later transitions at 2e-4.  The check
# walks down this ladder until every chain accepts a kept transition.
STEP_SIZES = tuple(1.25e-5 / 8 ** k for k in range(5))
_log = logging.getLogger(__name__)


class MagiSelfTestError(RuntimeError):
    """The library failed its self-test; ``report`` holds the numbers."""

    def __init__(self, report: "Report"):
        super().__init__(report.failure_message())
        self.report = report


@dataclass
class Check:
    name: str
    drift: str
    worst: float                # worst observed error, in the units of `tol`
    tol: float
    ok: bool
    seconds: float
    detail: str = ""
    by_path: Dict[str, float] = field(default_factory=dict)


@dataclass
class Report:
    library: str
    sha256: str
    version: str                # magi_version()
    device: str
    selftest_version: int
    drifts: List[str]
    checks: List[Check]
    seconds: float = 0.0
    cached: bool = False

    @property
    def ok(self) -> bool:
        return bool(self.checks) and all(c.ok for c in self.checks)

    def failed(self) -> List[Check]:
        return [c for c in self.checks if not c.ok]

    def failure_message(self) -> str:
        bad = "; ".join(f"{c.name} [{c.drift}] worst {c.worst:.3e} > tolerance {c.tol:.1e}" + (f" ({c.detail})" if c.detail else "") for c in self.failed())
        return (f"self-test of {self.library} failed: {bad or 'no check ran'}.  The library is not used (MAGI_SELFTEST=0 skips the self-test, "
                "MAGI_SELFTEST=force runs it again)")

    def format(self) -> str:
        lines = [f"self-test v{self.selftest_version} of {self.library}" + ("  (cached)" if self.cached else ""),
                 f"  sha256 {self.sha256}", f"  {self.version} on {self.device}; drifts: {', '.join(self.drifts)}",
                 "  %-14s %-16s %12s %10s %8s  %s" % ("check", "drift", "worst", "tolerance", "seconds", "")]
        for c in self.checks:
            lines.append("  %-14s %-16s %12.3e %10.1e %8.3f  %s%s" % (c.name, c.drift, c.worst, c.tol, c.seconds, "ok" if c.ok else "FAILED",
                                                                      f"  {c.detail}" if c.detail else ""))
        lines.append(f"  {'PASSED' if self.ok else 'FAILED'} in {self.seconds:.2f} s")
        return "\n".join(lines)

    def to_json(self) -> dict:
        d = asdict(self)
        d.pop("cached")
        return d

    @staticmethod
    def from_json(d: dict, cached: bool = True) -> "Report":
        d = dict(d)
        d["checks"] = [Check(**c) for c in d["checks"]]
        return Report(cached=cached, **d)


# ------------------------------------------------------------------------------------------------
# the synthetic problem
# ------------------------------------------------------------------------------------------------


def synthetic_problem(D: int, P: int) -> Dict[str, np.ndarray]:
    """The problem every self-test runs on; a function of the drift's shape alone, every random number from one fixed-seed generator.

    Uniform grid of N_GRID = 161 points with spacing 0.025 (two operator blocks), every second point observed in every component.  States
    are smooth and positive, inside the box drift.resolve probes with -- X in (0.05, 0.6), theta in (0.2, 2.0): one sine per component
    (amplitude 0.2 around 0.325, 0.5 .. 1.5 periods over the grid) plus 0.01 N(0, 1) at the three test states.  It is NOT a solution of the
    ODE (the drift is arbitrary): the drift term of the posterior is large, which suits a check of drift code.  Hyper-parameters are
    fixed: phi1 = var(X_d), phi2 = 0.6, sigma^2 = (0.1 sd)^2, nu = 2.01, dense matrices (built by the library under test)."""
    rng = np.random.default_rng(161)
    N = N_GRID
    I = np.arange(N) * 0.025
    u = np.arange(N) / (N - 1.0)
    periods, phase = rng.uniform(0.5, 1.5, D), rng.uniform(0.0, 1.0, D)
    X = 0.325 + 0.2 * np.sin(2.0 * np.pi * (u[:, None] * periods[None] + phase[None]))
    theta = rng.uniform(0.3, 1.8, P)
    sd = X.std(axis=0)
    rows = np.arange(0, N, 2)
    obs_idx = (rows[:, None] * D + np.arange(D)[None]).reshape(-1).astype(np.int64)
    y = X.reshape(-1)[obs_idx] + 0.01 * rng.standard_normal(obs_idx.shape[0])
    N_ds = np.full(D, float(len(rows)))
    LB = (0.01 * sd) ** 2
    sig2 = (0.1 * sd) ** 2
    sp0 = np.log(np.expm1(sig2 - LB))
    tp0 = np.log(np.expm1(theta))
    n_states, n_dirs = 3, 4
    pr = {"I": I, "phi1s": sd ** 2, "phi2s": np.full(D, 0.6), "nu": np.float64(2.01), "mu": X.mean(axis=0), "N_ds": N_ds, "obs_idx": obs_idx,
          "y": y, "beta": np.float64(D * N / N_ds.sum()), "LB": LB, "X0": X, "sp0": sp0, "tp0": tp0,
          "state_X": X[None] + 0.01 * rng.standard_normal((n_states, N, D)),
          "state_sp": sp0[None] + 0.3 * rng.standard_normal((n_states, D)),
          "state_tp": np.log(np.expm1(rng.uniform(0.3, 1.8, (n_states, P)))),
          # direction scales of tests/test_fullsize_gpu.py
          "dir_X": 1e-3 * rng.standard_normal((n_dirs, N, D)), "dir_sp": 1e-2 * rng.standard_normal((n_dirs, D)),
          "dir_tp": 1e-2 * rng.standard_normal((n_dirs, P)),
          "probe_X": rng.uniform(0.05, 0.6, (N_PROBE, D)), "probe_th": rng.uniform(0.2, 2.0, P), "probe_g": rng.standard_normal((N_PROBE, D))}
    return pr


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------


def _normalised_error(got: np.ndarray, want: np.ndarray) -> float:
    """max over points of |got - want| / (rel * max_j |want_j| + abs) * rel: the error in units where the tolerance is TOL_DRIFT[0]."""
    rel, ab = TOL_DRIFT
    if not np.isfinite(got).all():
        return float("inf")
    scale = rel * np.abs(want).max(axis=1, keepdims=True) + ab
    return float((np.abs(got - want) / scale).max() * rel)


def _check_drift(eng, drift, pr) -> List[Check]:
    """magi_drift_probe against the host evaluators of the trace the header was printed from; a drift that uses t is probed at N_PROBE
    random times inside the synthetic grid's range (magi_drift_probe_at), any other exactly as before."""
    from .engine import MagiHipError
    X, th, g = pr["probe_X"], pr["probe_th"], pr["probe_g"]
    tt = probe_times(pr) if getattr(drift, "time_dependent", False) else None
    f_want = np.asarray(drift.f_np(tt, X, th), dtype=np.float64)
    J, T = drift.jac_np(X, th, tt)
    c_want = np.einsum("nd,ndk->nk", g, J)
    t_want = np.einsum("nd,ndp->np", g, T)
    out = []

    def one(name, parts):
        t0 = time.perf_counter()
        by, detail = {}, ""
        try:
            for label, path, wants in parts:
                got = eng.drift_probe(drift, X, th, g, path, t=tt)
                for what, a, b in zip(("f", "c", "t"), got, wants):
                    if b is not None:
                        by[f"{label}.{what}"] = _normalised_error(a, b)
        except MagiHipError as e:
            by["error"], detail = float("inf"), str(e)
        worst = max(by.values())
        out.append(Check(name, drift.name, worst, TOL_DRIFT[0], bool(worst <= TOL_DRIFT[0]), time.perf_counter() - t0, detail, by))

    one("drift.f", [("path0", 0, (f_want, None, None)), ("path3", 3, (f_want, None, None))])
    one("drift.jt", [("path0", 0, (None, c_want, t_want))])
    one("drift.runtime", [("path1", 1, (f_want, c_want, t_want))])
    if _separable(drift):          # (a library that disagrees answers MAGI_E_BADARG: the check fails)
        one("drift.sep", [("path2", 2, (f_want, None, None))])
    return out


def probe_times(pr) -> np.ndarray:
    """The times a time-dependent drift is probed at: N_PROBE draws from the range of the synthetic grid, a generator of their own (the
    synthetic problem of every other library stays what it was)."""
    return np.random.default_rng(162).uniform(pr["I"][0], pr["I"][-1], N_PROBE)


def _separable(drift) -> bool:
    """Whether the drift's code carries the separable members (all compiled-in drifts do; a traced drift's header says)."""
    return drift.header is None or "static constexpr bool SEP = true;" in drift.header


def _rel(a, b) -> float:
    """max-norm error of a against b relative to b's max norm (a scalar: relative error)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.isfinite(a).all():
        return float("inf")
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max())


# (chains in the batch, option stream_family): k_stream<1>, k_stream<2>, the matrix-core kernel (k_stream_sep / k_stream_mc)
FAMILIES = ((1, "auto"), (2, "auto"), (5, "mc"))


def _engine(lib_path, device, drift, pr, family="auto"):
    from .engine import MagiEngine
    eng = MagiEngine(device, drift=drift, _library=lib_path)
    try:
        eng.set_option("stream_family", family)
        eng.build_matrices(pr["I"], pr["phi1s"], pr["phi2s"], float(pr["nu"]), bandsize=None, want_host=False)
        if getattr(drift, "time_dependent", False):        # the synthetic grid is the times the drift is evaluated at
            eng.set_times(pr["I"])
        eng.set_problem(pr["mu"], pr["N_ds"], pr["obs_idx"], pr["y"], float(pr["beta"]), pr["LB"], drift)
    except Exception:
        eng.close()
        raise
    return eng


def _check_families(engines, drift, pr, ref) -> Check:
    t0 = time.perf_counter()
    worst, seen = 0.0, []
    S = pr["state_X"].shape[0]
    for (n, fam), eng in zip(FAMILIES, engines):
        seen.append(eng.stream_kernel_name(n))
        batches = [[s] for s in range(S)] if n == 1 else [[(b + k) % S for k in range(n)] for b in range(0, S, n)]
        for parity in (0, 1):
            eng.set_option("fused_parity", parity)
            for idx in batches:
                got = eng.logpost_grad(pr["state_X"][idx], pr["state_sp"][idx], pr["state_tp"][idx], 1.0, fused=True)
                for k, s in enumerate(idx):
                    worst = max([worst] + [_rel(got[j][k], ref[s][j]) for j in range(4)])
        eng.set_option("fused_parity", 0)
    return Check("families", drift.name, worst, TOL_FAMILIES, bool(worst <= TOL_FAMILIES), time.perf_counter() - t0, " ".join(seen))


def _check_gradient(eng, drift, pr, ref) -> Check:
    t0 = time.perf_counter()
    rel, ab = TOL_GRADIENT
    h, worst = 1e-4, 0.0
    X, sp, tp = pr["state_X"][0], pr["state_sp"][0], pr["state_tp"][0]
    _, gX, gs, gt = ref[0]
    for vX, vs, vt in zip(pr["dir_X"], pr["dir_sp"], pr["dir_tp"]):
        lp_p = eng.logpost_grad(X + h * vX, sp + h * vs, tp + h * vt, 1.0)[0]
        lp_m = eng.logpost_grad(X - h * vX, sp - h * vs, tp - h * vt, 1.0)[0]
        fd = (lp_p - lp_m) / (2 * h)
        an = float((gX * vX).sum() + gs @ vs + gt @ vt)
        bound = rel * max(abs(an), abs(fd)) + ab
        err = abs(fd - an) / bound * rel if np.isfinite(fd) and np.isfinite(an) else float("inf")
        worst = max(worst, err)                                        # (in units where the bound is `rel`)
    return Check("gradient", drift.name, worst, rel, bool(worst <= rel), time.perf_counter() - t0)


def _check_sampler(engines, ref_eng, drift, pr) -> Check:
    """Fixed-L HMC and NUTS, anneal = 0, stale_cache = 0: every kept state's reported target_log_prob against the three-phase log posterior
    at that state; everything finite; every chain accepts at least one of its kept transitions (the step size walks down STEP_SIZES until it does)."""
    from .engine import MagiHipError
    t0 = time.perf_counter()
    worst, notes = 0.0, []
    burnin, results = 2, 4
    rep = lambda v, n: np.repeat(np.asarray(v)[None], n, axis=0)
    try:
        for (n, fam), eng in zip(FAMILIES, engines):
            for mode, name in ((1, "hmc"), (0, "nuts")):
                accepted = False
                for eps in STEP_SIZES:
                    cfg = eng.default_cfg(num_results=results, num_burnin_steps=burnin, num_adaptation_steps=0, mode=mode, hmc_leapfrogs=4,
                                          max_tree_depth=3, anneal=0, stale_cache=0, step_size=eps)
                    eng.sampler_init(cfg, rep(pr["X0"], n), rep(pr["sp0"], n), rep(pr["tp0"], n), seed=161, chain_ids=list(range(n)))
                    eng.sampler_run(burnin + results)
                    d = eng.sampler_diag()
                    if (d.is_accepted[:, burnin:].sum(axis=1) >= 1).all():        # (asks more than one accepted transition per run: one among the kept)
                        accepted = True
                        break
                if not accepted:
                    worst = float("inf")
                    notes.append(f"{name} x{n}: a chain accepted nothing down to step size {STEP_SIZES[-1]:.1e}")
                    continue
                Xs, sps, tps = eng.sampler_samples()
                finite = all(np.isfinite(a).all() for a in (Xs, sps, tps, d.target_log_prob, d.step_size))
                if not finite:
                    worst = float("inf")
                    notes.append(f"{name} x{n}: non-finite output")
                    continue
                lp = ref_eng.logpost_grad(Xs.reshape((n * results,) + Xs.shape[2:]), sps.reshape(n * results, -1), tps.reshape(n * results, -1), 1.0)[0]
                tlp = d.target_log_prob[:, burnin:].reshape(-1)
                worst = max(worst, float(np.max(np.abs(tlp - lp) / np.abs(lp))))
                notes.append(f"{name} x{n} step {d.step_size[:, -1].max():.1e} acc {int(d.is_accepted.sum())}/{n * (burnin + results)}")
    except MagiHipError as e:
        worst = float("inf")
        notes.append(str(e))
    return Check("sampler", drift.name, worst, TOL_SAMPLER, bool(worst <= TOL_SAMPLER), time.perf_counter() - t0, "; ".join(notes))


# ------------------------------------------------------------------------------------------------
# run / ensure
# ------------------------------------------------------------------------------------------------


def _resolve_drifts(lib, drift):
    """The Drift objects a self-test of this library covers: the traced drift it was built for, or built-ins (all three by default)."""
    from . import drift as _drift
    from .engine import DRIFT_SHAPES
    user = bool(lib.magi_user_drift_info(None, None))
    if user:
        if drift is None or isinstance(drift, str) or drift.is_builtin:
            raise ValueError("this library is specialised for a traced f_vec: pass its Drift (the host evaluators are the truth of the self-test)")
        return [drift]
    if drift is None:
        return [_drift.builtin_drift(n) for n in DRIFT_SHAPES]
    if isinstance(drift, str):
        return [_drift.builtin_drift(drift)]
    if not drift.is_builtin:
        raise ValueError("the base library carries the compiled-in drifts only")
    return [drift]


def file_sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def device_name(lib, device: int) -> str:
    """Identity of HIP device `device` for a verdict's key: its name and memory size (hipDeviceGetName, hipDeviceTotalMem, resolved through
    the library's own dependency on the HIP runtime; a box without the amdgpu id table reports an empty name)."""
    import ctypes as C
    buf, mem = C.create_string_buffer(256), C.c_size_t(0)
    fn, tm = lib.hipDeviceGetName, lib.hipDeviceTotalMem
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.c_int, C.c_int]
    tm.restype, tm.argtypes = C.c_int, [C.POINTER(C.c_size_t), C.c_int]
    if fn(buf, 256, int(device)) != 0 or tm(C.byref(mem), int(device)) != 0:
        return "unknown"
    return "%s (%d GiB)" % (buf.value.decode(errors="replace") or "HIP device", mem.value >> 30)


def run(lib_path: Optional[str] = None, drift=None, device: int = 0, raise_on_failure: bool = True) -> Report:
    """Self-test the library file `lib_path` (default: the base library) on handles of its own.  ``drift``: the traced Drift a specialised
    library was built for; a built-in name / Drift, or None = all three, for the base library.  Starts no process, sets no environment
    variable, leaves no handle behind.  Raises MagiSelfTestError on failure unless ``raise_on_failure`` is False."""
    from . import engine
    t_all = time.perf_counter()
    path = os.path.abspath(lib_path or engine.LIB_PATH)
    lib = engine.load_library(path)
    drifts = _resolve_drifts(lib, drift)
    checks: List[Check] = []
    for d in drifts:
        pr = synthetic_problem(d.D, d.P)
        engines = []
        try:
            for n, fam in FAMILIES:
                engines.append(_engine(path, device, d, pr, fam))
            ref_eng = engines[0]
            checks += _check_drift(ref_eng, d, pr)
            ref = [ref_eng.logpost_grad(pr["state_X"][s], pr["state_sp"][s], pr["state_tp"][s], 1.0) for s in range(pr["state_X"].shape[0])]
            checks.append(_check_families(engines, d, pr, ref))
            checks.append(_check_gradient(ref_eng, d, pr, ref))
            checks.append(_check_sampler(engines, ref_eng, d, pr))
        finally:                                           # (no handle, no matrices: MagiHipError, not a verdict on the library)
            for e in engines:
                e.close()
    rep = Report(library=path, sha256=file_sha256(path), version=lib.magi_version().decode(), device=device_name(lib, device),
                 selftest_version=VERSION, drifts=[d.name for d in drifts], checks=checks, seconds=time.perf_counter() - t_all)
    if raise_on_failure and not rep.ok:
        raise MagiSelfTestError(rep)
    return rep


_memory: Dict[tuple, Report] = {}       # verdicts of this process (all of them; the only store when the library's directory is read-only)
_skip_logged = False


def verdict_path(lib_path: str) -> str:
    return os.path.abspath(lib_path) + ".selftest.json"


def _load_verdict(path: str, key: dict) -> Optional[Report]:
    try:
        with open(path) as fh:
            d = json.load(fh)
        rep = Report.from_json(d)
    except (OSError, ValueError, TypeError, KeyError):
        return None
    if (rep.sha256, rep.device, rep.selftest_version) != (key["sha256"], key["device"], key["selftest_version"]) or not set(key["drifts"]) <= set(rep.drifts):
        return None
    return rep


def ensure(lib_path: str, drift=None, device: int = 0, force: bool = False, runner: Optional[Callable] = None, get_device_name: Optional[Callable] = None) -> Optional[Report]:
    """The verdict on `lib_path` for (its bytes, this device, this self-test version): from this process's memory, from
    ``<library>.selftest.json``, or by running the self-test once -- under an exclusive ``flock`` beside the library, so that the ranks of
    a job or the workers of a test run do not all run it; the verdict is written with one ``os.replace``.  A failing verdict is kept and
    keeps raising MagiSelfTestError.  MAGI_SELFTEST=0 skips everything (returns None), MAGI_SELFTEST=force ignores stored verdicts.
    ``runner(lib_path, drift, device) -> Report`` and ``get_device_name(device) -> str`` are seams for the tests."""
    global _skip_logged
    mode = os.environ.get("MAGI_SELFTEST", "")
    if mode == "0":
        if not _skip_logged:
            _log.warning("MAGI_SELFTEST=0: libraries are used without their self-test")
            _skip_logged = True
        return None
    force = force or mode == "force"
    path = os.path.abspath(lib_path)
    if runner is None:
        runner = lambda p, d, dev: run(p, d, dev, raise_on_failure=False)
    if get_device_name is None:
        from . import engine
        get_device_name = lambda dev: device_name(engine.load_library(path), dev)
    if drift is None:                                      # (the base library: all compiled-in drifts)
        from .engine import DRIFT_SHAPES
        names = sorted(DRIFT_SHAPES)
    else:
        names = [drift] if isinstance(drift, str) else [drift.name]
    key = {"sha256": file_sha256(path), "device": get_device_name(device), "selftest_version": VERSION, "drifts": names}
    mkey = (path, key["sha256"], key["device"], VERSION, tuple(names))
    rep = None if force else _memory.get(mkey)
    vpath = verdict_path(path)
    if rep is None and not force:
        rep = _load_verdict(vpath, key)
    if rep is None:
        try:
            lock = open(path + ".selftest.lock", "w")
        except OSError:                                    # a prebuilt, read-only cache: once per process, verdict in memory only
            rep = runner(path, drift, device)
        else:
            with lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    rep = None if force else _load_verdict(vpath, key)            # another process ran it while we waited
                    if rep is None:
                        rep = runner(path, drift, device)
                        tmp = f"{vpath}.{os.getpid()}.tmp"
                        try:
                            with open(tmp, "w") as fh:
                                json.dump(rep.to_json(), fh, indent=1)
                            os.replace(tmp, vpath)
                        except OSError:
                            pass
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    _memory[mkey] = rep
    if not rep.ok:
        raise MagiSelfTestError(rep)
    return rep


def main(argv=None, runner: Optional[Callable] = None, get_device_name: Optional[Callable] = None) -> int:
    import argparse
    from . import engine
    ap = argparse.ArgumentParser(prog="python -m magi_v2_amd.selftest", description="self-test a libmagi_hip build (default: the base library, all compiled-in drifts)")
    ap.add_argument("--lib", help="library file (default: the base library, or the drift-specialised library of --drift)")
    ap.add_argument("--drift", help="a compiled-in drift (%s) or an example drift of magi_v2_amd.drift_examples" % ", ".join(sorted(engine.DRIFT_SHAPES)))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--force", action="store_true", help="run even when a verdict is stored")
    a = ap.parse_args(argv)
    drift, lib = a.drift, a.lib
    if drift is not None and drift not in engine.DRIFT_SHAPES:
        from . import drift as _drift, drift_examples, jit
        if drift not in drift_examples.EXAMPLES:
            ap.error(f"unknown drift {drift!r}")
        drift = _drift.resolve(*drift_examples.EXAMPLES[drift])
        lib = lib or jit.library_for(drift)
    try:
        rep = ensure(lib or engine.LIB_PATH, drift, a.device, force=a.force, runner=runner, get_device_name=get_device_name)
    except MagiSelfTestError as e:
        print(e.report.format())
        print(str(e), file=sys.stderr)
        return 1
    if rep is None:
        print("MAGI_SELFTEST=0: nothing was tested")
        return 0
    print(rep.format())
    return 0


if __name__ == "__main__":
    sys.exit(main())
