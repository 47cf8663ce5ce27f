"""Case tables and reference of tests/test_reuse_model_cpu.py and tests/test_reuse_model_gpu.py: one handle through every change of MODEL state.

tests/test_reuse_gpu.py walks a handle through matrices, bands, problem data, times, batches and kernel families.  Since then the handle has
gained the diagonal metric (d_scale / d_macc / d_mwork), the supports of theta (dTsup, th_kind, th_bound), the priors (dPrior, fixed_mask, an
LB entry REPLACED by a fixed variance and restored from lb_orig), the observation model (dYobs rewritten in place with g(y), dObsw,
obs_links) and the post-processing calls on the handle's stream.  The states here cross them.  Everything in this file is CPU-only.

Base problems
  B129   tests/util.structureless_problem(129, "sirw", spd=True): D = 4, P = 5, states in (0.05, 0.3) -- both links are defined --, two block
         rows (dYobs, dObsw and the padded tail 129 .. 256 cross a tile boundary), every operator block counts; used dense and at band 20.
         "B129v": the same data on the matrices of another seed (same shape, other values); "B129-": every third observation dropped
         (another n_obs).
  B41    the golden sirw_N41 matrices (D = 4) with the sirw problem (P = 5) or the seir4 problem (P = 3: the state size changes on one
         set of matrices); "B41v": C^-1 x 0.97 and K^-1 x 1.05.  Its components 1 .. 3 touch 0, so only component 0 carries a link there.

Models (MODELS; theta entries for P = 5 / P = 3)
  M0  none
  M1  supports positive, real, lower, upper (, positive); lognormal and normal priors on theta; gamma and inverse-gamma priors on sigma^2
  M2  M1 + one variance fixed, log and sqrt links, weights in (0.25, 4) on a random half of the observations
  M3  other links, other weights, ANOTHER fixed component (the earlier one gets its LB back), the bounds moved, theta_0 real
  M4  weights only

A Stop is (base, band, drift, model); stop_state builds its ModelState -- a tests/util.ReuseState (masked oracle problem, unmasked matrices,
band, a batch of nine pre-transformed states) plus the model's tables as obs_reference.logpost_grad_obs takes them.  HISTORIES lists the
stops of every history of the GPU file in order: the CPU file proves on the reference alone that a handle which answered for the stop
before would be seen."""
import dataclasses

import numpy as np

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import obs_reference as O
from tests.util import REUSE_HMC, ReuseState, reuse_state, structureless_states

TEMP = 0.8
BAND = 20
MAX_BATCH = 9
# trees of depth <= 5, 7 and 5 transitions per run; four kept draws: split R-hat and the ESS of sampler_summary are defined (R >= 4)
NUTS = dict(num_burnin_steps=3, num_results=4, step_size=2e-3, max_tree_depth=5, stale_cache=0)
HMC = dict(REUSE_HMC)
SEED = 808
PAIR = ((1, "auto"), (5, "mc"))          # k_stream<1>; five states on k_stream_sep<CW=8>
THETA_SEIR4 = np.array([6.0, 0.6, 1.8])

_SIG_M1 = [("gamma", 2.0, 10.0), ("invgamma", 3.0, 0.1), None, None]
_TH5_M1 = [("lognormal", 0.5, 1.0), ("normal", 0.0, 2.0), ("lognormal", -1.0, 1.5), ("normal", 1.5, 1.0), ("gamma", 2.0, 4.0)]
_TH3_M1 = [("lognormal", 1.5, 1.0), ("normal", 0.0, 2.0), ("normal", 1.5, 1.0)]
_SUP5_M1 = ["positive", "real", ("lower", 0.1), ("upper", 3.0), "positive"]
_SUP3_M1 = [("lower", 1.0), "real", ("upper", 4.0)]
# model -> support {P: spec}, theta prior {P: spec}, sigma^2 prior, links {base kind: spec}, the seed of its weights (None: no weights)
MODELS = {
    "M0": dict(support=None, th_prior=None, sig_prior=None, links=None, weights=None),
    "M1": dict(support={5: _SUP5_M1, 3: _SUP3_M1}, th_prior={5: _TH5_M1, 3: _TH3_M1}, sig_prior=_SIG_M1, links=None, weights=None),
    "M2": dict(support={5: _SUP5_M1, 3: _SUP3_M1}, th_prior={5: _TH5_M1, 3: _TH3_M1}, sig_prior=_SIG_M1[:2] + [("fixed", 0.04), None],
               links={"B129": ("log", "identity", "sqrt", "log"), "B41": ("log", None, None, None)}, weights=1),
    "M3": dict(support={5: ["real", "real", ("lower", 0.05), ("upper", 2.5), "positive"], 3: ["real", "real", ("upper", 5.0)]},
               th_prior={5: [("normal", 1.0, 3.0), None, ("lognormal", -1.0, 1.5), ("normal", 1.0, 1.0), ("gamma", 2.0, 4.0)],
                         3: [("normal", 5.0, 3.0), None, ("normal", 1.5, 1.0)]},
               sig_prior=[("fixed", 0.06), ("invgamma", 3.0, 0.1), None, ("gamma", 2.0, 10.0)],
               links={"B129": ("sqrt", "log", "identity", "sqrt"), "B41": ("sqrt", None, None, None)}, weights=2),
    "M4": dict(support=None, th_prior=None, sig_prior=None, links=None, weights=3),
}


@dataclasses.dataclass(frozen=True)
class Stop:
    base: str
    band: object
    drift: str
    model: str

    @property
    def name(self):
        return f"{self.base}/{'dense' if self.band is None else 'b%d' % self.band}/{self.drift}/{self.model}"


def _walk(base, band, drift, models):
    return [Stop(base, band, drift, m) for m in models]


WALK = ("M0", "M1", "M2", "M3", "M4", "M0", "M2")
HISTORIES = {
    "1 model walk": _walk("B129", BAND, "sirw", WALK),
    # other matrices of the same shape under M2 (set_matrices forgets the problem, pack_resident keeps it and the model), the shape changed
    # and back (the model is reset), M2 under another n_obs
    "2 matrices under a model": [Stop("B129", None, "sirw", "M2"), Stop("B129v", None, "sirw", "M2"), Stop("B129v", BAND, "sirw", "M2"),
                                 Stop("B129v", None, "sirw", "M2"), Stop("B41", None, "sirw", "M0"), Stop("B129", None, "sirw", "M0"),
                                 Stop("B129-", None, "sirw", "M2")],
    "3 P under a model": [Stop("B41", None, "sirw", "M1"), Stop("B41", None, "seir4", "M0"), Stop("B41", None, "seir4", "M1"),
                          Stop("B41", None, "sirw", "M0")],
    "6 group member 0": [Stop("B41", None, "sirw", "M2"), Stop("B41", None, "sirw", "M3")],
    "6 group member 1": [Stop("B41", None, "sirw", "M0"), Stop("B41v", None, "sirw", "M0")],
}
# (history 4 changes the metric, not the target: METRIC_* below; history 5 and 7 change nothing a posterior depends on)


class ModelState(ReuseState):
    """A ReuseState under a model: ``spec`` = what the engine's set_theta_support / set_prior / set_obs_model are given (support, sig_prior,
    th_prior, link, weight), ``tables`` = the same normalised (kinds, bounds, sig_prior, th_prior, links; each None when the model has
    none): what obs_reference.logpost_grad_obs takes and what the engine's getters return."""

    def __init__(self, stop, pr, matrices, batch, spec, tables, extra=None):
        super().__init__(stop.name, pr, matrices, stop.band, batch)
        self.stop, self.spec, self.tables, self.extra = stop, spec, tables, extra or {}

    def reference(self, long=False):
        t = self.tables
        return O.logpost_grad_obs(t["links"], self.spec["weight"], t["sig_prior"], t["th_prior"], t["kinds"], t["bounds"], long=long)


_bases, _states = {}, {}


def _fewer_observations(pr):
    keep = np.arange(len(pr.obs_idx)) % 3 != 2
    idx = pr.obs_idx[keep]
    N_ds = np.bincount(idx % pr.D, minlength=pr.D).astype(np.float64)
    return dataclasses.replace(pr, obs_idx=idx, y=pr.y[keep], N_ds=N_ds)


def base_problem(base, drift):
    """(unmasked orc.Problem, batch of MAX_BATCH states, extra) of a base problem under a drift; once per session, read-only."""
    key = (base, drift)
    if key in _bases:
        return _bases[key]
    if base.startswith("B129"):
        from tests.test_structureless_cpu import fixture
        assert drift == "sirw"
        pr, X = fixture(129, "sirw", spd=True)
        batch = structureless_states(pr, X, MAX_BATCH, 0)
        if base == "B129v":
            other, _ = fixture(129, "sirw", spd=True, salt=1)
            pr = dataclasses.replace(pr, C_inv=other.C_inv, m=other.m, K_inv=other.K_inv)
        elif base == "B129-":
            pr = _fewer_observations(pr)
        else:
            assert base == "B129"
        extra = {}
    else:
        c41 = reuse_state("C41")
        pr = c41.pr
        batch = tuple(a[:MAX_BATCH] for a in c41.batch)
        if drift == "seir4":
            pr = dataclasses.replace(pr, drift="seir4", P=3)
            rng = np.random.default_rng(4103)
            batch = (batch[0], batch[1], np.log(np.expm1(THETA_SEIR4))[None] + 0.05 * rng.standard_normal((MAX_BATCH, 3)))
        else:
            assert drift == "sirw"
        if base == "B41v":
            pr = dataclasses.replace(pr, C_inv=0.97 * pr.C_inv, K_inv=1.05 * pr.K_inv)
        else:
            assert base == "B41"
        from tests.util import load_g4
        g = load_g4("sirw_N41")
        extra = {k: np.asarray(g[k], dtype=np.float64) for k in ("I", "phi1s", "phi2s", "Xhat_init")}
        extra["I"] = extra["I"].reshape(-1)
    _bases[key] = (pr, batch, extra)
    return _bases[key]


def model_spec(model, base, pr):
    """What the engine is given for a model on a problem: dict(support, sig_prior, th_prior, link, weight)."""
    m = MODELS[model]
    pick = lambda table: None if table is None else table[pr.P]
    link = None if m["links"] is None else m["links"]["B129" if base.startswith("B129") else "B41"]
    weight = None if m["weights"] is None else O.draw_weights(len(pr.obs_idx), 7000 + m["weights"])
    return dict(support=pick(m["support"]), sig_prior=m["sig_prior"], th_prior=pick(m["th_prior"]), link=link, weight=weight)


def model_tables(spec, pr):
    sup = host.theta_support(spec["support"], pr.P)
    return dict(kinds=None if spec["support"] is None else sup[0], bounds=None if spec["support"] is None else sup[1],
                sig_prior=None if spec["sig_prior"] is None else host.prior_spec(spec["sig_prior"], pr.D, "sigma_sq"),
                th_prior=None if spec["th_prior"] is None else host.prior_spec(spec["th_prior"], pr.P, "theta", sup),
                links=None if spec["link"] is None else host.obs_model_spec(spec["link"], pr.D))


def stop_state(stop):
    """The ModelState of a Stop; once per session, read-only."""
    if stop not in _states:
        dense, batch, extra = base_problem(stop.base, stop.drift)
        pr = dense if stop.band is None else dataclasses.replace(dense, C_inv=orc.band_part(dense.C_inv, stop.band), m=orc.band_part(dense.m, stop.band),
                                                                 K_inv=orc.band_part(dense.K_inv, stop.band))
        spec = model_spec(stop.model, stop.base, pr)
        _states[stop] = ModelState(stop, pr, (dense.C_inv, dense.m, dense.K_inv), batch, spec, model_tables(spec, pr), extra)
    return _states[stop]


def prior_allowed(th_prior_spec, support_spec, P):
    """Whether the library accepts the theta priors under the supports (a lognormal, gamma or inverse-gamma prior needs a support inside
    (0, inf)): host.prior_spec restates magi_set_prior's rule."""
    try:
        host.prior_spec(th_prior_spec, P, "theta", host.theta_support(support_spec, P))
        return True
    except ValueError:
        return False


# ---- history 4: the metrics -------------------------------------------------------------------------------------------------------------

def metric_arrays(tag, n, N, D, P):
    """(inv_mass_X [n, N, D], inv_mass_sig [n, D], inv_mass_th [n, P]) of metric ``tag``: inverse masses log-uniform in [0.5, 2]^2, another
    draw per chain."""
    rng = np.random.default_rng([sum(map(ord, tag)), 4711])
    draw = lambda *shape: np.exp(rng.uniform(2.0 * np.log(0.5), 2.0 * np.log(2.0), shape))
    return draw(n, N, D), draw(n, D), draw(n, P)


# ---- history 5: what the header says about each call between two magi_sampler_run calls --------------------------------------------------

# call -> "continues" (the continued run is the uninterrupted one bit for bit) or "refused" (the next magi_sampler_run returns MAGI_E_STATE)
PAUSE_CALLS = {"summarize": "continues", "elpd": "continues", "gp_predict": "continues", "matern_cross": "continues", "ode_solve_rk4": "continues",
               "ode_solve_adaptive": "continues", "dense_apply": "continues", "theta_init": "continues", "fit_hparams": "continues"}
# the C names of those calls as include/magi_hip.h lists them in its paragraph on paused runs
PAUSE_HEADER_NAMES = ("magi_summarize", "magi_elpd", "magi_gp_predict", "magi_matern_cross", "magi_ode_solve", "magi_ode_solve_adaptive",
                      "magi_dense_apply", "magi_theta_init", "magi_fit_hparams")
