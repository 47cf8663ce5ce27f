"""What keeps tests/test_reuse_model_gpu.py honest, on the reference alone (case tables: tests/reuse_model_reference.py).

That file moves ONE handle through supports, priors, observation models, matrices under a model, P under a model and metrics, and holds it
to a fresh handle bit for bit; a handle that answered for the stop BEFORE a transition (a table pointer, an LB entry, a transformed datum,
a weight plane, a graph left over) must therefore differ from the fresh one.  Here, mirroring tests/test_reuse_cpu.py:

  * for every pair of consecutive stops of every history the reference's log posterior AND its X-gradient at the later stop differ from the
    earlier stop's, both evaluated at the later stop's inputs, by >= 1e-6 of scale -- 1000 x the loosest bar of the GPU comparisons (1e-9
    fused).  Pairs that differ in N have no common input (asserted as such); pairs that differ in P (sirw <-> seir4 on the B41 matrices) use
    each stop's own theta.  A condition on the fixtures: seeds, bounds and weights are chosen so that it holds; the smallest margin of every
    history is printed;
  * the metrics of history 4: the whitened reference run (tests/metric_reference.py) under the earlier metric parts from the run under the
    later one within the first two transitions;
  * the models are what the histories need (all four supports, both links, a fixed component that MOVES between M2 and M3), and the two orders
    the library refuses are refused by the rule host.prior_spec restates;
  * a short reference run from the states the GPU file starts its chains at is finite under every model: the bit-for-bit comparisons there
    are not NaN against NaN;
  * include/magi_hip.h says what the GPU file asserts: which matrix changes of the same shape keep the model and which forget the problem, and that each call of history 5 may be made
    between two magi_sampler_run calls.

History 7 (direct launches against graph replay) changes nothing a posterior depends on and has no counterpart here."""
import os

import numpy as np
import pytest

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests import metric_reference as M
from tests import reuse_model_reference as R

MARGIN = 1e-6
N_STATES = 5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magi_hip.h")


def _gap(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _pair_margin(prev, nxt):
    """Smallest of (value gap, X-gradient gap) over the first N_STATES inputs of the later stop; None when the shapes differ."""
    if (prev.pr.D, len(prev.pr.I)) != (nxt.pr.D, len(nxt.pr.I)):
        assert prev.batch[0].shape[1:] != nxt.batch[0].shape[1:]
        return None
    X, sp, tp = nxt.states(N_STATES)
    tp_prev = tp if prev.pr.P == nxt.pr.P else prev.states(N_STATES)[2]
    f_old, f_new = prev.reference(), nxt.reference()
    worst = np.inf
    for c in range(N_STATES):
        new = f_new(X[c], sp[c], tp[c], R.TEMP, nxt.pr)
        old = f_old(X[c], sp[c], tp_prev[c], R.TEMP, prev.pr)
        assert np.isfinite(new[0]) and np.isfinite(new[1]).all() and np.isfinite(old[0]) and np.isfinite(old[1]).all()
        worst = min(worst, abs(old[0] - new[0]) / abs(new[0]), _gap(old[1], new[1]))
    return worst


@pytest.mark.parametrize("history", sorted(R.HISTORIES))
def test_a_stale_model_would_be_seen_after_every_transition(history):
    stops = R.HISTORIES[history]
    margins = {}
    for a, b in zip(stops[:-1], stops[1:]):
        m = _pair_margin(R.stop_state(a), R.stop_state(b))
        if m is not None:
            margins[f"{a.name} -> {b.name}"] = m
    print(f"sensitivity of '{history}': smallest margin {min(margins.values()):.3g}", {k: f"{v:.3g}" for k, v in margins.items()})
    assert margins
    for pair, m in margins.items():
        assert m >= MARGIN, (pair, m)


def test_the_states_of_a_batch_are_pairwise_apart_under_a_model():
    """Five states share a batch: a chain that read another chain's tables or operands shows."""
    st = R.stop_state(R.Stop("B129", R.BAND, "sirw", "M2"))
    X, sp, tp = st.states(N_STATES)
    fn = st.reference()
    out = [fn(X[c], sp[c], tp[c], R.TEMP, st.pr) for c in range(N_STATES)]
    worst = min(min(abs(out[a][0] - out[b][0]) / abs(out[b][0]), _gap(out[a][1], out[b][1])) for a in range(N_STATES) for b in range(a))
    print(f"smallest distance of two states of the batch: {worst:.3g}")
    assert worst >= MARGIN


def test_without_a_model_the_reference_is_the_oracle_bit_for_bit():
    for stop in (R.Stop("B129", R.BAND, "sirw", "M0"), R.Stop("B41", None, "seir4", "M0")):
        st = R.stop_state(stop)
        X, sp, tp = st.states(1)
        got, want = st.reference()(X[0], sp[0], tp[0], R.TEMP, st.pr), orc.logpost_grad(X[0], sp[0], tp[0], R.TEMP, st.pr)
        assert got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)


def test_the_models_are_what_the_histories_need():
    m = R.MODELS
    for P in (5, 3):
        kinds = host.theta_support(m["M1"]["support"][P], P)[0]
        assert set(kinds) >= {host.THETA_REAL, host.THETA_LOWER, host.THETA_UPPER}
    assert set(host.theta_support(m["M1"]["support"][5], 5)[0]) == {host.THETA_POSITIVE, host.THETA_REAL, host.THETA_LOWER, host.THETA_UPPER}
    names = lambda spec: {e[0] for e in spec if e is not None}
    assert names(m["M1"]["th_prior"][5]) >= {"normal", "lognormal"} and names(m["M1"]["sig_prior"]) == {"gamma", "invgamma"}
    fixed = lambda model: [d for d, e in enumerate(m[model]["sig_prior"]) if e is not None and e[0] == "fixed"]
    assert fixed("M1") == [] and fixed("M2") == [2] and fixed("M3") == [0]          # M2 -> M3: LB[2] comes back from lb_orig, LB[0] is replaced
    assert set(m["M2"]["links"]["B129"]) == {"log", "sqrt", "identity"} and m["M2"]["links"]["B129"] != m["M3"]["links"]["B129"]
    assert m["M4"]["weights"] is not None and all(m["M4"][k] is None for k in ("support", "th_prior", "sig_prior", "links"))
    for model in ("M2", "M3", "M4"):
        st = R.stop_state(R.Stop("B129", R.BAND, "sirw", model))
        w = st.spec["weight"]
        assert ((w > 0.25) & (w < 4.0)).all() and (w != 1.0).sum() == len(w) // 2
    w2, w3 = (R.stop_state(R.Stop("B129", R.BAND, "sirw", k)).spec["weight"] for k in ("M2", "M3"))
    assert not np.array_equal(w2, w3)
    # another n_obs: the weights of "B129-" are as many as its observations
    a, b = R.stop_state(R.Stop("B129", None, "sirw", "M2")), R.stop_state(R.Stop("B129-", None, "sirw", "M2"))
    assert len(b.pr.obs_idx) < len(a.pr.obs_idx) and len(b.spec["weight"]) == len(b.pr.obs_idx) and b.pr.N_ds.sum() == len(b.pr.obs_idx)
    # both links are defined at every datum and every state of B129; on B41 only component 0 stays away from 0
    for base, comps in (("B129", range(4)), ("B41", (0,))):
        st = R.stop_state(R.Stop(base, None, "sirw", "M2"))
        cols = st.pr.obs_idx % 4
        for d in comps:
            assert st.pr.y[cols == d].min() > 0.0 and st.batch[0][:, :, d].min() > 0.0
    # the orders the library refuses: M2's lognormal prior on theta_0 under M3's real support, M3's support over M2's installed prior
    assert not R.prior_allowed(m["M2"]["th_prior"][5], m["M3"]["support"][5], 5)
    assert R.prior_allowed(m["M3"]["th_prior"][5], m["M2"]["support"][5], 5) and R.prior_allowed(m["M3"]["th_prior"][5], None, 5)
    # every other consecutive pair of the walk can be applied prior-first (obs model, prior, support): no refusal on the way
    for a, b in zip(R.WALK[:-1], R.WALK[1:]):
        sup_a = None if m[a]["support"] is None else m[a]["support"][5]
        th_b = None if m[b]["th_prior"] is None else m[b]["th_prior"][5]
        assert R.prior_allowed(th_b, sup_a, 5), (a, b)


STOPS = sorted({s for h in R.HISTORIES.values() for s in h}, key=lambda s: s.name)


@pytest.mark.parametrize("stop", STOPS, ids=lambda s: s.name)
def test_a_short_reference_run_is_finite_under_every_model(stop):
    """Two NUTS transitions and two fixed-L HMC transitions of chain 20 from the first state of the stop's batch, on the reference: every
    state, energy and target is finite and every transition takes a leapfrog."""
    st = R.stop_state(stop)
    init = tuple(a[0] for a in st.states(1))
    for kw in (dict(max_tree_depth=R.NUTS["max_tree_depth"]), dict(hmc_leapfrogs=R.HMC["hmc_leapfrogs"])):
        with np.errstate(all="ignore"):
            X, sg, th, info, extra = M.sample_chain(st.pr, None, None, None, 1, 1, seed=R.SEED, chain=20, step_size=R.NUTS["step_size"], stale_cache=False,
                                                    initial=init, logpost_grad=st.reference(), **kw)
        assert np.isfinite(X).all() and np.isfinite(sg).all() and np.isfinite(th).all()
        assert np.isfinite(extra["all"]["energy"]).all() and np.isfinite(extra["all"]["target_log_prob"]).all()
        assert (extra["all"]["leapfrogs"] >= 1).all()


def test_the_metrics_of_history_4_part_within_two_transitions():
    """Identity, metric A, metric B on B41: the whitened reference runs of chain 20 differ pairwise, in the state after two transitions,
    by >= 1e-6 of its scale."""
    st = R.stop_state(R.Stop("B41", None, "sirw", "M0"))
    N, D, P = len(st.pr.I), st.pr.D, st.pr.P
    init = tuple(a[0] for a in st.states(1))
    runs = {}
    for tag in (None, "A", "B"):
        table = None if tag is None else {0: M.pack_metric(*(a[0] for a in R.metric_arrays(tag, 2, N, D, P)))}
        with np.errstate(all="ignore"):
            out = M.sample_chain(st.pr, None, None, None, 1, 1, seed=R.SEED, chain=20, step_size=R.NUTS["step_size"], stale_cache=False,
                                 max_tree_depth=R.NUTS["max_tree_depth"], initial=init, metric=table)
        assert np.isfinite(out[4]["q"]).all() and (out[4]["all"]["leapfrogs"] >= 1).all()
        runs[tag] = out[4]["q"]
    gaps = {f"{a} -> {b}": _gap(runs[a], runs[b]) for a, b in ((None, "A"), ("A", "B"), ("B", None))}
    print("metric history, state gap after two transitions:", {k: f"{v:.3g}" for k, v in gaps.items()})
    assert min(gaps.values()) >= MARGIN
    A, B = R.metric_arrays("A", 2, N, D, P), R.metric_arrays("B", 2, N, D, P)
    assert all(((a > 0.25) & (a < 4.0)).all() for a in A + B) and not np.array_equal(A[0][0], A[0][1])


def _header_text():
    with open(HEADER) as f:
        return " ".join(f.read().replace("\n *", " ").split())


def test_the_header_states_what_the_gpu_histories_assert():
    text = _header_text()
    assert "magi_set_matrices and magi_build_dense forget the problem, whatever the shape" in text
    assert "magi_pack_resident and magi_build_matrices at an unchanged (N, D) keep the problem AND its model" in text
    at = text.index("Between two magi_sampler_run calls of one run")
    para = text[at: at + 1600]
    for name in R.PAUSE_HEADER_NAMES:
        assert name in para, name
    assert "the continued run is the uninterrupted one bit for bit" in para
    assert set(R.PAUSE_CALLS.values()) == {"continues"}          # the header names no call of history 5 that ends a paused run
