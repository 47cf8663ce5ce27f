"""The kernels compiled for traced drifts at the documented shape limits and at the edges of the printer's and the separator's vocabulary
(magi_v2_amd.drift_examples.EDGE_EXAMPLES), against what the CALLABLE computes.

selftest.py probes such a library against ``f_np`` / ``jac_np``, the host evaluators of the same sympy trace and the same CSE, and the other
GPU tests use nine drifts of D in {2, 3, 5}, P in {3, 4, 6, 7}.  Here: D = 1 (three idle component lanes of four), D = 7 and 8 with the wide
lane groups (one idle lane, none), P = 8 (the parameter blocks filled to their next field), pow() of every kind, tanh / sin / log / exp of
state entries, rational constants, four basis functions in one component, a constant basis function, a coefficient that is the number 1, a
merged pair, a component that is identically zero -- each held to the longdouble evaluation of the callable (the probe) and to the oracle on
N = 129 structureless matrices (log posterior, gradient, NUTS draw for draw, the theta initialiser on NON-symmetric K^-1).  The conditions
under which these comparisons mean something are asserted in tests/test_drift_edges_cpu.py.  Every tolerance is one the project already uses.

Nothing here needs N above 129: two operator block rows with a one-row last block, 17 point workgroups of 8 points at D > 4 and 9 of 16
otherwise, ragged in both cases; what larger grids add (more block rows, the task table) is held by tests/test_structureless_gpu.py."""
import numpy as np
import pytest

from magi_v2_amd.drift_examples import EDGE_EXAMPLES
from magi_v2_amd.engine import MagiEngine, MagiHipError
from oracle import magi_oracle as orc
from tests import test_drift_edges_cpu as E
from tests.test_structureless_gpu import _assert_chain_equals_oracle, _compare_with_oracle, _run_nuts
from tests.util import engine_for

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _registered():
    with E.edge_drifts():
        yield


@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES))
def test_drift_probe_equals_the_longdouble_truth_of_the_callable_on_every_path(name):
    """257 points (a full block of the probe kernel and a one-thread tail) on paths 0 (DriftT::f / jt), 1 (the runtime-switch entries),
    3 (DriftT::f1) and, for separable entries, 2 (sum_k coefs * basis), at selftest.TOL_DRIFT."""
    d = E.traced(name)
    X, th, g = E.probe(name)
    want = E.truth(name)
    sep = E.STRUCTURE[name][0]
    eng = MagiEngine(0, drift=d)
    try:
        worst = {}
        for path in (0, 1):
            worst[f"path{path}"] = E.probe_errors(eng.drift_probe(d, X, th, g, path), want)
        worst["path3"] = E.probe_errors(eng.drift_probe(d, X, th, None, 3), want)
        if sep:
            worst["path2"] = E.probe_errors(eng.drift_probe(d, X, th, None, 2), want)
        else:
            with pytest.raises(MagiHipError, match="separable"):
                eng.drift_probe(d, X, th, None, 2)
        if name == "mixed3":
            # x = 0 and g along component 1: every term of df_1/dtheta that holds x vanishes exactly, so t = (g_1, 0, 0, 0, 0, 0) to the bit
            # unless the parameter-free group (coefficient 1.0) leaks into the theta-gradient; the zero component gives 0.0 on every path
            X0, g0 = X.copy(), np.zeros_like(g)
            X0[:, 0], g0[:, 1] = 0.0, g[:, 1]
            for path in (0, 1):
                f, _, t = eng.drift_probe(d, X0, th, g0, path)
                np.testing.assert_array_equal(t, np.concatenate([g0[:, 1:2], np.zeros((len(X0), 5))], axis=1), err_msg=f"path {path}")
                np.testing.assert_array_equal(f[:, 2], 0.0, err_msg=f"path {path}")
            for path in (0, 1, 2, 3):
                np.testing.assert_array_equal(eng.drift_probe(d, X, th, g if path < 2 else None, path)[0][:, 2], 0.0, err_msg=f"path {path}")
    finally:
        eng.close()
    print("drift probe against the longdouble truth, fraction of TOL_DRIFT:", name, {p: {k: f"{v / E.TOL:.1e}" for k, v in by.items()} for p, by in worst.items()})
    for path, by in worst.items():
        for what, e in by.items():
            assert e <= E.TOL, (name, path, what, e)


def _kernel_family(name):
    return "k_stream_sep" if E.STRUCTURE[name][0] else "k_stream_mc"


@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES))
def test_log_posterior_and_gradient_match_oracle_at_the_shape_and_vocabulary_edges(name, stream_family):
    """N = 129 structureless matrices, 1, 2, 3 and 9 states: three-phase at 1e-10, fused at 1e-9, even and odd slot bit-equal."""
    d = E.traced(name)
    pr, X = E.fixture(name)
    eng = engine_for(pr, drift=d)
    try:
        if stream_family == "mc":
            for n in (3, 9):
                assert eng.stream_kernel_name(n).startswith(_kernel_family(name)), (name, n, eng.stream_kernel_name(n))
        _compare_with_oracle(eng, pr, X, E.STATE_BATCHES, f"N={E.N_FIX} {name} {stream_family}")
    finally:
        eng.close()


def test_banded_chain8_matches_the_masked_oracle(stream_family):
    """D = 8, P = 8 under the band mask b = 20 (banded storage of both operator block rows)."""
    d = E.traced("chain8")
    pr, X = E.fixture("chain8", band=20)
    eng = engine_for(pr, 20, matrices=pr.unmasked, drift=d)
    try:
        _compare_with_oracle(eng, pr, X, E.STATE_BATCHES, f"N={E.N_FIX} chain8 b=20 {stream_family}", temp=1.0)
    finally:
        eng.close()


@pytest.mark.parametrize("name,chains", [(n, c) for n in E.SAMPLER_CASES for c in (1, 3)] + [("chain8", 9)])
def test_nuts_matches_oracle_draw_for_draw_at_the_shape_edges(name, chains, stream_family):
    """The NUTS parameters of tests/test_structureless_gpu.py on the entry's spd fixture: 4 + 3 transitions of up to 127 leapfrogs; 9 chains
    of chain8 open a second chain group.  Integer diagnostics exact, target_log_prob to 1e-8, states to 1e-8 of scale."""
    d = E.traced(name)
    pr, X = E.fixture(name, spd=True)
    sig0, th0 = E.nuts_inits(pr, X)
    X0, s0, t0 = orc.initial_state(X, sig0, th0, pr.LB)
    eng = engine_for(pr, drift=d)
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    ids = list(range(20, 20 + chains))
    try:
        if stream_family == "mc" and chains >= 3:
            assert eng.stream_kernel_name(chains).startswith(_kernel_family(name))
        Xs, tp, diag = _run_nuts(eng, (rep(X0), rep(s0), rep(t0)), ids)
        print(name, chains, stream_family, eng.stream_kernel_name(chains), "leapfrogs", diag.leapfrogs_taken.tolist())
    finally:
        eng.close()
    for i in sorted({0, chains - 1}):
        assert ids[i] in E.sampler_chains(name)
        (oX, _, otp, _, _), trace = oracle = E.oracle_nuts(name, ids[i])
        print(f"  chain {ids[i]}: X {np.abs(Xs[i] - oX).max() / np.abs(oX).max() / 1e-8:.1e} of its bar, theta_pre "
              f"{(np.abs(tp[i] - otp) / (1e-9 + 1e-7 * np.abs(otp))).max():.1e}, target_log_prob "
              f"{np.max(np.abs(diag.target_log_prob[i] / np.array([r.target_log_prob for _, r, _ in trace]) - 1.0)) / 1e-8:.1e}")
        _assert_chain_equals_oracle(Xs, tp, diag, i, oracle)


@pytest.mark.parametrize("name", E.THETA_INIT_CASES)
def test_theta_initialiser_equals_oracle_on_non_symmetric_matrices(name):
    """K^-1 r and K^-T r differ here (on Matern matrices they are one vector, and a dropped or doubled transpose passes): chain8 fills every
    state and parameter slot, logistic1 makes the reference's reshape the identity, cascade7 is not linear in theta.  The bars of
    tests/test_theta_init_gpu.py; the CPU file shows that a one-sided gradient ends > 1000 of them away."""
    d = E.traced(name)
    pr, _ = E.fixture(name)
    Xhat, mu, _, _ = E.theta_init_inputs(name)
    want, olosses = E.oracle_theta_init(name)
    eng = engine_for(pr, drift=d)
    try:
        got, losses = eng.theta_init(eng.user_drift, Xhat, mu, E.THETA_INIT_ITERS, want_trace=True)
    finally:
        eng.close()
    print(name, f"theta initialiser: theta {(np.abs(got - want) / (1e-10 + 1e-8 * np.abs(want))).max():.2e} of its bar, "
          f"loss trace {np.max(np.abs(losses / olosses[:E.THETA_INIT_ITERS] - 1.0)) / 1e-8:.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(losses, olosses[:E.THETA_INIT_ITERS], rtol=1e-8)
