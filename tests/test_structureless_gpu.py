"""The streaming kernels against the CPU oracle where every operator block counts.

Every other comparison of the log-posterior, gradient and sampler kernels with the oracle runs on Matern-built matrices, which are numerically
banded: only the diagonal 128 x 128 blocks and their neighbours have any effect there (tests/test_structureless_cpu.py measures it), so a far
block that is dropped, transposed, read from the wrong tile, paired with the wrong partner or summed into the wrong slot goes unseen.  Here the
matrices are structureless (tests/util.py: structureless_problem -- i.i.d. entries, non-symmetric; A A^T + I/2 for the sampler), legal input
of magi_set_matrices, and removing ANY single block moves the oracle's gradient by >= 1e-5 of its scale, while the oracle itself sits within
1e-13 of its longdouble evaluation (same file).  What that reaches: the task table and its launch-order permutation (csrc/pack.hip), the
FH_bb + FK_bb pairs of the separable kernel, the |bi - bj| > wb block skip with wb >= 1 and nb >= 3, the backward (odd-slot) walk over far
blocks, the column-sum rotation of the matrix-core kernels, the nb-slot reduction of k_point, GEMM class <7> (FE = Ksym m, FH = m^T FE +
Csym) and its forced super-block tile order.

Tolerances are the project's: 1e-10 for the reference-order three-phase path, 1e-9 for the sampler's single-phase ("fused") path, of the value
and of each gradient's largest entry; summation-order rounding on these inputs is O(sqrt(N) 2^-53) ~ 1e-14."""
import functools

import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests.test_structureless_cpu import BAND_DRIFTS, BANDS, EDGE_SIZES, SAMPLER_CASES, STATE_BATCHES, TRACED, fixture, register_traced
from tests.util import STRUCTURELESS_SIG_PRE, engine_for, structureless_states, structureless_theta

pytestmark = pytest.mark.gpu


def _assert_close(got, ref, tol, what):
    """Value relative to itself, every gradient to tol of its own largest entry (as test_logpost_at_n4096_against_the_cpu_oracle)."""
    figures = [abs(got[0] - ref[0]) / abs(ref[0])] + [np.abs(np.asarray(g) - r).max() / np.abs(r).max() for g, r in zip(got[1:], ref[1:])]
    print(what, "value / dX / dsigma / dtheta:", " ".join(f"{v:.2e}" for v in figures), f"(bar {tol:g})")
    for name, v in zip(("value", "dX", "dsigma", "dtheta"), figures):
        assert v <= tol, (what, name, v, tol)


def _compare_with_oracle(eng, pr, X, batches, what, temp=0.8):
    """Three-phase at 1e-10; fused at 1e-9 in even AND odd slots (fused_parity: the backward walk, the other halves of the plan ring and of
    the operand mirrors), the two bit for bit equal."""
    for n in batches:
        Xb, sp, tp = structureless_states(pr, X, n, 0)
        truth = [orc.logpost_grad(Xb[c], sp[c], tp[c], temp, pr) for c in range(n)]
        args = (Xb, sp, tp) if n > 1 else (Xb[0], sp[0], tp[0])
        pick = (lambda out, c: [a[c] for a in out]) if n > 1 else (lambda out, c: out)
        eng.set_option("fused_parity", 0)
        three = eng.logpost_grad(*args, temp)
        even = eng.logpost_grad(*args, temp, fused=True)
        eng.set_option("fused_parity", 1)
        odd = eng.logpost_grad(*args, temp, fused=True)
        eng.set_option("fused_parity", 0)
        for a, b in zip(even, odd):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: fused, even against odd slot, {n} states")
        for c in range(n):
            _assert_close(pick(three, c), truth[c], 1e-10, f"{what} {eng.stream_kernel_name(n)} three-phase state {c}/{n}")
            _assert_close(pick(even, c), truth[c], 1e-9, f"{what} {eng.stream_kernel_name(n)} fused state {c}/{n}")


@pytest.mark.parametrize("N,drift", [(N, d) for N in EDGE_SIZES for d in ("seir3", "sirw")] + [(1024, "seir4")])
def test_log_posterior_and_gradient_match_oracle_on_structureless_matrices(N, drift, stream_family):
    """Block-edge sizes (one to five block rows, ragged and full last blocks) with SEIR-3 and SIRW (three basis functions: a second plane on
    grid.z of the separable kernel), and the production shape N = 1024 x 4 (544 tasks, paired stasks, the permuted launch order).  At N = 513
    and N = 1024 the state batches 1, 2, 3, 8, 9, 16, 17: k_stream<1>, <2>, the 8- and 16-wide mirrors, a second chain group with a ragged tail."""
    pr, X = fixture(N, drift)
    eng = engine_for(pr)
    try:
        _compare_with_oracle(eng, pr, X, STATE_BATCHES if N in (513, 1024) else (1, 3), f"N={N} {drift} {stream_family}")
    finally:
        eng.close()


@pytest.mark.parametrize("drift", TRACED)
def test_traced_drifts_match_oracle_on_structureless_matrices(drift, stream_family):
    """N = 513 (five block rows) with the protein-transduction system (not separable: k_stream_mc from three states on) and the seasonal
    SEIR (its operand mirror holds basis functions of t): 1 and 5 states."""
    d = register_traced(drift, 513)
    pr, X = fixture(513, drift)
    eng = engine_for(pr, drift=d)
    try:
        if stream_family == "mc":
            assert eng.stream_kernel_name(5).startswith("k_stream_mc" if drift == "ptrans" else "k_stream_sep")
        _compare_with_oracle(eng, pr, X, (1, 5), f"N=513 {drift} {stream_family}")
    finally:
        eng.close()


def test_forced_super_block_tile_order_matches_oracle_at_n1024():
    """gemm_remap_min = 1: the single-phase operators (GEMM class <7> of csrc/build.hip) are formed in the super-block tile order; on Matern
    matrices that order is only ever compared with the plain one.  Here the fused path built that way is held to the oracle."""
    pr, X = fixture(1024, "seir4")
    eng = engine_for(pr, options={"gemm_remap_min": 1})
    try:
        _compare_with_oracle(eng, pr, X, (1, 3), "N=1024 seir4 remap")
    finally:
        eng.close()


@pytest.mark.parametrize("drift", BAND_DRIFTS)
@pytest.mark.parametrize("band", BANDS)
def test_band_edges_match_the_masked_oracle_at_five_block_rows(band, drift, stream_family):
    """N = 513 (nb = 5) against the reference's band_part(., b, b) semantics: b = 0 the diagonal mask (the library takes it: storage of one
    column); 20: wb = 1, every far block skipped; 42 / 43: 3 b = 126 / 129, wb goes from 1 to 2; 85 / 86: 6 b + 1 = 511 / 517, banded against
    dense fused storage; 255 / 256: 2 b + 1 = 511 / 513, banded against dense three-phase storage.  The golden band fixtures (N = 161, two
    block rows) can never skip a block."""
    pr, X = fixture(513, drift, band=band)
    eng = engine_for(pr, band, matrices=pr.unmasked)
    try:
        _compare_with_oracle(eng, pr, X, (1, 5), f"N=513 {drift} b={band} {stream_family}", temp=1.0)
    finally:
        eng.close()


# ---- sampler -------------------------------------------------------------------------------------------------------------------

NUTS = dict(burnin=4, results=3, step=2e-3, depth=7, seed=808)


def _inits(pr, X):
    sig0 = np.log1p(np.exp(STRUCTURELESS_SIG_PRE)) + pr.LB
    return sig0, structureless_theta(pr.drift)


@functools.lru_cache(maxsize=None)
def _spd_fixture(N, drift, band=None, salt=0):
    return fixture(N, drift, spd=True, band=band, salt=salt)


@functools.lru_cache(maxsize=None)
def _oracle_nuts(N, drift, band, salt, chain):
    pr, X = _spd_fixture(N, drift, band, salt)
    sig0, th0 = _inits(pr, X)
    trace = []
    out = orc.sample_chain(pr, X, sig0, th0, NUTS["results"], NUTS["burnin"], seed=NUTS["seed"], chain=chain, step_size=NUTS["step"],
                           stale_cache=False, trace=trace, max_tree_depth=NUTS["depth"])
    return out, trace


def _assert_chain_equals_oracle(Xs, tp, d, i, oracle):
    """The assertions of test_deep_trees_match_oracle_draw_for_draw_in_every_kernel_family."""
    (oX, osp, otp, info, _), trace = oracle
    np.testing.assert_array_equal(d.tree_depth[i], [r.depth for _, r, _ in trace])
    np.testing.assert_array_equal(d.leapfrogs_taken[i], [r.leapfrogs for _, r, _ in trace])
    np.testing.assert_array_equal(d.is_accepted[i], [int(r.is_accepted) for _, r, _ in trace])
    np.testing.assert_allclose(d.target_log_prob[i], [r.target_log_prob for _, r, _ in trace], rtol=1e-8)
    np.testing.assert_allclose(Xs[i], oX, rtol=0, atol=1e-8 * np.abs(oX).max())
    np.testing.assert_allclose(tp[i], otp, rtol=1e-7, atol=1e-9)


def _run_nuts(eng, states, ids):
    cfg = eng.default_cfg(num_results=NUTS["results"], num_burnin_steps=NUTS["burnin"], step_size=NUTS["step"], max_tree_depth=NUTS["depth"], stale_cache=0)
    eng.sampler_init(cfg, *states, seed=NUTS["seed"], chain_ids=ids)
    lf, _ = eng.sampler_run(NUTS["burnin"] + NUTS["results"])
    Xs, sp, tp = eng.sampler_samples()
    d = eng.sampler_diag()
    assert lf == d.leapfrogs_taken.sum() and d.leapfrogs_taken.max() >= 31 and d.is_accepted.sum() >= len(ids)
    return Xs, tp, d


@pytest.mark.parametrize("N,drift,chains,band", [(N, d, c, None) for N, d in SAMPLER_CASES for c in (1, 2, 3, 9)] + [(513, "seir3", 3, 43)])
def test_deep_trees_match_oracle_draw_for_draw_on_a_structureless_density(N, drift, chains, band, stream_family):
    """NUTS on a target whose far blocks are as large as its near ones (spd fixtures, three and five block rows; one case under the band mask
    b = 43, wb = 2): first step 2e-3, trees capped at depth 7, 4 + 3 transitions, no stale cache -- depth-7 trees from the first transition on
    (127, 31, 31, 127, 127, 127, 63 leapfrogs for chain 20 at N = 384 / SEIR-3; 6-7 of 7 transitions accept).  Integer diagnostics exact,
    target_log_prob to 1e-8, states to 1e-8 of scale.
    The length is what the reference itself resolves: the oracle chain run with its fn_L evaluated in longdouble (same Philox streams) gives
    the same integers on all seven transitions and states within 1.5e-11 of scale (theta_pre within 3.4e-11, target_log_prob within 2.4e-11
    relative) over every fixture and chain id used here, all below the 1e-10 that keeps a transition -- the 1e-8 bar has > 100 x over the
    reference's own sensitivity."""
    pr, X = _spd_fixture(N, drift, band)
    sig0, th0 = _inits(pr, X)
    X0, s0, t0 = orc.initial_state(X, sig0, th0, pr.LB)
    eng = engine_for(pr, band, matrices=pr.unmasked)
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    ids = list(range(20, 20 + chains))
    try:
        Xs, tp, d = _run_nuts(eng, (rep(X0), rep(s0), rep(t0)), ids)
        print(N, drift, chains, band, stream_family, eng.stream_kernel_name(chains), "leapfrogs", d.leapfrogs_taken.tolist())
    finally:
        eng.close()
    for i in sorted({0, chains - 1}):
        _assert_chain_equals_oracle(Xs, tp, d, i, _oracle_nuts(N, drift, band, 0, ids[i]))


def test_fixed_length_hmc_first_transition_matches_oracle_on_a_structureless_density(stream_family):
    """ONE fixed-L transition (L = 8, step 1e-3, three chains, SIRW at N = 384): the log acceptance ratio sums up eight leapfrogs' energies.
    Asserted as test_fixed_length_hmc_first_transition_from_a_small_step_matches_oracle."""
    pr, X = _spd_fixture(384, "sirw")
    sig0, th0 = _inits(pr, X)
    X0, s0, t0 = orc.initial_state(X, sig0, th0, pr.LB)
    L, chains = 8, 3
    eng = engine_for(pr)
    cfg = eng.default_cfg(num_results=1, num_burnin_steps=0, step_size=1e-3, mode=1, hmc_leapfrogs=L)
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    ids = list(range(7, 7 + chains))
    try:
        eng.sampler_init(cfg, rep(X0), rep(s0), rep(t0), seed=31, chain_ids=ids)
        eng.sampler_run(1)
        Xs, sp, tp = eng.sampler_samples()
        d = eng.sampler_diag()
    finally:
        eng.close()
    for i in (0, chains - 1):
        trace = []
        oX, osp, otp, info, _ = orc.sample_chain(pr, X, sig0, th0, 1, 0, seed=31, chain=ids[i], step_size=1e-3, hmc_leapfrogs=L, trace=trace)
        r = trace[0][1]
        assert np.isfinite(r.log_accept_ratio) and r.is_accepted
        assert int(d.is_accepted[i, 0]) == int(r.is_accepted)
        np.testing.assert_allclose(d.log_accept_ratio[i, 0], r.log_accept_ratio, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(d.target_log_prob[i, 0], r.target_log_prob, rtol=1e-9)
        np.testing.assert_allclose(tp[i], otp, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(Xs[i], oX, rtol=0, atol=1e-8 * np.abs(oX).max())


def test_problem_group_members_match_their_own_oracle_chains():
    """Two structureless densities of one shape (N = 384, SEIR-3; the second from another seed) in one problem group, two chains each: every
    chain against the ORACLE chain of its member (the other group tests compare with the members' own handles)."""
    from magi_v2_amd.engine import MagiGroup
    members = [_spd_fixture(384, "seir3", None, salt) for salt in (0, 1)]
    engs = [engine_for(pr) for pr, _ in members]
    ids = [[20, 21], [21, 28]]                                  # (ids may repeat across members)
    states = []
    for pr, X in members:
        sig0, th0 = _inits(pr, X)
        states.append(orc.initial_state(X, sig0, th0, pr.LB))
    stacked = [np.concatenate([np.repeat(np.asarray(s[k])[None], 2, axis=0) for s in states]) for k in range(3)]
    g = MagiGroup(engs)
    try:
        assert g.stream_kernel_name(4) == "k_stream_group<2>"
        Xs, tp, d = _run_nuts(g, stacked, ids[0] + ids[1])
    finally:
        g.close()
        for e in engs:
            e.close()
    assert not np.array_equal(Xs[1], Xs[2])                     # chain id 21 in two different problems
    for m in range(2):
        for c in range(2):
            _assert_chain_equals_oracle(Xs, tp, d, 2 * m + c, _oracle_nuts(384, "seir3", None, m, ids[m][c]))
