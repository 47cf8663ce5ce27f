"""The device-resident NUTS state machine against the oracle on every branch it takes.

The cases are ``tests.util.BRANCH_CASES``; tests/test_sampler_branches_cpu.py proves on the CPU which branches each of them takes (sub-tree
U-turn checks that end a subtree early at levels 1-2, 3-4 and >= 5, or at its last leaf; trees of depth 9 and 10 with checkpoint levels 7-9;
divergence inside a subtree and in a transition that had accepted; the depth cap at 1, 7 and 12; a rejected subtree next to a proposal that
must survive; min_temp, anneal, target_accept_prob, num_adaptation_steps, max_energy_diff in fixed-L HMC), that a device deciding them
wrongly would change the integer diagnostics compared here, and that no case sits on a rounding knife-edge.

Every case runs draw for draw in both kernel families (``stream_family``) for the chain counts that select each instantiation: 1 and 2
(k_stream<1>, k_stream<2>), 3 (the 8-wide mirror) and, for one U-early and one Div-mid case, 9 (the 16-wide mirror); the first and the last
chain of a batch are compared.  EVERY diagnostic is compared: integers exactly, floats at the tolerances of
test_deep_trees_match_oracle_draw_for_draw_in_every_kernel_family (``tests.util.BRANCH_TOL``).

``energy`` had no tolerance before.  Measured on the CPU over the table, numpy oracle vs the C port's summation order: largest
|energy difference| 3.9e-9 (case target_accept, |energy| ~ 9.4e3, i.e. 4e-13 relative); ENERGY_CPU_DISCREPANCY = 4e-9 bounds it (asserted
in the CPU file), atol = 100 x that = 4e-7 next to rtol 1e-8 -- at most 1.3e-7 of a chain's largest |target_log_prob|."""
import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import util as U

pytestmark = pytest.mark.gpu


def _ids(n):
    """Chain ids of a batch of n: 20 first, 21 last -- the two chains the CPU file vets."""
    return [U.BRANCH_CHAINS[0]] + list(range(22, 20 + n)) + ([U.BRANCH_CHAINS[1]] if n > 1 else [])


def _states(case, n):
    g, pr, pr_dense = U.branch_problem(case)
    X0, s0, t0 = orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), pr.LB)
    rep = lambda v: np.repeat(np.asarray(v)[None], n, axis=0)
    return rep(X0), rep(s0), rep(t0)


def _cfg(eng, case):
    return eng.default_cfg(num_results=case.results, num_burnin_steps=case.burnin, stale_cache=0, **case.cfg)


def _assert_chain_is_the_oracles(case, chain, i, Xs, sp, tp, d):
    (oX, osp, otp, _, _), trace, _ = U.branch_oracle_run(case, chain)
    col = lambda f, t=np.float64: np.array([getattr(r, f) for _, r, _ in trace]).astype(t)
    T = case.burnin + case.results
    where = f"{case.name} chain {chain}"
    for name, field in (("tree_depth", "depth"), ("leapfrogs_taken", "leapfrogs"), ("has_divergence", "has_divergence"),
                        ("reach_max_depth", "reach_max_depth"), ("is_accepted", "is_accepted")):
        np.testing.assert_array_equal(getattr(d, name)[i], col(field, np.int64), err_msg=f"{where}: {name}")
    temps = [orc.temperature(k, case.cfg.get("min_temp", 0.1)) if case.cfg.get("anneal", 1) else 1.0 for k in range(T)]
    np.testing.assert_allclose(d.beta_temp[i], temps, rtol=1e-15, atol=0, err_msg=where)
    tol = U.BRANCH_TOL
    np.testing.assert_allclose(d.step_size[i], [s for _, _, s in trace], rtol=tol["step_size"][0], atol=tol["step_size"][1], err_msg=where)
    lar = col("log_accept_ratio")
    fin = np.isfinite(lar)
    np.testing.assert_array_equal(np.isfinite(d.log_accept_ratio[i]), fin, err_msg=where)
    np.testing.assert_allclose(d.log_accept_ratio[i][fin], lar[fin], rtol=tol["log_accept_ratio"][0], atol=tol["log_accept_ratio"][1], err_msg=where)
    np.testing.assert_allclose(d.target_log_prob[i], col("target_log_prob"), rtol=tol["target_log_prob"][0], atol=tol["target_log_prob"][1], err_msg=where)
    np.testing.assert_allclose(d.energy[i], col("energy"), rtol=U.ENERGY_TOL[0], atol=U.ENERGY_TOL[1], err_msg=f"{where}: energy")
    np.testing.assert_allclose(Xs[i], oX, rtol=0, atol=tol["X"][1] * np.abs(oX).max(), err_msg=where)
    np.testing.assert_allclose(sp[i], osp, rtol=tol["sig_pre"][0], atol=tol["sig_pre"][1], err_msg=where)
    np.testing.assert_allclose(tp[i], otp, rtol=tol["th_pre"][0], atol=tol["th_pre"][1], err_msg=where)


@pytest.mark.parametrize("case,chains", [(c, n) for c in U.BRANCH_CASES for n in c.batches], ids=repr)
def test_branch_case_matches_oracle_draw_for_draw_in_every_kernel_family(case, chains, stream_family):
    _, _, pr_dense = U.branch_problem(case)
    eng = U.engine_for(pr_dense, case.band)
    try:
        ids = _ids(chains)
        eng.sampler_init(_cfg(eng, case), *_states(case, chains), seed=case.seed, chain_ids=ids)
        lf, _ = eng.sampler_run(case.burnin + case.results)
        Xs, sp, tp = eng.sampler_samples()
        d = eng.sampler_diag()
    finally:
        eng.close()
    assert lf == d.leapfrogs_taken.sum()
    for i in sorted({0, chains - 1}):
        _assert_chain_is_the_oracles(case, ids[i], i, Xs, sp, tp, d)


def test_problem_group_of_two_members_takes_early_u_turns_like_the_oracle(monkeypatch):
    """The group kernels are instantiations of their own: two members of one shape (the SIRW fixture and a variant of it with other data and
    another K^-1), two chains each, on a configuration whose subtrees end early at a level-2 check in both members."""
    from magi_v2_amd.engine import MagiGroup
    monkeypatch.delenv("MAGI_STREAM_FAMILY", raising=False)              # (a group runs the VALU kernels only)
    cases = [U.branch_case("u_early_l2"), U.branch_case("u_early_member2")]
    assert cases[0].cfg == cases[1].cfg and cases[0].seed == cases[1].seed
    engs = [U.engine_for(U.branch_problem(c)[2], c.band) for c in cases]
    try:
        grp = MagiGroup(engs)
        try:
            assert grp.stream_kernel_name(4) == "k_stream_group<2>"
            states = [np.concatenate(parts) for parts in zip(*(_states(c, 2) for c in cases))]
            grp.sampler_init(_cfg(grp, cases[0]), *states, seed=cases[0].seed, chain_ids=list(U.BRANCH_CHAINS) * 2)
            lf, _ = grp.sampler_run(cases[0].burnin + cases[0].results)
            Xs, sp, tp = grp.sampler_samples()
            d = grp.sampler_diag()
        finally:
            grp.close()
    finally:
        for e in engs:
            e.close()
    assert lf == d.leapfrogs_taken.sum()
    for m, case in enumerate(cases):
        for j, chain in enumerate(U.BRANCH_CHAINS):
            _assert_chain_is_the_oracles(case, chain, 2 * m + j, Xs, sp, tp, d)
