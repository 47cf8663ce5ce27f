"""The device-resident sampler against the oracle on leaves with non-finite energies.

A leapfrog step that leaves the domain of a square-root or logarithmic drift gives a NaN energy; csrc/decide.h counts the leaf as energy -inf, as
TFP and the oracle do.  Around that one line everything must tolerate NaN in a chain's leaf buffers: the speculative next leaf written from a
NaN state, sub-tree U-turn dots over NaN momenta, logaddexp(-inf, -inf) and log(0 / n), masks that must select and not multiply (0 x NaN
leaks into a neighbouring chain of a batch, a neighbouring member of a problem group or the unused columns of a matrix-core operand), fixed-L HMC
integrating on through NaN, dual averaging fed -inf.  The cases are ``tests.util.DOMAIN_CASES``; tests/test_nonfinite_cpu.py proves on the CPU
what each of them takes, that no evaluated state is within rounding of the domain's edge, that no decision sits on a rounding knife-edge and that
a device without the rule would fail the comparisons made here.

Every case runs draw for draw in both kernel families for its batch sizes (chain ids 20 .. and 21 last; first and last chain compared):
integers exactly, floats at ``tests.util.BRANCH_TOL`` / ``ENERGY_TOL`` with -inf required where the oracle has -inf, every kept sample and the
final state finite.  With ``stream_family = mc`` the square-root drift runs on k_stream_sep and the logarithmic one on k_stream_mc (asserted
through ``stream_kernel_name``).

Measured on an MI355X (error as a fraction of the tolerance, worst field): sqrt_deep 1.4e-3, sqrt_last_leaf 5.2e-3, gompertz_first_leaf 3.5e-6,
sqrt_hmc 1.8e-5, gompertz_hmc 1.3e-5, sqrt_n161 4.0e-4, the group 9.5e-3; every integer and every -inf in place on every kernel."""
import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import util as U

pytestmark = pytest.mark.gpu

MC_KERNEL = {"sqrt_outflow": "k_stream_sep", "gompertz": "k_stream_mc"}


def _ids(n):
    return [U.BRANCH_CHAINS[0]] + list(range(22, 20 + n)) + ([U.BRANCH_CHAINS[1]] if n > 1 else [])


def _drift(case):
    from magi_v2_amd import drift
    from magi_v2_amd.drift_examples import DOMAIN_EXAMPLES
    return drift.resolve(*DOMAIN_EXAMPLES[case.tag])


def _engine(case):
    _, _, pr_dense = U.domain_problem(case)
    return U.engine_for(pr_dense, case.band, drift=_drift(case))


def _states(case, n):
    fx, pr, _ = U.domain_problem(case)
    X0, s0, t0 = orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), pr.LB)
    rep = lambda v: np.repeat(np.asarray(v)[None], n, axis=0)
    return rep(X0), rep(s0), rep(t0)


def _cfg(eng, case):
    return eng.default_cfg(num_results=case.results, num_burnin_steps=case.burnin, stale_cache=0, **case.cfg)


def _close(got, ref, tol, what, worst, scale_atol=1.0):
    """Finite where the oracle is finite and within (rtol, atol) there; the oracle's very value (-inf) elsewhere."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    np.testing.assert_array_equal(got[~fin], ref[~fin], err_msg=what)
    rtol, atol = tol
    bound = atol * scale_atol + rtol * np.abs(ref[fin])
    err = np.abs(got[fin] - ref[fin])
    name = what.split(": ")[-1]
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err > 0, err / bound, 0.0)
        worst[name] = max(worst.get(name, 0.0), float(frac.max()))
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))


def _assert_chain_is_the_oracles(case, chain, i, Xs, sp, tp, d, worst):
    run = U.domain_oracle_run(case, chain)
    oX, osp, otp = run.out[:3]
    col = lambda f, t=np.float64: np.array([getattr(r, f) for _, r, _ in run.trace]).astype(t)
    where = f"{case.name} chain {chain}"
    for name, field in (("tree_depth", "depth"), ("leapfrogs_taken", "leapfrogs"), ("has_divergence", "has_divergence"),
                        ("reach_max_depth", "reach_max_depth"), ("is_accepted", "is_accepted")):
        np.testing.assert_array_equal(getattr(d, name)[i], col(field, np.int64), err_msg=f"{where}: {name}")
    tol = U.BRANCH_TOL
    _close(d.step_size[i], [s for _, _, s in run.trace], tol["step_size"], f"{where}: step_size", worst)
    _close(d.log_accept_ratio[i], col("log_accept_ratio"), tol["log_accept_ratio"], f"{where}: log_accept_ratio", worst)
    _close(d.target_log_prob[i], col("target_log_prob"), tol["target_log_prob"], f"{where}: target_log_prob", worst)
    _close(d.energy[i], col("energy"), U.ENERGY_TOL, f"{where}: energy", worst)
    _close(Xs[i], oX, tol["X"], f"{where}: X", worst, scale_atol=np.abs(oX).max())
    _close(sp[i], osp, tol["sig_pre"], f"{where}: sig_pre", worst)
    _close(tp[i], otp, tol["th_pre"], f"{where}: th_pre", worst)


def _run(eng, case, states, ids, parts=None):
    """(samples, diag, final state, leapfrogs) of the case's chains; ``parts``: the transitions of each magi_sampler_run call."""
    eng.sampler_init(_cfg(eng, case), *states, seed=case.seed, chain_ids=ids)
    lf = sum(eng.sampler_run(n)[0] for n in (parts or [case.burnin + case.results]))
    return eng.sampler_samples(), eng.sampler_diag(), eng.sampler_state(), lf


@pytest.mark.parametrize("case,chains", [(c, n) for c in U.DOMAIN_CASES for n in c.batches], ids=repr)
def test_domain_case_matches_oracle_draw_for_draw_in_every_kernel_family(case, chains, stream_family):
    eng = _engine(case)
    try:
        kernel = eng.stream_kernel_name(chains)
        ids = _ids(chains)
        (Xs, sp, tp), d, state, lf = _run(eng, case, _states(case, chains), ids)
    finally:
        eng.close()
    if stream_family == "mc":
        assert kernel.startswith(MC_KERNEL[case.tag]), kernel
    elif stream_family == "auto" and chains == 1:
        assert kernel == "k_stream<1>", kernel
    assert lf == d.leapfrogs_taken.sum()
    assert all(np.isfinite(a).all() for a in (Xs, sp, tp)) and all(np.isfinite(a).all() for a in state)
    worst = {}
    for i in sorted({0, chains - 1}):
        _assert_chain_is_the_oracles(case, ids[i], i, Xs, sp, tp, d, worst)
    print(case.name, chains, stream_family, kernel, "worst error / tolerance:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_pause_and_resume_across_nan_transitions(stream_family):
    """magi_sampler_run called three times, split right after the two NaN transitions of chain 20 (1: a NaN first leaf, chains 20 and 21;
    7: a NaN leaf inside a depth-4 sub-tree): the same run bit for bit -- whatever the NaN leaf left in the buffers is not read again."""
    case = U.domain_case("sqrt_deep")
    assert U.domain_oracle_run(case, 20).nan_transitions() == [1, 7] and U.domain_oracle_run(case, 21).nan_transitions() == [1]
    ids = _ids(3)
    eng = _engine(case)
    try:
        whole = _run(eng, case, _states(case, 3), ids)
        parts = _run(eng, case, _states(case, 3), ids, parts=[2, 6, 2])
    finally:
        eng.close()
    assert whole[3] == parts[3]
    for a, b in zip(whole[0] + whole[2], parts[0] + parts[2]):
        np.testing.assert_array_equal(a, b)
    for f in ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence", "reach_max_depth", "is_accepted", "target_log_prob",
              "energy", "beta_temp"):
        np.testing.assert_array_equal(getattr(whole[1], f), getattr(parts[1], f), err_msg=f)
    assert whole[1].has_divergence[0, 1] == 1 and whole[1].has_divergence[0, 7] == 1 and np.isneginf(whole[1].log_accept_ratio[0, 1])


def test_problem_group_whose_first_member_takes_nan_leaves(monkeypatch):
    """Two members of one shape in one leapfrog graph: member 0 (``sqrt_deep``) takes NaN leaves, member 1 (``sqrt_interior``: the same system
    started from x(0) = 4, every evaluated state >= 0.3 inside the domain) takes none.  All four chains are the oracle's, and member 1's chains
    equal those of a handle of its own bit for bit: nothing of member 0's NaN reaches its sums."""
    from magi_v2_amd.engine import MagiGroup
    monkeypatch.delenv("MAGI_STREAM_FAMILY", raising=False)              # (a group runs the VALU kernels only)
    cases = [U.domain_case("sqrt_deep"), U.domain_case("sqrt_interior")]
    assert cases[0].cfg == cases[1].cfg and cases[0].seed == cases[1].seed
    ids = list(U.BRANCH_CHAINS)
    engs = [_engine(c) for c in cases]
    try:
        alone = _run(engs[1], cases[1], _states(cases[1], 2), ids)
        grp = MagiGroup(engs)
        try:
            assert grp.stream_kernel_name(4) == "k_stream_group<2>"
            states = [np.concatenate(parts) for parts in zip(*(_states(c, 2) for c in cases))]
            (Xs, sp, tp), d, state, lf = _run(grp, cases[0], states, ids * 2)
        finally:
            grp.close()
    finally:
        for e in engs:
            e.close()
    assert lf == d.leapfrogs_taken.sum()
    assert all(np.isfinite(a).all() for a in (Xs, sp, tp)) and all(np.isfinite(a).all() for a in state)
    worst = {}
    for m, case in enumerate(cases):
        for j, chain in enumerate(ids):
            _assert_chain_is_the_oracles(case, chain, 2 * m + j, Xs, sp, tp, d, worst)
    print("group worst error / tolerance:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert d.has_divergence[0, 1] == 1 and np.isneginf(d.log_accept_ratio[0, 1])
    for a, b in zip((Xs, sp, tp) + state, alone[0] + alone[2]):
        np.testing.assert_array_equal(a[2:], b)
    for f in ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence", "is_accepted", "target_log_prob", "energy"):
        np.testing.assert_array_equal(getattr(d, f)[2:], getattr(alone[1], f), err_msg=f)


@pytest.mark.parametrize("name", ["sqrt_deep", "gompertz_first_leaf", "sqrt_n161"])
def test_log_posterior_outside_the_domain_is_nan_and_stays_in_its_state(name, stream_family):
    """Five states per call, the third with one entry of component 0 outside the domain: its value is NaN in the three-phase and in the fused
    form, the call raises nothing, and the four other states are what they are without it (a mask that multiplied would leak 0 x NaN into them).
    Gradient entries of the NaN state that are finite on both sides agree to 1e-9 of the scale of the gradient at the mirrored state inside the
    domain.  Equal NaN masks are not required: with a band the reference's ``band_part`` multiplies its out-of-band zeros by NaN -- every entry
    of its gradient is NaN -- while the banded device storage never reads them."""
    case = U.domain_case(name)
    fx, pr, _ = U.domain_problem(case)
    rng = np.random.default_rng(11)
    n, bad, row = 5, 2, 7
    X0, s0, t0 = orc.initial_state(fx["Xhat_init"], fx["sigma_sqs_init"], np.ones(pr.P), pr.LB)
    X = np.abs(X0[None] + rng.normal(0, 0.01, (n,) + X0.shape)) + 1e-3
    sp, tp = s0[None] + rng.normal(0, 0.3, (n, pr.D)), t0[None] + rng.normal(0, 0.2, (n, pr.P))
    inside = X.copy()
    X[bad, row, 0] = -inside[bad, row, 0]
    assert inside[bad, row, 0] >= 1e-3
    eng = _engine(case)
    try:
        outs = [eng.logpost_grad(X, sp, tp, 0.7, fused=fused) for fused in (False, True)]
        kernel = eng.stream_kernel_name(n)
    finally:
        eng.close()
    if stream_family == "mc":
        assert kernel.startswith(MC_KERNEL[case.tag]), kernel
    with np.errstate(all="ignore"), U.domain_drifts():
        ref = [orc.logpost_grad(X[c], sp[c], tp[c], 0.7, pr) for c in range(n)]
        scale = np.abs(orc.logpost_grad(inside[bad], sp[bad], tp[bad], 0.7, pr)[1]).max()
    assert np.isnan(ref[bad][0])
    for out, form in zip(outs, ("three-phase", "fused")):
        for c in range(n):
            L, gX, gs, gt = ref[c]
            if c == bad:
                assert np.isnan(out[0][c]), (form, out[0][c])
                for got, want in ((out[1][c], gX), (out[2][c], gs), (out[3][c], gt)):
                    both = np.isfinite(got) & np.isfinite(want)
                    np.testing.assert_allclose(got[both], want[both], rtol=1e-8, atol=1e-9 * scale, err_msg=form)
            else:
                assert abs(out[0][c] - L) <= 1e-9 * abs(L), (form, c)
                np.testing.assert_allclose(out[1][c], gX, rtol=0, atol=1e-9 * np.abs(gX).max(), err_msg=f"{form} {c}")
                np.testing.assert_allclose(out[2][c], gs, rtol=1e-8, atol=1e-9 * np.abs(gX).max(), err_msg=f"{form} {c}")
                np.testing.assert_allclose(out[3][c], gt, rtol=1e-8, atol=1e-9 * np.abs(gX).max(), err_msg=f"{form} {c}")
