"""The proof that the cases of tests/test_sampler_branches_gpu.py see what they claim -- all of it on the CPU, with the oracle alone.

A draw-for-draw run tests a branch of the NUTS state machine only if the run takes it.  ``orc.nuts_one_step(events=...)`` counts the branches
a transition takes (the census); the table ``tests.util.BRANCH_CASES`` lists, per sampler configuration, the branches it is there for.  Here:

* the census records and nothing else: with and without it a chain is the same bit for bit;
* every branch of ``tests.util.BRANCHES`` is claimed by a case, and every case takes every branch it claims (chain 20, the first chain of
  every device batch), within the suite's size limits (<= 12 transitions, <= 1023 leapfrogs per transition);
* SENSITIVITY: with the class of sub-tree U-turn checks a case is there for forced to "no U-turn" (a wrapper around
  ``orc._has_not_u_turn`` local to this file), the case's tree depths or leapfrog counts change -- a device that got those checks wrong
  would fail the case's exact integer comparison; likewise a Div-mid case with max_energy_diff back at 1000;
* ROBUSTNESS: the device sums in another order than numpy, and a case whose decision sat on a rounding knife-edge would fail for no fault of a
  kernel.  Every case runs a second time on the C port's log posterior (oracle/logpost_c.py: another summation order, pinned to the numpy
  oracle at 1e-10 in tests/test_oracle_golden.py): the integer diagnostics must be identical and every compared float within 1/100 of
  the device tolerance.  A case that fails this is replaced by another seed or step, never given a looser bound.

NaN energies are not reached by these cases (asserted below); an overflow-driven one cannot be made to happen at the same leaf on both sides,
one from a drift with a limited domain can: tests/test_nonfinite_cpu.py / tests/test_nonfinite_gpu.py (``tests.util.DOMAIN_CASES``).
Unreached, and why: checkpoint levels 10 and 11 (a level-10 check needs a subtree of 1024 leaves, i.e. a transition of >= 2047 leapfrogs --
twice the per-transition budget of a quick test;
level 9 and depth 10 are reached by ``depth10_fixed_step``, a depth cap of 12 is run by two cases)."""
import collections
import sys

import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import util as U

CASES = U.BRANCH_CASES
INT_FIELDS = ("depth", "leapfrogs", "is_accepted", "has_divergence", "reach_max_depth")


def _fields(out, trace):
    """The floats the device test compares, by name (X with its own scale)."""
    col = lambda f: np.array([getattr(r, f) for _, r, _ in trace], dtype=np.float64)
    return {"step_size": np.array([s for _, _, s in trace]), "log_accept_ratio": col("log_accept_ratio"), "target_log_prob": col("target_log_prob"),
            "X": out[0], "sig_pre": out[1], "th_pre": out[2]}


def _ints(trace):
    return {f: [int(getattr(r, f)) for _, r, _ in trace] for f in INT_FIELDS}


def _forced_run(case, monkeypatch, levels=None, **over):
    """Chain 20 of the case with the sub-tree checks of ``levels`` answering "no U-turn" (the trajectory-level test stays), and / or with
    sample_chain arguments replaced."""
    real = orc._has_not_u_turn

    def forced(rho, p_left, p_right):
        loc = sys._getframe(1).f_locals                   # nuts_one_step: the trajectory-level test passes momentum_sum itself
        if loc.get("momentum_sum") is not rho and loc["k"] in levels:
            return True
        return real(rho, p_left, p_right)

    if levels is not None:
        monkeypatch.setattr(orc, "_has_not_u_turn", forced)
    g, pr, _ = U.branch_problem(case)
    trace = []
    kw = dict(U.branch_oracle_kwargs(case), **over)
    orc.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=U.BRANCH_CHAINS[0],
                     trace=trace, **kw)
    monkeypatch.undo()
    return trace


def test_the_census_changes_nothing():
    case = U.branch_case("u_last")
    g, pr, _ = U.branch_problem(case)
    runs = []
    for events in (None, collections.Counter()):
        trace = []
        out = orc.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=20,
                               trace=trace, events=events, **U.branch_oracle_kwargs(case))
        runs.append((out, trace))
        assert events is None or sum(events.values()) > 0
    (oa, ta), (ob, tb) = runs
    for a, b in zip(oa[:3], ob[:3]):
        np.testing.assert_array_equal(a, b)
    for k in oa[3]:
        np.testing.assert_array_equal(oa[3][k], ob[3][k], err_msg=k)
    assert _ints(ta) == _ints(tb) and max(_ints(ta)["depth"]) == 7
    for (_, ra, sa), (_, rb, sb) in zip(ta, tb):
        assert (ra.energy, ra.target_log_prob, ra.log_accept_ratio, sa) == (rb.energy, rb.target_log_prob, rb.log_accept_ratio, sb)


def test_every_branch_is_claimed_by_a_case():
    claimed = {b for c in CASES for b in c.claims}
    assert claimed == set(U.BRANCHES), set(U.BRANCHES) ^ claimed
    assert len({c.name for c in CASES}) == len(CASES)
    nine = [c for c in CASES if 9 in c.batches]                                    # the 16-wide mirror: one U-early and one Div-mid case
    assert len(nine) == 2 and any("u_early_12" in c.claims for c in nine) and any("div_mid" in c.claims for c in nine)
    assert {U.branch_problem(c)[1].drift for c in CASES} == {"seir3", "seir4", "sirw"}     # the three instantiations of the decision code


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_takes_the_branches_it_is_listed_for(case):
    _, trace, ev = U.branch_oracle_run(case, U.BRANCH_CHAINS[0])
    print(case.name, "depths", _ints(trace)["depth"], "census",
          {k: v for k, v in sorted(ev.items(), key=str) if k[0] not in ("check", "merge_not_chosen", "traj_u", "depth")})
    assert case.claims
    for b in case.claims:
        assert U.BRANCHES[b](case, ev, trace), (case.name, b)
    for chain in U.BRANCH_CHAINS:
        _, tr, e = U.branch_oracle_run(case, chain)
        assert e[("nan",)] == 0                                                    # (NaN energies: tests/test_nonfinite_cpu.py)
        assert len(tr) <= 12 and max(r.leapfrogs for _, r, _ in tr) <= 1023


def test_configuration_cases_move_what_they_are_there_for():
    """min_temp = 0.5 binds (and is what beta_temp follows); the three arms of the step-size update are visible in step_size."""
    case = U.branch_case("min_temp")
    (_, _, _, info, _), trace, _ = U.branch_oracle_run(case, 20)
    temps = [orc.temperature(k, 0.5) for k in range(case.burnin + case.results)]
    np.testing.assert_array_equal(info["beta_temp"], temps[case.burnin:])
    assert temps[5] > 0.5 and temps[6:] == [0.5] * (len(temps) - 6) and orc.temperature(6) < 0.5
    ss = lambda name: [s for _, _, s in U.branch_oracle_run(U.branch_case(name), 20)[1]]
    s0, s2, sall = ss("adapt_0"), ss("adapt_2"), ss("adapt_all")
    assert s0[1] != s0[0] and s0[1:] == [s0[1]] * (len(s0) - 1)                    # at the boundary (step 0), then frozen
    assert len(set(s2[:4])) == 4 and s2[3:] == [s2[3]] * (len(s2) - 3)              # before (0, 1), at (2), after
    assert len(set(sall)) == len(sall)                                              # before, all the way
    ta = [s for _, _, s in U.branch_oracle_run(U.branch_case("target_accept"), 20)[1]]
    tb = [s for _, _, s in _plain(U.branch_case("target_accept"), target_accept_prob=0.75)]
    assert ta[0] == tb[0] and ta[1] != tb[1]
    an = U.branch_oracle_run(U.branch_case("anneal_off"), 20)[0][3]
    np.testing.assert_array_equal(an["beta_temp"], 1.0)


def _plain(case, **over):
    g, pr, _ = U.branch_problem(case)
    trace = []
    orc.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=20, trace=trace,
                     **dict(U.branch_oracle_kwargs(case), **over))
    return trace


# branch -> the check levels whose wrong answer it is there to catch
FORCED = {"u_early_12": (1, 2), "u_early_34": (3, 4), "u_early_high": tuple(U.HIGH), "u_last_high": tuple(U.HIGH), "fail_ge_7": tuple(range(7, 13))}


@pytest.mark.parametrize("case,branch", [(c, b) for c in CASES for b in c.claims if b in FORCED], ids=repr)
def test_a_device_that_got_these_checks_wrong_would_fail_the_case(case, branch, monkeypatch):
    ref = _ints(U.branch_oracle_run(case, 20)[1])
    got = _ints(_forced_run(case, monkeypatch, levels=FORCED[branch]))
    assert orc._has_not_u_turn.__name__ == "_has_not_u_turn"
    print(case.name, branch, "depth", ref["depth"], "->", got["depth"], "leapfrogs", ref["leapfrogs"], "->", got["leapfrogs"])
    assert got["depth"] != ref["depth"] or got["leapfrogs"] != ref["leapfrogs"]


@pytest.mark.parametrize("case", [c for c in CASES if "div_mid" in c.claims], ids=repr)
def test_a_device_that_ignored_max_energy_diff_would_fail_the_case(case, monkeypatch):
    ref = _ints(U.branch_oracle_run(case, 20)[1])
    got = _ints(_forced_run(case, monkeypatch, max_energy_diff=1000.0))
    assert got["depth"] != ref["depth"] or got["leapfrogs"] != ref["leapfrogs"]
    assert got["has_divergence"] != ref["has_divergence"]


def test_hmc_case_without_the_divergence_bound_accepts_what_it_rejected():
    case = U.branch_case("hmc_div")
    ref = _ints(U.branch_oracle_run(case, 20)[1])
    got = _ints(_plain(case, max_energy_diff=1000.0))
    assert got["is_accepted"] != ref["is_accepted"]


def test_hmc_case_has_an_inner_leaf_over_the_bound_in_a_transition_that_does_not_diverge(monkeypatch):
    """Fixed-L HMC tests the END state against max_energy_diff.  In chain 21 of ``hmc_div`` (the last chain of every batch) a transition's inner
    leaves exceed the bound while its end state does not: has_divergence = 0 there -- the device, which accumulated the flag over the leaves
    as NUTS does, reported 1 until this case ran."""
    case = U.branch_case("hmc_div")
    real, inner = orc.hmc_one_step, []

    def spy(q, cur_target, cur_grad, step_size, temp, fn_L, step, chain, key, num_leapfrog, max_energy_diff=1000.0):
        p = orc.rng_normal(q.shape[0], step, chain, key)
        e0, x, grd, worst = cur_target - 0.5 * np.dot(p, p), q, cur_grad, 0.0
        for it in range(num_leapfrog - 1):                                    # the same leapfrogs, energies of the inner leaves only
            ph = p + 0.5 * step_size * grd
            x = x + step_size * ph
            Lx, gLx = fn_L(x)
            grd = temp * gLx
            p = ph + 0.5 * step_size * grd
            worst = max(worst, -(temp * Lx - 0.5 * np.dot(p, p) - e0))
        inner.append(worst)
        return real(q, cur_target, cur_grad, step_size, temp, fn_L, step, chain, key, num_leapfrog, max_energy_diff)

    monkeypatch.setattr(orc, "hmc_one_step", spy)
    g, pr, _ = U.branch_problem(case)
    trace = []
    orc.sample_chain(pr, g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), case.results, case.burnin, seed=case.seed, chain=U.BRANCH_CHAINS[1],
                     trace=trace, **U.branch_oracle_kwargs(case))
    assert _ints(trace) == _ints(U.branch_oracle_run(case, U.BRANCH_CHAINS[1])[1])
    bound = case.cfg["max_energy_diff"]
    assert any(w >= bound + 0.01 and not r.has_divergence for w, (_, r, _) in zip(inner, trace))        # (0.01: far from the edge)


def _discrepancy(case):
    """{field: largest |numpy - C port| / device tolerance} over the case's two chains, and the largest |energy| difference."""
    worst, e_abs = {}, 0.0
    for chain in U.BRANCH_CHAINS:
        (oa, ta, _), (ob, tb, _) = U.branch_oracle_run(case, chain), U.branch_oracle_run(case, chain, "c")
        assert _ints(ta) == _ints(tb), (case.name, chain)
        fa, fb = _fields(oa, ta), _fields(ob, tb)
        for k, (rtol, atol) in U.BRANCH_TOL.items():
            a, b = fa[k], fb[k]
            fin = np.isfinite(a)
            np.testing.assert_array_equal(fin, np.isfinite(b))
            if k == "X":
                atol = atol * np.abs(b).max()
            d = np.abs(a - b)[fin] / (atol + rtol * np.abs(b)[fin])
            worst[k] = max(worst.get(k, 0.0), float(d.max()) if d.size else 0.0)
        ea, eb = (np.array([r.energy for _, r, _ in t]) for t in (ta, tb))
        e_abs = max(e_abs, float(np.abs(ea - eb).max()))
    return worst, e_abs


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_no_decision_of_the_case_sits_on_a_rounding_knife_edge(case):
    worst, e_abs = _discrepancy(case)
    print(case.name, "numpy vs C port, fraction of the device tolerance:", {k: f"{v:.1e}" for k, v in worst.items()}, f"|energy| {e_abs:.1e}")
    for k, v in worst.items():
        assert v <= 1e-2, (case.name, k, v)
    assert e_abs <= U.ENERGY_CPU_DISCREPANCY, (case.name, e_abs)


def test_the_energy_tolerance_absorbs_rounding_only():
    """ENERGY_TOL = (1e-8, 100 x the table's largest CPU-vs-CPU difference): if that came out looser than 1e-6 of |target_log_prob| it would absorb
    something other than rounding.  The scale is the chain's largest |target_log_prob|: on SIRW the tempered log posterior crosses zero while
    the terms it is summed from (and 0.5 p.p, ~ dim / 2) keep their size, so a single step's |target_log_prob| is no measure of the rounding."""
    rtol, atol = U.ENERGY_TOL
    assert atol == 100.0 * U.ENERGY_CPU_DISCREPANCY
    for case in CASES:
        for chain in U.BRANCH_CHAINS:
            _, trace, _ = U.branch_oracle_run(case, chain)
            scale = max(abs(r.target_log_prob) for _, r, _ in trace)
            loosest = max(atol + rtol * abs(r.energy) for _, r, _ in trace)
            print(case.name, chain, f"energy bound {loosest:.1e} = {loosest / scale:.1e} of max |target_log_prob| = {scale:.3g}")
            assert loosest <= 1e-6 * scale, (case.name, chain, loosest, scale)
