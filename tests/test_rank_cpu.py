"""What the device tolerances of tests/test_rank_gpu.py rest on, proven on the CPU (tests/rank_reference.py): the unit is wired in, the
ranks are scipy's average ranks, the z bar is four times what scipy's ndtri itself misses mpmath by, no truncation decision and no choice
between two legs of the fixture sits on a rounding edge, the float64 transcription agrees with the longdouble one inside the bars, and
each wrong definition misses a bar by >= 100 x."""
import os
import re
import warnings

import numpy as np
import pytest

import rank_reference as rr
import summary_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = ("rhat_rank", "ess_bulk", "ess_tail")
VARIANT_SHAPES = ((3, 257), (4, 1000))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_unit_is_declared_drift_free_and_mirrored():
    from magi_v2_amd import engine, jit
    header = _read("include", "magi_hip.h")
    for sym in ("magi_rank_diagnostics", "magi_sampler_rank_diagnostics"):
        assert re.search(r"\bint " + sym + r"\(magi_handle\* h,", header), sym
        assert sym in engine.exported_symbols()
    assert "rank.hip" in jit._DRIFT_FREE
    m = re.search(r"constexpr int RANK_LDS = (\d+);", _read("magi_v2_amd", "csrc", "rank.hip"))
    assert m and int(m.group(1)) == rr.RANK_LDS
    S = [C * R for C, R in rr.SHAPES]
    assert {rr.RANK_LDS - 1, rr.RANK_LDS, rr.RANK_LDS + 1} <= set(S)
    big = [(C, R) for C, R in rr.SHAPES if C * R > 2 * rr.RANK_LDS]
    assert big and all(C == 3 and (C * R) & (C * R - 1) for C, R in big)
    assert all(rr.lag_for(C, R) == (0 if C * R <= 4000 else 64) for C, R in rr.SHAPES)


@pytest.mark.parametrize("C, R", rr.SHAPES)
def test_ranks_are_scipys_average_ranks_and_signed_zeros_tie(C, R):
    from scipy.stats import rankdata
    y = rr.fixture(C, R)
    assert y.shape == (C, R, rr.K_FIXTURE) and rr.K_FIXTURE == 16
    for k in range(rr.K_FIXTURE):
        if k == sr.COL_NAN:
            continue
        flat = y[:, :, k].reshape(-1)
        np.testing.assert_array_equal(rr.rankdata(flat), rankdata(flat, method="average"), err_msg=str(k))
    pm0 = y[:, :, rr.COL_PM0].reshape(-1)
    zero = pm0 == 0.0
    assert np.any(np.signbit(pm0[zero])) and not np.all(np.signbit(pm0[zero]))
    assert len(set(rr.rankdata(pm0)[zero])) == 1                      # one rank for -0.0 and +0.0
    assert len(set(rr.rankdata(pm0, "ties_by_key")[zero])) == 2
    assert np.unique(pm0[~zero]).shape[0] == np.count_nonzero(~zero)  # its only ties


def test_the_z_bar_is_four_times_what_ndtri_itself_misses_mpmath_by():
    from scipy.special import ndtri
    worst = {}
    for C, R in rr.SHAPES:
        w = 0.0
        for c in rr.fixture_reference(C, R)["columns"]:
            if c["nonfinite"]:
                continue
            S = C * R
            for rank_of, exact in ((c["rank"], c["z_exact"]), (c["rank_f"], c["zf_exact"])):
                w = max(w, rr.z_error(ndtri(rr.fractions(rank_of.reshape(-1), S)), exact.reshape(-1)))
        worst[C * R] = round(w, 2)
    print("ndtri against mpmath, in U max(1, |z|), by S:", worst)
    top = max(worst.values())
    assert rr.Z_ERR_NDTRI / 2 <= top <= rr.Z_ERR_NDTRI, worst             # the constant is the measurement, rounded up
    assert rr.Z_BAR == 4.0 * rr.Z_ERR_NDTRI
    # the exact scores are odd in p - 1/2 and increase with p
    p = np.array([0.625 / (2 ** 22 + 0.25), 1e-3, 0.25, 0.5, 0.75])
    x = rr.phi_inv_exact(p)
    assert x[3] == 0 and x[4] == -x[2] and np.all(np.diff(x) > 0) and abs(float(x[0]) + 5.3) < 0.2


@pytest.mark.parametrize("C, R", rr.SHAPES)
def test_no_decision_of_the_fixture_sits_on_a_rounding_edge(C, R):
    ref = rr.fixture_reference(C, R)
    cols = ref["columns"]
    assert ref["n_nonfinite"] == 1 and cols[sr.COL_NAN]["nonfinite"]
    n_diag = 0
    for k, c in enumerate(cols):
        if c["nonfinite"]:
            continue
        for name in rr.SERIES:
            leg = c["legs"][name]
            if leg["kstar"] is None or np.isnan(leg["rhat"]):        # a constant series, or split chains that are all one constant (the
                continue                                              # dropped middle draw of an odd R differs): no diagnostics by design
            n_diag += 1
            print(C, R, k, name, "K*", leg["kstar"], "min|P|", leg["min_abs_P"], "|tau - floor|", leg["tau_gap"], "kappa", leg["kappa"])
            assert leg["min_abs_P"] > 1e-6, (k, name, leg["min_abs_P"])
            assert leg["tau_gap"] > 1e-6, (k, name, leg["tau_gap"])
            assert leg["kappa"] <= 1e7, (k, name)
        for a, b, what in ((c["legs"]["z"]["rhat"], c["legs"]["zf"]["rhat"], "max"), (c["legs"]["lo"]["ess"], c["legs"]["hi"]["ess"], "min")):
            if np.isfinite(a) and np.isfinite(b):
                # the two legs are the same number but for their rounding (a handful of draws: the same scores in another order, or tau
                # at its floor in both) -- a turn of the choice moves the result by |a - b|, 1e-4 of the smallest bar --, or the choice
                # is not within 1e-6 of turning
                gap = abs(a - b) / max(abs(a), abs(b))
                assert gap <= 1e-15 or gap > 1e-6, (k, what, float(a), float(b))
    assert n_diag >= 4 * (rr.K_FIXTURE - 3) - 8 or C * R < 10
    assert np.isnan(cols[sr.COL_CONST]["rhat_rank"]) and np.isnan(cols[sr.COL_CONST]["ess_bulk"]) and np.isnan(cols[sr.COL_CONST]["ess_tail"])
    top = cols[rr.COL_TOP]
    assert np.isnan(top["ess_tail"]) and top["legs"]["hi"]["kstar"] is None        # its upper indicator is constant
    if R >= 4:
        assert np.isfinite(top["ess_bulk"])


def test_fixture_behaves_as_the_definitions_promise():
    C, R = 4, 1000
    cols = rr.fixture_reference(C, R)["columns"]
    classic = sr.column(rr.fixture(C, R)[:, :, rr.COL_SCALE], ())
    assert abs(classic["rhat"] - 1) < 0.01                            # equal means: the moment-based R-hat sees nothing
    assert cols[rr.COL_SCALE]["legs"]["zf"]["rhat"] > 1.1 and cols[rr.COL_SCALE]["rhat_rank"] == cols[rr.COL_SCALE]["legs"]["zf"]["rhat"]
    assert abs(cols[rr.COL_SCALE]["legs"]["z"]["rhat"] - 1) < 0.01
    assert abs(cols[rr.COL_CAUCHY]["rhat_rank"] - 1) < 0.01 and cols[rr.COL_CAUCHY]["ess_bulk"] > 2000     # heavy tails do not hurt ranks
    assert cols[sr.COL_OFFSET]["rhat_rank"] > 2
    tied = cols[rr.COL_TIED]
    assert np.unique(rr.fixture(C, R)[:, :, rr.COL_TIED]).shape[0] <= 10 and np.isfinite(tied["ess_bulk"]) and np.isfinite(tied["ess_tail"])
    assert np.all(tied["rank"] * 2 == np.rint(tied["rank"] * 2))
    assert cols[sr.PHIS.index(0.99)]["ess_tail"] < cols[sr.PHIS.index(0.0)]["ess_tail"]


@pytest.mark.parametrize("C, R", rr.SHAPES)
def test_float64_transcription_agrees_with_longdouble_inside_the_bars(C, R):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # (W = 0 in a series of a handful of draws: rhat = inf in both)
        got = rr.diagnostics(rr.fixture(C, R), rr.lag_for(C, R), dtype=np.float64)
        worst = rr.check_against(got, rr.fixture_reference(C, R), rr.fixture_bars(C, R))
    print(C, R, "worst error / bar:", worst)
    assert all(w <= 0.01 for s, w in worst.items() if s in DIAG), worst          # (the headroom the bars were derived with)
    assert all(w <= 0.25 for s, w in worst.items() if s not in DIAG), worst      # ndtri itself: a quarter of the device's bar


@pytest.mark.parametrize("variant", rr.VARIANTS)
def test_a_wrong_definition_misses_a_bar_by_two_orders_of_magnitude(variant):
    best = 0.0
    for C, R in VARIANT_SHAPES:
        ref, bars = rr.fixture_reference(C, R), rr.fixture_bars(C, R)
        bad = rr.diagnostics(rr.fixture(C, R), rr.lag_for(C, R), variant=variant)
        for k, (c, cb) in enumerate(zip(ref["columns"], bad["columns"])):
            if bars[k] is None:
                continue
            for s in DIAG:
                r, b = c[s], cb[s]
                if np.isnan(r) != np.isnan(b):
                    miss = np.inf                                     # a diagnostic where there is none: no bar admits it
                elif np.isnan(r):
                    continue
                else:
                    miss = float(abs(b - r) / abs(r)) / bars[k][s]
                if miss > best:
                    best, where = miss, (C, R, k, s)
    print(variant, "misses by", best, "bars at", where)
    assert best >= 100.0, (variant, best)


def test_the_warning_names_the_columns_beyond_the_thresholds():
    from magi_v2_amd import host
    block = lambda rh, eb, et: dict(rhat_rank=np.array(rh), ess_bulk=np.array(eb), ess_tail=np.array(et))
    rank = dict(X=block([[1.0, 1.02], [np.nan, 1.005]], [[500.0, 150.0], [np.nan, 900.0]], [[450.0, 450.0], [np.nan, 10.0]]),
                sigma_sqs=block([1.0, 1.0], [400.0, 401.0], [400.0, 400.0]), thetas=block([1.5], [20.0], [np.nan]))
    summary = {b: {"mean": np.zeros(np.shape(rank[b]["rhat_rank"]))} for b in host.RANK_BLOCKS}
    assert host.merge_rank_diagnostics(summary, rank) is summary and set(summary["X"]) == {"mean"} | set(host.RANK_KEYS)
    flags = host.rank_diagnostics_flags(summary, 2)
    assert flags == {"X": dict(rhat_rank=1, ess_bulk=1, ess_tail=1), "sigma_sqs": dict(rhat_rank=0, ess_bulk=0, ess_tail=0),
                     "thetas": dict(rhat_rank=1, ess_bulk=1, ess_tail=0)}
    with pytest.warns(UserWarning, match=r"X: 1 with rhat_rank > 1.01, 1 with ess_bulk and 1 with ess_tail < 200; thetas: 1 with rhat_rank"):
        assert host.warn_rank_diagnostics(summary, 2) == flags
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host.warn_rank_diagnostics({b: rank["sigma_sqs"] for b in host.RANK_BLOCKS}, 4)
