"""What the device tolerances of tests/test_summary_gpu.py rest on, proven on the CPU (tests/summary_reference.py): no truncation decision
of the fixture sits on a rounding edge, the columns' conditioning stays inside what the tolerances assume, the float64 transcription agrees
with the longdouble one at those tolerances, order statistics and quantiles are numpy's, and a wrong definition misses by >= 100 x."""
import numpy as np
import pytest

import summary_reference as sr

DIAG_SHAPES = [s for s in sr.SHAPES if s[1] >= 4]


def _diag_columns(C, R):
    return [(k, c) for k, c in enumerate(sr.fixture_reference(C, R)["columns"]) if c["kstar"] is not None]


@pytest.mark.parametrize("C, R", sr.SHAPES)
def test_fixture_has_the_special_columns_and_no_decision_on_a_rounding_edge(C, R):
    ref = sr.fixture_reference(C, R)
    cols = ref["columns"]
    assert len(cols) == sr.K_FIXTURE == 11 and ref["n_nonfinite"] == 1 and cols[sr.COL_NAN]["nonfinite"]
    assert cols[sr.COL_CONST]["sd"] == 0 and np.isnan(cols[sr.COL_CONST]["rhat"]) and np.isnan(cols[sr.COL_CONST]["ess"])
    diag = _diag_columns(C, R)
    assert len(diag) == sr.K_FIXTURE - 2
    for k, c in diag:
        print(C, R, k, "K*", c["kstar"], "min|P|", c["min_abs_P"], "|tau - floor|", c["tau_gap"], "kappa", c["kappa"], "ess", float(c["ess"]),
              "rhat", float(c["rhat"]))
        assert c["min_abs_P"] > 1e-6, (k, c["min_abs_P"])
        assert c["tau_gap"] > 1e-6, (k, c["tau_gap"])
        assert c["kappa"] <= 1e7, (k, c["kappa"])


def test_fixture_behaves_as_the_definition_promises():
    cols = sr.fixture_reference(4, 1000)["columns"]
    Mn = 4000
    assert cols[sr.PHIS.index(-0.9)]["ess"] > Mn                     # antithetic: better than independent draws
    assert 3 < cols[sr.PHIS.index(0.99)]["ess"] < 200
    assert cols[sr.COL_OFFSET]["rhat"] > 2
    assert all(abs(cols[j]["rhat"] - 1) < 0.05 for j in (0, 1, 4, 5, 6))
    assert sr.fixture_reference(1, 64)["columns"][sr.COL_OFFSET]["rhat"] > 1.2      # one chain whose halves differ: the split sees it


@pytest.mark.parametrize("C, R", sr.SHAPES)
def test_float64_transcription_agrees_with_longdouble_at_the_device_tolerances(C, R):
    got = sr.summarize(sr.fixture(C, R), dtype=np.float64)
    got["probs"] = sr.PROBS
    worst = sr.check_against(got, sr.fixture_reference(C, R))
    print(C, R, worst)
    assert all(w <= 0.01 for s, w in worst.items() if s != "quantiles"), worst       # (the headroom the tolerances were derived with)


@pytest.mark.parametrize("C, R", sr.SHAPES)
def test_order_statistics_are_numpys_sort_and_quantiles_numpys_linear_method(C, R):
    y = sr.fixture(C, R)
    probs = (0.0, 0.025, 0.25, 0.5, 0.9, 0.975, 1.0)
    for k in range(sr.K_FIXTURE):
        if k == sr.COL_NAN:
            continue
        pooled = y[:, :, k].reshape(-1)
        c = sr.column(y[:, :, k], probs)
        np.testing.assert_array_equal(c["order"], np.sort(pooled))
        want = np.quantile(pooled, probs)
        err = np.abs(c["quantiles"].astype(np.float64) - want)
        assert np.all(err <= 4 * np.spacing(np.abs(want))), (k, err)
        assert c["quantiles"][0] == pooled.min() and c["quantiles"][-1] == pooled.max()


@pytest.mark.parametrize("variant", sr.VARIANTS)
@pytest.mark.parametrize("C, R", DIAG_SHAPES)
def test_a_wrong_definition_misses_the_tolerance_by_two_orders_of_magnitude(C, R, variant):
    ref = sr.fixture_reference(C, R)
    bad = sr.summarize(sr.fixture(C, R), variant=variant)
    miss, floor_both = {}, []
    for (k, c), cb in zip(_diag_columns(C, R), [b for b in bad["columns"] if b["kstar"] is not None]):
        rt = sr.rtol_spread(c["kappa"])
        if c["tau_at_floor"] and cb["tau_at_floor"]:
            # tau is the floor 1 / log10(M n) under both definitions (with the variant's M n where it differs): the ESS cannot tell
            # them apart on such a column, whatever the tolerance
            floor_both.append(k)
        else:
            miss["ess", k] = float(abs(bad["ess"][k] - ref["ess"][k]) / abs(ref["ess"][k]) / rt)
        if variant == "no_split":
            miss["rhat", k] = float(abs(bad["rhat"][k] - ref["rhat"][k]) / abs(ref["rhat"][k]) / rt)
    print(C, R, variant, "miss in tolerances:", {k: "%.3g" % v for k, v in miss.items()}, "tau at the floor under both:", floor_both)
    assert len(miss) >= 1
    for key, m in miss.items():
        assert m >= 100.0, (key, m)


def test_max_lag_truncates_and_nonpositive_means_all():
    y = sr.fixture(4, 1000)[:, :, 3]                                  # phi = 0.99: K* lies far out
    full, cut = sr.column(y), sr.column(y, max_lag=5)
    assert full["kstar"] > 3 and cut["kstar"] == 3 and cut["ess"] > full["ess"]
    assert sr.column(y, max_lag=-1)["ess"] == full["ess"] == sr.column(y, max_lag=10 ** 6)["ess"]
