"""What the device comparisons of tests/test_ppc_gpu.py rest on, proven on the CPU (tests/ppc_reference.py): the reference is calibrated on
data generated from the model itself and sees a misfit, the bars are 100 x the float64 / longdouble distance of the reference over the
GPU fixture table, no fixture decides a p-value on a rounding edge, and every named fault of a definition moves a compared quantity by
at least 1000 bars on some fixture -- so the device tests can fail for the right reasons.  Then the host side: ``host.ppc_result`` and its
``pit_ks``, and the header's definition text."""
import os

import numpy as np
import pytest

import ppc_reference as pr
from oracle import magi_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself --------------------------------------------------------------------------------------------------------------------

def test_the_noise_is_the_arithmetic_of_the_oracles_box_muller_on_a_stream_of_its_own():
    """With the momentum stream in place of STREAM_PPC, z0 and z1 of row r, chain c are the even and odd normals of the oracle's
    rng_normal(., step = r, chain = c): the same counter layout and Box-Muller arithmetic.  The stream itself is a sixth one."""
    assert pr.STREAM_PPC == 5 and pr.STREAM_PPC not in (orc.STREAM_MOMENTUM, orc.STREAM_DIRECTION, orc.STREAM_LEAF, orc.STREAM_MERGE, orc.STREAM_HMC)
    z0, z1, _ = pr.noise(2, 3, 9, seed=77, chain_ids=[4, 1], dtype=np.float64, fault="stream_momentum")
    for s, (c, r) in enumerate([(4, 0), (4, 1), (4, 2), (1, 0), (1, 1), (1, 2)]):
        z = orc.rng_normal(18, r, c, 77)
        np.testing.assert_array_equal(z0[s], z[0::2])
        np.testing.assert_array_equal(z1[s], z[1::2])
    own = pr.noise(2, 3, 9, seed=77, chain_ids=[4, 1], dtype=np.float64)[0]
    assert not np.any(own == z0)


def test_the_longdouble_erfc_agrees_with_scipy_to_float64_accuracy():
    """(to 1e-14 relative: scipy's own float64 erfc carries the rounding of x^2 in e^(-x^2), a few ulp times x^2 at |x| = 8)"""
    from scipy.special import erfc
    x = np.concatenate([np.linspace(-8.0, 8.0, 801), [1.999999, 2.0, 2.000001, 0.0, 1e-300]])
    got, want = pr.erfc(x.astype(np.longdouble)).astype(np.float64), erfc(x)
    assert np.all(np.abs(got - want) <= 1e-14 * want), float(np.max(np.abs(got - want) / want))
    assert np.isnan(pr.erfc(np.array([np.nan], dtype=np.longdouble))[0])


def _calibrated(misfit):
    c = pr.calibration_data(misfit)
    return c, pr.ppc(dtype=np.float64, **c)


def test_on_data_generated_from_the_model_the_check_is_calibrated():
    """n_obs = 400 over two components, S = 512, the seeds of ppc_reference.CALIBRATION: the Kolmogorov distance of the PIT values from
    uniform stays below the alpha = 0.001 critical value 1.95 / sqrt(n) per component, and every p-value inside [0.01, 0.99]."""
    from magi_v2_amd import host
    c, r = _calibrated(False)
    assert c["x"].shape == (2, 256, 400)
    ks = host.pit_ks(r["pit"].astype(np.float64), c["comp"], 2)
    n = pr.CALIBRATION["n_per_component"]
    print("pit_ks", ks, "critical", 1.95 / np.sqrt(n), "p-values", r["pval"].tolist())
    assert np.all(ks < 1.95 / np.sqrt(n))
    assert np.all((r["pval"] >= 0.01) & (r["pval"] <= 0.99))
    assert r["n_T_excluded"].tolist() == [0, 0] and r["n_nonfinite"] == 0


def test_a_sinusoidal_misfit_of_two_noise_sd_is_seen_by_acf1():
    _, r = _calibrated(True)
    print("p-values under the misfit", r["pval"].tolist())
    assert np.all(r["pval"][:, pr.STATS.index("acf1")] < 0.01)


# ---- the bars ----------------------------------------------------------------------------------------------------------------------------------

def _table_distance():
    worst = {q: 0.0 for q in pr.COMPARED}
    for f in pr.FIXTURES:
        d = pr.distance(pr.crafted_reference(*f, long=False), pr.crafted_reference(*f))
        for q, v in d.items():
            worst[q] = max(worst[q], v)
    return worst


def test_bars_are_100_x_the_float64_longdouble_distance_over_the_fixture_table():
    """Each constant of ppc_reference.BAR is MARGIN (100) x the largest float64 / longdouble distance of the reference over FIXTURES, in the
    units of the scale the reference states per entry, rounded up by at most a quarter."""
    worst = _table_distance()
    print({q: f"{pr.MARGIN * v:.3e}" for q, v in worst.items()})
    for q in pr.COMPARED:
        assert np.isfinite(worst[q]) and worst[q] > 0.0
        assert pr.MARGIN * worst[q] <= pr.BAR[q] <= 1.25 * pr.MARGIN * worst[q], (q, worst[q])


@pytest.mark.parametrize("C,R,K,domain", pr.FIXTURES)
def test_no_fixture_decides_a_p_value_on_a_rounding_edge_and_only_the_domain_case_excludes_draws(C, R, K, domain):
    """pval and n_T_excluded are compared exactly: for every fixture, draw, component and statistic |T_rep - T_obs| exceeds 1000 x the
    bars of the two, the float64 and the longdouble reference count alike, and the excluded draws are those the table states."""
    f, a, b = pr.crafted(C, R, K, domain), pr.crafted_reference(C, R, K, domain), pr.crafted_reference(C, R, K, domain, long=False)
    margin = pr.knife_edge(a) / max(pr.BAR["T_obs"], pr.BAR["T_rep"])
    print("smallest |T_rep - T_obs| in bars:", margin)
    assert margin >= 1000.0
    np.testing.assert_array_equal(a["pval"], b["pval"])
    assert a["n_T_excluded"].tolist() == b["n_T_excluded"].tolist() == f["n_excluded"].tolist()
    assert (a["n_T_excluded"].sum() > 0) == domain
    assert np.all(np.isnan(a["pval"][1])) and np.all(np.isnan(a["T_obs"][:, 1]))          # component 1 owns no column
    single = 0 if K == 1 else 2                                                           # the component with a single datum
    assert np.isnan(a["pval"][single, 3]) and np.all(np.isfinite(a["pval"][single, :3]))
    if domain:
        bad = np.zeros(C * R, dtype=bool)
        bad[list(pr.DOMAIN_DRAWS)] = True
        assert np.array_equal(~np.isfinite(a["T_obs"][:, 0, 0].astype(np.float64)), bad)
        assert np.array_equal(np.isnan(a["y_rep"][:, pr.DOMAIN_COLUMN].astype(np.float64)), bad) and a["n_nonfinite"] == 1
        assert np.isnan(a["pit"][pr.DOMAIN_COLUMN])
    else:
        assert a["n_nonfinite"] == 0


def test_the_table_holds_every_case_the_device_test_needs():
    fs = [pr.crafted(*f) for f in pr.FIXTURES]
    assert {(f["x"].shape[0], f["x"].shape[1]) for f in fs} == set(pr.SHAPES) and {f["x"].shape[2] for f in fs} == set(pr.KS)
    assert {int(l) for f in fs for l in f["link"][[0, 2]]} == {0, 1, 2}
    assert any(f["extra_var"] is None for f in fs) and any(f["extra_var"] is not None for f in fs)
    assert any(f["chain_ids"] is None for f in fs) and any(f["chain_ids"] is not None and len(f["chain_ids"]) == 3 for f in fs)
    assert any(f["fixed"] for f in fs)
    assert all(set(np.unique(f["weight"])) <= {1.0, 2.0, 4.0} for f in fs) and any(np.isnan(f["y"]).any() for f in fs)
    assert len(pr.FIXTURES) == len(pr.SHAPES) * len(pr.KS) + 1 and pr.FIXTURES[-1] == pr.DOMAIN + (True,)


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fault", pr.FAULTS)
def test_every_named_fault_moves_a_compared_quantity_by_1000_bars_on_some_fixture(fault):
    """The float64 reference with one definition deliberately wrong against the longdouble reference, at the device bars: some compared
    quantity of some fixture moves by at least 1000 x its bar (a changed pattern of non-finite entries counts as infinitely far)."""
    best, where = 0.0, None
    for f in pr.FIXTURES:
        d = pr.distance(pr.crafted_reference(*f, long=False, fault=fault), pr.crafted_reference(*f))
        q = max(d, key=lambda s: d[s] / pr.BAR[s])
        if d[q] / pr.BAR[q] > best:
            best, where = d[q] / pr.BAR[q], (f, q)
    print(fault, "moves", where, "by", best, "bars")
    assert best >= 1000.0


# ---- the host side -----------------------------------------------------------------------------------------------------------------------------

def test_pit_ks_is_the_kolmogorov_distance_per_component():
    from magi_v2_amd import host
    from scipy.stats import kstest
    rng = np.random.default_rng(5)
    pit = rng.random(90)
    comp = np.repeat([0, 2], 45)
    pit[7] = np.nan                                                   # a column without a datum does not count
    ks = host.pit_ks(pit, comp, 3)
    for d in (0, 2):
        p = pit[(comp == d) & np.isfinite(pit)]
        assert ks[d] == pytest.approx(kstest(p, "uniform").statistic, rel=0, abs=1e-15)
    assert np.isnan(ks[1])
    assert host.pit_ks(np.array([0.25]), [0], 1)[0] == 0.75
    assert host.pit_ks(np.full(4, 0.5), np.zeros(4), 1)[0] == 0.5


def test_ppc_result_assembles_the_dictionary():
    from magi_v2_amd import host
    f = pr.crafted(2, 33, 65)
    r = pr.crafted_reference(2, 33, 65, long=False)
    S, K, D = 66, 65, 3
    idx = np.stack([np.arange(K), f["comp"]], axis=1)
    out = host.ppc_result(f["comp"], D, r["mean"], r["sd"], r["quantiles"], r["pit"], r["pval"], r["n_T_excluded"], r["n_nonfinite"], obs_index=idx,
                          probs=np.asarray(pr.PROBS), y_rep=r["y_rep"].reshape(2, 33, K), T_obs=r["T_obs"].reshape(2, 33, D, 4))
    assert list(out)[:3] == ["obs_index", "comp", "n_obs"] and out["n_obs"] == K and out["obs_index"].shape == (K, 2)
    assert set(out["pvalues"]) == set(host.PPC_STATS) == {"chi2", "mean", "maxabs", "acf1"}
    for t, s in enumerate(host.PPC_STATS):
        np.testing.assert_array_equal(out["pvalues"][s], r["pval"][:, t])
    assert out["y_rep"].shape == (2, 33, K) and out["T_obs"].shape == (2, 33, D, 4) and "T_rep" not in out
    assert out["n_T_excluded"].tolist() == [0, 0, 0] and out["n_nonfinite"] == 0 and out["quantiles"].shape == (3, K)
    np.testing.assert_array_equal(out["pit_ks"], host.pit_ks(r["pit"], f["comp"], D))
    assert np.isnan(out["pit_ks"][1]) and 0.0 < out["pit_ks"][0] <= 1.0
    lean = host.ppc_result(f["comp"], D, r["mean"], r["sd"], r["quantiles"], r["pit"], r["pval"], r["n_T_excluded"])
    assert "y_rep" not in lean and "T_obs" not in lean and lean["obs_index"] is None


def test_the_header_states_the_definitions_and_the_engine_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    for words in ("int magi_ppc(", "int magi_sampler_ppc(", "STREAM_PPC = 5", "max(gy_rep, 0)^2", "1/2 erfc(-u_obs[s][k] / sqrt 2)", "n_T_excluded"):
        assert words in text, words
    internal = open(os.path.join(ROOT, "magi_v2_amd", "csrc", "magi_internal.h")).read()
    assert "STREAM_MOMENTUM = 0, STREAM_DIRECTION = 1, STREAM_LEAF = 2, STREAM_MERGE = 3, STREAM_HMC = 4" in internal and "STREAM_PPC = 5" in internal
    from magi_v2_amd import engine, jit
    assert {"magi_ppc", "magi_sampler_ppc"} <= set(engine.exported_symbols())
    assert "ppc.hip" in jit._DRIFT_FREE
