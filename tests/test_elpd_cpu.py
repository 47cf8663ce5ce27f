"""What the device comparisons of tests/test_elpd_gpu.py rest on, proven on the CPU (tests/elpd_reference.py): the bars are the float64 /
longdouble distance of the reference times a stated margin, no fixture sits on a rounding edge of a decision, and every named fault of a
definition moves a compared output by at least 1000 bars on some fixture -- so the device tests can fail for the right reasons.  Then the
host side: totals, ``compare_elpd``, ``scale="data"``, and the header's definition text."""
import math
import os

import numpy as np
import pytest

import elpd_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in er.SHAPES if s[0] * s[1] <= 5000]


def _distance(a, b, k, s):
    """|longdouble - float64| of output s of column k in the units check_against divides by."""
    c = a["columns"][k]
    return float(abs(a[s][k] - np.longdouble(b[s][k]))) / c["scale"]


@pytest.mark.parametrize("C,R", er.SHAPES)
def test_bars_are_the_float64_longdouble_distance_times_the_margin(C, R):
    """One rule per output: BAR[out] x max(1, max|l|).  On every fixture of the GPU table MARGIN (64) x the float64 / longdouble distance of
    the reference stays inside the bar, and the bar is at least FLOOR_ULP ulp of the scale.  The margin covers what the device does
    differently from numpy at the same precision: its own log / exp / log1p / expm1, and sums in 256 lane-strided partials instead of
    pairwise ones."""
    a, b = er.crafted_reference(C, R, True), er.crafted_reference(C, R, False)
    assert a["n_nonfinite"] == b["n_nonfinite"] == 2
    worst = {}
    for k, c in enumerate(a["columns"]):
        for s in er.OUTPUTS:
            x, y = a[s][k], b[s][k]
            if not np.isfinite(x):
                assert (np.isnan(x) and np.isnan(y)) or x == y, (s, k)
                continue
            worst[s] = max(worst.get(s, 0.0), _distance(a, b, k, s))
    print(C * R, {s: f"{v:.2e}" for s, v in worst.items()})
    for s, v in worst.items():
        assert er.MARGIN * v <= er.BAR[s], (s, v)
        assert er.BAR[s] >= er.FLOOR_ULP * 2 * er.U


def test_the_bars_are_not_loose():
    """Each bar is within a factor 2 of MARGIN x the largest float64 / longdouble distance over the whole fixture table."""
    worst = {}
    for C, R in er.SHAPES:
        a, b = er.crafted_reference(C, R, True), er.crafted_reference(C, R, False)
        for k in range(er.K_CRAFTED):
            for s in er.OUTPUTS:
                if np.isfinite(a[s][k]):
                    worst[s] = max(worst.get(s, 0.0), _distance(a, b, k, s))
    print({s: f"{v:.3e}" for s, v in worst.items()})
    for s in er.OUTPUTS:
        assert er.MARGIN * worst[s] <= er.BAR[s] <= 2.0 * er.MARGIN * worst[s], (s, worst[s])


@pytest.mark.parametrize("C,R", er.SHAPES)
def test_no_fixture_sits_on_a_rounding_edge(C, R):
    S = C * R
    M = er.tail_length(S)
    # M and m are exact integers of S: 3 sqrt(S) is an integer (9 S a square) or at least 1e-6 from one; likewise sqrt(M)
    for v in (9 * S, M):
        t = math.isqrt(v)
        assert t * t == v or min(math.sqrt(v) - t, t + 1 - math.sqrt(v)) > 1e-6, v
    assert M == min(S // 5, math.ceil(3 * math.sqrt(S))) and M <= 2048
    ref = er.crafted_reference(C, R, True)
    kh = ref["khat"]
    names = er.COLUMNS
    for k, c in enumerate(ref["columns"]):
        if c["gap"] is not None:
            assert c["gap"] > 1e-6, (names[k], c["gap"])          # (the ties placed on purpose have distance 0 and are not counted)
    if M < 5:
        assert all(np.isinf(kh[k]) for k in range(len(names)) if not ref["columns"][k]["nonfinite"])
        return
    assert np.isinf(kh[names.index("constant")]) and np.isinf(kh[names.index("tied_tail")])
    assert np.isnan(kh[names.index("nan")]) and np.isnan(kh[names.index("neg_inf")])
    if S >= 2048:                                         # (the classes of the issue; a tail of 5 or 20 draws does not resolve them)
        assert kh[names.index("light")] < 0.5 and 0.7 < kh[names.index("z2")] < 1.3 and kh[names.index("heavy")] > 3.0
    # the straddling ties: the draw just below the tail carries the tail's smallest ratio
    l = er.crafted(C, R).reshape(S, -1)[:, names.index("straddle")]
    r = er.log_ratios(l)
    o = er.tail_order(r)
    assert r[o[S - M - 1]] == r[o[S - M]] == r[o[S - M + 1]] and o[S - M - 1] < o[S - M] < o[S - M + 1]


def test_the_bound_of_the_tail_sort():
    assert er.tail_length(er.LOO_MAX_S) == 2048 and er.tail_length(er.LOO_MAX_S + 1) == 2049
    assert er.LOO_MAX_S >= 2 ** 16


@pytest.mark.parametrize("fault", er.FAULTS)
def test_every_named_fault_of_the_statistics_is_seen(fault):
    """Applied to the reference, the fault moves a compared output by at least 1000 bars on at least one small fixture.  The exception is
    proven instead: ties ordered by DESCENDING index cannot move any output -- tied draws have equal l and equal r, so which of them sits
    inside the tail changes no term of either sum (only their order) -- and what the index order buys is bit-identical results."""
    best = 0.0
    for C, R in SMALL:
        good, bad = er.crafted_reference(C, R, True), er.elpd(er.crafted(C, R), fault=fault)
        for k, c in enumerate(good["columns"]):
            if c["nonfinite"]:
                continue
            for s in er.OUTPUTS:
                g, b = good[s][k], bad[s][k]
                if np.isfinite(g) != np.isfinite(b):
                    best = np.inf
                elif np.isfinite(g):
                    best = max(best, float(abs(g - b)) / (er.BAR[s] * c["scale"]))
    print(fault, best)
    if fault == "ties_desc_index":
        assert best <= 1.0
    else:
        assert best >= 1000.0


# ---- the log-likelihood of draws ---------------------------------------------------------------------------------------------------------------

def _draws():
    """Draws around data on N = 9 points, D = 3: component 0 under a log link, 1 under sqrt with a fixed variance and NaN-masked entries,
    2 the identity with one point observed; weights 1 / 2 / 4; a non-default LB."""
    rng = np.random.default_rng(5)
    N, D, C, R = 9, 3, 2, 6
    truth = 0.5 + 0.4 * np.sin(np.arange(N)[:, None] * 0.7 + np.arange(D)[None, :])
    y = truth * np.exp(0.05 * rng.standard_normal((N, D)))
    y[1::2, 1] = np.nan
    y[:, 2] = np.nan
    y[4, 2] = truth[4, 2]
    X = truth[None, None] * np.exp(0.03 * rng.standard_normal((C, R, N, D)))
    sig_pre = rng.standard_normal((C, R, D)) - 5.0
    W = rng.choice([1.0, 2.0, 4.0], size=(N, D))
    return X, sig_pre, y, np.array([1e-4, 2e-4, 3e-4]), np.array([1, 2, 0]), W, {1: 2.5e-3}


def test_the_log_likelihood_bar_and_its_faults():
    X, sp, y, LB, links, W, fixed = _draws()
    ref, idx, cond = er.loglik(X, sp, y, LB, links, W, fixed)
    f64, idx64, _ = er.loglik(X, sp, y, LB, links, W, fixed, dtype=np.float64)
    assert idx.tolist() == idx64.tolist() == sorted(idx.tolist(), key=lambda p: p[1] * 9 + p[0]) and len(idx) == 9 + 5 + 1
    bar = er.loglik_bar(ref, cond)
    worst = float((np.abs(ref - f64.astype(np.longdouble)).astype(np.float64) / bar).max())
    print("float64 / longdouble distance of the log-likelihood, fraction of its bar:", worst)
    assert worst <= 0.25
    for fault in er.LL_FAULTS:
        bad, bidx, _ = er.loglik(X, sp, y, LB, links, W, fixed, fault=fault)
        if fault == "nan_counted":
            assert bad.shape[2] == 27 != ref.shape[2]
            continue
        moved = float((np.abs(bad - ref).astype(np.float64) / bar).max())
        print(fault, moved)
        assert moved >= 1000.0, fault


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------------

def _result(elpd_loo, khat=None, idx=None, scale="link", shift=None):
    from magi_v2_amd import host
    e = np.asarray(elpd_loo, dtype=np.float64)
    n = e.shape[0]
    point = {"lpd": e + 0.5, "p_waic": np.full(n, 0.25), "elpd_waic": e + 0.25, "elpd_loo": e, "p_loo": np.full(n, 0.5),
             "khat": np.zeros(n) if khat is None else np.asarray(khat, dtype=np.float64)}
    return host.elpd_result(point, np.stack([np.arange(n), np.zeros(n, dtype=int)], axis=1) if idx is None else idx, 0, shift=shift, scale=scale)


def test_totals_and_compare_elpd_against_hand_computed_values():
    from magi_v2_amd import host
    a = _result([-1.0, -2.0, -3.0, -6.0], khat=[0.1, 0.8, 0.71, 0.7])
    assert a["elpd_loo"] == -12.0 and a["n_obs"] == 4 and a["n_khat_bad"] == 2 and a["p_loo"] == 2.0 and a["elpd_waic"] == -11.0
    # var(ddof 1) of (-1, -2, -3, -6) = 14 / 3; se = sqrt(4 * 14 / 3)
    assert a["se_elpd_loo"] == pytest.approx(math.sqrt(56.0 / 3.0), rel=1e-15) and a["se_p_loo"] == 0.0
    b = _result([-1.5, -1.0, -3.5, -7.0])
    rows = host.compare_elpd({"a": a, "b": b})
    assert [r["name"] for r in rows] == ["a", "b"] and rows[0]["elpd_diff"] == 0.0 and rows[0]["se_diff"] == 0.0
    # differences b - a = (-0.5, 1, -0.5, -1): sum -1, var(ddof 1) = (0.0625 + 1.5625 + 0.0625 + 0.5625) / 3 = 0.75; se = sqrt(4 * 0.75)
    assert rows[1]["elpd_diff"] == -1.0 and rows[1]["se_diff"] == pytest.approx(math.sqrt(3.0), rel=1e-15) and rows[1]["elpd"] == -13.0
    assert rows[0]["n_khat_bad"] == 2 and rows[1]["p"] == 2.0
    waic = host.compare_elpd({"a": a, "b": b}, kind="waic")
    assert waic[1]["elpd_diff"] == -1.0 and waic[0]["n_khat_bad"] is None
    other = _result([-1.0, -2.0, -3.0, -6.0], idx=np.array([[0, 0], [1, 0], [2, 0], [4, 0]]))
    with pytest.raises(ValueError, match="obs_index"):
        host.compare_elpd({"a": a, "other": other})
    with pytest.raises(ValueError, match="obs_index"):
        host.compare_elpd({"a": a, "short": _result([-1.0, -2.0])})
    with pytest.raises(ValueError, match="scale"):
        host.compare_elpd({"a": a, "data": _result([-1.0, -2.0, -3.0, -6.0], scale="data")})
    with pytest.raises(ValueError):
        host.compare_elpd({"a": a}, kind="dic")


def test_scale_data_adds_the_links_log_jacobian():
    from magi_v2_amd import host
    X = np.array([[2.0, 4.0, 3.0], [np.nan, 9.0, 1.0], [0.5, np.nan, 7.0]])
    idx = np.array([[0, 0], [2, 0], [0, 1], [1, 1], [0, 2], [1, 2], [2, 2]])
    j = host.elpd_jacobian(host.obs_model_spec(["log", "sqrt", "identity"], 3), X, idx)
    np.testing.assert_allclose(j, [-math.log(2.0), -math.log(0.5), -math.log(4.0), -math.log(6.0), 0.0, 0.0, 0.0], rtol=1e-15)
    assert not host.elpd_jacobian(None, X, idx).any()
    r = _result(np.arange(7.0), idx=idx, shift=j, scale="data")
    plain = _result(np.arange(7.0), idx=idx)
    np.testing.assert_array_equal(r["pointwise"]["elpd_loo"], plain["pointwise"]["elpd_loo"] + j)
    np.testing.assert_array_equal(r["pointwise"]["lpd"], plain["pointwise"]["lpd"] + j)
    np.testing.assert_array_equal(r["pointwise"]["p_loo"], plain["pointwise"]["p_loo"])
    assert r["scale"] == "data" and r["elpd_waic"] == pytest.approx(plain["elpd_waic"] + j.sum(), rel=1e-15)
    X[0, 1] = 0.0
    X[1, 1] = 0.0
    with pytest.raises(ValueError, match="component 1 has 2 observation"):
        host.elpd_jacobian(host.obs_model_spec(["log", "sqrt", "identity"], 3), X, idx)


def test_tail_margin_sees_a_near_tie_and_ignores_repeated_draws():
    rng = np.random.default_rng(2)
    ll = -0.5 * rng.standard_normal((100, 2)) ** 2
    bar = np.full(ll.shape, 1e-15)
    wide = er.tail_margin(ll, bar)
    assert np.isfinite(wide) and wide > 1000.0
    o = np.argsort(ll[:, 0])
    rep = ll.copy()
    rep[o[3], 0] = rep[o[4], 0]                              # a repeated draw inside the tail: equal on both sides, not counted
    assert er.tail_margin(rep, bar) >= min(wide, 1000.0)
    near = ll.copy()
    near[o[3], 0] = near[o[4], 0] * (1.0 + 1e-14)
    assert er.tail_margin(near, bar) < 1000.0
    assert er.tail_margin(ll[:24], bar[:24]) == np.inf        # M = 4: no smoothing, no order decision


def test_past_the_device_bound_the_api_falls_back_to_waic_with_a_warning():
    from magi_v2_amd import host
    assert host.ELPD_LOO_MAX_DRAWS == er.LOO_MAX_S
    assert host.elpd_wants_loo(8000) and host.elpd_wants_loo(er.LOO_MAX_S) and not host.elpd_wants_loo(10 ** 6, False)
    assert host.elpd_wants_loo(10 ** 6, True)                 # insisting is the caller's right: the device then refuses
    with pytest.warns(UserWarning, match="lpd and WAIC only"):
        assert not host.elpd_wants_loo(er.LOO_MAX_S + 1)


def test_header_defines_every_output():
    src = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    doc = src[src.index("pointwise log-likelihood, WAIC and PSIS-LOO"):src.index("int magi_sampler_elpd(")]
    for word in er.OUTPUTS + ("n_nonfinite", "obs_index", "n_obs_out", "loglik_out", "466033", "Zhang", "ddof = 1"):
        assert word in doc, word
    from magi_v2_amd import engine, host
    assert host.ELPD_POINTWISE == er.OUTPUTS and "magi_elpd" in engine.exported_symbols() and "magi_sampler_elpd" in engine.exported_symbols()
    from magi_v2_amd import jit
    assert "elpd.hip" in jit._DRIFT_FREE
