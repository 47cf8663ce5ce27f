"""Traced drifts at the documented shape limits (D = 1, 7, 8; P = 8) and at the edges of the printer's and the separator's vocabulary
(magi_v2_amd.drift_examples.EDGE_EXAMPLES): everything a CPU can check, and the CONDITIONS under which tests/test_drift_edges_gpu.py means
something.

Truth is independent of sympy and of float64: the callable itself on ``numpy.longdouble`` arrays, its Jacobians by complex step in
``numpy.clongdouble`` (the pattern of tests/test_drift_cpu.complex_step_jacobians).  selftest.py probes the device code against ``f_np`` /
``jac_np``, the host evaluators of the same sympy trace: a wrong printer rule or a wrong grouping in ``_separate`` can agree with itself there,
not here.

Conditions (asserted; they are not measurements of the kernels): the float64 callable sits within 1/100 of the probe tolerance of the
longdouble truth at every probe point; every base of a non-integer power and every argument of a logarithm is DOMAIN_MARGIN inside its domain at
every point used; every operation the tables are there for moves the truth by >= 1e6 x the probe tolerance when its term is taken out of the
callable; the N = 129 structureless fixtures give the value comparison weight and cost nothing in conditioning; every oracle chain compared
on the GPU builds a deep tree, accepts, never diverges and keeps its integers in longdouble; the theta initialiser's comparison is run long
enough for a dropped K^-T product to show."""
import contextlib
import ctypes
import functools
import re

import numpy as np
import pytest

from magi_v2_amd import drift as drift_mod, jit, selftest
from magi_v2_amd.drift_examples import EDGE_EXAMPLES, EDGE_TRACE_ONLY
from magi_v2_amd.engine import exported_symbols
from oracle import magi_oracle as orc
from tests.test_structureless_cpu import _longdouble, _scaled_gap, logpost_grad_longdouble
from tests.util import DOMAIN_MARGIN, STRUCTURELESS_BOX, structureless_problem, structureless_states, structureless_theta

TOL = selftest.TOL_DRIFT[0]                               # the probe tolerance, in the units of selftest._normalised_error
N_PROBE = 257                                             # one full 256-thread block of the probe kernel and a one-thread tail
N_FIX = 129                                               # two operator block rows, the last of one row; 17 point workgroups of 8 (D > 4), 9 of 16 otherwise: all ragged
STATE_BATCHES = (1, 2, 3, 9)                              # states per log-posterior call: k_stream<1>, <2>, the matrix-core kernels, a second chain group
SAMPLER_CASES = ("chain8", "cascade7", "logistic1", "mixed3")
THETA_INIT_CASES = ("chain8", "logistic1", "cascade7")
# Adam steps of the theta-initialiser comparison.  The objective is unbounded below on these indefinite matrices, so theta keeps moving at
# about lr per step: 60 steps end > 1e8 comparison tolerances from the loop with a one-sided gradient (30 would: 4e7), and the oracle's loop
# agrees with its longdouble re-run to < 1e-6 of the bars.  Not the 200 of tests/test_theta_init_gpu.py: cascade7's th7 reaches -x5, the pole of
# its Michaelis-Menten link, at step 90, where the oracle itself is 2e-8 from its longdouble re-run (2 x the loss trace's bar)
THETA_INIT_ITERS = 60

# drift -> (low, high) of every probed parameter; others (0.3, 1.8).  logistic1: K >= 2.5 keeps df/dx = r (1 - 2 x / K), the ONLY entry of its
# row at D = 1 and so its own scale, away from its zero at x = K / 2
THETA_BOX = {"hill_pow": (0.6, 2.0), "logistic1": (2.5, 4.0)}
# what has a limited domain, per drift: the bases of non-integer powers and the arguments of logarithms, as functions of (X[n, D], theta[P])
# (cascade7: the denominator of its Michaelis-Menten link, a pole rather than an edge -- the theta initialiser moves th7 towards -x5)
DOMAIN = {"hill_pow": lambda X, th: [X[:, 0], X[:, 1], th[2]], "mixed3": lambda X, th: [1.0 + X[:, 0] ** 2], "cascade7": lambda X, th: [th[7] + X[:, 5]]}

# the kernel family every entry must land in: SEP, NBMAX, nbasis(d) per component, TDEP of the emitted header
STRUCTURE = {"logistic1": (True, 2, (2,), False), "chain8": (True, 2, (2,) * 8, False), "cascade7": (False, 1, (0,) * 7, False),
             "hill_pow": (False, 1, (0, 0), False), "mixed3": (True, 4, (4, 3, 0), False), "five_term": (False, 1, (0, 0), False)}


def _col(d, D, v):
    """[n, D] with v in column d (a term of component d, to be taken out of a callable)."""
    return np.concatenate([v if k == d else 0 * v for k in range(D)], axis=1)


# operation -> (drift, the term that carries it as a callable of (X, theta) returning [n, D]): the forms no other compiled library holds
TERMS = {
    "pow(x, theta)": ("hill_pow", lambda X, th: _col(0, 2, th[0] * X[:, 1:2] ** th[1] / (th[2] ** th[1] + X[:, 1:2] ** th[1]))),
    "pow(x, 5)": ("hill_pow", lambda X, th: _col(0, 2, -0.3 * X[:, 0:1] ** 5)),
    "pow(x, 2.5)": ("hill_pow", lambda X, th: _col(0, 2, -th[3] * X[:, 0:1] ** 2.5)),
    "1 / pow(y, 6)": ("hill_pow", lambda X, th: _col(1, 2, -0.02 * X[:, 1:2] ** -6)),
    "pow(x, 1/3)": ("hill_pow", lambda X, th: _col(1, 2, -th[0] * X[:, 0:1] ** (1.0 / 3.0) * X[:, 1:2])),
    "pow(2, x)": ("hill_pow", lambda X, th: _col(1, 2, th[3] * 2 ** X[:, 0:1])),
    "exp(-x)": ("mixed3", lambda X, th: _col(0, 3, th[2] * np.exp(-X[:, 0:1]))),
    "sin": ("mixed3", lambda X, th: _col(0, 3, -th[3] * np.sin(X[:, 1:2]))),
    "tanh": ("mixed3", lambda X, th: _col(0, 3, th[4] * np.tanh(X[:, 0:1] * X[:, 1:2]))),
    "log(1 + x^2)": ("mixed3", lambda X, th: _col(0, 3, -th[5] * np.log(1.0 + X[:, 0:1] ** 2))),
    "constant basis": ("mixed3", lambda X, th: _col(1, 3, th[0] + 0 * X[:, 0:1])),
    "coefficient 1.0": ("mixed3", lambda X, th: _col(1, 3, -X[:, 1:2])),
    "merged pair, first": ("mixed3", lambda X, th: _col(1, 3, 2.0 * th[0] * th[1] * X[:, 0:1])),
    "merged pair, second": ("mixed3", lambda X, th: _col(1, 3, -th[0] * th[1] * X[:, 0:1] * X[:, 1:2])),
    "rational 1/3": ("mixed3", lambda X, th: _col(1, 3, np.square(X[:, 2:3]) / 3)),
    "rational 1/49": ("mixed3", lambda X, th: _col(1, 3, -(X[:, 0:1] / 7) ** 2)),
    "reciprocal": ("mixed3", lambda X, th: _col(1, 3, 0.1 * np.reciprocal(1.0 + X[:, 1:2] ** 2))),
    "constant source (D = 8)": ("chain8", lambda X, th: _col(0, 8, th[0] + 0 * X[:, 0:1])),
    "x / (1 + y^2) link": ("chain8", lambda X, th: _col(6, 8, -th[7] * X[:, 6:7] / (1.0 + X[:, 7:8] ** 2))),
    "x / (K + x) link": ("cascade7", lambda X, th: _col(6, 7, th[6] * X[:, 5:6] / (th[7] + X[:, 5:6]))),
    "x^2 / K (D = 1)": ("logistic1", lambda X, th: _col(0, 1, -th[0] * X[:, 0:1] ** 2 / th[1])),
}


def box(name):
    return STRUCTURELESS_BOX.get(name, (0.1, 0.9))


def example(name):
    return (EDGE_EXAMPLES | EDGE_TRACE_ONLY)[name]


@functools.lru_cache(maxsize=None)
def traced(name):
    f_vec, D, P = example(name)
    return drift_mod.resolve(f_vec, D, P)


@functools.lru_cache(maxsize=None)
def probe(name):
    """(X[257, D], theta[P], g[257, D]) inside the drift's boxes: read-only."""
    _, D, P = example(name)
    rng = np.random.default_rng([sorted(EDGE_EXAMPLES | EDGE_TRACE_ONLY).index(name), 257])
    return rng.uniform(*box(name), (N_PROBE, D)), rng.uniform(*THETA_BOX.get(name, (0.3, 1.8)), P), rng.standard_normal((N_PROBE, D))


def truth_of(f_vec, X, th, g, real=np.longdouble, cplx=np.clongdouble):
    """(f, c, t) of a callable at the points X: c_k = sum_d g_d df_d/dx_k, t_p = sum_d g_d df_d/dtheta_p, the derivatives from
    Im f(x + ih) / h in ``cplx`` -- no sympy, and with the defaults no float64."""
    n, D = X.shape
    P = len(th)
    h = real("1e-30")
    Xr, thr, gr = X.astype(real), th.astype(real), g.astype(real)
    J, T = np.zeros((n, D, D), dtype=real), np.zeros((n, D, P), dtype=real)
    for k in range(D):
        Xc = Xr.astype(cplx); Xc[:, k] += 1j * h
        J[:, :, k] = np.imag(f_vec(None, Xc, thr.astype(cplx))) / h
    for p in range(P):
        tc = thr.astype(cplx); tc[p] += 1j * h
        T[:, :, p] = np.imag(f_vec(None, Xr.astype(cplx), tc)) / h
    return np.asarray(f_vec(None, Xr, thr), dtype=real), np.einsum("nd,ndk->nk", gr, J), np.einsum("nd,ndp->np", gr, T)


@functools.lru_cache(maxsize=None)
def truth(name):
    """The longdouble truth at the drift's probe set, computed once and shared: read-only."""
    return truth_of(example(name)[0], *probe(name))


def probe_errors(got, want):
    """selftest's measure (the error in units where the tolerance is TOL_DRIFT[0]) of each of f, c, t that ``got`` holds."""
    return {k: selftest._normalised_error(np.asarray(a), b) for k, a, b in zip("fct", got, want) if a is not None}


def domain_margin(name, X, th):
    """Smallest distance of a limited-domain argument from 0 over the points X, as a fraction of max|X| (inf: the drift has none)."""
    if name not in DOMAIN:
        return np.inf
    return min(float(np.min(a)) for a in DOMAIN[name](np.asarray(X).reshape(-1, X.shape[-1]), th)) / float(np.abs(X).max())


# ---- the oracle's side of the fixtures ---------------------------------------------------------------------------------------------

def _oracle_entry(f_vec):
    """An entry of the oracle's drift table, fn(X, th) -> (f, J, T): the callable, its Jacobians by complex step (independent of sympy)."""
    def fn(X, th):
        X, th = np.asarray(X, dtype=np.float64), np.asarray(th, dtype=np.float64)
        n, D = X.shape
        J, T = np.zeros((n, D, D)), np.zeros((n, D, len(th)))
        for k in range(D):
            Xc = X.astype(complex); Xc[:, k] += 1e-30j
            J[:, :, k] = np.imag(f_vec(None, Xc, th.astype(complex))) / 1e-30
        for p in range(len(th)):
            tc = th.astype(complex); tc[p] += 1e-30j
            T[:, :, p] = np.imag(f_vec(None, X.astype(complex), tc)) / 1e-30
        return np.asarray(f_vec(None, X, th), dtype=np.float64), J, T
    return fn


@contextlib.contextmanager
def edge_drifts():
    """EDGE_EXAMPLES registered with the oracle (``orc.DRIFTS``, which ``Problem.drift`` names) for the duration only: other tests iterate
    over that table."""
    added = {name: (_oracle_entry(f_vec), D, P) for name, (f_vec, D, P) in EDGE_EXAMPLES.items() if name not in orc.DRIFTS}
    orc.DRIFTS.update(added)
    try:
        yield
    finally:
        for name in added:
            del orc.DRIFTS[name]


@pytest.fixture(autouse=True)
def _registered():
    with edge_drifts():
        yield


SEEDS = {"logistic1": 11, "chain8": 12, "cascade7": 18, "hill_pow": 17, "mixed3": 15}


@functools.lru_cache(maxsize=None)
def fixture(name, spd=False, band=None):
    """(orc.Problem, X[129, D]) of tests/util.structureless_problem for an entry: read-only.  Call it inside ``edge_drifts()``."""
    return structureless_problem(N_FIX, name, 1000 * SEEDS[name] + (500 if spd else 0) + (5 if band is not None else 0), spd=spd, band=band)


def logpost_states(name, band=None):
    """Every state the GPU file's log-posterior comparison evaluates: [(X, sigma_pre, theta_pre)]."""
    pr, X = fixture(name, band=band)
    out = []
    for n in STATE_BATCHES:
        Xb, sp, tp = structureless_states(pr, X, n, 0)
        out += [(Xb[c], sp[c], tp[c]) for c in range(n)]
    return out


def nuts_inits(pr, X):
    from tests.test_structureless_gpu import _inits
    return _inits(pr, X)


@functools.lru_cache(maxsize=None)
def oracle_nuts(name, chain, long=False):
    """(sample_chain's output, trace) of one oracle chain on the entry's spd fixture with the NUTS parameters of
    tests/test_structureless_gpu.py; ``long``: the operator products in longdouble.  Shared and read-only; call it inside ``edge_drifts()``."""
    from tests.test_nonfinite_cpu import _longdouble_logpost_grad
    from tests.test_structureless_gpu import NUTS
    pr, X = fixture(name, spd=True)
    sig0, th0 = nuts_inits(pr, X)
    trace = []
    out = orc.sample_chain(pr, X, sig0, th0, NUTS["results"], NUTS["burnin"], seed=NUTS["seed"], chain=chain, step_size=NUTS["step"],
                           stale_cache=False, trace=trace, max_tree_depth=NUTS["depth"], logpost_grad=_longdouble_logpost_grad if long else None)
    return out, trace


def sampler_chains(name):
    """The chain ids the GPU file compares: first and last of 1 and 3 chains from id 20 (chain8: of 9 as well)."""
    return (20, 22, 28) if name == "chain8" else (20, 22)


def theta_init_inputs(name):
    """What the theta initialiser is given on the NON-symmetric fixture: (Xhat, mu, m, K^-1)."""
    pr, X = fixture(name)
    return X, pr.mu, pr.m, pr.K_inv


# ---- the trace against the truth -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES | EDGE_TRACE_ONLY))
def test_host_evaluators_of_the_trace_equal_the_longdouble_truth(name):
    d = traced(name)
    f_vec, D, P = example(name)
    assert not d.is_builtin and (d.D, d.P) == (D, P) and not d.time_dependent
    X, th, g = probe(name)
    J, T = d.jac_np(X, th)
    got = (d.f_np(None, X, th), np.einsum("nd,ndk->nk", g, J), np.einsum("nd,ndp->np", g, T))
    errs = probe_errors(got, truth(name))
    print(name, "f_np / jac_np against the longdouble truth, fraction of TOL_DRIFT:", {k: f"{v / TOL:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES | EDGE_TRACE_ONLY))
def test_no_probe_point_is_ill_conditioned(name):
    """CONDITION: the callable in float64, with its float64 complex step, is within 1/100 of the probe tolerance of the longdouble truth."""
    errs = probe_errors(truth_of(example(name)[0], *probe(name), real=np.float64, cplx=np.complex128), truth(name))
    print(name, "float64 callable against the longdouble truth, fraction of TOL_DRIFT / 100:", {k: f"{v / (TOL / 100):.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL / 100, errs


@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES))
def test_every_limited_domain_argument_is_inside_its_domain_at_every_point_used(name):
    """CONDITION: DOMAIN_MARGIN at the probe points, at every log-posterior state (with its softplus parameters) and at the theta
    initialiser's input."""
    X, th, _ = probe(name)
    worst = domain_margin(name, X, th)
    for Xs, _, tp in logpost_states(name) + (logpost_states(name, band=20) if name == "chain8" else []):
        worst = min(worst, domain_margin(name, Xs, np.log1p(np.exp(tp))))
    print(name, f"smallest limited-domain argument / max|X|: {worst:.2e}")
    assert worst >= DOMAIN_MARGIN


@pytest.mark.parametrize("op", sorted(TERMS))
def test_every_operation_carries_weight_at_the_probe_points(op):
    """CONDITION: the callable without the operation's term (exactly one term of the trace less) moves the truth by >= 1e6 x the probe
    tolerance -- in f and in a derivative -- at some probe point: a term that a neighbour drowns does not count as tested."""
    name, term = TERMS[op]
    f_vec, D, P = example(name)
    without = lambda t, X, th: f_vec(t, X, th) - term(X, th)
    sp, _, _, _, full = drift_mod._trace(f_vec, D, P)
    cut = drift_mod._trace(without, D, P)[4]
    count = lambda es: sum(len(sp.Add.make_args(sp.expand(e))) if sp.expand(e) != 0 else 0 for e in es)
    assert count(cut) == count(full) - 1, (op, count(cut), count(full))
    moved = probe_errors(truth_of(without, *probe(name)), truth(name))
    print(op, "truth moves by (x TOL_DRIFT):", {k: f"{v / TOL:.1e}" for k, v in moved.items()})
    assert moved["f"] >= 1e6 * TOL and max(moved["c"], moved["t"]) >= 1e6 * TOL, (op, moved)


# ---- structure -----------------------------------------------------------------------------------------------------------------------

def header_structure(header):
    """(SEP, NBMAX, nbasis per component, TDEP) read off the text of a generated header."""
    D = int(re.search(r"#define MAGI_USER_D (\d+)", header).group(1))
    flag = lambda what: re.search(rf"static constexpr bool {what} = (true|false);", header).group(1) == "true"
    nbmax = int(re.search(r"static constexpr int NBMAX = (\d+);", header).group(1))
    body = re.search(r"static constexpr int nbasis\(int(?: d)?\) \{ return (.*?); \}", header).group(1)

    def nbasis(d):
        for piece in body.split(" : "):
            m = re.fullmatch(r"d == (\d+) \? (\d+)", piece)
            if m is None:
                return int(piece)
            if int(m.group(1)) == d:
                return int(m.group(2))
    return flag("SEP"), nbmax, tuple(nbasis(d) for d in range(D)), flag("TDEP")


@pytest.mark.parametrize("name", sorted(STRUCTURE))
def test_every_entry_lands_in_the_kernel_family_it_is_there_for(name):
    d = traced(name)
    assert header_structure(d.header) == STRUCTURE[name]
    f_vec, D, P = example(name)
    sp, xs, ths, _, exprs = drift_mod._trace(f_vec, D, P)
    pairs = drift_mod._separate(sp, xs, ths, exprs)
    sep, _, nb, _ = STRUCTURE[name]
    assert (pairs is not None) == sep and selftest._separable(d) == sep
    if sep:
        assert tuple(len(p) for p in pairs) == nb


def test_the_emitted_code_holds_the_forms_the_tables_are_there_for():
    """The vocabulary itself, in the text that is compiled (a printer that changes its spelling moves the gap: say so here)."""
    h = traced("hill_pow").header
    for tok in ("pow(x[1], th[1])", "pow(th[2], th[1])", "log(x[1])", "log(th[2])", "pow(x[0], 5.0)", "pow(x[0], 2.5)", "/pow(x[1], 6.0)",
                "pow(x[0], 0.33333333333333331)", "pow(2.0, x[0])", "M_LN2", "0.31415926535897931"):
        assert tok in h, tok
    m = traced("mixed3").header
    for tok in ("tanh(", "sin(", "cos(", "exp(-x[0])", "(1.0/49.0)", "(1.0/3.0)", "ph[1][0] = 1.0;", "c[1][1] = 1.0;", "c[1][2] = th[0]*th[1];",
                "ph[1][2] = -x[0]*(x[1] - 2.0);", "o[2] = 0.0;", "ph[2][0] = 0.0;", "((x[0])*(x[0]))", "2.0*q_2*x[0]", "((2.0/3.0))*g[1]*x[2]"):
        assert tok in m, tok
    assert "(1.0/((q_4)))" in traced("cascade7").header                                        # (a small negative power: a reciprocal of products)
    assert "ph[0][0] = 1.0;" in traced("chain8").header and "return 2;" in traced("logistic1").header and "return o[0];" in traced("logistic1").header


# ---- build ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES))
def test_library_builds_for_gfx950_and_exports_the_full_abi(name):
    d = traced(name)
    lib = ctypes.CDLL(jit.library_for(d))
    for sym in exported_symbols():
        assert hasattr(lib, sym), sym
    D, P = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.magi_user_drift_info(ctypes.byref(D), ctypes.byref(P)) == 1 and (D.value, P.value) == (d.D, d.P)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EDGE_EXAMPLES))
def test_fixture_states_weigh_the_matrices_and_sit_at_the_longdouble_floor(name):
    """CONDITIONS at every state of the GPU file's log-posterior comparison (temperature 0.8 as there): (t1 + t2) / beta >= 0.1 |t3 + t4|, and
    the fp64 oracle within 1/100 of the 1e-10 bar of its longdouble evaluation."""
    worst, ratio = 0.0, np.inf
    for band in ((None, 20) if name == "chain8" else (None,)):
        pr, _ = fixture(name, band=band)
        assert pr.N == N_FIX and (pr.D, pr.P) == example(name)[1:]
        pr_ld = _longdouble(pr)
        for X, sp, tp in logpost_states(name, band):
            t1, t2, t3, t4, _, _ = orc.logpost_terms(X, sp, tp, pr)
            ratio = min(ratio, (t1 + t2) / pr.beta / abs(t3 + t4))
            temp = 1.0 if band is not None else 0.8
            got, want = orc.logpost_grad(X, sp, tp, temp, pr), logpost_grad_longdouble(X, sp, tp, temp, pr_ld)
            worst = max(worst, abs(float(got[0] - want[0]) / float(want[0])), *[_scaled_gap(a, b) for a, b in zip(got[1:], want[1:])])
    print(name, f"smallest (t1 + t2) / beta / |t3 + t4|: {ratio:.3g}; fp64 oracle against longdouble: {worst:.2e}")
    assert ratio >= 0.1 and worst <= 1e-12, (name, ratio, worst)


# ---- sampler -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_every_oracle_chain_builds_deep_trees_accepts_and_keeps_its_integers_in_longdouble(name):
    """CONDITIONS on the chains the GPU file compares draw for draw: a tree of >= 31 leapfrogs, >= 6 of 7 transitions accepted, no
    divergence, and the same integers with the operator products in longdouble (no decision on a rounding knife-edge)."""
    ints = lambda trace: [(r.depth, r.leapfrogs, int(r.is_accepted), int(r.has_divergence)) for _, r, _ in trace]
    for chain in sampler_chains(name):
        (oX, _, otp, _, _), trace = oracle_nuts(name, chain)
        (lX, _, ltp, _, _), ltrace = oracle_nuts(name, chain, True)
        print(name, chain, "leapfrogs", [r.leapfrogs for _, r, _ in trace], "accepted", sum(int(r.is_accepted) for _, r, _ in trace),
              f"longdouble re-run: X {np.abs(oX - lX).max() / np.abs(oX).max():.1e} of scale, theta_pre {np.abs(otp - ltp).max():.1e}")
        assert len(trace) == 7 and max(r.leapfrogs for _, r, _ in trace) >= 31
        assert sum(int(r.is_accepted) for _, r, _ in trace) >= 6 and not any(r.has_divergence for _, r, _ in trace)
        assert ints(trace) == ints(ltrace)
        assert min(domain_margin(name, oX[k], np.log1p(np.exp(otp[k]))) for k in range(len(oX))) >= DOMAIN_MARGIN          # (the kept states, each with its parameters)
        # (1/100 of the device bars of _assert_chain_equals_oracle: X to 1e-8 of scale, theta_pre at rtol 1e-7 / atol 1e-9)
        assert np.abs(oX - lX).max() <= 1e-10 * np.abs(oX).max() and (np.abs(otp - ltp) <= 1e-11 + 1e-9 * np.abs(otp)).all()


# ---- theta initialiser ---------------------------------------------------------------------------------------------------------------

def _adam_with_one_sided_gradient(name, iters):
    """orc.fit_thetas_init with the gradient T^T 2 K r in place of T^T (K + K^T) r: what a loop that drops (or doubles) the K^-T product
    computes.  On a symmetric K^-1 the two are the same loop."""
    Xhat, mu, m, K_inv = theta_init_inputs(name)
    N, D = Xhat.shape

    def fn(th):
        val, _ = orc.theta_init_objective(th, Xhat, mu, m, K_inv, name)
        f, _, T = orc.DRIFTS[name][0](Xhat, th)
        r = np.reshape(f, (D, N, 1)) - m @ np.transpose((Xhat - mu).reshape(N, 1, D), (2, 0, 1))
        g = 2.0 * (K_inv @ r)[:, :, 0]
        return val, np.array([np.sum(np.reshape(T[:, :, p], (D, N)) * g) for p in range(T.shape[2])])
    return orc.adam_minimise(fn, np.ones(example(name)[2]), iters, 0.01)[0]


@functools.lru_cache(maxsize=None)
def oracle_theta_init(name):
    """orc.fit_thetas_init on the non-symmetric fixture, THETA_INIT_ITERS steps: shared, read-only; call it inside ``edge_drifts()``."""
    Xhat, mu, m, K_inv = theta_init_inputs(name)
    return orc.fit_thetas_init(Xhat, mu, m, K_inv, name, example(name)[2], num_iters=THETA_INIT_ITERS)


@pytest.mark.parametrize("name", THETA_INIT_CASES)
def test_a_dropped_transpose_moves_the_theta_initialiser_by_1000_tolerances(name):
    """CONDITION of the GPU comparison (theta at rtol 1e-8, atol 1e-10): on the non-symmetric fixture the one-sided loop ends >= 1000
    tolerances from the oracle's theta.  (Adam's first steps move theta by lr whatever the gradient's size: a short run proves nothing
    unless this is measured.)"""
    _, _, _, K_inv = theta_init_inputs(name)
    assert np.abs(K_inv - np.transpose(K_inv, (0, 2, 1))).max() >= 0.1 * np.abs(K_inv).max()
    want, losses = oracle_theta_init(name)
    wrong = _adam_with_one_sided_gradient(name, THETA_INIT_ITERS)
    gap = float((np.abs(wrong - want) / (1e-10 + 1e-8 * np.abs(want))).max())
    print(name, f"one-sided gradient after {THETA_INIT_ITERS} steps: {gap:.3g} tolerances from the oracle's theta; theta", want)
    assert np.isfinite(want).all() and np.isfinite(losses).all() and gap >= 1000.0


@pytest.mark.parametrize("name", THETA_INIT_CASES)
def test_the_theta_initialisers_path_is_well_conditioned(name):
    """CONDITION: the oracle's loop with its matrix products in longdouble ends within 1/100 of the bars (theta at rtol 1e-8, atol 1e-10; loss
    trace at rtol 1e-8) of the float64 loop, and no parameter vector on the way is within DOMAIN_MARGIN of a pole or a domain's edge."""
    Xhat, mu, m, K_inv = theta_init_inputs(name)
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    path = []

    def fn(th):
        path.append(np.array(th, dtype=np.float64))
        val, grad = orc.theta_init_objective(th, ld(Xhat), ld(mu), ld(m), ld(K_inv), name)
        return val, np.asarray(grad, dtype=np.float64)
    th_ld, loss_ld = orc.adam_minimise(fn, np.ones(example(name)[2]), THETA_INIT_ITERS, 0.01)
    want, losses = oracle_theta_init(name)
    gaps = float((np.abs(want - th_ld) / (1e-10 + 1e-8 * np.abs(th_ld))).max()), float(np.abs(losses / loss_ld - 1.0).max() / 1e-8)
    margin = min(domain_margin(name, Xhat, th) for th in path)
    print(name, f"float64 against longdouble loop, fraction of the bars: theta {gaps[0]:.1e}, loss trace {gaps[1]:.1e}; margin along the path {margin:.2e}")
    assert max(gaps) <= 1e-2 and margin >= DOMAIN_MARGIN
